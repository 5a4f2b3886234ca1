"""
CPU guard of the schedule matrix: the host mirror of the schedule executor (tests/schedule_dispatch.py) is held to the C++
it restates (api.hip, generic.hip, common.h, read as text), its restatement of the joining of H steps to a brute-force
property, and the cases of tests/test_hip_schedule_matrix.py to reaching every route of tnmf_hip_run_schedule, every edge
of k_schedule's block loops, every fusion, every form of the accumulator blend, the ring of pinned slots and every
refusal.  No GPU, no build.
"""
import ctypes
import os
import re

import numpy as np

import direct_dispatch as dd
import schedule_dispatch as sd
import schedule_reference as sr
from conftest import ROOT
from tnmf_amd import _lib

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _flat(text):
    return re.sub(r'\s+', ' ', text.replace('\\\n', ' '))


# ----------------------------------------------------------------------------------------------------------------------
# the mirror against the sources
# ----------------------------------------------------------------------------------------------------------------------
def test_mirrored_constants_and_rules_are_those_of_the_source():
    """The lines the mirror restates.  When one of them changes, tests/schedule_dispatch.py and the matrix's cases have to
    be looked at again."""
    api, gen, hdr = (_flat(_read(n)) for n in ('api.hip', 'generic.hip', 'common.h'))
    # ---- validation: the 2-D entry and the volume entry, the same lines in the same order; the list's check stated once
    assert api.count('if (n_ops < 0 || (n_ops > 0 && !ops)) return TNMF_E_NULL; '
                     'if (!V || !W_inout || !H_inout || !acc) return TNMF_E_NULL;') == 2
    check = api[api.index('int check_ops(const tnmf_hip_op *ops, int n_ops, int N) {'):api.index('inline bool is_vol(')]
    for line in (
            'if (ops[i].kind != TNMF_OP_UPDATE_H && ops[i].kind != TNMF_OP_GRAD_W && ops[i].kind != TNMF_OP_APPLY_W) '
            'return TNMF_E_UNSUPPORTED; if (ops[i].kind == TNMF_OP_APPLY_W) continue;',
            'if (ops[i].n0 < 0 || ops[i].n1 < ops[i].n0 || ops[i].n1 > N) return TNMF_E_GEOM;'):
        assert line in check and api.count(line) == 1, line
    assert check.index('return TNMF_E_UNSUPPORTED;') < check.index('return TNMF_E_GEOM;')
    vol = api[api.index('int vol_api_run_schedule('):api.index('int vol_api_pad_fold(')]
    assert vol.index('!acc) return TNMF_E_NULL;') < vol.index('CHECK(check_ops(ops, n_ops, v.N));') < vol.index('vol_scratch(') \
        < vol.index('switch (op.kind)')
    two = api[api.index('int tnmf_hip_run_schedule('):api.index('int tnmf_hip_axpby(')]
    assert two.index('!acc) return TNMF_E_NULL;') < two.index('CHECK(check_ops(ops, n_ops, g.N));') \
        < two.index('std::vector<tnmf_hip_op> joined;')
    for line in (
            # ---- joining
            'run.erase(std::remove_if(run.begin(), run.end(), [](const tnmf_hip_op &o) { return o.n1 <= o.n0; }), run.end());',
            'std::sort(sorted_run.begin(), sorted_run.end(), [](const tnmf_hip_op &a, const tnmf_hip_op &b) { return a.n0 < b.n0; });',
            'for (size_t k = 1; k < sorted_run.size(); ++k) disjoint = disjoint && sorted_run[k].n0 >= sorted_run[k - 1].n1;',
            'if (!disjoint) { joined.insert(joined.end(), run.begin(), run.end()); }',
            'if (!joined.empty() && joined.back().kind == TNMF_OP_UPDATE_H && k > 0 && joined.back().n1 == sorted_run[k].n0) '
            'joined.back().n1 = sorted_run[k].n1; else joined.push_back(sorted_run[k]);',
            # ---- the route
            f'const bool tiny = (size_t)g.N * g.M * g.Hy * g.Hx <= ((size_t)1 << {sd.TINY.bit_length() - 1});',
            'if (n_ops > 0 && tiny && ctx->persistent != 0 && (ctx->path == TNMF_PATH_AUTO || ctx->path == TNMF_PATH_GENERIC) && '
            'generic_schedule_fits(ctx, g, dtype)) {',
            'const int P = generic_schedule_chunks(ctx, g); const size_t r_bytes = R_scratch ? 0 : align_up((size_t)g.N * vs, 256);',
            'void *Rs = R_scratch ? R_scratch : static_cast<void *>(ws_at(ctx, 0));',
            'if (rc != TNMF_E_UNSUPPORTED) { ctx->last_schedule_persistent = rc == TNMF_OK; return rc; }',
            # ---- the ring
            'const int slot = ctx->ops_next; ctx->ops_next = (slot + 1) % tnmf_hip_ctx::kOpSlots;',
            'const size_t need = (size_t)n_ops * sizeof(tnmf_hip_op);',
            'if (ctx->ops_done[slot]) TNMF_HIP_TRY(hipEventSynchronize(ctx->ops_done[slot]));',
            f'if (hipHostMalloc(&ctx->ops_pinned[slot], align_up(need, {sd.SLOT_GROWTH}), hipHostMallocDefault) != hipSuccess) {{',
            f'ctx->ops_cap[slot] = align_up(need, {sd.SLOT_GROWTH});',
            # ---- the per-operation path
            'Geo gmax = g; gmax.N = nmax; const Scratch scm = plan_scratch(ctx, gmax, dtype);',
            'void *Rb = R_scratch ? static_cast<void *>(static_cast<char *>(R_scratch) + (size_t)op.n0 * vs) : '
            'static_cast<void *>(ws_at(ctx, scm.r_off));',
            'Scratch sc = plan_scratch(ctx, gs, dtype); sc.part_off = scm.part_off;',
            'if (gs.N > 0 && !corr_H_on_fft(ctx, gs, dtype)) {',
            'const bool apply_now = i + 1 < n_ops && ops[i + 1].kind == TNMF_OP_APPLY_W;',
            'CHECK(launch_finalize_blend_apply(g, dtype, partials, P, acc, op.a, op.b, apply_now, W_inout, eps, s)); if (apply_now) ++i;',
            'CHECK(do_corr_H(ctx, gs, dtype, sc, Vb, Rb, Hb, grad, grad + wn * es, s)); '
            'CHECK(launch_axpby(ctx, dtype, acc, grad, op.a, op.b, 2 * wn, s));',
            'int P = generic_corr_H_chunks(ctx, g); const int Pm = mfma_corr_H_chunks(ctx, g); if (Pm > P) P = Pm;',
            'return ctx->path == TNMF_PATH_FFT || use_fft_hybrid(ctx, g, dtype);',
            # ---- volumes: per operation, nothing joined, the chunk count clamped
            'int P = vol_corr_H_chunks(ctx, vs_); if (P > Pmax) P = Pmax;'):
        assert line in api, line
    assert 'std::vector<tnmf_hip_op> joined' not in vol and 'generic_run_schedule' not in vol
    assert f'static constexpr int kOpSlots = {sd.K_OP_SLOTS};' in hdr
    assert ctypes.sizeof(_lib.Op) == sd.OP_BYTES
    assert sd.KINDS['H'] == _lib.OP_UPDATE_H and sd.KINDS['G'] == _lib.OP_GRAD_W and sd.KINDS['W'] == _lib.OP_APPLY_W
    for line in (
            # ---- generic_schedule_fits, the small form, the chunks, the grid
            'if (g.Ay * g.Ax > kBlock * kMaxShiftsPerThread) return false;',
            f'return schedule_lds_any(g, dtype, tR, tW, tH, &small_max) <= {sd.LDS_MAX // 1024} * 1024;',
            f'if (lds > {sd.LDS_MAX // 1024} * 1024 || ctx->persistent == 0) return TNMF_E_UNSUPPORTED;',
            'const size_t r = ((size_t)(tR.TY + g.Ay - 1) * (tR.TX + g.Ax - 1) + nA) * sizeof(T);',
            'const size_t w = (2 * (size_t)(tW.TY + g.Ay - 1) * (tW.TX + g.Ax - 1) + nA) * sizeof(T);',
            'size_t h = ((size_t)(tH.TY + g.Ay - 1) * (tH.TX + g.Ax - 1) + 2 * (size_t)tH.TY * tH.TX) * sizeof(T);',
            'const size_t red = (size_t)(kBlock / gs) * nA * 2 * sizeof(double);',
            'Geo one = g; one.N = 1; if (!reconstruct_is_small<T>(one, tR, lds_small)) return 0;',
            'const int per = g.C * tR.tiles_y * tR.tiles_x;',
            'return per > 0 ? (63 / per) : 0;',
            'if (*small_max > 0 && ls > lds) lds = ls;',
            f'const int grid = ctx->num_cu < {sd.GRID_CAP} ? ctx->num_cu : {sd.GRID_CAP}; int P = cdiv(grid, g.M * g.C); '
            f'return P < 1 ? 1 : (P > {sd.P_CAP} ? {sd.P_CAP} : P);',
            f'const int want = ctx->num_cu < {sd.GRID_CAP} ? ctx->num_cu : {sd.GRID_CAP}; return (int)(resident < want ? resident : want);',
            'a.tR = make_tile(g.Dy, g.Dx); a.tW = make_tile(g.Hy, g.Hx); a.tH = make_tile(g.Dy, g.Dx);',
            # ---- k_schedule: offsets, forms, block counts, the chunk clamp, the flip, the fusion
            'const size_t vs = (size_t)g.C * g.Dy * g.Dx, hs = (size_t)g.M * g.Hy * g.Hs;',
            'const T *Vb = static_cast<const T *>(a.V) + (size_t)op.n0 * vs; T *Hb = static_cast<T *>(a.H) + (size_t)op.n0 * hs; '
            'T *Rb = static_cast<T *>(a.R) + (size_t)op.n0 * vs;',
            'if (gs.N <= a.small_max) {',
            'const unsigned nb = (unsigned)(gs.N * g.C * sty * stx);',
            'const unsigned nb = (unsigned)(gs.N * g.C * a.tR.tiles_y * a.tR.tiles_x);',
            'const unsigned nb = (unsigned)(gs.N * g.M * a.tW.tiles_y * a.tW.tiles_x);',
            'const int items = gs.N * a.tH.tiles_y * a.tH.tiles_x; const int P = items < a.P ? (items > 0 ? items : 1) : a.P;',
            'for (unsigned b = wg; b < (unsigned)(P * MC); b += nwg) '
            'corr_H_block<T>(gs, a.tH, P, (int)(b % P), (int)(b / P), Vb, Rb, Hb, a.partials, smem_raw);',
            'const bool apply_now = i + 1 < a.n_ops && a.ops[i + 1].kind == TNMF_OP_APPLY_W;',
            'for (unsigned r = wg; r < (unsigned)MC; r += nwg) {',
            'if (apply_now) apply_normalize_row<T, true>(nA, r, W, acc, acc + (size_t)MC * nA, (T)a.eps);',
            'if (apply_now) ++i;',
            'const T p = pos[base + i] + eps; pos[base + i] = p;'):
        assert line in gen, line
    # the flip and the blend: the same two lines in k_finalize_blend_apply and in k_schedule
    for line in ('const size_t o = (size_t)r * nA + (nA - 1 - sh);',
                 'acc[o] = ca == T(0) ? tn : (ca == T(1) ? acc[o] + tn : ca * acc[o] + tn);',
                 'acc[total + o] = ca == T(0) ? tp : (ca == T(1) ? acc[total + o] + tp : ca * acc[total + o] + tp);'):
        assert gen.count(line) == 2, line
    assert 'acc[i] = a == T(0) ? t : (a == T(1) ? acc[i] + t : a * acc[i] + t);' in gen      # k_axpby: the FFT arm, volumes
    assert (dd.kSmallTY, dd.kSmallTX, dd.kSmallQ, dd.kBlock, dd.kMaxShiftsPerThread) == (2, 32, 4, 256, 4)
    assert 'return blocks < 64 && g.M >= kSmallQ && g.Dy > 1 && *lds_small <= 64 * 1024;' in gen


def test_validation_order():
    N = 5
    assert sd.validate((), N, pointers=False) == 'E_NULL'
    assert sd.validate((('H', 0, 9), ('?', 0, 1)), N) == 'E_GEOM'              # per operation, in list order
    assert sd.validate((('?', 0, 99),), N) == 'E_UNSUPPORTED'                   # the kind before the range
    assert sd.validate((('W', 7, -3), ('H', 0, 5), ('G', 5, 5, 0., 1.)), N) is None
    for name, (ops, err) in sd.REFUSED_LISTS.items():
        for G in sd.REFUSAL_GEOMETRIES.values():
            assert sd.validate(ops, G[0]) == err, name


# ----------------------------------------------------------------------------------------------------------------------
# the joining: executing the joined list equals executing the original
# ----------------------------------------------------------------------------------------------------------------------
def _toy(ops, N):
    """A list on a toy integer state: an H step that is neither idempotent nor commutes with itself on a shared sample
    (it reads W), a W gradient that reads H and W, a W update that reads the accumulator."""
    p = 1000003
    h, w, acc = list(range(1, N + 1)), 7, 11
    for op in ops:
        if op[0] == 'H':
            for n in range(op[1], op[2]):
                h[n] = (h[n] * h[n] * 3 + w + n) % p
        elif op[0] == 'G':
            g = sum((k + 1) * h[n] for k, n in enumerate(range(op[1], op[2]))) * w
            acc = (int(op[3] * 10) * acc + int(op[4] * 10) * g) % p
        else:
            w = (w * 5 + acc) % p
    return h, w, acc


def test_joined_lists_compute_what_the_original_computes():
    rng = np.random.default_rng(2024)
    classes = set()
    for _ in range(4000):
        N = int(rng.integers(1, 9))
        ops = []
        for _ in range(int(rng.integers(1, 13))):
            k = 'HHHGW'[int(rng.integers(5))]
            n0 = int(rng.integers(0, N + 1))
            n1 = int(rng.integers(n0, N + 1))
            ops.append(('W',) if k == 'W' else (k, n0, n1) + ((float(rng.integers(0, 3)), 1.) if k == 'G' else ()))
        joined = sd.join(ops)
        assert _toy(joined, N) == _toy(ops, N), ops
        assert len(joined) <= len(ops) and all(op[2] > op[1] for op in joined if op[0] == 'H')
        assert [op for op in joined if op[0] != 'H'] == [op for op in ops if op[0] != 'H']
        for run in sd.runs_of(ops):
            classes |= sd.run_class(run)
    assert classes == {'run_empties', 'run_duplicate', 'run_nested', 'run_overlapping', 'run_disjoint_shuffled', 'run_touching',
                       'run_gap'}
    # known answers: touching ranges merge, a gap keeps them apart, any overlap keeps the run as it is, minus its empties
    assert sd.join([('H', 6, 10), ('H', 0, 2), ('H', 3, 3), ('H', 2, 4)]) == [('H', 0, 4), ('H', 6, 10)]
    assert sd.join([('H', 0, 5), ('H', 9, 9), ('H', 3, 8)]) == [('H', 0, 5), ('H', 3, 8)]
    assert sd.join([('H', 1, 3), ('H', 1, 3)]) == [('H', 1, 3), ('H', 1, 3)]
    assert sd.join([('H', 2, 4), ('H', 0, 6)]) == [('H', 2, 4), ('H', 0, 6)]         # (nested: the original order, not the sorted)
    # a run never merges with the H step in front of a W gradient: nothing is reordered across it
    assert sd.join([('H', 0, 2), ('G', 0, 2, 0., 1.), ('H', 2, 4)]) == [('H', 0, 2), ('G', 0, 2, 0., 1.), ('H', 2, 4)]


# ----------------------------------------------------------------------------------------------------------------------
# routes of known cases
# ----------------------------------------------------------------------------------------------------------------------
def _cell(cid, T=None, mode=None, cu=dd.NUM_CU):
    c = sd.MATRIX[cid]
    return sd.cell(c.geometry, T or c.dtypes[0], c.path, c.modes[0] if mode is None else mode, list(c.ops), c.padded, c.r_scratch,
                   cu)


def test_routes_and_plans_of_known_cases():
    c = _cell('c1_asag')
    assert (c.route, c.last_path, c.info['small_max'], c.info['P'], c.info['grid']) == ('persistent', 'generic', 0, 6, 128)
    assert _cell('c1_asag', mode=0).route == 'per_op'
    c = _cell('t2_asag')
    assert c.info['small_max'] == 7 and {'recon_small_and_plain_in_one_list', 'phase_lt_grid', 'phase_gt_grid_ragged'} <= c.edges
    assert _cell('wide').info['P'] == 1 and 'rows_gt_grid' in _cell('wide').edges
    assert {'MC_1', 'P_at_cap_64', 'P_lt_items', 'P_clamped_to_items', 'small_max_0'} <= _cell('one').edges
    assert {'MC_1', 'P_clamped_to_items'} <= _cell('tile').edges and _cell('tile').info['phases'] == [1, 1, 1, 2]
    assert {'MC_2', 'P_at_cap_64'} <= _cell('two').edges
    assert 'small_max_0' in _cell('m3').edges and 'small_max_0' in _cell('c1_asag').edges
    # the boundary of `tiny`: on Hx
    g18, g18p = dd.geo(sd.AT18), dd.geo(sd.OVER18)
    assert g18.N * g18.M * g18.Hy * g18.Hx == 1 << 18 and g18p.N * g18p.M * g18p.Hy * g18p.Hx == (1 << 18) + g18p.N * g18p.M * g18p.Hy
    assert (_cell('at18').route, _cell('over18').route) == ('persistent', 'per_op')
    # paths other than auto / generic never take the persistent kernel
    for cid in ('t2_mfma', 't2_split', 't2_hybrid', 't2_fft'):
        assert _cell(cid).route == 'per_op' and sd.is_tiny(dd.geo(sd.MATRIX[cid].geometry))
    # generic_schedule_fits false on tiny problems the per-operation path runs (lists of H steps)
    for cid, why in (('shifts', 'shifts'), ('tall', 'lds')):
        g = dd.geo(sd.MATRIX[cid].geometry)
        assert sd.is_tiny(g) and sd.fits_why(g, 'd') == why and _cell(cid).route == 'per_op'
        assert dd.generic_reconstruct(g, 'd') is not None and dd.generic_corr_W(g, 'd', True) is not None
        assert dd.generic_corr_H(g, 'd') is None           # (which is why these lists hold H steps only)
    assert sd.schedule_lds(dd.geo(sd.TALL), 'd') == 67584 and sd.fits_why(dd.geo(sd.TALL), 'f') is None
    # the FFT arm under auto: the whole batch of BIG, not its small slices; five samples and more on the split kernel
    c = _cell('big_whole')
    assert {'fft_arm_auto', 'fft_arm_auto_next_to_direct', 'fft_arm_then_separate_W', 'finalize_apply_now_mfma'} <= c.edges
    assert 'join_changes_family' in _cell('big_join').edges
    assert {'fft_arm_path_fft_f'} <= _cell('big_fft', 'f').edges and {'fft_arm_path_fft_d'} <= _cell('big_fft', 'd').edges
    assert _cell('vol_asag').route == 'volume'
    # no case asks a kernel family for a shape it refuses: a list never stops half way
    for cid, c in sd.MATRIX.items():
        for T in c.dtypes:
            for mode in c.modes:
                assert 'kernel_family_refuses' not in _cell(cid, T, mode).edges, (cid, T, mode)
    # the cells do not depend on the compute units between 128 and 304
    for cu in (128, 304):
        for cid in sd.MATRIX:
            assert _cell(cid, cu=cu).route == _cell(cid).route


def test_ring_of_pinned_slots():
    plan = sd.ring(sd.RING_LENGTHS)
    assert [p[0] for p in plan] == [0, 1, 2, 3, 0, 1]
    assert [p[1] for p in plan] == [False, False, False, False, True, True]          # calls five and six wait for one and two
    assert [p[2] for p in plan] == [4096, 8192, 4096, 8192, 0, 0]                    # 200 and 130 operations: past 4096 bytes
    assert sd.SLOT_GROWTH // sd.OP_BYTES == 128 and min(n for n in sd.RING_LENGTHS if n > 128) == 129


def test_partials_of_every_slice_fit_the_region_of_the_largest():
    """The per-operation path puts the split-K partials of every slice where plan_scratch(gmax) put the largest slice's:
    the chunk count of every slice of every case is at most the region's (the volume path clamps; this path assumes)."""
    rows = sd.scratch_fits(sd.MATRIX) + sd.scratch_fits(sd.MATRIX, 304)
    assert len(rows) > 100
    for cid, T, n, P, region in rows:
        assert 1 <= P <= region, (cid, T, n, P, region)
    # and beyond the matrix: every slice length of its geometries, alone and next to the whole batch
    for G in {c.geometry for c in sd.MATRIX.values() if len(c.geometry[4]) < 3}:
        for T in 'fd':
            for path in ('auto', 'generic', 'mfma'):
                if path == 'mfma' and T == 'd':
                    continue
                region = [sd.partials_region(G, n, T) for n in range(1, G[0] + 1)]
                assert region == sorted(region), (G, T, path)
                for n in range(1, G[0] + 1):
                    assert sd.slice_chunks(G, n, T, path, False) <= region[n - 1], (G, T, path, n)


# ----------------------------------------------------------------------------------------------------------------------
# the matrix
# ----------------------------------------------------------------------------------------------------------------------
def test_matrix_reaches_every_cell():
    got = sd.reached(sd.MATRIX)
    assert not sd.missing(sd.MATRIX), sd.missing(sd.MATRIX)
    for key in sorted(sd.required()):
        assert got[key], key
    assert not sd.UNREACHABLE
    assert set(sd.NOT_COVERED) == {('last_path', 'split / hybrid'), ('route', 'occupancy_below_one_per_CU'),
                                   ('route', 'cooperative_launch_refused'), ('ring', 'hipHostMalloc_fails')}
    assert all(k not in got for k in sd.NOT_COVERED)
    assert len(sd.required()) == 100 and len(sd.MATRIX) == 31


def test_a_case_taken_out_is_named_by_the_cells_it_alone_carried():
    sole = sd.sole_carriers(sd.MATRIX)
    assert len(sole) >= 10, 'few sole carriers: the check below would be nearly vacuous'
    for cid, cells in sole.items():
        rest = {c: v for c, v in sd.MATRIX.items() if c != cid}
        lost = sd.missing(rest)
        for cell in cells:
            assert cell in lost, (cid, cell)
    rest = {c: v for c, v in sd.MATRIX.items() if not c.startswith('vol_')}
    assert ('route', 'volume') in sd.missing(rest) and ('volume', 'run_nested') in sd.missing(rest)
    rest = {c: v for c, v in sd.MATRIX.items() if c not in ('one', 'tile')}
    assert ('persistent', 'MC_1') in sd.missing(rest)


def test_lists_stay_within_eight_dependent_half_steps():
    worst = 0
    for cid, c in sd.MATRIX.items():
        ch = sr.chains(sd.to_slices(c.ops), c.geometry[0])
        worst = max(worst, ch['W'], ch['H'], ch['acc'])
        # poisoned accumulators: the first operation that touches acc overwrites it
        first = next((op for op in c.ops if op[0] in 'GW'), None)
        assert sd.zeroed_before_W(list(c.ops)) is None, cid
        if c.poison:
            assert first is not None and first[0] == 'G' and first[3] == 0, cid
    assert 7 <= worst <= sd.MAX_CHAIN
    seen = set()
    for N in (sd.T2[0], sd.BIG[0]):
        for seed in sd.RANDOM_SEEDS:
            ops, poison = sd.random_list(seed, N)
            assert 1 <= len(ops) <= 12
            ch = sr.chains(sd.to_slices(ops), N)
            assert max(ch['W'], ch['H'], ch['acc']) <= sd.MAX_CHAIN
            assert sd.validate(ops, N) is None and sd.zeroed_before_W(list(ops)) is None
            first = next((op for op in ops if op[0] in 'GW'), None)
            assert poison == bool(first and first[0] == 'G' and first[3] == 0)
            for op in ops:
                if op[0] != 'W':
                    n = op[2] - op[1]
                    seen.add('empty' if n == 0 else 'one' if n == 1 else 'all' if n == N else 'ragged')
                if op[0] == 'G':
                    seen.add(sd.ab_form(op[3], op[4]))
            seen |= {op[0] for op in ops} | ({'poison'} if poison else set())
    assert seen == {'empty', 'one', 'all', 'ragged', 'ab_0_1', 'ab_0_lambda', 'ab_1_1', 'ab_mix', 'H', 'G', 'W', 'poison'}
    assert len(sd.RANDOM_SEEDS) == 24


def test_chains_of_known_lists():
    ch = sr.chains(sd.to_slices(sd.ASAG), 10)
    # H(0,2) 1; G 2; W 2; H(2,10) 3; G 4, blended onto 2: 4; W 4
    assert (ch['H'], ch['acc'], ch['W']) == (3, 4, 4)
    assert sr.chains([('G', slice(2, 2), 0., 1.)], 5)['acc'] == 0
    assert sr.chains([('H', slice(0, 5)), ('H', slice(3, 4))], 5)['H'] == 2


# ----------------------------------------------------------------------------------------------------------------------
# what the older tests reached, counted with the mirror (DESIGN section 4e quotes the numbers)
# ----------------------------------------------------------------------------------------------------------------------
def _older_tests():
    L = sd.LAMBDA
    c1b = ((9, 10), (3, 6), (0, 3), (6, 9))
    g7b = ((4, 6), (0, 2), (6, 7), (2, 4))
    whole = (('H', 0, 10), ('G', 0, 10, 0., 1.), ('W',))
    asg = lambda bs: tuple(op for b in bs for op in (('H',) + b, ('G',) + b + (0., 1.), ('W',)))  # noqa: E731
    cyc = tuple(op for i, b in enumerate(sorted(g7b)) for op in (('H',) + b, ('G',) + b + (0. if i == 0 else 1., 1.))) + (('W',),)
    gsg = tuple(('H',) + b for b in g7b) + (('G',) + g7b[-1] + (0., 1.), ('W',))
    asag = tuple(op for i, b in enumerate(g7b) for op in (('H',) + b, ('G',) + b + ((0., L) if i == 0 else (1 - L, L)), ('W',)))
    gsag = tuple(('H',) + b for b in g7b) + (('G',) + g7b[-1] + (1 - L, L), ('W',))
    G7 = (7, 2, (20, 24), 5, (4, 5))
    run = (('H', 30, 40), ('H', 0, 5), ('H', 9, 9), ('H', 10, 20), ('H', 5, 10), ('H', 25, 30), ('G', 5, 9, 0., 1.), ('W',))
    return {
        'config1_fullbatch': sd.case(sd.C1, whole),
        'config1_asg': sd.case(sd.C1, asg(c1b)),
        **{f'seven_{n}': sd.case(G7, ops, modes=(1,)) for n, ops in (('cyclic', cyc), ('asg', asg(g7b)), ('gsg', gsg),
                                                                       ('asag', asag), ('gsag', gsag))},
        'joined_run': sd.case(sd.BIG, run, modes=(1,)),
        'overlapping_run': sd.case(sd.BIG, (('H', 0, 15), ('H', 10, 25)), modes=(1,)),
    }


def test_what_the_older_tests_reached():
    old = {k: v for k, v in sd.reached(_older_tests()).items() if v != ['ring'] and v != ['refusals']}
    req = sd.required()
    hit = {k for k in old if k in req}
    assert len(hit) == OLDER_TESTS_REACHED, (len(hit), sorted(req - hit))
    for key in (('persistent', 'nan_acc'), ('persistent', 'G_G_W'), ('persistent', 'W_alone'), ('persistent', 'empty_G_ab_0_1'),
                ('per_op', 'fft_arm_auto_next_to_direct'), ('route', 'tiny_at_2^18'), ('route', 'fits_false_shifts'),
                ('persistent', 'rows_gt_grid'), ('persistent', 'recon_small_and_plain_in_one_list'), ('persistent', 'no_r_scratch'),
                ('ring', 'ring_reuse'), ('refusal_volume', 'unknown_last'), ('route', 'volume')):
        assert key not in hit, key


OLDER_TESTS_REACHED = 29          # of the 100 required cells
