"""The host model of the context's buffers (tests/context_dispatch.py) against the sources and against itself: which entry
point touches which buffer is read off api.hip as text, the byte formulas and the one history-dependent branch are pinned
line by line, and at 64, 256 and 304 compute units the sequences carry every transition, every `regrow` pair grows, every
`dirty` pair does not, and what the predecessors of a `dirty` pair laid out covers what its last call uses.  No GPU, no torch."""
import os
import re

import pytest

import context_dispatch as cx
import schedule_dispatch as sd

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tnmf_amd', 'csrc')


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


API = source('api.hip')

# what in a function's body means "this buffer": the ensure_* of api.hip, and the calls into the two families that keep a
# buffer of their own (fft.hip: ensure_ws behind fft_prepare / fft_reserve; split_kernels.h: the W images of launch())
TOKENS = {
    'ws': r'\bensure_scratch\(|\bvol_scratch\(',
    'hw': r'\bensure_hwork\(',
    'qb': r'ensure_buffer\(&ctx->qb',
    'ob': r'ensure_buffer\(&ctx->ob',
    'fft.ws': r'\bfft_reserve\(|\bfft_reconstruct\(|\bfft_grad_H\(|\bfft_update_H\(|\bfft_grad_W\(',
    'wimg': r'\bsplit_corr_W\(',
}


def functions(text):
    """{name: body} of every function definition that starts in column 0 (or behind `static` / `inline`) and ends with a
    `}` in column 0."""
    out = {}
    pat = re.compile(r'^(?:static |inline )*(?:int|bool|Scratch|const char \*|size_t)\s+\*?(\w+)\([^;{]*\)\s*\{\n(.*?)^\}', re.M | re.S)
    for m in pat.finditer(text):
        out[m.group(1)] = m.group(2)
    return out


def touched(name, funcs, memo):
    """Buffers the body of `name` names, and those of every function of api.hip it calls."""
    if name in memo:
        return memo[name]
    memo[name] = set()
    body = funcs[name]
    got = {b for b, pat in TOKENS.items() if re.search(pat, body)}
    for other in funcs:
        if other != name and re.search(r'\b%s\(' % re.escape(other), body):
            got |= touched(other, funcs, memo)
    memo[name] = got
    return got


def test_uses_is_what_api_hip_says():
    funcs = functions(API)
    entries = sorted(n for n in funcs if n.startswith('tnmf_hip_'))
    # (the scan sees every entry point api.hip defines, not a corner of it)
    defined = set(re.findall(r'^(?:int|const char \*)\s*(tnmf_hip_\w+)\(', API, re.M))
    one_liners = {'tnmf_hip_abi_version', 'tnmf_hip_ctx_last_path', 'tnmf_hip_ctx_last_schedule_persistent', 'tnmf_hip_strerror'}
    assert defined - set(entries) == one_liners and len(entries) >= 60      # (four accessors that read one field, or none)
    memo = {}
    scanned = {n: touched(n, funcs, memo) for n in entries}
    scanned = {n: b for n, b in scanned.items() if b}
    model = {n: {u.split(':')[0] for u in uses} for n, uses in cx.USES.items()}
    assert sorted(scanned) == sorted(model), (sorted(set(scanned) ^ set(model)))
    for n in scanned:
        assert scanned[n] == model[n], (n, sorted(scanned[n]), sorted(model[n]))
    # the helpers the scan follows are where the model says they are
    for helper in ('vol_scratch', 'beta_fields_of', 'sample_objective_of', 'update_H_2d', 'grad_W_2d', 'energy_2d',
                   'vol_api_update_H_ex', 'vol_api_run_schedule', 'do_reconstruct', 'do_corr_W', 'do_corr_H'):
        assert helper in funcs, helper
    assert set(x for u in cx.USES.values() for x in u) == set(cx.LAYOUTS)
    # nobody else lays out a buffer of the context: the other sources name none of them
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(('.hip', '.h')) and name not in ('api.hip', 'common.h', 'fft.hip', 'split.hip', 'split_kernels.h'):
            assert not re.search(r'ctx->(ws|hw|qb|ob|wimg)\b|ensure_(scratch|hwork|buffer)', source(name)), name


def test_a_deleted_row_of_uses_is_noticed():
    funcs = functions(API)
    memo = {}
    scanned = {n for n in funcs if n.startswith('tnmf_hip_') and touched(n, funcs, memo)}
    for gone in cx.USES:
        assert scanned != set(cx.USES) - {gone}


PINNED = (
    # ensure_buffer
    'const size_t want = align_up(bytes + (slack ? bytes / 8 : 0), 1 << 20);',
    'int ensure_scratch(tnmf_hip_ctx *ctx, size_t bytes) { return ensure_buffer(&ctx->ws, &ctx->ws_bytes, bytes, true); }',
    'int ensure_hwork(tnmf_hip_ctx *ctx, size_t bytes) { return ensure_buffer(&ctx->hw, &ctx->hw_bytes, bytes, false); }',
    # plan_scratch
    's.r_bytes = align_up((size_t)g.N * g.C * g.Dy * g.Dx * esize(dtype), 256);',
    's.part_bytes = align_up((size_t)P * g.M * g.C * g.Ay * g.Ax * 2 * sizeof(double), 256);',
    's.red_bytes = align_up((size_t)(kEnergyPartials + 8) * sizeof(double), 256);',
    's.total = s.red_off + s.red_bytes;',
    # vol_scratch
    'const int rc = ensure_scratch(ctx, r_bytes + e_bytes + p_bytes + extra);',
    # the field Q, the objective's partial sums
    'CHECK(ensure_buffer(&ctx->qb, &ctx->qb_bytes, align_up(n * esize(dtype), 256), false));',
    'if (B > 1) CHECK(ensure_buffer(&ctx->ob, &ctx->ob_bytes, align_up(N * B * sizeof(double), 256), false));',
    'CHECK(ensure_buffer(&ctx->ob, &ctx->ob_bytes, p_bytes + atom_terms_taps_bytes(g, dtype), false));',
    'CHECK(ensure_buffer(&ctx->ob, &ctx->ob_bytes, wk.total, false));',
    'CHECK(ensure_buffer(&ctx->ob, &ctx->ob_bytes, correlogram_partial_bytes(p), false));',
    # the H half step's work arrays, and the one branch that looks at what ran before
    'const size_t nE = align_up((size_t)g.N * g.M * g.Hy * g.Hs * es, 256);',
    'const size_t nG = align_up((size_t)g.N * g.M * g.Hy * g.Hx * es, 256);',
    'CHECK(ensure_hwork(ctx, nE));',
    'if (ctx->hw_bytes < nE + 2 * nG) {',
    'CHECK(ensure_hwork(ctx, nE + 2 * nG));',
    'CHECK(ensure_hwork(ctx, 3 * nP + nE));',
    'CHECK(ensure_hwork(ctx, lat + 2 * nS + pad));',
    'const size_t lat = lateral ? 2 * nS : 0, pad = mode == TNMF_MODE_VALID ? 0 : 3 * nP;',
    # the two layouts of tnmf_hip_run_schedule, the ring
    'CHECK(ensure_scratch(ctx, r_bytes + p_bytes + o_bytes + 1024));',
    'const size_t o_bytes = align_up((size_t)n_ops * sizeof(tnmf_hip_op), 256);',
    'CHECK(ensure_scratch(ctx, scm.total + align_up(2 * wn * es, 256)));',
    'CHECK(vol_scratch(ctx, vmax, dtype, &Rws, nullptr, &part, &Pmax, align_up(2 * wn * es, 256)));',
    'ctx->ops_next = (slot + 1) % tnmf_hip_ctx::kOpSlots;',
    'ctx->ops_cap[slot] = align_up(need, 4096);',
)


@pytest.mark.parametrize('line', PINNED)
def test_the_formulas_the_model_restates_stand_in_api_hip(line):
    assert API.count(line) >= 1, line


def test_constants_and_the_other_two_allocators():
    assert 'constexpr int kEnergyPartials = %d;' % cx.K_ENERGY_PARTIALS in source('generic.h')
    assert 'constexpr int kObjChunk = %d;' % cx.K_OBJ_CHUNK in source('beta.h')
    assert 'static constexpr int kOpSlots = %d;' % sd.K_OP_SLOTS in source('common.h')
    assert 'const size_t wbytes = (size_t)MT * g.C * Cfg::wimg;' in source('split_kernels.h')
    assert 'if (wbytes > ctx->wimg_bytes) {' in source('split_kernels.h')
    fft = source('fft.hip')
    assert re.search(r'align_up\(bytes, \(?(size_t\))?1 << 20\)?', fft) or '1 << 20' in fft
    assert 'return align_up((size_t)g.N * atom_terms_plan(g).slots * (g.M / group) * 2 * sizeof(double), 256);' in source('atoms.hip')
    assert 'return align_up((size_t)g.N * p.strips * p.pairs * p.wg_doubles * sizeof(double), 256);' in source('atom_gram.hip')
    assert 'return align_up((size_t)p.nseg * p.strips * p.pairs * p.nh * 256 * sizeof(double), 256);' in source('correlogram.hip')


def test_capacity_rules_by_hand():
    MiB = cx.MiB
    # ensure_buffer(..., slack): an eighth on top, then whole MiB
    assert cx.ensure_buffer(0, 1, True) == MiB and cx.ensure_buffer(0, 1, False) == MiB
    assert cx.ensure_buffer(0, MiB, False) == MiB
    assert cx.ensure_buffer(0, MiB, True) == 2 * MiB                 # 1 MiB + 128 KiB
    assert cx.ensure_buffer(0, MiB + 1, False) == 2 * MiB and cx.ensure_buffer(0, MiB + 1, True) == 2 * MiB
    assert cx.ensure_buffer(0, 8 * MiB, True) == 9 * MiB
    assert cx.ensure_buffer(2 * MiB, MiB + 1, True) == 2 * MiB       # fits: nothing moves
    # the ring: slot and whether the call waits for the event of the call four before it
    assert [cx.ring_slot(n) for n in (1, 4, 5, 9)] == [(0, False), (3, False), (0, True), (0, True)]
    assert [(s, w) for s, w, _ in sd.ring((1,) * 9)] == [cx.ring_slot(n) for n in range(1, 10)]
    # a slot's capacity: 4 KiB steps of 32-byte operations
    ctx = cx.Context(256)
    ctx.path = 'generic'
    op = cx.Op('schedule', 'sched', cx.SMALL, 'f')
    for n in (3, 5, 6, 130, 129, 200):
        cx.call(ctx, op, n)
    assert ctx.ring_cap == [8192, 8192, 4096, 8192] and ctx.ring_next == 2
    assert {'ring_wrap', 'ring_slot_regrow'} <= ctx.seen


def test_operands_of_predecessors_stay_far_from_overflow():
    """2^12 times operands below OPERAND_MAX: the largest intermediate is a sum of squares of reconstructions over the
    largest sample, far inside float32."""
    worst = 0.
    for (fam, size), (N, C, D, M, A) in cx.GEOMETRY.items():
        r = cx.OPERAND_MAX * cx.PREDECESSOR_SCALE * M * cx.prod(A) * 4.     # |R| <= sum of M * prod(A) products, |V| <= 4 * that
        worst = max(worst, r * r * N * C * cx.prod(D))
    assert worst < 1e30 < 3.4e38, worst


@pytest.mark.parametrize('cus', cx.CUS)
def test_sequences_carry_every_transition(cus):
    assert cx.missing(cus=cus) == []
    assert not set(cx.NOT_REACHED) & set(cx.TRANSITIONS)
    assert cx.check_sizes(cus)
    for name, seq in cx.SEQUENCES.items():
        rcs = [rc for rc, _ in cx.run(seq, cus)[0]]
        assert all(rc == 0 or isinstance(item, cx.Ctl) and item.what == 'refuse' for rc, item in zip(rcs, seq.items)), name
    # every (entry point, layout) of the ops is a row of USES
    for op in cx.OPS:
        for path in cx.KINDS[op.kind][3]:
            if cx.allowed(op, path):
                for persistent in (0, 1):
                    for b, u in cx.uses_of(op, cus, path, persistent)[0].items():
                        assert u.layout in cx.USES[cx.KINDS[op.kind][0]], (op, path, u.layout)


def _calls(seq):
    return [it for it in seq.items if isinstance(it, cx.Op)]


@pytest.mark.parametrize('cus', cx.CUS)
def test_regrow_pairs_grow_and_dirty_pairs_do_not(cus):
    for name, seq in cx.SEQUENCES.items():
        if seq.kind != 'pair':
            continue
        buffer = name[name.index('(') + 1:].split(':')[0].split(')')[0]
        ctx = cx.Context(cus)
        before_last = None
        extents = []
        for i, item in enumerate(seq.items):
            if item is _calls(seq)[-1] and i == len(seq.items) - 1:
                before_last = ctx.cap[buffer]
            cx.step(ctx, item)
            if isinstance(item, cx.Op) and ctx.last[buffer] is not None:
                extents.append(ctx.last[buffer].extent)
        if name.startswith('regrow('):
            assert 0 < before_last < ctx.cap[buffer], (name, before_last, ctx.cap[buffer])
            assert f'regrow({buffer})' in ctx.seen
        else:
            assert before_last == ctx.cap[buffer] > 0, (name, 'the last call of a dirty pair grew the buffer')
            # what the predecessors laid out covers everything the last call uses of the buffer
            assert max(extents[:-1]) >= extents[-1], (name, extents)
            assert name.split('[')[0] in ctx.seen, name


def test_removing_a_sole_carrier_loses_exactly_its_transitions():
    sole = cx.sole_carriers()
    assert sole
    for base, cells in sole.items():
        rest = {n: s for n, s in cx.SEQUENCES.items() if cx.base_of(n) != base}
        assert set(cx.missing(rest)) == set(cells), base


def test_walks_between_them_reach_every_pair_transition_twice():
    count = {}
    for seed in cx.WALK_SEEDS:
        seq = cx.SEQUENCES[f'walk[{seed}]']
        assert 35 <= len(_calls(seq)) <= 45
        for t in cx.reached(seq):
            count[t] = count.get(t, 0) + 1
    pairs = [t for t in cx.TRANSITIONS if t.startswith('dirty(')]
    assert len(pairs) >= 40
    assert [t for t in pairs if count.get(t, 0) < 2] == []
    assert all(count.get(f'regrow({b})', 0) >= 2 for b in ('ws', 'hw', 'qb', 'ob', 'fft.ws'))


def test_ring_and_tap_runs_are_what_they_claim():
    for T in 'fd':
        seq = cx.SEQUENCES[f'ring[{T}]']
        n_sched = sum(1 for it in seq.items if isinstance(it, tuple) and it[0] == 'schedule_n')
        assert n_sched >= 6
        got = cx.reached(seq)
        assert {'ring_wrap', 'ring_slot_regrow', 'dirty(ws: sched_persistent -> plan)', 'dirty(ws: plan -> sched_persistent)'} <= got
        got = cx.reached(cx.SEQUENCES[f'tap[{T}]'])
        assert {'tap_set', 'tap_cleared', 'tap_then_ob_user'} <= got
        got = cx.reached(cx.SEQUENCES[f'lateral_fallback[{T}]'])
        assert {'lateral_fallback_regrow', 'lateral_fallback_no_regrow'} <= got
        _, ctxs = cx.run(cx.SEQUENCES[f'reserved_first[{T}]'])
        assert 'reserved_first' in ctxs[False].seen and 'reserved_too_small' not in ctxs[False].seen


def test_nothing_is_history_dependent_and_the_unreached_are_explained():
    assert cx.HISTORY_DEPENDENT == {}                 # DESIGN.md 4ae explains every entry one by one: there is none
    assert set(cx.NOT_REACHED) == {'hipMalloc_refused', 'persistent_refused_falls_through'}
    assert all(len(why) > 40 for why in cx.NOT_REACHED.values())
    assert all(len(why) > 20 for why in cx.SAME_STEP.values())
