"""
CPU guard of the direct-kernel matrix: the host mirror of the dispatch (tests/direct_dispatch.py) is held to the C++ it
restates (api.hip, mfma.hip, generic.hip, read as text), and the geometries of tests/test_hip_direct_matrix.py are held to
reaching every dispatchable instance of the four MFMA kernels and of the generic direct kernels in both dtypes, and every
edge class of every kernel.  No GPU, no build.
"""
import os
import re

import numpy as np
import pytest

import direct_dispatch as dd
from conftest import ROOT

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _flat(text):
    """Source text with runs of white space and line continuations folded, so that a rule can be quoted on one line."""
    return re.sub(r'\s+', ' ', text.replace('\\\n', ' '))


# ----------------------------------------------------------------------------------------------------------------------
# the mirror against the sources
# ----------------------------------------------------------------------------------------------------------------------
def test_instance_lists_are_those_of_the_source():
    """The SET_LDS list of mfma_prepare_device and the LAUNCH_RC / LAUNCH_CH / LAUNCH_CP arms name the instances
    all_instances() lists; the generic launchers name theirs."""
    src = _read('mfma.hip')
    prep = src[src.index('int mfma_prepare_device()'):src.index('int mfma_reconstruct(')]
    rc = tuple((int(a), int(b)) for a, b in re.findall(r'SET_LDS\(\(k_mfma_reconstruct<(\d+), (\d+)>\)\);', prep))
    ch = tuple(int(a) for a in re.findall(r'SET_LDS\(\(k_mfma_corr_H<(\d+)>\)\);', prep))
    assert rc == dd.RECONSTRUCT_INSTANCES and ch == dd.CORR_H_NT

    body = src[src.index('int mfma_reconstruct('):src.index('int mfma_corr_W(')]
    launched = set()
    for cb, arm in re.findall(r'(?:case (\d)|default): (LAUNCH_RC(?:_NB)?\(\d(?:, \d)?\));', body[body.index('switch (pl.CB)'):]):
        nums = tuple(int(v) for v in re.findall(r'\d', arm))
        launched |= {(nums[0], nb) for nb in (0, 2, 3, 4)} if 'LAUNCH_RC_NB' in arm else {nums}
    assert launched == set(dd.RECONSTRUCT_INSTANCES), launched
    assert re.findall(r'case (\d): LAUNCH_RC\(CB_, (\d)\); break;', body) == [('2', '2'), ('3', '3'), ('4', '4')]
    assert 'default: LAUNCH_RC(CB_, 0); break;' in body

    body = src[src.index('int mfma_corr_W('):src.index('int mfma_corr_H_chunks(')]
    chain = _flat(body[body.index('const int nbp = Axp >> 1;'):body.index('#undef LAUNCH_CP')])
    conds = re.findall(r'(?:if \(([^)]*)\)|else) LAUNCH_CP\((\d), (\d)\);', chain)
    assert tuple((int(a), int(b)) for _, a, b in conds) == dd.PERSIST_ARMS
    assert [c for c, _, _ in conds] == ['ne <= 1 && nbp == 3', 'ne <= 1 && nbp == 4', 'ne <= 1 && nbp == 5',
                                        'ne <= 1 && nbp == 6', 'ne <= 2 && nbp == 8', 'ne <= 1', 'ne == 2', '']
    assert 'k_mfma_corr_W_persist<true, NE_, NBP_>' in body and 'k_mfma_corr_W_persist<false, NE_, NBP_>' in body
    assert '(k_mfma_corr_W<true>)' in body and '(k_mfma_corr_W<false>)' in body

    body = src[src.index('int mfma_corr_H(tnmf_hip_ctx'):]
    assert tuple(int(a) for a in re.findall(r'LAUNCH_CH\((\d+)\);', body)) == dd.CORR_H_NT

    gen = _read('generic.hip')
    for q in (4, 8, 16):
        assert f'k_reconstruct_small<T, {q}>' in gen
    for name in ('k_reconstruct<T>', '(k_corr_W<T, true>)', '(k_corr_W<T, false>)', 'k_corr_H<T>'):
        assert f'hipLaunchKernelGGL({name}' in gen, name
    assert len(dd.all_instances('mfma')) == 37 and len(dd.all_instances('generic')) == 14


def test_mirrored_constants_and_rules_are_those_of_the_source():
    """The lines the mirror restates.  When one of them changes, tests/direct_dispatch.py and the matrix's geometries have
    to be looked at again."""
    mfma, gen, api = _flat(_read('mfma.hip')), _flat(_read('generic.hip')), _flat(_read('api.hip'))
    for line in (
            f'constexpr int CW_TY = {dd.CW_TY}, CW_TX = {dd.CW_TX}, CW_RB = {dd.CW_RB}, CW_XSTR = {dd.CW_XSTR};',
            f'constexpr int CP_TY = {dd.CP_TY}, CP_RB = {dd.CP_RB}, CP_XE4 = {dd.CP_XE4};',
            f'constexpr int CH_RH = {dd.CH_RH};',
            f'constexpr int RC_RBK = {dd.RC_RBK};',
            f'constexpr int kBlock = {dd.kBlock};',
            # mfma_common and the three has-functions
            'if (dtype != 0) return false; if (g.Dy == 1 || g.Ay == 1) return false;',
            'if (g.Ax > 32 || g.Ay > 32) return false;',
            'if (g.Hx < 4) return false;',
            'return g.Ay >= 3 && g.Ay <= 16;',
            'const size_t lds_w = ((size_t)2 * (CW_TY + g.Ay - 1) * CW_XSTR + (size_t)g.Ay * ((g.Ax + 1) & ~1) * 32) * sizeof(float); return lds_w <= 64 * 1024;',
            'fake.num_cu = 256;',
            'return pl.lds <= 80 * 1024 && pl.NT <= 12 && pl.cg.TW <= 72 && g.Hx >= 4 && g.Dx >= 4;',
            # plan_reconstruct
            'pl.CB = (nbq >= 2 && nbq <= 4 && g.M <= 32) ? 1 : (g.C < 4 ? g.C : 4);',
            'pl.xblocks = cdiv(g.Dx, 64);',
            'const size_t ring = (size_t)4 * pl.CB * 256 * sizeof(float);',
            'const size_t per_atom = ((size_t)pl.CB * Axp4 * 16 + (size_t)RC_RBK * HST) * sizeof(float);',
            'const size_t budget = 72 * 1024;',
            'if (MB > 32) MB = 32; if (MB > g.M) MB = g.M; if (MB < 1) MB = 1;',
            # plan_corr_H
            'pl.JG = cdiv(tiles, 12); pl.NT = cdiv(tiles, pl.JG); pl.MT = cdiv(g.M, 32);',
            'cg.cblocks = cdiv(g.Hx, 72); cg.TW = (cdiv(g.Hx, cg.cblocks) + 3) & ~3; cg.XSTW = (cg.TW + 31) & ~31;',
            'while ((cg.AST & 31) != 2) ++cg.AST;',
            'long P = (2L * ctx->num_cu) / ((long)pl.MT * pl.JG);',
            'const long minP = (items * 2 * cg.TW + 32767) / 32768;',
            'if (P > items) P = items; if (P > 8192) P = 8192;',
            'const size_t plane = (size_t)(CH_RH + g.Ay - 1) * XST; const size_t ZL = cg.TW + XST + 8;',
            'const size_t stage = ((size_t)32 * cg.AST + 2 * ((size_t)nch_max * plane + ZL)) * sizeof(float);',
            # mfma_corr_W
            'const size_t lds_p = ((size_t)2 * SH * CW_XSTR + (size_t)g.C * g.Ay * Axp * 32) * sizeof(float);',
            'const int wpieces = SH * ((CW_TX + Axp - 1 + 3) / 4);',
            'if (lds_p <= 52 * 1024 && wpieces <= CP_XE4 * kBlock && g.Dx >= 4 &&',
            'const int tiles_y = cdiv(g.Hy, CP_TY), tiles_x = cdiv(g.Hx, CW_TX), MT = cdiv(g.M, 32);',
            'long P = (2L * ctx->num_cu) / MT;',
            'if (P > ntiles) P = ntiles;',
            'const int ne = (wpieces + kBlock - 1) / kBlock;',
            'const int tiles_y = cdiv(g.Hy, CW_TY), tiles_x = cdiv(g.Hx, CW_TX), MT = cdiv(g.M, 32);'):
        assert line in mfma, line
    for line in (
            'if (rows == 1) { t.TY = 1; t.TX = kBlock; } else if (cols >= 32 || rows < 16) { t.TY = 8; t.TX = 32; } else { t.TY = 16; t.TX = 16; }',
            f'constexpr int kSmallTY = {dd.kSmallTY}, kSmallTX = {dd.kSmallTX}, kSmallQ = {dd.kSmallQ};',
            f'constexpr int kMaxShiftsPerThread = {dd.kMaxShiftsPerThread};',
            'return ((size_t)q * ((size_t)(kSmallTY + g.Ay - 1) * (kSmallTX + g.Ax - 1) + (size_t)g.Ay * g.Ax) + (size_t)q * 64) * sizeof(T);',
            'return blocks < 64 && g.M >= kSmallQ && g.Dy > 1 && *lds_small <= 64 * 1024;',
            'if (g.M > 8 && reconstruct_small_lds<T>(g, 16) <= 64 * 1024)',
            'else if (g.M > 4 && reconstruct_small_lds<T>(g, 8) <= 64 * 1024)',
            'const Tile t = make_tile(g.Dy, g.Dx); const size_t lds = ((size_t)(t.TY + g.Ay - 1) * (t.TX + g.Ax - 1) + (size_t)g.Ay * g.Ax) * sizeof(T); if (lds > 64 * 1024) return TNMF_E_UNSUPPORTED;',
            'const Tile t = make_tile(g.Hy, g.Hx); const size_t lds = (2 * (size_t)(t.TY + g.Ay - 1) * (t.TX + g.Ax - 1) + (size_t)g.Ay * g.Ax) * sizeof(T); if (lds > 64 * 1024) return TNMF_E_UNSUPPORTED;',
            'if (nA > kBlock * kMaxShiftsPerThread) return TNMF_E_UNSUPPORTED; const int gs = nA < kBlock ? nA : kBlock; const int G = kBlock / gs;',
            'size_t lds = ((size_t)(t.TY + g.Ay - 1) * (t.TX + g.Ax - 1) + 2 * (size_t)t.TY * t.TX) * sizeof(T); const size_t red = (size_t)G * nA * 2 * sizeof(double);',
            'long P = ((long)ctx->num_cu * 8 + (long)g.M * g.C - 1) / ((long)g.M * g.C);',
            'if (P > items) P = items; if (P > 4096) P = 4096;'):
        assert line in gen, line
    for line in (
            'if (ctx->path == TNMF_PATH_GENERIC || ctx->path == TNMF_PATH_FFT) return false;',
            'case kReconstruct: return mfma_has_reconstruct(g, dtype); case kCorrW: return mfma_has_corr_W(g, dtype); default: return mfma_has_corr_H(g, dtype);',
            'if (g.Hs == g.Hx && use_mfma(ctx, g, dtype, kReconstruct)) {',
            'if ((!fused || g.Hs == g.Hx) && use_mfma(ctx, g, dtype, kCorrW)) {',
            'if (g.Hs == g.Hx && use_mfma(ctx, g, dtype, kCorrH)) {',
            'if (ctx->path == TNMF_PATH_MFMA) return g.Hs != g.Hx ? TNMF_E_STRIDE : TNMF_E_UNSUPPORTED;',
            'return fused && g.Hs != g.Hx ? TNMF_E_STRIDE : TNMF_E_UNSUPPORTED;',
            'if (ctx->path == TNMF_PATH_AUTO && (size_t)g.N * g.M * g.Hy * g.Hx < ((size_t)1 << 16)) return false;',
            'if (extra) return TNMF_E_UNSUPPORTED;'):
        assert line in api, line


@pytest.mark.parametrize('geometry,want', [
    # the baseline configurations and the shapes of test_hip_parity.py, as the comments of mfma.hip describe them
    ((1, 1, (128, 128), 16, (9, 9)), dict(rc=(1, 3), cw=(True, 1, 5), nt=6)),
    ((1, 1, (256, 256), 32, (12, 12)), dict(rc=(1, 3), cw=(True, 1, 6), nt=9)),
    ((1, 3, (256, 256), 32, (12, 12)), dict(rc=(1, 3), cw=(False, 0, 0), nt=9)),
    ((1, 3, (512, 512), 64, (16, 16)), dict(rc=(3, 0), cw=(False, 0, 0), nt=12)),
    ((2, 3, (33, 31), 7, (5, 8)), dict(rc=(1, 2), cw=(True, 1, 4), nt=8)),
])
def test_plans_of_known_shapes(geometry, want):
    g = dd.geo(geometry)
    rc, cw, ch = dd.plan_reconstruct(g), dd.plan_corr_W(g), dd.plan_corr_H(g)
    assert ((rc.CB, rc.NB), (cw.persist, cw.NE, cw.NBP), ch.NT) == (want['rc'], want['cw'], want['nt'])
    assert rc.lds <= 72 * 1024 + 16 * 1024 and ch.lds <= 80 * 1024


def test_make_tile_and_small_calls():
    assert dd.make_tile(1, 1000)[:2] == (1, 256)
    assert dd.make_tile(40, 32)[:2] == (8, 32) and dd.make_tile(15, 20)[:2] == (8, 32)
    assert dd.make_tile(16, 31)[:2] == (16, 16)
    small = lambda G, T: dd.generic_reconstruct(dd.geo(G), T)[0]  # noqa: E731
    assert small((3, 1, (32, 32), 10, (7, 7)), 'f') == ('k_reconstruct_small', 'f', 16)
    assert small((3, 1, (32, 32), 8, (7, 7)), 'd') == ('k_reconstruct_small', 'd', 8)
    assert small((3, 1, (32, 32), 4, (7, 7)), 'f') == ('k_reconstruct_small', 'f', 4)
    assert small((3, 1, (32, 32), 3, (7, 7)), 'f') == ('k_reconstruct', 'f')          # fewer atoms than waves
    assert small((16, 1, (32, 32), 10, (7, 7)), 'f') == ('k_reconstruct', 'f')        # 64 blocks
    assert small((2, 1, (300,), 10, (7,)), 'f') == ('k_reconstruct', 'f')             # 1-D


# ----------------------------------------------------------------------------------------------------------------------
# what can and cannot be dispatched
# ----------------------------------------------------------------------------------------------------------------------
def test_unreachable_is_what_no_accepted_geometry_selects():
    """Enumeration over the whole accepted domain of the persistent form (Ay, Ax <= 32, one channel: its LDS bound only
    tightens with C and the piece count does not depend on C): exactly seven (NE, NBP) arms are selected, <*, 3, 0> never."""
    arms = dd.persist_arms_reached()
    assert set(arms) == set(dd.PERSIST_ARMS) - {(3, 0)}, arms
    for C in range(1, 9):
        for Ay in range(2, 33):
            for Ax in range(1, 33):
                ok, wpieces, lds_p = dd.persist_accepts(C, Ay, Ax)
                if ok:
                    assert wpieces <= 2 * dd.kBlock and dd.persist_instance(wpieces, Ax) in arms, (C, Ay, Ax)
                if wpieces > 2 * dd.kBlock:
                    # (Ay >= 26 with Ax >= 21: at one channel the smallest such footprint is 101 KiB, at 30 x 21)
                    assert Ay >= 26 and Ax >= 21 and lds_p >= 103424 > 52 * 1024
    assert set(dd.UNREACHABLE) == {('k_mfma_corr_W_persist', f, 3, 0) for f in (True, False)}
    # every other instance is dispatchable: over C <= 8, Ay, Ax <= 32 and a few atom counts the plans name them all
    seen = set()
    for C in range(1, 9):
        for Ay in range(2, 33):
            for Ax in range(1, 33):
                for M in (4, 40):
                    for Dx in (3, 40):
                        G = (2, C, (20, Dx), M, (Ay, Ax))
                        seen |= {dd.cell(G, 'f', 'mfma', p).inst for p in dd.PRIMITIVES}
    assert seen - {None} == dd.all_instances('mfma') - set(dd.UNREACHABLE)
    assert len(dd.all_instances('mfma') - set(dd.UNREACHABLE)) == 35


def test_no_accepted_reconstruct_reads_before_a_row():
    """k_mfma_reconstruct loads 16 bytes from min(x, Hx - 4): no geometry mfma_has_reconstruct accepts may have rows
    narrower than four floats.  The rule before the guard accepted them under 'auto' and 'mfma' alike."""
    before, after = [], []
    for Dx in range(1, 6):
        for Ax in range(1, 6):
            for Ay in range(2, 18):
                g = dd.geo((2, 1, (20, Dx), 4, (Ay, Ax)))
                if g.Hx < 4 and dd.mfma_has_reconstruct(g, 'f', hx_guard=False):
                    before.append(g)
                if g.Hx < 4 and dd.mfma_has_reconstruct(g, 'f'):
                    after.append(g)
    assert not after
    assert len(before) == 6 * 14 and dd.geo((2, 1, (20, 3), 4, (3, 1))) in before     # Hx of 1, 2, 3 with Ay in 3..16
    for gid in ('h_hx3', 'h_hx1'):
        G = dd.MATRIX[gid]
        assert dd.cell(G, 'f', 'auto', 'reconstruct').family == 'generic'
        assert dd.cell(G, 'f', 'mfma', 'reconstruct') == dd._refused('E_UNSUPPORTED')
    assert dd.cell(dd.MATRIX['t_narrow'], 'f', 'mfma', 'reconstruct').inst == ('k_mfma_reconstruct', 1, 0)   # Hx = 4 stays


# ----------------------------------------------------------------------------------------------------------------------
# the matrix
# ----------------------------------------------------------------------------------------------------------------------
def _cells(family):
    out = []
    for gid, T, path in dd.matrix_cases():
        G = dd.MATRIX[gid]
        for prim in dd.PRIMITIVES:
            for padded in ((False, True) if path == 'generic' and not dd.geo(G).one_d else (False,)):
                c = dd.cell(G, T, path, prim, padded)
                if c.family == family:
                    out.append((gid, T, path, prim, c))
    return out


def test_matrix_reaches_every_dispatchable_instance():
    """Fused and unfused, every template argument, both dtypes of the generic kernels.  A geometry taken out of the matrix
    makes this name the instances only it reached."""
    reached = {c.inst for fam in ('mfma', 'generic') for *_, c in _cells(fam)}
    want = dd.all_instances() - set(dd.UNREACHABLE) - set(dd.NOT_COVERED)
    assert reached == want, sorted(want - reached, key=str)
    assert not dd.NOT_COVERED


def test_matrix_reaches_every_edge_of_every_kernel():
    met = {}
    for gid, T, path, prim, c in _cells('mfma'):
        key = c.inst[:2] if c.kernel in ('k_mfma_corr_W_persist', 'k_mfma_corr_W') else (c.kernel,)   # fused, unfused each
        met.setdefault(key, set()).update(c.edges)
    for key, got in sorted(met.items(), key=str):
        missing = set(dd.EDGES[key[0]]) - got
        assert not missing, (key, sorted(missing))
    assert len(met) == 6
    # the last column tile of the persistent form with one, two and three columns
    hx = {dd.geo(dd.MATRIX[gid]).Hx % 32 for gid, *_, c in _cells('mfma') if c.kernel == 'k_mfma_corr_W_persist'}
    assert {0, 1, 2, 3} <= hx, hx
    gmet = {}
    for gid, T, path, prim, c in _cells('generic'):
        gmet.setdefault((prim, T), set()).update(c.edges)
    for prim, want in dd.GENERIC_EDGES.items():
        for T in dd.DTYPES:
            # (float64 is never the MFMA family's to hand over)
            missing = {e for e in want if T == 'f' or not e.startswith('handover')} - gmet[(prim, T)]
            assert not missing, (prim, T, sorted(missing))


def test_matrix_cases_are_the_ones_that_add_a_cell():
    cases = dd.matrix_cases()
    assert len(set(cases)) == len(cases)
    by_path = {p: [c for c in cases if c[2] == p] for p in dd.PATHS}
    assert len(by_path['generic']) == 2 * len(dd.MATRIX)
    assert {gid for gid, *_ in by_path['auto']} == {'p20_tall', 't_narrow', 't_narrow_c2', 'h_hx3', 'h_hx1', 'h_ay2',
                                                     'h_ay17', 'h_24', 'h_32'}
    for gid, T, path in cases:
        G = dd.MATRIX[gid]
        fams = {dd.cell(G, T, path, prim).family for prim in dd.PRIMITIVES}
        assert fams <= {'mfma', 'generic', 'refused'}, (gid, T, path, fams)       # no split, no FFT in this matrix
        if path == 'generic':
            assert fams == {'generic'}, (gid, T)                                     # nothing beyond the 64 KiB refusals
    # what path='mfma' refuses in the matrix: the cases the GPU test expects the library's error for
    refused = {(gid, prim) for gid, T, path in by_path['mfma'] for prim in dd.PRIMITIVES
               if dd.cell(dd.MATRIX[gid], T, path, prim).family == 'refused'}
    assert refused == {('p20_tall', 'reconstruct'), ('h_hx3', 'reconstruct'), ('h_hx1', 'reconstruct'),
                       ('h_ay2', 'reconstruct'), ('h_ay17', 'reconstruct'), ('h_24', 'reconstruct'),
                       ('h_32', 'reconstruct'), ('h_24', 'grad_H'), ('h_24', 'update_H'), ('h_32', 'grad_H'),
                       ('h_32', 'update_H'), ('t_narrow', 'grad_W'), ('t_narrow_c2', 'grad_W'), ('h_hx3', 'grad_W'),
                       ('h_hx1', 'grad_W')}
    # row-padded activations: the MFMA family wants them contiguous, except for the unfused H gradient (it reads no H)
    G = dd.MATRIX['p13']
    assert dd.cell(G, 'f', 'mfma', 'reconstruct', padded=True) == dd._refused('E_STRIDE')
    assert dd.cell(G, 'f', 'mfma', 'update_H', padded=True) == dd._refused('E_STRIDE')
    assert dd.cell(G, 'f', 'mfma', 'grad_H', padded=True).family == 'mfma'
    assert dd.cell(dd.MATRIX['h_32'], 'f', 'mfma', 'update_H', padded=True) == dd._refused('E_STRIDE')   # (the stride first)
    assert dd.cell(dd.MATRIX['h_32'], 'f', 'mfma', 'grad_H', padded=True) == dd._refused('E_UNSUPPORTED')
    assert dd.cell(G, 'f', 'auto', 'reconstruct', padded=True).family == 'generic'


def test_contractions_stay_inside_what_the_bars_are_held_for():
    """C*Ay*Ax <= 768 (H gradient), M*Ay*Ax <= 16384 (reconstruct), N*Dy*Dx <= 512^2 (W gradient) -- with one exception
    the hand-over of 32 x 32 atoms cannot avoid: 1024 terms in its H gradient, whose bar the GPU test scales by
    sqrt(1024 / 768)."""
    over = {(gid, prim): dd.contraction(G, prim) for gid, G in dd.MATRIX.items() for prim in dd.PRIMITIVES
            if dd.contraction(G, prim) > dd.K_HELD[prim]}
    assert over == {('h_32', 'grad_H'): 1024, ('h_32', 'update_H'): 1024}
    for gid, G in dd.MATRIX.items():
        g = dd.geo(G)
        assert G[0] * G[3] * g.Hy * g.Hx <= 1 << 22, gid          # skinny: the largest H is 3.2e6 entries


def test_corner_activations_leave_an_empty_region():
    """With single ones at the corners and the centre of every plane, R is a sum of shifted copies of W: on every geometry
    some pixel of every sample is reached by none of them (the GPU test's leak check needs it)."""
    for gid, (N, C, D, M, A) in dd.MATRIX.items():
        Hs = tuple(d + a - 1 for d, a in zip(D, A))
        for n in range(N):
            reached = np.zeros(D, dtype=bool)
            for m in range(M):
                for j, spot in enumerate(dd.corner_spots(Hs)):
                    if (n + m + j) % 2 == 0:
                        # H[spot] contributes to R[d] for spot - (A - 1) <= d <= spot
                        sl = tuple(slice(max(s - a + 1, 0), min(s, d - 1) + 1) for s, a, d in zip(spot, A, D))
                        reached[sl] = True
            assert reached.any() and not reached.all(), (gid, n)


def test_quoted_counts():
    """The counts quoted in the matrix's comments, on 256 compute units."""
    cw = dd.cell(dd.MATRIX['p15_loop'], 'f', 'mfma', 'update_H').info
    assert (cw.ntiles, cw.P) == (81, 73) and cw.ntiles % cw.P != 0
    ch = dd.cell(dd.MATRIX['p15_loop'], 'f', 'mfma', 'grad_W').info
    assert (ch.NT, ch.items, ch.P) == (5, 102, 73)
    rc = dd.cell(dd.MATRIX['p15_loop'], 'f', 'mfma', 'reconstruct').info
    assert (rc.CB, rc.NB, rc.MB, rc.chunks) == (1, 3, 32, 7)
    # the issue's example of the same loop: 588 tiles on P = 73 with a reconstruct of 16000 terms
    big = (3, 1, (100, 410), 200, (8, 10))
    assert dd.plan_corr_W(dd.geo(big))[-2:] == (588, 73) and dd.contraction(big, 'reconstruct') == 16000
    rc = dd.cell(dd.MATRIX['p28'], 'f', 'mfma', 'reconstruct').info
    assert (rc.NB, rc.MB, rc.chunks) == (4, 30, 2)
    rc = dd.cell(dd.MATRIX['r40'], 'f', 'mfma', 'reconstruct').info
    assert (rc.CB, rc.MB, rc.chunks) == (4, 17, 3)
    ch = dd.cell(dd.MATRIX['r40'], 'f', 'mfma', 'grad_W').info
    assert (ch.NT, ch.JG, ch.nch_max) == (12, 1, 4)
    ch = dd.cell(dd.MATRIX['t_c5'], 'f', 'mfma', 'grad_W').info
    assert (ch.NT, ch.JG, ch.cblocks, ch.TW) == (12, 3, 2, 72)
    ch = dd.cell(dd.MATRIX['nt8'], 'f', 'mfma', 'grad_W').info
    assert (ch.NT, ch.cblocks, ch.TW) == (8, 3, 52)
    ch = dd.cell(dd.MATRIX['p16_c3'], 'f', 'mfma', 'grad_W').info
    assert (ch.NT, ch.JG, ch.nch_max) == (11, 2, 2)
    assert not dd.cell(dd.MATRIX['r30'], 'f', 'mfma', 'grad_H').info.persist
    assert not dd.cell(dd.MATRIX['t_c5'], 'f', 'mfma', 'grad_H').info.persist
    assert dd.cell(dd.MATRIX['g_1d_long'], 'd', 'generic', 'grad_W').info[5] == 2
    assert dd.cell(dd.MATRIX['h_32'], 'f', 'generic', 'grad_W').info[5] == 4
