"""
CPU guard of the lateral matrix: the host mirror of the H half step in full (tests/lateral_dispatch.py) is held to the
C++ it restates (inhibit.hip, generic.h, generic.hip, modes.h, api.hip, read as text), and the cases of
tests/test_hip_lateral_matrix.py are held to reaching all eight k_inhibition instances, both dtypes of k_mu_update_extra,
k_fold_update, k_pad_H, k_fold_H and k_convolve_axis, every edge class on every instance that can have it, every refusal
and every route of update_H_2d.  No GPU, no build.
"""
import os
import re

import direct_dispatch as dd
import lateral_dispatch as ld
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
def test_mirrored_constants_and_rules_are_those_of_the_source():
    """The lines the mirror restates.  When one of them changes, tests/lateral_dispatch.py and the matrix's cases have to
    be looked at again."""
    inh, hdr, gen, api = (_flat(_read(n)) for n in ('inhibit.hip', 'generic.h', 'generic.hip', 'api.hip'))
    for line in (
            f'constexpr int kTY = {ld.kTY}, kTX = {ld.kTX}, kThreads = {ld.kThreads};',
            f'constexpr int kPre = {ld.kPre};',
            # the kernel's tile and its staging
            'const int ry = (ly - 1) / 2, rx = (lx - 1) / 2;',
            'const int SH = kTY + 2 * ry, SW = (kTX + 2 * rx + 8) | 1;',
            'constexpr int S1 = kTX + 1;',
            'const unsigned whole = gridDim.x / 8 * 8; if (bid < whole) bid = (bid & 7) * (whole / 8) + (bid >> 3);',
            'const int nel = SH * SW; const bool pre_ok = nel <= kPre * kThreads;',
            'const int npre = (nel + kThreads - 1) / kThreads;',
            f'for (int k0 = 0; k0 < npre; k0 += {ld.kBatch}) {{ T tmp[kPre]; fetch(m, k0, tmp, {ld.kBatch}); park(k0, tmp, {ld.kBatch}); }}',
            'const bool cross = xc != T(0);',
            'E[o] = inh * (g4[j] - A0[(size_t)(4 * rg + j + ry) * SW + col + rx]);',
            'E[o] = inh * (gv - H[o]) + xc * (S[j] - gv);',
            # the launcher: LDS formula, both byte limits, the plane and grid guards, the reversal of the taps
            'const size_t SH = kTY + 2 * ry, SW = (kTX + 2 * rx + 8) | 1; const size_t lds = (SH * SW + SH * (kTX + 1)) * sizeof(T);',
            f'if (lds > {ld.LDS_MAX // 1024} * 1024) return TNMF_E_UNSUPPORTED;',
            'if ((size_t)Hy * ld * sizeof(T) >= ((size_t)1 << 31)) return TNMF_E_UNSUPPORTED;',
            'taps.ky[i] = i < ly ? (T)ky_host[ly - 1 - i] : T(0); taps.kx[i] = i < lx ? (T)kx_host[lx - 1 - i] : T(0);',
            'const int tiles_y = cdiv(Hy, kTY), tiles_x = cdiv(ld, kTX); const size_t blocks = (size_t)N * tiles_y * tiles_x; '
            'if (blocks > 0x7fffffffull) return TNMF_E_GEOM;',
            f'if (lds > {ld.LDS_PLAIN // 1024} * 1024) TNMF_HIP_TRY(hipFuncSetAttribute((const void *)k_inhibition<T, LY_, LX_>, '
            f'hipFuncAttributeMaxDynamicSharedMemorySize, {ld.LDS_MAX // 1024} * 1024));',
            'if (ly < 1 || lx < 1 || ly > kMaxTaps || lx > kMaxTaps || !(ly & 1) || !(lx & 1)) return TNMF_E_UNSUPPORTED; '
            'if (N <= 0) return TNMF_OK;',
            # the fold + update: the duplicate positions are those of modes.h
            'const int jy[2] = {Py == 1 ? 0 : uy + Ay - 1, Py == 1 ? -1 : pad_dup(uy, Sy, Ay, mode)};'):
        assert line in inh, line
    modes = _flat(_read('modes.h'))
    for line in (
            # the per-axis rule, stated once: the shift length, the limits, the duplicate-position table
            'return mode == TNMF_MODE_VALID ? D + a - 1 : (mode == TNMF_MODE_FULL ? D - a + 1 : D);',
            'return S >= 1 && (mode != TNMF_MODE_CIRCULAR || a - 1 <= S) && (mode != TNMF_MODE_REFLECT || a - 1 < S);',
            'if (mode == TNMF_MODE_CIRCULAR) return u >= S - l ? u - (S - l) : -1; '
            'if (mode == TNMF_MODE_REFLECT) return (u >= 1 && u <= l) ? l - u : -1; return -1;'):
        assert modes.count(line) == 1, line
    for name in ('generic.hip', 'inhibit.hip', 'volume.hip', 'event_walk.h'):   # ... and nowhere else
        text = _read(name)
        assert '#include "modes.h"' in text and not re.search(r'TNMF_MODE_(FULL|CIRCULAR|REFLECT)', text), name
    assert f'constexpr int kMaxTaps = {ld.kMaxTaps};' in hdr
    assert ld.PLANE_LIMIT == 1 << 31 and ld.BLOCKS_LIMIT == 0x7fffffff
    for line in (
            # launch_pad_fold and its guards; the convolution of the front end's fall-back
            'const int Sy = mode_shift_len(mode, g.Dy, g.Ay), Sx = mode_shift_len(mode, g.Dx, g.Ax); '
            'if (!mode_axis_ok(mode, Sy, g.Ay) || !mode_axis_ok(mode, Sx, g.Ax)) return TNMF_E_GEOM;',
            'const int jy[2] = {Py == 1 ? 0 : uy + Ay - 1, Py == 1 ? -1 : pad_dup(uy, Sy, Ay, mode)};',
            'if (ntaps < 1 || ntaps > kMaxTaps || (ntaps & 1) == 0) return TNMF_E_UNSUPPORTED;',
            'const int src = i + rad - t;'):
        assert line in gen, line
    pad_fold = gen.index('int launch_pad_fold(')
    assert len(re.findall(r'return TNMF_E_GEOM;', gen[pad_fold:gen.index('with_dtype(', pad_fold)])) == 1   # (the three limits)
    for line in (
            # update_H_2d
            'const bool lateral = inhibition > 0 || cross_inhibition > 0;',
            'const double *ky = geom->ndim == 2 ? kernel0 : &one, *kx = geom->ndim == 2 ? kernel1 : kernel0; '
            'const int ly = geom->ndim == 2 ? len0 : 1, lx = geom->ndim == 2 ? len1 : len0;',
            'return cross_inhibition > 0 && M > 1 ? cross_inhibition / (M - 1) : 0.0;',
            'const double xc = cross_weight(cross_inhibition, g.M);',
            'const size_t nE = align_up((size_t)g.N * g.M * g.Hy * g.Hs * es, 256); '
            'const size_t nG = align_up((size_t)g.N * g.M * g.Hy * g.Hx * es, 256);',
            'CHECK(ensure_hwork(ctx, nE)); E = ctx->hw; '
            'CHECK(launch_inhibition(ctx, dtype, g.N, g.M, g.Hy, g.Hs, H_inout, E, ky, ly, kx, lx, inhibition, xc, s));',
            'if (!E || (rc != TNMF_E_UNSUPPORTED && rc != TNMF_E_STRIDE)) return rc;',
            'if (ctx->hw_bytes < nE + 2 * nG) {',
            'CHECK(do_corr_W(ctx, g, dtype, V, Rs, W, nullptr, neg, pos, false, 0.0, s));',
            'return launch_mu_update_extra(ctx, dtype, H_inout, neg, pos, E, (size_t)g.N * g.M * g.Hy, g.Hx, g.Hs, reg, s);',
            'const int Sy = geom->ndim == 1 ? 1 : mode_shift_len(mode, g.Dy, g.Ay), Sx = mode_shift_len(mode, g.Dx, g.Ax); '
            'if (Sy < 1 || Sx < 1) return TNMF_E_GEOM;',
            'CHECK(ensure_hwork(ctx, 3 * nP + nE));',
            'CHECK(launch_pad_fold(ctx, g, dtype, mode, false, H_inout, Hp, s)); CHECK(do_reconstruct(ctx, g, dtype, W, Hp, Rs, s));',
            'if (lateral) CHECK(launch_inhibition(ctx, dtype, g.N, g.M, Sy, Sx, H_inout, E, ky, ly, kx, lx, inhibition, xc, s));',
            'return launch_fold_update(ctx, g, dtype, mode, Sy, Sx, H_inout, negp, posp, E, reg, s);',
            # do_corr_W with the extra term, the work buffer
            'if (extra && (!fused || ctx->path == TNMF_PATH_FFT)) return TNMF_E_UNSUPPORTED;',
            'if (extra) return TNMF_E_UNSUPPORTED;',
            'int ensure_hwork(tnmf_hip_ctx *ctx, size_t bytes) { return ensure_buffer(&ctx->hw, &ctx->hw_bytes, bytes, false); }',
            'if (bytes <= *have) return TNMF_OK;',
            'const size_t want = align_up(bytes + (slack ? bytes / 8 : 0), 1 << 20);'):
        assert line in api, line
    assert ld.HW_ALIGN == 1 << 20
    assert 'if (extra && (!fused || g.Hs % SP_TX != 0 || Cfg::ONE_D)) return TNMF_E_UNSUPPORTED;' in _flat(_read('split_kernels.h'))
    # volumes share the guards of the modes
    assert 'if (!mode_axis_ok(mode, q.S[i], v.A[i])) return TNMF_E_GEOM;' in _flat(_read('volume.hip'))


def test_launch_chain_is_that_of_the_source():
    """The INH_LAUNCH chain: three compile-time instances in this order, then the run-time one; both dtypes, which every
    launcher reaches as <T> inside a with_dtype call (common.h: a float arm and a double arm)."""
    src = _flat(_read('inhibit.hip'))
    chain = src[src.index('if (ly == 23 && lx == 23)'):src.index('#undef INH_LAUNCH')]
    arms = re.findall(r'(?:if \(ly == (\d+) && lx == (\d+)\)|else) INH_LAUNCH\((\d+), (\d+)\);', chain)
    assert [(int(c), int(d)) for _, _, c, d in arms] == list(ld.COMPILED) + [(0, 0)]
    assert all((a, b) == (c, d) for a, b, c, d in arms[:-1]) and arms[-1][:2] == ('', '')
    common = _flat(_read('common.h'))
    assert 'if (dtype == 0) return f(float{}); return f(double{});' in common[common.index('with_dtype(int dtype, F &&f)'):]
    assert 'return with_dtype(dtype, [&](auto zero) { return launch_inhibition_t<decltype(zero)>(' in src
    assert len(ld.all_inhibition_instances()) == 8
    for k in ('k_mu_update_extra', 'k_fold_update'):
        assert f'with_dtype(dtype, [&](auto zero) {{ using T = decltype(zero); hipLaunchKernelGGL({k}<T>' in src
    gen = _flat(_read('generic.hip'))
    for k in ('k_fold_H', 'k_pad_H', 'k_convolve_axis'):
        assert f'with_dtype(dtype, [&](auto zero) {{ using T = decltype(zero); hipLaunchKernelGGL({k}<T>' in gen
    assert re.search(r'if \(fold\) with_dtype\(.*?k_fold_H<T>.*?\}\); else with_dtype\(.*?k_pad_H<T>', gen)


def test_lengths_quoted_in_the_design_notes():
    """The boundaries DESIGN section 4d quotes, from the constants alone."""
    square = lambda T, l: ld.inhibition(T, 1, 1, 32, 32, l, l)  # noqa: E731
    assert square('f', 27).staging == 'prefetch' and square('f', 29).staging == 'batched'
    assert (square('f', 31).nel, square('f', 31).npre, square('f', 31).staging) == (4402, 18, 'batched')
    assert {l for l in range(1, 128, 2) if (l, l) in ld.COMPILED and square('f', l).staging == 'batched'} == {31}
    # the default ranges of direct_dispatch.MATRIX (atom size - 1 per axis): only (31, 31) is batched, (17, 17) is absent
    default = {tuple(2 * (a - 1) + 1 for a in G[4]) for G in dd.MATRIX.values() if len(G[4]) == 2 and max(G[4]) <= 16}
    assert {t for t in default if ld.inhibition('f', 1, 1, 32, 32, *t).staging == 'batched'} == {(31, 31)}
    assert (17, 17) not in default
    # the attribute arm: float32 from 79 taps, float64 from 41; float64 runs up to 91 taps, float32 is never refused
    assert not square('f', 77).attr and square('f', 79).attr and not square('d', 39).attr and square('d', 41).attr
    assert square('d', 91).error is None and square('d', 91).lds == 160064 and square('d', 93).error == 'E_UNSUPPORTED'
    assert square('f', 127).error is None and square('f', 127).lds == 126400
    assert ld.inhibition('f', 1, 1, 32, 32, 129, 3).why == 'kMaxTaps' and ld.inhibition('f', 1, 1, 32, 32, 4, 3).why == 'odd'
    assert ld.inhibition('f', 1, 1, 1 << 15, 1 << 14, 3, 3).why == 'plane'
    assert ld.inhibition('d', 1 << 22, 1, 1024, 1024, 3, 3).why == 'blocks'


def test_modes_of_known_shapes():
    ax = ld.mode_axis
    assert ax(20, 12, 'full') == ld.Axis(9, 11, 'full_long', None)              # a 12-tap atom on a 20-pixel axis runs
    assert ax(9, 9, 'full') == ld.Axis(1, 8, 'full_S1', None) and ax(8, 9, 'full').error == 'E_GEOM'
    assert ax(10, 10, 'circular').dup == 'circ_all_but_one' and ax(6, 7, 'circular').dup == 'circ_all'
    assert ax(6, 8, 'circular').error == 'E_GEOM'
    assert ax(10, 10, 'reflect').dup == 'refl_max' and ax(10, 11, 'reflect').error == 'E_GEOM'
    assert all(ax(9, 1, m).dup == 'l0' for m in ld.MODES[1:])
    assert ld.mode_axes((2, 1, (14,), 3, (14,)), 'circular') == (ld.Axis(1, 0, 'row', None), ld.Axis(14, 13, 'circ_all_but_one', None))


def test_routes_of_known_cases():
    """The families without an epilogue for the extra term fall back; the first call grows the work buffer only where the
    gradients do not fit the first MiB; the split kernel's epilogue wants rows of whole 32-element tiles."""
    plan = lambda cid, *a: ld.plan(ld.MATRIX[cid], *a)  # noqa: E731
    assert (plan('rt_13x9-f').route, plan('rt_13x9-f').family) == ('epilogue', 'generic')
    p = plan('route_mfma-f')
    assert (p.route, p.family, p.regrow, p.hw_bytes) == ('fallback', 'mfma', False, 1 << 20)
    p = plan('route_mfma_regrow-f')
    assert (p.route, p.regrow, p.hw_bytes) == ('fallback', True, 3 << 20)
    assert not ld.plan(ld.MATRIX['route_mfma_regrow-f'], None, 'both', p.hw_bytes).regrow
    p = plan('route_fft_regrow-d')
    assert (p.route, p.family, p.regrow) == ('fallback', 'fft', True)
    assert plan('route_mfma_padded-f').copied and plan('route_mfma_padded-f').family == 'mfma'
    assert (plan('route_split_padded-f').route, plan('route_split_padded-f').family) == ('epilogue', 'split')
    assert plan('route_split_padded-f').inh.inst == ('f', 23, 23)
    assert (plan('route_split_contig-f').route, plan('route_split_contig-f').family) == ('fallback', 'split')
    # one sample of the same problem is below the split kernel's 2^16 activations
    assert (plan('route_split_padded-f', 1).route, plan('route_split_padded-f', 1).family) == ('epilogue', 'generic')
    assert (plan('route_split_contig-f', 1).route, plan('route_split_contig-f', 1).family) == ('fallback', 'mfma')
    p = plan('m_full_long-d')
    assert (p.route, p.family, p.axes[0].dup, p.inh.tiles_y, p.inh.blocks) == ('modes', 'generic', 'full_long', 1, 2)
    assert plan('m_refl_refused-f').error == plan('m_circ_refused-d').error == 'E_GEOM'
    assert plan('lds_93_refused-d').error == 'E_UNSUPPORTED' and plan('lds_93_refused-d', None, 'none').route == 'plain'
    # one atom: the cross term is dropped
    assert 'M_1_cross_dropped' in plan('rt_tiny_m1-d').edges and 'both_terms' not in plan('rt_tiny_m1-d').edges


# ----------------------------------------------------------------------------------------------------------------------
# the matrix
# ----------------------------------------------------------------------------------------------------------------------
def test_matrix_reaches_every_instance_edge_route_and_refusal():
    got = ld.reached(ld.MATRIX)
    assert not ld.missing(ld.MATRIX), ld.missing(ld.MATRIX)
    for inst in ld.all_inhibition_instances():
        assert ('k_inhibition',) + inst in got, inst
    for T in dd.DTYPES:
        for k in ('k_mu_update_extra', 'k_fold_update', 'k_pad_H', 'k_fold_H', 'k_convolve_axis'):
            assert (k, T) in got, (k, T)
        assert set(ld.ROUTE_EDGES) <= set(got[('k_inhibition', T, 0, 0)])
    # the list, for the reader of a failure: every required cell with the cases that carry it
    for key, edge in sorted(ld.required(), key=str):
        if key not in ld.NOT_COVERED:
            assert got[key][edge], (key, edge)
    assert not ld.UNREACHABLE
    assert set(ld.NOT_COVERED) == {('refusal', 'plane'), ('refusal', 'blocks')}
    assert all(k not in got for k in ld.NOT_COVERED)


def test_a_case_taken_out_is_named_by_the_cells_it_alone_carried():
    sole = ld.sole_carriers(ld.MATRIX)
    assert sole, 'no sole carriers: the check below would be vacuous'
    for cid, cells in sole.items():
        rest = {c: v for c, v in ld.MATRIX.items() if c != cid}
        lost = ld.missing(rest)
        for cell in cells:
            if cell[0] not in ld.NOT_COVERED:
                assert cell in lost, (cid, cell)
    # and whole families of cases: no float64 LDS cases -> the float64 attribute arm is named, and so on
    rest = {c: v for c, v in ld.MATRIX.items() if not c.startswith('m_full_long')}
    assert (('k_fold_update', 'd'), 'full_long') not in ld.missing(rest)      # (the 1-D case carries the class too)
    rest = {c: v for c, v in rest.items() if not c.startswith('m1_full_long')}
    assert {(('k_fold_update', 'd'), 'full_long'), (('k_fold_update', 'f'), 'full_long')} <= set(ld.missing(rest))


def test_matrix_cases_are_what_the_issue_asks_for():
    M = ld.MATRIX
    # asymmetric kernels of different lengths per axis, unless the case is there for a compile-time instance
    for cid, case in M.items():
        p = ld.plan(case)
        if case.kernels == 'random' and len(case.taps) == 2 and p.inh is not None and p.inh.inst[1:] == (0, 0):
            assert case.taps[0] != case.taps[1] or cid.startswith(('rt_29', 'lds_')), cid
        if case.layout == 'padded':
            assert case.mode == 'valid' and len(case.geometry[4]) == 2
    # the parabolic kernels once per instance, at the reference's own shapes (range = atom size - 1)
    para = {ld.plan(c).inh.inst for c in M.values() if c.kernels == 'parabolic'}
    assert para == ld.all_inhibition_instances()
    for c in M.values():
        if c.kernels == 'parabolic':
            assert c.taps == tuple(2 * (a - 1) + 1 for a in c.geometry[4])
    # one case per route at the project's usual strengths
    usual = {(ld.plan(c).route, ld.plan(c).family) for c in M.values() if c.strengths == ld.USUAL}
    assert usual == {('epilogue', 'generic'), ('epilogue', 'split'), ('fallback', 'mfma'), ('fallback', 'fft'),
                     ('modes', 'generic')}
    # the longest kernels that run, the first that is refused, the full mode with an atom longer than its activations
    assert ld.plan(M['lds_127-f']).inh.lds == 126400 and ld.plan(M['lds_91-d']).inh.attr
    assert ld.plan(M['lds_93_refused-d']).why == 'lds'
    _, _, D, _, A = M['m_full_long-f'].geometry
    assert A[0] - 1 > D[0] - A[0] + 1
    # skinny: the oracle's separable convolution is windows + tensordot
    for cid, case in M.items():
        n, _, _, m, _ = case.geometry
        g = dd.geo(case.geometry)
        assert n * m * g.Hy * g.Hx * max(case.taps) <= 1 << 24, cid
    assert len(M) == 100


def test_spots_sit_on_different_atoms():
    """The spot operands: neighbouring atoms carry different spots, every plane carries at least one."""
    for cid, case in ld.MATRIX.items():
        N, _, D, M, A = case.geometry
        spots = dd.corner_spots(tuple(d + a - 1 for d, a in zip(D, A)))
        for n in range(N):
            for m in range(M):
                mine = {j for j in range(len(spots)) if (n + m + j) % 2 == 0}
                assert mine, cid
                if m + 1 < M:
                    assert not mine & {j for j in range(len(spots)) if (n + m + 1 + j) % 2 == 0}, cid
