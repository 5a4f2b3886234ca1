"""
CPU guard of the volume matrix: the host mirror of the three-shift-axis family (tests/volume_dispatch.py) is held to the
C++ it restates (volume.hip, modes.h, api.hip, read as text), its index maps of the reconstruction modes to the oracle's pad and
fold, and the cases of tests/test_hip_volume_matrix.py to reaching every cell at 256 and at 304 compute units.  No GPU, no
build.
"""
import itertools
import os
import re

import numpy as np

import schedule_dispatch as sd
import volume_dispatch as vd
from conftest import ROOT
from oracle import tnmf_oracle as orc

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')


def _flat(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r'\s+', ' ', f.read().replace('\\\n', ' '))


# ----------------------------------------------------------------------------------------------------------------------
# the mirror against the sources
# ----------------------------------------------------------------------------------------------------------------------
def test_mirrored_constants_and_rules_are_those_of_the_source():
    """The lines the mirror restates.  When one of them changes, tests/volume_dispatch.py and the matrix's cases have to be
    looked at again."""
    vol, api, gen = _flat('volume.hip'), _flat('api.hip'), _flat('generic.h')
    for line in (
            f'constexpr int kVolBlock = {vd.kVolBlock};',
            f'constexpr int kVolTaps = {vd.kVolTaps};',
            # ---- vol_corr_H_chunks
            'const long entries = (long)v.M * v.C * v.A[0] * v.A[1], rows = (long)v.N * v.D[0] * v.D[1];',
            f'long P = ({vd.WG_PER_CU}L * ctx->num_cu + entries - 1) / entries;',
            f'if (P > rows / {vd.ROWS_PER_CHUNK}) P = rows / {vd.ROWS_PER_CHUNK};',
            f'if (P > {vd.P_CAP}) P = {vd.P_CAP};',
            'return P < 1 ? 1 : (int)P;',
            # ---- k_vol_corr_H: the chunk, the tap blocks, the lanes, the waves
            'const int p = blockIdx.x % P, e = blockIdx.x / P;',
            'const long r0 = rows * p / P, r1 = rows * (p + 1) / P;',
            'for (int a0 = 0; a0 < v.A[2]; a0 += kVolTaps) {',
            'const int nt = v.A[2] - a0 < kVolTaps ? v.A[2] - a0 : kVolTaps;',
            'for (long r = r0 + wave; r < r1; r += kVolBlock / 64) {',
            'for (int x = lane; x < v.D[2]; x += 64) {',
            '* v.H[2] + v.A[2] - 1 - a0;',
            'const size_t o = ((size_t)mc * nzy + azy) * v.A[2] + a0 + t;',
            'for (int p = 0; p < P; ++p) {',
            # ---- the grids
            'const int tiles = cdiv(v.D[0] * v.D[1] * v.D[2], kVolBlock); const dim3 grid((unsigned)(tiles * v.N * v.C));',
            'const int tiles = cdiv(v.H[0] * v.H[1] * v.H[2], kVolBlock); const dim3 grid((unsigned)(tiles * v.N * v.M));',
            'const dim3 grid((unsigned)(entries * P));',
            'const int n = v.M * v.C * v.A[0] * v.A[1] * v.A[2];',
            'dim3(cdiv(n, kVolBlock)), dim3(kVolBlock), 0, s, n, P, partials,',
            'if (entries * P > 0x7fffffffL) return TNMF_E_GEOM;',
            # ---- vol_fits
            f'const long long lim = {hex(vd.LIM)}LL;',
            'const long long tiles = (hvox + kVolBlock - 1) / kVolBlock;',
            'return vox < lim && hvox < lim && avox * v.M * v.C < lim && tiles * v.N * (v.M > v.C ? v.M : v.C) < lim;',
            # ---- the reconstruction modes: the index maps and the guards are those of modes.h (below)
            'const int uz = pad_src(jz, q.S[0], q.A[0], mode), uy = pad_src(jy, q.S[1], q.A[1], mode), '
            'ux = pad_src(jx, q.S[2], q.A[2], mode);',
            'q.S[i] = mode_shift_len(mode, v.D[i], v.A[i]); if (!mode_axis_ok(mode, q.S[i], v.A[i])) return TNMF_E_GEOM;',
            'const int jz[2] = {uz + q.A[0] - 1, pad_dup(uz, q.S[0], q.A[0], mode)};',
            # ---- k_vol_lateral
            'if (xc != T(0)) for (int m = 0; m < M; ++m) S += G[o0 + (size_t)m * vox];',
            'G[o] = inh * (gv - H[o]) + xc * (S - gv);'):
        assert line in vol, line
    modes = _flat('modes.h')
    for line in (
            # ---- the per-axis rule of the modes, stated once: the index maps, the shift length, the limits
            'if (mode == TNMF_MODE_FULL) { const int u = j - l; return (u >= 0 && u < S) ? u : -1; }',
            'if (j >= l) return j - l; return mode == TNMF_MODE_CIRCULAR ? S - l + j : l - j;',
            'if (mode == TNMF_MODE_CIRCULAR) return u >= S - l ? u - (S - l) : -1;',
            'if (mode == TNMF_MODE_REFLECT) return (u >= 1 && u <= l) ? l - u : -1;',
            'return mode == TNMF_MODE_VALID ? D + a - 1 : (mode == TNMF_MODE_FULL ? D - a + 1 : D);',
            'return S >= 1 && (mode != TNMF_MODE_CIRCULAR || a - 1 <= S) && (mode != TNMF_MODE_REFLECT || a - 1 < S);'):
        assert modes.count(line) == 1, line
    for name in ('generic.hip', 'inhibit.hip', 'volume.hip', 'event_walk.h'):   # ... and nowhere else
        text = _flat(name)
        assert '#include "modes.h"' in text and not re.search(r'TNMF_MODE_(FULL|CIRCULAR|REFLECT)', text), name
    # the cap of the strided grids: pad / fold and the lateral terms
    assert vol.count(f'const size_t cap = (size_t)ctx->num_cu * {vd.GRID_PER_CU}; if (blocks > cap) blocks = cap;') == 2
    for line in (
            # ---- to_vol, in its order
            'if (!in) return TNMF_E_NULL; if (in->dtype != 0 && in->dtype != 1) return TNMF_E_DTYPE;',
            'if (v->N < 0 || v->M <= 0 || v->C <= 0) return TNMF_E_GEOM;',
            'if (v->D[i] <= 0 || v->A[i] <= 0) return TNMF_E_GEOM; v->H[i] = v->D[i] + v->A[i] - 1;',
            'if (in->h_row_stride > 0 && in->h_row_stride != v->H[2]) return TNMF_E_STRIDE;',
            # ---- vol_scratch
            'const size_t r_bytes = align_up((size_t)v.N * v.C * vol_vox(v) * esize(dtype), 256);',
            'const size_t e_bytes = align_up((size_t)(kEnergyPartials + 8) * sizeof(double), 256);',
            'const size_t p_bytes = align_up((size_t)chunks * v.M * v.C * vol_avox(v) * 2 * sizeof(double), 256);',
            'if (red) *red = reinterpret_cast<double *>(ws_at(ctx, r_bytes));',
            'if (part) *part = reinterpret_cast<double *>(ws_at(ctx, r_bytes + e_bytes));',
            # ---- the arms
            'if (!R && v.N > 0) { if (!H) return TNMF_E_NULL; void *Rs; CHECK(vol_scratch(ctx, v, dtype, &Rs, nullptr)); '
            'CHECK(vol_reconstruct(v, dtype, W, H, Rs, s)); R = Rs; }',
            'if (v.N > 0 && !r_is_valid) { if (!W) return TNMF_E_NULL; void *Rs = R_scratch ? const_cast<void *>(R_scratch) : Rws; '
            'CHECK(vol_reconstruct(v, dtype, W, H, Rs, s)); R = Rs; }',
            'if (!Rs) { if (r_is_valid) return TNMF_E_NULL; CHECK(vol_scratch(ctx, v, dtype, &Rs, nullptr)); } '
            'if (!r_is_valid) CHECK(vol_reconstruct(v, dtype, W, H_inout, Rs, s));',
            'if (is_vol(geom)) return vol_api_grad_W(ctx, geom, V, R_or_null, R_or_null != nullptr, W, H, neg, pos, stream);',
            # ---- vol_api_update_H_ex
            'if (!mode_known(mode)) return TNMF_E_UNSUPPORTED; if (v.N == 0) return TNMF_OK;',
            'if (inhibition < 0 || cross_inhibition < 0) return TNMF_E_GEOM;',
            'if (klen[i] < 1 || klen[i] > kMaxTaps || !(klen[i] & 1)) return TNMF_E_UNSUPPORTED;',
            'return cross_inhibition > 0 && M > 1 ? cross_inhibition / (M - 1) : 0.0;',
            'const double xc = cross_weight(cross_inhibition, v.M);',
            'if (mode == TNMF_MODE_VALID && !lateral) return vol_api_update_H(ctx, geom, V, W, H_inout, R_scratch, 0, eps, sparsity, stream);',
            'S[i] = mode_shift_len(mode, v.D[i], v.A[i]); if (S[i] < 1) return TNMF_E_GEOM;',
            'CHECK(vol_lateral(ctx, dtype, (size_t)v.N, v.M, svox, G0, H_inout, inhibition, xc, s));'):
        assert line in api, line
    ex = api[api.index('int vol_api_update_H_ex('):api.index('int vol_api_run_schedule(')]
    assert ex.index('return TNMF_E_UNSUPPORTED;') < ex.index('if (v.N == 0)') < ex.index('inhibition < 0') < ex.index('kMaxTaps') \
        < ex.index('S[i] < 1') < ex.index('ensure_hwork') < ex.index('vol_lateral(') < ex.index('vol_pad_fold(')
    assert f'constexpr int kEnergyPartials = {vd.kEnergyPartials};' in gen and f'constexpr int kMaxTaps = {vd.kMaxTaps};' in gen
    assert vd.WAVES == 4


def test_to_vol_refuses_in_the_library_s_order():
    G = vd.REFUSAL_GEOMETRY
    N, C, D, M, A = G
    assert vd.to_vol(G, null=True)[0] == 'E_NULL'
    assert vd.to_vol((-1, C, D, M, A), dtype=2)[0] == 'E_DTYPE'                       # the dtype before the geometry
    assert vd.to_vol((N, C, (0, 4, 5), M, A), h_row_stride=99)[0] == 'E_GEOM'         # the geometry before the stride
    assert vd.to_vol(G, h_row_stride=99)[0] == 'E_STRIDE'
    v = vd.vol(G)
    assert v.H == (4, 5, 7) and vd.to_vol(G, h_row_stride=7)[0] is None and vd.to_vol(G, h_row_stride=8)[0] == 'E_STRIDE'
    assert vd.to_vol(G, h_row_stride=6)[0] == 'E_STRIDE'                              # (shorter than a row: the same answer)
    assert vd.to_vol((0, C, D, M, A))[0] is None                                      # an empty slice is a geometry
    for name, err in vd.TO_VOL_REFUSALS.items():
        assert vd.refused_geometry(name)[3] == err, name


def test_vol_fits_at_its_four_boundaries():
    """The arithmetic of vol_fits, just below and just above each of its four products (mirror only: NOT_COVERED)."""
    lim = vd.LIM
    mk = lambda N, C, D, M, A: vd.Vol(N, M, C, D, A, tuple(d + a - 1 for d, a in zip(D, A)))  # noqa: E731
    # vox: 2^31 - 2 fits, 2^31 - 1 does not (one-voxel atoms: hvox == vox)
    assert vd.vol_fits(mk(1, 1, (1, 2, (lim - 1) // 2), 1, (1, 1, 1))) and (lim - 1) % 2 == 0
    assert not vd.vol_fits(mk(1, 1, (1, 1, lim), 1, (1, 1, 1)))
    # hvox alone: vox below the limit, hvox at it
    v = mk(1, 1, (1, 1, lim - 3), 1, (1, 1, 3))
    assert vd.prod(v.D) == lim - 3 and vd.prod(v.H) == lim - 1 and vd.vol_fits(v)
    v = mk(1, 1, (1, 1, lim - 2), 1, (1, 1, 3))
    assert vd.prod(v.D) == lim - 2 and vd.prod(v.H) == lim and not vd.vol_fits(v)
    # avox * M * C alone (2^31 - 1 is prime: the product meets it only through one factor)
    v = mk(1, 2, (1, 1, 1), 1, (1, 1, (lim - 1) // 2))
    assert vd.prod(v.A) * v.M * v.C == lim - 1 and vd.prod(v.H) < lim and vd.vol_fits(v)
    v = mk(1, 2, (1, 1, 1), 1, (1, 1, (lim - 1) // 2 + 1))
    assert vd.prod(v.A) * v.M * v.C == lim + 1 and vd.prod(v.H) < lim and not vd.vol_fits(v)
    assert vd.vol_fits(mk(0, 1, (1, 1, 1), lim - 1, (1, 1, 1))) and not vd.vol_fits(mk(0, 1, (1, 1, 1), lim, (1, 1, 1)))
    # tiles * N * max(M, C): hvox = 256 * 2^15 -> 2^15 tiles; N * max(M, C) = 2^16 gives 2^31, one sample fewer fits
    D = (1, 256, 1 << 15)
    assert not vd.vol_fits(mk(1 << 13, 2, D, 8, (1, 1, 1)))
    assert vd.vol_fits(mk((1 << 13) - 1, 2, D, 8, (1, 1, 1)))
    assert not vd.vol_fits(mk(1 << 13, 8, D, 2, (1, 1, 1)))                           # the larger of M and C
    assert vd.vol_fits(mk(1 << 13, 2, D, 7, (1, 1, 1)))
    for case in vd.MATRIX.values():
        assert vd.vol_fits(vd.vol(case.geometry))


# ----------------------------------------------------------------------------------------------------------------------
# the index maps of the reconstruction modes against the oracle
# ----------------------------------------------------------------------------------------------------------------------
def _inside(S, a, mode):
    return vd.pad_fold_guard((S + a - 1 if mode == 'full' else S,), (a,), mode) is None


def _d_of(S, a, mode):
    return S + a - 1 if mode == 'full' else S


def _mirror_pad(H, A, mode):
    """pad built from vol_pad_src alone, k axes."""
    k = len(A)
    S = H.shape[-k:]
    P = tuple(_d_of(s, a, mode) + a - 1 for s, a in zip(S, A))
    out = np.zeros(H.shape[:-k] + P)
    for j in itertools.product(*(range(p) for p in P)):
        u = tuple(vd.vol_pad_src(j[i], S[i], A[i], mode) for i in range(k))
        if min(u) >= 0:
            out[(Ellipsis,) + j] = H[(Ellipsis,) + u]
    return out


def _mirror_fold(Gp, S, A, mode):
    """fold built from the main position plus vol_pad_dup, k axes: the 2^k terms of k_vol_fold."""
    k = len(A)
    out = np.zeros(Gp.shape[:-k] + tuple(S))
    for u in itertools.product(*(range(s) for s in S)):
        pos = [(u[i] + A[i] - 1, vd.vol_pad_dup(u[i], S[i], A[i], mode)) for i in range(k)]
        for j in itertools.product(*pos):
            if min(j) >= 0:
                out[(Ellipsis,) + u] += Gp[(Ellipsis,) + j]
    return out


def test_index_maps_are_the_oracle_s_pad_and_fold():
    rng = np.random.default_rng(5)
    seen = set()
    for mode in ('full', 'circular', 'reflect'):
        for S in range(1, 7):
            for a in range(1, 8):
                if not _inside(S, a, mode):
                    continue
                seen.add(vd.axis_class(_d_of(S, a, mode), a, mode))
                H = rng.random((2, 1, S))
                Hp = orc.pad_activations(H, (a,), mode)
                assert np.array_equal(_mirror_pad(H, (a,), mode), Hp), (mode, S, a)
                Gp = rng.random(Hp.shape)
                assert np.allclose(_mirror_fold(Gp, (S,), (a,), mode), orc.fold_gradient(Gp, (S,), (a,), mode), rtol=1e-15,
                                   atol=0), (mode, S, a)
                # one step past a limit: refused
        assert _inside(3, 4, 'circular') and not _inside(3, 5, 'circular')
        assert _inside(3, 3, 'reflect') and not _inside(3, 4, 'reflect')
        assert _inside(1, 7, 'full')
    assert seen == {c for cs in vd.AXIS_CLASSES.values() for c in cs}
    # every limit, one step past it, per mode and length
    for S in range(1, 7):
        assert vd.pad_fold_guard((S,), (S + 1,), 'circular') is None and vd.pad_fold_guard((S,), (S + 2,), 'circular') == 'E_GEOM'
        assert vd.pad_fold_guard((S,), (S,), 'reflect') is None and vd.pad_fold_guard((S,), (S + 1,), 'reflect') == 'E_GEOM'
        assert vd.pad_fold_guard((S,), (S,), 'full') is None and vd.pad_fold_guard((S,), (S + 1,), 'full') == 'E_GEOM'
    # 3-D products, the axes at different states at once
    for mode, S, A in (('circular', (2, 3, 4), (3, 4, 5)), ('reflect', (3, 4, 5), (3, 4, 5)), ('full', (1, 2, 3), (4, 1, 2)),
                       ('circular', (5, 4, 3), (3, 4, 1)), ('reflect', (5, 4, 3), (3, 4, 1)), ('full', (5, 5, 2), (3, 1, 4))):
        H = rng.random((2, 2) + S)
        Hp = orc.pad_activations(H, A, mode)
        assert np.array_equal(_mirror_pad(H, A, mode), Hp), (mode, S, A)
        Gp = rng.random(Hp.shape)
        assert np.allclose(_mirror_fold(Gp, S, A, mode), orc.fold_gradient(Gp, S, A, mode), rtol=1e-14, atol=0), (mode, S, A)


# ----------------------------------------------------------------------------------------------------------------------
# the matrix
# ----------------------------------------------------------------------------------------------------------------------
def test_chunk_counts_tap_blocks_and_grids_of_known_cases():
    M = vd.MATRIX
    for cid, case in M.items():
        if case.kind != 'prim':
            continue
        v = vd.vol(case.geometry)
        for cu in vd.CUS:
            P = vd.vol_corr_H_chunks(v, cu)
            assert P == vd.chosen_P(case, cu), (cid, cu, P)
            b = vd.chunk_bounds(v, P)
            assert b[0][0] == 0 and b[-1][1] == vd.corr_H_rows(v) and all(x[1] == y[0] for x, y in zip(b, b[1:]))
            assert vd.grids(v, cu)['corr_H'] == vd.corr_H_entries(v) * P
            part = vd.vol_scratch(v, 'f', cu)['part'][1]
            assert part >= P * v.M * v.C * vd.prod(v.A) * 16
    assert [vd.tap_blocks(a) for a in (7, 8, 9, 16, 19)] == [[7], [8], [8, 1], [8, 8], [8, 8, 3]]
    assert [vd.lane_trips(d) for d in (20, 64, 65, 130)] == [(1, 20), (1, 64), (2, 1), (3, 2)]
    v = vd.vol(M['p_cap'].geometry)
    assert (vd.corr_H_entries(v), vd.corr_H_rows(v)) == (1, 8320) and 8320 // 8 > 1024 and 8320 % 1024 == 128
    assert sorted({r1 - r0 for r0, r1 in vd.chunk_bounds(v, 1024)}) == [8, 9]
    v = vd.vol(M['p_entries'].geometry)
    assert (vd.corr_H_entries(v), vd.corr_H_rows(v) // 8) == (600, 4)
    v = vd.vol(M['p_one'].geometry)
    assert vd.corr_H_entries(v) == 1344 > 4 * 304 and vd.corr_H_rows(v) // 8 == 2
    v = vd.vol(M['p_rows3'].geometry)
    assert vd.waves_with_rows(v, 1) == 3
    v = vd.vol(M['p_ragged'].geometry)
    assert vd.chunk_bounds(v, 3) == [(0, 8), (8, 17), (17, 26)]
    # the cases carrying `chunks_ragged` (the issue leaves the choice to the mirror)
    ragged = {cid for cu in vd.CUS for cid in vd.reached_by(M, cu)[('corr_H', 'chunks_ragged')]}
    assert ragged == {'p_cap', 'p_ragged'}
    # the strided grids: 16 planes of 62 x 60 x 61 (pad) and of 60^3 (fold) take two passes at either CU count
    v = vd.vol(M['pad_large'].geometry)
    assert v.N * v.M * vd.prod(v.H) == 3630720 and v.N * v.M * vd.prod(v.D) == 3456000
    for cu, per_pass in ((256, 2097152), (304, 2490368)):
        assert cu * vd.GRID_PER_CU * vd.kVolBlock == per_pass
        assert vd.strided_grid(3630720, cu) == (cu * 32, 2) and vd.strided_grid(3456000, cu) == (cu * 32, 2)
    assert vd.strided_grid(0, 256) == (0, 0) and vd.strided_grid(257, 256) == (2, 1)
    assert vd.grids(vd.vol(M['vox256'].geometry), 256)['reconstruct'] == 1
    assert vd.grids(vd.vol(M['vox257'].geometry), 256)['reconstruct'] == 2


def test_arms_of_the_entries():
    v, v0 = vd.vol(vd.REFUSAL_GEOMETRY), vd.vol((0,) + vd.REFUSAL_GEOMETRY[1:])
    assert vd.grad_W_arm(v, False, False) == ('library_scratch', ('k_vol_reconstruct', 'k_vol_corr_H', 'k_vol_corr_H_finalize'))
    assert vd.grad_W_arm(v, True, False)[0] == 'caller_scratch' and vd.grad_W_arm(v, True, True) == (
        'valid_R', ('k_vol_corr_H', 'k_vol_corr_H_finalize'))
    assert vd.grad_W_arm(v0, True, False) == ('empty', ('k_vol_corr_H', 'k_vol_corr_H_finalize'))
    assert vd.grad_H_arm(v, True)[1] == ('k_vol_corr_W',) and vd.grad_H_arm(v0, False) == ('empty', ())
    assert vd.update_H_arm(v, False, True)[0] == 'E_NULL' and vd.update_H_arm(v, True, True)[1] == ('k_vol_corr_W<fused>',)
    assert vd.cross_factor(3, 0.05) == 0.025 and vd.cross_factor(1, 0.05) == 0. and vd.cross_factor(2, 0.) == 0.
    ex = vd.update_H_ex_arm
    assert ex(v, 'valid')[1] == ('k_vol_reconstruct', 'k_vol_corr_W<fused>')
    assert ex(v, 'valid', 0.1)[1] == ('k_convolve_axis',) * 3 + ('k_vol_lateral', 'k_vol_reconstruct', 'k_vol_corr_W',
                                                                 'k_mu_update_extra')
    assert ex(v, 'circular')[1] == ('k_vol_pad', 'k_vol_reconstruct', 'k_vol_corr_W', 'k_vol_fold', 'k_vol_fold', 'k_mu_update_extra')
    assert ex(v, 'valid', mode_code=4)[0] == 'E_UNSUPPORTED' and ex(v0, 'valid', mode_code=4)[0] == 'E_UNSUPPORTED'
    assert ex(v0, 'valid', -1.)[0] is None and ex(v, 'valid', -1.)[0] == 'E_GEOM'      # an empty slice returns before the strengths
    assert ex(v, 'valid', 0., 0., (2, 2, 2))[0] is None                                # kernels are read only with a lateral term
    assert ex(v, 'valid', 0.1, 0., (3, 3, 2))[0] == 'E_UNSUPPORTED' and ex(v, 'valid', 0.1, 0., (129, 3, 3))[0] == 'E_UNSUPPORTED'
    assert ex(vd.vol((2, 1, (3, 4, 5), 2, (3, 4, 6))), 'full')[0] == 'E_GEOM'
    assert ex(vd.vol(vd.MATRIX['pad_circ_refused'].geometry), 'circular', 0.1) == ('E_GEOM', ('k_convolve_axis',) * 3 + ('k_vol_lateral',), 0.)
    sc = vd.vol_scratch(v, 'd', 256)
    assert 2 * 2 * 60 * 8 == 1920 and sc['R'] == (0, 2048) and sc['red'] == (2048, 16640) and sc['part'][0] == 18688      # whole 256 bytes


def test_matrix_reaches_every_cell_at_both_device_sizes():
    assert vd.missing() == []
    for cu in vd.CUS:
        got = vd.reached_by(vd.MATRIX, cu)
        for cell in sorted(vd.required()):
            assert got.get(cell), (cu, cell)
        assert all(k not in got for k in vd.NOT_COVERED) and all(k not in got for k in vd.UNREACHABLE)
    # a case chosen for a value of P carries that cell at both
    for cid, cell in (('p_cap', 'P_cap_1024'), ('p_entries', 'P_by_entries'), ('p_one', 'P_1_entries_gt_4cu'),
                      ('p_rows3', 'P_1_rows_lt_8'), ('t7', 'P_by_rows')):
        for cu in vd.CUS:
            assert ('corr_H', cell) in vd.reached(vd.MATRIX[cid], cu), (cid, cu)
    assert set(vd.NOT_COVERED) == {('refusal', 'vol_fits'), ('refusal', 'workspace')}
    assert set(vd.UNREACHABLE) == {('refusal', 'corr_H_grid')}
    assert all(len(why) > 40 and 'time' not in why for why in list(vd.NOT_COVERED.values()) + list(vd.UNREACHABLE.values()))
    assert len(vd.required()) == 102 and len(vd.MATRIX) == 31


def test_a_case_taken_out_is_named_by_the_cells_it_alone_carried():
    sole = vd.sole_carriers()
    assert len(sole) >= 15, 'few sole carriers: the check below would be nearly vacuous'
    for cid, cells in sole.items():
        rest = {c: v for c, v in vd.MATRIX.items() if c != cid}
        lost = vd.missing(rest)
        for cell in cells:
            assert cell in lost, (cid, cell)
    assert ('corr_H', 'taps_2_full_plus_ragged') in vd.missing({c: v for c, v in vd.MATRIX.items() if c != 't19_d65'})
    assert ('pad', 'grid_stride_fold') in vd.missing({c: v for c, v in vd.MATRIX.items() if c != 'pad_large'})
    # a cell reached at one device size only is missing
    only256 = dict(vd.MATRIX, p_entries=vd.prim((3, 2, (3, 3, 5), 5, (6, 10, 2)), {256: 2, 304: 3}))      # rows / 8 = 3
    assert vd.missing(only256) == [('corr_H', 'P_by_entries')]


# ----------------------------------------------------------------------------------------------------------------------
# what the older tests reached, counted with the mirror (DESIGN section 4g quotes the number)
# ----------------------------------------------------------------------------------------------------------------------
def _older_tests():
    P = lambda g, slices=False: vd.prim(g, None, slices)  # noqa: E731
    fit, lat, mb = (3, 2, (8, 9, 10), 3, (3, 2, 4)), (3, 2, (8, 9, 10), 3, (2, 3, 3)), (5, 1, (6, 7, 8), 2, (2, 2, 3))
    full, half, tap = (2, 1, (10, 4, 9), 3, (8, 4, 3)), (2, 1, (5, 6, 7), 2, (2, 2, 3)), (3, 2, (5, 6, 70), 3, (2, 3, 4))
    gold = (2, 2, (7, 8, 9), 3, (3, 2, 4))
    old = {
        # tests/test_hip_volumes.py
        'shape0': P((2, 1, (5, 6, 70), 3, (2, 3, 4)), True), 'shape1': P((3, 2, (4, 9, 7), 5, (3, 1, 2)), True),
        'shape2': P((1, 1, (3, 4, 5), 2, (3, 4, 5)), True), 'shape3': P((2, 3, (6, 5, 4), 4, (1, 1, 1)), True),
        'fit': P(fit), 'fit_lateral': P(lat), 'fit_f32': P((4, 1, (10, 12, 33), 4, (3, 3, 5))),
        'minibatch_2': P((2,) + mb[1:]), 'minibatch_1': P((1,) + mb[1:]), 'half_steps': P(half), 'full_mode': P(full),
        **{f'fit_{m}': vd.pad(fit, m) for m in vd.MODES[1:]}, 'half_steps_pad': vd.pad(half, 'circular'),
        'full_mode_pad': vd.pad(full, 'full'),
        **{f'fit_ex_{m}': vd.ex(fit, m, ('none',), 'parabolic') for m in vd.MODES},
        'fit_lateral_ex': vd.ex(lat, 'valid', ('both',), 'parabolic'), 'half_steps_ex': vd.ex(half, 'circular', ('both',), 'parabolic'),
        'full_mode_ex': vd.ex(full, 'full', ('both',), 'parabolic'),
        # tests/golden/*3d*.npz through test_hip_parity.py
        'golden_c1': P((2, 1, (7, 9, 11), 3, (2, 3, 4))), 'golden_c2': P((3, 2, (6, 8, 10), 4, (3, 2, 3))),
        'golden_c2_slice': P((2, 2, (6, 8, 10), 4, (3, 2, 3))), 'golden_modes': P(gold),
        **{f'golden_{m}': vd.pad(gold, m) for m in vd.MODES[1:]},
        # tests/schedule_dispatch.VOL: slices of 2, 8, 1, 4, 10, ... samples
        **{f'schedule_{n}': P((n,) + sd.VOL[1:], n == 10) for n in (1, 2, 3, 4, 5, 6, 8, 10)},
        # tests/test_hip_objective.py: the volume taps
        'tap': P(tap), 'tap_ex': vd.ex(tap, 'valid', ('none', 'both'), 'parabolic'), 'tap_circular': vd.ex(tap, 'circular', ('none',), 'parabolic'),
        'tap_pad': vd.pad(tap, 'circular'),
    }
    return old


def test_what_the_older_tests_reached():
    req = vd.required()
    hit = None
    for cu in vd.CUS:
        got = {c for c in vd.reached_by(_older_tests(), cu, backend_only=True) if c in req}
        hit = got if hit is None else hit & got
    assert len(hit) == OLDER_TESTS_REACHED, (len(hit), sorted(hit))
    # (P bounded by the entries was reached, but only inside a whole float32 fit held to 1e-5: 36 entries, 480 rows)
    assert vd.reached_by(_older_tests(), 256, backend_only=True)[('corr_H', 'P_by_entries')] == ['fit_f32']
    for cell in (('corr_H', 'taps_1_full_exact'), ('corr_H', 'taps_1_full_plus_1'), ('corr_H', 'taps_2_full_exact'),
                 ('corr_H', 'taps_2_full_plus_ragged'), ('corr_H', 'lanes_64'), ('corr_H', 'lanes_65'), ('corr_H', 'lanes_3_trips'),
                 ('corr_H', 'P_cap_1024'), ('corr_H', 'P_1_rows_lt_8'), ('corr_H', 'P_1_entries_gt_4cu'), ('corr_H', 'idle_waves'),
                 ('tiles', 'vox_256'), ('tiles', 'vox_257'), ('tiles', 'atom_longer_than_sample_on_two_axes'),
                 ('arm', 'grad_W', 'valid_R'), ('arm', 'grad_W', 'library_scratch'), ('arm', 'grad_H', 'R_given'),
                 ('pad', 'circ_all'), ('pad', 'refl_max'), ('pad', 'l0_next_to_padded'), ('pad', 'grid_stride_pad'), ('pad', 'adjoint'),
                 ('lateral', 'valid_inh_only'), ('lateral', 'circular_cross_only'), ('lateral', 'M_1_cross_dropped'),
                 ('lateral', 'random_kernels'), ('refusal', 'grad_W_stride_plus_1'), ('refusal', 'stride_equal_accepted')):
        assert cell not in hit, cell


OLDER_TESTS_REACHED = 25         # of the 102 required cells
