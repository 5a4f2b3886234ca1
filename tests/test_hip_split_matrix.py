"""
The split (3 x bf16) H-update kernel, every instance of it: each geometry of split_dispatch.MATRIX is chosen with the
host mirror of the dispatch so that together they reach all 48 k_split_corr_W<FUSED, MULTI, AY, NR4, EXTRA> instances and
every edge of every MFMA form (tests/test_split_dispatch_cpu.py checks that without a GPU).  On each, path='split' is
held against the float64 oracle at the bars of test_split_h_update_on_adversarial_operands -- never worse than twice the
error of the exact f32 chain (path='mfma'; 'generic' for 1-D signals) plus 2^-22, against the output's maximum and element
by element -- in the unfused gradient, the fused update on C-contiguous and on row-padded activations, and the fused
update with lateral and cross-atom inhibition (the EXTRA epilogue on 2-D problems, its refusal and the fallback on 1-D
ones), on the whole batch and on a mini-batch slice.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import split_dispatch as sd
from oracle import tnmf_oracle as orc
from test_hip_parity import _adversarial_case, _row_padded, dev, make_backend, relmax

pytestmark = pytest.mark.gpu

SPARSITY, EPS = 0.05, 1e-9
INHIBITION, CROSS_INHIBITION = 0.1, 0.05

CASES = [(gid, ops) for gid, g in sd.MATRIX.items() for ops in (('random',) if sd.one_d(g) else ('random', 'wide_V'))]


def _operands(gid, ops):
    """(V, W, H) as float64 images of float32 values: the oracle sees exactly what the kernels see."""
    N, C, D, M, A = geometry = sd.MATRIX[gid]
    if ops == 'wide_V':
        V, Wn, Hn = _adversarial_case('wide_V', geometry)[5:]
    else:
        rng = np.random.default_rng(zlib.crc32(gid.encode()))
        V = rng.random((N, C) + D)
        Wn = rng.random((M, C) + A)
        Wn /= Wn.sum(axis=tuple(range(-len(A), 0)), keepdims=True)
        Hn = rng.random((N, M) + tuple(d + a - 1 for d, a in zip(D, A)))
    return tuple(np.asarray(x, dtype=np.float32).astype(np.float64) for x in (V, Wn, Hn))


def _elementwise(got, want):
    want = np.asarray(want, dtype=np.float64)
    floor = 1e-12 * np.abs(want).max() + 1e-37        # (below ~1e-37 float32 itself has no bits left)
    return (np.abs(np.asarray(got, dtype=np.float64) - want) / (np.abs(want) + floor)).max()


def _lateral_oracle(V, Wn, Hn, A, impl, s):
    """H after OracleNMF.update_H on the samples s, with lateral and cross-atom inhibition."""
    ref = orc.OracleNMF(n_atoms=Wn.shape[0], atom_shape=A, impl=impl)   # default inhibition range: atom size - 1
    ref.V, ref.W, ref.H = V, Wn, Hn.copy()
    ref.update_H(s, sparsity=SPARSITY, inhibition=INHIBITION, cross_inhibition=CROSS_INHIBITION)
    return ref.H


def _lateral_on_R(V, Wn, Hn, R, A, impl, s):
    """The same half step in float64 on a given reconstruction R of H[s] -- the one the library computed for itself:
    measured against it, a kernel family is not charged with the rounding of the reconstruction that runs in front of it
    (the row-padded activations of the split kernel's EXTRA epilogue are reconstructed by the generic kernels, the
    contiguous copy the f32 MFMA family takes by its own MFMA kernels)."""
    k, M = len(A), Wn.shape[0]
    on = orc._correlate_with_W(Wn, V[s], impl)
    op = orc._correlate_with_W(Wn, R, impl)
    g = orc.convolve_multi_1d(Hn[s], orc.inhibition_kernels(tuple(a - 1 for a in A)), range(-k, 0))
    E = INHIBITION * (g - Hn[s]) + CROSS_INHIBITION / (M - 1) * (g.sum(axis=1, keepdims=True) - g)
    H = Hn.copy()
    H[s] = Hn[s] * on / (op + E + EPS + SPARSITY)
    return H


@pytest.mark.parametrize('gid,ops', CASES, ids=[f'{g}-{o}' for g, o in CASES])
def test_split_kernel_cell_against_oracle(gid, ops):
    """One geometry of the matrix: gradient, fused update (contiguous and row-padded) and fused update with lateral terms
    on path='split' against the float64 oracle and against the exact f32 family; random operands everywhere, eight
    decades of dynamic range in V (the wide_V operands of the adversarial test) on 2-D geometries."""
    from tnmf_amd import _lib
    orc.set_threads(orc.default_threads(cap=64))
    N, C, D, M, A = geometry = sd.MATRIX[gid]
    k = len(A)
    two_d = k == 2
    impl = 'c' if two_d else 'contract'
    exact = 'mfma' if two_d else 'generic'
    Hx = D[-1] + A[-1] - 1
    # the tile loop with a partial last round runs on this device as it does on the 256 CUs the geometry was chosen for
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for kind in sd.KINDS:
        if sd.cell(geometry, kind).tile_loop_partial:
            c = sd.cell(geometry, kind, num_cu)
            assert c.tiles > c.P, (gid, kind, num_cu, c)

    V, Wn, Hn = _operands(gid, ops)
    R = orc.reconstruct(Wn, Hn, impl)
    R32 = np.asarray(R, dtype=np.float32).astype(np.float64)
    on, pos_full = orc.gradient_H(V, Wn, Hn, slice(None), impl)
    op = orc._correlate_with_W(Wn, R32, impl)                  # pos of the R the kernels are given
    want_H = Hn * on / (pos_full + EPS + SPARSITY)
    want_HR = Hn * on / (op + EPS + SPARSITY)
    kernels = orc.inhibition_kernels(tuple(a - 1 for a in A))
    want_L = _lateral_oracle(V, Wn, Hn, A, impl, slice(None))
    want_Ls = _lateral_oracle(V, Wn, Hn, A, impl, slice(1, N))

    err, lat = {}, {}
    for path in ('split', exact):
        be = make_backend(V.astype(np.float32), A, M, path)
        W, H = dev(Wn, np.float32), dev(Hn, np.float32)
        neg, pos = torch.empty_like(H), torch.empty_like(H)
        # the V and R correlations alone: grad_H with the oracle's R
        Rd = dev(R32, np.float32)
        g = be._geom(N, M)
        _lib.check(be._lib.tnmf_hip_grad_H(be._ctx, ctypes.byref(g), ctypes.c_void_p(be._V_dev.data_ptr()),
                                           ctypes.c_void_p(Rd.data_ptr()), ctypes.c_void_p(W.data_ptr()),
                                           ctypes.c_void_p(H.data_ptr()), ctypes.c_void_p(neg.data_ptr()),
                                           ctypes.c_void_p(pos.data_ptr()), be._stream()), 'tnmf_hip_grad_H')
        assert be.last_path == path
        e = dict(neg_max=relmax(be.to_ndarray(neg), on), neg_el=_elementwise(be.to_ndarray(neg), on),
                 pos_max=relmax(be.to_ndarray(pos), op), pos_el=_elementwise(be.to_ndarray(pos), op))

        # fused update on C-contiguous activations, the library's own reconstruction in front of it
        Hc = dev(Hn, np.float32)
        be.fused_update_H(V, W, Hc, slice(None), sparsity=SPARSITY, eps=EPS)
        assert be.last_path == path
        e.update(H_max=relmax(be.to_ndarray(Hc), want_H), H_el=_elementwise(be.to_ndarray(Hc), want_H))

        # the fused kernel alone, on the oracle's R (r_is_valid): C-contiguous, and for the split kernel on 2-D problems
        # also row-padded (what initialize() allocates under the default dispatch) -- the same bits, and the pad columns
        # stay exact zeros (k_inhibition reads them as zero pixels)
        def update_on_R(Ht, ld):
            g = be._geom(N, M, ld)
            _lib.check(be._lib.tnmf_hip_update_H(be._ctx, ctypes.byref(g), ctypes.c_void_p(be._V_dev.data_ptr()),
                                                 ctypes.c_void_p(W.data_ptr()), ctypes.c_void_p(Ht.data_ptr()),
                                                 ctypes.c_void_p(Rd.data_ptr()), 1, EPS, SPARSITY, be._stream()),
                       'tnmf_hip_update_H')
            assert be.last_path == path

        HcR = dev(Hn, np.float32)
        update_on_R(HcR, 0)
        e.update(HR_max=relmax(be.to_ndarray(HcR), want_HR), HR_el=_elementwise(be.to_ndarray(HcR), want_HR))
        if two_d and path == 'split':
            HpR = _row_padded(dev(Hn, np.float32))
            update_on_R(HpR, HpR.stride(2))
            assert torch.equal(HpR, HcR), (HpR - HcR).abs().max().item()
            assert not HpR._base[..., Hx:].any()

        # fused update with lateral and cross-atom inhibition on row-padded activations (2-D split: the EXTRA epilogue;
        # 1-D: refused, the fallback), on the whole batch and on the samples of a mini-batch behind the first: against
        # the oracle's half step (L, Ls) and against the same on the library's own reconstruction (LR, LRs)
        for key, s, want in (('L', slice(None), want_L), ('Ls', slice(1, N), want_Ls)):
            HL = _row_padded(dev(Hn, np.float32)) if two_d else dev(Hn, np.float32)
            R_lib = be.to_ndarray(be.reconstruct(W, HL[s])).astype(np.float64)
            want_R = _lateral_on_R(V, Wn, Hn, R_lib, A, impl, s)
            be.fused_update_H(V, W, HL, s, sparsity=SPARSITY, eps=EPS, inhibition=INHIBITION,
                              cross_inhibition=CROSS_INHIBITION, inhibition_kernels=kernels)
            assert be.last_path == path
            got = be.to_ndarray(HL)
            if s.start:
                assert np.array_equal(got[:s.start], Hn[:s.start].astype(np.float32)), 'samples outside the slice changed'
            if two_d:
                assert not HL._base[..., Hx:].any()
            lat[path + key] = relmax(got, want)
            kr = key.replace('L', 'LR')
            e.update({kr + '_max': relmax(got, want_R), kr + '_el': _elementwise(got, want_R)})
        err[path] = e
        del be
    print(gid, ops, {p: {q: f'{v:.2e}' for q, v in e.items()} for p, e in err.items()}, {q: f'{v:.2e}' for q, v in lat.items()})
    for key in err['split']:
        assert err['split'][key] <= 2 * err[exact][key] + 2.0 ** -22, (key, err)
    assert err['split']['neg_max'] < 2e-6 and err['split']['pos_max'] < 2e-6
    for key in ('H_max', 'HR_max', 'LR_max', 'LRs_max'):
        assert err['split'][key] < 2e-5, (key, err)
    assert max(lat.values()) < 2e-5, lat
