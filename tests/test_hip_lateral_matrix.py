"""
The H half step in full, every instance of it: k_inhibition in its eight instances and both staging
forms, k_mu_update_extra, k_fold_update, k_pad_H / k_fold_H and the front end's fall-back onto k_convolve_axis.  Each case
of lateral_dispatch.MATRIX is chosen with the host mirror of update_H_2d so that together they reach every instance, every
edge of the tile grid, the LDS arm above 64 KiB on both sides of its boundaries, every refusal and every route
(tests/test_lateral_dispatch_cpu.py checks that without a GPU).  On each, one fused H step is held against
OracleNMF.update_H (float64, C flavour) with the case's own inhibition kernels -- asymmetric ones, of different lengths per
axis, so that a flipped or transposed tap table shows -- at the project's bars for a fused step: 2 * 2e-5 (float32) /
2 * 1e-10 (float64) of the output's maximum, twice that for a chained second step, once for a primitive.  Both terms,
inhibition alone and cross-atom inhibition alone run on the same operands: random ones, and single large activations at
the corners and the centre of each plane on a small floor, where the footprint of a spot in the lateral term is the kernel
itself.  Strengths are chosen (on the oracle, lateral_dispatch.MATRIX) so that the lateral term is at least 0.9 of every
denominator: an error in it shows in H at full size.  After every call the family that ran is the one the mirror names,
the pad columns of row-padded activations are still zeros, and a refused call has the mirror's error code and left H
bit-identical.
"""
import zlib

import numpy as np
import pytest
import torch

import direct_dispatch as dd
import lateral_dispatch as ld
from oracle import tnmf_oracle as orc
from test_hip_direct_matrix import padded, slices_of
from test_hip_parity import dev, relmax
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF
from tnmf_amd.backends.HIP import HIP_Backend

pytestmark = pytest.mark.gpu

TOL = {'f': 2e-5, 'd': 1e-10}
NP = {'f': np.float32, 'd': np.float64}
EPS = 1e-9
SPARSITY = 0.05            # of the cases at the project's usual strengths; lateral-dominated cases run without
MIN_SHARE = 0.9            # of the lateral term in every denominator of a lateral-dominated case
E_CODE = {'E_UNSUPPORTED': _lib.E_UNSUPPORTED, 'E_GEOM': -2}
SPOT, FLOOR = 1.0, 0.01

CASES = list(ld.MATRIX)


def f32(x):
    """float64 image of float32 values: the oracle sees exactly what the kernels see."""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def kernels_of(cid):
    """The case's inhibition kernels, one per shift axis.  'random': positive taps in [0.25, 1.25) with a centre tap in
    [1.5, 2.5) (so that G - H stays non-negative, as with the reference's kernels, whose centre tap is one), no symmetry.
    'parabolic': the reference's own (TransformInvariantNMF.py:163)."""
    case = ld.MATRIX[cid]
    if case.kernels == 'parabolic':
        return orc.inhibition_kernels(tuple((t - 1) // 2 for t in case.taps))
    rng = np.random.default_rng(zlib.crc32(('taps-' + cid.rsplit('-', 1)[0]).encode()))
    out = []
    for t in case.taps:
        k = 0.25 + rng.random(t)
        k[(t - 1) // 2] = 1.5 + rng.random()
        out.append(f32(k))
    return tuple(out)


def operands(cid):
    """(V, W, {'random': H, 'spots': H}) of a case, the same for both dtypes.  'spots': single activations of SPOT at the
    corners and the centre of each plane (plane (n, m) carries spot j when n + m + j is even: neighbouring atoms sit at
    different spots) on a floor of about FLOOR."""
    case = ld.MATRIX[cid]
    N, C, D, M, A = case.geometry
    k = len(A)
    rng = np.random.default_rng(zlib.crc32(cid.rsplit('-', 1)[0].encode()))
    V = rng.random((N, C) + D)
    Wn = rng.random((M, C) + A)
    Wn /= Wn.sum(axis=tuple(range(-k, 0)), keepdims=True)
    Hs = orc.transform_shape(D, A, case.mode)
    Hr = rng.random((N, M) + Hs)
    Hsp = FLOOR * (0.5 + 0.5 * rng.random((N, M) + Hs))
    for n in range(N):
        for m in range(M):
            for j, spot in enumerate(dd.corner_spots(Hs)):
                if (n + m + j) % 2 == 0:
                    Hsp[(n, m) + spot] = SPOT
    return f32(V), f32(Wn), {'random': f32(Hr), 'spots': f32(Hsp)}


def strengths_of(case, terms):
    inh, cross = case.strengths
    return {'both': (inh, cross), 'inh': (inh, 0.), 'cross': (0., cross), 'none': (0., 0.)}[terms]


def sparsity_of(case):
    return SPARSITY if case.strengths == ld.USUAL else 0.


class Oracle:
    """OracleNMF on the case's operands and kernels."""

    def __init__(self, cid):
        orc.set_threads(orc.default_threads(cap=16))
        self.cid, self.case = cid, ld.MATRIX[cid]
        self.kernels = kernels_of(cid)
        self.V, self.W, self.H = operands(cid)
        self.M, self.A = self.case.geometry[3], self.case.geometry[4]

    def step(self, H, s, terms, steps=1):
        """H after `steps` calls of OracleNMF.update_H on the samples s.  One atom: the reference would divide the cross
        term by M - 1 = 0; the library drops it (api.hip:913), and so does this."""
        ref = orc.OracleNMF(n_atoms=self.M, atom_shape=self.A, impl='c', reconstruction_mode=self.case.mode)
        ref._kernels = self.kernels
        ref.V, ref.W, ref.H = self.V, self.W, H.copy()
        inh, cross = strengths_of(self.case, terms)
        out = []
        for _ in range(steps):
            ref.update_H(s, sparsity=sparsity_of(self.case), inhibition=inh, cross_inhibition=cross if self.M > 1 else 0.)
            out.append(ref.H.copy())
        return out if steps > 1 else out[0]

    def share(self, H, terms):
        """Smallest share of the lateral term in a denominator of the whole-batch step."""
        inh, cross = strengths_of(self.case, terms)
        k = len(self.A)
        _, pos = orc.gradient_H(self.V, self.W, H, slice(None), 'c', self.case.mode)
        g = orc.convolve_multi_1d(H, self.kernels, range(-k, 0))
        lat = inh * (g - H)
        if cross > 0 and self.M > 1:
            lat = lat + (cross / (self.M - 1)) * (g.sum(axis=1, keepdims=True) - g)
        return float((lat / (pos + lat + EPS + sparsity_of(self.case))).min())


def check(name, got, want, tol):
    err = relmax(got, want)
    print(f'    {name}: {err:.2e} (bar {tol:.1e})')
    assert err < tol, (name, err, tol)


def describe(p):
    if p.route == 'refused':
        return f'refused {p.error} ({p.why})'
    i = p.inh
    inh = 'no lateral term' if i is None else (f'k_inhibition<{i.inst[0]}, {i.inst[1]}, {i.inst[2]}> {i.staging} npre={i.npre} '
                                               f'lds={i.lds}{" (attribute arm)" if i.attr else ""} blocks={i.blocks}')
    return f'{inh}; route {p.route}{" (regrow, E twice)" if p.regrow else ""} on {p.family}{" (contiguous copy)" if p.copied else ""}'


@pytest.mark.parametrize('cid', CASES)
def test_lateral_case_against_oracle(cid):
    case = ld.MATRIX[cid]
    N, C, D, M, A = case.geometry
    T, dt, k = case.dtype, NP[case.dtype], len(case.geometry[4])
    ref = Oracle(cid)
    kernels, V, Wn = ref.kernels, ref.V, ref.W
    be = HIP_Backend(path=case.path, reconstruction_mode=case.mode)
    np.random.seed(1)
    be.initialize(V.astype(dt), tuple(A), M, None, tuple(range(-k, 0)))
    W = dev(Wn, dt)
    Hx = ref.H['random'].shape[-1]
    hw = [0]
    dominated = case.strengths != ld.USUAL
    print(f'{cid}: {case}')

    def device_H(Hn):
        return padded(dev(Hn, dt)) if case.layout == 'padded' else dev(Hn, dt)

    def pads_are_zero(H):
        if case.layout == 'padded':
            assert not H._base[..., Hx:].any(), 'pad columns written'

    def run(H, s, terms):
        inh, cross = strengths_of(case, terms)
        be.fused_update_H(V, W, H, s, sparsity=sparsity_of(case), eps=EPS, inhibition=inh, cross_inhibition=cross,
                          inhibition_kernels=kernels)

    def planned(s, terms):
        p = ld.plan(case, len(range(N)[s]), terms, hw[0])
        hw[0] = p.hw_bytes
        return p

    # ---- refused cases: the mirror's error code, H bit-identical; the unfused primitives of a refused mode refuse too
    if ld.plan(case).route == 'refused':
        p = ld.plan(case)
        print(f'  {describe(p)}')
        for kind, Hn in ref.H.items():
            for s in slices_of(N):
                for terms in ('both', 'inh', 'cross'):
                    H = device_H(Hn)
                    before = H.clone()
                    with pytest.raises((NotImplementedError, _lib.TnmfHipError)) as exc:
                        run(H, s, terms)
                    err = exc.value.__cause__ if isinstance(exc.value, NotImplementedError) else exc.value
                    assert isinstance(err, _lib.TnmfHipError) and err.code == E_CODE[planned(s, terms).error], (err, p.error)
                    # (TNMF_E_UNSUPPORTED with lateral terms reaches the front end as NotImplementedError: its fall-back)
                    assert isinstance(exc.value, NotImplementedError) == (p.error == 'E_UNSUPPORTED')
                    assert torch.equal(H, before), 'a refused in-place update wrote H'
                    pads_are_zero(H)
        if p.why == 'pad':
            H = dev(ref.H['random'], dt)
            for call in (lambda: be.reconstruct(W, H), lambda: be.reconstruction_gradient_H(V, W, H)):
                with pytest.raises(_lib.TnmfHipError) as exc:
                    call()
                assert exc.value.code == E_CODE['E_GEOM']
        if p.why == 'lds':
            # the front end's fall-back: NotImplementedError -> the reference's own lines on the backend's primitives
            # (k_convolve_axis for the separable convolution), with the same asymmetric kernels
            nmf = TransformInvariantNMF(n_atoms=M, atom_shape=tuple(A), backend=be)
            nmf._inhibition_kernels_1D = kernels
            for kind, Hn in ref.H.items():
                for terms in ('both', 'inh', 'cross'):
                    inh, cross = strengths_of(case, terms)
                    nmf._V, nmf._W, nmf._H = V.astype(dt), W, device_H(Hn)
                    nmf._update_H(slice(None), sparsity=sparsity_of(case), inhibition=inh, cross_inhibition=cross)
                    assert be.last_path == ld.family(case.geometry, T, case.path, 'grad_H', False)
                    check(f'fall-back step, {kind} operands, {terms}', be.to_ndarray(nmf._H), ref.step(Hn, slice(None), terms),
                          2 * TOL[T])
        del be
        return

    # ---- two consecutive whole-batch steps on the fresh backend: the fall-back's first call may have to grow the work
    # buffer and compute E a second time, the second call never
    Hn = ref.H['random']
    want = ref.step(Hn, slice(None), 'both', steps=2)
    H = device_H(Hn)
    for i in range(2):
        p = planned(slice(None), 'both')
        print(f'  step {i + 1}: {describe(p)}')
        run(H, slice(None), 'both')
        assert be.last_path == p.family, (p.family, be.last_path)
        check(f'H after step {i + 1}', be.to_ndarray(H), want[i], (2 << i) * TOL[T])
        pads_are_zero(H)

    # ---- both terms, inhibition alone, cross inhibition alone (modes: and none): random and spot operands, the whole
    # batch, the last sample and an interior one
    for kind, Hn in ref.H.items():
        for terms in ('both', 'inh', 'cross') + (('none',) if case.mode != 'valid' else ()):
            inh, cross = strengths_of(case, terms)
            dropped = terms == 'none' or (terms == 'cross' and M == 1)
            if dominated and not dropped:
                share = ref.share(Hn, terms)
                print(f'  {kind} operands, {terms}: lateral share of the denominator >= {share:.3f}')
                assert share >= MIN_SHARE, (kind, terms, share)
            for s in slices_of(N):
                p = planned(s, terms)
                H = device_H(Hn)
                before = H.clone()
                run(H, s, terms)
                assert be.last_path == p.family, (p.family, be.last_path)
                print(f'  {kind} operands, {terms}, samples {s}: {describe(p)}')
                got = be.to_ndarray(H)
                check('H step', got[s], ref.step(Hn, s, terms)[s], 2 * TOL[T])
                rest = torch.ones(N, dtype=torch.bool)
                rest[s] = False
                assert torch.equal(H[rest], before[rest]), 'samples outside the slice were written'
                pads_are_zero(H)
        if M == 1:
            # one atom: the cross term is dropped (the reference would divide by M - 1 = 0) -- the step with it is the
            # step without it, bit for bit
            Ha, Hb = device_H(Hn), device_H(Hn)
            run(Ha, slice(None), 'both')
            run(Hb, slice(None), 'inh')
            assert torch.equal(Ha, Hb)

    # ---- the separable convolution of the front end's fall-back (k_convolve_axis), with the same kernels
    if ld.convolves(case):
        for kind, Hn in ref.H.items():
            got = be.convolve_multi_1d(device_H(Hn), kernels, tuple(range(-k, 0)))
            check(f'convolve_multi_1d, {kind} operands', be.to_ndarray(got), orc.convolve_multi_1d(Hn, kernels, range(-k, 0)),
                  TOL[T])

    # ---- the modes' unfused primitives share the pad / fold kernels (k_pad_H, k_fold_H) and their guard
    if case.mode != 'valid':
        for kind, Hn in ref.H.items():
            H = dev(Hn, dt)
            check(f'R, {kind} operands', be.to_ndarray(be.reconstruct(W, H)), orc.reconstruct(Wn, Hn, 'c', case.mode), TOL[T])
            for s in slices_of(N):
                neg, pos = be.reconstruction_gradient_H(V, W, H, s)
                on, op = orc.gradient_H(V, Wn, Hn, s, 'c', case.mode)
                assert tuple(neg.shape) == on.shape
                check(f'neg_H, {kind} operands, samples {s}', be.to_ndarray(neg), on, TOL[T])
                check(f'pos_H, {kind} operands, samples {s}', be.to_ndarray(pos), op, TOL[T])
    del be
