"""
The direct kernels, every instance of them: the float32 MFMA kernels of mfma.hip (k_mfma_reconstruct, k_mfma_corr_W and its
persistent form, k_mfma_corr_H) and the generic kernels of generic.hip in both dtypes.  Each geometry of
direct_dispatch.MATRIX is chosen with the host mirror of the dispatch so that together they reach all 35 dispatchable
MFMA instances, all 14 generic ones and every edge of every kernel (tests/test_direct_dispatch_cpu.py checks that without
a GPU).  On each, path='mfma', path='generic' and -- where it mixes the two families -- path='auto' are held against the
float64 C oracle at the project's bars: 2e-5 (float32) / 1e-10 (float64) of the output's maximum per primitive, twice that
for one fused step, four times for the chained second step -- on the whole batch, on the last sample and on an interior
one, on random operands and on activations (and, for the H gradient, samples) that are single ones at the corners and the
centre of each plane, where a wrong halo offset or a swapped atom is an error of order one and the region no placed atom
reaches must stay empty.  After every call the family that ran is the one the mirror names; where path='mfma' does not
cover a shape the library's refusal is expected, and nothing has been written.
"""
import ctypes
import math
import zlib

import numpy as np
import pytest
import torch

import direct_dispatch as dd
from oracle import tnmf_oracle as orc
from test_hip_parity import dev, make_backend, relmax

pytestmark = pytest.mark.gpu

TOL = {'f': 2e-5, 'd': 1e-10}
NP = {'f': np.float32, 'd': np.float64}
EPS = 1e-9
SPARSITY, INHIBITION, CROSS_INHIBITION = 0.05, 0.1, 0.05

CASES = dd.matrix_cases()


def bar(geometry, T, primitive):
    """The project's bar, scaled by sqrt(K / K_held) where a contraction is longer than the bar is held for (rounding
    of a k-ordered chain of non-negative terms grows like a random walk): from the geometry, never from a measurement."""
    return TOL[T] * max(1.0, math.sqrt(dd.contraction(geometry, primitive) / dd.K_HELD[primitive]))


def operands(gid, kind):
    """(V, W, H) as float64 images of float32 values: the oracle sees exactly what the kernels see.  'random': as the
    other parity tests draw them.  'corners': the same V and W; H is zero except for single ones at the corners and the
    centre of a plane -- plane (n, m) carries spot j when n + m + j is even, so neighbouring atoms sit at different
    corners and R is a sum of shifted copies of W with nothing in between."""
    N, C, D, M, A = dd.MATRIX[gid]
    k = len(A)
    rng = np.random.default_rng(zlib.crc32(gid.encode()))
    V = rng.random((N, C) + D)
    Wn = rng.random((M, C) + A)
    Wn /= Wn.sum(axis=tuple(range(-k, 0)), keepdims=True)
    Hs = tuple(d + a - 1 for d, a in zip(D, A))
    Hn = rng.random((N, M) + Hs)
    if kind == 'corners':
        Hn = _spots((N, M), Hs)
    return tuple(np.asarray(x, dtype=np.float32).astype(np.float64) for x in (V, Wn, Hn))


def _spots(lead, shape):
    out = np.zeros(lead + shape)
    for n in range(lead[0]):
        for m in range(lead[1]):
            for j, spot in enumerate(dd.corner_spots(shape)):
                if (n + m + j) % 2 == 0:
                    out[(n, m) + spot] = 1.0
    return out


def check(name, got, want, tol, kernel=''):
    err = relmax(got, want)
    print(f'    {name} [{kernel}]: {err:.2e} (bar {tol:.1e})')
    assert err < tol, (name, err, tol)


def check_empty_region(got, want, tol, kernel):
    """Where the oracle's R is exactly zero (no placed atom reaches), the kernel's R stays below the bar."""
    empty = np.asarray(want) == 0
    assert empty.any()
    leak = np.abs(np.asarray(got, dtype=np.float64)[empty]).max() / np.abs(want).max()
    print(f'    empty region ({empty.mean():.0%} of R) [{kernel}]: {leak:.2e} (bar {tol:.1e})')
    assert leak < tol, ('leak into the empty region', leak, tol)


def slices_of(N):
    """The whole batch, the last sample and an interior one (where the batch has them)."""
    out = [slice(None)]
    if N > 1:
        out.append(slice(N - 1, N))
    if N > 2:
        out.append(slice(1, 2))
    return out


def padded(Hc):
    """The values of a contiguous [N, M, Hy, Hx] tensor in storage whose rows are longer than Hx (whole 128-byte lines,
    one more where Hx fills its lines exactly), as test_hip_split_matrix.py builds them."""
    ld = (Hc.shape[3] // 32 + 1) * 32
    store = torch.zeros(tuple(Hc.shape[:3]) + (ld,), dtype=Hc.dtype, device=Hc.device)
    Hp = store[..., :Hc.shape[3]]
    Hp.copy_(Hc)
    return Hp


class _Oracle:
    """The float64 results of one geometry, computed once for its (dtype, path) cases."""

    def __init__(self, gid):
        self.gid, self.memo = gid, {}
        orc.set_threads(orc.default_threads(cap=16))

    def get(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def primitives(self, kind):
        def make():
            V, Wn, Hn = operands(self.gid, kind)
            R = orc.reconstruct(Wn, Hn, 'c')
            gH = orc.gradient_H(V, Wn, Hn, slice(None), 'c')
            gW = [orc.gradient_W(V, Wn, Hn, s, 'c') for s in slices_of(V.shape[0])]
            return R, gH, gW
        return self.get(('prim', kind), make)

    def spot_samples(self):
        """(X, correlation of X with W): X is zero except single ones at the corners and the centre of each sample plane,
        so the correlation is a sum of shifted copies of W."""
        def make():
            V, Wn, _ = operands(self.gid, 'random')
            X = _spots(V.shape[:2], V.shape[2:])
            return X, orc._correlate_with_W(Wn, X, 'c')
        return self.get('spots', make)

    def chain(self):
        """H step with sparsity 0.1, W step on the new H, H step with the new W (test_fft_family_against_oracle)."""
        def make():
            V, Wn, Hn = operands(self.gid, 'random')
            on, op = self.primitives('random')[1]
            H1 = Hn * on / (op + EPS + 0.1)
            on, op = orc.gradient_W(V, Wn, H1, slice(None), 'c')
            W1 = Wn * on / (op + EPS)
            W1 = W1 / W1.sum(axis=tuple(range(2, Wn.ndim)), keepdims=True)
            on, op = orc.gradient_H(V, W1, H1, slice(None), 'c')
            return H1, W1, H1 * on / (op + EPS)
        return self.get('chain', make)

    def lateral(self):
        """H after OracleNMF.update_H with lateral and cross-atom inhibition (default range: atom size - 1)."""
        def make():
            V, Wn, Hn = operands(self.gid, 'random')
            ref = orc.OracleNMF(n_atoms=Wn.shape[0], atom_shape=Wn.shape[2:], impl='c')
            ref.V, ref.W, ref.H = V, Wn, Hn.copy()
            ref.update_H(slice(None), sparsity=SPARSITY, inhibition=INHIBITION, cross_inhibition=CROSS_INHIBITION)
            return ref.H
        return self.get('lateral', make)


_oracle = [None]


def oracle_of(gid):
    if _oracle[0] is None or _oracle[0].gid != gid:
        _oracle[0] = _Oracle(gid)
    return _oracle[0]


@pytest.mark.parametrize('gid,T,path', CASES, ids=['-'.join(c) for c in CASES])
def test_direct_kernel_cell_against_oracle(gid, T, path):
    """One geometry, one dtype, one path, one backend."""
    from tnmf_amd import _lib
    N, C, D, M, A = G = dd.MATRIX[gid]
    g = dd.geo(G)
    dt, two_d = NP[T], len(A) == 2
    ref = oracle_of(gid)
    V = operands(gid, 'random')[0]
    be = make_backend(V.astype(dt), A, M, path)
    cells = {p: dd.cell(G, T, path, p) for p in dd.PRIMITIVES}
    print(f'{gid} {T} {path}: ' + ', '.join(f'{p} on {c.inst or c.family}' for p, c in cells.items()))
    # the tile loops with a partial last round run on this device as they do on the 256 CUs the geometry was chosen for
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for p, c in cells.items():
        for flag in ('tile_loop_partial', 'item_loop'):
            if flag in c.edges:
                assert flag in dd.cell(G, T, path, p, num_cu=num_cu).edges, (gid, p, flag, num_cu)

    def sub(s):
        return (len(range(N)[s]), C, D, M, A)

    def expect(call, s=slice(None), pad=False):
        """The mirror's answer for a backend call on the samples s: (family, kernel); ('refused', None) where the
        library must answer TNMF_E_UNSUPPORTED."""
        fam, err = dd.api_family(sub(s), T, path, call, pad)
        assert err in (None, 'E_UNSUPPORTED'), (call, err)      # (E_STRIDE never reaches the caller: HIP.py copies)
        return fam, dd.cell(sub(s), T, path, call, pad).kernel

    def ran(fam):
        assert be.last_path == fam, (fam, be.last_path)

    def refused(call):
        with pytest.raises(_lib.TnmfHipError) as exc:
            call()
        assert exc.value.code == _lib.E_UNSUPPORTED, exc.value

    # ---- the three primitives: random and corner activations, whole batch and one-sample slices
    for kind in ('random', 'corners'):
        _, Wn, Hn = operands(gid, kind)
        R, (on, op), gW = ref.primitives(kind)
        W, H = dev(Wn, dt), dev(Hn, dt)
        for i, s in enumerate(slices_of(N)):
            print(f'  {kind} operands, samples {s}')
            fam, kern = expect('reconstruct', s)
            if fam == 'refused':
                refused(lambda: be.reconstruct(W, H[s]))
            else:
                got = be.to_ndarray(be.reconstruct(W, H[s]))
                ran(fam)
                check('R', got, R[s], bar(G, T, 'reconstruct'), kern)
                if kind == 'corners':
                    check_empty_region(got, R[s], bar(G, T, 'reconstruct'), kern)
            fam, kern = expect('grad_H', s)
            if fam == 'refused':
                refused(lambda: be.reconstruction_gradient_H(V, W, H, s))
            else:
                neg, pos = be.reconstruction_gradient_H(V, W, H, s)
                ran(fam)
                assert tuple(neg.shape) == on[s].shape
                check('neg_H', be.to_ndarray(neg), on[s], bar(G, T, 'grad_H'), kern)
                check('pos_H', be.to_ndarray(pos), op[s], bar(G, T, 'grad_H'), kern)
            fam, kern = expect('grad_W', s)
            if fam == 'refused':
                refused(lambda: be.reconstruction_gradient_W(V, W, H, s))
            else:
                neg, pos = be.reconstruction_gradient_W(V, W, H, s)
                ran(fam)
                check('neg_W', be.to_ndarray(neg), gW[i][0], bar(G, T, 'grad_W'), kern)
                check('pos_W', be.to_ndarray(pos), gW[i][1], bar(G, T, 'grad_W'), kern)

    _, Wn, Hn = operands(gid, 'random')
    W = dev(Wn, dt)

    # ---- the H-gradient kernel alone on samples that are single ones (given as V and as R: neg == pos, a sum of shifted
    # copies of W), and what path='mfma' answers for the H primitives it does not cover: nothing has been written
    X, want = ref.spot_samples()
    Xd, H = dev(X, dt), dev(Hn, dt)
    neg, pos = torch.empty_like(H), torch.empty_like(H)
    geom = be._geom(N, M)
    rc = be._lib.tnmf_hip_grad_H(be._ctx, ctypes.byref(geom), ctypes.c_void_p(Xd.data_ptr()), ctypes.c_void_p(Xd.data_ptr()),
                                 ctypes.c_void_p(W.data_ptr()), ctypes.c_void_p(H.data_ptr()),
                                 ctypes.c_void_p(neg.data_ptr()), ctypes.c_void_p(pos.data_ptr()), be._stream())
    print('  single-one samples')
    if cells['grad_H'].family == 'refused':
        assert rc == _lib.E_UNSUPPORTED, rc
    else:
        _lib.check(rc, 'tnmf_hip_grad_H')
        ran(cells['grad_H'].family)
        check('neg_H of single ones', be.to_ndarray(neg), want, bar(G, T, 'grad_H'), cells['grad_H'].kernel)
        check('pos_H of single ones', be.to_ndarray(pos), want, bar(G, T, 'grad_H'), cells['grad_H'].kernel)
    if cells['update_H'].family == 'refused':
        Hf = dev(Hn, dt)
        rc = be._lib.tnmf_hip_update_H(be._ctx, ctypes.byref(geom), ctypes.c_void_p(be._V_dev.data_ptr()),
                                       ctypes.c_void_p(W.data_ptr()), ctypes.c_void_p(Hf.data_ptr()),
                                       ctypes.c_void_p(Xd.data_ptr()), 1, EPS, SPARSITY, be._stream())
        assert rc == _lib.E_UNSUPPORTED, rc
        assert torch.equal(Hf, H), 'a refused in-place update wrote H'

    # ---- fused half steps, chained
    print('  fused steps')
    H1, W1, H2 = ref.chain()
    fam_H, kern_H = expect('update_H')
    fam_W, kern_W = expect('grad_W')
    Hf, Wf = dev(Hn, dt), dev(Wn, dt)
    if fam_H == 'refused':
        refused(lambda: be.fused_update_H(V, W, Hf, slice(None), sparsity=0.1, eps=EPS))
        assert torch.equal(Hf, dev(Hn, dt)), 'a refused in-place update wrote H'
    else:
        be.fused_update_H(V, W, Hf, slice(None), sparsity=0.1, eps=EPS)
        ran(fam_H)
        check('H step', be.to_ndarray(Hf), H1, 2 * bar(G, T, 'update_H'), kern_H)
    if fam_W == 'refused':
        refused(lambda: be.fused_update_W(V, Wf, Hf, slice(None), eps=EPS))
    elif fam_H != 'refused':
        be.fused_update_W(V, Wf, Hf, slice(None), eps=EPS)
        ran(fam_W)
        check('W step', be.to_ndarray(Wf), W1, 2 * max(bar(G, T, 'update_H'), bar(G, T, 'grad_W')), kern_W)
        be.fused_update_H(V, Wf, Hf, slice(None), sparsity=0., eps=EPS)
        ran(fam_H)
        check('second H step', be.to_ndarray(Hf), H2, 4 * bar(G, T, 'update_H'), kern_H)

    # ---- one H step with lateral and cross-atom inhibition: the generic kernel adds the term in its epilogue, the MFMA
    # kernel has none and tnmf_hip_update_H_ex takes the unfused gradient of the same family and one update kernel
    if two_d and max(A) <= 16 and fam_H != 'refused':
        print('  lateral terms')
        HL = dev(Hn, dt)
        be.fused_update_H(V, W, HL, slice(None), sparsity=SPARSITY, eps=EPS, inhibition=INHIBITION,
                          cross_inhibition=CROSS_INHIBITION, inhibition_kernels=orc.inhibition_kernels(tuple(a - 1 for a in A)))
        ran(fam_H)
        check('H step with lateral terms', be.to_ndarray(HL), ref.lateral(), 2 * bar(G, T, 'update_H'), kern_H)

    # ---- row-padded activations on the generic kernels: the same bits as C-contiguous ones, the pad columns untouched
    if two_d and path == 'generic':
        print('  row-padded activations')
        Hc, Hp = dev(Hn, dt), padded(dev(Hn, dt))
        assert be._row_stride(Hp) == Hp.stride(2) > g.Hx
        for s in slices_of(N):
            Rc, Rp = be.reconstruct(W, Hc[s]), be.reconstruct(W, Hp[s])
            ran(expect('reconstruct', s, True)[0])
            assert torch.equal(Rc, Rp)
            (nc, pc), (npd, ppd) = be.reconstruction_gradient_H(V, W, Hc, s), be.reconstruction_gradient_H(V, W, Hp, s)
            ran(expect('grad_H', s, True)[0])
            assert torch.equal(nc, npd) and torch.equal(pc, ppd)
            (nc, pc), (npd, ppd) = be.reconstruction_gradient_W(V, W, Hc, s), be.reconstruction_gradient_W(V, W, Hp, s)
            ran(expect('grad_W', s, True)[0])
            assert torch.equal(nc, npd) and torch.equal(pc, ppd)
            assert not Hp._base[..., g.Hx:].any()
        s = slices_of(N)[-1]
        Hc, Hp = dev(Hn, dt), padded(dev(Hn, dt))
        be.fused_update_H(V, W, Hc, s, sparsity=SPARSITY, eps=EPS)
        be.fused_update_H(V, W, Hp, s, sparsity=SPARSITY, eps=EPS)
        ran(expect('update_H', s, True)[0])
        assert torch.equal(Hc, Hp), (Hc - Hp).abs().max().item()
        assert not Hp._base[..., g.Hx:].any()
        Wc, Wp = dev(Wn, dt), dev(Wn, dt)
        be.fused_update_W(V, Wc, Hc, s, eps=EPS)
        be.fused_update_W(V, Wp, Hp, s, eps=EPS)
        ran(expect('grad_W', s, True)[0])
        assert torch.equal(Wc, Wp), (Wc - Wp).abs().max().item()
    del be
