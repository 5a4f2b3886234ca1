"""
The FFT kernel family, every instance of it: each geometry of fft_dispatch.MATRIX is chosen with the host mirror of the
dispatch so that together they reach all 260 kernel instances the product build can run (row and column transforms of
every length in both dtypes, the five channel classes of k_fft_grad_H on every column length, the sixteen atom heights of
the mixed kernels, the resident-spectrum kernels in every channel group, the 1-D forms) and every edge of every kernel:
exact fit, one short and the shortest activation of each transform length, partial tiles of rows, columns, atoms, channels
and sample groups (tests/test_fft_dispatch_cpu.py checks that without a GPU).  On each, path='fft' and path='hybrid' are
held against the float64 C oracle at the bars of test_fft_family_against_oracle and test_hybrid_dispatch_on_ragged_shapes:
2e-5 (float32) / 1e-10 (float64) of the output's maximum per primitive, twice that for one fused step, four times for the
chained steps -- on the whole batch, on the last sample and on an interior one, on random operands and on activations that
are single ones at the corners and the centre of each plane, where a wrong crop offset, a wrap-round at exact fit or a
swapped atom is an error of order one and the region no placed atom reaches must stay empty.
"""
import zlib

import numpy as np
import pytest

import fft_dispatch as fd
from oracle import tnmf_oracle as orc
from test_hip_parity import dev, make_backend, relmax

pytestmark = pytest.mark.gpu

TOL = {'f': 2e-5, 'd': 1e-10}
NP = {'f': np.float32, 'd': np.float64}
DIRECT = ('split', 'mfma', 'generic')
EPS = 1e-9

CASES = [(gid, T, path) for gid, g in fd.MATRIX.items() for T in fd.DTYPES if fd.fft_has(g, T) for path in fd.PATHS]


def operands(gid, kind):
    """(V, W, H) as float64 images of float32 values: the oracle sees exactly what the kernels see.  'random': as the
    other parity tests draw them.  'corners': the same V and W; H is zero except for single ones at the four corners and
    the centre of a plane (1-D: both ends and the centre) -- plane (n, m) carries spot k when n + m + k is even, so
    neighbouring atoms sit at different corners and R is a sum of shifted copies of W with nothing in between."""
    N, C, D, M, A = fd.MATRIX[gid]
    k = len(A)
    rng = np.random.default_rng(zlib.crc32(gid.encode()))
    V = rng.random((N, C) + D)
    Wn = rng.random((M, C) + A)
    Wn /= Wn.sum(axis=tuple(range(-k, 0)), keepdims=True)
    Hs = tuple(d + a - 1 for d, a in zip(D, A))
    Hn = rng.random((N, M) + Hs)
    if kind == 'corners':
        Hn = np.zeros_like(Hn)
        ends = [(0, h - 1) for h in Hs]
        spots = [(x,) for x in ends[0]] if k == 1 else [(y, x) for y in ends[0] for x in ends[1]]
        spots.append(tuple(h // 2 for h in Hs))
        for n in range(N):
            for m in range(M):
                for j, spot in enumerate(spots):
                    if (n + m + j) % 2 == 0:
                        Hn[(n, m) + spot] = 1.0
    return tuple(np.asarray(x, dtype=np.float32).astype(np.float64) for x in (V, Wn, Hn))


def check(name, got, want, tol):
    err = relmax(got, want)
    print(f'    {name}: {err:.2e} (bar {tol:.0e})')
    assert err < tol, (name, err, tol)


def check_empty_region(got, want, tol):
    """Where the oracle's R is exactly zero (no placed atom reaches), the kernel's R stays below the bar."""
    empty = np.asarray(want) == 0
    assert empty.any()
    leak = np.abs(np.asarray(got, dtype=np.float64)[empty]).max() / np.abs(want).max()
    print(f'    empty region ({empty.mean():.0%} of R): {leak:.2e} (bar {tol:.0e})')
    assert leak < tol, ('leak into the empty region', leak, tol)


def slices_of(N):
    return (slice(None), slice(N - 1, N), slice(1, 2))      # whole batch, last sample, an interior one


class _Oracle:
    """The float64 results of one geometry, computed once for its four (dtype, path) cases."""

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
            N = V.shape[0]
            R = orc.reconstruct(Wn, Hn, 'c')
            gH = orc.gradient_H(V, Wn, Hn, slice(None), 'c')
            gW = {0: orc.gradient_W(V, Wn, Hn, slice(None), 'c')}
            for i, s in enumerate(slices_of(N)[1:], 1):
                gW[i] = orc.gradient_W(V, Wn, Hn, s, 'c')
            return R, gH, gW
        return self.get(('prim', kind), make)

    @staticmethod
    def _step_W(V, Wn, Hn):
        on, op = orc.gradient_W(V, Wn, Hn, slice(None), 'c')
        Wo = Wn * on / (op + EPS)
        return Wo / Wo.sum(axis=tuple(range(2, Wn.ndim)), keepdims=True)

    def chain_fft(self):
        """test_fft_family_against_oracle: H step with sparsity 0.1, W step on the new H, H step with the new W."""
        def make():
            V, Wn, Hn = operands(self.gid, 'random')
            on, op = self.primitives('random')[1]
            H1 = Hn * on / (op + EPS + 0.1)
            W1 = self._step_W(V, Wn, H1)
            on, op = orc.gradient_H(V, W1, H1, slice(None), 'c')
            return H1, W1, H1 * on / (op + EPS)
        return self.get('chain_fft', make)

    def chain_hybrid(self):
        """test_hybrid_dispatch_on_ragged_shapes: two iterations of H step, W step."""
        def make():
            V, Wn, Hn = operands(self.gid, 'random')
            Ho, Wo = Hn, Wn
            for it in range(2):
                on, op = self.primitives('random')[1] if it == 0 else orc.gradient_H(V, Wo, Ho, slice(None), 'c')
                Ho = Ho * on / (op + EPS)
                Wo = self._step_W(V, Wo, Ho)
            return Ho, Wo
        return self.get('chain_hybrid', make)

    def step_W(self):
        def make():
            V, Wn, Hn = operands(self.gid, 'random')
            return self._step_W(V, Wn, Hn)
        return self.get('step_W', make)


_oracle = [None]


def oracle_of(gid):
    if _oracle[0] is None or _oracle[0].gid != gid:
        _oracle[0] = _Oracle(gid)
    return _oracle[0]


@pytest.mark.parametrize('gid,T,path', CASES, ids=['-'.join(c) for c in CASES])
def test_fft_family_cell_against_oracle(gid, T, path):
    """One geometry, one dtype, one path, one backend: the three primitives on the whole batch and on two one-sample slices
    with random and with corner activations, then the fused half steps chained on the cached spectra."""
    N, C, D, M, A = g = fd.MATRIX[gid]
    dt, tol = NP[T], TOL[T]
    ref = oracle_of(gid)
    V = operands(gid, 'random')[0]
    be = make_backend(V.astype(dt), A, M, path)
    fam_H = fd.family(g, T, path, 'grad_H')
    print(f'{gid} {T} {path}: lengths {fd.make_layout(g, T, path)[:2]}, {len(fd.cells(g, T, path))} kernel instances')

    def ran_on(prim):
        want = fd.family(g, T, path, prim)
        assert (be.last_path == 'fft') if want == 'fft' else (be.last_path in DIRECT), (prim, want, be.last_path)

    for kind in ('random', 'corners'):
        _, Wn, Hn = operands(gid, kind)
        R, (on, op), gW = ref.primitives(kind)
        W, H = dev(Wn, dt), dev(Hn, dt)
        for i, s in enumerate(slices_of(N)):
            print(f'  {kind} operands, samples {s}')
            got = be.to_ndarray(be.reconstruct(W, H[s]))
            ran_on('reconstruct')
            check('R', got, R[s], tol)
            if kind == 'corners':
                check_empty_region(got, R[s], tol)
            if fam_H != 'refused':
                neg, pos = be.reconstruction_gradient_H(V, W, H, s)
                ran_on('grad_H')
                assert tuple(neg.shape) == on[s].shape
                check('neg_H', be.to_ndarray(neg), on[s], tol)
                check('pos_H', be.to_ndarray(pos), op[s], tol)
            neg, pos = be.reconstruction_gradient_W(V, W, H, s)
            ran_on('grad_W')
            check('neg_W', be.to_ndarray(neg), gW[i][0], tol)
            check('pos_W', be.to_ndarray(pos), gW[i][1], tol)

    # fused half steps on the cached spectra, random operands
    _, Wn, Hn = operands(gid, 'random')
    print('  fused steps')
    if fam_H == 'refused':                      # 1-D under path='fft': the W step alone
        Wf = dev(Wn, dt)
        be.fused_update_W(V, Wf, dev(Hn, dt), slice(None), eps=EPS)
        ran_on('update_W')
        check('W step', be.to_ndarray(Wf), ref.step_W(), 2 * tol)
    elif path == 'fft':
        H1, W1, H2 = ref.chain_fft()
        W, H = dev(Wn, dt), dev(Hn, dt)
        neg, pos = be.reconstruction_gradient_H(V, W, H)
        own = Hn * be.to_ndarray(neg).astype(np.float64) / (be.to_ndarray(pos).astype(np.float64) + EPS + 0.1)
        Hf = dev(Hn, dt)
        be.fused_update_H(V, W, Hf, slice(None), sparsity=0.1, eps=EPS)
        ran_on('update_H')
        # (the fusion computes what the unfused kernels of the same family do: test_fft_family_at_baseline_sizes)
        check('H step against the unfused gradients', be.to_ndarray(Hf), own, 1e-5 if T == 'f' else 2 * tol)
        check('H step', be.to_ndarray(Hf), H1, 2 * tol)
        Wf = dev(Wn, dt)
        be.fused_update_W(V, Wf, Hf, slice(None), eps=EPS)       # the cached spectra of the updated H
        ran_on('update_W')
        check('W step', be.to_ndarray(Wf), W1, 2 * tol)
        be.fused_update_H(V, Wf, Hf, slice(None), sparsity=0., eps=EPS)   # cached spectra again, new W
        ran_on('update_H')
        check('second H step', be.to_ndarray(Hf), H2, 4 * tol)
    else:
        Ho, Wo = ref.chain_hybrid()
        Hf, Wf = dev(Hn, dt), dev(Wn, dt)
        for _ in range(2):
            be.fused_update_H(V, Wf, Hf, slice(None), sparsity=0., eps=EPS)
            ran_on('update_H')
            be.fused_update_W(V, Wf, Hf, slice(None), eps=EPS)
            ran_on('update_W')
        check('H after two iterations', be.to_ndarray(Hf), Ho, 4 * tol)
        check('W after two iterations', be.to_ndarray(Wf), Wo, 4 * tol)
    del be
