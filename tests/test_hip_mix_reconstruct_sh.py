"""
k_mix_reconstruct_sh, the mixed reconstruct of large one-channel calls with the row spectra staged through LDS
(path='hybrid', float32).  Its arithmetic is that of k_mix_reconstruct<T, AY, 1, 16, 8> -- the same packed multiply-adds on
the same values in the same order per output -- so the first check is BIT equality: the reconstruction of a whole call
(new kernel) against the same samples reconstructed in slices small enough to stay under the threshold (samples are
independent; tests/mix_reconstruct_sh_dispatch.py names the kernel of either call).  Then the float64 C oracle at the bar
tests/test_hip_fft_matrix.py holds this primitive to (2e-5 of the output's maximum), a sentinel around the output, a second
dictionary on the same activations, and one H step, W step, H step chain whose reconstructions all run on the new kernel
(the second H step with the row spectra of the UPDATED dictionary: FftState::W_ok).

The C ABI always reconstructs with the clamp at zero (nonneg) on; "off" is not reachable from here.  The bit comparison
therefore runs on non-negative activations, where the clamp only removes rounding noise, and on activations of mixed
sign, where it acts on half of the output.  The kernel's own output, row spectra in the library's workspace, is not
reachable either: the sentinel sits in front of and behind R (rows past the last sample), and a stray write into the
spectra of a neighbouring sample or row would show as a bit difference to the sliced calls.

The geometries (CASES) are the smallest that cross the kernel's threshold of 24 MiB of row spectra and still meet each of
its edges (tests/test_mix_reconstruct_sh_dispatch_cpu.py checks that without a GPU).
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import mix_reconstruct_sh_dispatch as rsh
from oracle import tnmf_oracle as orc
from test_hip_parity import dev, make_backend, relmax

pytestmark = pytest.mark.gpu

TOL = 2e-5
EPS = 1e-9
SENTINEL = -7777.0
FUSED_CASE = 'ay5_one_block_m12'


def operands(cid):
    """(V, W, W2, H, H of mixed sign) as float64 images of float32 values: the oracle sees exactly what the kernel sees."""
    N, C, D, M, A = rsh.CASES[cid][0]
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    V = rng.random((N, C) + D)
    Ws = []
    for _ in range(2):
        Wn = rng.random((M, C) + A)
        Ws.append(Wn / Wn.sum(axis=(-2, -1), keepdims=True))
    Hn = rng.random((N, M) + tuple(d + a - 1 for d, a in zip(D, A)))
    Hs = Hn * rng.choice((-1.0, 1.0), size=Hn.shape)
    return tuple(np.asarray(x, dtype=np.float32).astype(np.float64) for x in (V, Ws[0], Ws[1], Hn, Hs))


def check(name, got, want, tol=TOL):
    err = relmax(got, want)
    print(f'    {name}: {err:.2e} (bar {tol:.0e})')
    assert err < tol, (name, err, tol)


def reconstruct_guarded(be, W, H):
    """tnmf_hip_reconstruct of the whole of H into the middle of a buffer of sentinels -> R; the sentinels stay."""
    from tnmf_amd import _lib
    n, (Dy, Dx) = H.shape[0], be._sample_shape
    guard = 32 * Dx
    buf = torch.full((2 * guard + n * Dy * Dx,), SENTINEL, dtype=torch.float32, device=H.device)
    R = buf[guard:guard + n * Dy * Dx].view(n, 1, Dy, Dx)
    be._foreign_H()
    g = be._geom(n, W.shape[0], 0)
    _lib.check(be._lib.tnmf_hip_reconstruct(be._ctx, ctypes.byref(g), ctypes.c_void_p(W.data_ptr()),
                                            ctypes.c_void_p(H.data_ptr()), ctypes.c_void_p(R.data_ptr()), be._stream()),
               'tnmf_hip_reconstruct')
    torch.cuda.synchronize()
    assert be.last_path == 'fft'
    assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n * Dy * Dx:] == SENTINEL).all()), 'stray write'
    assert not bool((R == SENTINEL).any()), 'an output was not written'
    return R


def reconstruct_in_slices(be, W, H, per_call):
    parts = []
    for i in range(0, H.shape[0], per_call):
        parts.append(be.reconstruct(W, H[i:i + per_call]))
        assert be.last_path == 'fft'
    return torch.cat(parts)


@pytest.mark.parametrize('cid', list(rsh.CASES))
def test_reconstruct_bit_equal_and_against_oracle(cid):
    g, n = rsh.CASES[cid]
    N, _, _, M, A = g
    s = slice(None) if n is None else slice(N - n, N)      # a slice: the LAST samples of the bound problem
    per_call = rsh.under_threshold(g, n)
    assert rsh.reconstruct_kernel(g, n) == 'k_mix_reconstruct_sh' and rsh.reconstruct_kernel(g, per_call) == 'k_mix_reconstruct'
    print(f'{cid}: (kx tiles, row blocks, samples) = {rsh.rsh_grid(g, n)}, slices of {per_call}, edges {sorted(rsh.edges(g, n))}')
    orc.set_threads(orc.default_threads(cap=16))
    V, Wn, W2n, Hn, Hsn = operands(cid)
    be = make_backend(V.astype(np.float32), A, M, 'hybrid')
    W, W2, H, Hs = dev(Wn, np.float32), dev(W2n, np.float32), dev(Hn, np.float32)[s], dev(Hsn, np.float32)[s]
    # non-negative activations: bit equality, the oracle, the sentinels
    whole = reconstruct_guarded(be, W, H)
    assert torch.equal(whole, reconstruct_in_slices(be, W, H, per_call)), 'differs from k_mix_reconstruct'
    check('R', be.to_ndarray(whole), orc.reconstruct(Wn, Hn[s], 'c'))
    # another dictionary on the same activations
    whole2 = reconstruct_guarded(be, W2, H)
    assert torch.equal(whole2, reconstruct_in_slices(be, W2, H, per_call)), 'second W: differs from k_mix_reconstruct'
    check('R with the second W', be.to_ndarray(whole2), orc.reconstruct(W2n, Hn[s], 'c'))
    assert not torch.equal(whole, whole2)
    # activations of mixed sign: the clamp at zero acts
    signed = reconstruct_guarded(be, W, Hs)
    assert torch.equal(signed, reconstruct_in_slices(be, W, Hs, per_call)), 'mixed signs: differs from k_mix_reconstruct'
    zeros = float((signed == 0).float().mean())
    print(f'    mixed signs: {zeros:.0%} of R clamped to zero')
    assert 0.2 < zeros < 0.8 and bool((signed >= 0).all())
    del be


def test_fused_steps_on_the_new_kernel():
    """H step, W step on the new H, H step with the new W: every reconstruction of the chain is a whole call above the
    threshold, the last one with row spectra of W that the W step has made stale."""
    g, n = rsh.CASES[FUSED_CASE]
    assert n is None and rsh.reconstruct_kernel(g) == 'k_mix_reconstruct_sh'
    _, _, _, M, A = g
    orc.set_threads(orc.default_threads(cap=16))
    V, Wn, _, Hn, _ = operands(FUSED_CASE)
    be = make_backend(V.astype(np.float32), A, M, 'hybrid')
    on, op = orc.gradient_H(V, Wn, Hn, slice(None), 'c')
    H1 = Hn * on / (op + EPS)
    on, op = orc.gradient_W(V, Wn, H1, slice(None), 'c')
    W1 = Wn * on / (op + EPS)
    W1 /= W1.sum(axis=(-2, -1), keepdims=True)
    on, op = orc.gradient_H(V, W1, H1, slice(None), 'c')
    H2 = H1 * on / (op + EPS)
    Hf, Wf = dev(Hn, np.float32), dev(Wn, np.float32)
    be.fused_update_H(V, Wf, Hf, slice(None), sparsity=0., eps=EPS)
    check('H step', be.to_ndarray(Hf), H1, 2 * TOL)
    be.fused_update_W(V, Wf, Hf, slice(None), eps=EPS)
    assert be.last_path == 'fft'
    check('W step', be.to_ndarray(Wf), W1, 2 * TOL)
    be.fused_update_H(V, Wf, Hf, slice(None), sparsity=0., eps=EPS)
    check('second H step', be.to_ndarray(Hf), H2, 4 * TOL)
    del be
