"""
k_mix_grad_W3, the three-multiply mixed W gradient of large calls, against the float64 C oracle: neg_W and pos_W of
reconstruction_gradient_W (path='hybrid', float32) at the bar tests/test_hip_fft_matrix.py holds this primitive to, 2e-5
of the output's maximum, and one fused W step at twice that.  The geometries (tests/mix_grad_w3_dispatch.py: CASES) are
the smallest that cross the kernel's threshold of 24 MiB of row spectra and still meet each of its edges: atom and kx
tails, one to three atom blocks, atom heights 1, 3, 5, 9, 12, planes shorter than one LDS chunk and planes that are no
multiple of it, groups of one, two and three samples with a short last group, and calls on slices of a bound problem
(tests/test_mix_grad_w3_dispatch_cpu.py checks all that without a GPU).
"""
import zlib

import numpy as np
import pytest

import mix_grad_w3_dispatch as w3
from oracle import tnmf_oracle as orc
from test_hip_parity import dev, make_backend, relmax

pytestmark = pytest.mark.gpu

TOL = 2e-5
EPS = 1e-9
WHOLE = [cid for cid, (_, n) in w3.CASES.items() if n is None]


def operands(cid):
    """(V, W, H) as float64 images of float32 values: the oracle sees exactly what the kernel sees."""
    N, C, D, M, A = w3.CASES[cid][0]
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    V = rng.random((N, C) + D)
    Wn = rng.random((M, C) + A)
    Wn /= Wn.sum(axis=(-2, -1), keepdims=True)
    Hn = rng.random((N, M) + tuple(d + a - 1 for d, a in zip(D, A)))
    return tuple(np.asarray(x, dtype=np.float32).astype(np.float64) for x in (V, Wn, Hn))


def check(name, got, want, tol=TOL):
    err = relmax(got, want)
    print(f'    {name}: {err:.2e} (bar {tol:.0e})')
    assert err < tol, (name, err, tol)


def gradient(be, V, Wn, Hn, s=slice(None)):
    neg, pos = be.reconstruction_gradient_W(V, dev(Wn, np.float32), dev(Hn, np.float32), s)
    assert be.last_path == 'fft'
    return be.to_ndarray(neg), be.to_ndarray(pos)


@pytest.mark.parametrize('cid', WHOLE)
def test_gradient_against_oracle(cid):
    g, _ = w3.CASES[cid]
    assert w3.grad_W_kernel(g) == 'k_mix_grad_W3'
    print(f'{cid}: (atom blocks, kx tiles, groups, samples per group) = {w3.w3_grid(g)}, edges {sorted(w3.edges(g))}')
    orc.set_threads(orc.default_threads(cap=16))
    V, Wn, Hn = operands(cid)
    be = make_backend(V.astype(np.float32), g[4], g[3], 'hybrid')
    want_neg, want_pos = orc.gradient_W(V, Wn, Hn, slice(None), 'c')
    neg, pos = gradient(be, V, Wn, Hn)
    check('neg_W', neg, want_neg)
    check('pos_W', pos, want_pos)
    if cid == WHOLE[0]:
        # one full W step on the same operands: multiplicative update, then the atoms normalised
        Wo = Wn * want_neg / (want_pos + EPS)
        Wo /= Wo.sum(axis=(-2, -1), keepdims=True)
        Wf = dev(Wn, np.float32)
        be.fused_update_W(V, Wf, dev(Hn, np.float32), slice(None), eps=EPS)
        assert be.last_path == 'fft'
        check('W step', be.to_ndarray(Wf), Wo, 2 * TOL)
    del be


def test_gradient_on_slices_of_a_bound_problem():
    """The first geometry, called on an interior and on the last third of a problem three times its size: descriptor
    bases, V^/R^ sources and sample counts are those of the slice, not of the binding."""
    cid = 'slices_of_a_binding'
    g, n = w3.CASES[cid]
    assert w3.grad_W_kernel(g, n) == 'k_mix_grad_W3' and g[0] == 3 * n
    orc.set_threads(orc.default_threads(cap=16))
    V, Wn, Hn = operands(cid)
    be = make_backend(V.astype(np.float32), g[4], g[3], 'hybrid')
    for s in (slice(n, 2 * n), slice(2 * n, 3 * n)):
        print(f'  samples {s}')
        want_neg, want_pos = orc.gradient_W(V, Wn, Hn, s, 'c')
        neg, pos = gradient(be, V, Wn, Hn, s)
        check('neg_W', neg, want_neg)
        check('pos_W', pos, want_pos)
    del be


def test_blank_band_of_rows_leaks_nothing():
    """V = 0 on rows 20 .. 32 of every sample (the band crosses a chunk boundary).  Real and imaginary parts are
    differences of three running sums here (A1 - A3, A1 - A2), so a band that contributes exact zeros is where a
    cancellation error would show.  (a) dense activations: neg_W equals the oracle's at the bar and is non-negative after
    the clamp of the inverse row transform.  (b) activations confined to rows 24 .. 29, which meet only blank rows of V
    at the five lags nearest the band: there the oracle's neg_W is exactly zero and the kernel's stays below the bar,
    non-negative, while the other lags and pos_W hold the bar as usual."""
    cid = 'atom_tail_ay12'
    g, _ = w3.CASES[cid]
    orc.set_threads(orc.default_threads(cap=16))
    V, Wn, Hn = operands(cid)
    V[:, :, 20:33, :] = 0
    be = make_backend(V.astype(np.float32), g[4], g[3], 'hybrid')
    Hb = np.zeros_like(Hn)
    Hb[:, :, 24:30, :] = Hn[:, :, 24:30, :]
    for name, H in (('dense H', Hn), ('H on rows 24 .. 29', Hb)):
        print(f'  {name}')
        want_neg, want_pos = orc.gradient_W(V, Wn, H, slice(None), 'c')
        neg, pos = gradient(be, V, Wn, H)
        check('neg_W', neg, want_neg)
        check('pos_W', pos, want_pos)
        assert (neg >= 0).all() and (pos >= 0).all()
        if H is Hb:
            blank = want_neg == 0
            assert blank.any() and not blank.all() and round(blank.mean() * 12) == 5, blank.mean()
            leak = np.abs(neg[blank]).max() / np.abs(want_neg).max()
            print(f'    blank lags ({blank.mean():.0%} of neg_W): {leak:.2e} (bar {TOL:.0e})')
            assert leak < TOL
    del be
