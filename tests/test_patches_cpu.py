"""
Patches on the CPU: the host functions of tnmf_amd/patches_host.py against the independent reference
tests/patches_reference.py, and ``detection_patches`` / ``atom_patch_moments`` / ``atom_modes`` over an oracle-backed backend
without the hooks -- on a planted problem whose answer is known in closed form.  Also the header, the exports and the Makefile.
"""
import ctypes
import dataclasses
import functools
import os
import re

import numpy as np
import pytest

import patches_dispatch as pd
import patches_reference as pref
from conftest import ROOT
from test_events_cpu import _Stub, fitted
from tnmf_amd import _lib, patches_host as ph, transforms as tr
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF, modes_from_moments

U = pref.U


def table_of(name, A):
    """The fold table of a case's transforms by the package's builder."""
    if name is None:
        return None, None, None, 1
    return ph.fold_table(transforms_of(name, A), A)


def transforms_of(name, A):
    """'T1': one map, a magnification by 2 -- weighted entries, and pixels of the rim without an entry; 'rot8': eight
    rotations, several entries per pixel."""
    return {'T1': lambda: tr.scales(A, [2.]), 'rot8': lambda: tr.rotations(A, 8)}.get(name, lambda: name)()


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (rows, h, W, V, R) of a case of patches_dispatch: float64 arrays of float32-representable values, read-only; R is
    the render of the rows in range rounded to float32, as the device's own render would be."""
    N, C, P, D, A, mode, _ = pd.PATCH_CASES[name]
    rows, h = pd.patch_rows(name)
    rng = np.random.default_rng(7)
    W = (rng.random((P, C) + A) + 0.1).astype(np.float32).astype(np.float64)
    V = (rng.random((N, C) + D) * 3.).astype(np.float32).astype(np.float64)
    if name == 'grid-stride':      # (the render of 9 000 rows: that of the distinct places with their strengths added up)
        places, inverse = np.unique(rows, axis=0, return_inverse=True)
        total = np.bincount(inverse.reshape(-1), weights=h, minlength=len(places))
        R = pref.render(W, D, N, mode, places, total)
    else:
        R = pref.render(W, D, N, mode, rows, h)
    R = np.asarray(R, dtype=np.float64).astype(np.float32).astype(np.float64)
    out = (rows, h, W, V, R)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, source):
    """(x, mag, images per row) of the case in the image frame, by the definition, against the case's own R."""
    rows, h, W, V, R = case(name)
    return pref.patches(V, R, W, pd.PATCH_CASES[name][5], rows, h, source)


# -- 1. the table of the fold ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, A', [('flip', (5,)), ('rot90', (5, 5)), ('dihedral', (3, 3)), ('rot8', (5, 5)), ('T1', (5, 5))])
def test_the_fold_table_is_the_transposed_operator(name, A):
    ops = transforms_of(name, A)
    ops = ops if isinstance(ops, tr.AtomOperators) else tr.from_group(ops, A)
    ptr, src, w, T = ph.fold_table(transforms_of(name, A), A)
    nA = int(np.prod(A))
    assert T == ops.T and len(ptr) == T * nA + 1 and ptr[0] == 0 and ptr[-1] == len(src) == len(w) == ops.nnz
    assert ptr.dtype == np.int32 and src.dtype == np.int32 and w.dtype == np.float64
    L = ops.dense().reshape(T, nA, nA)
    dense = np.zeros((T, nA, nA))
    for t in range(T):
        for i in range(nA):
            ks = slice(ptr[t * nA + i], ptr[t * nA + i + 1])
            assert np.all(np.diff(src[ks]) > 0), 'a row in ascending out pixel'
            dense[t, src[ks], i] = w[ks]
    assert np.array_equal(dense, L)
    want = pref.table_from_dense(L)
    assert all(np.array_equal(a, b) for a, b in zip((ptr, src, w), want[:3]))
    if name in ('rot8', 'T1'):   # several entries per pixel; under the magnification pixels without an entry
        assert np.diff(ptr).max() > 1 and (np.diff(ptr).min() == 0) == (name == 'T1')
    # summed over the planes of an atom the fold of the patches is the fold of the W half step
    rng = np.random.default_rng(3)
    X = rng.random((2 * T, 2) + A)
    Y = ph.fold_patches_numpy(X, np.arange(2 * T), (ptr, src, w, T))
    np.testing.assert_allclose(Y.reshape((2, T, 2) + A).sum(axis=1), tr.fold(X, transforms_of(name, A)), rtol=1e-13)
    # <W[m], y> = <W_eff[p], x>
    Wm = rng.random((2, 2) + A)
    We = tr.expand(Wm, transforms_of(name, A))
    np.testing.assert_allclose(np.sum(np.repeat(Wm, T, axis=0) * Y, axis=tuple(range(1, Y.ndim))),
                               np.sum(We * X, axis=tuple(range(1, X.ndim))), rtol=1e-12)


def test_the_backend_keys_its_fold_table_on_the_atom_shape():
    """HIP_Backend._fold_table on a stand-in for a backend that is initialised a second time with atoms of another shape:
    the table of a group name is that of the CURRENT atom shape (its row starts are T * prod(A) + 1, and the kernel reads
    them by the geometry of the call), the earlier one is kept under its own key, operators are keyed by their digest."""
    import types

    import torch

    from tnmf_amd.backends.HIP import HIP_Backend
    be = types.SimpleNamespace(atom_shape=(5,), _fold_tables={}, _device=torch.device('cpu'))
    first = HIP_Backend._fold_table(be, 'flip')
    assert first[3] == 2 and first[0].numel() == 2 * 5 + 1 and HIP_Backend._fold_table(be, 'flip') is first
    be.atom_shape = (7,)                                         # initialize() again, other atoms
    second = HIP_Backend._fold_table(be, 'flip')
    assert second is not first and second[0].numel() == 2 * 7 + 1 and second[1].numel() == 2 * 7
    for got, want in zip(second[:3], ph.fold_table('flip', (7,))[:3]):
        assert np.array_equal(got.numpy(), want)
    be.atom_shape = (3, 3)
    third = HIP_Backend._fold_table(be, 'rot90')
    assert third[0].numel() == 4 * 9 + 1
    be.atom_shape = (5, 5)
    assert HIP_Backend._fold_table(be, 'rot90')[0].numel() == 4 * 25 + 1
    ops = tr.rotations((5, 5), 8)
    assert HIP_Backend._fold_table(be, ops) is HIP_Backend._fold_table(be, tr.rotations((5, 5), 8))
    be.atom_shape = (5,)
    assert HIP_Backend._fold_table(be, 'flip') is first and HIP_Backend._fold_table(be, None) == (None, None, None, 1)
    with pytest.raises(ValueError):
        HIP_Backend._fold_table(be, ops)                          # operators of another atom shape


# -- 2. the host patches against the definition -------------------------------------------------------------------------------
@pytest.mark.parametrize('source', pref.SOURCES)
@pytest.mark.parametrize('name', ['valid-2d', 'full-2d', 'circular-2d', 'reflect-2d', '1d-5', '1d-valid'])
def test_host_patches_against_the_reference(name, source):
    """Bound per element: (c + 4 K) U mag -- the c roundings of the definition (patches_reference.ROUNDINGS) and the host's
    own float64 render of R, which adds at most 4 K terms (K rows of at most 4 images) at a pixel; against R rendered in
    extended precision from the same rows."""
    N, C, P, D, A, mode, tables = pd.PATCH_CASES[name]
    rows, h, W, V, _ = case(name)
    good = pref.in_range(rows, N, P, pref.shift_shape(D, A, mode))
    rows, h = rows[good], h[good]
    R = pref.render(W, D, N, mode, rows, h)
    want, mag, _ = pref.patches(V, R, W, mode, rows, h, source)
    got = ph.event_patches_numpy(W, D, N, mode, rows[:, 0], rows[:, 1], rows[:, 2:], h, V, source, None, 'image')
    assert got.dtype == np.float64 and got.shape == want.shape
    bound = (pref.ROUNDINGS[source] + 4 * len(rows)) * U * mag
    live = bound > 0
    print(f'{name} {source}: {len(rows)} rows, largest error / bound {np.max(np.abs(got - want)[live] / bound[live]):.3g}')
    assert np.all(np.abs(got - want) <= bound)
    for t in tables[1:]:
        table = table_of(t, A)
        y, by = pref.fold(want, bound, rows[:, 1], table)
        got_y = ph.event_patches_numpy(W, D, N, mode, rows[:, 0], rows[:, 1], rows[:, 2:], h, V, source,
                                       transforms_of(t, A), 'atom')
        assert np.all(np.abs(got_y - y) <= by)


def test_host_moments_against_the_reference():
    """|S - S_ref| <= (K_m + 2) U sum |y_i y_j|, |g - g_ref| <= (K_m + 2) U sum h |y_i|: K_m products, K_m - 1 additions in
    any order."""
    rng = np.random.default_rng(5)
    for D in pd.MOMENT_D:
        atom = np.repeat(np.arange(len(pd.MOMENT_RUNS)), pd.MOMENT_RUNS)
        order = rng.permutation(len(atom))
        atom = atom[order]
        Y, h = rng.standard_normal((len(atom), D)), rng.random(len(atom)) + 0.5
        S, g, s2, count = ph.patch_moments_numpy(Y, h, atom, len(pd.MOMENT_RUNS))
        rS, rg, rs2, rcount, Sm, gm = pref.moments(Y, h, atom, len(pd.MOMENT_RUNS))
        K = np.array(pd.MOMENT_RUNS, dtype=np.float64)
        assert np.array_equal(count, rcount) and np.array_equal(count, K)
        assert np.all(np.abs(S - rS) <= (K + 2)[:, None, None] * U * Sm) and np.all(np.abs(g - rg) <= (K + 2)[:, None] * U * gm)
        assert np.all(np.abs(s2 - rs2) <= (K + 2) * U * rs2)
        assert np.array_equal(S, S.transpose(0, 2, 1)) and not S[0].any() and not g[0].any() and s2[0] == 0


def test_modes_from_moments():
    rng = np.random.default_rng(6)
    D, runs = 7, (0, 1, 2, 30)
    atom = np.repeat(np.arange(4), runs)
    Y, h = rng.standard_normal((len(atom), D)), rng.random(len(atom)) + 0.5
    mom = ph.patch_moments_numpy(Y, h, atom, 4)
    mean, modes, var, total = modes_from_moments(*mom, 3)
    rmean, rmodes, rvar, rtotal = pref.modes(*mom, 3)
    assert mean.shape == (4, D) and modes.shape == (4, 3, D) and var.shape == (4, 3) and total.shape == (4,)
    assert np.isnan(mean[0]).all() and np.isnan(modes[:2]).all() and not var[:2].any() and not total[:2].any()
    assert not np.isnan(mean[1:]).any()
    np.testing.assert_allclose(mean[1:], rmean[1:], rtol=1e-13)
    np.testing.assert_allclose(var, rvar, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(total, rtotal, rtol=1e-12)
    np.testing.assert_allclose(modes[2:], rmodes[2:], atol=1e-8)
    assert np.all(np.diff(var[3]) <= 0) and var.min() >= 0
    np.testing.assert_allclose(np.linalg.norm(modes[2:], axis=-1), 1., rtol=1e-12)
    big = np.take_along_axis(modes[2:], np.argmax(np.abs(modes[2:]), axis=-1)[..., None], axis=-1)
    assert np.all(big > 0), 'the entry of largest magnitude is positive'
    # two rows of one atom: the scatter has rank one
    assert var[2, 0] > 0 and np.all(var[2, 1:] <= 1e-12 * var[2, 0])
    # n_modes outside [1, D] or not an integer, and moments whose shapes do not match
    for bad in (0, 8, 1.5, True):
        with pytest.raises(ValueError):
            modes_from_moments(*mom, bad)
    with pytest.raises(ValueError):
        modes_from_moments(mom[0][:, :3], *mom[1:], 2)


# -- 3. the front end on a planted problem --------------------------------------------------------------------------------------
A0, D0, K0 = (5, 5), (32, 32), 24


@functools.lru_cache(maxsize=None)
def planted(transforms=None, seed=0):
    """One atom W0 of 5 x 5 with 24 occurrences h_k (W0 + c_k Delta) on two samples, none touching another, no noise: W0 and
    Delta are multiples of 2^-12, h_k multiples of 1/8 in [0.5, 2], c_k = +-1, so V is exact in float32 as well.  With
    ``transforms='rot90'`` occurrence k is planted in orientation t_k.  -> dict(V, W0, Delta, h, c, t, sample, shift)."""
    rng = np.random.default_rng(seed)
    T = 1 if transforms is None else tr.size(transforms)
    W0 = rng.integers(8, 64, A0) / 2. ** 10
    Delta = rng.choice([-1., 1.], A0) * rng.integers(1, 4, A0) / 2. ** 12
    h = rng.integers(4, 17, K0) / 8.
    c = np.where(np.arange(K0) % 3 == 0, -1., 1.)[rng.permutation(K0)]
    t = rng.integers(0, T, K0)
    t[:T] = np.arange(T)
    V = np.zeros((2, 1) + D0)
    sample, shift = np.repeat([0, 1], K0 // 2), np.zeros((K0, 2), dtype=np.int64)
    cells = np.concatenate([rng.permutation(16)[:K0 // 2] for _ in range(2)])   # 12 of the 16 cells of 8 x 8 per sample
    for k, cell in enumerate(cells):
        oy, ox = (cell // 4) * 8 + rng.integers(0, 4), (cell % 4) * 8 + rng.integers(0, 4)
        occ = W0 + c[k] * Delta
        if transforms is not None:
            occ = tr.apply(tr.GROUPS[transforms][t[k]], occ)
        V[sample[k], 0, oy:oy + 5, ox:ox + 5] = h[k] * occ
        shift[k] = (oy + 4, ox + 4)          # 'valid' mode: shift = origin + A - 1
    assert np.array_equal(V, V.astype(np.float32).astype(np.float64)) and V.min() >= 0
    hW = h[:, None, None] * W0                                  # what the render of a planted row holds
    assert np.array_equal(hW, hW.astype(np.float32).astype(np.float64))
    return dict(V=V, W0=W0, Delta=Delta, h=h, c=c, t=t, sample=sample, shift=shift)


def planted_model(transforms=None, backend=None, dtype=np.float64, to_backend=np.array):
    """A model that holds the planted atom over the planted samples (``to_backend``: the dictionary as the backend keeps it),
    and the planted rows as Detections."""
    pl = planted(transforms)
    kw = {} if transforms is None else dict(transforms=transforms)
    nmf = TransformInvariantNMF(n_atoms=1, atom_shape=A0, backend=backend or _Stub('valid'), **kw)
    nmf._W = to_backend(np.array(pl['W0'][None, None], dtype=dtype))
    np.random.seed(42)
    nmf.fit(np.array(pl['V'], dtype=dtype), n_iterations=0, keep_W=True)
    det = Detections(sample=pl['sample'], atom=np.zeros(K0, dtype=np.int64), transform=pl['t'], shift=pl['shift'],
                     origin=pl['shift'] - 4, strength=pl['h'].astype(dtype))
    return nmf, det, pl


def check_planted(nmf, det, pl, u_elem, transforms=None):
    """The closed form of the planted problem.  With y_k = h_k (W0 + c_k Delta) exactly, cbar = sum h^2 c / sum h^2 and
    alpha_k = h_k (c_k - cbar):  mean = W0 + cbar Delta;  y_k - h_k mean = alpha_k Delta, so the scatter is
    Cm = (sum alpha^2 / s2) Delta Delta^T: rank one, first mode +-Delta / |Delta|, variance[0] / total = 1.
    What the arithmetic may add, derived and not measured:
      * a patch differs from y_k by e_k, |e_k|_inf <= eps_y = 2 u_elem max|V| + 27 U max|V| (V and the render R rounded to the
        element type; the 9 roundings of the definition on terms of at most 3 max|V|);
      * the moments: |dS| <= (K + 2) U sum |y_i y_j|, |dg| <= (K + 2) U sum h |y_i|, s2 to (K + 2) U relative: into Cm a
        perturbation of norm E_mom <= (|dS|_F + (2 |g| |dg| + |dg|^2) / s2) / s2 + 3 (K + 2) U |Cm|;
      * Weyl on the other eigenvalues: restricted to the complement of Delta the scatter of the actual patches is
        sum (f_k . x)^2 / s2 with f_k = e_k - h_k ebar, sum |f_k|^2 <= sum |e_k|^2 <= K D eps_y^2, so they are at most
        K D max|e|^2 / s2 + E_mom.  The planted V and the render of the planted rows are exact in the element type
        (asserted in planted(): products of at most 13 bits), so of e_k only the rounding of V that the issue counts is
        charged: the bound asserted is K D (u_elem max|V|)^2 / s2 + E_mom, not the looser one with eps_y;
      * Davis-Kahan on the direction: sin(angle) <= 2 |E| / gap with gap = variance[0] and
        |E| <= E_mom + (2 sqrt(sum alpha^2 |Delta|^2) sqrt(K D) eps_y + K D eps_y^2) / s2;  |mode - Delta / |Delta|| <= 2 sin."""
    W0, Delta, h, c = pl['W0'], pl['Delta'], pl['h'], pl['c']
    K, D = K0, 25
    vmax = pl['V'].max()
    y = h[:, None, None] * (W0 + c[:, None, None] * Delta)
    eps_y = 2 * u_elem * vmax + 27 * U * vmax
    patches = nmf.detection_patches(det)
    assert patches.shape == (K, 1) + A0 and patches.dtype == np.float64
    print(f'planted {transforms}: |patch - h (W0 + c Delta)| / bound {np.abs(patches[:, 0] - y).max() / eps_y:.3g}')
    assert np.all(np.abs(patches[:, 0] - y) <= eps_y)
    np.testing.assert_array_equal(nmf.detection_patches(det, 'cleaned', 'atom'), patches)
    data = nmf.detection_patches(det, source='data')
    assert np.all(np.abs(data - patches) <= eps_y), 'nothing else lies under an occurrence'
    assert np.all(np.abs(nmf.detection_patches(det, source='residual')[:, 0] - (y - h[:, None, None] * W0)) <= eps_y)
    image = nmf.detection_patches(det, frame='image')
    if transforms is None:
        np.testing.assert_array_equal(image, patches)
    else:   # the image frame holds the occurrence as planted: turned
        for k in range(K):
            turned = tr.apply(tr.GROUPS[transforms][pl['t'][k]], y[k])
            assert np.all(np.abs(image[k, 0] - turned) <= eps_y)
        assert np.abs(image - patches).max() > 100 * eps_y
    # the moments and the modes
    S, g, s2, count = nmf.atom_patch_moments(det)
    assert S.shape == (1, D, D) and g.shape == (1, D) and s2.shape == (1,) and count.tolist() == [K]
    assert np.array_equal(S, S.transpose(0, 2, 1))
    mean, modes, var, total = nmf.atom_modes(det)
    assert mean.shape == (1, 1) + A0 and modes.shape == (1, 3, 1) + A0 and var.shape == (1, 3) and total.shape == (1,)
    assert nmf.atom_modes_info_['count'].tolist() == [K] and nmf.atom_modes_info_['s2'].tobytes() == s2.tobytes()
    for got, want in zip(modes_from_moments(S, g, s2, count, 3), (mean.reshape(1, D), modes.reshape(1, 3, D), var, total)):
        np.testing.assert_array_equal(got, want)
    s2x = np.sum(h * h)
    cbar = np.sum(h * h * c) / s2x
    alpha = h * (c - cbar)
    lam = np.sum(alpha ** 2) * np.sum(Delta ** 2) / s2x
    yf = y.reshape(K, D)
    dS = np.linalg.norm((K + 2) * U * np.abs(yf).T @ np.abs(yf))
    dg = np.linalg.norm((K + 2) * U * h @ np.abs(yf))
    gn = np.linalg.norm(h @ yf)
    E_mom = (dS + (2 * gn * dg + dg * dg) / s2x) / s2x + 3 * (K + 2) * U * lam
    weyl = K * D * (u_elem * vmax) ** 2 / s2x + E_mom
    E = E_mom + (2 * np.sqrt(np.sum(alpha ** 2) * np.sum(Delta ** 2)) * np.sqrt(K * D) * eps_y + K * D * eps_y ** 2) / s2x
    mean_bound = (np.sum(h) * eps_y + (K + 2) * U * np.sum(h[:, None] * np.abs(yf), axis=0).max()) / s2x \
        + 3 * (K + 2) * U * np.abs(W0).max()
    want_mode = Delta / np.linalg.norm(Delta)
    want_mode = want_mode if want_mode.reshape(-1)[np.argmax(np.abs(want_mode))] > 0 else -want_mode
    print(f'planted {transforms}: |mean - ref| / bound {np.abs(mean[0, 0] - (W0 + cbar * Delta)).max() / mean_bound:.3g}, '
          f'other eigenvalues / bound {var[0, 1:].max() / weyl:.3g}, |mode - ref| / bound '
          f'{np.linalg.norm(modes[0, 0, 0] - want_mode) / (4 * E / lam):.3g}, 1 - variance / total '
          f'{1 - var[0, 0] / total[0]:.3g}')
    assert np.all(np.abs(mean[0, 0] - (W0 + cbar * Delta)) <= mean_bound)
    assert abs(var[0, 0] - lam) <= E and np.all(var[0, 1:] <= weyl)
    assert np.linalg.norm(modes[0, 0, 0] - want_mode) <= 4 * E / lam
    assert abs(1 - var[0, 0] / total[0]) <= (D - 1) * weyl / (lam - E)
    return patches, (S, g, s2, count)


def check_additive(tag, whole, parts, bounds):
    """The moments of two disjoint parts of a list sum to those of the list, within ``bounds`` (per moment, broadcast over
    the atoms); prints the largest ratio of a difference to its bound."""
    worst = 0.
    for w, a, b, bound in zip(whole, *parts, bounds):
        err, bound = np.abs(a + b - w), np.broadcast_to(bound, w.shape)
        assert np.all(err <= bound)
        if np.any(bound > 0):
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
    print(f'{tag}: |moments of the halves - moments of the list| / bound {worst:.3g}')


@pytest.mark.parametrize('transforms', [None, 'rot90'])
def test_the_planted_problem_on_the_host(transforms):
    nmf, det, pl = planted_model(transforms)
    assert np.array_equal(nmf.W[0, 0], pl['W0'])
    if transforms is not None:
        assert set(pl['t'].tolist()) == {0, 1, 2, 3}
    _, mom = check_planted(nmf, det, pl, 2. ** -53, transforms)
    if transforms is not None:   # the image frame does not align: its scatter is not of rank one
        image = nmf.detection_patches(det, frame='image')
        S, g, s2, count = ph.patch_moments_numpy(image, pl['h'], np.zeros(K0, dtype=np.int64), 1)
        _, _, var, total = modes_from_moments(S, g, s2, count, 3)
        assert var[0, 1] > 1e-3 * var[0, 0]
    # the moments are additive: two halves of det sum to det, within the summation bound
    halves = [dataclasses.replace(det, **{f.name: getattr(det, f.name)[sel] for f in dataclasses.fields(Detections)})
              for sel in (slice(0, 11), slice(11, None))]
    parts = [nmf.atom_patch_moments(half) for half in halves]
    y = np.abs(nmf.detection_patches(det).reshape(K0, -1))
    bounds = ((K0 + 2) * U * y.T @ y, (K0 + 2) * U * pl['h'] @ y, (K0 + 2) * U * np.sum(pl['h'] ** 2), 0.)
    check_additive(f'planted {transforms}', mom, parts, bounds)
    # max_rows is the hip backend's chunk length: the result does not depend on it
    for a, b in zip(nmf.atom_patch_moments(det, max_rows=_lib.EVENT_SEGMENT), mom):
        np.testing.assert_array_equal(a, b)


def test_the_refusals_are_those_of_the_list_operations():
    nmf, det, _ = planted_model()
    calls = (lambda m: m.detection_patches(det), lambda m: m.atom_patch_moments(det), lambda m: m.atom_modes(det))
    for kw in (dict(source='clean'), dict(source=None), dict(frame='plane'), dict(frame=0)):
        with pytest.raises(ValueError):
            nmf.detection_patches(det, **kw)
    for kw in (dict(n_modes=0), dict(n_modes=26), dict(n_modes=1.5), dict(n_modes=True), dict(source='x')):
        with pytest.raises(ValueError):
            nmf.atom_modes(det, **kw)
    # more modes than C * prod(atom_shape) are refused before the pass over the list
    passes = []
    nmf.atom_patch_moments = lambda *a, **k: passes.append(a)
    try:
        with pytest.raises(ValueError):
            nmf.atom_modes(det, n_modes=26)
    finally:
        del nmf.atom_patch_moments
    assert not passes and nmf.atom_modes(det, n_modes=25)[1].shape == (1, 25, 1) + A0
    for kw in (dict(max_rows=0), dict(max_rows=2.5), dict(source='')):
        with pytest.raises(ValueError):
            nmf.atom_patch_moments(det, **kw)
    unfitted = TransformInvariantNMF(n_atoms=1, atom_shape=A0, backend=_Stub())
    for call in calls:
        with pytest.raises(RuntimeError):
            call(unfitted)
        for name, value in (('_beta', 1.), ('_weighted', True)):
            old = getattr(nmf, name)
            setattr(nmf, name, value)
            try:
                with pytest.raises(NotImplementedError):
                    call(nmf)
            finally:
                setattr(nmf, name, old)
    vol = fitted((1, 1, 5, 5, 5), 1, (2, 2, 2))
    vdet = vol.detections(threshold=float(np.quantile(vol.H, 0.9)), min_distance=0)
    for call in (lambda m: m.detection_patches(vdet), lambda m: m.atom_patch_moments(vdet), lambda m: m.atom_modes(vdet)):
        with pytest.raises(NotImplementedError):
            call(vol)
    # duplicates are allowed, and an empty list gives empty patches, zero moments and NaN modes
    none = dataclasses.replace(det, **{f.name: getattr(det, f.name)[:0] for f in dataclasses.fields(Detections)})
    assert nmf.detection_patches(none).shape == (0, 1) + A0
    S, g, s2, count = nmf.atom_patch_moments(none)
    assert not S.any() and not g.any() and not s2.any() and not count.any()
    assert np.isnan(nmf.atom_modes(none)[1]).all()
    twice = dataclasses.replace(det, **{f.name: np.concatenate([getattr(det, f.name)] * 2)
                                        for f in dataclasses.fields(Detections)})
    assert nmf.detection_patches(twice, source='data').shape == (2 * K0, 1) + A0


def test_a_fitted_model_in_every_mode_matches_the_reference():
    """The front end's rows (shuffle, shard, plane = atom * T + transform) reach the host functions as the reference reads
    them: 'cleaned' patches in the atom frame of a fitted rot90 model in 'circular' mode."""
    nmf = fitted((2, 1, 8, 8), 2, (3, 3), 'circular', transforms='rot90')
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)), min_distance=0)
    assert len(det) > 10 and len(set(det.transform.tolist())) > 1
    W = np.asarray(nmf.transformed_atoms, dtype=np.float64).reshape((-1,) + nmf.W.shape[1:])
    rows = np.column_stack([det.sample, det.atom * 4 + det.transform, det.shift])
    V = np.asarray(nmf.V, dtype=np.float64)
    R = pref.render(W, V.shape[2:], len(V), 'circular', rows, det.strength)
    x, mag, _ = pref.patches(V, R, W, 'circular', rows, det.strength, 'cleaned')
    bound = (pref.ROUNDINGS['cleaned'] + 4 * len(rows)) * U * mag
    y, by = pref.fold(x, bound, rows[:, 1], ph.fold_table('rot90', (3, 3)))
    got = nmf.detection_patches(det)
    assert np.all(np.abs(got - y) <= by) and np.abs(y).max() > 0
    S, g, s2, count = nmf.atom_patch_moments(det)
    rS, rg, rs2, rcount, Sm, gm = pref.moments(got, det.strength, det.atom, 2)
    Km = rcount[:, None, None]
    assert np.array_equal(count, rcount) and np.all(np.abs(S - rS) <= (Km + 2) * U * Sm)
    assert np.all(np.abs(g - rg) <= (Km[:, 0] + 2) * U * gm)


# -- 4. the ABI -------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_typed():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tnmf_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    vp, ll, ci = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    gp = ctypes.POINTER(_lib.Geom)
    for name, argtypes in (('tnmf_hip_events_patches', [vp, gp, ci, ci, vp, vp, vp, ll, vp, vp, vp, vp, vp, ci, vp, vp]),
                           ('tnmf_hip_patch_moments', [vp, ci, ci, vp, vp, vp, vp, ll, ci, vp, vp, vp, vp, vp])):
        assert re.search(r'\bint %s\s*\(' % name, header)
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is ci and list(fn.argtypes) == argtypes
    assert _lib.ABI_VERSION == 8 and lib.tnmf_hip_abi_version() == 8
    assert 'patches.hip' in open(os.path.join(ROOT, 'tnmf_amd', 'csrc', 'Makefile')).read()
    # argument errors are answered without a device: no context
    g = _lib.make_geom(1, 1, 1, (4,), (2,), 0)
    assert lib.tnmf_hip_events_patches(None, ctypes.byref(g), 0, 0, None, None, None, 0, None, None, None, None, None, 1,
                                       None, None) == -1
    assert lib.tnmf_hip_patch_moments(None, 4, 1, None, None, None, None, 0, 0, None, None, None, None, None) == -1
