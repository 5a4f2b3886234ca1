"""
atom_gram() and what builds on it (atom_overlaps, atom_set_gain, atom_scales, rescale_atoms, atom_elimination) on the CPU: the
host fallback (tnmf_amd/atoms_host.py) directly and through the front end on an oracle backend without the ``atom_gram`` hook,
against brute force -- ``R_partial`` products, objectives recomputed with activations zeroed or rescaled, every active set of
the non-negative solve.  Float64 throughout; every bound is relative 1e-10 of the size of the terms.
"""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_atom_gains_cpu import CASES, MODES, _AtomStub, model, snapshot, transforms_of, weights_of
from test_events_cpu import fitted
from tnmf_amd import _lib
from tnmf_amd.atoms_host import (atom_gram_numpy, atom_terms_numpy, gram_drop, gram_elimination, gram_scales,
                                 gram_set_gain)
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

RTOL = 1e-10


def brute_gram(nmf, G):
    """B[n, m, m'] = sum G R_m R_m' from R_partial, per sample."""
    g = np.ones(nmf.V.shape) if G is None else G
    parts = [nmf.R_partial(m) for m in range(nmf.n_atoms)]
    axes = tuple(range(1, nmf.V.ndim))
    return np.stack([np.stack([np.sum(g * p * q, axis=axes) for q in parts], axis=1) for p in parts], axis=1)


def objective_with(nmf, scales):
    """The objective with the activations of atom m multiplied by scales[m]; the model is left as it was."""
    T, keep = nmf.n_transforms, nmf._H.copy()
    try:
        for m, s in enumerate(scales):
            nmf._H[:, m * T:(m + 1) * T] *= s
        return nmf.objective()
    finally:
        nmf._H[...] = keep


def without(nmf, atoms):
    return objective_with(nmf, [0. if m in atoms else 1. for m in range(nmf.n_atoms)])


# -- 1. the definition ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [None, 'mask', 'real'], ids=str)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', ['1d-c3', '2d-c1', 'rot90-c3', 'operators'])
def test_the_gram_matrix_is_the_products_of_the_partial_reconstructions(case, mode, kind):
    shape_V, M, A, t = CASES[case]
    G = weights_of(shape_V, kind)
    nmf = model(shape_V, M, A, mode, G, transforms_of(t, A))
    want = brute_gram(nmf, G)
    got = nmf.atom_gram(per_sample=True)
    assert got.shape == (shape_V[0], M, M) and got.dtype == np.float64
    d = np.sqrt(np.diagonal(want, axis1=1, axis2=2))
    assert np.all(np.abs(got - want) <= RTOL * d[:, :, None] * d[:, None, :])
    np.testing.assert_array_equal(got, got.transpose(0, 2, 1))
    np.testing.assert_array_equal(nmf.atom_gram(), got.sum(axis=0))
    # the diagonal is b, and a is the a of the atom terms: the same numbers
    a, b = nmf.atom_terms()
    np.testing.assert_array_equal(np.diagonal(got, axis1=1, axis2=2), b)
    np.testing.assert_array_equal(nmf._atom_gram()[0], a)


@pytest.mark.parametrize('group', [1, 2, 4])
@pytest.mark.parametrize('mode', MODES)
def test_the_fallback_shares_a_and_the_diagonal_with_the_atom_terms(mode, group):
    import events_reference as eref
    rng = np.random.default_rng(11)
    D, A = (7, 6), (3, 2)
    W, V = rng.random((4, 2) + A), rng.random((3, 2) + D)
    H = rng.random((3, 4) + eref.shift_shape(D, A, mode))
    G = weights_of(V.shape, 'mask')
    a, B = atom_gram_numpy(W, H, mode, np.where(G > 0, V, np.nan), G, group)   # (what a mask hides is not data)
    ta, tb = atom_terms_numpy(W, H, mode, V, G, group)
    assert B.shape == (3, 4 // group, 4 // group) and np.all(np.isfinite(B))
    np.testing.assert_array_equal(a, ta)
    np.testing.assert_array_equal(np.diagonal(B, axis1=1, axis2=2), tb)
    with pytest.raises(ValueError):
        atom_gram_numpy(W, H, mode, V, G, 3)


# -- 2. sets of atoms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [None, 'real'], ids=str)
@pytest.mark.parametrize('mode', ['valid', 'reflect'])
def test_the_gain_of_a_set_is_the_objective_without_it_minus_the_objective(mode, kind):
    shape_V = (2, 2, 9, 10)
    G = weights_of(shape_V, kind)
    nmf = model(shape_V, 4, (3, 3), mode, G)
    base = nmf.objective()
    energy = 0.5 * float(np.sum((1. if G is None else G) * nmf.V ** 2))
    for k in range(1, 5):
        for S in itertools.combinations(range(4), k):
            assert abs(nmf.atom_set_gain(S) - (without(nmf, S) - base)) <= RTOL * energy, S
    gains = nmf.atom_gains()
    for m in range(4):
        assert abs(nmf.atom_set_gain([m]) - gains[m]) <= RTOL * abs(gains[m])
    assert nmf.atom_set_gain([]) == 0.
    assert nmf.atom_set_gain(np.array([2, 0])) == nmf.atom_set_gain((0, 2))
    for bad in ([0, 0], [4], [-1], [0.5], [True], 'ab', 3, [None]):
        with pytest.raises(ValueError):
            nmf.atom_set_gain(bad)


# -- 3. joint scale factors ---------------------------------------------------------------------------------------------------
def brute_scales(a, B, nonnegative=True):
    """The least E over every active set: (value of 1/2 s^T B s - c^T s, s)."""
    M = len(a)
    c = a + B @ np.ones(M)
    best = None
    for k in range(M + 1):
        for P in itertools.combinations(range(M), k):
            z, P = np.zeros(M), list(P)
            if P:
                z[P] = np.linalg.lstsq(B[np.ix_(P, P)], c[P], rcond=None)[0]
            if (np.all(z >= 0) or not nonnegative) and (best is None or 0.5 * z @ B @ z - c @ z < best[0]):
                best = (0.5 * z @ B @ z - c @ z, z)
    return best


def synthetic(rng, M, duplicate=False, dead=False):
    X = rng.random((M, 9)) * (rng.random((M, 9)) > 0.4)
    if duplicate and M > 1:
        X[1] = X[0]
    if dead:
        X[-1] = 0.
    v = 3. * rng.random(9) - 0.5
    return X @ (v - X.sum(axis=0)), X @ X.T


def test_the_scales_against_brute_force_over_all_active_sets():
    rng = np.random.default_rng(2)
    some_at_zero = 0
    for trial in range(240):
        M = 1 + trial % 6
        a, B = synthetic(rng, M, duplicate=trial % 4 == 1, dead=trial % 5 == 2)
        s = gram_scales(a, B)
        assert s.shape == (M,) and np.all(s >= 0)
        live = np.diag(B) > 0
        assert np.all(s[~live] == 1.)
        c = a + B @ np.ones(M)
        z = np.where(live, s, 0.)
        value, (want, zb) = 0.5 * z @ B @ z - c @ z, brute_scales(a, B)
        assert abs(value - want) <= RTOL * max(abs(want), float(np.abs(c) @ np.abs(zb))), (trial, value, want)
        if np.linalg.cond(B[np.ix_(live, live)]) < 1e6 if live.any() else False:   # the minimiser is unique
            np.testing.assert_allclose(z, zb, rtol=1e-6, atol=1e-9)
        some_at_zero += bool(np.any(z[live] == 0))
        free = gram_scales(a, B, nonnegative=False)
        zf = np.where(live, free, 0.)
        assert np.all(np.abs(B @ zf - c) <= 1e-9 * (np.abs(B) @ np.abs(zf) + np.abs(c)))   # the normal equations
    assert some_at_zero >= 20   # (the constraint was active often enough to be tested)


def test_the_scales_of_a_model_against_brute_force():
    for M, shape_V, A in ((1, (2, 1, 20), (4,)), (3, (2, 2, 9, 10), (3, 3)), (6, (2, 1, 9, 10), (3, 4))):
        nmf = model(shape_V, M, A, 'reflect', weights_of(shape_V, 'real'), n_iterations=1)
        a, B = (x.sum(axis=0) for x in nmf._atom_gram())
        s = nmf.atom_scales()
        c = a + B @ np.ones(M)
        value, (want, _) = 0.5 * s @ B @ s - c @ s, brute_scales(a, B)
        assert abs(value - want) <= RTOL * abs(want)
        np.testing.assert_array_equal(s, gram_scales(a, B))
        np.testing.assert_array_equal(nmf.atom_scales(nonnegative=False), gram_scales(a, B, False))
        for bad in ('yes', 1, None):
            with pytest.raises(ValueError):
                nmf.atom_scales(nonnegative=bad)


def test_dead_atoms_keep_scale_one_and_duplicates_share_the_load():
    nmf = model((2, 1, 9, 10), 4, (3, 3), 'valid')
    nmf._H[:, 3] = 0.                 # atom 3 is dead
    nmf._W[1] = nmf._W[0]             # atoms 0 and 1 are exact duplicates with the same activations
    nmf._H[:, 1] = nmf._H[:, 0]
    B = nmf.atom_gram()
    assert np.all(B[3] == 0.) and np.all(B[:, 3] == 0.) and B[0, 0] == B[1, 1]
    assert abs(B[0, 1] - B[0, 0]) <= 1e-14 * B[0, 0]   # (the diagonal is summed as b is, the rest as a matrix product)
    ov = nmf.atom_overlaps()
    assert abs(ov[0, 1] - 1.) <= 1e-14 and np.all(ov[3] == 0.) and np.all(ov[:, 3] == 0.) and np.all(np.diag(ov)[:3] == 1.)
    assert np.all(ov <= 1. + 1e-12) and np.all(ov >= 0.)
    s = nmf.atom_scales()
    assert s[3] == 1. and abs(s[0] - s[1]) <= 1e-9 * s[0] and s[0] > 0        # minimum norm: the pair shares its load
    # ... and the pair's joint factor is what one of them alone would get with the other folded in
    a, Bm = (x.sum(axis=0) for x in nmf._atom_gram())
    keep = [0, 2]
    a2, B2 = a[keep].copy(), Bm[np.ix_(keep, keep)].copy()
    a2[0], B2[0, 0], B2[0, 1], B2[1, 0] = 2 * a[0], 4 * Bm[0, 0], 2 * Bm[0, 2], 2 * Bm[0, 2]
    np.testing.assert_allclose(gram_scales(a2, B2), s[keep], rtol=1e-8)
    assert gram_scales(np.zeros(2), np.zeros((2, 2))).tolist() == [1., 1.]
    # a shifted copy: atom 1 is atom 0 moved one column inside its window, and H absorbs the shift
    nmf = model((2, 1, 9, 10), 2, (3, 4), 'full')
    nmf._W[0, :, :, 0] = 0.
    nmf._W[1] = np.roll(nmf._W[0], -1, axis=-1)
    nmf._H[:, 1] = 0.
    nmf._H[:, 1, :, 1:] = nmf._H[:, 0, :, :-1]
    nmf._H[:, 0, :, -1] = 0.
    assert abs(nmf.atom_overlaps()[0, 1] - 1.) <= 1e-12


# -- 4. applying them ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', [None, 'rot90'], ids=str)
@pytest.mark.parametrize('kind', [None, 'real'], ids=str)
def test_rescale_atoms_lowers_the_objective_by_what_it_returns(kind, t):
    shape_V = (2, 1, 9, 9)
    G = weights_of(shape_V, kind)
    nmf = model(shape_V, 3, (3, 3), 'circular', G, t)
    before, W, H = nmf.objective(), nmf.W.copy(), nmf.H.copy()
    s = nmf.atom_scales()
    drop = nmf.rescale_atoms()
    assert drop >= 0 and abs((before - nmf.objective()) - drop) <= RTOL * before
    np.testing.assert_array_equal(nmf.atom_scales_, s)
    np.testing.assert_array_equal(nmf.W, W)
    shape = (1, 3) + (1,) * (H.ndim - 2)
    np.testing.assert_allclose(nmf.H, H * s.reshape(shape), rtol=1e-15)
    # at the optimum the factors are 1 and nothing is left to gain
    np.testing.assert_allclose(nmf.atom_scales(), 1., atol=1e-8)
    assert abs(nmf.rescale_atoms()) <= RTOL * before
    # given factors: the same exact quadratic
    before = nmf.objective()
    given = np.array([0.5, 1., 2.])
    drop = nmf.rescale_atoms(given)
    assert drop < 0 and abs((before - nmf.objective()) - drop) <= RTOL * before
    np.testing.assert_array_equal(nmf.atom_scales_, given)
    keep = snapshot(nmf)
    for bad in ([1., 1.], [1., -1., 1.], [1., np.nan, 1.], 'abc', [[1., 1., 1.]]):
        with pytest.raises(ValueError):
            nmf.rescale_atoms(bad)
    for was, now in zip(keep, snapshot(nmf)):
        np.testing.assert_array_equal(was, now)


def test_rescale_atoms_with_a_process_group_needs_the_scales():
    nmf = model((2, 1, 9, 9), 2, (3, 3))
    nmf._backend._world = 2
    keep = snapshot(nmf)
    def no_pass(*_):
        raise AssertionError('the pass over H ran before the refusal')
    nmf._backend.atom_gram = no_pass
    try:
        with pytest.raises(NotImplementedError, match='needs the scales'):
            nmf.rescale_atoms()
    finally:
        del nmf._backend.atom_gram
    for was, now in zip(keep, snapshot(nmf)):
        np.testing.assert_array_equal(was, now)
    assert isinstance(nmf.rescale_atoms([1., 0.5]), float)


# -- 5. backward elimination ------------------------------------------------------------------------------------------------------
def test_elimination_against_an_exhaustive_greedy_on_recomputed_objectives():
    shape_V = (2, 2, 9, 10)
    nmf = model(shape_V, 4, (3, 3), 'reflect', weights_of(shape_V, 'real'))
    base, keep = nmf.objective(), snapshot(nmf)
    order, rise = nmf.atom_elimination()
    assert order.dtype == np.int64 and rise.dtype == np.float64 and sorted(order) == [0, 1, 2, 3]
    gone = []
    for k in range(4):
        trials = {m: without(nmf, gone + [m]) - base for m in range(4) if m not in gone}
        best = min(trials, key=trials.get)
        assert order[k] == best and abs(rise[k] - trials[best]) <= RTOL * base * 100
        gone.append(best)
    energy = 0.5 * float(np.sum(weights_of(shape_V, 'real') * nmf.V ** 2))
    assert abs(rise[-1] - (energy - base)) <= RTOL * energy and np.all(np.diff(rise) >= 0)
    # rescale=True: the others are refitted (s >= 0) at every step; checked on objectives recomputed with those factors
    a, B = (x.sum(axis=0) for x in nmf._atom_gram())
    order, rise = nmf.atom_elimination(rescale=True)
    gone = []
    for k in range(4):
        trials = {}
        for m in range(4):
            if m not in gone:
                s = gram_scales(a, B, True, gone + [m])
                assert np.all(s[gone + [m]] == 0.)
                trials[m] = objective_with(nmf, s) - base
                assert abs(trials[m] + gram_drop(a, B, s)) <= RTOL * energy
                # no other non-negative factors of the remaining atoms do better (a coarse scan around the optimum)
                for bump in np.eye(4):
                    if bump[gone + [m]].sum() == 0:
                        for eps in (-1e-3, 1e-3):
                            alt = np.maximum(s + eps * bump, 0.)
                            assert -gram_drop(a, B, alt) >= trials[m] - RTOL * energy
        best = min(trials, key=trials.get)
        assert order[k] == best and abs(rise[k] - trials[best]) <= RTOL * energy
        gone.append(best)
    assert rise[0] <= 0. + RTOL * energy and abs(rise[-1] - (energy - base)) <= RTOL * energy
    np.testing.assert_array_equal(gram_elimination(a, B)[0], nmf.atom_elimination()[0])
    assert gram_set_gain(a, B, [1, 3]) == nmf.atom_set_gain([1, 3])
    for bad in ('yes', 1, None):
        with pytest.raises(ValueError):
            nmf.atom_elimination(rescale=bad)
    for was, now in zip(keep, snapshot(nmf)):
        np.testing.assert_array_equal(was, now)


# -- 6. the order of the samples, refusals ------------------------------------------------------------------------------------
def test_samples_come_in_the_order_of_H_under_a_shuffle():
    nmf = model((5, 1, 9, 8), 2, (3, 3))
    plain = nmf.atom_gram(per_sample=True)
    nmf._shuffle_idx = np.array([3, 0, 4, 1, 2])
    try:
        order = np.argsort(nmf._shuffle_idx)
        np.testing.assert_array_equal(nmf.atom_gram(per_sample=True), plain[order])
        np.testing.assert_allclose(nmf.atom_gram(), plain.sum(axis=0), rtol=1e-14)   # (another order of the sum)
    finally:
        nmf._shuffle_idx = None


CALLS = {
    'atom_gram': lambda m: m.atom_gram(), 'atom_overlaps': lambda m: m.atom_overlaps(),
    'atom_set_gain': lambda m: m.atom_set_gain([0]), 'atom_scales': lambda m: m.atom_scales(),
    'rescale_atoms': lambda m: m.rescale_atoms(), 'rescale_atoms-given': lambda m: m.rescale_atoms([1., 2.]),
    'atom_elimination': lambda m: m.atom_elimination(),
}


@pytest.mark.parametrize('name', list(CALLS))
def test_refusals_are_those_of_atom_terms_and_leave_the_model_as_it_was(name):
    call = CALLS[name]
    with pytest.raises(RuntimeError, match='the atom gains of a model need a fitted model: call fit first'):
        call(TransformInvariantNMF(n_atoms=2, atom_shape=(3, 4), backend=_AtomStub()))
    nmf = model((2, 1, 9, 10), 2, (3, 4), 'reflect')
    before = snapshot(nmf)
    nmf._beta = 1.
    try:
        with pytest.raises(NotImplementedError, match=r'atom_gains covers the Frobenius objective \(beta_loss 2\), with or '
                                                      r'without weights'):
            call(nmf)
    finally:
        nmf._beta = 2.
    vol = fitted((1, 1, 5, 5, 5), 2, (2, 2, 2))
    keep = [np.array(x) for x in (vol.W, vol.H)]
    with pytest.raises(NotImplementedError, match='atom gains: 1 or 2 shift axes only'):
        call(vol)
    for was, now in zip(before + keep, snapshot(nmf) + [vol.W, vol.H]):
        np.testing.assert_array_equal(was, now)
    assert not hasattr(nmf, 'atom_scales_')


def test_per_sample_is_validated_like_atom_gains():
    nmf = model((2, 1, 9, 10), 2, (3, 4))
    for bad in ('yes', 1, 0, None, 1.0):
        with pytest.raises(ValueError, match='per_sample must be a bool'):
            nmf.atom_gram(per_sample=bad)
    assert nmf.atom_gram(per_sample=np.bool_(True)).shape == (2, 2, 2) and nmf.atom_gram().shape == (2, 2)


# -- 7. the ABI ---------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_built():
    text = open(os.path.join(ROOT, 'include', 'tnmf_hip.h')).read()
    assert '---- atom Gram' in text
    header = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'\bint tnmf_hip_atom_gram\s*\(', header) and 'tnmf_hip_atom_gram' in _lib.EXPORTS
    makefile = open(os.path.join(ROOT, 'tnmf_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\batom_gram\.hip\b', makefile, flags=re.M)
    assert re.search(r'^HDRS\s*:=.*\batom_gram\.h\b', makefile, flags=re.M)
    assert _lib.ABI_VERSION == 8
    lib = _lib.load()
    assert lib.tnmf_hip_abi_version() == 8
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert list(lib.tnmf_hip_atom_gram.argtypes) == [vp, ctypes.POINTER(_lib.Geom), ci, vp, vp, vp, vp, vp, vp, vp, vp]
    g = _lib.make_geom(1, 1, 1, (4,), (2,), 0)   # an argument error is answered without a device: no context
    assert lib.tnmf_hip_atom_gram(None, ctypes.byref(g), 1, None, None, None, None, None, None, None, None) == -1
    assert lib.tnmf_hip_atom_gram(None, None, 1, None, None, None, None, None, None, None, None) == -1
