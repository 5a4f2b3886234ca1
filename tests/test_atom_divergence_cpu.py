"""
atom_divergence_terms() / atom_divergence_gains() / atom_divergence_gram() on the CPU: the host fallbacks
(tnmf_amd/atoms_host.py) against the reference (tests/atom_divergence_reference.py), and through the front end on a stub
backend without the hooks against two statements that need no reference: the gain is the difference of two objectives, and
``-a`` and ``b`` are the first and second derivative of the objective in an atom's scale factor.  Float64 throughout.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import atom_divergence_reference as dref
import atoms_reference as aref
import events_reference as eref
from conftest import ROOT
from test_atom_gains_cpu import _AtomStub, snapshot, weights_of
from test_events_cpu import fitted
from tnmf_amd import _lib
from tnmf_amd.atoms_host import atom_divergence_gram_numpy, atom_divergence_terms_numpy
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

MODES = ['valid', 'full', 'circular', 'reflect']
BETAS = [0., 1., 0.5, 1.5, 3.]
RTOL = 1e-12
EPS = 1e-9


class _DivergenceStub(_AtomStub):
    """``_AtomStub`` with the beta-divergence objective per sample, weighted when weights are bound -- and none of the atom
    hooks: the front end scores the atoms on the host."""

    supports_beta_loss = True

    def sample_objective(self, V, W, H, beta=2., eps=1e-9):
        V, R = self._V_local, self.reconstruct(W, H)
        g = np.ones(V.shape) if self._G is None else np.where(self._G > 0, self._G, 0.)
        d = 0.5 * (V - R) ** 2 if beta == 2 else dref.element(V, np.maximum(R, 0.) + eps, beta)
        return np.sum(np.where(g > 0, g * d, 0.), axis=tuple(range(1, V.ndim)))

    def reconstruction_energy(self, V, W, H, beta=2., eps=1e-9):
        return float(np.sum(self.sample_objective(V, W, H, beta, eps)))


def model(shape_V, n_atoms, atom_shape, beta, mode='valid', weights=None, transforms=None, seed=0):
    V = np.random.default_rng(seed).random(shape_V) + 0.05
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=n_atoms, atom_shape=atom_shape, backend=_DivergenceStub(mode), transforms=transforms,
                                beta_loss=beta)
    nmf.fit(V, n_iterations=2, sparsity_H=0.1, update_W=False, weights=weights)
    return nmf


# -- 1. the host fallbacks against the reference ---------------------------------------------------------------------------
CASES = {'1d-c1': ((3, 1, 25), (5,)), '2d-c3': ((2, 3, 8, 9), (3, 3))}


@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('kind', [None, 'mask', 'real'], ids=str)
@pytest.mark.parametrize('group', [1, 2])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', list(CASES))
def test_the_fallbacks_equal_the_reference(case, mode, group, kind, beta):
    shape_V, A = CASES[case]
    rng = np.random.default_rng(7)
    D = shape_V[2:]
    W = rng.random((4, shape_V[1]) + A)
    H = rng.random((shape_V[0], 4) + eref.shift_shape(D, A, mode)) * (rng.random((shape_V[0], 4) + (1,) * len(A)) > 0.2)
    V, G = rng.random(shape_V) + 0.05, weights_of(shape_V, kind)
    if kind == 'mask':
        V = np.where(G > 0, V, np.nan)   # what a mask hides is not data
    parts = aref.parts_loop(W, H, D, mode, group)
    ref = dref.terms(parts, V, G, None, beta, EPS)
    a, b, gain = atom_divergence_terms_numpy(W, H, mode, V, G, group, beta, EPS)
    assert a.shape == b.shape == gain.shape == (shape_V[0], 4 // group)
    for name, got in (('a', a), ('b', b), ('gain', gain)):
        err = np.abs(got - ref[name])
        assert np.all(err <= RTOL * ref['scale_' + name]), (name, float(np.max(err / ref['scale_' + name])))
    a2, B = atom_divergence_gram_numpy(W, H, mode, V, G, group, beta, EPS)
    Bref, Bscale = dref.gram(parts, V, G, None, beta, EPS)
    np.testing.assert_array_equal(a2, a)
    assert np.all(np.abs(B - Bref) <= RTOL * Bscale)
    np.testing.assert_array_equal(B, B.transpose(0, 2, 1))
    np.testing.assert_array_equal(np.diagonal(B, axis1=1, axis2=2), b)


def test_the_curvature_is_negative_somewhere_outside_beta_1_to_2_and_nowhere_inside():
    rng = np.random.default_rng(1)
    R = rng.random((2, 1, 9, 9)) + 0.1
    V = R * (0.25 + 2.5 * rng.random(R.shape))
    for beta, some in ((0., True), (0.5, True), (1., False), (1.5, False), (3., True)):
        neg, live = dref.curvature_is_negative(V, R, None, beta, EPS)
        assert (neg > 0) == some and live == R.size


# -- 2. through the front end: the gain is a difference of two objectives ---------------------------------------------------
FRONT = {   # shape of V, atoms, atom shape, transforms
    '1d-c3': ((2, 3, 19), 2, (4,), None),
    '2d-c1': ((2, 1, 9, 10), 3, (3, 4), None),
    'rot90': ((2, 1, 8, 8), 2, (3, 3), 'rot90'),
}


def without_atom(nmf, m):
    """sample_objective() with the planes of atom m at 0; H is restored."""
    T = nmf.n_transforms
    keep = np.array(nmf._H[:, m * T:(m + 1) * T])
    nmf._H[:, m * T:(m + 1) * T] = 0.
    try:
        return nmf.sample_objective()
    finally:
        nmf._H[:, m * T:(m + 1) * T] = keep


@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('kind', [None, 'mask', 'real'], ids=str)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', list(FRONT))
def test_the_gain_is_the_objective_without_the_atom_minus_the_objective(case, mode, kind, beta):
    shape_V, M, A, t = FRONT[case]
    nmf = model(shape_V, M, A, beta, mode, weights_of(shape_V, kind), t)
    before = snapshot(nmf)
    got = nmf.atom_divergence_gains(per_sample=True)
    assert got.shape == (shape_V[0], M) and got.dtype == np.float64
    base = nmf.sample_objective()
    for m in range(M):
        gone = without_atom(nmf, m)
        # two sums of at most a few hundred non-negative float64 terms each: 1e-12 of their sum covers the subtraction
        assert np.all(np.abs(got[:, m] - (gone - base)) <= 1e-12 * (gone + base)), (m, got[:, m], gone - base)
    np.testing.assert_array_equal(nmf.atom_divergence_gains(), got.sum(axis=0))
    for was, now in zip(before, snapshot(nmf)):
        np.testing.assert_array_equal(was, now)


@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('kind', [None, 'real'], ids=str)
@pytest.mark.parametrize('case', list(FRONT))
def test_finite_differences_in_an_atoms_scale_factor_give_minus_a_and_b(case, kind, beta):
    shape_V, M, A, t = FRONT[case]
    nmf = model(shape_V, M, A, beta, 'reflect', weights_of(shape_V, kind), t)
    a, b = nmf.atom_divergence_terms()
    B = nmf.atom_divergence_gram(per_sample=True)
    np.testing.assert_array_equal(np.diagonal(B, axis1=1, axis2=2), b)
    T, h = nmf.n_transforms, 1e-4
    base = nmf.sample_objective()
    for m in range(M):
        planes = slice(m * T, (m + 1) * T)
        keep = np.array(nmf._H[:, planes])
        try:
            nmf._H[:, planes] = keep * (1. + h)
            up = nmf.sample_objective()
            nmf._H[:, planes] = keep * (1. - h)
            down = nmf.sample_objective()
        finally:
            nmf._H[:, planes] = keep
        first, second = (up - down) / (2. * h), (up - 2. * base + down) / (h * h)
        ea = np.abs(first + a[:, m]) / np.abs(a[:, m])
        eb = np.abs(second - b[:, m]) / np.abs(b[:, m])
        print(f'finite differences {case} beta={beta} atom {m}: relative error of -a {ea.max():.2e}, of b {eb.max():.2e}')
        assert np.all(ea <= 1e-6) and np.all(eb <= 1e-6)


# -- 3. beta 2 is the Frobenius family, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [None, 'real'], ids=str)
@pytest.mark.parametrize('case', list(FRONT))
def test_at_beta_2_the_three_methods_are_the_frobenius_ones(case, kind):
    shape_V, M, A, t = FRONT[case]
    nmf = model(shape_V, M, A, 2., 'circular', weights_of(shape_V, kind), t)
    for got, want in zip(nmf.atom_divergence_terms(), nmf.atom_terms()):
        assert got.tobytes() == want.tobytes()
    for per_sample in (False, True):
        assert nmf.atom_divergence_gains(per_sample).tobytes() == nmf.atom_gains(per_sample).tobytes()
        assert nmf.atom_divergence_gram(per_sample).tobytes() == nmf.atom_gram(per_sample).tobytes()
    # and so are the fallbacks called with beta 2
    rng = np.random.default_rng(3)
    W, H, V = rng.random((2, 1, 3)), rng.random((2, 2, 9)), rng.random((2, 1, 7))
    a, b, gain = atom_divergence_terms_numpy(W, H, 'valid', V, None, 1, 2., EPS)
    np.testing.assert_array_equal(gain, a + 0.5 * b)


# -- 4. the order of the samples, refusals ----------------------------------------------------------------------------------
def test_samples_come_in_the_order_of_H_under_a_shuffle():
    nmf = model((5, 1, 9, 8), 2, (3, 3), 1.)
    plain = nmf.atom_divergence_gains(per_sample=True)
    a, b = nmf.atom_divergence_terms()
    B = nmf.atom_divergence_gram(per_sample=True)
    nmf._shuffle_idx = np.array([3, 0, 4, 1, 2])
    try:
        order = np.argsort(nmf._shuffle_idx)
        np.testing.assert_array_equal(nmf.atom_divergence_gains(per_sample=True), plain[order])
        for got, want in zip(nmf.atom_divergence_terms(), (a, b)):
            np.testing.assert_array_equal(got, want[order])
        np.testing.assert_array_equal(nmf.atom_divergence_gram(per_sample=True), B[order])
    finally:
        nmf._shuffle_idx = None


def test_refusals_leave_the_model_as_it_was():
    for name in ('atom_divergence_terms', 'atom_divergence_gains', 'atom_divergence_gram'):
        with pytest.raises(RuntimeError):
            getattr(TransformInvariantNMF(n_atoms=2, atom_shape=(3, 4), backend=_DivergenceStub(), beta_loss=1.), name)()
    nmf = model((2, 1, 9, 10), 2, (3, 4), 1., 'reflect')
    before = snapshot(nmf)
    for bad in ('yes', 1, 0, None, 1.0):
        with pytest.raises(ValueError):
            nmf.atom_divergence_gains(per_sample=bad)
        with pytest.raises(ValueError):
            nmf.atom_divergence_gram(per_sample=bad)
    assert nmf.atom_divergence_gains(per_sample=np.bool_(True)).shape == (2, 2)
    assert nmf.atom_divergence_gram().shape == (2, 2)
    # the refusals of the Frobenius family stay as they are
    with pytest.raises(NotImplementedError, match=r'atom_gains covers the Frobenius objective'):
        nmf.atom_gains()
    for was, now in zip(before, snapshot(nmf)):
        np.testing.assert_array_equal(was, now)


def test_volumes_are_refused():
    nmf = fitted((1, 1, 5, 5, 5), 1, (2, 2, 2))
    for name in ('atom_divergence_terms', 'atom_divergence_gains', 'atom_divergence_gram'):
        with pytest.raises(NotImplementedError):
            getattr(nmf, name)()


# -- 5. the ABI ---------------------------------------------------------------------------------------------------------------
def test_both_entry_points_are_declared_exported_and_built():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tnmf_hip.h')).read(), flags=re.S)
    makefile = open(os.path.join(ROOT, 'tnmf_amd', 'csrc', 'Makefile')).read()
    for entry, source in (('tnmf_hip_atom_terms_beta', 'atoms_beta.hip'), ('tnmf_hip_atom_gram_beta', 'atom_gram_beta.hip')):
        assert re.search(rf'\bint {entry}\s*\(', header) and entry in _lib.EXPORTS
        assert re.search(rf'^SRCS\s*:=.*\b{re.escape(source)}\b', makefile, flags=re.M)
    assert re.search(r'^HDRS\s*:=.*\batom_beta\.h\b', makefile, flags=re.M)
    assert re.search(r'^HDRS\s*:=.*\batom_gram_kernel\.h\b', makefile, flags=re.M)   # the kernel text both Gram files include
    assert _lib.ABI_VERSION == 8
    lib = _lib.load()
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    gp = ctypes.POINTER(_lib.Geom)
    assert list(lib.tnmf_hip_atom_terms_beta.argtypes) == [vp, gp, ci, cd, cd, vp, vp, vp, vp, vp, vp, vp]
    assert list(lib.tnmf_hip_atom_gram_beta.argtypes) == [vp, gp, ci, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp]
    g = _lib.make_geom(1, 1, 1, (4,), (2,), 0)   # an argument error is answered without a device: no context
    assert lib.tnmf_hip_atom_terms_beta(None, ctypes.byref(g), 1, 1., 1e-9, None, None, None, None, None, None, None) == -1
    assert lib.tnmf_hip_atom_gram_beta(None, ctypes.byref(g), 1, 1., 1e-9, None, None, None, None, None, None, None,
                                       None) == -1
