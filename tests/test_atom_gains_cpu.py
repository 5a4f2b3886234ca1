"""
atom_terms() / atom_gains() on the CPU: the host fallback (tnmf_amd/atoms_host.py) directly and through the front end on an
oracle backend without the ``atom_terms`` hook, against the definition evaluated literally and against the naive reference
(atoms_reference.parts_loop).  Float64 throughout; every bound is relative 1e-10 of the sum of the absolute terms.
"""
import os
import re

import numpy as np
import pytest

import atoms_reference as aref
import events_reference as eref
from conftest import ROOT
from oracle import tnmf_oracle as orc
from oracle_backend import OracleBackend
from test_events_cpu import fitted
from tnmf_amd import _lib, sharding, transforms as tr
from tnmf_amd.atoms_host import atom_terms_numpy, pad_activations_numpy
from tnmf_amd.backends._Backend import sliceNone
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

MODES = ['valid', 'full', 'circular', 'reflect']
RTOL = 1e-10


class _AtomStub(OracleBackend):
    """The oracle's primitives in any reconstruction mode, with weights, transform groups and atom operators bound the way
    the hip backend binds them -- and no ``atom_terms`` hook: the front end scores the atoms on the host."""

    supports_weights = True
    supports_transforms = True
    supports_atom_operators = True

    def __init__(self, mode='valid'):
        super().__init__(impl='contract')
        self._reconstruction_mode = mode
        self._G = None

    def _initialize_matrices(self, V, atom_shape, n_atoms, W=None, axes_W_normalization=None, weights=None,
                             transforms=None):
        T = 1 if transforms is None else tr.size(transforms)
        self._shard = (0, V.shape[0])
        self._V_local, self._G = V, weights
        H = np.empty((V.shape[0], n_atoms * T) + self._transform_shape, dtype=V.dtype)
        for i, h in sharding.reference_init_stream(V.shape[0], H.shape[1:], self._shard, V.dtype):
            H[i] = h
        if W is None:
            W = sharding.reference_init_W(n_atoms, self.n_channels, self.atom_shape, V.dtype)
        return W, H

    def reconstruct(self, W, H):
        return orc.reconstruct(W, H, self.impl, self._reconstruction_mode)

    def reconstruction_gradient_H(self, V, W, H, s=sliceNone):
        return orc.gradient_H(self._V_local, W, H, s, self.impl, self._reconstruction_mode)

    def reconstruction_energy(self, V, W, H, beta=2., eps=1e-9):
        g = 1. if self._G is None else self._G
        return 0.5 * float(np.sum(g * (self._V_local - self.reconstruct(W, H)) ** 2))

    def expand_W(self, W, transforms, W_eff=None):
        e = tr.expand(W, transforms)
        if W_eff is None:
            return e
        W_eff[...] = e
        return W_eff

    def fused_update_H(self, V, W, H, s=sliceNone, sparsity=0., eps=1e-9, **_):
        # (a step of the unweighted objective whatever is bound: all these tests need is some (W, H) away from the start)
        neg, pos = self.reconstruction_gradient_H(V, W, H, s)
        orc.multiplicative_update(H[s], neg, pos, eps, sparsity)


def model(shape_V, n_atoms, atom_shape, mode='valid', weights=None, transforms=None, n_iterations=2, seed=0):
    V = np.random.default_rng(seed).random(shape_V) + 0.05
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=n_atoms, atom_shape=atom_shape, backend=_AtomStub(mode), transforms=transforms)
    nmf.fit(V, n_iterations=n_iterations, sparsity_H=0.1, update_W=False, weights=weights)
    return nmf


def weights_of(shape_V, kind, seed=3):
    rng = np.random.default_rng(seed)
    if kind is None:
        return None
    if kind == 'mask':   # 0 / 1, shared by the channels
        return np.broadcast_to((rng.random((shape_V[0], 1) + shape_V[2:]) > 0.3).astype(float), shape_V).copy()
    return rng.random(shape_V) + 0.1


def literal(nmf, G):
    """gain[n, m] = 1/2 ||V - R + R_m||^2 - 1/2 ||V - R||^2 from R and R_partial(m), and the sum of the absolute terms."""
    V, R = nmf.V, nmf.R
    g = np.ones(V.shape) if G is None else G
    axes = tuple(range(1, V.ndim))
    gain, scale = [], []
    for m in range(nmf.n_atoms):
        Rm = nmf.R_partial(m)
        gain.append(0.5 * np.sum(g * (V - R + Rm) ** 2, axis=axes) - 0.5 * np.sum(g * (V - R) ** 2, axis=axes))
        scale.append(np.sum(np.abs(Rm) * np.abs(g * (V - R)), axis=axes) + 0.5 * np.sum(g * Rm ** 2, axis=axes))
    return np.stack(gain, axis=1), np.stack(scale, axis=1)


CASES = {   # shape of V, atoms, atom shape, transforms
    '1d-c1': ((3, 1, 25), 3, (5,), None),
    '1d-c3': ((2, 3, 19), 2, (4,), None),
    '2d-c1': ((2, 1, 9, 10), 3, (3, 4), None),
    '2d-c3': ((2, 3, 8, 9), 2, (3, 3), None),
    'rot90': ((2, 1, 8, 8), 2, (3, 3), 'rot90'),
    'rot90-c3': ((2, 3, 7, 8), 2, (3, 3), 'rot90'),
    'operators': ((2, 1, 9, 8), 2, (3, 3), 'operators'),
}


def transforms_of(name, atom_shape):
    return tr.rotations(atom_shape, 3) if name == 'operators' else name


# -- 1. the definition ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [None, 'mask', 'real'], ids=str)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', list(CASES))
def test_the_gain_is_the_objective_without_the_atom_minus_the_objective(case, mode, kind):
    shape_V, M, A, t = CASES[case]
    G = weights_of(shape_V, kind)
    nmf = model(shape_V, M, A, mode, G, transforms_of(t, A))
    want, scale = literal(nmf, G)
    got = nmf.atom_gains(per_sample=True)
    assert got.shape == (shape_V[0], M) and got.dtype == np.float64
    assert np.all(np.abs(got - want) <= RTOL * scale), float(np.max(np.abs(got - want) / scale))
    np.testing.assert_array_equal(nmf.atom_gains(), got.sum(axis=0))
    a, b = nmf.atom_terms()
    np.testing.assert_array_equal(a + 0.5 * b, got)
    assert np.all(b >= 0)


@pytest.mark.parametrize('kind', [None, 'real'], ids=str)
@pytest.mark.parametrize('group', [1, 2])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', ['1d-c1', '2d-c3'])
def test_the_fallback_equals_the_pixel_by_pixel_reference(case, mode, group, kind):
    shape_V, _, A, _ = CASES[case]
    rng = np.random.default_rng(7)
    D = shape_V[2:]
    W = rng.random((4, shape_V[1]) + A)
    H = rng.random((shape_V[0], 4) + eref.shift_shape(D, A, mode)) * (rng.random((shape_V[0], 4) + (1,) * len(A)) > 0.2)
    V, G = rng.random(shape_V), weights_of(shape_V, kind)
    a, b = atom_terms_numpy(W, H, mode, V, G, group)
    ra, rb, scale = aref.terms(aref.parts_loop(W, H, D, mode, group), V, G)
    assert a.shape == (shape_V[0], 4 // group)
    assert np.all(np.abs(a - ra) <= RTOL * scale) and np.all(np.abs(b - rb) <= RTOL * rb)
    # the two forms of the reference agree as well: the padded correlation is the sum of the images
    pa, pb, _ = aref.terms(aref.parts_valid(W, pad_activations_numpy(H, A, mode), group), V, G)
    assert np.all(np.abs(pa - ra) <= RTOL * scale) and np.all(np.abs(pb - rb) <= RTOL * rb)


# -- 2. sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [None, 'real'], ids=str)
@pytest.mark.parametrize('mode', MODES)
def test_the_a_terms_of_all_atoms_add_up_to_the_reconstruction_against_the_residual(mode, kind):
    shape_V = (2, 3, 8, 9)
    G = weights_of(shape_V, kind)
    nmf = model(shape_V, 3, (3, 3), mode, G)
    g = np.ones(shape_V) if G is None else G
    gd = g * (nmf.V - nmf.R)
    a, _ = nmf.atom_terms()
    want, scale = np.sum(nmf.R * gd, axis=(1, 2, 3)), np.sum(np.abs(nmf.R) * np.abs(gd), axis=(1, 2, 3))
    assert np.all(np.abs(a.sum(axis=1) - want) <= RTOL * scale)


@pytest.mark.parametrize('kind', [None, 'mask', 'real'], ids=str)
@pytest.mark.parametrize('mode', MODES)
def test_the_gain_of_a_single_atom_is_the_energy_of_the_data_minus_the_objective(mode, kind):
    shape_V = (3, 2, 21)
    G = weights_of(shape_V, kind)
    nmf = model(shape_V, 1, (4,), mode, G)
    g = np.ones(shape_V) if G is None else G
    energy = 0.5 * np.sum(g * nmf.V ** 2)
    assert abs(nmf.atom_gains()[0] - (energy - nmf.objective())) <= RTOL * energy


@pytest.mark.parametrize('t', [None, 'rot90'], ids=str)
@pytest.mark.parametrize('mode', MODES)
def test_a_is_the_activations_against_the_gradient_of_H(mode, t):
    nmf = model((2, 1, 8, 8), 2, (3, 3), mode, None, t)
    neg, pos = nmf._backend.reconstruction_gradient_H(nmf._V, nmf._W_dict, nmf._H)
    T = nmf.n_transforms
    each = np.sum(nmf._H * (neg - pos), axis=(2, 3)).reshape(2, 2, T).sum(axis=2)
    scale = np.sum(nmf._H * (neg + pos), axis=(2, 3)).reshape(2, 2, T).sum(axis=2)
    a, _ = nmf.atom_terms()
    assert np.all(np.abs(a - each) <= RTOL * scale)


# -- 3. edge cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', [None, 'rot90'], ids=str)
def test_an_atom_without_activations_gets_exact_zeros(t):
    nmf = model((2, 1, 8, 8), 3, (3, 3), 'reflect', None, t)
    T = nmf.n_transforms
    nmf._H[:, T:2 * T] = 0.
    a, b = nmf.atom_terms()
    assert np.all(a[:, 1] == 0.) and np.all(b[:, 1] == 0.) and np.all(b[:, [0, 2]] > 0)
    assert nmf.atom_gains()[1] == 0.


def test_a_mask_that_hides_a_sample_gives_it_exact_zeros_whatever_it_holds():
    shape_V = (3, 2, 8, 9)
    G = weights_of(shape_V, 'mask')
    G[1] = 0.
    V = np.random.default_rng(0).random(shape_V) + 0.05
    V[1] = np.nan
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=_AtomStub('valid'))
    nmf.fit(V, n_iterations=0, weights=G)
    a, b = nmf.atom_terms()
    assert np.all(a[1] == 0.) and np.all(b[1] == 0.)
    assert np.all(np.isfinite(a)) and np.all(b[[0, 2]] > 0)


# -- 4. the order of the samples, refusals ------------------------------------------------------------------------------------
def test_samples_come_in_the_order_of_H_under_a_shuffle():
    nmf = model((5, 1, 9, 8), 2, (3, 3))
    plain = nmf.atom_gains(per_sample=True)
    H = nmf.H
    nmf._shuffle_idx = np.array([3, 0, 4, 1, 2])
    try:
        order = np.argsort(nmf._shuffle_idx)
        np.testing.assert_array_equal(nmf.H, H[order])
        np.testing.assert_array_equal(nmf.atom_gains(per_sample=True), plain[order])
        a, b = nmf.atom_terms()
        np.testing.assert_array_equal(a + 0.5 * b, plain[order])
        np.testing.assert_array_equal(nmf.atom_gains(), plain.sum(axis=0))
    finally:
        nmf._shuffle_idx = None


def snapshot(nmf):
    return [np.array(x) for x in (nmf.W, nmf.H, nmf.V, nmf.R)]


def test_refusals_leave_the_model_as_it_was():
    with pytest.raises(RuntimeError):
        TransformInvariantNMF(n_atoms=2, atom_shape=(3, 4), backend=_AtomStub()).atom_gains()
    with pytest.raises(RuntimeError):
        TransformInvariantNMF(n_atoms=2, atom_shape=(3, 4), backend=_AtomStub()).atom_terms()
    nmf = model((2, 1, 9, 10), 2, (3, 4), 'reflect')
    before = snapshot(nmf)
    nmf._beta = 1.
    try:
        with pytest.raises(NotImplementedError, match=r'atom_gains covers the Frobenius objective \(beta_loss 2\), with or '
                                                      r'without weights'):
            nmf.atom_gains()
        with pytest.raises(NotImplementedError):
            nmf.atom_terms()
    finally:
        nmf._beta = 2.
    for bad in ('yes', 1, 0, None, 1.0):
        with pytest.raises(ValueError):
            nmf.atom_gains(per_sample=bad)
    assert nmf.atom_gains(per_sample=np.bool_(True)).shape == (2, 2)
    assert nmf.atom_gains().shape == (2,)
    for was, now in zip(before, snapshot(nmf)):
        np.testing.assert_array_equal(was, now)


def test_volumes_are_refused():
    nmf = fitted((1, 1, 5, 5, 5), 1, (2, 2, 2))
    with pytest.raises(NotImplementedError):
        nmf.atom_gains()
    with pytest.raises(NotImplementedError):
        nmf.atom_terms()


# -- 5. the ABI ---------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_built():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tnmf_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint tnmf_hip_atom_terms\s*\(', header) and 'tnmf_hip_atom_terms' in _lib.EXPORTS
    makefile = open(os.path.join(ROOT, 'tnmf_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\batoms\.hip\b', makefile, flags=re.M) and re.search(r'^HDRS\s*:=.*\batoms\.h\b', makefile,
                                                                                       flags=re.M)
    assert _lib.ABI_VERSION == 8
    import ctypes
    lib = _lib.load()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert list(lib.tnmf_hip_atom_terms.argtypes) == [vp, ctypes.POINTER(_lib.Geom), ci, vp, vp, vp, vp, vp, vp, vp]
    g = _lib.make_geom(1, 1, 1, (4,), (2,), 0)   # an argument error is answered without a device: no context
    assert lib.tnmf_hip_atom_terms(None, ctypes.byref(g), 1, None, None, None, None, None, None, None) == -1
