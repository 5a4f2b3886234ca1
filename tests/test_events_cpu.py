"""
Events on CPU: the host fallback ``events_numpy`` and the front end's ``reconstruct_detections`` / ``refit_detections`` over
an oracle-backed backend without the events hooks, against the float64 oracle on the scattered dense H and against the
naive reference tests/events_reference.py.
"""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

import events_reference as eref
from conftest import ROOT
from oracle import tnmf_oracle as orc
from oracle_backend import OracleBackend
from tnmf_amd import _lib, sharding, transforms as tr
from tnmf_amd.backends._Backend import sliceNone
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF, event_images, events_numpy

MODES = ['valid', 'full', 'circular', 'reflect']
SHAPES = {'1d': ((11,), (4,)), '2d': ((8, 9), (3, 4))}
EPS = 1e-9


def hand_made(D, A, mode, seed=0, n_random=12):
    """Distinct events of 2 samples and 3 planes: the corners of the shift range, one in the wrap / mirror zone of EVERY axis
    (4 images on two axes), its neighbours, and random ones.  Strengths 1..4."""
    S = eref.shift_shape(D, A, mode)
    k = len(D)
    rng = np.random.default_rng(seed)
    rows = {(0, 0) + (0,) * k, (1, 2) + tuple(s - 1 for s in S), (0, 1) + tuple(s // 2 for s in S)}
    if mode == 'circular':
        rows |= {(1, 1) + tuple(s - 1 for s in S), (0, 2) + tuple(s - (a - 1) for s, a in zip(S, A))}
    if mode == 'reflect':
        rows |= {(1, 1) + (1,) * k, (0, 2) + tuple(a - 1 for a in A)}
    if k == 2:
        rows |= {(1, 0, 0, S[1] - 1), (1, 0, S[0] - 1, 0)}
    while len(rows) < 8 + n_random:
        rows.add((int(rng.integers(2)), int(rng.integers(3))) + tuple(int(rng.integers(s)) for s in S))
    rows = np.array(sorted(rows))
    return rows[:, 0], rows[:, 1], rows[:, 2:], rng.integers(1, 5, len(rows)).astype(np.float64)


# -- 1. the image table, pinned by the oracle's padded reconstruction ------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', ['1d', '2d'])
def test_render_equals_the_oracle_on_the_scattered_H(case, mode):
    D, A = SHAPES[case]
    S = eref.shift_shape(D, A, mode)
    W = np.random.default_rng(1).integers(0, 4, (3, 2) + A).astype(np.float64)
    sample, plane, shift, h = hand_made(D, A, mode)
    want = orc.reconstruct(W, eref.scatter(2, 3, S, sample, plane, shift, h), 'contract', mode)
    assert want.any()
    assert np.array_equal(events_numpy(W, D, 2, mode, sample, plane, shift, h), want)
    assert np.array_equal(eref.render(W, D, 2, mode, sample, plane, shift, h), want)
    if mode in ('circular', 'reflect'):   # an event in the zone of every axis stands for 2^k images
        zone = (1, 1) + (tuple(s - 1 for s in S) if mode == 'circular' else (1,) * len(D))
        row = np.flatnonzero(np.all(np.column_stack([sample, plane, shift]) == zone, axis=1))
        assert len(row) == 1
        event, _ = event_images(shift, A, S, mode)
        assert np.sum(event == row[0]) == 2 ** len(D) == len(eref.images(shift[row[0]], A, S, mode))


def test_duplicates_add_up_in_a_render():
    D, A = SHAPES['2d']
    W = np.random.default_rng(2).integers(0, 4, (3, 1) + A).astype(np.float64)
    sample, plane, shift, h = hand_made(D, A, 'circular', seed=3)
    twice = [np.concatenate([x, x[:5]]) for x in (sample, plane, shift, h)]
    once = (sample, plane, shift, np.concatenate([2 * h[:5], h[5:]]))
    assert np.array_equal(events_numpy(W, D, 2, 'circular', *twice), events_numpy(W, D, 2, 'circular', *once))
    assert np.array_equal(eref.render(W, D, 2, 'circular', *twice), eref.render(W, D, 2, 'circular', *once))


# -- 2. the refit step is the dense H half step on the support ---------------------------------------------------------------
@pytest.mark.parametrize('sparsity', [0., 0.3])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', ['1d', '2d'])
def test_five_refit_steps_equal_five_dense_half_steps(case, mode, sparsity):
    """Relative 1e-12: every sum has at most a few hundred positive float64 terms, ~1e-14 per step."""
    D, A = SHAPES[case]
    S = eref.shift_shape(D, A, mode)
    rng = np.random.default_rng(4)
    W, V = rng.random((3, 2) + A), rng.random((2, 2) + D) + 0.1
    sample, plane, shift, h = hand_made(D, A, mode, seed=5)
    h = h * rng.random(len(h))
    h[3] = 0.   # stays 0
    H = eref.scatter(2, 3, S, sample, plane, shift, h)
    for _ in range(5):
        neg, pos = orc.gradient_H(V, W, H, slice(None), 'contract', mode)
        orc.multiplicative_update(H, neg, pos, EPS, sparsity)
    want = H[(sample, plane) + tuple(shift.T)]
    assert want[3] == 0. and np.count_nonzero(H) == len(h) - 1
    got = events_numpy(W, D, 2, mode, sample, plane, shift, h, V=V, n_iterations=5, sparsity=sparsity, eps=EPS)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    ref = eref.refit(V, W, mode, sample, plane, shift, h, 5, sparsity, EPS)
    np.testing.assert_allclose(ref, want, rtol=1e-12, atol=0)


# -- 3. the front end ---------------------------------------------------------------------------------------------------------
class _Stub(OracleBackend):
    """The oracle's primitives in any reconstruction mode, with the hooks a transformed model needs for an H half step.
    No ``find_peaks``, no events hooks: the front end works on the host."""

    supports_transforms = True

    def __init__(self, mode='valid', shard=None):
        super().__init__(impl='contract')
        self._reconstruction_mode = mode
        self._fixed_shard = shard

    def _initialize_matrices(self, V, atom_shape, n_atoms, W=None, axes_W_normalization=None, transforms=None):
        T = 1 if transforms is None else tr.size(transforms)
        n0, n1 = self._shard = self._fixed_shard or (0, V.shape[0])
        self._V_local = V[n0:n1]
        H = np.empty((n1 - n0, n_atoms * T) + self._transform_shape, dtype=V.dtype)
        for i, h in sharding.reference_init_stream(V.shape[0], H.shape[1:], self._shard, V.dtype):
            H[i] = h
        if W is None:
            W = sharding.reference_init_W(n_atoms, self.n_channels, self.atom_shape, V.dtype)
        return W, H

    @property
    def shard(self):
        return self._shard

    def reconstruct(self, W, H):
        return orc.reconstruct(W, H, self.impl, self._reconstruction_mode)

    def reconstruction_gradient_H(self, V, W, H, s=sliceNone):
        return orc.gradient_H(self._V_local, W, H, s, self.impl, self._reconstruction_mode)

    def reconstruction_gradient_W(self, V, W, H, s=sliceNone):
        return orc.gradient_W(self._V_local, W, H, s, self.impl, self._reconstruction_mode)

    def reconstruction_energy(self, V, W, H, beta=2., eps=1e-9):
        return orc.energy(self._V_local, W, H, self.impl, self._reconstruction_mode)

    def expand_W(self, W, transforms, W_eff=None):
        e = tr.expand(W, transforms)
        if W_eff is None:
            return e
        W_eff[...] = e
        return W_eff

    def fused_update_H(self, V, W, H, s=sliceNone, sparsity=0., eps=1e-9, beta=2., **_):
        neg, pos = self.reconstruction_gradient_H(V, W, H, s)
        orc.multiplicative_update(H[s], neg, pos, eps, sparsity)


def fitted(shape_V, n_atoms, atom_shape, mode='valid', seed=0, shard=None, minibatches=False, **kw):
    V = np.random.default_rng(seed).random(shape_V) + 0.05
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=n_atoms, atom_shape=atom_shape, backend=_Stub(mode, shard), **kw)
    if minibatches:
        nmf.fit_minibatches(V, batch_size=2, n_epochs=2, sparsity_H=0.1)
    else:
        nmf.fit(V, n_iterations=2, sparsity_H=0.1, update_W='transforms' not in kw)
    return nmf


def check_model(nmf, sparsity):
    be = nmf._backend
    mode = be._reconstruction_mode
    det = nmf.detections(threshold=0., min_distance=0)          # every positive entry of H
    assert len(det) == int(np.count_nonzero(nmf.H > 0)) > 0
    R = nmf.reconstruct_detections(det)
    assert R.shape == nmf.R.shape and R.dtype == nmf.R.dtype
    np.testing.assert_allclose(R, nmf.R, rtol=1e-12, atol=0)
    refit = nmf.refit_detections(det, 3, sparsity_H=sparsity)
    assert isinstance(refit, Detections) and refit is not det
    for name in ('sample', 'atom', 'transform', 'shift', 'origin'):
        np.testing.assert_array_equal(getattr(refit, name), getattr(det, name))
    H = np.array(nmf._H)                                        # three dense steps, the backend's order
    for _ in range(3):
        neg, pos = orc.gradient_H(be._V_local, nmf._W_dict, H, slice(None), 'contract', mode)
        orc.multiplicative_update(H, neg, pos, nmf.eps, sparsity)
    stepped = H
    if nmf._shuffle_idx is not None:
        H = H[np.argsort(nmf._shuffle_idx)]
    H = H.reshape(nmf.H.shape)
    at = (det.sample - be.shard[0], det.atom) + ((det.transform,) if nmf.transforms is not None else ())
    np.testing.assert_allclose(refit.strength, H[at + tuple(det.shift.T)], rtol=1e-12, atol=0)
    # the refitted strengths render to the reconstruction of the stepped activations
    np.testing.assert_allclose(nmf.reconstruct_detections(refit), orc.reconstruct(nmf._W_dict, stepped, 'contract', mode),
                               rtol=1e-11, atol=0)
    return det, refit


@pytest.mark.parametrize('mode', ['valid', 'circular'])
@pytest.mark.parametrize('sparsity', [0., 0.2])
def test_fit_detect_reconstruct_refit(mode, sparsity):
    check_model(fitted((3, 2, 9, 10), 2, (3, 4), mode), sparsity)
    check_model(fitted((3, 1, 25), 2, (5,), mode), sparsity)


def test_with_rot90_the_plane_is_atom_and_transform():
    nmf = fitted((2, 1, 8, 8), 2, (3, 3), 'circular', transforms='rot90')
    assert nmf.H.shape == (2, 2, 4, 8, 8)
    det, _ = check_model(nmf, 0.1)
    assert set(det.transform.tolist()) == {0, 1, 2, 3}
    # one detection alone renders its own orientation of its atom
    one = Detections(*[getattr(det, f.name)[7:8] for f in dataclasses.fields(Detections)])
    H = np.zeros_like(nmf._H)
    H[(one.sample[0], one.atom[0] * 4 + one.transform[0]) + tuple(one.shift[0])] = one.strength[0]
    np.testing.assert_allclose(nmf.reconstruct_detections(one), nmf._backend.reconstruct(nmf._W_eff, H), rtol=1e-12)


def test_samples_map_back_through_a_shuffle_after_fit_minibatches():
    nmf = fitted((5, 1, 9, 8), 2, (3, 3), minibatches=True)
    nmf._shuffle_idx = np.array([3, 0, 4, 1, 2])
    assert np.array_equal(nmf.H[3], nmf._H[0])                  # internal sample 0 is sample 3 of V
    det, _ = check_model(nmf, 0.)
    only = dataclasses.replace(det, **{f.name: getattr(det, f.name)[det.sample == 3]
                                       for f in dataclasses.fields(Detections)})
    R = nmf.reconstruct_detections(only)                        # in the order of R: the backend's
    np.testing.assert_allclose(R[0], nmf.R[0], rtol=1e-12)
    assert not R[1:].any()


def test_a_rank_takes_the_samples_of_its_block_only():
    nmf = fitted((6, 1, 20), 2, (4,), shard=(2, 5))
    assert nmf._H.shape[0] == 3
    det, _ = check_model(nmf, 0.1)
    assert set(det.sample.tolist()) == {2, 3, 4}
    for bad in (1, 5):
        with pytest.raises(ValueError):
            nmf.reconstruct_detections(dataclasses.replace(det, sample=np.full_like(det.sample, bad)))


# -- 4. refusals ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model():
    nmf = fitted((2, 1, 9, 10), 2, (3, 4), 'reflect')
    return nmf, nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)), min_distance=0)


def _with(det, name, row, value):
    col = np.array(getattr(det, name))
    col[row] = value
    return dataclasses.replace(det, **{name: col})


@pytest.mark.parametrize('name, value', [('sample', -1), ('sample', 2), ('atom', -1), ('atom', 2), ('transform', 1),
                                         ('transform', -1), ('shift', (9, 0)), ('shift', (0, 10)), ('shift', (-1, 3)),
                                         ('strength', -1.), ('strength', np.nan), ('strength', np.inf)], ids=str)
def test_bad_rows_raise_value_error(model, name, value):
    nmf, det = model
    assert len(det) > 3
    bad = _with(det, name, 2, value)
    with pytest.raises(ValueError):
        nmf.reconstruct_detections(bad)
    with pytest.raises(ValueError):
        nmf.refit_detections(bad, 1)


def test_a_refit_refuses_duplicates_a_render_takes_them(model):
    nmf, det = model
    twice = dataclasses.replace(det, **{f.name: np.concatenate([getattr(det, f.name), getattr(det, f.name)[:1]])
                                        for f in dataclasses.fields(Detections)})
    with pytest.raises(ValueError):
        nmf.refit_detections(twice, 1)
    first = dataclasses.replace(det, **{f.name: getattr(det, f.name)[:1] for f in dataclasses.fields(Detections)})
    np.testing.assert_allclose(nmf.reconstruct_detections(twice),
                               nmf.reconstruct_detections(det) + nmf.reconstruct_detections(first), rtol=1e-12)


@pytest.mark.parametrize('kw', [dict(n_iterations=-1), dict(n_iterations=1.5), dict(n_iterations=True),
                                dict(sparsity_H=-0.1), dict(sparsity_H=float('nan')), dict(sparsity_H='0')], ids=str)
def test_bad_refit_arguments_raise_value_error(model, kw):
    nmf, det = model
    with pytest.raises(ValueError):
        nmf.refit_detections(det, **kw)


def test_zero_iterations_and_no_rows(model):
    nmf, det = model
    assert nmf.refit_detections(det, 0).strength.tobytes() == det.strength.tobytes()
    none = dataclasses.replace(det, **{f.name: getattr(det, f.name)[:0] for f in dataclasses.fields(Detections)})
    assert not nmf.reconstruct_detections(none).any() and nmf.reconstruct_detections(none).shape == nmf.R.shape
    assert len(nmf.refit_detections(none, 2)) == 0


def test_before_a_fit_both_raise_runtime_error(model):
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 4), backend=_Stub())
    with pytest.raises(RuntimeError):
        nmf.reconstruct_detections(model[1])
    with pytest.raises(RuntimeError):
        nmf.refit_detections(model[1])


def test_volumes_are_refused():
    nmf = fitted((1, 1, 5, 5, 5), 1, (2, 2, 2))
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)), min_distance=0)
    with pytest.raises(NotImplementedError):
        nmf.reconstruct_detections(det)
    with pytest.raises(NotImplementedError):
        nmf.refit_detections(det, 1)


def test_a_refit_is_frobenius_and_unweighted_a_render_is_not(model):
    nmf, det = model
    want = nmf.reconstruct_detections(det)
    nmf._beta = 1.
    try:
        with pytest.raises(NotImplementedError):
            nmf.refit_detections(det, 1)
        assert np.array_equal(nmf.reconstruct_detections(det), want)
    finally:
        nmf._beta = 2.
    nmf._weighted = True
    try:
        with pytest.raises(NotImplementedError):
            nmf.refit_detections(det, 1)
        assert np.array_equal(nmf.reconstruct_detections(det), want)
    finally:
        nmf._weighted = False


# -- 5. the ABI -------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_typed():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tnmf_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    vp, ll, cd, ci = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_double, ctypes.c_int
    gp = ctypes.POINTER(_lib.Geom)
    for name, argtypes in (('tnmf_hip_events_render', [vp, gp, vp, vp, ll, vp, vp, ll, vp, vp]),
                           ('tnmf_hip_events_update', [vp, gp, ci, vp, vp, vp, ll, vp, vp, cd, cd, vp])):
        assert re.search(r'\bint %s\s*\(' % name, header)
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is ci and list(fn.argtypes) == argtypes
    assert _lib.ABI_VERSION == 8
    cells = {1: int(re.search(r'#define TNMF_EVENTS_CELL_1D (\d+)', header).group(1)),
             2: int(re.search(r'#define TNMF_EVENTS_CELL_2D (\d+)', header).group(1))}
    assert _lib.EVENT_CELLS == {1: (cells[1],), 2: (cells[2], cells[2])}
    # argument errors are answered without a device: no context
    g = _lib.make_geom(1, 1, 1, (4,), (2,), 0)
    assert lib.tnmf_hip_events_render(None, ctypes.byref(g), None, None, 0, None, None, 0, None, None) == -1
    assert lib.tnmf_hip_events_update(None, ctypes.byref(g), 0, None, None, None, 0, None, None, 1e-9, 0., None) == -1
