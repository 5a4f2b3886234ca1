"""
The W side of the events on CPU: the naive reference tests/events_w_reference.py and the host fallback ``events_fit_numpy``
against the float64 oracle on the scattered dense H, and the front end's ``fit_detections`` over an oracle-backed backend
without the events hooks.
"""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

import events_reference as eref
import events_w_reference as wref
from conftest import ROOT
from oracle import tnmf_oracle as orc
from oracle_backend import OracleBackend
from tnmf_amd import _lib, sharding, transforms as tr
from tnmf_amd.backends._Backend import sliceNone
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF, events_fit_numpy

MODES = ['valid', 'full', 'circular', 'reflect']
SHAPES = {'1d': ((25,), (5,)), '2d': ((9, 10), (3, 4))}
EPS = 1e-9
N, P, C = 2, 3, 2


def hand_made(D, A, mode, seed=0):
    """16 distinct events of 2 samples and 3 planes: corners of the shift range, one in the wrap / mirror zone of EVERY axis
    (2^k images), one in the zone of the last axis alone, and random ones.  Strengths 1..4."""
    S = eref.shift_shape(D, A, mode)
    k = len(D)
    rng = np.random.default_rng(seed)
    rows = {(0, 0) + (0,) * k, (1, 2) + tuple(s - 1 for s in S), (0, 1) + tuple(s // 2 for s in S)}
    if mode == 'circular':
        rows |= {(1, 1) + tuple(s - 1 for s in S), (0, 2) + (S[0] // 2,) * (k - 1) + (S[-1] - (A[-1] - 1),)}
    if mode == 'reflect':
        rows |= {(1, 1) + (1,) * k, (0, 2) + (S[0] // 2,) * (k - 1) + (A[-1] - 1,)}
    while len(rows) < 16:
        rows.add((int(rng.integers(N)), int(rng.integers(P))) + tuple(int(rng.integers(s)) for s in S))
    rows = np.array(sorted(rows))
    return rows[:, 0], rows[:, 1], rows[:, 2:], rng.integers(1, 5, len(rows)).astype(np.float64)


# -- 1. the gradient of the list is the dense W gradient of the scattered H -------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', ['1d', '2d'])
def test_reference_gradient_equals_the_oracle_on_the_scattered_H(case, mode):
    D, A = SHAPES[case]
    S = eref.shift_shape(D, A, mode)
    rng = np.random.default_rng(1)
    W, V = rng.random((P, C) + A), rng.random((N, C) + D) + 0.1
    sample, plane, shift, h = hand_made(D, A, mode)
    if mode in ('circular', 'reflect'):
        assert max(len(eref.images(u, A, S, mode)) for u in shift) == 2 ** len(D)
    H = eref.scatter(N, P, S, sample, plane, shift, h)
    want = orc.gradient_W(V, W, H, slice(None), 'contract', mode)
    R = eref.render(W, D, N, mode, sample, plane, shift, h)
    got = wref.grad_W(V, R, W, D, mode, sample, plane, shift, h)
    np.testing.assert_allclose(got[0], want[0], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-12, atol=0)
    # duplicate rows add up: the gradient is linear in the strengths for a fixed R
    twice = [np.concatenate([x, x[:4]]) for x in (sample, plane, shift, h)]
    once = (sample, plane, shift, np.concatenate([2 * h[:4], h[4:]]))
    np.testing.assert_allclose(wref.grad_W(V, R, W, D, mode, *twice), wref.grad_W(V, R, W, D, mode, *once), rtol=1e-13)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', ['1d', '2d'])
def test_five_alternating_iterations_equal_five_dense_iterations(case, mode):
    """Relative 1e-12: every sum has a few hundred positive float64 terms, ~1e-14 per step (measured: 8e-16)."""
    D, A = SHAPES[case]
    S = eref.shift_shape(D, A, mode)
    axes = tuple(range(-len(A), 0))
    rng = np.random.default_rng(4)
    W, V = rng.random((P, C) + A), rng.random((N, C) + D) + 0.1
    orc.normalize(W, axes)
    sample, plane, shift, h = hand_made(D, A, mode, seed=5)
    h = h * rng.random(len(h))
    h[3] = 0.   # stays 0
    H, Wd = eref.scatter(N, P, S, sample, plane, shift, h), W.copy()
    for _ in range(5):
        neg, pos = orc.gradient_H(V, Wd, H, slice(None), 'contract', mode)
        orc.multiplicative_update(H, neg, pos, EPS, 0.1)
        neg, pos = orc.gradient_W(V, Wd, H, slice(None), 'contract', mode)
        orc.multiplicative_update(Wd, neg, pos, EPS, 0.)
        orc.normalize(Wd, axes)
    want = H[(sample, plane) + tuple(shift.T)]
    assert want[3] == 0. and np.count_nonzero(H) == len(h) - 1 and np.all(np.isfinite(Wd))
    W_in, h_in = W.copy(), h.copy()
    got_W, got = events_fit_numpy(W, None, D, N, mode, sample, plane, shift, h, V, 5, sparsity=0.1, eps=EPS)
    assert np.array_equal(W, W_in) and np.array_equal(h, h_in)      # the arguments are left as they are
    worst = max(np.abs(got_W / Wd - 1).max(), np.abs(got[want > 0] / want[want > 0] - 1).max())
    print(f'{case} {mode}: host fallback vs 5 dense iterations {worst:.3g}')
    np.testing.assert_allclose(got_W, Wd, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    ref_W, ref = wref.fit(V, W, mode, sample, plane, shift, h, 5, 0.1, EPS)
    np.testing.assert_allclose(ref_W, Wd, rtol=1e-12, atol=0)
    np.testing.assert_allclose(ref, want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got_W.sum(axis=axes), 1., rtol=1e-14)


def test_an_atom_without_evidence_keeps_its_entries():
    D, A = SHAPES['2d']
    axes = (-2, -1)
    rng = np.random.default_rng(6)
    W, V = rng.random((P, C) + A), rng.random((N, C) + D) + 0.1
    orc.normalize(W, axes)
    sample, plane, shift, h = hand_made(D, A, 'reflect', seed=7)
    h = np.where(plane == 1, 0., h)                                  # plane 1: zero strengths only
    live = plane != 2                                                # plane 2: no events at all
    args = [x[live] for x in (sample, plane, shift, h)]
    got_W, got = events_fit_numpy(W, None, D, N, 'reflect', *args, V, 3, eps=EPS)
    ref_W, ref = wref.fit(V, W, 'reflect', *args, 3, 0., EPS)
    assert np.all(np.isfinite(got_W)) and np.all(np.isfinite(got))
    assert got_W[1].tobytes() == W[1].tobytes() and got_W[2].tobytes() == W[2].tobytes()
    assert ref_W[1].tobytes() == W[1].tobytes() and ref_W[2].tobytes() == W[2].tobytes()
    assert not np.array_equal(got_W[0], W[0])
    np.testing.assert_allclose(got_W, ref_W, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
    # the dense step, for the record: 0 * neg / (pos + eps) = 0, then 0 / 0 in the normalisation
    H, Wd = eref.scatter(N, P, eref.shift_shape(D, A, 'reflect'), *args), W.copy()
    neg, pos = orc.gradient_W(V, Wd, H, slice(None), 'contract', 'reflect')
    orc.multiplicative_update(Wd, neg, pos, EPS, 0.)
    with np.errstate(invalid='ignore'):
        orc.normalize(Wd, axes)
    assert np.all(np.isnan(Wd[1:])) and np.all(np.isfinite(Wd[0]))
    # zero data under the events of a plane: the same rule
    V0 = np.zeros_like(V)
    kept, _ = events_fit_numpy(W, None, D, N, 'reflect', *args, V0, 1, update_H=False, eps=EPS)
    assert kept.tobytes() == W.tobytes()


# -- 2. the front end -----------------------------------------------------------------------------------------------------------
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


def dense_iterations(nmf, n, sparsity, update_H=True):
    """(W, H in the layout of the H property) after n dense oracle iterations from the model's state, the backend's order."""
    be = nmf._backend
    mode, axes = be._reconstruction_mode, nmf._axes_W_normalization
    W, H = np.array(nmf._W), np.array(nmf._H)
    for _ in range(n):
        W_eff = W if nmf.transforms is None else tr.expand(W, nmf.transforms)
        if update_H:
            neg, pos = orc.gradient_H(be._V_local, W_eff, H, slice(None), 'contract', mode)
            orc.multiplicative_update(H, neg, pos, nmf.eps, sparsity)
        neg, pos = orc.gradient_W(be._V_local, W_eff, H, slice(None), 'contract', mode)
        if nmf.transforms is not None:
            neg, pos = tr.fold(neg, nmf.transforms), tr.fold(pos, nmf.transforms)
        orc.multiplicative_update(W, neg, pos, nmf.eps, 0.)
        orc.normalize(W, axes)
    if nmf._shuffle_idx is not None:
        H = H[np.argsort(nmf._shuffle_idx)]
    return W, H.reshape(nmf.H.shape)


def check_model(nmf, sparsity):
    be = nmf._backend
    det = nmf.detections(threshold=0., min_distance=0)          # every positive entry of H
    assert len(det) == int(np.count_nonzero(nmf.H > 0)) > 0
    want_W, want_H = dense_iterations(nmf, 3, sparsity)
    H_before, W_before = nmf.H.copy(), nmf.W.copy()
    fit = nmf.fit_detections(det, 3, sparsity_H=sparsity)
    assert isinstance(fit, Detections) and fit is not det
    for name in ('sample', 'atom', 'transform', 'shift', 'origin'):
        np.testing.assert_array_equal(getattr(fit, name), getattr(det, name))
    at = (det.sample - be.shard[0], det.atom) + ((det.transform,) if nmf.transforms is not None else ())
    np.testing.assert_allclose(fit.strength, want_H[at + tuple(det.shift.T)], rtol=1e-12, atol=0)
    np.testing.assert_allclose(nmf.W, want_W, rtol=1e-12, atol=0)
    assert not np.array_equal(nmf.W, W_before) and np.all(np.isfinite(nmf.W))
    np.testing.assert_allclose(nmf.W.sum(axis=nmf._axes_W_normalization), 1., rtol=1e-14)
    assert nmf.H.tobytes() == H_before.tobytes()                # the dense H is left as it is
    if nmf.transforms is not None:                              # transformed_atoms follow the new W
        assert np.array_equal(nmf.transformed_atoms.reshape(nmf._W_eff.shape), tr.expand(nmf.W, nmf.transforms))
    return det, fit


@pytest.mark.parametrize('mode', ['valid', 'circular'])
def test_fit_detect_fit_detections(mode):
    check_model(fitted((3, 2, 9, 10), 2, (3, 4), mode), 0.1)
    check_model(fitted((3, 1, 25), 2, (5,), mode), 0.)


def test_with_rot90_the_gradient_is_folded_and_the_orientations_refreshed():
    nmf = fitted((2, 1, 8, 8), 2, (3, 3), 'circular', transforms='rot90')
    det, _ = check_model(nmf, 0.1)
    assert set(det.transform.tolist()) == {0, 1, 2, 3}


def test_under_a_shuffle_after_fit_minibatches():
    nmf = fitted((5, 1, 9, 8), 2, (3, 3), minibatches=True)
    nmf._shuffle_idx = np.array([3, 0, 4, 1, 2])
    check_model(nmf, 0.)


def test_on_the_block_of_a_rank():
    nmf = fitted((6, 1, 20), 2, (4,), shard=(2, 5))
    det, _ = check_model(nmf, 0.1)
    assert set(det.sample.tolist()) == {2, 3, 4}


@pytest.fixture()
def model():
    nmf = fitted((2, 1, 9, 10), 2, (3, 4), 'reflect')
    return nmf, nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)), min_distance=0)


def _rows(det, keep):
    return dataclasses.replace(det, **{f.name: getattr(det, f.name)[keep] for f in dataclasses.fields(Detections)})


def test_update_W_off_is_refit_detections(model):
    nmf, det = model
    W = nmf.W.copy()
    want = nmf.refit_detections(det, 3, sparsity_H=0.05)
    got = nmf.fit_detections(det, 3, sparsity_H=0.05, update_W=False)
    for f in dataclasses.fields(Detections):
        assert getattr(got, f.name).tobytes() == getattr(want, f.name).tobytes()
    assert nmf.W.tobytes() == W.tobytes()


def test_update_H_off_leaves_the_strengths_bit_equal(model):
    nmf, det = model
    W = nmf.W.copy()
    want_W, _ = dense_iterations_on(nmf, det, 2)
    got = nmf.fit_detections(det, 2, update_H=False)
    assert got.strength.tobytes() == det.strength.tobytes()
    assert not np.array_equal(nmf.W, W)
    np.testing.assert_allclose(nmf.W, want_W, rtol=1e-12, atol=0)


def dense_iterations_on(nmf, det, n):
    """n dense oracle W steps on the H that holds the detections alone."""
    be = nmf._backend
    mode, axes = be._reconstruction_mode, nmf._axes_W_normalization
    H = eref.scatter(nmf._H.shape[0], nmf.n_atoms, nmf._H.shape[2:], det.sample, det.atom, det.shift, det.strength)
    W = np.array(nmf._W)
    for _ in range(n):
        neg, pos = orc.gradient_W(be._V_local, W, H, slice(None), 'contract', mode)
        orc.multiplicative_update(W, neg, pos, nmf.eps, 0.)
        orc.normalize(W, axes)
    return W, H


def test_an_atom_without_detections_keeps_its_entries(model):
    nmf, det = model
    W = nmf.W.copy()
    only = _rows(det, det.atom == 0)
    assert 0 < len(only) < len(det)
    got = nmf.fit_detections(only, 3)
    assert nmf.W[1].tobytes() == W[1].tobytes() and not np.array_equal(nmf.W[0], W[0])
    assert np.all(np.isfinite(nmf.W)) and np.all(np.isfinite(got.strength))
    np.testing.assert_allclose(nmf.W.sum(axis=(-2, -1)), 1., rtol=1e-14)
    none = _rows(det, slice(0, 0))
    W = nmf.W.copy()
    assert len(nmf.fit_detections(none, 2)) == 0 and nmf.W.tobytes() == W.tobytes()
    assert nmf.fit_detections(det, 0).strength.tobytes() == det.strength.tobytes() and nmf.W.tobytes() == W.tobytes()


# -- 3. refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(update_H=False, update_W=False), dict(n_iterations=-1), dict(n_iterations=1.5),
                                dict(n_iterations=True), dict(sparsity_H=-0.1), dict(sparsity_H=float('nan')),
                                dict(sparsity_H='0'), dict(update_W=1), dict(update_H=None)], ids=str)
def test_bad_arguments_raise_value_error(model, kw):
    nmf, det = model
    W = nmf.W.copy()
    with pytest.raises(ValueError):
        nmf.fit_detections(det, **kw)
    assert nmf.W.tobytes() == W.tobytes()


def test_duplicate_and_bad_rows_are_refused(model):
    nmf, det = model
    W = nmf.W.copy()
    twice = dataclasses.replace(det, **{f.name: np.concatenate([getattr(det, f.name), getattr(det, f.name)[:1]])
                                        for f in dataclasses.fields(Detections)})
    with pytest.raises(ValueError):
        nmf.fit_detections(twice, 1)
    for name, value in (('sample', 2), ('atom', -1), ('transform', 1), ('shift', (9, 0)), ('strength', np.nan)):
        col = np.array(getattr(det, name))
        col[2] = value
        with pytest.raises(ValueError):
            nmf.fit_detections(dataclasses.replace(det, **{name: col}), 1)
    assert nmf.W.tobytes() == W.tobytes()


def test_before_a_fit_it_raises_runtime_error(model):
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 4), backend=_Stub())
    with pytest.raises(RuntimeError):
        nmf.fit_detections(model[1])


def test_volumes_are_refused():
    nmf = fitted((1, 1, 5, 5, 5), 1, (2, 2, 2))
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)), min_distance=0)
    with pytest.raises(NotImplementedError):
        nmf.fit_detections(det, 1)


def test_it_is_frobenius_and_unweighted(model):
    nmf, det = model
    W = nmf.W.copy()
    nmf._beta = 1.
    try:
        with pytest.raises(NotImplementedError):
            nmf.fit_detections(det, 1)
    finally:
        nmf._beta = 2.
    nmf._weighted = True
    try:
        with pytest.raises(NotImplementedError):
            nmf.fit_detections(det, 1)
    finally:
        nmf._weighted = False
    assert nmf.W.tobytes() == W.tobytes()


# -- 4. the ABI -------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_typed():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tnmf_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    vp, ll, ci = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    gp = ctypes.POINTER(_lib.Geom)
    name = 'tnmf_hip_events_grad_W'
    assert re.search(r'\bint %s\s*\(' % name, header)
    assert name in _lib.EXPORTS
    fn = getattr(lib, name)
    assert fn.restype is ci and list(fn.argtypes) == [vp, gp, ci, vp, vp, vp, vp, ll, vp, vp, vp, vp, vp]
    assert _lib.ABI_VERSION == 8 and lib.tnmf_hip_abi_version() == 8
    assert _lib.EVENT_SEGMENT == int(re.search(r'#define TNMF_EVENTS_SEGMENT (\d+)', header).group(1))
    # argument errors are answered without a device: no context
    g = _lib.make_geom(1, 1, 1, (4,), (2,), 0)
    assert fn(None, ctypes.byref(g), 0, None, None, None, None, 0, None, None, None, None, None) == -1
