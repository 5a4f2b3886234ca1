"""
Gains of events on CPU: the host fallback ``events_gain_numpy`` and the front end's ``detection_gains`` /
``prune_detections`` over an oracle-backed backend without the events hooks, in float64, against
tests/events_gain_reference.py -- the gain read literally as a difference of two energies, and its closed form.

The bar: |closed form - difference| <= 1e-10 * (E + mag_e), E the energy of the list and mag_e the sum of the magnitudes of
the closed form's terms.  Both sides are float64 sums over at most ~1e4 pixels, whose rounding is of the order
2^-53 * pixels * E ~ 1e-12 * E: two orders below the bar.
"""
import ctypes
import dataclasses
import functools
import os
import re

import numpy as np
import pytest

import events_gain_reference as gref
import events_reference as eref
from conftest import ROOT
from test_events_cpu import MODES, SHAPES, _Stub, fitted, hand_made
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import (Detections, TransformInvariantNMF, event_boxes, event_images,
                                            events_gain_numpy)

BAR = 1e-10


def rows_of(det, keep):
    return Detections(**{f.name: getattr(det, f.name)[keep] for f in dataclasses.fields(Detections)})


# -- 1. the closed form is the difference of the energies ---------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', ['1d', '2d'])
def test_closed_form_equals_the_leave_one_out_difference(case, mode):
    """hand_made() has the corners of the shift range -- in 'valid' mode occurrences that overhang the sample -- and rows in
    the wrap / mirror zone of EVERY axis; two rows are given twice and one has strength 0."""
    D, A = SHAPES[case]
    S = eref.shift_shape(D, A, mode)
    rng = np.random.default_rng(31)
    W, V = rng.random((3, 2) + A), rng.random((2, 2) + D) + 0.1
    sample, plane, shift, h = hand_made(D, A, mode, seed=6, n_random=8)
    h = h * rng.random(len(h))
    h[4] = 0.
    sample, plane, shift, h = (np.concatenate([x, x[:2]]) for x in (sample, plane, shift, h))   # duplicates
    n_images = np.bincount(event_images(shift, A, S, mode)[0], minlength=len(h))
    assert n_images.max() == (2 ** len(D) if mode in ('circular', 'reflect') else 1)
    if mode in ('circular', 'reflect'):
        assert set(n_images.tolist()) >= {1, 2}
    if mode == 'valid':   # the first corner shows one pixel of the atom
        assert len(list(eref.pixels(W, D, mode, 0, 0, (0,) * len(D)))) == W.shape[1]
    want, E = gref.leave_one_out(V, W, mode, sample, plane, shift, h)
    R = eref.render(W, D, 2, mode, sample, plane, shift, h)
    closed, mag = gref.closed_form(V, R, W, mode, sample, plane, shift, h)
    host = events_gain_numpy(W, D, 2, mode, sample, plane, shift, h, V)
    assert host.dtype == np.float64 and host.shape == h.shape
    bar = BAR * (E + mag)
    print(f'{case} {mode}: closed form vs difference {np.abs(closed - want).max():.3g}, host fallback '
          f'{np.abs(host - want).max():.3g}, bar >= {bar.min():.3g}')
    assert np.all(np.abs(closed - want) <= bar) and np.all(np.abs(host - want) <= bar)
    assert closed[4] == 0. and host[4] == 0. and mag[4] == 0.
    assert np.array_equal(closed[-2:], closed[:2]) and np.array_equal(host[-2:], host[:2])   # each against the whole list
    assert np.abs(want).max() > 1e-3


def test_overlapping_images_are_added_before_they_are_squared():
    """'reflect', u = 1 on a 4-tap atom: the images at offsets +1 and -1 share pixels, so b is not the sum of two norms."""
    W = np.arange(1., 5.).reshape(1, 1, 4)
    V = np.zeros((1, 1, 9))
    sample, plane, shift, h = np.array([0]), np.array([0]), np.array([[1]]), np.array([2.])
    phi = np.zeros(9)
    phi[1:5] += W[0, 0]
    phi[0:3] += W[0, 0, 1:]
    want = 0.5 * 4. * np.sum(phi * phi) - 2. * np.sum(phi * 2. * phi)      # h^2 b / 2 + h <phi, 0 - h phi>
    R = eref.render(W, (9,), 1, 'reflect', sample, plane, shift, h)
    assert np.array_equal(R[0, 0], 2. * phi)
    for got in (gref.closed_form(V, R, W, 'reflect', sample, plane, shift, h)[0],
                gref.leave_one_out(V, W, 'reflect', sample, plane, shift, h)[0],
                events_gain_numpy(W, (9,), 1, 'reflect', sample, plane, shift, h, V)):
        assert got[0] == want
    assert want != 0.5 * 4. * (np.sum(W ** 2) + np.sum(W[0, 0, 1:] ** 2)) - 2. * np.sum(phi * 2. * phi)


# -- 2. the front end --------------------------------------------------------------------------------------------------------
def check_model(nmf, n_rows=30):
    """detection_gains of the strongest rows of a fitted model against the leave-one-out difference."""
    be = nmf._backend
    mode = be._reconstruction_mode
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)), min_distance=1)
    det = rows_of(det, np.argsort(-det.strength, kind='stable')[:n_rows])
    assert len(det) > 5
    W = np.asarray(nmf.transformed_atoms, dtype=np.float64).reshape((-1,) + nmf.W.shape[1:])
    V = np.asarray(nmf.V, dtype=np.float64)[be.shard[0]:be.shard[1]]
    sample, plane = det.sample - be.shard[0], det.atom * nmf.n_transforms + det.transform
    want, E = gref.leave_one_out(V, W, mode, sample, plane, det.shift, det.strength)
    R = eref.render(W, V.shape[2:], len(V), mode, sample, plane, det.shift, det.strength)
    _, mag = gref.closed_form(V, R, W, mode, sample, plane, det.shift, det.strength)
    got = nmf.detection_gains(det)
    assert got.dtype == np.float64 and got.shape == (len(det),)
    print(f'{mode}: detection_gains({len(det)}) vs difference {np.abs(got - want).max():.3g} of {np.abs(want).max():.3g}')
    assert np.all(np.abs(got - want) <= BAR * (E + mag))
    return det, got


@pytest.mark.parametrize('mode', MODES)
def test_detection_gains_of_a_fitted_model(mode):
    check_model(fitted((3, 2, 9, 10), 2, (3, 4), mode))
    check_model(fitted((3, 1, 25), 2, (5,), mode))


def test_with_rot90_the_gain_is_that_of_the_oriented_atom():
    det, _ = check_model(fitted((2, 1, 8, 8), 2, (3, 3), 'circular', transforms='rot90'))
    assert len(set(det.transform.tolist())) > 1


def test_under_a_shuffle_and_on_the_block_of_a_rank():
    nmf = fitted((5, 1, 9, 8), 2, (3, 3), minibatches=True)
    nmf._shuffle_idx = np.array([3, 0, 4, 1, 2])
    check_model(nmf)
    det, _ = check_model(fitted((6, 1, 20), 2, (4,), shard=(2, 5)))
    assert set(det.sample.tolist()) <= {2, 3, 4}


def test_after_a_long_refit_the_gain_is_half_h_squared_b():
    """gain - h^2 b / 2 = h a, and a = neg - pos in the terms of the refit step h' = h neg / (pos + eps): with the relative
    change r = h' / h - 1 of one more step, h a = h ((pos + eps) r + eps) -- the refit's residual.  The gains must equal
    h^2 b / 2 within that (and the rounding bar), and the residual must be small for the test to say anything."""
    nmf = fitted((2, 1, 12, 13), 2, (3, 3), 'reflect')
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.97)), min_distance=2)
    assert 5 < len(det) < 40
    long = nmf.refit_detections(det, 3000)
    step = nmf.refit_detections(long, 1).strength
    h = long.strength
    live = h > 0
    r = np.zeros(len(h))
    r[live] = np.abs(step[live] / h[live] - 1.)
    W, V = np.asarray(nmf.W, dtype=np.float64), np.asarray(nmf.V, dtype=np.float64)
    R = eref.render(W, V.shape[2:], len(V), 'reflect', det.sample, det.atom, det.shift, h)
    b, pos = np.zeros(len(h)), np.zeros(len(h))
    for e in range(len(h)):
        taps = list(eref.pixels(W, V.shape[2:], 'reflect', det.sample[e], det.atom[e], det.shift[e]))
        phi = {}
        for at, w in taps:
            phi[at] = phi.get(at, 0.) + w
        b[e] = sum(w * phi[at] for at, w in taps)
        pos[e] = sum(w * R[at] for at, w in taps)
    gains = nmf.detection_gains(long)
    _, mag = gref.closed_form(V, R, W, 'reflect', det.sample, det.atom, det.shift, h)
    residual = h * ((pos + nmf.eps) * r + nmf.eps)
    print(f'largest relative change of one more step {r.max():.3g}; |gain - h^2 b / 2| '
          f'{np.abs(gains - 0.5 * h * h * b).max():.3g} of {gains.max():.3g}, residual {residual.max():.3g}')
    assert np.all(np.abs(gains - 0.5 * h * h * b) <= residual * (1 + 1e-6) + BAR * mag)
    assert residual.max() <= 1e-6 * gains.max()
    assert np.all(gains >= -residual - BAR * mag)


# -- 3. pruning ---------------------------------------------------------------------------------------------------------------
MIN_GAIN = 2e-3
PLANTED_SEED = 0


@functools.lru_cache(maxsize=None)
def planted_model():
    """The planted problem (events_gain_reference.planted) under a float64 model that holds its dictionary."""
    case = gref.planted(PLANTED_SEED)
    nmf = TransformInvariantNMF(n_atoms=case['W'].shape[0], atom_shape=case['W'].shape[2:], backend=_Stub(case['mode']))
    nmf._W = np.array(case['W'])
    np.random.seed(42)
    nmf.fit(np.array(case['V']), n_iterations=0, keep_W=True)
    assert np.array_equal(nmf.W, case['W'])
    det = Detections(sample=case['sample'], atom=case['plane'], transform=np.zeros_like(case['plane']), shift=case['shift'],
                     origin=case['shift'] - 3, strength=case['strength'])
    return nmf, det, case


def key(det):
    return sorted(map(tuple, np.column_stack([det.sample, det.atom, det.transform, det.shift]).tolist()))


def test_prune_keeps_exactly_the_planted_rows():
    nmf, det, case = planted_model()
    pruned, gains = nmf.prune_detections(det, MIN_GAIN)
    assert isinstance(pruned, Detections) and gains.dtype == np.float64 and gains.shape == (len(pruned),)
    assert key(pruned) == key(rows_of(det, case['true'])) and len(pruned) == int(case['true'].sum()) < len(det)
    # the survivors keep their order and are refitted: near the planted strengths, V being their render plus noise below 0.01
    # per pixel, which moves the strength of an occurrence alone by at most 0.01 * sum(w) / |w|^2 <= 0.16 (16 taps, sum 1)
    want = rows_of(det, case['true'])
    for name in ('sample', 'atom', 'transform', 'shift', 'origin'):
        np.testing.assert_array_equal(getattr(pruned, name), getattr(want, name))
    np.testing.assert_allclose(pruned.strength, want.strength, rtol=0, atol=0.16)
    # ... and carry their final gains: those of the returned list
    np.testing.assert_allclose(gains, nmf.detection_gains(pruned), rtol=1e-12)
    assert gains.min() >= MIN_GAIN
    # every round's gains stay clear of the threshold by more than 1e-3 relative, so no other arithmetic flips a row;
    # the neighbouring spurious rows overlap, so one round cannot drop both
    sizes, r = [], 0
    while True:
        rows, g = nmf.prune_detections(det, MIN_GAIN, max_rounds=r)
        assert np.all(np.abs(g - MIN_GAIN) > 1e-3 * MIN_GAIN), (r, g)
        sizes.append(len(rows))
        if len(sizes) > 1 and sizes[-1] == sizes[-2]:
            break
        r += 1
    print(f'rows per round {sizes}')
    assert len(sizes) >= 4 and sizes[-1] == len(pruned) and sizes[0] == len(det)


def test_rows_with_meeting_boxes_are_not_dropped_in_one_round():
    nmf, det, case = planted_model()
    once, _ = nmf.prune_detections(det, MIN_GAIN, max_rounds=1)
    gone = sorted(set(key(det)) - set(key(once)))
    assert len(gone) >= 2 and not set(gone) & set(key(rows_of(det, case['true'])))
    lo, hi = event_boxes(np.array([g[3:] for g in gone]), (4, 4), (24, 26), (27, 29), 'valid')
    for i in range(len(gone)):
        for j in range(i):
            if gone[i][0] == gone[j][0]:
                assert not np.all(np.maximum(lo[i], lo[j]) < np.minimum(hi[i], hi[j])), (gone[i], gone[j])


def test_zero_rounds_is_a_refit_with_its_gains():
    nmf, det, _ = planted_model()
    rows, gains = nmf.prune_detections(det, MIN_GAIN, n_iterations=7, sparsity_H=0.01, max_rounds=0)
    refit = nmf.refit_detections(det, 7, sparsity_H=0.01)
    for f in dataclasses.fields(Detections):
        assert np.array_equal(getattr(rows, f.name), getattr(refit, f.name))
    assert np.array_equal(gains, nmf.detection_gains(refit))
    none = rows_of(det, np.zeros(len(det), dtype=bool))
    rows, gains = nmf.prune_detections(none, MIN_GAIN)
    assert len(rows) == 0 and gains.shape == (0,) and nmf.detection_gains(none).shape == (0,)
    everything, _ = nmf.prune_detections(det, -1e300)       # nothing lies below: one round, no row leaves
    assert key(everything) == key(det)


def test_event_boxes():
    lo, hi = event_boxes(np.array([[0, 0], [2, 11], [1, 1]]), (3, 4), (8, 9), (10, 12), 'valid')
    assert lo.tolist() == [[0, 0], [0, 8], [0, 0]] and hi.tolist() == [[1, 1], [3, 9], [2, 2]]
    lo, hi = event_boxes(np.array([[7, 8], [3, 3]]), (3, 4), (8, 9), (8, 9), 'circular')   # wraps on both axes: the whole span
    assert lo.tolist() == [[0, 0], [3, 3]] and hi.tolist() == [[8, 9], [6, 7]]


# -- 4. refusals --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model():
    nmf = fitted((2, 1, 9, 10), 2, (3, 4), 'reflect')
    return nmf, nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)), min_distance=0)


def test_before_a_fit_both_raise_runtime_error(model):
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 4), backend=_Stub())
    with pytest.raises(RuntimeError):
        nmf.detection_gains(model[1])
    with pytest.raises(RuntimeError):
        nmf.prune_detections(model[1], 0.1)


def test_they_are_frobenius_and_unweighted(model):
    nmf, det = model
    for name, value, back in (('_beta', 1., 2.), ('_weighted', True, False)):
        setattr(nmf, name, value)
        try:
            with pytest.raises(NotImplementedError):
                nmf.detection_gains(det)
            with pytest.raises(NotImplementedError):
                nmf.prune_detections(det, 0.1)
        finally:
            setattr(nmf, name, back)
    assert nmf.detection_gains(det).shape == (len(det),)


def test_volumes_are_refused():
    nmf = fitted((1, 1, 5, 5, 5), 1, (2, 2, 2))
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)), min_distance=0)
    with pytest.raises(NotImplementedError):
        nmf.detection_gains(det)
    with pytest.raises(NotImplementedError):
        nmf.prune_detections(det, 0.1)


@pytest.mark.parametrize('kw', [dict(min_gain=float('nan')), dict(min_gain=float('inf')), dict(min_gain='0.1'),
                                dict(min_gain=True), dict(min_gain=None), dict(min_gain=0.1, max_rounds=-1),
                                dict(min_gain=0.1, max_rounds=1.5), dict(min_gain=0.1, max_rounds=True),
                                dict(min_gain=0.1, n_iterations=-1), dict(min_gain=0.1, sparsity_H=-1.)], ids=str)
def test_bad_prune_arguments_raise_value_error(model, kw):
    nmf, det = model
    with pytest.raises(ValueError):
        nmf.prune_detections(det, **kw)


def test_bad_rows_raise_value_error_and_duplicates_are_scored_but_not_pruned(model):
    nmf, det = model
    bad = dataclasses.replace(det, strength=np.where(np.arange(len(det)) == 1, -1., det.strength))
    with pytest.raises(ValueError):
        nmf.detection_gains(bad)
    with pytest.raises(ValueError):
        nmf.prune_detections(bad, 0.1)
    twice = rows_of(det, np.r_[np.arange(len(det)), 0])
    gains = nmf.detection_gains(twice)
    assert gains[-1] == gains[0]
    with pytest.raises(ValueError):
        nmf.prune_detections(twice, 0.1)


# -- 5. the ABI ---------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_typed():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tnmf_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    vp, ll, ci = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    assert re.search(r'\bint tnmf_hip_events_gain\s*\(', header) and 'tnmf_hip_events_gain' in _lib.EXPORTS
    fn = lib.tnmf_hip_events_gain
    assert fn.restype is ci
    assert list(fn.argtypes) == [vp, ctypes.POINTER(_lib.Geom), ci, vp, vp, vp, ll, vp, vp, vp, vp, vp]
    assert _lib.ABI_VERSION == 8
    g = _lib.make_geom(1, 1, 1, (4,), (2,), 0)   # an argument error is answered without a device: no context
    assert fn(None, ctypes.byref(g), 0, None, None, None, 0, None, None, None, None, None) == -1
