"""
The landscape of events on CPU: the host fallback ``events_landscape_numpy`` and the front end's ``detection_landscape`` /
``refine_detections`` / ``relocate_detections`` over an oracle-backed backend without the events hooks, in float64, against
tests/landscape_reference.py -- g = a^2 / (2 b) read literally as a difference of two energies of actual renders.

The bar of the brute force: 1e-10 of 1/2 ||V||^2.  Every energy is a float64 sum over a few hundred pixels of terms below
||V||^2, rounded to ~1e-14 of it, and the difference of two of them carries no more: four orders below the bar.
"""
import ctypes
import dataclasses
import functools
import itertools
import os
import re

import numpy as np
import pytest

import events_gain_reference as gref
import events_reference as eref
import landscape_reference as lref
from conftest import ROOT
from test_events_cpu import MODES, _Stub, fitted
from tnmf_amd import _lib
from tnmf_amd.events_host import events_gain_numpy, events_landscape_numpy, landscape_gains, relocation_hops
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF

BAR = 1e-10
GEOMETRIES = {'1d': ((40,), (5,), 1), '3x3-c1': ((12, 14), (3, 3), 1), '3x3-c3': ((12, 14), (3, 3), 3),
              '5x7-c1': ((12, 14), (5, 7), 1), '5x7-c3': ((12, 14), (5, 7), 3)}


def rows_of(det, keep):
    return Detections(**{f.name: getattr(det, f.name)[keep] for f in dataclasses.fields(Detections)})


def key(det):
    return sorted(map(tuple, np.column_stack([det.sample, det.atom, det.transform, det.shift]).tolist()))


def holding(W, V, mode):
    """A float64 model over the oracle backend that holds the dictionary W and the samples V."""
    nmf = TransformInvariantNMF(n_atoms=W.shape[0], atom_shape=W.shape[2:], backend=_Stub(mode))
    nmf._W = np.array(W)
    np.random.seed(42)
    nmf.fit(np.array(V), n_iterations=0, keep_W=True)
    assert np.array_equal(nmf.W, W)
    return nmf


def as_det(sample, plane, shift, strength, A, mode, T=1):
    shift = np.asarray(shift, dtype=np.int64).reshape(len(sample), -1)
    offset = np.array([a - 1 if mode == 'valid' else 0 for a in A], dtype=np.int64)
    plane = np.asarray(plane, dtype=np.int64)
    return Detections(sample=np.asarray(sample, dtype=np.int64), atom=plane // T, transform=plane % T, shift=shift,
                      origin=shift - offset, strength=np.asarray(strength))


@functools.lru_cache(maxsize=None)
def problem(name, mode):
    """-> (V, W, sample, plane, shift, h, names): every place of landscape_reference.places() on sample 1, two of them twice
    and one with strength 0, and a few rows of sample 0."""
    D, A, C = GEOMETRIES[name]
    rng = np.random.default_rng(17)
    W, V = rng.random((2, C) + A) + 0.1, rng.random((2, C) + D) * 2.
    at = lref.places(D, A, mode)
    names = list(at) + ['interior', 'corner0']                  # duplicates
    shift = np.array([at[n] for n in names], dtype=np.int64)
    sample = np.ones(len(names), dtype=np.int64)
    plane = (np.arange(len(names)) % 2).astype(np.int64)
    plane[-2:] = plane[[names.index('interior'), names.index('corner0')]]
    h = rng.random(len(names)) + 0.5
    h[-2:] = h[[names.index('interior'), names.index('corner0')]]
    h[names.index('far')] = 0.
    S = eref.shift_shape(D, A, mode)
    extra = np.column_stack([rng.integers(s, size=3) for s in S])
    sample, plane = np.concatenate([sample, [0, 0, 0]]), np.concatenate([plane, [0, 1, 0]])
    shift, h = np.concatenate([shift, extra]), np.concatenate([h, [1., 0.5, 2.]])
    return V, W, sample, plane, shift, h, names + ['extra'] * 3


# -- 1. the landscape is the difference of the energies ------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(GEOMETRIES))
def test_brute_force(name, mode):
    V, W, sample, plane, shift, h, names = problem(name, mode)
    D, A, C = GEOMETRIES[name]
    k, S = len(D), eref.shift_shape(D, A, mode)
    nmf = holding(W, V, mode)
    a, b = nmf.detection_landscape(as_det(sample, plane, shift, h, A, mode))
    assert a.shape == b.shape == (len(h),) + (3,) * k and a.dtype == b.dtype == np.float64
    a, b = a.reshape(len(h), -1), b.reshape(len(h), -1)
    host = events_landscape_numpy(W, D, 2, mode, sample, plane, shift, h, V, with_magnitude=True)
    assert np.array_equal(host[0], a) and np.array_equal(host[1], b)
    R = eref.render(W, D, 2, mode, sample, plane, shift, h)
    ra, rb, rmag = lref.landscape(V, R, W, mode, sample, plane, shift, h)
    want = lref.brute_force(V, W, mode, sample, plane, shift, h, ra, rb)
    scale = 0.5 * float(np.sum(V * V))
    g = landscape_gains(a, b)
    print(f'{name} {mode}: {len(h)} rows; |g - brute force| <= {np.abs(g - want).max():.3g}, reference '
          f'{np.abs(lref.gains(ra, rb) - want).max():.3g}, bar {BAR * scale:.3g}; g up to {g.max():.3g}')
    assert np.all(np.abs(g - want) <= BAR * scale) and np.all(np.abs(lref.gains(ra, rb) - want) <= BAR * scale)
    assert np.all(np.abs(a - ra) <= 1e-12 * rmag) and np.all(np.abs(b - rb) <= 1e-12 * rb)
    assert np.all(np.abs(host[2] - rmag) <= 1e-12 * rmag)
    assert g.max() > 1e-3 * scale
    # the places: a neighbour outside the shift shape gives exactly 0, and only that one (b > 0 wherever phi has a pixel)
    outside = np.array([[not all(0 <= x + d < s for x, d, s in zip(u, delta, S)) for delta in lref.deltas(k)]
                        for u in shift])
    assert outside.any() and not a[outside].any() and not b[outside].any() and np.all(b[~outside] > 0)
    for corner in ('corner0', f'corner{2 ** k - 1}'):
        assert outside[names.index(corner)].sum() == 3 ** k - 2 ** k
    # duplicates put back only themselves: the same numbers twice; a zero strength is a row like any other
    for twin, first in ((-5, names.index('interior')), (-4, names.index('corner0'))):
        assert np.array_equal(a[twin], a[first]) and np.array_equal(b[twin], b[first])
    assert h[names.index('far')] == 0. and a[names.index('far')].any()
    n_images = np.bincount(eref_images(shift, A, S, mode), minlength=len(h))
    if mode in ('circular', 'reflect'):
        assert set(n_images.tolist()) == ({1, 2} if k == 1 else {1, 2, 4})
    # both paths of the kernel have rows here
    st = lref.staged((2, C, 2, D, A, mode), shift)
    assert not st[names.index('edge')] and not st[names.index('corner0')] and not st.all()
    # (5 x 7 in 'reflect' on 12 x 14: the mirror zone and the far border leave no shift with whole neighbours)
    assert st[names.index('interior')] == lref.staged((2, C, 2, D, A, mode), list(np.ndindex(*S))).any()
    assert st[names.index('interior')] or (name.startswith('5x7') and mode == 'reflect')


def eref_images(shift, A, S, mode):
    return np.concatenate([[e] * len(eref.images(u, A, S, mode)) for e, u in enumerate(shift)]).astype(np.int64)


def test_brute_force_with_rot90():
    nmf = fitted((2, 1, 10, 11), 2, (3, 3), 'circular', transforms='rot90')
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)), min_distance=1)
    det = rows_of(det, np.argsort(-det.strength, kind='stable')[:16])
    assert len(set(det.transform.tolist())) > 1
    W = np.asarray(nmf.transformed_atoms, dtype=np.float64).reshape((-1,) + nmf.W.shape[1:])
    V = np.asarray(nmf.V, dtype=np.float64)
    plane = det.atom * 4 + det.transform
    a, b = (x.reshape(len(det), 9) for x in nmf.detection_landscape(det))
    R = eref.render(W, V.shape[2:], 2, 'circular', det.sample, plane, det.shift, det.strength)
    ra, rb, _ = lref.landscape(V, R, W, 'circular', det.sample, plane, det.shift, det.strength)
    want = lref.brute_force(V, W, 'circular', det.sample, plane, det.shift, det.strength, ra, rb)
    scale = 0.5 * float(np.sum(V * V))
    assert np.all(np.abs(landscape_gains(a, b) - want) <= BAR * scale) and np.abs(want).max() > 1e-4 * scale


# -- 2. the identities with the gains -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['1d', '5x7-c3'])
def test_identities_with_the_gains(name, mode):
    V, W, sample, plane, shift, h, _ = problem(name, mode)
    D, A, C = GEOMETRIES[name]
    a, b = events_landscape_numpy(W, D, 2, mode, sample, plane, shift, h, V)
    centre = (a.shape[1] - 1) // 2
    R = eref.render(W, D, 2, mode, sample, plane, shift, h)
    gain, mag = gref.closed_form(V, R, W, mode, sample, plane, shift, h)
    # a_e = <phi, V - R> of the gains, read off rows of strength 1 (gain = a_e + b / 2 there) -- and in general:
    a_e = a[:, centre] - h * b[:, centre]
    want = events_gain_numpy(W, D, 2, mode, sample, plane, shift, h, V)
    scale = mag + h * h * b[:, centre] + 1e-300
    assert np.all(np.abs(h * a_e + 0.5 * h * h * b[:, centre] - want) <= 1e-12 * scale)
    assert np.all(np.abs(h * a_e + 0.5 * h * h * b[:, centre] - gain) <= 1e-12 * scale)
    ones = events_gain_numpy(W, D, 2, mode, sample, plane, shift, np.ones_like(h), V)
    a1, b1 = events_landscape_numpy(W, D, 2, mode, sample, plane, shift, np.ones_like(h), V)
    assert np.allclose(a1[:, centre] - b1[:, centre], ones - 0.5 * b1[:, centre], rtol=0, atol=1e-11 * np.abs(a1).max())


# -- 3. refine ------------------------------------------------------------------------------------------------------------------
def blob(A):
    """A symmetric, single-peaked atom of small integers: every sum of the landscape is exact, so equal ones are equal."""
    axes = [2. ** np.minimum(np.arange(a), np.arange(a)[::-1]) for a in A]
    return functools.reduce(np.multiply.outer, axes)[None, None]


@pytest.mark.parametrize('k', [1, 2])
def test_refine_a_symmetric_landscape_and_a_blend(k):
    D, A = ((30,), (5,)) if k == 1 else ((16, 18), (5, 5))
    W = blob(A)
    u = tuple(d // 2 for d in D)
    one = (np.array([0]), np.array([0]))
    V = eref.render(W, D, 1, 'full', *one, np.array([u]), np.array([2.]))
    nmf = holding(W, V, 'full')
    det = as_det(*one, [u], [1.5], A, 'full')
    offset, gain, peak = nmf.refine_detections(det)
    assert offset.shape == (1, k) and offset.dtype == np.float64 and peak.dtype == bool and gain.shape == (1,)
    assert np.all(offset == 0.) and peak[0] and gain[0] == pytest.approx(0.5 * 4. * np.sum(W * W), rel=1e-12)
    for axis in range(k):
        for sign in (1, -1):
            e = np.zeros(k, dtype=np.int64)
            e[axis] = sign
            V = (0.75 * eref.render(W, D, 1, 'full', *one, np.array([u]), np.array([2.]))
                 + 0.25 * eref.render(W, D, 1, 'full', *one, np.array([u]) + e, np.array([2.])))
            nmf = holding(W, V, 'full')
            offset, gain, peak = nmf.refine_detections(det)
            assert peak[0] and 0 < sign * offset[0, axis] < 0.5, offset
            assert np.all(np.delete(offset[0], axis) == 0.)
            a, b = nmf.detection_landscape(det)
            want = lref.refine(a, b, k)
            assert np.array_equal(offset, want[0]) and np.array_equal(gain, want[1]) and np.array_equal(peak, want[2])
            assert det.origin[0, axis] + offset[0, axis] == pytest.approx(u[axis] + 0.25 * sign, abs=0.15)


@pytest.mark.parametrize('mode', MODES)
def test_refine_equals_the_formula_on_the_reference_landscape(mode):
    V, W, sample, plane, shift, h, names = problem('5x7-c1', mode)
    D, A, C = GEOMETRIES['5x7-c1']
    nmf = holding(W, V, mode)
    offset, gain, peak = nmf.refine_detections(as_det(sample, plane, shift, h, A, mode))
    R = eref.render(W, D, 2, mode, sample, plane, shift, h)
    ra, rb, _ = lref.landscape(V, R, W, mode, sample, plane, shift, h)
    want = lref.refine(ra, rb, 2)
    assert np.array_equal(peak, want[2]) and np.allclose(gain, want[1], rtol=1e-11, atol=0)
    assert np.allclose(offset, want[0], rtol=0, atol=1e-8) and np.all(np.abs(offset) <= 0.5)
    # a row that is no maximum along an axis: no peak, offset 0 there (peaks: the tests of the blob above)
    assert (~peak).any()
    for e in np.flatnonzero(~peak):
        assert (offset[e] == 0.).any()


def test_a_row_that_is_not_a_local_maximum():
    W = blob((5, 5))
    D, u = (16, 18), (8, 9)
    one = (np.array([0]), np.array([0]))
    V = eref.render(W, D, 1, 'full', *one, np.array([u]), np.array([2.]))
    nmf = holding(W, V, 'full')
    offset, gain, peak = nmf.refine_detections(as_det(*one, [(u[0] + 2, u[1])], [1.], (5, 5), 'full'))
    assert not peak[0] and offset[0, 0] == 0. and offset[0, 1] == 0. and gain[0] > 0   # (axis 1 is symmetric: exactly 0)


# -- 4. relocate ----------------------------------------------------------------------------------------------------------------
SCENE_SEED = 3


@functools.lru_cache(maxsize=None)
def scene(seed=SCENE_SEED, mode='valid'):
    """A noiseless planted scene: per sample 10 of the 16 cells of 10 x 10 pixels hold one occurrence of a 4 x 4 atom, 2 or 3
    pixels inside the cell, so the footprints of the rows and of all their neighbours keep to their cells; and the same
    rows displaced by one pixel, each by its own nonzero delta."""
    rng = np.random.default_rng(seed)
    D, A, N, M = (40, 40), (4, 4), 2, 2
    W = rng.random((M, 1) + A) + 0.1
    W = (W / W.sum(axis=(2, 3), keepdims=True)).astype(np.float32).astype(np.float64)   # (both element types hold it)
    first = np.array([a - 1 if mode == 'valid' else 0 for a in A])
    rows = []
    for n in range(N):
        for cell in rng.permutation(16)[:10]:
            origin = np.array([cell // 4, cell % 4]) * 10 + rng.integers(2, 4, 2)
            rows.append((n, int(rng.integers(M))) + tuple(int(x) for x in origin + first))
    rows = np.array(rows, dtype=np.int64)[rng.permutation(len(rows))]
    h = 1. + rng.integers(0, 9, len(rows)) / 8.
    V = eref.render(W, D, N, mode, rows[:, 0], rows[:, 1], rows[:, 2:], h).astype(np.float32).astype(np.float64)
    nonzero = np.array([d for d in lref.deltas(2) if any(d)])
    moved = rows.copy()
    moved[:, 2:] += nonzero[rng.integers(len(nonzero), size=len(rows))]
    for x in (W, V, rows, moved, h):
        x.setflags(write=False)
    return dict(W=W, V=V, D=D, A=A, mode=mode, rows=rows, moved=moved, h=h)


def scene_det(sc, rows, h=None):
    return as_det(rows[:, 0], rows[:, 1], rows[:, 2:], sc['h'] if h is None else h, sc['A'], sc['mode'])


def objective_of(nmf, det):
    return 0.5 * float(np.sum((np.asarray(nmf.V, dtype=np.float64) - nmf.reconstruct_detections(det)) ** 2))


def test_the_reference_landscape_recovers_the_scene():
    """The seed of the scene is held to this: at every displaced row the reference's best neighbour is the planted place."""
    sc = scene()
    rows, moved = sc['rows'], sc['moved']
    R = eref.render(sc['W'], sc['D'], 2, sc['mode'], moved[:, 0], moved[:, 1], moved[:, 2:], sc['h'])
    a, b, _ = lref.landscape(sc['V'], R, sc['W'], sc['mode'], moved[:, 0], moved[:, 1], moved[:, 2:], sc['h'])
    g = lref.gains(a, b)
    back = np.array([lref.deltas(2).index(tuple(d)) for d in (rows[:, 2:] - moved[:, 2:]).tolist()])
    assert np.array_equal(np.argmax(g, axis=1), back) and len(rows) == 20 and np.all(back != 4)


def test_relocate_recovers_the_planted_rows():
    sc = scene()
    nmf = holding(sc['W'], sc['V'], sc['mode'])
    start = scene_det(sc, sc['moved'])
    got, gains = nmf.relocate_detections(start)
    want = scene_det(sc, sc['rows'])
    assert isinstance(got, Detections) and gains.dtype == np.float64 and gains.shape == (len(got),)
    for name in ('sample', 'atom', 'transform', 'shift', 'origin'):      # row by row: the order is kept
        np.testing.assert_array_equal(getattr(got, name), getattr(want, name))
    np.testing.assert_allclose(got.strength, want.strength, rtol=1e-6)
    scale = 0.5 * float(np.sum(sc['V'] ** 2))
    E = objective_of(nmf, got)
    print(f'objective {E:.3g} of {scale:.3g}; history {nmf.relocation_history_.tolist()}')
    assert E <= 1e-8 * scale < objective_of(nmf, nmf.refit_detections(start))
    np.testing.assert_allclose(gains, nmf.detection_gains(got), rtol=1e-12)
    hist = nmf.relocation_history_
    assert hist.shape == (2, 3) and hist[0, :2].tolist() == [20., 20.] and hist[1].tolist() == [0., 0., 0.]
    # the hops' improvements add up to what the objective fell by: their footprints are disjoint
    before = objective_of(nmf, nmf.refit_detections(start))
    hopped, _ = nmf.relocate_detections(start, n_iterations=50, max_rounds=1)
    assert hist[0, 2] == pytest.approx(before - objective_of(nmf, hopped), rel=1e-6)
    # a list at a local optimum comes back unchanged after one round
    again, _ = nmf.relocate_detections(got)
    assert key(again) == key(got) and nmf.relocation_history_.tolist() == [[0., 0., 0.]]
    assert np.array_equal(again.shift, got.shift)


def test_zero_rounds_is_a_refit_with_its_gains():
    sc = scene()
    nmf = holding(sc['W'], sc['V'], sc['mode'])
    start = scene_det(sc, sc['moved'])
    rows, gains = nmf.relocate_detections(start, n_iterations=7, sparsity_H=0.01, max_rounds=0)
    refit = nmf.refit_detections(start, 7, sparsity_H=0.01)
    for f in dataclasses.fields(Detections):
        assert np.array_equal(getattr(rows, f.name), getattr(refit, f.name))
    assert np.array_equal(gains, nmf.detection_gains(refit)) and nmf.relocation_history_.shape == (0, 3)
    none = rows_of(start, np.zeros(len(start), dtype=bool))
    rows, gains = nmf.relocate_detections(none)
    assert len(rows) == 0 and gains.shape == (0,)
    a, b = nmf.detection_landscape(none)
    assert a.shape == b.shape == (0, 3, 3) and nmf.refine_detections(none)[0].shape == (0, 2)


def test_rows_with_meeting_footprints_hop_in_different_rounds():
    sc = scene()
    W, A, D = sc['W'], sc['A'], sc['D']
    true = np.array([[0, 0, 13, 13], [0, 1, 13, 18], [0, 1, 30, 30]])          # origins (10, 10), (10, 15): one pixel apart
    h = np.array([1.5, 1.25, 2.])
    V = eref.render(W, D, 1, 'valid', true[:, 0], true[:, 1], true[:, 2:], h)
    moved = true + np.array([[0, 0, 0, 1], [0, 0, 0, -1], [0, 0, 1, 0]])       # the first two towards each other
    nmf = holding(W, V, 'valid')
    got, _ = nmf.relocate_detections(as_det(moved[:, 0], moved[:, 1], moved[:, 2:], h, A, 'valid'))
    hist = nmf.relocation_history_
    print(hist.tolist())
    assert np.array_equal(got.shift, true[:, 2:])
    assert hist[:, :2].tolist() == [[3., 2.], [1., 1.], [0., 0.]]
    once, _ = nmf.relocate_detections(as_det(moved[:, 0], moved[:, 1], moved[:, 2:], h, A, 'valid'), max_rounds=1)
    assert np.array_equal(once.shift[2], true[2, 2:]) and np.sum(np.all(once.shift[:2] == true[:2, 2:], axis=1)) == 1
    # the objective never rises from round to round
    E = [objective_of(nmf, nmf.relocate_detections(as_det(moved[:, 0], moved[:, 1], moved[:, 2:], h, A, 'valid'),
                                                   max_rounds=r)[0]) for r in range(4)]
    print(E)
    assert all(later <= earlier * (1 + 1e-12) for earlier, later in zip(E, E[1:])) and E[2] < 1e-3 * E[0]


def test_a_hop_onto_an_existing_row_is_not_made():
    sc = scene()
    W, A, D = sc['W'], sc['A'], sc['D']
    V = eref.render(W, D, 1, 'valid', np.array([0]), np.array([0]), np.array([[13, 13]]), np.array([2.]))
    nmf = holding(W, V, 'valid')
    pair = as_det([0, 0], [0, 0], [[13, 13], [13, 14]], [1., 1.], A, 'valid')   # the second wants the place of the first
    a, b = nmf.detection_landscape(pair)
    sample, plane, shift, strength = nmf._events_of(pair, True)
    g = landscape_gains(a, b).reshape(2, 9)
    assert np.argmax(g[1]) == 3                                                  # delta (0, -1): onto row 0
    got, _ = nmf.relocate_detections(pair, n_iterations=0)
    assert np.array_equal(got.shift, pair.shift) and np.array_equal(got.strength, pair.strength)
    assert nmf.relocation_history_[0, 0] >= 1 and nmf.relocation_history_[0, 1] == 0 and len(nmf.relocation_history_) == 1
    # alone, the same row hops
    alone, _ = nmf.relocate_detections(rows_of(pair, [1]), n_iterations=0)
    assert alone.shift.tolist() == [[13, 13]] and alone.strength[0] == pytest.approx(2. - 0., rel=1e-12)
    # relocation_hops: ties go to the row of the lower index and to the neighbour of the lower index
    a = np.zeros((2, 9))
    b = np.ones((2, 9))
    a[:, [1, 7]] = 1.
    hops = relocation_hops(np.array([0, 0]), np.array([0, 0]), np.array([[13, 13], [13, 14]]), np.zeros(2), a, b, A, D,
                           (43, 43), 'valid', 0.)
    assert hops[0].tolist() == [0] and hops[1].tolist() == [[12, 13]] and hops[3] == 2 and hops[4] == 0.5


def test_a_row_with_nowhere_to_go_stays():
    """The choice of a round on landscapes the data does not support: every neighbour with a <= 0 or out of range gives
    g = 0 there, and a row whose own gain is negative would 'improve' by hopping onto nothing."""
    A, D, S = (3, 3), (12, 14), (14, 16)
    one = (np.array([0]), np.array([0]))
    a, b = np.full((1, 9), -0.3), np.ones((1, 9))
    a[0, 4] = 0.1                                                   # own gain 1 * (0.1 - 1) + 1 / 2 < 0
    hops = relocation_hops(*one, np.array([[5, 5]]), np.ones(1), a, b, A, D, S, 'valid', 0.)
    assert len(hops[0]) == 0 and hops[1].shape == (0, 2) and hops[3] == 0 and hops[4] == 0.
    a, b = np.zeros((1, 9)), np.zeros((1, 9))                       # a corner row whose in-range neighbours see nothing
    a[0, 4], b[0, 4] = -0.2, 1.
    hops = relocation_hops(*one, np.array([[0, 0]]), np.ones(1), a, b, A, D, S, 'valid', 0.)
    assert len(hops[0]) == 0 and hops[3] == 0
    a[0, 8], b[0, 8] = 0.5, 2.                                      # ... and with one neighbour that sees something
    hops = relocation_hops(*one, np.array([[0, 0]]), np.ones(1), a, b, A, D, S, 'valid', 0.)
    assert hops[0].tolist() == [0] and hops[1].tolist() == [[1, 1]] and hops[2].tolist() == [0.25] and hops[3] == 1


@pytest.mark.parametrize('mode', MODES)
def test_relocate_on_lists_the_data_does_not_support(mode):
    """Sparse noise and random rows, the corners of the shift shape among them: rows with a negative gain of their own and
    neighbours with a <= 0 everywhere.  The call returns a list -- distinct rows in range, strengths finite and >= 0 -- and
    the objective does not rise."""
    D, A = (12, 14), (3, 3)
    S = eref.shift_shape(D, A, mode)
    rng = np.random.default_rng(23)
    W = rng.random((2, 1) + A) + 0.1
    W /= W.sum(axis=(2, 3), keepdims=True)
    seen_negative = seen_stuck = 0
    for trial in range(4):
        V = rng.random((2, 1) + D) * (rng.random((2, 1) + D) < 0.15)
        nmf = holding(W, V, mode)
        rows = {(n, 0) + c for n in range(2) for c in itertools.product(*[(0, s - 1) for s in S])}
        while len(rows) < 25:
            rows.add((int(rng.integers(2)), int(rng.integers(2))) + tuple(int(rng.integers(s)) for s in S))
        rows = np.array(sorted(rows))
        det = as_det(rows[:, 0], rows[:, 1], rows[:, 2:], rng.random(len(rows)) + 0.5, A, mode)
        for kw in (dict(), dict(n_iterations=0), dict(n_iterations=2, max_rounds=3)):
            start = nmf.refit_detections(det, kw.get('n_iterations', 50))
            a, b = (x.reshape(len(det), 9) for x in nmf.detection_landscape(start))
            h = start.strength
            own = h * (a[:, 4] - h * b[:, 4]) + 0.5 * h * h * b[:, 4]
            g = landscape_gains(a, b)
            g[:, 4] = 0.
            seen_negative += int(np.sum(own < 0))
            seen_stuck += int(np.sum((own < 0) & (g.max(axis=1) == 0)))
            got, gains = nmf.relocate_detections(det, **kw)
            assert len(got) == len(det) and len(set(key(got))) == len(det)
            assert np.all(np.isfinite(got.strength)) and np.all(got.strength >= 0) and np.all(np.isfinite(gains))
            assert np.all(got.shift >= 0) and np.all(got.shift < np.array(S))
            assert np.array_equal(got.atom, det.atom) and np.array_equal(got.sample, det.sample)
            assert objective_of(nmf, got) <= objective_of(nmf, start) * (1 + 1e-12)
    print(f'{mode}: rows with a negative gain of their own {seen_negative}, of them with g = 0 all around {seen_stuck}')
    assert seen_negative > 0


# -- 5. refusals and validation -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model():
    nmf = fitted((2, 1, 9, 10), 2, (3, 4), 'reflect')
    return nmf, nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)), min_distance=0)


def calls(nmf, det):
    return (lambda: nmf.detection_landscape(det), lambda: nmf.refine_detections(det), lambda: nmf.relocate_detections(det))


def test_before_a_fit_they_raise_runtime_error(model):
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 4), backend=_Stub())
    for call in calls(nmf, model[1]):
        with pytest.raises(RuntimeError):
            call()


def test_they_are_frobenius_and_unweighted(model):
    nmf, det = model
    for name, value, back in (('_beta', 1., 2.), ('_weighted', True, False)):
        setattr(nmf, name, value)
        try:
            for call in calls(nmf, det):
                with pytest.raises(NotImplementedError, match='covers the plain Frobenius objective'):
                    call()
        finally:
            setattr(nmf, name, back)
    assert nmf.detection_landscape(det)[0].shape == (len(det), 3, 3)


def test_volumes_are_refused():
    nmf = fitted((1, 1, 5, 5, 5), 1, (2, 2, 2))
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)), min_distance=0)
    for call in calls(nmf, det):
        with pytest.raises(NotImplementedError):
            call()


@pytest.mark.parametrize('kw', [dict(min_improvement=float('nan')), dict(min_improvement=float('inf')),
                                dict(min_improvement=-1e-9), dict(min_improvement='0.1'), dict(min_improvement=True),
                                dict(min_improvement=None), dict(max_rounds=-1), dict(max_rounds=1.5),
                                dict(max_rounds=True), dict(n_iterations=-1), dict(sparsity_H=-1.)], ids=str)
def test_bad_relocate_arguments_raise_value_error(model, kw):
    nmf, det = model
    with pytest.raises(ValueError):
        nmf.relocate_detections(det, **kw)


def test_bad_rows_raise_value_error_and_duplicates_are_scored_but_not_moved(model):
    nmf, det = model
    bad = dataclasses.replace(det, strength=np.where(np.arange(len(det)) == 1, -1., det.strength))
    for call in calls(nmf, bad):
        with pytest.raises(ValueError):
            call()
    twice = rows_of(det, np.r_[np.arange(len(det)), 0])
    a, b = nmf.detection_landscape(twice)
    assert np.array_equal(a[-1], a[0]) and np.array_equal(b[-1], b[0])
    assert nmf.refine_detections(twice)[0].shape == (len(twice), 2)
    with pytest.raises(ValueError):
        nmf.relocate_detections(twice)


# -- 6. the ABI -----------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_typed():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tnmf_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    vp, ll, ci = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    assert re.search(r'\bint tnmf_hip_events_landscape\s*\(', header) and 'tnmf_hip_events_landscape' in _lib.EXPORTS
    fn = lib.tnmf_hip_events_landscape
    assert fn.restype is ci
    assert list(fn.argtypes) == [vp, ctypes.POINTER(_lib.Geom), ci, vp, vp, vp, ll, vp, vp, vp, vp, vp, vp]
    assert _lib.ABI_VERSION == 8
    g = _lib.make_geom(1, 1, 1, (4,), (2,), 0)   # an argument error is answered without a device: no context
    assert fn(None, ctypes.byref(g), 0, None, None, None, 0, None, None, None, None, None, None) == -1
    assert fn(ctypes.c_void_p(1), ctypes.byref(_lib.make_geom(1, 1, 1, (4, 4, 4), (2, 2, 2), 0)), 0, None, None, None, 0,
              None, None, None, None, None, None) == _lib.E_UNSUPPORTED
    assert fn(ctypes.c_void_p(1), ctypes.byref(g), 0, None, None, None, (2 ** 31 - 1) // 9 + 1, None, None, None, None,
              None, None) == _lib.E_UNSUPPORTED


def test_the_host_mirror_of_the_path_rule_has_the_kernels_limit():
    src = open(os.path.join(ROOT, 'tnmf_amd', 'csrc', 'landscape.hip')).read()
    rule = re.search(r'constexpr int kPatchMax = (\d+);', src)
    assert rule and int(rule.group(1)) == lref.PATCH_MAX
