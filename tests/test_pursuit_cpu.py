"""
Forward selection of events on CPU: the front end's ``pursue_detections`` over an oracle-backed backend without the pursuit
hooks (the host fallback ``pursuit_numpy`` under the shared driver), in float64, against tests/pursuit_reference.py.

Separated scenes have a known answer: the planted support, found in one round.  Noisy, overlapping scenes are checked by
invariants -- distinct rows, box-disjoint additions, and the energy bookkeeping 1/2 ||V||^2 - sum of the gains = E(list), which
a pair added in overlap breaks by the size of a gain -- and against the reference's rounds.
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
import pursuit_reference as pur
from conftest import ROOT
from test_events_cpu import MODES, _Stub
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import (Detections, TransformInvariantNMF, event_boxes, event_images,
                                            events_norms_numpy)

SEEDS = (0, 1, 2, 3)
NOISY_SEEDS = (0, 1, 2)
NOISY_MIN_GAIN = 0.02


def model_of(W, V, mode, dtype=np.float64, backend=None, **kw):
    """A model that holds the dictionary W and is bound to V, as ``fit_batch(V, n_iterations=0, keep_W=True)`` leaves it."""
    nmf = TransformInvariantNMF(n_atoms=W.shape[0], atom_shape=W.shape[2:],
                                backend=_Stub(mode) if backend is None else backend, **kw)
    nmf._W = np.array(W, dtype=dtype)
    np.random.seed(42)
    nmf.fit_batch(np.array(V, dtype=dtype), n_iterations=0, keep_W=True)
    assert np.array_equal(nmf.W, W.astype(dtype))
    return nmf


def key(det):
    return sorted(map(tuple, np.column_stack([det.sample, det.atom, det.transform, det.shift]).tolist()))


def rows_of(det, keep):
    return Detections(**{f.name: getattr(det, f.name)[keep] for f in dataclasses.fields(Detections)})


@functools.lru_cache(maxsize=None)
def separated(seed, mode):
    case = pur.separated(seed, mode)
    return case, pur.Table(case['W'], case['V'].shape[2:], mode)


@functools.lru_cache(maxsize=None)
def noisy(seed, mode):
    case = gref.planted(seed, mode, n_spurious=0)
    return case, pur.Table(case['W'], case['V'].shape[2:], mode)


# -- 1. separated scenes: the planted support in one round ---------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('seed', SEEDS)
def test_separated_scenes_are_recovered_exactly(seed, mode):
    case, table = separated(seed, mode)
    V, W, rows, h = case['V'], case['W'], case['rows'], case['strength']
    A, D = W.shape[2:], V.shape[2:]
    # the scene is well posed, on the reference alone: in each true event's window the runner-up stays clear of the event
    b = table.norms()
    g = pur.gain_map(table.correlate(V), b)
    own = np.array([g[tuple(r)] for r in rows])
    worst = 0.
    for r, x in zip(rows, own):
        window = g[(r[0], slice(None)) + tuple(slice(max(0, u - (a - 1)), u + a) for u, a in zip(r[2:], A))].copy()
        assert window.max() == x
        window[(r[1],) + tuple(min(u, a - 1) for u, a in zip(r[2:], A))] = 0.
        worst = max(worst, window.max() / x)
    print(f'{mode} seed {seed}: runner-up / own gain <= {worst:.3f}, smallest true gain {own.min():.3g}')
    assert worst <= 0.95 and own.min() >= 1e-3
    ref = pur.pursue(V, W, mode, 1e-6, table=table)
    assert sorted(map(tuple, ref['rows'].tolist())) == sorted(map(tuple, rows.tolist()))
    by_row = {tuple(r): x for r, x in zip(ref['rows'].tolist(), ref['strength'])}
    # V is the render rounded to float32: every pixel under a true event moves by at most 2^-24 of h * phi there (the true
    # footprints are disjoint), so a moves by at most 2^-24 * h * b and the strength a / b by 2^-24 * h
    assert max(abs(by_row[tuple(r)] - x) for r, x in zip(rows.tolist(), h)) <= 2. ** -24 * h.max()

    nmf = model_of(W, V, mode)
    det, gains = nmf.pursue_detections(min_gain=1e-6, refit_iterations=0)
    assert isinstance(det, Detections) and gains.dtype == np.float64 and gains.shape == (len(det),)
    assert key(det) == sorted((n, p, 0) + tuple(u) for n, p, *u in rows.tolist())
    assert nmf.pursuit_history_.shape == (2, 3) and nmf.pursuit_history_[:, 1].tolist() == [10, 0]
    np.testing.assert_array_equal(nmf.pursuit_history_[:, :2], ref['history'][:, :2])
    np.testing.assert_allclose(nmf.pursuit_history_[:, 2], ref['history'][:, 2], rtol=1e-10, atol=0)   # (two float64 sums)
    planted = {(n, p) + tuple(u): x for (n, p, *u), x in zip(rows.tolist(), h)}
    got = np.array([planted[(n, p) + tuple(u)] for n, p, u in zip(det.sample, det.atom, det.shift.tolist())])
    print(f'    strengths off the planted ones by {np.abs(det.strength - got).max():.3g}')
    assert np.abs(det.strength - got).max() <= 1e-6
    offset = np.array([a - 1 if mode == 'valid' else 0 for a in A])
    np.testing.assert_array_equal(det.origin, det.shift - offset)


def test_the_separated_scenes_hold_wrapped_and_mirrored_events():
    """Events of 2 and of 4 images in 'reflect', of 2 images in 'circular' -- there an event that wraps on both axes has the whole
    sample for its box, so no scene with a second event in that sample is separated."""
    for mode, want in (('circular', {1, 2}), ('reflect', {1, 2, 4})):
        for seed in SEEDS:
            case, table = separated(seed, mode)
            event, _ = event_images(case['rows'][:, 2:], case['W'].shape[2:], table.S, mode)
            assert set(np.bincount(event).tolist()) >= want, (mode, seed)


def wrapped_scene():
    """One event per sample that wraps on BOTH axes in 'circular' (4 images, the whole sample for its box): alone in its sample
    it is separated from everything, so the answer is known.  -> (V, W, rows, strength)."""
    case, _ = separated(2, 'circular')
    W, D = case['W'], case['V'].shape[2:]
    rows = np.array([[0, 1, D[0] - 1, D[1] - 2], [1, 0, D[0] - 3, D[1] - 1]], dtype=np.int64)
    h = np.array([1.25, 1.75])
    V = eref.render(W, D, 2, 'circular', rows[:, 0], rows[:, 1], rows[:, 2:], h).astype(np.float32).astype(np.float64)
    return V, W, rows, h


def test_a_circular_event_wrapped_on_both_axes_is_recovered():
    V, W, rows, h = wrapped_scene()
    event, _ = event_images(rows[:, 2:], W.shape[2:], V.shape[2:], 'circular')
    assert np.bincount(event).tolist() == [4, 4]
    nmf = model_of(W, V, 'circular')
    det, gains = nmf.pursue_detections(1e-6, refit_iterations=0, n_iterations=0)
    assert key(det) == sorted((n, p, 0) + tuple(u) for n, p, *u in rows.tolist())
    assert nmf.pursuit_history_[:, 1].tolist() == [2, 0]
    assert np.abs(det.strength[np.argsort(det.sample)] - h).max() <= 2. ** -24 * h.max()   # (as above)
    booked = 0.5 * float(np.sum(V * V)) - float(nmf.pursuit_history_[:, 2].sum())
    assert abs(booked - pur.energy(V, W, 'circular', rows, det.strength[np.argsort(det.sample)])) <= 1e-12


@pytest.mark.parametrize('mode', MODES)
def test_norms_of_the_host_fallback(mode):
    case, table = separated(0, mode)
    want = table.norms()
    got = events_norms_numpy(case['W'], case['V'].shape[2:], mode)
    assert got.shape == want.shape and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    W = case['W'][:, :, :, :3]        # 'valid', the first corner: one pixel of the atom shows
    got = events_norms_numpy(W, (4, 7), 'valid')
    assert got[0, 0, 0] == float(np.sum(W[0, :, 3, 2] ** 2)) and np.all(got > 0)


# -- 2. noisy, overlapping scenes: invariants -------------------------------------------------------------------------------------
def boxes_disjoint(rows, A, D, S, mode):
    lo, hi = event_boxes(rows[:, 2:], A, D, S, mode)
    return all(rows[i, 0] != rows[j, 0] or not pur.meet(lo, hi, i, j) for i in range(len(rows)) for j in range(i))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('seed', NOISY_SEEDS)
def test_noisy_scenes_keep_the_energy_bookkeeping(seed, mode):
    case, table = noisy(seed, mode)
    V, W = case['V'], case['W']
    A, D = W.shape[2:], V.shape[2:]
    nmf = model_of(W, V, mode)
    det, gains = nmf.pursue_detections(NOISY_MIN_GAIN, refit_iterations=0, n_iterations=0)
    hist = nmf.pursuit_history_
    rows = np.column_stack([det.sample, det.atom, det.shift])
    assert len(np.unique(rows, axis=0)) == len(rows) > 0 and np.all(det.transform == 0)
    assert int(hist[:, 1].sum()) == len(rows) and hist[-1, 1] == 0 and np.all(hist[:-1, 1] > 0)
    first = 0
    for count in hist[:, 1].astype(int):      # the rows are appended round by round
        assert boxes_disjoint(rows[first:first + count], A, D, table.S, mode)
        first += count
    E = pur.energy(V, W, mode, rows, det.strength)
    booked = 0.5 * float(np.sum(V * V)) - float(hist[:, 2].sum())
    print(f'{mode} seed {seed}: {len(hist)} rounds, candidates {hist[:, 0].astype(int).tolist()}, added '
          f'{hist[:, 1].astype(int).tolist()}, |booked - E| = {abs(booked - E):.3g} of {E:.3g}')
    assert abs(booked - E) <= NOISY_MIN_GAIN / 100
    # the same rounds as the reference's
    ref = pur.pursue(V, W, mode, NOISY_MIN_GAIN, table=table)
    np.testing.assert_array_equal(hist[:, :2], ref['history'][:, :2])
    np.testing.assert_allclose(hist[:, 2], ref['history'][:, 2], rtol=1e-10, atol=1e-12)
    assert sorted(map(tuple, rows.tolist())) == sorted(map(tuple, ref['rows'].tolist()))
    np.testing.assert_allclose(gains, nmf.detection_gains(det), rtol=1e-12)


def test_the_host_filter_drops_candidates_in_circular():
    """Peaks >= A apart whose wrapped occurrences still meet: in some round of some noisy 'circular' scene fewer rows are added
    than candidates found although every candidate's exact gain is its map value (float64) and above the threshold."""
    dropped = 0
    for seed in NOISY_SEEDS:
        case, table = noisy(seed, 'circular')
        ref = pur.pursue(case['V'], case['W'], 'circular', NOISY_MIN_GAIN, table=table)
        dropped += int(np.sum(ref['history'][:, 0] - ref['history'][:, 1] > 0))
    assert dropped > 0


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('seed', NOISY_SEEDS)
def test_with_the_default_refits_the_objective_never_rises(seed, mode):
    case, table = noisy(seed, mode)
    V, W = case['V'], case['W']
    nmf = model_of(W, V, mode)
    energies = [0.5 * float(np.sum(V * V))]
    for r in range(1, 12):
        det, _ = nmf.pursue_detections(NOISY_MIN_GAIN, max_rounds=r, n_iterations=0)
        rows = np.column_stack([det.sample, det.atom, det.shift])
        energies.append(pur.energy(V, W, mode, rows, det.strength))
        if len(nmf.pursuit_history_) < r or nmf.pursuit_history_[-1, 1] == 0:
            break
    print(f'{mode} seed {seed}: objective per round {np.round(energies, 5).tolist()}')
    assert len(energies) >= 3 and np.all(np.diff(energies) <= 1e-12 * energies[0])
    det, gains = nmf.pursue_detections(NOISY_MIN_GAIN)          # ... and the final refit lowers it once more
    rows = np.column_stack([det.sample, det.atom, det.shift])
    assert pur.energy(V, W, mode, rows, det.strength) <= energies[-1] * (1 + 1e-12)
    assert gains.shape == (len(det),)


# -- 3. start, max_events, transforms, shuffles ----------------------------------------------------------------------------------
def test_start_continues_a_list_and_max_events_cuts_by_gain():
    case, table = separated(1, 'reflect')
    V, W, rows = case['V'], case['W'], case['rows']
    nmf = model_of(W, V, 'reflect')
    everything, gains = nmf.pursue_detections(1e-6, refit_iterations=0, n_iterations=0)
    order = np.argsort(-gains, kind='stable')
    top, _ = nmf.pursue_detections(1e-6, max_events=4, refit_iterations=0, n_iterations=0)
    assert key(top) == key(rows_of(everything, order[:4])) and nmf.pursuit_history_[:, 1].tolist() == [4]
    rest, _ = nmf.pursue_detections(1e-6, refit_iterations=0, n_iterations=0, start=top)
    assert key(rest) == key(everything) and nmf.pursuit_history_[:, 1].tolist() == [6, 0]
    for name in ('sample', 'atom', 'transform', 'shift'):                      # the start rows come first, in their order
        np.testing.assert_array_equal(getattr(rest, name)[:4], getattr(top, name))
    full, _ = nmf.pursue_detections(1e-6, max_events=4, start=top)             # already full: no round
    assert key(full) == key(top) and nmf.pursuit_history_.shape == (0, 3)
    none, g = nmf.pursue_detections(1e-6, max_rounds=0)
    assert len(none) == 0 and g.shape == (0,) and nmf.pursuit_history_.shape == (0, 3)
    none, _ = nmf.pursue_detections(1e3)                                       # nothing explains that much: one empty round
    assert len(none) == 0 and nmf.pursuit_history_.tolist() == [[0., 0., 0.]]


def test_a_transforms_model_recovers_the_orientation():
    rng = np.random.default_rng(5)
    W = rng.random((2, 1, 4, 4)) + 0.05
    W /= W.sum(axis=(2, 3), keepdims=True)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(4, 4), backend=_Stub('valid'), transforms='rot90')
    nmf._W = W.copy()
    np.random.seed(42)
    nmf.fit_batch(np.zeros((1, 1, 20, 22)) + 1e-3, n_iterations=0, keep_W=True)
    planted = Detections(sample=np.array([0, 0]), atom=np.array([1, 0]), transform=np.array([3, 1]),
                         shift=np.array([[5, 6], [14, 15]]), origin=np.array([[2, 3], [11, 12]]),
                         strength=np.array([2., 1.5]))
    V = nmf.reconstruct_detections(planted)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(4, 4), backend=_Stub('valid'), transforms='rot90')
    nmf._W = W.copy()
    np.random.seed(42)
    nmf.fit_batch(V, n_iterations=0, keep_W=True)
    det, gains = nmf.pursue_detections(1e-6, refit_iterations=0, n_iterations=0)
    assert key(det) == key(planted) and set(det.transform.tolist()) == {1, 3}
    np.testing.assert_allclose(np.sort(det.strength), [1.5, 2.], rtol=1e-12)
    assert np.all(gains > 0.01)


def test_under_a_shuffle_and_on_the_block_of_a_rank():
    case, _ = separated(0, 'valid')
    V, W, rows = case['V'], case['W'], case['rows']
    V3 = np.concatenate([V, V[:1]])
    nmf = model_of(W, V3, 'valid')
    nmf._shuffle_idx = np.array([2, 0, 1])     # the H property shows internal sample argsort(shuffle)[i] at place i
    nmf._backend._V_local = nmf._V = V3[nmf._shuffle_idx]
    det, _ = nmf.pursue_detections(1e-6, refit_iterations=0)
    shown = nmf.V
    np.testing.assert_allclose(nmf.reconstruct_detections(det), nmf._V, atol=1e-6)
    for n in range(3):
        mine = rows_of(det, det.sample == n)
        want = rows[rows[:, 0] == int(np.flatnonzero([np.array_equal(shown[n], v) for v in V])[0])]
        assert sorted(map(tuple, np.column_stack([mine.atom, mine.shift]).tolist())) == sorted(map(tuple, want[:, 1:].tolist()))
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(4, 4), backend=_Stub('valid', shard=(1, 3)))
    nmf._W = np.array(W)
    np.random.seed(42)
    nmf.fit_batch(np.array(V3), n_iterations=0, keep_W=True)
    det, _ = nmf.pursue_detections(1e-6, refit_iterations=0)
    assert set(det.sample.tolist()) == {1, 2} and len(det) == 10


# -- 4. refusals ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model():
    case, _ = separated(0, 'reflect')
    return model_of(case['W'], case['V'], 'reflect')


@pytest.mark.parametrize('kw', [dict(min_gain=0.), dict(min_gain=-1.), dict(min_gain=float('nan')),
                                dict(min_gain=float('inf')), dict(min_gain='0.1'), dict(min_gain=True), dict(min_gain=None),
                                dict(min_gain=0.1, max_events=-1), dict(min_gain=0.1, max_events=1.5),
                                dict(min_gain=0.1, max_events=True), dict(min_gain=0.1, max_rounds=-1),
                                dict(min_gain=0.1, max_rounds=1.5), dict(min_gain=0.1, max_rounds=True),
                                dict(min_gain=0.1, max_rounds=None), dict(min_gain=0.1, refit_iterations=-1),
                                dict(min_gain=0.1, refit_iterations=2.), dict(min_gain=0.1, refit_iterations=False),
                                dict(min_gain=0.1, n_iterations=-1), dict(min_gain=0.1, sparsity_H=-1.)], ids=str)
def test_bad_arguments_raise_value_error(model, kw):
    with pytest.raises(ValueError):
        model.pursue_detections(**kw)


def test_a_start_with_bad_or_duplicate_rows_raises_value_error(model):
    det, _ = model.pursue_detections(1e-6, max_events=3)
    with pytest.raises(ValueError):
        model.pursue_detections(1e-6, start=rows_of(det, [0, 1, 0]))
    with pytest.raises(ValueError):
        model.pursue_detections(1e-6, start=dataclasses.replace(det, sample=det.sample + 7))


def test_before_a_fit_it_raises_runtime_error():
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 4), backend=_Stub())
    with pytest.raises(RuntimeError):
        nmf.pursue_detections(0.1)


def test_it_is_frobenius_and_unweighted(model):
    for name, value, back in (('_beta', 1., 2.), ('_weighted', True, False)):
        setattr(model, name, value)
        try:
            with pytest.raises(NotImplementedError, match='plain Frobenius'):
                model.pursue_detections(0.1)
        finally:
            setattr(model, name, back)
    assert len(model.pursue_detections(1e-6)[0]) == 10


def test_volumes_are_refused():
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=1, atom_shape=(2, 2, 2), backend=_Stub())
    nmf.fit(np.random.default_rng(0).random((1, 1, 5, 5, 5)), n_iterations=1)
    with pytest.raises(NotImplementedError, match='volumes'):
        nmf.pursue_detections(0.1)


# -- 5. the ABI -------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_typed():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tnmf_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    vp, ll, ci, gp = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(_lib.Geom)
    want = {'tnmf_hip_events_norms': [vp, gp, ci, vp, vp, vp],
            'tnmf_hip_pursuit_score': [vp, gp, vp, vp, vp, vp, ll, vp],
            'tnmf_hip_pursuit_pick': [vp, gp, ci, vp, vp, ll, vp, vp, vp, vp, vp, vp, vp]}
    for name, argtypes in want.items():
        assert re.search(r'\bint %s\s*\(' % name, header) and name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is ci and list(fn.argtypes) == argtypes
    assert _lib.ABI_VERSION == 8
    g = _lib.make_geom(1, 1, 1, (4,), (2,), 0)   # an argument error is answered without a device: no context
    assert lib.tnmf_hip_events_norms(None, ctypes.byref(g), 0, None, None, None) == -1
    assert lib.tnmf_hip_pursuit_score(None, ctypes.byref(g), None, None, None, None, 0, None) == -1
    assert lib.tnmf_hip_pursuit_pick(None, ctypes.byref(g), 0, None, None, 0, None, None, None, None, None, None, None) == -1
