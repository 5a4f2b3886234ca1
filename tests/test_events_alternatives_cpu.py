"""
The alternatives of events on CPU: the host route ``events_alternatives_numpy``, the round's choice ``relabel_hops`` and the
front end's ``detection_alternatives`` / ``relabel_detections`` over an oracle-backed backend without the events hooks, in
float64, against tests/alternatives_reference.py -- g = a^2 / (2 b) read literally as a difference of two energies of actual
renders.

The bar of the brute force: 1e-10 of 1/2 ||V||^2.  Every energy is a float64 sum over a few hundred pixels of terms below
||V||^2, rounded to ~1e-14 of it, and the difference of two of them carries no more: four orders below the bar.
"""
import ctypes
import dataclasses
import functools
import os
import re

import numpy as np
import pytest

import alternatives_reference as aref
import events_gain_reference as gref
import events_reference as eref
import landscape_reference as lref
from conftest import ROOT
from test_events_cpu import MODES, _Stub, fitted
from test_events_landscape_cpu import GEOMETRIES, as_det, key, objective_of, rows_of
from tnmf_amd import _lib
from tnmf_amd import transforms as tr
from tnmf_amd.events_host import (alternative_planes, events_alternatives_numpy, events_gain_numpy, landscape_gains,
                                  relabel_hops)
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF

BAR = 1e-10
# geometry -> (atoms, transform group): 'rot90' and 'dihedral' need square atoms; a 3-atom model without transforms
MODELS = {'1d': (3, None), '3x3-c1': (2, 'rot90'), '3x3-c3': (3, 'dihedral'), '5x7-c1': (3, None), '5x7-c3': (2, 'mirrors')}
OVERS = ('transforms', 'atoms', 'all')


def holding(W, V, mode, transforms=None):
    """A float64 model over the oracle backend that holds the dictionary W[M, C, *A] and the samples V."""
    nmf = TransformInvariantNMF(n_atoms=W.shape[0], atom_shape=W.shape[2:], backend=_Stub(mode), transforms=transforms)
    nmf._W = np.array(W)
    np.random.seed(42)
    nmf.fit(np.array(V), n_iterations=0, keep_W=True, update_W=False)
    assert np.array_equal(nmf.W, W)
    return nmf


def effective(W, transforms):
    return W if transforms is None else tr.expand(W, transforms)


def sets_of(M, T):
    """over -> (n_alt, stride), with plane = atom * T + transform."""
    return {'transforms': (T, 1), 'atoms': (M, T), 'all': (M * T, 1)}


@functools.lru_cache(maxsize=None)
def problem(name, mode):
    """-> (V, W, transforms, sample, plane, shift, h, names): every place of landscape_reference.places() on sample 1 under
    planes that run through the whole effective dictionary, two of them twice and one with strength 0, and a few rows of
    sample 0."""
    D, A, C = GEOMETRIES[name]
    M, transforms = MODELS[name]
    T = 1 if transforms is None else tr.size(transforms)
    P = M * T
    rng = np.random.default_rng(29)
    W, V = rng.random((M, C) + A) + 0.1, rng.random((2, C) + D) * 2.
    at = lref.places(D, A, mode)
    names = list(at) + ['interior', 'corner0']                  # duplicates
    shift = np.array([at[n] for n in names], dtype=np.int64)
    sample = np.ones(len(names), dtype=np.int64)
    plane = ((5 * np.arange(len(names)) + 1) % P).astype(np.int64)
    plane[-2:] = plane[[names.index('interior'), names.index('corner0')]]
    h = rng.random(len(names)) + 0.5
    h[-2:] = h[[names.index('interior'), names.index('corner0')]]
    h[names.index('far')] = 0.
    S = eref.shift_shape(D, A, mode)
    extra = np.column_stack([rng.integers(s, size=3) for s in S])
    sample, plane = np.concatenate([sample, [0, 0, 0]]), np.concatenate([plane, [0, P - 1, P // 2]])
    shift, h = np.concatenate([shift, extra]), np.concatenate([h, [1., 0.5, 2.]])
    return V, W, transforms, sample, plane, shift, h, names + ['extra'] * 3


# -- 1. g is the difference of the energies -------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(GEOMETRIES))
def test_brute_force(name, mode):
    V, W, transforms, sample, plane, shift, h, names = problem(name, mode)
    D, A, C = GEOMETRIES[name]
    M, T = W.shape[0], 1 if transforms is None else tr.size(transforms)
    W_eff = effective(W, transforms)
    nmf = holding(W, V, mode, transforms)
    det = as_det(sample, plane, shift, h, A, mode, T)
    R = eref.render(W_eff, D, 2, mode, sample, plane, shift, h)
    scale = 0.5 * float(np.sum(V * V))
    n_images = np.bincount(np.concatenate([[e] * len(eref.images(u, A, eref.shift_shape(D, A, mode), mode))
                                           for e, u in enumerate(shift)]).astype(np.int64), minlength=len(h))
    if mode in ('circular', 'reflect'):
        assert set(n_images.tolist()) == ({1, 2} if len(D) == 1 else {1, 2, 4})
    for over in OVERS:
        if over == 'transforms' and transforms is None:
            with pytest.raises(ValueError, match="over='transforms' needs a model with transforms"):
                nmf.detection_alternatives(det, over)
            continue
        n_alt, stride = sets_of(M, T)[over]
        a, b = nmf.detection_alternatives(det, over)
        assert a.shape == b.shape == ((len(h), M, T) if over == 'all' else (len(h), n_alt))
        assert a.dtype == b.dtype == np.float64
        a, b = a.reshape(len(h), -1), b.reshape(len(h), -1)
        host = events_alternatives_numpy(W_eff, D, 2, mode, sample, plane, shift, h, V, n_alt, stride, with_magnitude=True)
        assert np.array_equal(host[0], a) and np.array_equal(host[1], b)
        ra, rb, rmag = aref.alternatives(V, R, W_eff, mode, sample, plane, shift, h, n_alt, stride)
        want = aref.brute_force(V, W_eff, mode, sample, plane, shift, h, ra, rb, n_alt, stride)
        g = landscape_gains(a, b)
        print(f'{name} {mode} {over}: {len(h)} rows x {n_alt}; |g - brute force| <= {np.abs(g - want).max():.3g}, reference '
              f'{np.abs(aref.gains(ra, rb) - want).max():.3g}, bar {BAR * scale:.3g}; g up to {g.max():.3g}')
        assert np.all(np.abs(g - want) <= BAR * scale) and np.all(np.abs(aref.gains(ra, rb) - want) <= BAR * scale)
        assert np.all(np.abs(a - ra) <= 1e-12 * rmag) and np.all(np.abs(b - rb) <= 1e-12 * rb)
        assert np.all(np.abs(host[2] - rmag) <= 1e-12 * rmag)
        assert g.max() > 1e-3 * scale and np.all(b > 0)
        # the candidates: the row's own plane among them, once, where the index rule says
        planes, own = alternative_planes(plane, n_alt, stride)
        for e in range(len(h)):
            want_planes, want_own = aref.candidates(int(plane[e]), n_alt, stride)
            assert planes[e].tolist() == want_planes and own[e] == want_own
        # duplicates put back only themselves: the same numbers twice; a zero strength is a row like any other
        for twin, first in ((-5, names.index('interior')), (-4, names.index('corner0'))):
            assert np.array_equal(a[twin], a[first]) and np.array_equal(b[twin], b[first])
        assert h[names.index('far')] == 0. and a[names.index('far')].any()
    # both paths of the kernel have rows here ('full' has no clipped, wrapped or mirrored row: its walk is the patch limit's)
    st = aref.staged((2, C, M * T, D, A, mode), shift)
    assert (mode == 'full') == bool(st.all()) and st[names.index('edge')]
    # (5 x 7 in 'reflect' on 12 x 14: the mirror zone takes the interior, the GPU test adds a shift beyond it)
    assert st[names.index('interior')] or (name.startswith('5x7') and mode == 'reflect')


# -- 2. the identities at the row's own plane -------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['1d', '3x3-c3', '5x7-c3'])
def test_identities_with_the_gains_and_the_landscape(name, mode):
    V, W, transforms, sample, plane, shift, h, _ = problem(name, mode)
    D, A, C = GEOMETRIES[name]
    M, T = W.shape[0], 1 if transforms is None else tr.size(transforms)
    nmf = holding(W, V, mode, transforms)
    det = as_det(sample, plane, shift, h, A, mode, T)
    W_eff = effective(W, transforms)
    R = eref.render(W_eff, D, 2, mode, sample, plane, shift, h)
    gain, mag = gref.closed_form(V, R, W_eff, mode, sample, plane, shift, h)
    want = nmf.detection_gains(det)
    assert np.array_equal(want, events_gain_numpy(W_eff, D, 2, mode, sample, plane, shift, h, V))
    la, lb = (x.reshape(len(h), -1) for x in nmf.detection_landscape(det))
    centre = (la.shape[1] - 1) // 2
    every = np.arange(len(h))
    for over, (n_alt, stride) in sets_of(M, T).items():
        if over == 'transforms' and transforms is None:
            continue
        a, b = (x.reshape(len(h), -1) for x in nmf.detection_alternatives(det, over))
        own = alternative_planes(plane, n_alt, stride)[1]
        a0, b0 = a[every, own], b[every, own]
        a_e = a0 - h * b0
        scale = mag + h * h * b0 + 1e-300
        assert np.all(np.abs(h * a_e + 0.5 * h * h * b0 - want) <= 1e-12 * scale)
        assert np.all(np.abs(h * a_e + 0.5 * h * h * b0 - gain) <= 1e-12 * scale)
        # column j_own is the centre of the landscape: the same occurrence against the same residual
        assert np.array_equal(a0, la[:, centre]) and np.array_equal(b0, lb[:, centre])


# -- 3. the planted scene ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted(seed, mode):
    """N = 2, D = 40 x 44, one channel, 2 random atoms 5 x 5 under 'rot90': 20 rows at random shifts, no two rows of a sample
    within one pixel of each other on both axes, strengths in [0.5, 1.5); and the same rows, every one in a wrong orientation."""
    rng = np.random.default_rng(seed)
    D, A, N, M, T = (40, 44), (5, 5), 2, 2, 4
    W = rng.random((M, 1) + A)
    S = eref.shift_shape(D, A, mode)
    rows = []
    while len(rows) < 20:
        n, u = int(rng.integers(N)), tuple(int(rng.integers(s)) for s in S)
        if any(r[0] == n and abs(r[3] - u[0]) <= 1 and abs(r[4] - u[1]) <= 1 for r in rows):
            continue
        rows.append((n, int(rng.integers(M)), int(rng.integers(T))) + u)
    rows = np.array(rows, dtype=np.int64)
    h = 0.5 + rng.random(len(rows))
    wrong = rows.copy()
    wrong[:, 2] = (rows[:, 2] + rng.integers(1, T, len(rows))) % T
    W_eff = tr.expand(W, 'rot90')
    V = eref.render(W_eff, D, N, mode, rows[:, 0], rows[:, 1] * T + rows[:, 2], rows[:, 3:], h)
    whole = aref.staged((N, 1, M * T, D, A, mode), rows[:, 3:])      # one image, wholly inside the sample
    for x in (W, V, rows, wrong, h, whole):
        x.setflags(write=False)
    return dict(W=W, V=V, D=D, A=A, mode=mode, rows=rows, wrong=wrong, h=h, whole=whole, T=T)


def planted_det(sc, rows, h=None):
    return as_det(rows[:, 0], rows[:, 1] * sc['T'] + rows[:, 2], rows[:, 3:], sc['h'] if h is None else h, sc['A'],
                  sc['mode'], sc['T'])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('seed', [1, 2, 3])
def test_relabel_recovers_the_planted_orientations(seed, mode):
    """Every row of a noiseless scene starts in a wrong orientation.  In the three modes other than 'full' all 20 come back;
    in 'full' the orientation of every row whose occurrence lies wholly inside the sample is asserted; the objective ends
    below 1e-8 of 1/2 ||V||^2 in every mode."""
    sc = planted(seed, mode)
    nmf = holding(sc['W'], sc['V'], mode, 'rot90')
    start, true = planted_det(sc, sc['wrong']), planted_det(sc, sc['rows'])
    got, gains = nmf.relabel_detections(start, strengths='solve')
    assert isinstance(got, Detections) and gains.dtype == np.float64 and gains.shape == (20,)
    scale = 0.5 * float(np.sum(sc['V'] ** 2))
    E = objective_of(nmf, got)
    hist = nmf.relabel_history_
    right = got.transform == true.transform
    print(f'seed {seed} {mode}: {int(right.sum())} of 20 orientations ({int(sc["whole"].sum())} rows wholly inside), objective '
          f'{E / scale:.3g} of 1/2 ||V||^2, history {hist.tolist()}')
    assert E < 1e-8 * scale
    assert np.all(right[sc['whole']]) and (mode == 'full' or np.all(right))
    for name in ('sample', 'atom', 'shift', 'origin'):                   # row by row: the order is kept, the shifts stay
        np.testing.assert_array_equal(getattr(got, name), getattr(true, name))
    if np.all(right):
        np.testing.assert_allclose(got.strength, sc['h'], rtol=1e-6)
    assert hist.ndim == 2 and hist.shape[1] == 3 and hist[-1, 1] == 0 and np.all(hist[:-1, 1] > 0)
    assert len(set(key(got))) == 20


# -- 4. the rules of a round --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cells(seed=3, mode='valid'):
    """A noiseless scene whose footprints keep to cells of 10 x 10 pixels: per sample 10 of the 16 cells hold one occurrence
    of a 4 x 4 atom under 'rot90', and the same rows in wrong orientations."""
    rng = np.random.default_rng(seed)
    D, A, N, M, T = (40, 40), (4, 4), 2, 2, 4
    W = (rng.random((M, 1) + A) + 0.1).astype(np.float32).astype(np.float64)     # (both element types hold it)
    first = np.array([a - 1 if mode == 'valid' else 0 for a in A])
    rows = []
    for n in range(N):
        for cell in rng.permutation(16)[:10]:
            origin = np.array([cell // 4, cell % 4]) * 10 + rng.integers(2, 4, 2)
            rows.append((n, int(rng.integers(M)), int(rng.integers(T))) + tuple(int(x) for x in origin + first))
    rows = np.array(rows, dtype=np.int64)[rng.permutation(len(rows))]
    h = 1. + rng.integers(0, 9, len(rows)) / 8.
    V = eref.render(tr.expand(W, 'rot90'), D, N, mode, rows[:, 0], rows[:, 1] * T + rows[:, 2], rows[:, 3:], h)
    V = V.astype(np.float32).astype(np.float64)
    wrong = rows.copy()
    wrong[:, 2] = (rows[:, 2] + rng.integers(1, T, len(rows))) % T
    for x in (W, V, rows, wrong, h):
        x.setflags(write=False)
    return dict(W=W, V=V, D=D, A=A, mode=mode, rows=rows, wrong=wrong, h=h, T=T)


def test_hops_with_disjoint_boxes_lower_the_objective_by_the_sum_of_their_improvements():
    sc = cells()
    nmf = holding(sc['W'], sc['V'], sc['mode'], 'rot90')
    start = nmf.refit_detections(planted_det(sc, sc['wrong']), 50)
    a, b = nmf.detection_alternatives(start)
    sample, plane, shift, strength = nmf._events_of(start, True)
    S = eref.shift_shape(sc['D'], sc['A'], sc['mode'])
    hopped, target, h, n_candidates, total = relabel_hops(sample, plane, shift, strength, a, b, 4, 1, sc['A'], sc['D'], S,
                                                          sc['mode'], 0.)
    assert n_candidates == 20 and hopped.tolist() == list(range(20)) and total > 0
    assert np.array_equal(target, sc['rows'][:, 1] * 4 + sc['rows'][:, 2])
    after = dataclasses.replace(start, atom=target // 4, transform=target % 4, strength=h)
    before, scale = objective_of(nmf, start), 0.5 * float(np.sum(sc['V'] ** 2))
    print(f'objective {before:.6g} -> {objective_of(nmf, after):.3g}, the improvements sum to {total:.6g}')
    assert abs(before - objective_of(nmf, after) - total) <= BAR * scale
    # ... and so says the driver, whose history holds the same round
    got, gains = nmf.relabel_detections(planted_det(sc, sc['wrong']))
    hist = nmf.relabel_history_
    assert hist.shape == (2, 3) and hist[0].tolist() == [20., 20., total] and hist[1].tolist() == [0., 0., 0.]
    assert np.array_equal(got.transform, sc['rows'][:, 2]) and np.array_equal(got.atom, sc['rows'][:, 1])
    np.testing.assert_allclose(got.strength, sc['h'], rtol=1e-6)
    np.testing.assert_allclose(gains, nmf.detection_gains(got), rtol=1e-12)
    assert objective_of(nmf, got) <= 1e-8 * scale
    # a list at a local optimum comes back unchanged after one round
    again, _ = nmf.relabel_detections(got)
    assert key(again) == key(got) and nmf.relabel_history_.tolist() == [[0., 0., 0.]]
    # over='all' finds the atoms as well
    mixed = sc['wrong'].copy()
    mixed[::2, 1] = 1 - mixed[::2, 1]
    got, _ = nmf.relabel_detections(planted_det(sc, mixed), over='all', strengths='solve')
    assert np.array_equal(got.transform, sc['rows'][:, 2]) and np.array_equal(got.atom, sc['rows'][:, 1])
    # over='atoms' changes atoms only
    swapped = sc['rows'].copy()
    swapped[:, 1] = 1 - swapped[:, 1]
    got, _ = nmf.relabel_detections(planted_det(sc, swapped), over='atoms')
    assert np.array_equal(got.transform, sc['rows'][:, 2]) and np.array_equal(got.atom, sc['rows'][:, 1])


def test_rows_with_meeting_footprints_hop_in_different_rounds_and_the_objective_never_rises():
    sc = cells()
    W, A, D, T = sc['W'], sc['A'], sc['D'], 4
    true = np.array([[0, 0, 1, 13, 13], [0, 1, 2, 13, 15], [0, 1, 0, 30, 30]])   # origins (10, 10), (10, 12): they overlap
    h = np.array([1.5, 1.25, 2.])
    V = eref.render(tr.expand(W, 'rot90'), D, 1, 'valid', true[:, 0], true[:, 1] * T + true[:, 2], true[:, 3:], h)
    wrong = true.copy()
    wrong[:, 2] = (true[:, 2] + np.array([1, 3, 2])) % T
    nmf = holding(W, V, 'valid', 'rot90')
    one = dict(sc, mode='valid', h=h)
    got, _ = nmf.relabel_detections(planted_det(one, wrong))
    hist = nmf.relabel_history_
    print(hist.tolist())
    assert hist[0, :2].tolist() == [3., 2.] and hist[-1, 1] == 0. and hist.shape[1] == 3
    for strengths in ('mu', 'solve'):
        E = [objective_of(nmf, nmf.relabel_detections(planted_det(one, wrong), max_rounds=r, strengths=strengths)[0])
             for r in range(5)]
        print(strengths, E)
        assert all(later <= earlier * (1 + 1e-12) for earlier, later in zip(E, E[1:])) and E[-1] < E[0]
    got, _ = nmf.relabel_detections(planted_det(one, wrong), strengths='solve')
    assert np.array_equal(got.transform, true[:, 2]) and objective_of(nmf, got) <= 1e-8 * 0.5 * float(np.sum(V * V))


def test_a_hop_onto_an_existing_row_is_not_made():
    sc = cells()
    W, A, D = sc['W'], sc['A'], sc['D']
    W_eff = tr.expand(W, 'rot90')
    V = eref.render(W_eff, D, 1, 'valid', np.array([0]), np.array([0]), np.array([[13, 13]]), np.array([2.]))
    nmf = holding(W, V, 'valid', 'rot90')
    pair = as_det([0, 0], [0, 1], [[13, 13], [13, 13]], [1., 1.], A, 'valid', 4)   # the second wants the label of the first
    a, b = nmf.detection_alternatives(pair)
    assert np.argmax(landscape_gains(a, b)[1]) == 0
    got, _ = nmf.relabel_detections(pair, n_iterations=0, max_rounds=1)
    assert got.transform[1] != 0 and len(set(key(got))) == 2 and nmf.relabel_history_[0, 0] >= 1
    # the rule on lists: row 1's best plane is row 0's, so it stays; with the plane free it hops
    a, b = np.zeros((2, 4)), np.ones((2, 4))
    a[1, 0] = 1.
    rows = (np.array([0, 0]), np.array([0, 1]), np.array([[13, 13], [13, 13]]), np.zeros(2))
    hops = relabel_hops(*rows, a, b, 4, 1, A, D, (43, 43), 'valid', 0.)
    assert len(hops[0]) == 0 and hops[3] == 1 and hops[4] == 0.
    rows = (np.array([0, 0]), np.array([2, 1]), np.array([[13, 13], [13, 13]]), np.zeros(2))
    hops = relabel_hops(*rows, a, b, 4, 1, A, D, (43, 43), 'valid', 0.)
    assert hops[0].tolist() == [1] and hops[1].tolist() == [0] and hops[3] == 1 and hops[4] == 0.5
    # alone, the same row hops
    alone, _ = nmf.relabel_detections(rows_of(pair, [1]), n_iterations=0)
    assert alone.transform.tolist() == [0] and alone.atom.tolist() == [0] and alone.shift.tolist() == [[13, 13]]
    assert alone.strength[0] == pytest.approx(2., rel=1e-12)
    # relabel_hops: ties go to the row of the lower index and to the candidate of the lower index; the boxes of the two rows
    # meet, so the second waits for the next round
    a = np.zeros((2, 4))
    b = np.ones((2, 4))
    a[:, [2, 3]] = 1.
    hops = relabel_hops(np.array([0, 0]), np.array([0, 5]), np.array([[13, 13], [13, 14]]), np.zeros(2), a, b, 4, 1, A, D,
                        (43, 43), 'valid', 0.)
    assert hops[0].tolist() == [0] and hops[1].tolist() == [2] and hops[3] == 2 and hops[4] == 0.5
    far = relabel_hops(np.array([0, 0]), np.array([0, 5]), np.array([[13, 13], [13, 24]]), np.zeros(2), a, b, 4, 1, A, D,
                       (43, 43), 'valid', 0.)
    assert far[0].tolist() == [0, 1] and far[1].tolist() == [2, 6] and far[2].tolist() == [1., 1.] and far[4] == 1.
    # stride: the atoms in the row's orientation
    atoms = relabel_hops(np.array([0]), np.array([5]), np.array([[13, 13]]), np.zeros(1), a[:1, :2] + [[1., 0.]], b[:1, :2], 2,
                         4, A, D, (43, 43), 'valid', 0.)
    assert atoms[0].tolist() == [0] and atoms[1].tolist() == [1]


def test_a_row_with_nowhere_to_go_stays():
    """The choice of a round on alternatives the data does not support: every other plane with a <= 0 gives g = 0 there, and
    a row whose own gain is negative would 'improve' by hopping onto nothing."""
    A, D, S = (3, 3), (12, 14), (14, 16)
    one = (np.array([0]), np.array([1]))
    a, b = np.full((1, 4), -0.3), np.ones((1, 4))
    a[0, 1] = 0.1                                                   # own gain 1 * (0.1 - 1) + 1 / 2 < 0
    hops = relabel_hops(*one, np.array([[5, 5]]), np.ones(1), a, b, 4, 1, A, D, S, 'valid', 0.)
    assert len(hops[0]) == 0 and hops[1].shape == (0,) and hops[3] == 0 and hops[4] == 0.
    a[0, 3], b[0, 3] = 0.5, 2.                                      # ... and with one plane that sees something
    hops = relabel_hops(*one, np.array([[5, 5]]), np.ones(1), a, b, 4, 1, A, D, S, 'valid', 0.)
    assert hops[0].tolist() == [0] and hops[1].tolist() == [3] and hops[2].tolist() == [0.25] and hops[3] == 1
    # below min_improvement it stays; a single candidate plane has nowhere else to go
    assert len(relabel_hops(*one, np.array([[5, 5]]), np.ones(1), a, b, 4, 1, A, D, S, 'valid', 10.)[0]) == 0
    assert len(relabel_hops(*one, np.array([[5, 5]]), np.ones(1), a[:, :1], b[:, :1], 1, 1, A, D, S, 'valid', 0.)[0]) == 0
    assert len(relabel_hops(*(np.zeros(0, dtype=np.int64),) * 2, np.zeros((0, 2)), np.zeros(0), np.zeros((0, 4)),
                            np.zeros((0, 4)), 4, 1, A, D, S, 'valid', 0.)[0]) == 0


def test_zero_rounds_is_a_refit_with_its_gains():
    sc = cells()
    nmf = holding(sc['W'], sc['V'], sc['mode'], 'rot90')
    start = planted_det(sc, sc['wrong'])
    rows, gains = nmf.relabel_detections(start, n_iterations=7, sparsity_H=0.01, max_rounds=0)
    refit = nmf.refit_detections(start, 7, sparsity_H=0.01)
    for f in dataclasses.fields(Detections):
        assert np.array_equal(getattr(rows, f.name), getattr(refit, f.name))
    assert np.array_equal(gains, nmf.detection_gains(refit)) and nmf.relabel_history_.shape == (0, 3)
    none = rows_of(start, np.zeros(len(start), dtype=bool))
    rows, gains = nmf.relabel_detections(none)
    assert len(rows) == 0 and gains.shape == (0,) and nmf.relabel_history_.shape == (1, 3)
    for over, shape in (('transforms', (0, 4)), ('atoms', (0, 2)), ('all', (0, 2, 4))):
        a, b = nmf.detection_alternatives(none, over)
        assert a.shape == b.shape == shape


# -- 5. refusals and validation ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model():
    nmf = fitted((2, 1, 9, 10), 2, (3, 3), 'reflect', transforms='rot90')
    return nmf, nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)), min_distance=0)


def calls(nmf, det):
    return (lambda: nmf.detection_alternatives(det), lambda: nmf.relabel_detections(det))


def test_before_a_fit_they_raise_runtime_error(model):
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=_Stub(), transforms='rot90')
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
    assert nmf.detection_alternatives(det)[0].shape == (len(det), 4)


def test_volumes_are_refused():
    nmf = fitted((1, 1, 5, 5, 5), 1, (2, 2, 2))
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)), min_distance=0)
    for over in ('atoms', 'all'):
        for call in (lambda: nmf.detection_alternatives(det, over), lambda: nmf.relabel_detections(det, over)):
            with pytest.raises(NotImplementedError):
                call()


def test_the_candidate_sets_of_over(model):
    nmf, det = model
    assert nmf._alternative_set('transforms') == (4, 1) and nmf._alternative_set('atoms') == (2, 4)
    assert nmf._alternative_set('all') == (8, 1)
    for over in ('atom', 'transform', None, 3, ('all',)):
        for call in (lambda: nmf.detection_alternatives(det, over), lambda: nmf.relabel_detections(det, over)):
            with pytest.raises(ValueError, match='over must be one of'):
                call()
    plain = fitted((2, 1, 9, 10), 3, (3, 4), 'full')
    pdet = plain.detections(threshold=float(np.quantile(plain.H, 0.9)), min_distance=0)
    assert plain._alternative_set('atoms') == (3, 1) and plain._alternative_set('all') == (3, 1)
    for call in (lambda: plain.detection_alternatives(pdet, 'transforms'), lambda: plain.relabel_detections(pdet, 'transforms')):
        with pytest.raises(ValueError, match="over='transforms' needs a model with transforms"):
            call()
    assert plain.detection_alternatives(pdet, 'atoms')[0].shape == (len(pdet), 3)
    assert plain.detection_alternatives(pdet, 'all')[0].shape == (len(pdet), 3, 1)
    # the arithmetic of the three sets, against the rule spelled out row by row
    for P, n_alt, stride in ((8, 4, 1), (8, 2, 4), (8, 8, 1), (24, 8, 1), (24, 3, 8), (24, 24, 1), (12, 3, 2), (5, 1, 1)):
        planes, own = alternative_planes(np.arange(P), n_alt, stride)
        for p in range(P):
            want, j = aref.candidates(p, n_alt, stride)
            assert planes[p].tolist() == want and own[p] == j and all(0 <= q < P for q in want)
    planes, own = alternative_planes(np.arange(8), 4, 1)                     # 'transforms' of 2 atoms x 4
    assert planes[5].tolist() == [4, 5, 6, 7] and own[5] == 1
    planes, own = alternative_planes(np.arange(8), 2, 4)                     # 'atoms'
    assert planes[5].tolist() == [1, 5] and own[5] == 1 and planes[2].tolist() == [2, 6] and own[2] == 0
    with pytest.raises(ValueError):
        events_alternatives_numpy(np.ones((8, 1, 3, 3)), (9, 10), 1, 'full', [0], [0], [[0, 0]], [1.], np.ones((1, 1, 9, 10)),
                                  3, 1)


@pytest.mark.parametrize('kw', [dict(min_improvement=float('nan')), dict(min_improvement=float('inf')),
                                dict(min_improvement=-1e-9), dict(min_improvement='0.1'), dict(min_improvement=True),
                                dict(min_improvement=None), dict(max_rounds=-1), dict(max_rounds=1.5),
                                dict(max_rounds=True), dict(n_iterations=-1), dict(sparsity_H=-1.),
                                dict(strengths='exact'), dict(strengths='solve', sparsity_H=0.1),
                                dict(strengths='solve', tol=0.)], ids=str)
def test_bad_relabel_arguments_raise_value_error(model, kw):
    nmf, det = model
    with pytest.raises(ValueError):
        nmf.relabel_detections(det, **kw)


def test_bad_rows_raise_value_error_and_duplicates_are_scored_but_not_relabelled(model):
    nmf, det = model
    bad = dataclasses.replace(det, strength=np.where(np.arange(len(det)) == 1, -1., det.strength))
    for call in calls(nmf, bad):
        with pytest.raises(ValueError):
            call()
    twice = rows_of(det, np.r_[np.arange(len(det)), 0])
    a, b = nmf.detection_alternatives(twice, 'all')
    assert a.shape == (len(twice), 2, 4) and np.array_equal(a[-1], a[0]) and np.array_equal(b[-1], b[0])
    with pytest.raises(ValueError):
        nmf.relabel_detections(twice)
    before = (nmf.H.copy(), nmf.W.copy())
    got, gains = nmf.relabel_detections(det, n_iterations=5, max_rounds=2)
    assert len(got) == len(det) and len(set(key(got))) == len(det) and np.array_equal(got.shift, det.shift)
    assert np.array_equal(got.atom, det.atom) and np.array_equal(got.origin, det.origin)
    assert np.array_equal(nmf.H, before[0]) and np.array_equal(nmf.W, before[1])


# -- 6. the ABI -------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_typed():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tnmf_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(tnmf_hip_\w+)\s*\(', header))
    assert declared == set(_lib.EXPORTS) and len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    lib = _lib.load()
    vp, ll, ci = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    assert re.search(r'\bint tnmf_hip_events_alternatives\s*\(', header) and 'tnmf_hip_events_alternatives' in _lib.EXPORTS
    fn = lib.tnmf_hip_events_alternatives
    assert fn.restype is ci
    assert list(fn.argtypes) == [vp, ctypes.POINTER(_lib.Geom), ci, vp, vp, vp, ll, vp, vp, ci, ci, vp, vp, vp, vp]
    assert _lib.ABI_VERSION == 8 and lib.tnmf_hip_abi_version() == 8
    # an argument error is answered without a device: no context
    g = ctypes.byref(_lib.make_geom(1, 6, 1, (4,), (2,), 0))
    none, ctx = (None,) * 3, ctypes.c_void_p(1)
    assert fn(None, g, 0, *none, 0, None, None, 1, 1, None, None, None, None) == -1
    assert fn(ctx, None, 0, *none, 0, None, None, 1, 1, None, None, None, None) == -1
    assert fn(ctx, ctypes.byref(_lib.make_geom(1, 6, 1, (4, 4, 4), (2, 2, 2), 0)), 0, *none, 0, None, None, 1, 1, None, None,
              None, None) == _lib.E_UNSUPPORTED
    assert fn(ctx, ctypes.byref(_lib.make_geom(1, 6, 1, (4,), (2,), 2)), 0, *none, 0, None, None, 1, 1, None, None, None,
              None) == -3
    for n_alt, stride in ((0, 1), (-1, 1), (1, 0), (2, -1), (4, 1), (2, 2), (6, 2), (7, 1), (2 ** 30, 4)):
        assert fn(ctx, g, 0, *none, 1, None, None, n_alt, stride, None, None, None, None) == _lib.E_GEOM, (n_alt, stride)
    assert fn(ctx, g, 0, *none, -1, None, None, 1, 1, None, None, None, None) == _lib.E_GEOM
    assert fn(ctx, g, 4, *none, 1, None, None, 1, 1, None, None, None, None) == _lib.E_GEOM
    for n_alt, stride in ((1, 1), (2, 1), (3, 1), (6, 1), (2, 3), (3, 2), (1, 6)):   # the sets that divide 6 planes
        assert fn(ctx, g, 0, *none, (2 ** 31 - 1) // n_alt + 1, None, None, n_alt, stride, None, None, None,
                  None) == _lib.E_UNSUPPORTED, (n_alt, stride)
        assert fn(ctx, g, 0, *none, (2 ** 31 - 1) // n_alt, None, None, n_alt, stride, None, None, None, None) == -1
    assert fn(ctx, g, 0, *none, 2 ** 31, None, None, 1, 1, None, None, None, None) == _lib.E_UNSUPPORTED


def test_the_host_mirror_of_the_path_rule_has_the_kernels_limits():
    src = open(os.path.join(ROOT, 'tnmf_amd', 'csrc', 'alternatives.hip')).read()
    rule = re.search(r'constexpr int kPatchMax = (\d+);', src)
    assert rule and int(rule.group(1)) == aref.PATCH_MAX
    batch = re.search(r'constexpr int kBatch = (\d+);', src)
    assert batch and int(batch.group(1)) == aref.BATCH
