"""
Exact strengths of a list on CPU: the front end's ``solve_detections`` and the ``strengths='solve'`` keyword of the list drivers
over an oracle-backed backend without the hooks (the host fallbacks ``events_gram_numpy`` / ``events_solve_numpy``), in float64,
against tests/solve_reference.py -- dense occurrences, G_ref = Phi Phi', c_ref = Phi v and the KKT conditions; no solver.

Bars.  KKT: the solver stops at kkt <= tol on ITS matrix, which differs from G_ref by rounding orders below tol; against the
reference the bar is 2 * tol.  Objectives: by convexity E(h') >= E(h) + <g, h' - h> with g_i >= -r everywhere and |g_i| <= r on
the support of h, r = kkt * max |c|, so E(h) <= E(h') + r (|h|_1 + |h'|_1) for ANY h' >= 0.
"""
import dataclasses
import re

import numpy as np
import pytest

import events_gain_reference as gref
import solve_reference as sr
from conftest import ROOT
from test_events_cpu import MODES, fitted
from test_pursuit_cpu import NOISY_MIN_GAIN, key, model_of
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF
from tnmf_amd.events_host import events_gram_numpy, events_solve_numpy

TOL = 1e-8
NAMES = ('tnmf_hip_events_pairs', 'tnmf_hip_events_gram', 'tnmf_hip_events_project', 'tnmf_hip_events_nnls')


def det_of(case, strength=None):
    h = case['strength'] if strength is None else strength
    shift = np.array(case['shift'])
    return Detections(sample=np.array(case['sample']), atom=np.array(case['plane']),
                      transform=np.zeros(len(shift), dtype=np.int64), shift=shift, origin=shift,
                      strength=np.array(h, dtype=np.float64))


def reference(case):
    return sr.gram(case['V'], case['W'], case['mode'], case['sample'], case['plane'], case['shift'])


def slack(G, c, h, other):
    return sr.kkt(G, c, h) * np.max(np.abs(c)) * (np.sum(np.abs(h)) + np.sum(np.abs(other)))


# -- 1. the Gram matrix of the host fallback ---------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_the_host_gram_matrix_is_the_reference(mode):
    case = sr.decoys(0, mode)
    G_ref, c_ref = reference(case)
    args = (case['W'], case['V'].shape[2:], case['V'].shape[0], mode, case['sample'], case['plane'], case['shift'])
    G, c = events_gram_numpy(*args, V=case['V'])
    bar = 8 * sr.taps_of(case['W']) * 2. ** -52
    assert np.all(np.abs(G - G_ref) <= bar * G_ref) and np.all(np.abs(c - c_ref) <= bar * c_ref)
    assert np.array_equal(G, G.T)
    (row_start, col, val) = events_gram_numpy(*args, sparse=True)
    dense, present = sr.densify(len(c), row_start, col, val)
    assert np.array_equal(dense, G) and np.all(present[G_ref != 0])


# -- 2. solve_detections on the fallback ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_solve_detections_reaches_the_minimum(mode):
    case = sr.decoys(1, mode)
    G, c = reference(case)
    nmf = model_of(case['W'], case['V'], mode)
    det = det_of(case)
    solved = nmf.solve_detections(det, tol=TOL)
    h = solved.strength
    assert nmf.solve_converged_ and 0 < nmf.solve_n_iter_ <= 1000
    assert nmf.solve_history_.shape[1] == 2 and nmf.solve_history_[-1, 0] == nmf.solve_n_iter_
    assert nmf.solve_history_[-1, 1] <= TOL < nmf.solve_history_[0, 1]
    assert np.all(h >= 0) and h.dtype == np.float64
    k = sr.kkt(G, c, h)
    print(f'{mode}: K {len(h)}, {nmf.solve_n_iter_} iterations, kkt_ref {k:.3g}')
    assert k <= 2 * TOL
    E = sr.objective(case['V'], G, c, h)
    mu50 = nmf.refit_detections(det, n_iterations=50).strength
    E50 = sr.objective(case['V'], G, c, mu50)
    print(f'{mode}: E solve {E:.6g}, 50 MU {E50:.6g}')
    assert E <= E50
    assert key(solved) == key(det) and np.array_equal(solved.shift, det.shift)


@pytest.mark.parametrize('mode', MODES)
def test_solve_detections_is_not_above_five_thousand_refit_steps(mode):
    # (5000 steps on the host cost seconds at K = 90: a scene of the same make with 16 x 18 samples, 4 x 4 atoms, K about 40)
    case = sr.decoys(3, mode, D=(16, 18), A=(4, 4), n_true=5, n_random=8)
    G, c = reference(case)
    assert np.count_nonzero(G) > 6 * len(c), 'the rows couple'
    nmf = model_of(case['W'], case['V'], mode)
    det = det_of(case)
    h = nmf.solve_detections(det, tol=TOL).strength
    assert nmf.solve_converged_ and sr.kkt(G, c, h) <= 2 * TOL
    mu50 = nmf.refit_detections(det, n_iterations=50).strength
    mu5000 = nmf.refit_detections(det, n_iterations=5000).strength
    E, E50, E5000 = (sr.objective(case['V'], G, c, x) for x in (h, mu50, mu5000))
    print(f'{mode}: K {len(c)}, {nmf.solve_n_iter_} iterations, E solve {E:.8g}, 50 MU {E50:.8g}, 5000 MU {E5000:.8g}, '
          f'slack {slack(G, c, h, mu5000):.3g}')
    assert E <= E50
    assert E <= E5000 + slack(G, c, h, mu5000)


def test_zero_strengths_grow_and_a_row_on_blank_data_ends_at_zero():
    case = sr.decoys(2, 'valid')
    # one more sample that is blank, with one row on it
    V = np.concatenate([case['V'], np.zeros_like(case['V'][:1])])
    blank = dict(case, V=V, sample=np.append(case['sample'], 2), plane=np.append(case['plane'], 0),
                 shift=np.vstack([case['shift'], [[9, 9]]]), strength=np.append(np.zeros(len(case['sample'])), 1.))
    G, c = reference(blank)
    nmf = model_of(blank['W'], V, 'valid')
    det = det_of(blank)
    h = nmf.solve_detections(det).strength
    assert nmf.solve_converged_ and sr.kkt(G, c, h) <= 2 * TOL
    assert np.all(h[:-1][case['true']] > 0.5)   # the planted rows grew from 0
    assert h[-1] == 0. and (G @ h - c)[-1] >= 0
    assert np.all(nmf.refit_detections(det, n_iterations=5).strength[:-1] == 0)   # (what the multiplicative update does)


def test_max_iterations_zero_returns_the_projected_start_and_an_unconverged_run_does_not_raise():
    case = sr.decoys(0, 'valid')
    G, c = reference(case)
    nmf = model_of(case['W'], case['V'], 'valid')
    det = det_of(case)
    out = nmf.solve_detections(det, max_iterations=0)
    assert np.array_equal(out.strength, det.strength) and nmf.solve_n_iter_ == 0 and not nmf.solve_converged_
    assert nmf.solve_history_.shape == (1, 2)
    assert nmf.solve_history_[0, 1] == pytest.approx(sr.kkt(G, c, det.strength), rel=1e-9)
    out = nmf.solve_detections(det, max_iterations=13)
    assert nmf.solve_n_iter_ == 13 and not nmf.solve_converged_ and np.all(out.strength >= 0)
    assert nmf.solve_history_[:, 0].tolist() == [0, 10, 13]
    assert nmf.solve_history_[-1, 1] == pytest.approx(sr.kkt(G, c, out.strength), rel=1e-6)
    empty = nmf.solve_detections(Detections(**{f.name: getattr(det, f.name)[:0] for f in dataclasses.fields(Detections)}))
    assert len(empty) == 0 and nmf.solve_converged_ and nmf.solve_n_iter_ == 0


def test_the_host_solver_agrees_with_scipy():
    nnls = pytest.importorskip('scipy.optimize').nnls
    case = sr.decoys(0, 'reflect')
    G, c = reference(case)
    h, info = events_solve_numpy(G, c, np.ones(len(c)), 1e-10, 10000)
    assert info['converged']
    Phi = sr.occurrences(case['W'], case['V'].shape[2:], case['V'].shape[0], 'reflect', case['sample'], case['plane'],
                         case['shift'])
    x, _ = nnls(Phi.T, case['V'].reshape(-1))
    assert sr.objective(case['V'], G, c, h) <= sr.objective(case['V'], G, c, x) + slack(G, c, h, x)
    assert np.max(np.abs(h - x)) <= 1e-6


# -- 3. validation and refusals ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model():
    case = sr.decoys(0, 'valid')
    return model_of(case['W'], case['V'], 'valid'), det_of(case)


@pytest.mark.parametrize('kw', [dict(tol=0.), dict(tol=-1e-3), dict(tol=float('nan')), dict(tol=float('inf')),
                                dict(tol='x'), dict(tol=True), dict(max_iterations=-1), dict(max_iterations=2.5),
                                dict(max_iterations=True)])
def test_bad_solve_arguments_raise_value_error(model, kw):
    nmf, det = model
    before = (nmf.solve_history_.copy(), nmf.solve_n_iter_, nmf.solve_converged_)
    with pytest.raises(ValueError):
        nmf.solve_detections(det, **kw)
    for driver in (lambda **k: nmf.prune_detections(det, 0.01, **k), lambda **k: nmf.pursue_detections(0.01, **k),
                   lambda **k: nmf.relocate_detections(det, **k)):
        with pytest.raises(ValueError):
            driver(strengths='solve', **kw)
    assert np.array_equal(before[0], nmf.solve_history_) and before[1:] == (nmf.solve_n_iter_, nmf.solve_converged_)


def test_duplicates_and_volumes_and_other_objectives_are_refused(model):
    nmf, det = model
    twice = Detections(**{f.name: np.concatenate([getattr(det, f.name)[:3]] * 2) for f in dataclasses.fields(Detections)})
    with pytest.raises(ValueError, match='distinct'):
        nmf.solve_detections(twice)
    with pytest.raises(RuntimeError):
        TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=type(nmf._backend)('valid')).solve_detections(det)
    message = re.escape('solve_detections covers the plain Frobenius objective (beta_loss 2, no weights)')
    nmf._weighted = True
    try:
        with pytest.raises(NotImplementedError, match=message):
            nmf.solve_detections(det)
    finally:
        nmf._weighted = False
    nmf._beta = 1.
    try:
        with pytest.raises(NotImplementedError, match=message):
            nmf.solve_detections(det)
    finally:
        nmf._beta = 2.
    vol = fitted((1, 1, 5, 5, 5), 1, (2, 2, 2))
    with pytest.raises(NotImplementedError, match='volumes'):
        vol.solve_detections(vol.detections(threshold=float(np.quantile(vol.H, 0.9)), min_distance=0))


def test_the_drivers_refuse_a_sparsity_with_solve_and_an_unknown_keyword(model):
    nmf, det = model
    for driver in (lambda **k: nmf.prune_detections(det, 0.01, **k), lambda **k: nmf.pursue_detections(0.01, **k),
                   lambda **k: nmf.relocate_detections(det, **k)):
        with pytest.raises(ValueError, match='sparsity_H must be 0'):
            driver(strengths='solve', sparsity_H=0.1)
        with pytest.raises(ValueError, match="strengths must be 'mu' or 'solve'"):
            driver(strengths='exact')


# -- 4. the drivers --------------------------------------------------------------------------------------------------------------
def test_strengths_mu_is_the_call_without_the_keyword():
    case = gref.planted(0, 'reflect')
    nmf = model_of(case['W'], case['V'], 'reflect')
    det = det_of(case)
    for call in (lambda **k: nmf.prune_detections(det, 0.01, n_iterations=20, **k),
                 lambda **k: nmf.pursue_detections(NOISY_MIN_GAIN, max_rounds=3, n_iterations=20, **k),
                 lambda **k: nmf.relocate_detections(det, n_iterations=20, max_rounds=2, **k)):
        (a, ga), (b, gb) = call(), call(strengths='mu')
        for f in dataclasses.fields(Detections):
            assert np.array_equal(getattr(a, f.name), getattr(b, f.name)), f.name
        assert np.array_equal(ga, gb)


@pytest.mark.parametrize('mode', MODES)
def test_pursuit_with_solve_is_orthogonal_matching_pursuit(mode):
    case = gref.planted(0, mode, n_spurious=0)
    nmf = model_of(case['W'], case['V'], mode)
    mu, _ = nmf.pursue_detections(NOISY_MIN_GAIN)
    det, gains = nmf.pursue_detections(NOISY_MIN_GAIN, strengths='solve', tol=TOL)
    assert nmf.solve_converged_
    t = case['true']
    planted = sorted(map(tuple, np.column_stack([case['sample'][t], case['plane'][t], np.zeros(t.sum(), dtype=int),
                                                  case['shift'][t]]).tolist()))
    assert set(planted) <= set(key(det))
    as_case = lambda d: dict(case, sample=d.sample, plane=d.atom, shift=d.shift)   # noqa: E731
    G, c = reference(as_case(det))
    Gm, cm = reference(as_case(mu))
    h = det.strength
    E, Emu = sr.objective(case['V'], G, c, h), sr.objective(case['V'], Gm, cm, mu.strength)
    print(f'{mode}: {len(det)} rows (mu: {len(mu)}), E solve {E:.6g}, mu {Emu:.6g}, kkt_ref {sr.kkt(G, c, h):.3g}')
    assert sr.kkt(G, c, h) <= 2 * TOL
    assert E <= Emu + slack(G, c, h, mu.strength)
    # a = <phi, V - R> = 0 on the support: the gain of a row is h^2 b / 2, up to h * |a| and the rounding of the sums
    cmax, taps = np.max(np.abs(c)), sr.taps_of(case['W'])
    bar = h * 2 * TOL * cmax + 8 * taps * 2. ** -52 * (h * c + h * (G @ h) + 0.5 * h * h * np.diag(G))
    assert np.all(np.abs(gains - 0.5 * h * h * np.diag(G)) <= bar)


def test_prune_and_relocate_take_their_strengths_from_the_solver():
    case = gref.planted(1, 'valid')
    nmf = model_of(case['W'], case['V'], 'valid')
    det = det_of(case)
    kept, gains = nmf.prune_detections(det, 0.01, strengths='solve')
    assert nmf.solve_converged_
    assert key(kept) == key(Detections(**{f.name: getattr(det, f.name)[case['true']]
                                         for f in dataclasses.fields(Detections)}))
    G, c = reference(dict(case, sample=kept.sample, plane=kept.atom, shift=kept.shift))
    assert sr.kkt(G, c, kept.strength) <= 2 * TOL
    moved, _ = nmf.relocate_detections(kept, strengths='solve', max_rounds=2)
    G, c = reference(dict(case, sample=moved.sample, plane=moved.atom, shift=moved.shift))
    assert sr.kkt(G, c, moved.strength) <= 2 * TOL


# -- 5. the ABI -----------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_and_exported():
    header = open(f'{ROOT}/include/tnmf_hip.h').read()
    assert 'events: exact strengths' in header
    for name in NAMES:
        assert re.search(rf'\bint {name}\s*\(', header) and name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 8 and '#define TNMF_HIP_ABI_VERSION 8' in header
    assert 'solve.hip' in open(f'{ROOT}/tnmf_amd/csrc/Makefile').read()
