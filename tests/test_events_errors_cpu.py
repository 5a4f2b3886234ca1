"""
Standard errors of the strengths of a list on CPU: the host mirror ``events_inverse_diag_numpy`` and the front end's
``detection_errors`` over an oracle-backed backend without the hook, in float64, against tests/errors_reference.py -- the dense
Gram matrix, numpy.linalg.inv of its active block, components by breadth-first search.  The bar of d is that module's; a
standard error is sigma * sqrt(d), so its relative bar is half of d's (plus the two roundings of the square root and the
product: 2^-51).  The scenes are checked for cond_2 <= 1e4 here, on the reference alone, so that the bar means something.
"""
import dataclasses
import math
import re

import numpy as np
import pytest

import errors_reference as er
import events_reference as eref
import solve_reference as sr
from conftest import ROOT
from test_events_cpu import MODES, fitted
from test_events_solve_cpu import det_of
from test_pursuit_cpu import model_of
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF
from tnmf_amd.events_host import events_gram_numpy, events_inverse_diag_numpy, events_solve_numpy

INFO_KEYS = {'noise', 'dof', 'residual_energy', 'n_active', 'n_components', 'largest_component', 'n_singular', 'rounds'}


def host_gram(case):
    return events_gram_numpy(case['W'], case['V'].shape[2:], case['V'].shape[0], case['mode'], case['sample'], case['plane'],
                             case['shift'], V=case['V'], sparse=True)


def check_d(d, ref, what):
    """d against the reference inside its bar, NaN exactly off the active rows; prints the observed maximum beside the bar."""
    on = ref['size'] > 0
    assert np.all(np.isnan(d[~on])) and np.all(np.isfinite(d[on]))
    err = np.abs(d[on] - ref['d'][on]) / ref['d'][on]
    worst = np.argmax(err / ref['bar'][on])
    print(f'{what}: {on.sum()} active rows, max |d - ref| / ref {err.max():.3g}; closest to its bar {err[worst]:.3g} of '
          f'{ref["bar"][on][worst]:.3g} (n {ref["size"][on][worst]}, cond {ref["kappa"][on][worst]:.3g})')
    assert np.all(err <= ref['bar'][on])


# -- 1. the scenes, on the reference alone -------------------------------------------------------------------------------------
def test_the_chain_has_the_sizes_it_is_for_and_is_well_conditioned():
    case = er.chain()
    ref = case['ref']
    assert sorted(len(g) for g in ref['groups']) == sorted(er.CHAIN_SIZES)
    assert er.N_LDS == _lib.EVENT_INVERSE_LDS and {er.N_LDS - 1, er.N_LDS, er.N_LDS + 1, 300, 1, 64} <= set(er.CHAIN_SIZES)
    on = ref['size'] > 0
    print(f'chain: K {len(on)}, active {on.sum()}, cond <= {np.nanmax(ref["kappa"]):.3g}')
    assert np.nanmax(ref['kappa']) <= 1e4
    # every row of strength 0 touches active rows of two components: the block is block diagonal only WITHOUT them
    G = case['G']
    comp = np.full(len(on), -1)
    for k, g in enumerate(ref['groups']):
        comp[g] = k
    assert (~on).sum() == len(er.CHAIN_SIZES) - 1
    for i in np.flatnonzero(~on):
        touched = np.flatnonzero((G[i] != 0) & on)
        assert len(touched) == 2 and len(set(comp[touched])) == 2 and G[touched[0], touched[1]] == 0
    assert not np.array_equal(np.argsort(case['shift'][:, 0]), np.arange(len(on))), 'the rows are permuted'
    for mode in MODES:
        s = sr.decoys(0, mode)
        G, _ = sr.gram(s['V'], s['W'], mode, s['sample'], s['plane'], s['shift'])
        assert np.nanmax(er.inverse_diag(G, np.ones(len(G), dtype=bool), sr.taps_of(s['W']))['kappa']) <= 1e4


# -- 2. the host mirror -----------------------------------------------------------------------------------------------------------
def test_the_host_mirror_on_the_chain():
    case = er.chain()
    ref = case['ref']
    G, _ = host_gram(case)
    active = case['strength'] > 0
    d, info = events_inverse_diag_numpy(G, active, 300)
    check_d(d, ref, 'chain, host')
    assert info['sizes'].tolist() == sorted(er.CHAIN_SIZES) and not info['status'].any()
    assert (info['n_active'], info['n_components'], info['largest_component'], info['n_singular']) == \
        (int(active.sum()), len(er.CHAIN_SIZES), 300, 0)
    assert np.array_equal(info['row_size'], ref['size'])
    with pytest.raises(ValueError, match=r'300 rows.*max_component=299'):
        events_inverse_diag_numpy(G, active, 299)
    # a dense matrix gives the same
    d2, _ = events_inverse_diag_numpy(case['G'], active, 300)
    assert np.allclose(d2[active], d[active], rtol=1e-9, atol=0)


@pytest.mark.parametrize('mode', MODES)
def test_the_host_mirror_on_coupled_rows_with_some_not_active(mode):
    case = sr.decoys(0, mode)
    G_ref, _ = sr.gram(case['V'], case['W'], mode, case['sample'], case['plane'], case['shift'])
    active = np.arange(len(G_ref)) % 3 != 1
    ref = er.inverse_diag(G_ref, active, sr.taps_of(case['W']))
    d, info = events_inverse_diag_numpy(host_gram(case)[0], active)
    check_d(d, ref, f'decoys {mode}, host')
    assert info['sizes'].tolist() == [len(g) for g in ref['groups']] and info['n_singular'] == 0
    groups = {tuple(g) for g in ref['groups']}
    assert all(len({case['sample'][i] for i in g}) == 1 for g in groups), 'rows of two samples never share a component'
    vif = np.diag(G_ref)[active] * d[active]
    assert np.all(vif >= 1 - ref['bar'][active])


# -- 3. the front end on the oracle backend -----------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_detection_errors_against_the_reference(mode):
    case = sr.decoys(0, mode)
    nmf = model_of(case['W'], case['V'], mode)
    det = nmf.solve_detections(det_of(case), tol=1e-10)
    h = det.strength.astype(np.float64)
    assert np.any(h == 0) and np.any(h > 0)
    G, c = sr.gram(case['V'], case['W'], mode, case['sample'], case['plane'], case['shift'])
    taps = sr.taps_of(case['W'])
    ref = er.inverse_diag(G, h > 0, taps)
    state = (nmf.W.copy(), nmf.H.copy(), {f.name: np.array(getattr(det, f.name)) for f in dataclasses.fields(Detections)})
    stderr, vif = nmf.detection_errors(det, noise=0.5)
    info = nmf.errors_info_
    assert set(info) == INFO_KEYS and stderr.dtype == vif.dtype == np.float64 and stderr.shape == vif.shape == h.shape
    check_d((stderr / 0.5) ** 2, dict(ref, bar=ref['bar'] + 2. ** -50), f'front end {mode}')
    on = h > 0
    assert np.all(np.isnan(vif[~on])) and np.all(vif[on] >= 1 - ref['bar'][on]) and np.all(vif[ref['size'] == 1] == 1.)
    assert np.all(np.abs(vif[on] - np.diag(G)[on] * ref['d'][on]) <= (ref['bar'][on] + 8 * taps * 2. ** -52) * vif[on])
    assert (info['n_active'], info['n_components'], info['largest_component'], info['n_singular'], info['noise']) == \
        (int(on.sum()), len(ref['groups']), max(len(g) for g in ref['groups']), 0, 0.5)
    # noise scales the standard errors linearly and leaves the inflation alone
    twice, vif2 = nmf.detection_errors(det, noise=1.)
    assert np.array_equal(twice[on], 2. * stderr[on]) and np.array_equal(vif2[on], vif[on])
    # the estimate: the residual energy against ||V - R||^2 of the reference, the degrees of freedom
    R = eref.render(case['W'], case['V'].shape[2:], case['V'].shape[0], mode, case['sample'], case['plane'], case['shift'], h)
    energy = float(np.sum((case['V'] - R) ** 2))
    est, _ = nmf.detection_errors(det)
    info = nmf.errors_info_
    bar = 16 * taps * 2. ** -52 * (np.sum(case['V'] ** 2) + 2 * c @ h + h @ G @ h)
    print(f'{mode}: residual energy {info["residual_energy"]:.6g}, reference {energy:.6g}, bar {bar:.3g}')
    assert abs(info['residual_energy'] - energy) <= bar
    assert info['dof'] == case['V'].size - on.sum() and info['noise'] == math.sqrt(info['residual_energy'] / info['dof'])
    assert np.allclose(est[on], info['noise'] * stderr[on] / 0.5, rtol=2. ** -50, atol=0)
    # nothing of the model or the list moved
    assert np.array_equal(state[0], nmf.W) and np.array_equal(state[1], nmf.H)
    assert all(np.array_equal(v, getattr(det, k)) for k, v in state[2].items())


def singular_case(mode='valid'):
    """Ordinary rows and, among them, two orientations of the rotation-symmetric atom at one shift."""
    W = er.symmetric_atoms()
    rng = np.random.default_rng(8)
    D = (30, 32)
    S = eref.shift_shape(D, W.shape[2:], mode)
    # the twins and three rows that overlap them; further down, rows of the other atom under every orientation
    rows = {(0, 0, 1, 5, 6), (0, 0, 3, 5, 6), (0, 1, 0, 4, 7), (0, 1, 2, 7, 5), (0, 0, 0, 3, 4)}
    while len(rows) < 17:
        rows.add((0, 1, int(rng.integers(4)), int(rng.integers(12, S[0])), int(rng.integers(S[1]))))
    rows = np.array(sorted(rows), dtype=np.int64)[rng.permutation(len(rows))]
    det = Detections(sample=rows[:, 0], atom=rows[:, 1], transform=rows[:, 2], shift=rows[:, 3:], origin=rows[:, 3:],
                     strength=1. + np.arange(len(rows)) / 8.)
    T = 4
    W_eff = np.stack([np.rot90(W[m], k, axes=(1, 2)) for m in range(len(W)) for k in range(T)])
    V = eref.render(W_eff, D, 1, mode, det.sample, det.atom * T + det.transform, det.shift, det.strength) + 0.01
    twins = (det.atom == 0) & np.all(det.shift == (5, 6), axis=1)
    assert twins.sum() == 2
    return W, V, det, twins


def check_singular(nmf, det, twins, what):
    G, _ = sr.gram(nmf.V.astype(np.float64), nmf.transformed_atoms.astype(np.float64).reshape((-1,) + nmf.W.shape[1:]),
                   nmf._backend._reconstruction_mode, det.sample, det.atom * nmf.n_transforms + det.transform, det.shift)
    groups = er.components(G, np.ones(len(G), dtype=bool))
    bad = next(g for g in groups if set(np.flatnonzero(twins)) <= set(g))
    others = np.setdiff1d(np.arange(len(G)), bad)
    ref = er.inverse_diag(G, np.isin(np.arange(len(G)), others), sr.taps_of(nmf.W))
    stderr, vif = nmf.detection_errors(det, noise=1.)
    assert nmf.errors_info_['n_singular'] == 1 and nmf.errors_info_['n_components'] == len(groups)
    assert np.all(np.isposinf(stderr[bad])) and np.all(np.isposinf(vif[bad]))
    d = stderr ** 2
    d[bad] = np.nan
    check_d(d, dict(ref, bar=ref['bar'] + 2. ** -50), what)
    assert len(others) >= 5 and len(bad) >= 3 and np.nanmax(ref['kappa']) <= 1e4


def test_two_orientations_of_a_symmetric_atom_at_one_place_are_singular():
    W, V, det, twins = singular_case()
    nmf = model_of(W, V, 'valid', transforms='rot90')
    check_singular(nmf, det, twins, 'singular, host')


@pytest.fixture(scope='module')
def model():
    case = sr.decoys(0, 'valid')
    nmf = model_of(case['W'], case['V'], 'valid')
    return nmf, nmf.solve_detections(det_of(case))


@pytest.mark.parametrize('kw', [dict(noise=0.), dict(noise=-1.), dict(noise=float('nan')), dict(noise=float('inf')),
                                dict(noise='x'), dict(noise=True), dict(max_component=0), dict(max_component=2.5),
                                dict(max_component=True), dict(max_component=None)])
def test_bad_arguments_raise_value_error(model, kw):
    nmf, det = model
    with pytest.raises(ValueError):
        nmf.detection_errors(det, **kw)


def test_refusals_and_the_cap(model):
    nmf, det = model
    twice = Detections(**{f.name: np.concatenate([getattr(det, f.name)[:3]] * 2) for f in dataclasses.fields(Detections)})
    with pytest.raises(ValueError, match='distinct'):
        nmf.detection_errors(twice)
    with pytest.raises(RuntimeError):
        TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=type(nmf._backend)('valid')).detection_errors(det)
    message = re.escape('detection_errors covers the plain Frobenius objective (beta_loss 2, no weights)')
    for name, value, back in (('_weighted', True, False), ('_beta', 1., 2.)):
        setattr(nmf, name, value)
        try:
            with pytest.raises(NotImplementedError, match=message):
                nmf.detection_errors(det)
        finally:
            setattr(nmf, name, back)
    vol = fitted((1, 1, 5, 5, 5), 1, (2, 2, 2))
    with pytest.raises(NotImplementedError, match='volumes'):
        vol.detection_errors(vol.detections(threshold=float(np.quantile(vol.H, 0.9)), min_distance=0))
    nmf.detection_errors(det)
    largest = nmf.errors_info_['largest_component']
    assert largest >= 2
    with pytest.raises(ValueError, match=rf'{largest} rows.*max_component={largest - 1}'):
        nmf.detection_errors(det, max_component=largest - 1)
    nmf.detection_errors(det, max_component=largest)
    # more active rows than observations: the noise cannot be estimated, but can be given
    tiny = model_of(np.ones((1, 1, 1, 1)), np.ones((1, 1, 2, 2)), 'valid')
    every = np.array([(0, 0, 0, y, x) for y in range(2) for x in range(2)])
    all_rows = Detections(sample=every[:, 0], atom=every[:, 1], transform=every[:, 2], shift=every[:, 3:],
                          origin=every[:, 3:], strength=np.ones(4))
    with pytest.raises(ValueError, match='noise'):
        tiny.detection_errors(all_rows)
    stderr, vif = tiny.detection_errors(all_rows, noise=2.)
    assert tiny.errors_info_['dof'] == 0 and np.array_equal(stderr, np.full(4, 2.)) and np.array_equal(vif, np.ones(4))


# -- 4. the errors are the scatter of the strengths ------------------------------------------------------------------------------
def test_the_predicted_errors_are_the_scatter_of_the_solved_strengths_under_noise():
    """200 draws of Gaussian noise of known sigma on a planted scene, solved each: for a strength that is active in every
    draw, (m - 1) s^2 / (sigma^2 d) is chi-square with m - 1 degrees of freedom when h is the least-squares estimate on that
    support (linear in the noise, which is Gaussian), so s lies in sigma sqrt(d) * sqrt([lo, hi] / (m - 1)) with probability
    99.9 %, [lo, hi] that distribution's central 99.9 % interval."""
    rng = np.random.default_rng(2024)
    m, sigma, mode = 200, 0.01, 'valid'
    N, C, D, A, M = 1, 1, (16, 18), (4, 4), 2
    W = rng.random((M, C) + A) + 0.1
    W /= W.sum(axis=(2, 3), keepdims=True)
    rows = np.array([(0, 0, 3, 3), (0, 1, 4, 5), (0, 0, 6, 4), (0, 1, 9, 10), (0, 0, 10, 12), (0, 1, 2, 12), (0, 0, 11, 2),
                     (0, 1, 12, 3), (0, 0, 5, 7)])
    h0 = 1. + np.arange(len(rows)) / 8.
    Phi = sr.occurrences(W, D, N, mode, rows[:, 0], rows[:, 1], rows[:, 2:])
    G = Phi @ Phi.T
    assert np.count_nonzero(G) > 2 * len(rows), 'the rows couple'
    clean = h0 @ Phi
    d, info = events_inverse_diag_numpy(G, np.ones(len(rows), dtype=bool))
    assert info['n_singular'] == 0 and info['largest_component'] >= 3
    solved = np.empty((m, len(rows)))
    for k in range(m):
        c = Phi @ (clean + sigma * rng.standard_normal(clean.shape))
        solved[k], run = events_solve_numpy(G, c, h0, 1e-12, 100000)
        assert run['converged']
    assert np.all(solved > 0), 'every strength is active in every draw'
    lo, hi = er.chi_square_interval(m - 1, 1e-3)
    # (the quantiles against Wilson and Hilferty's cube-root approximation, z = 3.2905 for a tail of 0.0005)
    wh = [(m - 1) * (1 - 2 / (9 * (m - 1)) + z * math.sqrt(2 / (9 * (m - 1)))) ** 3 for z in (-3.2905, 3.2905)]
    assert abs(lo - wh[0]) < 0.5 and abs(hi - wh[1]) < 0.5 and lo < m - 1 < hi
    s = solved.std(axis=0, ddof=1)
    predicted = sigma * np.sqrt(d)
    print('s / predicted:', np.round(s / predicted, 3), 'interval', math.sqrt(lo / (m - 1)), math.sqrt(hi / (m - 1)))
    assert np.all(s >= predicted * math.sqrt(lo / (m - 1))) and np.all(s <= predicted * math.sqrt(hi / (m - 1)))


# -- 5. the ABI -----------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_typed():
    header = open(f'{ROOT}/include/tnmf_hip.h').read()
    name = 'tnmf_hip_events_inverse_diag'
    assert 'events: standard errors' in header and re.search(rf'\bint {name}\s*\(', header) and name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 8 and '#define TNMF_HIP_ABI_VERSION 8' in header
    assert _lib.EVENT_INVERSE_LDS == int(re.search(r'#define TNMF_EVENTS_INVERSE_LDS (\d+)', header).group(1))
    n = _lib.EVENT_INVERSE_LDS                    # the largest n with the triangle and the diagonal inside 160 KB
    assert n * (n + 3) // 2 * 8 <= 160 * 1024 < (n + 1) * (n + 4) // 2 * 8
    assert 'covariance.hip' in open(f'{ROOT}/tnmf_amd/csrc/Makefile').read()
    fn = getattr(_lib.load(), name)
    assert len(fn.argtypes) == 17 and fn.restype is not None


def test_null_arguments_answer_minus_one_without_a_device():
    fn = _lib.load().tnmf_hip_events_inverse_diag
    assert fn(None, 0, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None) == -1
    assert fn(None, -1, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None) == -1
