"""
Standard errors of the strengths of a list on the GPU: tnmf_hip_events_inverse_diag through the backend's hooks
(``event_components``, ``inverse_diag_event_list``, ``event_errors``) and ``detection_errors`` on ``backend='hip'``, against
tests/errors_reference.py in float64 on the same numbers: the dense Gram matrix, numpy.linalg.inv of its active block, components
by breadth-first search.  The bar of d is that module's, per component: kappa * (8 * taps + 4 * n^2) * 2^-52 * d_ref; the scenes
are checked for kappa <= 1e4 in tests/test_events_errors_cpu.py.  The chain (errors_reference.chain) holds components of 1, 2, 3,
63, 64, 65, N_LDS - 1, N_LDS, N_LDS + 1 and 300 rows: the elementwise path, both workgroup sizes and every size class of the LDS
path on either side of its limits, and the path through the scratch, in one launch sequence.
"""
import ctypes
import dataclasses
import re

import numpy as np
import pytest
import torch

import errors_reference as er
import events_reference as eref
import solve_reference as sr
from test_events_cpu import MODES
from test_events_errors_cpu import INFO_KEYS, check_d, check_singular, singular_case
from test_events_solve_cpu import det_of
from test_hip_events import DTYPES, backend, dev, p
from test_hip_events_solve import GEOMETRIES, case as gram_case
from test_hip_pursuit import hip_model
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF

pytestmark = pytest.mark.gpu


def device_csr(be, W, dt, sample, plane, shift):
    Wd = dev(W, dt)
    s, pl, u, _ = be._check_events(W.shape[0], sample, plane, shift, np.ones(len(sample)))
    images, cell_start, events = be.event_list(s, pl, u)
    return be.gram_event_list(Wd, images, cell_start, events)


def chain_backend(dt):
    case = er.chain()
    be = backend(1, 1, case['W'].shape[0], case['V'].shape[2:], case['W'].shape[2:], 'valid', dt)
    return case, be, device_csr(be, case['W'], dt, case['sample'], case['plane'], case['shift'])


# -- 1. the three paths on the chain ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
def test_every_size_path_on_the_chain(dt):
    case, be, csr = chain_backend(dt)
    ref = case['ref']
    active = torch.from_numpy(case['strength'] > 0).cuda()
    d, info = be.inverse_diag_event_list(csr, active, 300)
    torch.cuda.synchronize()
    d = d.cpu().numpy()
    check_d(d, ref, f'chain {dt}')
    assert info['sizes'].tolist() == sorted(er.CHAIN_SIZES) and not info['status'].any()
    assert (info['n_active'], info['n_components'], info['largest_component'], info['n_singular']) == \
        (int(active.sum()), len(er.CHAIN_SIZES), 300, 0)
    assert np.array_equal(info['row_size'].cpu().numpy(), ref['size'])
    # a chain of 300 rows in a random order: rounds of hooking and jumping, not of propagation (4 log2 K is generous)
    print(f'chain {dt}: {info["rounds"]} rounds')
    assert 1 <= info['rounds'] <= 4 * int(np.ceil(np.log2(len(d))))
    # vif: >= 1 inside the bar, exactly 1 for the row that is alone
    b = np.diag(case['G'])
    on = ref['size'] > 0
    assert np.all(b[on] * d[on] >= 1 - ref['bar'][on] - 8 * sr.taps_of(case['W']) * 2. ** -52)
    # the same bits again
    d2, info2 = be.inverse_diag_event_list(csr, active, 300)
    assert d2.cpu().numpy().tobytes() == d.tobytes() and info2['rounds'] == info['rounds']
    # a scratch that holds one tile of the largest component only: the components beyond the LDS go in two batches
    d3, _ = be.inverse_diag_event_list(csr, active, 300, scratch_doubles=300 * 300 + 300)
    assert d3.cpu().numpy().tobytes() == d.tobytes()


def test_the_components_and_their_lists():
    case, be, csr = chain_backend('f64')
    ref = case['ref']
    active = torch.from_numpy(case['strength'] > 0).cuda()
    comps = be.event_components(csr, active)
    start, member, local = (comps[k].cpu().numpy() for k in ('comp_start', 'member', 'local'))
    assert np.array_equal(np.diff(start), comps['sizes']) and start[0] == 0 and start[-1] == len(member)
    got = [member[a:b] for a, b in zip(start[:-1], start[1:])]
    assert len(got) == len(ref['groups']) and all(np.array_equal(g, r) for g, r in zip(got, ref['groups']))
    assert np.all(local[~(ref['size'] > 0)] == -1)
    assert all(np.array_equal(local[g], np.arange(len(g))) for g in got)
    # every row active: the bridges join the chain into one component
    everything = be.event_components(csr, torch.ones(len(local), dtype=torch.bool, device='cuda'))
    assert everything['sizes'].tolist() == [len(local)] and everything['rounds'] <= 4 * int(np.ceil(np.log2(len(local))))
    # no row active
    nothing = be.event_components(csr, torch.zeros(len(local), dtype=torch.bool, device='cuda'))
    assert nothing['sizes'].tolist() == [] and nothing['member'].numel() == 0 and nothing['comp_start'].tolist() == [0]
    d, info = be.inverse_diag_event_list(csr, torch.zeros(len(local), dtype=torch.bool, device='cuda'))
    assert np.all(np.isnan(d.cpu().numpy())) and info['n_components'] == 0


def test_the_cap_refuses_before_anything_is_written():
    case, be, csr = chain_backend('f64')
    active = torch.from_numpy(case['strength'] > 0).cuda()
    d = torch.full((len(case['strength']),), -7., dtype=torch.float64, device='cuda')
    with pytest.raises(ValueError, match=r'300 rows.*max_component=299'):
        be.inverse_diag_event_list(csr, active, 299, out=d)
    torch.cuda.synchronize()
    assert np.all(d.cpu().numpy() == -7.)
    be.inverse_diag_event_list(csr, active, 300, out=d)
    assert not np.any(d.cpu().numpy() == -7.), 'every element is written'


# -- 2. wrapped and mirrored occurrences, planes and samples ---------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', list(MODES) + ['taps-75'])
def test_the_mode_geometries(name, dt):
    """The four 2-D mode geometries of the Gram tests (rows of two samples at the same places among them) and the case of two
    samples and three planes with 75 taps; every third row is not active."""
    (N, C, P, D, A, mode), rows, W, V, G_ref, _ = gram_case(name)
    assert N == 2 and name in GEOMETRIES
    be = backend(N, C, P, D, A, mode, dt)
    csr = device_csr(be, W, dt, rows[:, 0], rows[:, 1], rows[:, 2:])
    # (every shift of a plane is in these lists: the whole block is far from well conditioned; a third of it is not)
    active = np.zeros(len(rows), dtype=bool)
    active[::3] = True
    ref = er.inverse_diag(G_ref, active, sr.taps_of(W))
    d, info = be.inverse_diag_event_list(csr, torch.from_numpy(active).cuda())
    d = d.cpu().numpy()
    print(f'{name} {dt}: sizes {info["sizes"].tolist()}, cond <= {np.nanmax(ref["kappa"]):.3g}')
    assert np.nanmax(ref['kappa']) <= 1e4
    check_d(d, ref, f'{name} {dt}')
    assert info['sizes'].tolist() == [len(g) for g in ref['groups']] and info['n_singular'] == 0
    comps =be.event_components(csr, torch.from_numpy(active).cuda())
    member, start = comps['member'].cpu().numpy(), comps['comp_start'].cpu().numpy()
    for a, b in zip(start[:-1], start[1:]):
        assert len(set(rows[member[a:b], 0])) == 1, 'rows of two samples never share a component'


# -- 3. event_errors and the front end ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('mode', MODES)
def test_detection_errors_on_the_device(mode, dt):
    case = sr.decoys(0, mode)
    nmf = hip_model(case['W'], case['V'], mode, dt)
    det = nmf.solve_detections(det_of(case), tol=1e-10)
    h = det.strength.astype(np.float64)
    on = h > 0
    assert np.any(~on) and np.any(on)
    G, c = sr.gram(case['V'], case['W'], mode, case['sample'], case['plane'], case['shift'])
    taps = sr.taps_of(case['W'])
    ref = er.inverse_diag(G, on, taps)
    state = (nmf.W.copy(), nmf.H.copy(), {f.name: np.array(getattr(det, f.name)) for f in dataclasses.fields(Detections)})
    stderr, vif = nmf.detection_errors(det, noise=0.5)
    info = nmf.errors_info_
    assert set(info) == INFO_KEYS and stderr.dtype == vif.dtype == np.float64 and stderr.shape == vif.shape == h.shape
    check_d((stderr / 0.5) ** 2, dict(ref, bar=ref['bar'] + 2. ** -50), f'front end {mode} {dt}')
    assert np.all(np.isnan(vif[~on])) and np.all(vif[on] >= 1 - ref['bar'][on]) and np.all(vif[ref['size'] == 1] == 1.)
    assert np.all(np.abs(vif[on] - np.diag(G)[on] * ref['d'][on]) <= (ref['bar'][on] + 8 * taps * 2. ** -52) * vif[on])
    assert (info['n_active'], info['n_components'], info['largest_component'], info['n_singular'], info['noise']) == \
        (int(on.sum()), len(ref['groups']), max(len(g) for g in ref['groups']), 0, 0.5)
    assert 1 <= info['rounds'] <= 4 * int(np.ceil(np.log2(len(h))))
    twice, vif2 = nmf.detection_errors(det, noise=1.)
    assert np.array_equal(twice[on], 2. * stderr[on]) and np.array_equal(vif2[on], vif[on])
    R = eref.render(case['W'], case['V'].shape[2:], case['V'].shape[0], mode, case['sample'], case['plane'], case['shift'], h)
    energy = float(np.sum((case['V'] - R) ** 2))
    est, _ = nmf.detection_errors(det)
    info = nmf.errors_info_
    bar = 16 * taps * 2. ** -52 * (np.sum(case['V'] ** 2) + 2 * c @ h + h @ G @ h)
    print(f'{mode} {dt}: residual energy {info["residual_energy"]:.9g}, reference {energy:.9g}, off by '
          f'{abs(info["residual_energy"] - energy):.3g}, bar {bar:.3g}')
    assert abs(info['residual_energy'] - energy) <= bar
    assert info['dof'] == case['V'].size - on.sum()
    assert np.allclose(est[on], info['noise'] * stderr[on] / 0.5, rtol=2. ** -50, atol=0)
    assert np.array_equal(state[0], nmf.W) and np.array_equal(state[1], nmf.H)
    assert all(np.array_equal(v, getattr(det, k)) for k, v in state[2].items())


def test_two_orientations_of_a_symmetric_atom_at_one_place_are_singular_on_the_device():
    W, V, det, twins = singular_case()
    nmf = hip_model(W, V, 'valid', 'f32', transforms='rot90')
    check_singular(nmf, det, twins, 'singular, device')


def test_refusals_on_the_device():
    case = sr.decoys(0, 'valid')
    nmf = hip_model(case['W'], case['V'], 'valid', 'f32')
    det = nmf.solve_detections(det_of(case))
    nmf.detection_errors(det)
    before = dict(nmf.errors_info_)
    largest = before['largest_component']
    with pytest.raises(ValueError, match=rf'{largest} rows.*max_component={largest - 1}'):
        nmf.detection_errors(det, max_component=largest - 1)
    for kw in (dict(noise=0.), dict(noise=float('nan')), dict(noise=True), dict(max_component=0), dict(max_component=1.5)):
        with pytest.raises(ValueError):
            nmf.detection_errors(det, **kw)
    twice = Detections(**{f.name: np.concatenate([getattr(det, f.name)[:3]] * 2) for f in dataclasses.fields(Detections)})
    with pytest.raises(ValueError, match='distinct'):
        nmf.detection_errors(twice)
    message = re.escape('detection_errors covers the plain Frobenius objective (beta_loss 2, no weights)')
    nmf._beta = 1.
    try:
        with pytest.raises(NotImplementedError, match=message):
            nmf.detection_errors(det)
    finally:
        nmf._beta = 2.
    assert nmf.errors_info_ == before
    V = np.random.default_rng(55).random((2, 1, 12, 14)).astype(np.float32) + 0.1
    np.random.seed(42)
    weighted = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend='hip')
    weighted.fit(V, n_iterations=2, weights=np.ones((2, 1, 1, 1), dtype=np.float32))
    some = weighted.detections(threshold=float(np.quantile(weighted.H, 0.9)))
    with pytest.raises(NotImplementedError, match=message):
        weighted.detection_errors(some)
    none = np.zeros(0, dtype=np.int64)
    with pytest.raises(NotImplementedError, match='event_errors is unweighted'):
        weighted._backend.event_errors(None, weighted._W, none, none, np.zeros((0, 2), dtype=np.int64), np.zeros(0))
    np.random.seed(42)
    vol = TransformInvariantNMF(n_atoms=1, atom_shape=(2, 2, 2), backend='hip')
    vol.fit(np.random.default_rng(3).random((1, 1, 5, 5, 5)).astype(np.float32), n_iterations=2)
    with pytest.raises(NotImplementedError, match='volumes'):
        vol.detection_errors(vol.detections(threshold=float(np.quantile(vol.H, 0.9)), min_distance=0))
    # an empty list
    empty = Detections(**{f.name: getattr(det, f.name)[:0] for f in dataclasses.fields(Detections)})
    stderr, vif = nmf.detection_errors(empty)
    assert stderr.shape == vif.shape == (0,) and nmf.errors_info_['n_components'] == 0


# -- 4. the entry's own refusals -----------------------------------------------------------------------------------------------------
def test_the_entry_refuses_bad_lists_before_anything_is_written():
    case, be, csr = chain_backend('f64')
    active = torch.from_numpy(case['strength'] > 0).cuda()
    comps = be.event_components(csr, active)
    K, sizes = len(case['strength']), comps['sizes']
    d = torch.full((K,), -7., dtype=torch.float64, device='cuda')
    status = torch.full((len(sizes),), -7, dtype=torch.int32, device='cuda')
    scratch = torch.empty(300 * 301, dtype=torch.float64, device='cuda')
    host = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))   # noqa: E731

    def call(sizes=sizes, n_comp=len(sizes), n_active=int(comps['member'].numel()), scratch_doubles=scratch.numel(),
             ctx=be._ctx, d=d):
        return be._lib.tnmf_hip_events_inverse_diag(ctx, K, csr[2].numel(), p(csr[0]), p(csr[1]), p(csr[2]), n_comp,
                                                    p(comps['comp_start']), host(sizes), n_active, p(comps['member']),
                                                    p(comps['local']), p(scratch), scratch_doubles, p(d), p(status), None)
    assert call(ctx=None) == -1 and call(d=None) == -1 and call(n_comp=-1) == -1 and call(scratch_doubles=-1) == -1
    assert call(sizes=np.ascontiguousarray(sizes[::-1])) == _lib.E_GEOM                 # not ascending
    assert call(n_active=int(comps['member'].numel()) - 1) == _lib.E_GEOM              # the sizes do not add up
    assert call(scratch_doubles=300 * 301 - 1) == _lib.E_GEOM                           # the largest tile does not fit
    torch.cuda.synchronize()
    assert np.all(d.cpu().numpy() == -7.) and np.all(status.cpu().numpy() == -7)
    assert call() == 0
    torch.cuda.synchronize()
    assert not np.any(d.cpu().numpy() == -7.) and not status.cpu().numpy().any()
