"""
Exact strengths of a list on the GPU: tnmf_hip_events_pairs / _gram / _project / _nnls through the C ABI and the backend's
hooks, and ``solve_detections`` on ``backend='hip'``, against tests/solve_reference.py in float64 on the same numbers.

The bars.  Gram matrix and projection: every term is non-negative for the non-negative W and V of these tests, so the sum of
the magnitudes is the value itself, and either side adds at most 4 * taps terms in double (the argument of
tests/test_hip_events_gain.py): |G - G_ref| <= 8 * taps * 2^-52 * G_ref entry by entry, likewise c.  Solver: it stops at
kkt <= tol on its own matrix, which differs from G_ref by that bar, orders below tol: kkt_ref <= 2 * tol.  One rounding of the
strengths to float32 moves g = Gh - c by at most 2^-24 * sum_j G_ij h_j: the front end's bar is tol + 2^-24 * max_i (G h)_i /
max |c|.  Two solutions of kkt <= tol: with r = tol * max |c|, E(h) <= E* + r |h|_1 for each and E(h) - E* >= lambda_min / 2 *
|h - h*|^2, so |h - h'| <= sqrt(2 r (|h|_1 + |h'|_1) / lambda_min).

Iterations of ``events_solve_numpy`` (float64, tol 1e-8) on the scenes used here, sr.decoys(0, mode): valid 120 / 130, full 90,
circular 90 / 80, reflect 180 / 190 from strengths 1 / from their own -- a margin of fifty to max_iterations = 10000.
"""
import ctypes
import dataclasses
import functools
import re

import numpy as np
import pytest
import torch

import events_reference as eref
import solve_reference as sr
from test_events_cpu import MODES
from test_hip_events import DTYPES, backend, dev, p
from test_hip_events_gain import events_of
from test_hip_pursuit import hip_model
from test_pursuit_cpu import NOISY_MIN_GAIN, key, model_of, noisy
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF

pytestmark = pytest.mark.gpu

TOL = 1e-8

# -- 1. Gram matrix and projection ------------------------------------------------------------------------------------------------
GEOMETRIES = {   # (N, C, P, D, A, mode)
    'valid': (2, 2, 3, (6, 7), (2, 3), 'valid'), 'full': (2, 2, 3, (6, 7), (2, 3), 'full'),
    'circular': (2, 2, 3, (6, 7), (2, 3), 'circular'), 'reflect': (2, 2, 3, (6, 7), (2, 3), 'reflect'),
    'taps-9': (2, 1, 3, (12, 14), (3, 3), 'reflect'),          # fewer taps than lanes
    'taps-75': (2, 3, 3, (12, 14), (5, 5), 'circular'),        # more than a wave's worth, not a multiple of it
    'wide-atom': (2, 1, 2, (20, 37), (3, 18), 'valid'),        # the reach of an image spans several 16 x 16 cells
    '1d-reflect': (2, 1, 2, (300,), (7,), 'reflect'),          # rows on both sides of the cell edge at 256
    '1d-circular': (2, 1, 2, (300,), (7,), 'circular'),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (geometry, distinct rows [K, 2 + k], W, V, G_ref, c_ref): float32-representable values, read-only."""
    geo = N, C, P, D, A, mode = GEOMETRIES[name]
    S = eref.shift_shape(D, A, mode)
    rng = np.random.default_rng(71)

    def random_rows(count):
        return [tuple(int(x) for x in r) for r in np.column_stack(
            [rng.integers(N, size=count), rng.integers(P, size=count)] + [rng.integers(s, size=count) for s in S])]
    if name in MODES:      # every shift of two planes of one sample, 20 random rows over both samples
        rows = [(0, pl) + u for pl in (0, 2) for u in np.ndindex(*S)] + random_rows(20)
        rows += [(1,) + r[1:] for r in rows[5:8]]                       # the same place in the other sample
    elif name.startswith('1d'):
        rows = [(n, pl, u) for n in (0, 1) for pl in (0, 1) for u in range(238, 262, 3 - n)]   # padded 244 .. 267
        rows += [(0, 0, u) for u in (0, 1, 2, 6, 293, 296, 299)] + random_rows(30)
    else:
        rows = random_rows(80)
    rows = np.array(sorted(set(rows)), dtype=np.int64)
    rows = rows[rng.permutation(len(rows))]
    W = (rng.random((P, C) + A) + 0.1).astype(np.float32).astype(np.float64)
    V = (rng.random((N, C) + D) * 3.).astype(np.float32).astype(np.float64)
    G, c = sr.gram(V, W, mode, rows[:, 0], rows[:, 1], rows[:, 2:])
    for a in (rows, W, V, G, c):
        a.setflags(write=False)
    return geo, rows, W, V, G, c


def device_gram(name, dt, capacity=None):
    """-> (CSR triple, c) as numpy, of the case on the backend's hooks; the first pairs call with ``capacity``."""
    (N, C, P, D, A, mode), rows, W, V, _, _ = case(name)
    be = backend(N, C, P, D, A, mode, dt)
    be._V_dev.copy_(dev(V, dt))
    Wd = dev(W, dt)
    s, pl, u, _ = be._check_events(P, rows[:, 0], rows[:, 1], rows[:, 2:], np.ones(len(rows)))
    images, cell_start, events = be.event_list(s, pl, u)
    csr = be.gram_event_list(Wd, images, cell_start, events, capacity=capacity)
    c = be.project_event_list(Wd, events)
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in csr), c.cpu().numpy()


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', list(GEOMETRIES))
def test_gram_and_projection_against_the_reference(name, dt):
    geo, rows, W, V, G_ref, c_ref = case(name)
    K, taps = len(rows), sr.taps_of(W)
    csr, c = device_gram(name, dt, capacity=1)       # (the first call does not fit: the retry with the count)
    G, present = sr.densify(K, *csr)
    bar = 8 * taps * 2. ** -52
    live = G_ref > 0
    print(f'{name} {dt}: K {K}, nnz {len(csr[1])} (reference {np.count_nonzero(G_ref)}), |G - ref| / ref <= '
          f'{np.max(np.abs(G - G_ref)[live] / G_ref[live]):.3g}, |c - ref| / ref <= '
          f'{np.max(np.abs(c - c_ref)[c_ref > 0] / c_ref[c_ref > 0]):.3g}, bar {bar:.3g}')
    assert np.all(np.abs(G - G_ref) <= bar * G_ref)
    assert np.all(np.abs(c - c_ref) <= bar * c_ref)
    assert np.all(present[G_ref != 0]), 'every entry of the reference that is not 0 is present'
    assert G.tobytes() == G.T.copy().tobytes(), 'bit-symmetric'
    other = rows[:, 0][:, None] != rows[:, 0][None, :]
    assert not present[other].any(), 'rows of different samples do not pair'
    csr2, c2 = device_gram(name, dt)                  # the same bits again, whatever the capacity
    assert all(a.tobytes() == b.tobytes() for a, b in zip(csr, csr2)) and c.tobytes() == c2.tobytes()


def test_the_cases_reach_what_they_are_for():
    for name in MODES:
        (N, C, P, D, A, mode), rows, _, _, G, _ = case(name)
        S = eref.shift_shape(D, A, mode)
        assert len(rows) >= 2 * int(np.prod(S)) + 10 and (np.diag(G) > 0).all()
        assert len(np.unique(rows[:, 1:], axis=0)) < len(rows), 'rows of both samples at the same place'
    # 1-D: close rows whose padded positions lie on both sides of 256
    _, rows, _, _, _, _ = case('1d-circular')
    q = rows[:, 2] + 6
    assert np.any((q[:, None] < 256) & (q[None, :] >= 256) & (np.abs(q[:, None] - q[None, :]) < 7))
    assert [sr.taps_of(case(n)[2]) for n in ('taps-9', 'taps-75')] == [9, 75]


def raw_pairs(geo, rows, dt, capacity):
    """-> (code, count, the stored keys) of one tnmf_hip_events_pairs call on a poisoned output."""
    N, C, P, D, A, mode = geo
    be = backend(N, C, P, D, A, mode, dt)
    s, pl, u, _ = be._check_events(P, rows[:, 0], rows[:, 1], rows[:, 2:], np.ones(len(rows)))
    images, cell_start, events = be.event_list(s, pl, u)
    assert capacity <= 64 or capacity >= 2 ** 31      # (what is not refused fits the 64 slots)
    out = torch.full((64,), -7, dtype=torch.int64, device='cuda')
    count = torch.full((1,), 99, dtype=torch.int64, device='cuda')
    g = _lib.make_geom(N, P, C, D, A, DTYPES.index(dt))
    code = be._lib.tnmf_hip_events_pairs(be._ctx, ctypes.byref(g), p(images), images.shape[0], p(cell_start), p(events),
                                         len(rows), p(out), capacity, p(count), None)
    torch.cuda.synchronize()
    return code, int(count.item()), out.cpu().numpy()


def test_pairs_at_offset_a_minus_one_and_not_at_a_and_the_capacity_contract():
    geo = N, C, P, D, A, mode = GEOMETRIES['wide-atom']
    rows = np.array([(0, 0, 5, 3), (0, 1, 5, 3 + A[1] - 1), (0, 0, 5, 3 + A[1]), (0, 1, 5 + A[0] - 1, 3), (0, 1, 5 + A[0], 3),
                     (1, 0, 5, 3)], dtype=np.int64)
    code, count, keys = raw_pairs(geo, rows, 'f32', 64)
    assert code == 0
    K = len(rows)
    found = sorted(set(divmod(int(x), K) for x in keys[:count]))
    want = sorted((i, j) for i in range(K) for j in range(i + 1, K) if rows[i, 0] == rows[j, 0]
                  and abs(rows[i, 2] - rows[j, 2]) < A[0] and abs(rows[i, 3] - rows[j, 3]) < A[1])
    assert found == want and (0, 1) in want and (0, 2) not in want and (0, 3) in want and (0, 4) not in want
    assert np.all(keys[count:] == -7)
    # a capacity below the count: the count is the whole, nothing is written beyond the capacity
    code, count2, keys = raw_pairs(geo, rows, 'f32', 2)
    assert code == 0 and count2 == count and np.all(keys[:2] >= 0)
    code, count3, keys = raw_pairs(geo, rows, 'f32', 0)
    assert code == 0 and count3 == count and keys[0] == -7
    # more than 2^31 - 1 stored entries: refused before anything is written
    code, count4, keys = raw_pairs(geo, rows, 'f32', 2 ** 31)
    assert code == _lib.E_UNSUPPORTED and count4 == 99 and keys[0] == -7


@pytest.mark.parametrize('dt', DTYPES)
def test_rows_outside_the_contract_get_zero(dt):
    (N, C, P, D, A, mode), rows, W, V, G_ref, c_ref = case('reflect')
    S = eref.shift_shape(D, A, mode)
    be = backend(N, C, P, D, A, mode, dt)
    be._V_dev.copy_(dev(V, dt))
    rows = np.array(rows[:12])
    bad = {2: (0, N), 4: (1, -1), 6: (2, S[0]), 8: (3, -3)}
    for e, (column, value) in bad.items():
        rows[e, column] = value
    ev, K = events_of(rows, 2), len(rows)
    ri = torch.tensor([0, 1, 2, 0, 4, 6, 8, 3, 0, -1, 5], dtype=torch.int32, device='cuda')
    rj = torch.tensor([0, 1, 2, 2, 5, 6, 9, 8, K, 3, 7], dtype=torch.int32, device='cuda')
    val = torch.full((len(ri),), float('nan'), dtype=torch.float64, device='cuda')
    c = torch.full((K,), float('nan'), dtype=torch.float64, device='cuda')
    g = _lib.make_geom(N, P, C, D, A, DTYPES.index(dt))
    Wd = dev(W, dt)
    assert be._lib.tnmf_hip_events_gram(be._ctx, ctypes.byref(g), _lib.MODES[mode], p(Wd), p(ev), K, p(ri), p(rj), len(ri),
                                        p(val), None) == 0
    assert be._lib.tnmf_hip_events_project(be._ctx, ctypes.byref(g), _lib.MODES[mode], p(Wd), p(ev), K, p(be._V_dev), p(c),
                                           None) == 0
    torch.cuda.synchronize()
    val, c = val.cpu().numpy(), c.cpu().numpy()
    good = np.array([i not in bad for i in range(K)])
    assert not np.isnan(val).any() and not np.isnan(c).any(), 'every element is written'
    assert not c[~good].any() and np.all(c[good] > 0)
    bar = 8 * sr.taps_of(W) * 2. ** -52
    for k, (i, j) in enumerate(zip(ri.tolist(), rj.tolist())):
        if 0 <= i < K and 0 <= j < K and good[i] and good[j]:
            assert abs(val[k] - G_ref[i, j]) <= bar * G_ref[i, j]
        else:
            assert val[k] == 0.
    assert val[0] > 0


# -- 2. the solver through the backend hook ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(mode):
    s = sr.decoys(0, mode)
    G, c = sr.gram(s['V'], s['W'], mode, s['sample'], s['plane'], s['shift'])
    lam = np.linalg.eigvalsh(G)
    own = np.array(s['strength'])
    own[np.flatnonzero(s['true'])[::2]] = 0.         # planted rows that start at 0
    for a in (G, c, own):
        a.setflags(write=False)
    return s, G, c, own, float(lam[0]), float(lam[-1])


def solve(mode, dt, start):
    s, _, _, _, _, _ = scene(mode)
    N, C = s['V'].shape[:2]
    P, A, D = s['W'].shape[0], s['W'].shape[2:], s['V'].shape[2:]
    be = backend(N, C, P, D, A, mode, dt)
    be._V_dev.copy_(dev(s['V'], dt))
    h, info = be.solve_events(None, dev(s['W'], dt), s['sample'], s['plane'], s['shift'], start, TOL, 10000)
    assert h.dtype == torch.float64 and h.is_cuda
    return h.cpu().numpy(), info


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('mode', MODES)
def test_the_solver_reaches_the_kkt_conditions_of_the_reference(mode, dt):
    s, G, c, own, lam_min, lam_max = scene(mode)
    K = len(c)
    h, info = solve(mode, dt, own)
    k = sr.kkt(G, c, h)
    print(f'{mode} {dt}: K {K}, nnz {info["nnz"]}, {info["iterations"]} iterations, kkt {info["kkt"]:.3g}, '
          f'kkt_ref {k:.3g}, cond {lam_max / lam_min:.3g}')
    assert info['converged'] and info['iterations'] <= 1000 and info['kkt'] <= TOL
    assert np.all(h >= 0) and k <= 2 * TOL
    assert np.any((own == 0) & (h > 0)), 'a row that starts at 0 ends positive'
    assert np.any(h == 0), 'a row ends at exactly 0'
    history = info['history']
    assert history.shape[1] == 2 and history[0, 0] == 0 and history[-1, 0] == info['iterations']
    assert history[-1, 1] == info['kkt'] and np.all(np.diff(history[:, 0]) == 10)
    # info against a recomputation: the two evaluations of g_i = sum_j G_ij h_j - c_i differ by the rounding of at most
    # K + 1 terms each
    scale = np.max(np.abs(G) @ h + np.abs(c)) / np.max(np.abs(c))
    assert abs(info['kkt'] - k) <= 2 * (K + 2) * 2. ** -53 * scale + 8 * sr.taps_of(s['W']) * 2. ** -52 * scale
    # the same bits again
    h2, info2 = solve(mode, dt, own)
    assert h2.tobytes() == h.tobytes() and info2['iterations'] == info['iterations'] and info2['kkt'] == info['kkt']
    # the start does not matter
    assert lam_min >= 1e-6 * lam_max
    h1, info1 = solve(mode, dt, np.ones(K))
    assert info1['converged'] and sr.kkt(G, c, h1) <= 2 * TOL
    bound = np.sqrt(2 * TOL * np.max(np.abs(c)) * (np.sum(h) + np.sum(h1)) / lam_min)
    print(f'{mode} {dt}: from ones {info1["iterations"]} iterations, |h - h1| {np.max(np.abs(h - h1)):.3g}, bound {bound:.3g}')
    assert np.linalg.norm(h - h1) <= bound


def test_zero_iterations_blank_data_and_bad_arguments_of_the_solver():
    s, G, c, own, _, _ = scene('valid')
    N, C = s['V'].shape[:2]
    be = backend(N, C, s['W'].shape[0], s['V'].shape[2:], s['W'].shape[2:], 'valid', 'f64')
    be._V_dev.copy_(dev(s['V'], 'f64'))
    Wd = dev(s['W'], 'f64')
    h, info = be.solve_events(None, Wd, s['sample'], s['plane'], s['shift'], own, TOL, 0)
    assert np.array_equal(h.cpu().numpy(), own) and info['iterations'] == 0 and not info['converged']
    assert info['kkt'] == pytest.approx(sr.kkt(G, c, own), rel=1e-9)
    h, info = be.solve_events(None, Wd, s['sample'], s['plane'], s['shift'], own, TOL, 13)
    assert info['iterations'] == 13 and info['history'][:, 0].tolist() == [0, 10, 13]
    assert info['kkt'] == pytest.approx(sr.kkt(G, c, h.cpu().numpy()), rel=1e-6)
    be._V_dev.zero_()          # max |c| = 0: the answer is 0 with kkt = 0
    h, info = be.solve_events(None, Wd, s['sample'], s['plane'], s['shift'], own, TOL, 100)
    assert not h.cpu().numpy().any() and info['kkt'] == 0. and info['converged'] and info['iterations'] == 0
    be._V_dev.copy_(dev(s['V'], 'f64'))
    one, out = torch.zeros(8, dtype=torch.float64, device='cuda'), (ctypes.c_int(5), ctypes.c_double(5.), ctypes.c_int(5))
    zero = torch.zeros(2, dtype=torch.int32, device='cuda')
    for tol, iters, every, code in ((0., 10, 10, _lib.E_UNSUPPORTED), (float('nan'), 10, 10, _lib.E_UNSUPPORTED),
                                    (1e-8, -1, 10, _lib.E_GEOM), (1e-8, 10, 0, _lib.E_GEOM)):
        assert be._lib.tnmf_hip_events_nnls(be._ctx, 1, 1, p(zero), p(zero), p(one), p(one), p(one), tol, iters, every,
                                            p(torch.zeros(15, dtype=torch.float64, device='cuda')), ctypes.byref(out[0]),
                                            ctypes.byref(out[1]), ctypes.byref(out[2]), None, 0, None, None) == code
        assert out[0].value == 5 and out[2].value == 5


def test_an_empty_list_through_the_hooks():
    s, _, _, _, _, _ = scene('valid')
    N, C = s['V'].shape[:2]
    be = backend(N, C, s['W'].shape[0], s['V'].shape[2:], s['W'].shape[2:], 'valid', 'f32')
    Wd = dev(s['W'], 'f32')
    none = np.zeros(0, dtype=np.int64)
    sample, plane, shift, _ = be._check_events(Wd.shape[0], none, none, np.zeros((0, 2), dtype=np.int64), np.zeros(0))
    images, cell_start, events = be.event_list(sample, plane, shift)
    row_start, col, val = be.gram_event_list(Wd, images, cell_start, events)
    assert row_start.tolist() == [0] and col.numel() == 0 and val.numel() == 0
    assert be.project_event_list(Wd, events).numel() == 0
    h, info = be.solve_events(None, Wd, none, none, np.zeros((0, 2), dtype=np.int64), np.zeros(0), TOL, 100)
    torch.cuda.synchronize()
    assert h.numel() == 0 and h.dtype == torch.float64
    assert info['iterations'] == 0 and info['converged'] and info['kkt'] == 0. and info['nnz'] == 0
    assert info['history'].shape == (0, 2)


# -- 3. the front end ------------------------------------------------------------------------------------------------------------
def frontend_reference(nmf, det):
    W_eff = nmf.transformed_atoms.astype(np.float64).reshape((-1,) + nmf.W.shape[1:]) if nmf.transforms is not None \
        else nmf.W.astype(np.float64)
    V = nmf.V.astype(np.float64)
    mode = nmf._backend._reconstruction_mode
    return V, sr.gram(V, W_eff, mode, det.sample, det.atom * nmf.n_transforms + det.transform, det.shift)


@pytest.mark.parametrize('transforms', [None, 'rot90'])
def test_solve_detections_on_a_fitted_model(transforms):
    rng = np.random.default_rng(5)
    V = (rng.random((2, 1, 16, 18)) ** 3).astype(np.float32)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(4, 4), backend='hip', transforms=transforms)
    nmf.fit(V, n_iterations=30, sparsity_H=0.05)
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.95)))
    assert 20 <= len(det) <= 600
    V64, (G, c) = frontend_reference(nmf, det)
    solved = nmf.solve_detections(det, tol=TOL)
    h = solved.strength
    assert h.dtype == np.float32 and nmf.solve_converged_ and key(solved) == key(det)
    h = h.astype(np.float64)
    k, cmax = sr.kkt(G, c, h), np.max(np.abs(c))
    bar = TOL + 2. ** -24 * np.max(G @ h) / cmax
    print(f'{transforms}: K {len(det)}, {nmf.solve_n_iter_} iterations, kkt_ref {k:.3g}, bar {bar:.3g}')
    assert np.all(h >= 0) and k <= bar
    E = sr.objective(V64, G, c, h)
    mu50 = nmf.refit_detections(det, n_iterations=50).strength.astype(np.float64)
    mu5000 = nmf.refit_detections(det, n_iterations=5000).strength.astype(np.float64)
    E50, E5000 = sr.objective(V64, G, c, mu50), sr.objective(V64, G, c, mu5000)
    slack = k * cmax * (np.sum(h) + np.sum(mu5000))
    print(f'{transforms}: E solve {E:.8g}, 50 MU {E50:.8g}, 5000 MU {E5000:.8g}, slack {slack:.3g}')
    assert E <= E50 and E <= E5000 + slack


@pytest.mark.parametrize('mode', MODES)
def test_pursuit_with_solve_on_the_noisy_scene(mode):
    scene_, _ = noisy(0, mode)
    W, V, t = scene_['W'], scene_['V'], scene_['true']
    nmf = hip_model(W, V, mode, 'f32')
    mu, _ = nmf.pursue_detections(NOISY_MIN_GAIN)
    det, gains = nmf.pursue_detections(NOISY_MIN_GAIN, strengths='solve', tol=TOL)
    rounds = nmf.pursuit_history_[:, 1].copy()
    assert nmf.solve_converged_
    planted = set(map(tuple, np.column_stack([scene_['sample'][t], scene_['plane'][t], np.zeros(t.sum(), dtype=int),
                                              scene_['shift'][t]]).tolist()))
    assert planted <= set(key(det))
    G, c = sr.gram(V, W, mode, det.sample, det.atom, det.shift)
    Gm, cm = sr.gram(V, W, mode, mu.sample, mu.atom, mu.shift)
    h, hm = det.strength.astype(np.float64), mu.strength.astype(np.float64)
    k, cmax = sr.kkt(G, c, h), np.max(np.abs(c))
    assert k <= TOL + 2. ** -24 * np.max(G @ h) / cmax
    E, Emu = sr.objective(V, G, c, h), sr.objective(V, Gm, cm, hm)
    print(f'{mode}: {len(det)} rows (mu {len(mu)}), E solve {E:.8g}, mu {Emu:.8g}, kkt_ref {k:.3g}')
    assert E <= Emu + k * cmax * (np.sum(h) + np.sum(hm))
    host = model_of(W, V, mode, dtype=np.float32)
    host_det, _ = host.pursue_detections(NOISY_MIN_GAIN, strengths='solve', tol=TOL)
    assert np.array_equal(host.pursuit_history_[:, 1], rounds) and key(host_det) == key(det)


def test_refusals_come_before_any_output_changes():
    scene_, _ = noisy(0, 'valid')
    nmf = hip_model(scene_['W'], scene_['V'], 'valid', 'f32')
    det, _ = nmf.pursue_detections(NOISY_MIN_GAIN, strengths='solve')
    before = (nmf.solve_history_.copy(), nmf.solve_n_iter_, nmf.solve_converged_, nmf.pursuit_history_.copy())

    def unchanged():
        return (np.array_equal(before[0], nmf.solve_history_) and before[1:3] == (nmf.solve_n_iter_, nmf.solve_converged_)
                and np.array_equal(before[3], nmf.pursuit_history_))
    twice = Detections(**{f.name: np.concatenate([getattr(det, f.name)[:3]] * 2) for f in dataclasses.fields(Detections)})
    with pytest.raises(ValueError, match='distinct'):
        nmf.solve_detections(twice)
    for kw in (dict(tol=0.), dict(tol=float('nan')), dict(tol=-1.), dict(max_iterations=-1), dict(max_iterations=1.5)):
        with pytest.raises(ValueError):
            nmf.solve_detections(det, **kw)
        with pytest.raises(ValueError):
            nmf.pursue_detections(NOISY_MIN_GAIN, strengths='solve', **kw)
    for driver in (lambda **k: nmf.prune_detections(det, 0.01, **k), lambda **k: nmf.pursue_detections(0.01, **k),
                   lambda **k: nmf.relocate_detections(det, **k)):
        with pytest.raises(ValueError, match='sparsity_H must be 0'):
            driver(strengths='solve', sparsity_H=0.1)
    message = re.escape('solve_detections covers the plain Frobenius objective (beta_loss 2, no weights)')
    nmf._beta = 1.
    try:
        with pytest.raises(NotImplementedError, match=message):
            nmf.solve_detections(det)
    finally:
        nmf._beta = 2.
    assert unchanged()
    # a weighted fit: the front end and the hook both refuse
    V = np.random.default_rng(55).random((2, 1, 12, 14)).astype(np.float32) + 0.1
    np.random.seed(42)
    weighted = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend='hip')
    weighted.fit(V, n_iterations=2, weights=np.ones((2, 1, 1, 1), dtype=np.float32))
    some = weighted.detections(threshold=float(np.quantile(weighted.H, 0.9)))
    with pytest.raises(NotImplementedError, match=message):
        weighted.solve_detections(some)
    none = np.zeros(0, dtype=np.int64)
    with pytest.raises(NotImplementedError):
        weighted._backend.solve_events(None, weighted._W, none, none, np.zeros((0, 2), dtype=np.int64), np.zeros(0), TOL, 10)
    # volumes
    np.random.seed(42)
    vol = TransformInvariantNMF(n_atoms=1, atom_shape=(2, 2, 2), backend='hip')
    vol.fit(np.random.default_rng(3).random((1, 1, 5, 5, 5)).astype(np.float32), n_iterations=2)
    with pytest.raises(NotImplementedError, match='volumes'):
        vol.solve_detections(vol.detections(threshold=float(np.quantile(vol.H, 0.9)), min_distance=0))
    with pytest.raises(NotImplementedError):
        vol._backend.solve_events(None, vol._W, [0], [0], [[0, 0, 0]], [1.], TOL, 10)
