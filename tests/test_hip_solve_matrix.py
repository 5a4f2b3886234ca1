"""
The kernels of tnmf_amd/csrc/solve.hip, every branch of them: the cases of solve_dispatch.MATRIX (lists of events: the pairs,
the Gram matrix, the projection) and solve_dispatch.SYSTEMS (synthetic CSR systems: the five solver kernels and the host
loop) are chosen with the host mirror tests/solve_dispatch.py so that together they execute every named branch
(tests/test_solve_dispatch_cpu.py checks that without a GPU).  The stride case is sized from the CU count of the device the
test runs on, and the mirror is asked whether it strides there.

Pairs, Gram matrix and projection are EXACT: W and V are integers in 0..3, every G_ij and c_i an integer far below 2^53, the
double sums exact in any order -- row_start, col, val and c equal tests/solve_reference.py::gram_sparse bit for bit, and the
pairs are the mirror's, key for key.

The solver has no element type (doubles whatever the fit's) and is driven directly, through tnmf_hip_events_nnls and
HIP_Backend.nnls_event_list.  The systems are integers with L a power of two, so
  (a) max_iterations = 0: the projected start and its kkt are the reference's bit for bit;
  (b) max_iterations = 1 (beta = 0): max(x - (G x - c) / L, 0) bit for bit at every row, and the kkt of that iterate;
  (c) check_every = 1: the kkt history against solve_reference.nnls_iterates wherever the reference's kkt is at least 1e-6.
      The bar: two float64 evaluations of the reference that sum in different orders (CSR order against dense) diverge by at
      most 4.83e-11 relative over the cases (measured: tests/test_solve_dispatch_cpu.py prints it, solve_dispatch.
      ORDER_DIVERGENCE = 5e-11 holds it); the GPU's lane split and fused multiply-adds are a third order of the same sums, and
      100 times that, 5e-9, is allowed (solve_dispatch.KKT_HISTORY_BAR); the iterates, where one is compared, likewise (9.42e-16
      of the largest strength measured, ITERATE_BAR = 1e-13).  Every restart sum the reference meets is at least
      1e-6 of the sum of its terms' magnitudes (checked on the CPU), so no correct implementation restarts elsewhere;
  (d) to convergence: kkt of the returned h on the reference's matrix <= 2 * tol, and |h - h*| within the bound of
      tests/test_hip_events_solve.py's docstring with lambda_min >= 1 from Gershgorin.
"""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

import solve_dispatch as sd
import solve_reference as sr
from test_hip_events import DTYPES, dev, p
from test_hip_events_matrix import backend, device_cus
from tnmf_amd import _lib

pytestmark = pytest.mark.gpu

TOL = sd.TOL
LISTS = [name for name in sd.MATRIX if name != 'doctored']      # ('doctored' is 'zero-tap' with raw lists: the pairs test)


def case(name):
    return sd.matrix_case(name, device_cus())


@functools.lru_cache(maxsize=None)
def reference(name):
    """((row_start, col, val), c) of the case in float64 on this device's CU count, computed once."""
    geo, sample, plane, shift, W, V = case(name)
    csr, c = sr.gram_sparse(V, W, geo[5], sample, plane, shift)
    assert np.array_equal(csr[2], np.round(csr[2])) and csr[2].max() < 2 ** 40 and np.array_equal(c, np.round(c))
    for a in csr + (c,):
        a.setflags(write=False)
    return csr, c


def device_lists(name, dt):
    geo, sample, plane, shift, W, V = case(name)
    be = backend(*geo, dt)
    be._V_dev.copy_(dev(V, dt))
    s, pl, u, _ = be._check_events(geo[2], sample, plane, shift, np.ones(len(sample)))
    return be, dev(W, dt), be.event_list(s, pl, u)


@pytest.mark.parametrize('name', list(sd.MATRIX))
def test_the_case_reaches_its_branches_on_this_device(name):
    """What the case is there for, by the mirror, with the CU count of this device -- the stride case strides here."""
    cu = device_cus()
    geo, sample, plane, shift, W, _ = case(name)
    if name == 'stride':
        got = sd.reached(geo, sample, plane, shift, None, cu, walk=False)
    elif name == 'doctored':
        got = sd.reached(geo, sample, plane, shift, W, cu, lists=sd.doctored(cu)[:3])
    else:
        got = sd.reached(geo, sample, plane, shift, W, cu, capacity=sd.BALLOT_CAPACITY if name == 'ballot' else None)
    for kernel, names in sd.MATRIX[name][1].items():
        assert set(names) <= got[kernel], (name, kernel, cu, sorted(set(names) - got[kernel]))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', LISTS)
def test_gram_and_projection_of_integers_are_exact(name, dt):
    geo, sample, plane, shift, W, V = case(name)
    N, C, P, D, A, mode = geo
    K = len(sample)
    (row_start, col, val), c_ref = reference(name)
    be, Wd, (images, cell_start, events) = device_lists(name, dt)
    # the lists the kernels walk are the ones the mirror counted its runs on
    img, cs, ev = sd.lists_of(geo, sample, plane, shift)
    assert np.array_equal(images.cpu().numpy(), img) and np.array_equal(cell_start.cpu().numpy(), cs)
    assert np.array_equal(events.cpu().numpy(), ev)
    got = tuple(a.cpu().numpy() for a in be.gram_event_list(Wd, images, cell_start, events))
    c = be.project_event_list(Wd, events).cpu().numpy()
    assert got[2].dtype == np.float64 and c.dtype == np.float64
    assert np.array_equal(got[0], row_start) and np.array_equal(got[1], col), 'the diagonal and every non-zero of the reference'
    assert got[2].tobytes() == val.tobytes() and c.tobytes() == c_ref.tobytes(), 'bit for bit'
    row = np.repeat(np.arange(K), np.diff(got[0]))
    order = np.argsort(got[1].astype(np.int64) * K + row, kind='stable')
    assert np.array_equal(row[order], got[1]) and np.array_equal(got[1][order], row), 'the pattern is symmetric'
    assert got[2][order].tobytes() == got[2].tobytes(), 'bit-symmetric'
    assert np.all(sample[row] == sample[got[1]]), 'rows of different samples do not pair'
    # over poisoned outputs through the C ABI: every element is written, none is read
    upper = row <= got[1]
    ri, rj = (torch.from_numpy(a[upper].astype(np.int32)).cuda() for a in (row, got[1]))
    out = torch.full((int(upper.sum()),), float('nan'), dtype=torch.float64, device='cuda')
    c2 = torch.full((K,), float('nan'), dtype=torch.float64, device='cuda')
    g = _lib.make_geom(N, P, C, D, A, DTYPES.index(dt))
    assert be._lib.tnmf_hip_events_gram(be._ctx, ctypes.byref(g), _lib.MODES[mode], p(Wd), p(events), K, p(ri), p(rj),
                                        ri.numel(), p(out), None) == 0
    assert be._lib.tnmf_hip_events_project(be._ctx, ctypes.byref(g), _lib.MODES[mode], p(Wd), p(events), K, p(be._V_dev),
                                           p(c2), None) == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == val[upper].tobytes() and c2.cpu().numpy().tobytes() == c_ref.tobytes()
    # the same bits again, through the retry with the count
    again = tuple(a.cpu().numpy() for a in be.gram_event_list(Wd, images, cell_start, events, capacity=1))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    assert be.project_event_list(Wd, events).cpu().numpy().tobytes() == c.tobytes()
    if name == 'zero-tap':     # M4 / C4: the blank rows
        blank = sd.blank_rows(geo, plane, shift, W)
        diagonal = got[2][row == got[1]]
        assert blank.sum() == 2 and not diagonal[blank].any() and not c[blank].any() and np.all(diagonal[~blank] > 0)
        assert np.all(np.diff(got[0])[blank] == 1), 'a blank row holds its diagonal and nothing else'
        h, info = be.solve_events(None, Wd, sample, plane, shift, np.ones(K), TOL, 10000)
        h = h.cpu().numpy()
        assert info['converged'] and not h[blank].any() and h[~blank].any(), 'through solve_events a blank row ends at exactly 0'


def raw_pairs(be, geo, dt, images, cell_start, events, K, capacity, room):
    out = torch.full((room,), -7, dtype=torch.int64, device='cuda')
    count = torch.full((1,), 99, dtype=torch.int64, device='cuda')
    N, C, P, D, A, mode = geo
    g = _lib.make_geom(N, P, C, D, A, DTYPES.index(dt))
    assert be._lib.tnmf_hip_events_pairs(be._ctx, ctypes.byref(g), p(images), images.shape[0], p(cell_start), p(events), K,
                                         p(out), capacity, p(count), None) == 0
    torch.cuda.synchronize()
    return int(count.item()), out.cpu().numpy()


@pytest.mark.parametrize('name', [n for n in sd.MATRIX if n != 'stride'])
def test_the_pairs_are_the_mirrors_key_for_key(name):
    """tnmf_hip_events_pairs against the wave-by-wave mirror: the same keys, duplicates included (the order is free)."""
    dt = 'f32'
    geo, sample, plane, shift, W, V = case(name)
    K = len(sample)
    be, Wd, (images, cell_start, events) = device_lists(name, dt)
    lists = sd.lists_of(geo, sample, plane, shift)
    if name == 'doctored':
        lists = sd.doctored(device_cus())[:3]
        images, cell_start, events = (torch.from_numpy(a.astype(np.int32)).cuda().contiguous() for a in lists)
    want, groups, _ = sd.pairs_walk(geo, *lists, K)
    room = len(want) + 64
    count, keys = raw_pairs(be, geo, dt, images, cell_start, events, K, room, room)
    assert count == len(want) and np.array_equal(np.sort(keys[:count]), np.sort(want))
    assert np.all(keys[count:] == -7), 'nothing is written behind the count'
    count2, keys2 = raw_pairs(be, geo, dt, images, cell_start, events, K, room, room)
    assert count2 == count and np.array_equal(np.sort(keys2[:count]), np.sort(want))
    claims = sd.MATRIX[name][1].get('pairs', ())
    if 'P4:pair-through-several-image-pairs' in claims:
        assert count > len(np.unique(want))
    if 'P4:zero-valued-candidate' in claims:
        (row_start, col, val), _ = reference(name)
        held = set((np.repeat(np.arange(K), np.diff(row_start)) * K + col).tolist())
        dropped = [k for k in np.unique(keys[:count]).tolist() if k not in held]
        assert dropped, 'a candidate of the pairs that the CSR does not hold'
        csr = be.gram_event_list(Wd, images, cell_start, events)
        mine = set((np.repeat(np.arange(K), np.diff(csr[0].cpu().numpy())) * K + csr[1].cpu().numpy()).tolist())
        assert mine == held and not mine & set(dropped)
    if name == 'ballot':       # P5: the one ballot has four hits, the capacity falls inside it
        assert groups == [4]
        count, keys = raw_pairs(be, geo, dt, images, cell_start, events, K, sd.BALLOT_CAPACITY, 64)
        stored = keys[:sd.BALLOT_CAPACITY].tolist()
        assert count == 4, 'the count is the whole'
        assert len(set(stored)) == sd.BALLOT_CAPACITY and set(stored) <= set(want.tolist()), 'every stored key is a pair'
        assert np.all(keys[sd.BALLOT_CAPACITY:] == -7), 'nothing is written at or beyond the capacity'
    if name == 'doctored':     # P6: the pairs among the rows that were left alone are those of the undoctored lists
        clean = sd.doctored(device_cus())[3]
        whole, _, _ = sd.pairs_walk(geo, *sd.lists_of(geo, sample, plane, shift), K)

        def among(k):
            i, j = np.divmod(k, K)
            return np.sort(k[np.isin(i, clean) & np.isin(j, clean)])
        assert len(among(whole)) and np.array_equal(among(keys[:count]), among(whole))
        assert count < len(whole)


@pytest.mark.parametrize('dt', DTYPES)
def test_solve_events_on_the_stride_case(dt):
    """End to end on the list that strides: it converges, and kkt <= 2 * tol on the reference's matrix."""
    geo, sample, plane, shift, W, V = case('stride')
    be = backend(*geo, dt)
    be._V_dev.copy_(dev(V, dt))
    t = time.perf_counter()
    h, info = be.solve_events(None, dev(W, dt), sample, plane, shift, np.ones(len(sample)), TOL, 10000)
    h = h.cpu().numpy()
    csr, c = reference('stride')
    k = sr.nnls_iterates(csr, c, h, 0)[0][1]
    print(f'stride {dt}: K {len(sample)}, nnz {info["nnz"]}, {info["iterations"]} iterations, kkt {info["kkt"]:.3g}, '
          f'kkt_ref {k:.3g}, {time.perf_counter() - t:.2f} s')
    assert info['converged'] and info['kkt'] <= TOL and info['nnz'] == len(csr[1])
    assert np.all(h >= 0) and k <= 2 * TOL


# -- the solver ---------------------------------------------------------------------------------------------------------------
DIRECT = [name for name, spec in sd.SYSTEMS.items() if spec[3] == (400, 1, 401)]     # every system, once


@functools.lru_cache(maxsize=None)
def solver_backend(dt='f64'):
    return backend(1, 1, 1, (8, 8), (2, 2), 'valid', dt)


@functools.lru_cache(maxsize=None)
def device_system(name):
    s = sd.system_case(name)
    return (torch.from_numpy(s['row_start'].astype(np.int32)).cuda(), torch.from_numpy(s['col'].astype(np.int32)).cuda(),
            torch.from_numpy(np.array(s['val'])).cuda(), torch.from_numpy(np.array(s['c'])).cuda())


SENTINEL = -7.


def nnls(name, max_iterations, check_every=1, capacity='ample', with_count=True):
    """One tnmf_hip_events_nnls call on the case over a poisoned workspace -> (h, iterations, kkt, converged, n_history, the
    whole history buffer with four sentinel rows behind the capacity)."""
    s = sd.system_case(name)
    K = s['K']
    be = solver_backend()
    row_start, col, val, c = device_system(name)
    assert col.numel() == val.numel() >= s['nnz']
    h = torch.from_numpy(np.array(s['start'])).cuda()
    ws = torch.full((7 * K + 8,), float('nan'), dtype=torch.float64, device='cuda')
    cap = max_iterations // check_every + 2 if capacity == 'ample' else capacity
    history = np.full(((cap or 0) + 4, 2), SENTINEL)
    it, conv, nh, kkt = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_double(-1.)
    code = be._lib.tnmf_hip_events_nnls(
        be._ctx, K, s['nnz'], p(row_start), p(col), p(val), p(c), p(h), TOL, max_iterations, check_every, p(ws),
        ctypes.byref(it), ctypes.byref(kkt), ctypes.byref(conv),
        None if cap is None else history.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), cap or 0,
        ctypes.byref(nh) if with_count else None, None)
    torch.cuda.synchronize()
    assert code == 0
    return h.cpu().numpy(), it.value, kkt.value, bool(conv.value), nh.value, history


def bits(x):
    return np.asarray(x, dtype=np.float64).tobytes()


@pytest.mark.parametrize('name', DIRECT)
def test_the_start_and_the_first_step_bit_for_bit(name):
    """(a) and (b): on integers with L a power of two nothing rounds but the one division of kkt."""
    s = sd.system_case(name)
    its = sd.reference_iterates(name)
    h, it, kkt, conv, nh, history = nnls(name, 0)
    assert bits(h) == bits(its[0][0]), 'the projected start'
    assert it == 0 and kkt == its[0][1] and conv == (its[0][1] <= TOL) and nh == 1
    assert history[0].tolist() == [0., its[0][1]] and np.all(history[1:] == SENTINEL)
    h, it, kkt, conv, nh, history = nnls(name, 1)
    x0, x1 = its[0][0], its[1][0]
    wrong = np.flatnonzero(h != x1)
    assert bits(h) == bits(x1), (name, 'rows', wrong[:8].tolist(), h[wrong[:8]].tolist(), x1[wrong[:8]].tolist())
    assert np.array_equal(x1 * s['L'], np.round(x1 * s['L'])), 'multiples of 1 / L: the kkt of the first step is exact too'
    assert it == 1 and nh == 2 and history[:2].tolist() == [[0., its[0][1]], [1., its[1][1]]] and kkt == its[1][1]
    if s['empty'] is not None:                              # S5: a row without entries, from a positive start
        assert s['start'][s['empty']] > 0 and h[s['empty']] == 0. and x0[s['empty']] == 0.
    if name == 'starts':                                    # S5: NaN, negative, 0, positive; a diagonal of 0
        assert np.isnan(s['start'][[3, 60, 100]]).all() and np.all(s['start'][[4, 61, 256]] < 0)
        assert not x0[[3, 60, 100, 4, 61, 256, 7, 8]].any() and s['start'][8] > 0 and h[8] == 0.


@pytest.mark.parametrize('name', DIRECT)
def test_the_kkt_history_and_the_solution(name):
    """(c) and (d), and for the doctored matrix S6: the reference is nnls_iterates on what the clamps leave of it."""
    s = sd.system_case(name)
    K = s['K']
    its = sd.reference_iterates(name)
    n = len(its) - 2
    t = time.perf_counter()
    h, it, kkt, conv, nh, history = nnls(name, 400)
    seconds = time.perf_counter() - t
    assert conv and kkt <= TOL and abs(it - n) <= 1 and nh == it + 1
    assert np.array_equal(history[:nh, 0], np.arange(nh)) and history[nh - 1, 1] == kkt and np.all(history[nh:] == SENTINEL)
    m = min(n, it)
    want = np.array([x[1] for x in its[:m + 1]])
    big = want >= 1e-6
    err = np.max(np.abs(history[:m + 1, 1] - want)[big] / want[big])
    restarts = [k for k in range(n) if its[k][2]]
    print(f'{name}: K {K}, {it} iterations (reference {n}), restarts at {restarts}, kkt history against the reference '
          f'{err:.3g} relative over {int(big.sum())} checks, bar {sd.KKT_HISTORY_BAR:.3g}, {seconds:.3f} s')
    assert err <= sd.KKT_HISTORY_BAR
    # (d)
    csr = (s['row_start'], s['col'][:s['nnz']], s['val'][:s['nnz']])
    k = sr.nnls_iterates(csr, s['c'], h, 0)[0][1]
    star = its[n][0]
    assert np.all(h >= 0) and not np.isnan(h).any() and k <= 2 * TOL
    if name != 'doctored-csr':     # (what is left of a doctored matrix is not symmetric: no bound from Gershgorin)
        assert s['margin'] >= 1
        bound = np.sqrt(2 * TOL * np.max(np.abs(s['c'])) * (np.sum(h) + np.sum(star)) / s['margin'])
        print(f'{name}: |h - h*| {np.linalg.norm(h - star):.3g}, bound {bound:.3g}')
        assert np.linalg.norm(h - star) <= bound
    if K >= 15:
        x0 = its[0][0]
        assert np.any((h == 0) & (star == 0) & (x0 > 0)) and np.any((x0 == 0) & (h > 0))
    if s['empty'] is not None:
        assert h[s['empty']] == 0.
    h2, it2, kkt2, _, _, history2 = nnls(name, 400)
    assert bits(h2) == bits(h) and it2 == it and kkt2 == kkt and bits(history2) == bits(history), 'the same bits again'


@pytest.mark.parametrize('dt', DTYPES)
def test_the_backend_hook_on_the_large_system(dt):
    """HIP_Backend.nnls_event_list, the hook the drivers call, on K = 4137 with its own check_every = 10."""
    name = 'K-4137'
    s = sd.system_case(name)
    its = sd.reference_iterates(name)
    n = len(its) - 2
    be = solver_backend(dt)
    row_start, col, val, c = device_system(name)
    h, info = be.nnls_event_list((row_start, col, val), c, torch.from_numpy(np.array(s['start'])).cuda(), TOL, 400)
    h = h.cpu().numpy()
    assert info['converged'] and info['iterations'] % 10 == 0 and n <= info['iterations'] < n + 11
    assert info['history'][:, 0].tolist() == list(range(0, info['iterations'] + 1, 10)) and info['history'][0, 1] == its[0][1]
    assert sr.nnls_iterates((s['row_start'], s['col'], s['val']), s['c'], h, 0)[0][1] <= 2 * TOL
    bound = np.sqrt(2 * TOL * np.max(np.abs(s['c'])) * (np.sum(h) + np.sum(its[n][0])) / s['margin'])
    assert np.linalg.norm(h - its[n][0]) <= bound


def test_check_every_and_the_history_buffer():
    """S7."""
    # every 7 of 45 iterations into three pairs: checks at 0, 7, ..., 42 and 45; the buffer holds the first three
    name = 'every-7'
    its = sd.reference_iterates(name)
    max_iterations, every, capacity = sd.system_case(name)['params']
    assert len(its) - 2 > max_iterations and max_iterations % every and capacity < max_iterations // every + 2
    h, it, kkt, conv, nh, history = nnls(name, max_iterations, every, capacity)
    assert it == max_iterations and not conv and nh == capacity
    assert history[:capacity, 0].tolist() == [0., 7., 14.] and np.all(history[capacity:] == SENTINEL)
    for row in history[:capacity]:
        assert abs(row[1] - its[int(row[0])][1]) <= sd.KKT_HISTORY_BAR * its[int(row[0])][1]
    assert abs(kkt - its[max_iterations][1]) <= sd.KKT_HISTORY_BAR * its[max_iterations][1] and its[max_iterations][1] >= 1e-6
    x = its[max_iterations][0]
    assert np.max(np.abs(h - x)) <= sd.ITERATE_BAR * np.max(x), 'the iterate returned is the one the kkt belongs to'
    # a check_every above max_iterations, no history buffer, no count
    name = 'every-above'
    its = sd.reference_iterates(name)
    max_iterations, every, capacity = sd.system_case(name)['params']
    assert every > max_iterations and capacity is None
    h, it, kkt, conv, nh, history = nnls(name, max_iterations, every, None, with_count=False)
    assert it == max_iterations and not conv and nh == -1 and np.all(history == SENTINEL)
    assert abs(kkt - its[max_iterations][1]) <= sd.KKT_HISTORY_BAR * its[max_iterations][1]
    assert np.max(np.abs(h - its[max_iterations][0])) <= sd.ITERATE_BAR * np.max(its[max_iterations][0])
    h, it, kkt, conv, nh, history = nnls(name, max_iterations, every, None)
    assert nh == 0
    # no iterations, room for four pairs: one is stored
    h, it, kkt, conv, nh, history = nnls('no-iterations', 0, 1, 4)
    assert it == 0 and nh == 1 and np.all(history[1:] == SENTINEL) and kkt == sd.reference_iterates('no-iterations')[0][1]
