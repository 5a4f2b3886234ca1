"""
CPU guard of the solve kernel matrix: the host mirror of the nine kernels of tnmf_amd/csrc/solve.hip and of the host loop
events_nnls (tests/solve_dispatch.py) is held to the sources it restates, the cases of tests/test_hip_solve_matrix.py are held
to executing every named branch, each item of the list the matrix was built for (P1-P6, M1-M4, C1-C4, S1-S7) through a case
named for it, and the additions to tests/solve_reference.py are held to the dense reference and to the host solver.  The
conditions under which the GPU test's bars are valid are checked here on the reference alone.  No GPU, no build: the sources
are read as text.
"""
import os
import re

import numpy as np
import pytest

import events_dispatch as ed
import events_reference as eref
import solve_dispatch as sd
import solve_reference as sr
from conftest import ROOT
from tnmf_amd import events_host

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')
SMALL = [name for name in sd.MATRIX if name != 'stride']

# the geometries of tests/test_hip_events_solve.py::GEOMETRIES (that module needs a GPU to import; the guard reads it as text)
OLD_GEOMETRIES = {
    'valid': (2, 2, 3, (6, 7), (2, 3), 'valid'), 'full': (2, 2, 3, (6, 7), (2, 3), 'full'),
    'circular': (2, 2, 3, (6, 7), (2, 3), 'circular'), 'reflect': (2, 2, 3, (6, 7), (2, 3), 'reflect'),
    'taps-9': (2, 1, 3, (12, 14), (3, 3), 'reflect'), 'taps-75': (2, 3, 3, (12, 14), (5, 5), 'circular'),
    'wide-atom': (2, 1, 2, (20, 37), (3, 18), 'valid'), '1d-reflect': (2, 1, 2, (300,), (7,), 'reflect'),
    '1d-circular': (2, 1, 2, (300,), (7,), 'circular'),
}


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


# -- the mirror against the sources ---------------------------------------------------------------------------------------------
def test_constants_are_those_of_the_sources():
    solve, events_h = _read(CSRC, 'solve.hip'), _read(CSRC, 'events.h')
    assert sd.THREADS == int(re.search(r'constexpr int kEventThreads = (\d+);', events_h).group(1))
    assert 'constexpr int kWaves = kEventThreads / 64;' in solve and sd.WAVES == sd.THREADS // 64
    assert sd.ROW_LANES == int(re.search(r'constexpr int kRowLanes = (\d+);', solve).group(1))
    assert 'constexpr int kRowsPerBlock = kEventThreads / kRowLanes;' in solve
    assert sd.ROWS_PER_BLOCK == sd.THREADS // sd.ROW_LANES == 16
    assert 'inline unsigned events_grid(const tnmf_hip_ctx *ctx, long long blocks, int per_cu = 64) {' in events_h
    assert 'return (unsigned)std::max<long long>(1, std::min<long long>(blocks, (long long)ctx->num_cu * per_cu));' in events_h
    assert sd.grid_for is ed.grid_for and sd.grid_for(10 ** 9, 7) == 7 * 64 and sd.grid_for(0) == 1
    assert 'long long events_nnls_workspace(long long n_rows) { return 7 * n_rows + kScalars; }' in solve
    assert 'kScalars = 8 }' in solve and 'ws = torch.empty(7 * K + 8, dtype=torch.float64' in _read('tnmf_amd', 'backends', 'HIP.py')
    geometries = re.search(r'GEOMETRIES = \{.*?\n\}', _read('tests', 'test_hip_events_solve.py'), re.S).group(0)
    for name, geo in OLD_GEOMETRIES.items():
        assert f"'{name}': {geo!r}" in geometries, name
    assert geometries.count("':") == len(OLD_GEOMETRIES)


def test_mirrored_rules_are_those_of_the_sources():
    """The lines the mirror restates.  When one of them changes, tests/solve_dispatch.py and the cases of the two matrices
    have to be looked at again."""
    src = _read(CSRC, 'solve.hip')
    for line in ('for (long long a = (long long)blockIdx.x * kWaves + wave; a < n_images; a += (long long)gridDim.x * kWaves) {',
                 'if ((unsigned)me.w >= (unsigned)K || me.y < 0 || me.z < 0) continue;',
                 'const int cy = me.y / g.ty, cx = me.z / g.tx;',
                 'if (cy >= g.ncy || cx >= g.ncx) continue;',
                 'if ((unsigned long long)n >= (unsigned long long)g.N) continue;',
                 'const int cy0 = max((me.y - (g.Ay - 1)) / g.ty, 0), cy1 = min((me.y + g.Ay - 1) / g.ty, g.ncy - 1);',
                 'const int cx0 = max((me.z - (g.Ax - 1)) / g.tx, 0), cx1 = min((me.z + g.Ax - 1) / g.tx, g.ncx - 1);',
                 'for (int ry = cy0; ry <= cy1; ++ry) {',
                 'const long long row = (n * g.ncy + ry) * g.ncx;',
                 'const int i0 = max(cell_start[row + cx0], 0), i1 = min(cell_start[row + cx1 + 1], n_images);',
                 'for (int base = i0; base < i1; base += 64) {',
                 'hit = (unsigned)im.w < (unsigned)K && im.w > me.w && abs(im.y - me.y) < g.Ay && abs(im.z - me.z) < g.Ax;',
                 'if (!m) continue;',
                 'if (slot < capacity) pairs[slot] = (long long)me.w * K + other;',
                 'for (long long p = (long long)blockIdx.x * kWaves + wave; p < n_pairs; p += (long long)gridDim.x * kWaves) {',
                 'for (long long e = (long long)blockIdx.x * kWaves + wave; e < n_events; e += (long long)gridDim.x * kWaves) {',
                 # (events_grid of events.h with its default per_cu = 64: test_constants_are_those_of_the_sources)
                 'const unsigned grid = events_grid(ctx, (n_images + kWaves - 1) / kWaves);',
                 'const unsigned grid = events_grid(ctx, (n_pairs + kWaves - 1) / kWaves);',
                 'const unsigned grid = events_grid(ctx, (n_events + kWaves - 1) / kWaves);',
                 # the solver
                 '*a = min(max(row_start[i], 0), nnz);',
                 '*b = min(max(row_start[i + 1], *a), nnz);',
                 'const int i = blockIdx.x * kRowsPerBlock + threadIdx.x / kRowLanes;',
                 'for (int k = a + sub; k < b; k += kRowLanes) {',
                 'if ((unsigned)j >= (unsigned)K) continue;',
                 'if (i < K && sub == 0) rowabs[i] = s, act[i] = d > 0. ? 1. : 0.;',
                 'for (int i = threadIdx.x; i < K; i += kEventThreads) L = fmax(L, rowabs[i]), cm = fmax(cm, fabs(c[i]));',
                 'scal[kInvL] = s_a[0] > 0. ? 1. / s_a[0] : 0.;',
                 'const int i = blockIdx.x * kEventThreads + threadIdx.x;',
                 'const double x = act[i] > 0. && scal[kCmax] > 0. && v > 0. ? v : 0.;',
                 'next = fmax(y - (gy - c[i]) * invL, 0.);',
                 'rr = (y - next) * (next - x);',
                 'p = x > 0. ? fabs(gi) : fmax(-gi, 0.);',
                 'for (int i = threadIdx.x; i < K; i += kEventThreads) sum += r[i], mx = fmax(mx, pg[i]);',
                 'if (!(s_a[0] > 0.)) {   // no restart: the momentum goes on',
                 't_next = 0.5 * (1. + sqrt(1. + 4. * t * t));',
                 'beta = (t - 1.) / t_next;',
                 'scal[kKkt] = cm > 0. ? s_b[0] / cm : 0.;',
                 'const dim3 rows((unsigned)((K + kRowsPerBlock - 1) / kRowsPerBlock)), flat((unsigned)cdiv(K, kEventThreads));',
                 'hipLaunchKernelGGL(k_nnls_reduce, dim3(1), block, 0, s, (int)rows.x,',
                 'if (it % check_every == 0 || it == max_iterations) {   // the one scalar the host reads',
                 'if (history && checks < history_capacity) history[2 * checks] = it, history[2 * checks + 1] = kkt;',
                 'if (kkt <= tol || it == max_iterations) {',
                 'if (n_history) *n_history = std::min(checks, history_capacity);'):
        assert line in src, line
    assert src.count('const int i = blockIdx.x * kRowsPerBlock + threadIdx.x / kRowLanes;') == 2      # k_nnls_rows, _step
    assert src.count('csr_run(row_start, i, nnz, &a, &b);') == 2 and src.count('for_each_tap(g, o') == 2
    assert '#include "event_walk.h"' in src and 'axis_images(' not in src
    header = _read(CSRC, 'solve.h')
    assert 'long long events_nnls_workspace(long long n_rows);' in header and 'while slot < capacity' in header
    walk, modes = _read(CSRC, 'event_walk.h'), _read(CSRC, 'modes.h')
    for line in ('if (mode == TNMF_MODE_CIRCULAR && u >= S - (a - 1)) {',
                 'if (mode == TNMF_MODE_REFLECT && u >= 1 && u <= a - 1) {'):
        assert modes.count(line) == 1, line   # (axis_images: the image table, in modes.h and nowhere else)
    assert '#include "modes.h"' in walk and 'TNMF_MODE_' not in walk and 'axis_images(mode, u, ' not in walk
    for line in ('for (int t = first; t < taps; t += step) {',
                 'for (int ky = 0; ky < o.ny; ++ky) {',
                 'if ((unsigned)ly >= (unsigned)g.Ay) continue;',
                 'for (int kx = 0; kx < o.nx; ++kx) {',
                 'if ((unsigned)lx < (unsigned)g.Ax) phi += (double)w[cAA + ly * g.Ax + lx];'):
        assert line in walk, line
    api = _read(CSRC, 'api.hip')
    for line in ('g->ncy = cdiv(g->Dy + g->Ay - 1, g->ty), g->ncx = cdiv(g->Dx + g->Ax - 1, g->tx);',
                 'if (n_images > 0x7fffffffLL || n_events > 0x7fffffffLL || capacity > 0x7fffffffULL) return TNMF_E_UNSUPPORTED;',
                 'if (n_rows < 0 || nnz < 0 || max_iterations < 0 || check_every < 1 || history_capacity < 0) return TNMF_E_GEOM;',
                 'if (history_capacity > 0 && !history_out) return TNMF_E_NULL;'):
        assert line in api, line
    backend = _read('tnmf_amd', 'backends', 'HIP.py')
    for line in ('key, order = torch.sort(key, stable=True)',
                 'upper = torch.unique(keys[:total])            # sorted: i * K + j, i < j',
                 'upper = torch.cat([every * K + every, upper])  # the diagonal first, then the rows above it',
                 'live = val[K:] != 0',
                 'cap = int(max_iterations) // int(check_every) + 2'):
        assert line in backend, line


# -- the matrix of lists against the mirror ------------------------------------------------------------------------------------
def _reached(name, num_cu=sd.NUM_CU):
    geo, sample, plane, shift, W, _ = sd.matrix_case(name, num_cu)
    if name == 'stride':
        return sd.reached(geo, sample, plane, shift, None, num_cu, walk=False)
    if name == 'doctored':
        return sd.reached(geo, sample, plane, shift, W, num_cu, lists=sd.doctored(num_cu)[:3])
    return sd.reached(geo, sample, plane, shift, W, num_cu, capacity=sd.BALLOT_CAPACITY if name == 'ballot' else None)


def _old_rows(name):
    """Rows like those of tests/test_hip_events_solve.py::case for the geometry (every shift of two planes for the four small
    ones, random rows for the others): what the earlier suite reached, by the mirror."""
    N, C, P, D, A, mode = geo = OLD_GEOMETRIES[name]
    S = eref.shift_shape(D, A, mode)
    rng = np.random.default_rng(71)
    rows = {(0, pl) + u for pl in (0, 2) for u in np.ndindex(*S)} if name in ('valid', 'full', 'circular', 'reflect') else set()
    rows |= {tuple(r) for r in ed._draw(rng, (N, P) + tuple(S), 60).tolist()}
    rows = np.array(sorted(rows), dtype=np.int64)
    return geo, rows[:, 0], rows[:, 1], rows[:, 2:]


def test_the_cases_together_reach_every_branch():
    """The union over the two matrices and the geometries of the earlier solve tests is the full list of names."""
    union = {kernel: set() for kernel in sd.BRANCHES}
    for name in sd.MATRIX:
        for kernel, names in _reached(name).items():
            union[kernel] |= names
    for name in OLD_GEOMETRIES:
        for kernel, names in sd.reached(*_old_rows(name)).items():
            union[kernel] |= names
    for name in sd.SYSTEMS:
        for kernel, names in sd.system_reached(name).items():
            union[kernel] |= names
    for kernel, names in sd.BRANCHES.items():
        assert union[kernel] == set(names), (kernel, sorted(set(names) - union[kernel]))


def test_every_new_item_is_reached_by_a_case_named_for_it():
    assert list(sd.MATRIX) == ['stride', 'runs', 'tall-atom', 'long-atom-1d', 'widest-circular', 'widest-reflect', 'one-tap',
                               'taps-64', 'zero-tap', 'ballot', 'doctored']
    assert list(sd.SYSTEMS) == [f'K-{K}' for K in sd.SIZES] + ['wide-4137', 'starts', 'doctored-csr', 'every-7', 'every-above',
                                                                'no-iterations']
    claimed = {kernel: {} for kernel in sd.BRANCHES}
    for matrix, reach in ((sd.MATRIX, _reached), (sd.SYSTEMS, sd.system_reached)):
        for name, spec in matrix.items():
            claims, got = spec[-1], reach(name)
            assert claims, name
            for kernel, names in claims.items():
                for b in names:
                    assert b in sd.BRANCHES[kernel], (name, kernel, b)
                    assert b in got[kernel], f'{name} no longer reaches {kernel}: {b}'
                    claimed[kernel].setdefault(b, []).append(name)
    for kernel, names in sd.NEW.items():
        for b in names:
            assert claimed[kernel].get(b), f'no case is named for {kernel}: {b}'
    items = {b[:2] for names in sd.NEW.values() for b in names}
    assert items == {f'{k}{i}' for k, n in (('P', 6), ('M', 4), ('C', 4), ('S', 7)) for i in range(1, n + 1)}
    assert [sd.SYSTEMS[f'K-{K}'][0] for K in sd.SIZES] == [1, 15, 16, 17, 256, 257, 4096, 4137]
    assert sd.BIG > 4096 and sd.BIG % sd.ROWS_PER_BLOCK and sd.cdiv(sd.BIG, sd.ROWS_PER_BLOCK) > sd.THREADS


@pytest.mark.parametrize('num_cu', [64, 256, 304])
def test_the_stride_case_strides_on_any_cu_count(num_cu):
    geo, sample, plane, shift, _, _ = sd.matrix_case('stride', num_cu)
    here = sd.reached(geo, sample, plane, shift, None, num_cu, walk=False)
    twice = sd.reached(geo, sample, plane, shift, None, 2 * num_cu, walk=False)
    for kernel, names in sd.MATRIX['stride'][1].items():
        assert set(names) <= here[kernel] and not set(names) & twice[kernel], (kernel, num_cu)
    assert len(sample) == num_cu * 256 + 300 and len(np.unique(np.column_stack([sample, plane, shift]), axis=0)) == len(sample)


def test_the_quoted_figures():
    """What the comments of the matrix say about its cases."""
    geo, sample, plane, shift, W, _ = sd.matrix_case('runs')
    counts = ed.cell_counts(geo, sample, shift)
    assert counts.shape == (2, 2, 1) and counts[:, :, 0].tolist() == [[150, 3], [3, 0]]
    geo, sample, plane, shift, W, _ = sd.matrix_case('ballot')
    keys, groups, _ = sd.pairs_walk(geo, *sd.lists_of(geo, sample, plane, shift), len(sample))
    assert groups == [4] and sorted(keys.tolist()) == [1, 2, 3, 4] and 0 < sd.BALLOT_CAPACITY < 4
    for name, taps in (('tall-atom', 360), ('long-atom-1d', 300), ('one-tap', 1), ('taps-64', 64), ('widest-circular', 48)):
        assert sd.taps_of(sd.geometry_of(name)) == taps
    # zero-tap: the blank rows, their G_ii and c_i, and a candidate that the CSR does not hold
    geo, sample, plane, shift, W, V = sd.matrix_case('zero-tap')
    blank = sd.blank_rows(geo, plane, shift, W)
    rows = np.column_stack([sample, plane, shift])
    assert sorted(map(tuple, rows[blank].tolist())) == [(0, 0, 0, 0), (1, 0, 0, 0)]
    G, c = sr.gram(V, W, geo[5], sample, plane, shift)
    assert not np.diag(G)[blank].any() and not c[blank].any() and np.all(np.diag(G)[~blank] > 0)
    keys, _, _ = sd.pairs_walk(geo, *sd.lists_of(geo, sample, plane, shift), len(sample))
    i, j = np.divmod(np.unique(keys), len(sample))
    assert np.any(G[i, j] == 0) and np.all((G != 0)[np.triu_indices(len(sample), 1)] <= np.isin(
        np.arange(len(sample) ** 2).reshape(G.shape), keys)[np.triu_indices(len(sample), 1)]), 'a superset of the pattern'
    # widest-circular: the two images of one event overlap each other: G_ii is more than the sum of the images' own norms
    geo, sample, plane, shift, W, V = sd.matrix_case('widest-circular')
    assert np.all(ed.image_table(geo, shift)[0] == 2) and sd.own_images_overlap(geo, shift)
    # doctored: four images and one row outside the contract, the lists otherwise those of the case
    img, cell_start, events, clean = sd.doctored()
    base = sd.lists_of(*sd.matrix_case('doctored')[:4])
    assert np.count_nonzero(np.any(img != base[0], axis=1)) == 4 and np.count_nonzero(np.any(events != base[2], axis=1)) == 1
    assert len(clean) == len(events) - 5 and np.array_equal(cell_start, base[1])


@pytest.mark.parametrize('name', SMALL + list(OLD_GEOMETRIES))
def test_the_walk_finds_the_close_image_pairs_and_gram_sparse_is_the_dense_reference(name):
    """The mirror's walk through the cells against brute force over all image pairs, and gram_sparse against gram."""
    if name in sd.MATRIX:
        geo, sample, plane, shift, W, V = sd.matrix_case(name)
    else:
        geo, sample, plane, shift = _old_rows(name)
        rng = np.random.default_rng(3)
        W = rng.integers(0, 4, (geo[2], geo[1]) + geo[4]).astype(np.float64)
        V = rng.integers(0, 4, (geo[0], geo[1]) + geo[3]).astype(np.float64)
    K = len(sample)
    _, _, Ay, Ax = sd.dims(geo)
    img, cell_start, events = sd.lists_of(geo, sample, plane, shift)
    keys, _, _ = sd.pairs_walk(geo, img, cell_start, events, K)
    e = img[:, 3]
    close = ((sample[e][:, None] == sample[e][None, :]) & (e[:, None] < e[None, :])
             & (np.abs(img[:, 1][:, None] - img[:, 1][None, :]) < Ay) & (np.abs(img[:, 2][:, None] - img[:, 2][None, :]) < Ax))
    a, b = np.nonzero(close)
    assert sorted(keys.tolist()) == sorted((e[a] * K + e[b]).tolist())
    G, c = sr.gram(V, W, geo[5], sample, plane, shift)
    csr, c2 = sr.gram_sparse(V, W, geo[5], sample, plane, shift)
    G2, present = sr.densify(K, *csr)
    assert np.array_equal(G, G2) and np.array_equal(c, c2), 'integers: exact in any order'
    assert np.array_equal(present, (G != 0) | np.eye(K, dtype=bool))
    assert G.max() < 2 ** 40 and np.array_equal(G, np.round(G)) and set(np.unique(W)) <= {0., 1., 2., 3.}
    i, j = np.divmod(np.unique(keys), K)
    assert np.all(present[np.triu_indices(K, 1)] <= np.isin(np.arange(K * K).reshape(K, K), keys)[np.triu_indices(K, 1)])


def test_gram_sparse_on_float_values_and_on_the_stride_case():
    rng = np.random.default_rng(8)
    geo, sample, plane, shift, _, _ = sd.matrix_case('widest-reflect')
    W, V = rng.random((geo[2], geo[1]) + geo[4]), rng.random((geo[0], geo[1]) + geo[3])
    G, c = sr.gram(V, W, geo[5], sample, plane, shift)
    csr, c2 = sr.gram_sparse(V, W, geo[5], sample, plane, shift)
    G2, _ = sr.densify(len(sample), *csr)
    assert np.allclose(G, G2, rtol=1e-13, atol=0) and np.allclose(c, c2, rtol=1e-13, atol=0)
    geo, sample, plane, shift, W, V = sd.matrix_case('stride')
    (row_start, col, val), c = sr.gram_sparse(V, W, geo[5], sample, plane, shift)
    some = np.arange(0, len(sample), 997)
    for i in some.tolist():                       # rows of the sparse matrix against the dense one of the row's sample
        mates = np.flatnonzero(sample == sample[i])
        G, cc = sr.gram(V[sample[i]:sample[i] + 1], W, geo[5], np.zeros(len(mates), dtype=int), plane[mates], shift[mates])
        me = int(np.flatnonzero(mates == i)[0])
        cols = col[row_start[i]:row_start[i + 1]]
        assert np.array_equal(mates[(G[me] != 0) | (mates == i)], cols) and c[i] == cc[me]
        assert np.array_equal(G[me][np.isin(mates, cols)], val[row_start[i]:row_start[i + 1]])


# -- the solver's systems ----------------------------------------------------------------------------------------------------------
def _dense(s):
    r, c, v = sr.csr_entries(s['K'], s['row_start'], s['col'][:s['nnz']], s['val'][:s['nnz']])
    G = np.zeros((s['K'], s['K']))
    np.add.at(G, (r, c), v)
    return G


@pytest.mark.parametrize('name', list(sd.SYSTEMS))
def test_the_systems_are_what_the_bars_of_the_gpu_test_need(name):
    """Integers, symmetric, L a power of two attained by the hubs alone, Gershgorin's lambda_min positive; every restart test
    the reference meets is decided by at least 1e-6 of the sum of its terms' magnitudes, so no correct implementation decides
    differently; the iteration restarts and goes on without restart; the solution has rows at exactly 0 and rows that start
    at 0 and end positive."""
    s = sd.system_case(name)
    K, G = s['K'], _dense(s)
    assert np.array_equal(G, np.round(G)) and G.min() >= 0
    assert np.array_equal(G, G.T) or name == 'doctored-csr'      # (what the clamps leave of a doctored matrix is not symmetric)
    assert np.array_equal(s['c'], np.round(s['c']))
    rowabs = G.sum(axis=1)
    assert rowabs.max() == s['L'] and np.log2(s['L']) % 1 == 0
    active = np.diag(G) > 0
    margin = (2 * np.diag(G) - rowabs)[active]
    assert margin.min() >= 1 or name == 'doctored-csr', 'strictly diagonally dominant: lambda_min >= 1'
    its = sd.reference_iterates(name)
    n = len(its) - 2
    assert its[n][1] <= sd.TOL and (n == 0 or its[n - 1][1] > sd.TOL) and n <= 100
    for x, _, restarted, total, magnitude in its[:n]:
        assert magnitude == 0 or abs(total) >= 1e-6 * magnitude
    if K >= 15:
        restarts = [k for k, it in enumerate(its[:n]) if it[2]]
        assert 3 <= len(restarts) <= 8 and restarts[0] >= 3, restarts
        h, x0 = its[n][0], its[0][0]
        assert np.any(active & (h == 0)) and np.any(active & (x0 == 0) & (h > 0))
    if K >= 256:
        lengths = set(np.diff(sd.nnls_system(K, sd.SYSTEMS[name][1])['csr'][0]).tolist())
        assert {0, 16, 20} <= lengths and max(lengths) > 32
        assert all(np.diff(s['row_start'])[h] > 32 or name == 'doctored-csr' for h in s['hubs'])
        assert np.flatnonzero(rowabs == s['L']).tolist() == s['hubs']


@pytest.mark.parametrize('name', ['K-17', 'K-257', 'K-4137', 'wide-4137', 'starts', 'doctored-csr'])
def test_the_iterates_against_the_host_solver_and_between_two_orders_of_summation(name):
    """nnls_iterates against tnmf_amd.events_host.events_solve_numpy (an independent statement of the same iteration), and
    its CSR order against its dense order: the divergence the GPU test's bar on the kkt history is derived from."""
    s = sd.system_case(name)
    its = sd.reference_iterates(name)
    n = len(its) - 2
    G = _dense(s)
    h, info = events_host.events_solve_numpy(G, s['c'], np.nan_to_num(np.maximum(s['start'], 0.)), sd.TOL, 400, 1)
    assert info['converged'] and abs(info['iterations'] - n) <= 1
    m = min(n, info['iterations'])
    mine = np.array([it[1] for it in its[:m + 1]])
    assert np.allclose(info['history'][:m + 1, 1], mine, rtol=1e-9, atol=1e-12)
    assert np.allclose(h, its[info['iterations']][0], rtol=0, atol=1e-9)
    dense = sr.nnls_iterates(G, s['c'], s['start'], n)
    assert [it[2] for it in dense[:n]] == [it[2] for it in its[:n]], 'the same restarts'
    other = np.array([it[1] for it in dense[:n + 1]])
    mine = np.array([it[1] for it in its[:n + 1]])
    big = mine >= 1e-6
    divergence = np.max(np.abs(other - mine)[big] / mine[big])
    print(f'{name}: {n} iterations, kkt history CSR order against dense order: relative divergence {divergence:.3g}')
    assert divergence <= sd.ORDER_DIVERGENCE, 'the figure the bar of the GPU test is a hundred times of'
    moved = max(np.max(np.abs(a[0] - b[0])) / np.max(a[0]) for a, b in zip(its[:n + 1], dense))
    print(f'{name}: the iterates between the two orders, relative to the largest strength: {moved:.3g}')
    assert moved <= sd.ORDER_DIVERGENCE_X
    assert mine[0] == other[0] and np.array_equal(its[1][0], dense[1][0]), 'integers: the start and the first step are exact'
