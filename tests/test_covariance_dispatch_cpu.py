"""
CPU guard of the inverse-diagonal kernel matrix: the host mirror of covariance.hip (tests/covariance_dispatch.py) is held to the
sources it restates, the lists of tests/test_hip_covariance_matrix.py are held to executing every named branch, each through a
case named for it, the exact components are held to being exact (the three integer bounds below 2^53, L0 X0 = I in integers)
and the mirror's numpy transcription of the kernels' steps is held to reproducing the integer reference bit for bit, the 300-row
component included.  The same transcription with one defect at a time shows that the component named for a branch could catch
the defect: no kernel is broken for it.  The host fallback (events_inverse_diag_numpy) runs the whole matrix.  No GPU, no build:
the sources are read as text.
"""
import os
import re
import time

import numpy as np
import pytest

import covariance_dispatch as cd
import errors_reference as er
from conftest import ROOT
from tnmf_amd import _lib
from tnmf_amd.events_host import events_inverse_diag_numpy

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def _differ(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return int(np.sum(~((x == y) | (np.isnan(x) & np.isnan(y)))))


# -- the mirror against the sources --------------------------------------------------------------------------------------------
def test_constants_and_rules_are_those_of_the_sources():
    """The lines the mirror restates.  When one of them changes, tests/covariance_dispatch.py and its cases have to be looked at
    again."""
    hip, header = _read(CSRC, 'covariance.hip'), _read(CSRC, 'covariance.h')
    api, abi, backend = _read(CSRC, 'api.hip'), _read('include', 'tnmf_hip.h'), _read('tnmf_amd', 'backends', 'HIP.py')
    assert cd.THREADS == int(re.search(r'constexpr int kEventThreads = (\d+);', _read(CSRC, 'events.h')).group(1))
    assert cd.N_LDS == _lib.EVENT_INVERSE_LDS == int(re.search(r'#define TNMF_EVENTS_INVERSE_LDS (\d+)', abi).group(1))
    assert 'constexpr int kInverseDiagLds = TNMF_EVENTS_INVERSE_LDS;' in header
    assert 'inline long long events_inverse_diag_tile(long long n) { return n * n + n; }' in header
    assert 'static_assert(kInverseDiagLds <= kEventThreads, "one thread per row of a component in LDS");' in header
    assert cd.EPS == float(re.search(r'constexpr double kEps = ([0-9.e-]+);', hip).group(1)) == 2. ** -52
    assert (cd.E_NULL, cd.E_GEOM, cd.E_UNSUPPORTED) == (-1, _lib.E_GEOM, _lib.E_UNSUPPORTED)
    for line in ('return a[j * n - j * (j - 1) / 2 + (i - j)]; }',
                 'return a[(size_t)j * n + i]; }',
                 'if (t < K && local[t] < 0) d[t] = std::numeric_limits<double>::quiet_NaN();',
                 'if (t >= n_active || comp_start[t] != t || comp_start[t + 1] != t + 1) return;',
                 'if (col[k] == i) g = val[k];',
                 'const bool ok = g > 0.;',
                 'for (int e = tid; e < m.size(); e += nt) m.a[e] = 0.;',
                 'for (int r = wave; r < n; r += n_waves) {',
                 'for (int k = a + lane; k < b; k += 64) {',
                 'if (lj < 0 || lj > r || mem[lj] != j) continue;',
                 'for (int i = tid; i < n; i += nt) diag0[i] = m.at(i, i);',
                 'for (int k = 0; k < j; ++k) s = fma(-m.at(i, k), m.at(j, k), s);',
                 'if (!(pivot > (double)n * kEps * diag0[j])) {',
                 'for (int i = j + tid; i < n; i += nt) m.at(i, j) = i == j ? l : m.at(i, j) / l;',
                 'for (int k = j + 1; k <= i; ++k) s = fma(m.at(i, k), m.at(k, j), s);',
                 '__syncthreads();                   // (column j of L has been read)',
                 'for (int k = i + lane; k < n; k += 64) {',
                 'if (n < 2 || n > n_cap || n > (int)blockDim.x) return;',
                 'for (int b = c0; b < c; ++b) {',
                 'at += (long long)n * n + n;',
                 'if (n <= kInverseDiagLds || at + (long long)n * n + n > scratch_doubles) return;',
                 'inverse_diag_component<false>(m, n, tile + (size_t)n * n, tile + (size_t)n * n, K, nnz, row_start, col, val,',
                 'const int n_single = end_of(1);',
                 'for (const int cap : {16, 32, 64, 128, kInverseDiagLds}) {',
                 'if (c1 == c0) continue;',
                 'const size_t lds = (size_t)cap * (cap + 3) / 2 * sizeof(double);',
                 'if (lds > 64 * 1024)',
                 '160 * 1024));',
                 'dim3(cap <= 64 ? 64 : kEventThreads), lds, s, K,',
                 'while (c1 < n_comp && used + events_inverse_diag_tile(sizes[c1]) <= scratch_doubles)',
                 'if (c1 == c0) return TNMF_E_GEOM;'):
        assert line in hip, line
    for line in ('if (!ctx) return TNMF_E_NULL;',
                 'if (n_rows < 0 || nnz < 0 || n_comp < 0 || n_active < 0 || scratch_doubles < 0) return TNMF_E_NULL;',
                 'if (n_rows > 0 && (!row_start || !local || !d_out || (nnz > 0 && (!col || !val)))) return TNMF_E_NULL;',
                 'if (n_comp > 0 && (!comp_start || !comp_sizes || !member || !status_out)) return TNMF_E_NULL;',
                 'if (n_active > n_rows || n_comp > n_active) return TNMF_E_GEOM;',
                 'long long total = 0, previous = 1;',
                 'if (n < previous) return TNMF_E_GEOM;',
                 'if (total > n_active) return TNMF_E_GEOM;',
                 'if (total != n_active) return TNMF_E_GEOM;',
                 'if (n_comp > 0 && previous > kInverseDiagLds) {',
                 'if (events_inverse_diag_tile(previous) > scratch_doubles) return TNMF_E_GEOM;',
                 'if (!scratch) return TNMF_E_NULL;'):
        assert line in api, line
    for line in ('scratch_doubles = min(sum(tiles), max(2 ** 24, tiles[-1])) if tiles else 0',
                 'if col.numel() > K:   # (the diagonal alone: no edges)',
                 'v = torch.where(active[u] & active[c], c, u)',
                 'jumps = max(1, (K - 1).bit_length())',
                 "new = label.scatter_reduce(0, label[u], label[v], 'amin', include_self=True)"):
        assert line in backend, line


def test_known_answers_of_the_rules():
    assert [cd.lds_bytes(cap) for cap in cd.CLASSES] == [1216, 4480, 17152, 67072, 162400]
    assert cd.lds_bytes(32) == 32 * 35 // 2 * 8 and cd.lds_bytes(cd.N_LDS) <= cd.LDS_RAISED < cd.lds_bytes(cd.N_LDS + 1)
    assert [cd.lds_threads(cap) for cap in cd.CLASSES] == [64, 64, 64, 256, 256]
    assert [cd.lds_raised(cap) for cap in cd.CLASSES] == [False, False, False, True, True]          # 64 KiB lies between 64 and 128
    assert [cd.class_of(n) for n in (1, 2, 16, 17, 32, 33, 64, 65, 128, 129, 200, 201, 300)] == \
        ['single', 16, 16, 32, 32, 64, 64, 128, 128, 200, 200, 'tile', 'tile']
    # the packed triangle: the columns follow each other without a gap, the last entry is the last double
    for n in (2, 5, 17):
        flat = [cd.packed_index(n, i, j) for j in range(n) for i in range(j, n)]
        assert flat == list(range(n * (n + 1) // 2))
    assert cd.packed_index(5, 4, 4) == 14 and cd.packed_index(5, 2, 1) == 6
    assert cd.tile_doubles(201) == 40602 and cd.tile_doubles(300) == 90300
    assert cd.singular_bar(64, 1. + 2. ** -46) == 2. ** -46 + 2. ** -92 and cd.singular_bar(16, 1.) == 2. ** -48
    # the refusals, in the order of the entry
    ok = dict(n_rows=10, nnz=30, n_comp=3, n_active=9, scratch_doubles=0, sizes=[1, 3, 5])
    assert cd.refusal(**ok) == 0
    assert cd.refusal(**dict(ok, ctx=False)) == cd.refusal(**dict(ok, nnz=-1)) == cd.refusal(**dict(ok, d=False)) == cd.E_NULL
    assert cd.refusal(**dict(ok, status=False)) == cd.E_NULL and cd.refusal(**dict(ok, n_comp=0, n_active=0, status=False)) == 0
    assert cd.refusal(**dict(ok, n_rows=2 ** 31)) == cd.E_UNSUPPORTED
    assert cd.refusal(**dict(ok, n_active=11)) == cd.refusal(**dict(ok, n_comp=10)) == cd.E_GEOM
    assert cd.refusal(**dict(ok, sizes=[3, 1, 5])) == cd.refusal(**dict(ok, sizes=[0, 4, 5])) == cd.E_GEOM
    assert cd.refusal(**dict(ok, sizes=[1, 3, 6])) == cd.refusal(**dict(ok, sizes=[1, 3, 4])) == cd.E_GEOM
    big = dict(n_rows=300, nnz=900, n_comp=2, n_active=299, sizes=[1, 298])
    assert cd.refusal(**big, scratch_doubles=298 * 299 - 1) == cd.E_GEOM and cd.refusal(**big, scratch_doubles=298 * 299) == 0
    assert cd.refusal(**big, scratch_doubles=298 * 299, scratch=False) == cd.E_NULL


def test_the_batch_planner_matches_hand_computed_plans():
    sizes = cd.case('tiles')['sizes'].tolist()
    assert sizes == [201, 257, 300]
    assert cd.plan_batches(sizes, cd.PLANS['three-batches']) == [[0], [1], [2]] and cd.PLANS['three-batches'] == 90300
    assert cd.plan_batches(sizes, cd.PLANS['exact-fit']) == [[0, 1], [2]] and cd.PLANS['exact-fit'] == 40602 + 66306
    assert cd.plan_batches(sizes, cd.PLANS['exact-fit'] - 1) == [[0], [1], [2]]                   # (one double less: <=, not <)
    assert cd.default_scratch(sizes) == 40602 + 66306 + 90300 and cd.plan_batches(sizes, cd.default_scratch(sizes)) == [[0, 1, 2]]
    assert cd.plan_batches(sizes, 90299) is None and cd.plan_batches([1, 2, 200], 0) == []
    # components of the LDS path come first and take no scratch; the default is capped at 2^24 doubles or one tile
    assert cd.plan_batches([1, 16, 200, 201, 201], 2 * 40602) == [[3, 4]]
    assert cd.default_scratch([5000] * 3) == 5000 * 5001 and cd.default_scratch([3000] * 3) == 2 ** 24
    assert cd.plan_batches([3000] * 3, 2 ** 24) == [[0], [1], [2]]
    assert 'batch:several' in cd.reached('tiles', 'three-batches') and 'batch:three-tiles' not in cd.reached('tiles', 'exact-fit')
    assert {'batch:exact-fit', 'batch:several'} <= cd.reached('tiles', 'exact-fit')
    assert {'batch:one', 'batch:three-tiles'} <= cd.reached('tiles', 'one-batch')


# -- coverage ------------------------------------------------------------------------------------------------------------------
def _reach(name):
    plans = cd.PLANS if name == 'tiles' else ('one-batch',)
    return set().union(*(cd.reached(name, plan) for plan in plans))


def test_every_branch_is_reached_and_every_case_reaches_what_it_names():
    union = set()
    for name, (_, _, claims) in cd.MATRIX.items():
        got = _reach(name)
        union |= got
        assert set(claims) <= got, (name, sorted(set(claims) - got))
    missing = set(cd.BRANCHES) - union - set(cd.NOT_REACHED)
    assert not missing, sorted(missing)
    assert not union & set(cd.NOT_REACHED) and len(cd.NOT_REACHED) == 7
    # 'all' holds every component: whatever a case on its own reaches but an empty class, all in one launch sequence
    alone = set().union(*(_reach(n) for n in cd.MATRIX if n != 'all'))
    absent = {b for b in alone if b.endswith((':empty', ':none'))} | {'batch:several'}
    assert _reach('all') == alone - absent and set(cd.MATRIX['all'][0]) == set(cd.COMPONENTS)
    for cap in cd.CLASSES:       # every class is empty in a case and on its own in another
        assert any(f'class-{cap}:empty' in _reach(n) for n in cd.MATRIX)
        assert any({f'class-{c}:{"non-empty" if c == cap else "empty"}' for c in cd.CLASSES} <= _reach(n) for n in cd.MATRIX), cap


def test_dropping_the_case_named_for_a_branch_loses_it_or_the_others_are_recorded():
    got = {name: _reach(name) for name in cd.MATRIX}
    assert cd.also() == cd.ALSO
    claimed = set()
    for branch in cd.BRANCHES:
        reach = tuple(n for n in cd.MATRIX if branch in got[n])
        claim = tuple(n for n in cd.MATRIX if branch in cd.MATRIX[n][2])
        claimed |= set(claim)
        assert set(claim) <= set(reach), branch
        if len(reach) > 1:
            assert cd.ALSO[branch] == reach, (branch, reach)
        elif branch not in cd.NOT_REACHED:
            assert reach == claim, (branch, reach, claim)
    assert set(cd.ALSO) <= set(cd.BRANCHES)
    # the sizes of the issue: one component each, two more in 17 .. 32, several of one row
    sizes = sorted(cd.component(c)['n'] for c in cd.COMPONENTS if cd.COMPONENTS[c][0] == 'exact' and not c.startswith('bar'))
    assert set(sizes) >= {2, 16, 17, 32, 33, 64, 65, 128, 129, 199, 200, 201, 257, 300}
    assert sum(16 < n <= 32 for n in sizes) == 4 and sum(cd.COMPONENTS[c][0] == 'single' for c in cd.COMPONENTS) == 7
    total = cd.case('all')['K']
    print(f'the whole matrix as one list: {total} rows, {len(cd.case("all")["csr"][1])} entries, '
          f'{len(cd.case("all")["sizes"])} components')
    assert 2000 <= total <= 3500


def test_the_layout_is_what_the_cases_are_for():
    for name in cd.MATRIX:
        c = cd.case(name)
        row_start, col, val = c['csr']
        K, active = c['K'], c['active']
        row = np.repeat(np.arange(K), np.diff(row_start))
        comp = np.full(K, -1)
        for k, g in enumerate(c['groups']):
            comp[g] = k
            assert np.all(np.diff(g) > 0)
        # every inactive row couples to rows of at least two components, and every component is touched by one
        for u in np.flatnonzero(~active):
            mine = col[row_start[u]:row_start[u + 1]]
            assert len(set(comp[mine[active[mine]]])) >= 2, (name, u)
        assert set(comp[row[~active[col] & active[row]]]) == set(range(len(c['groups']))), name
        # poison exactly where a row or a column is not active; the matrix is bit-symmetric
        dead = ~active[row] | ~active[col]
        assert np.all(val[dead] == cd.POISON) and np.all(np.abs(val[~dead]) < 2. ** 40)
        dense = np.zeros((K, K))
        dense[row, col] = val
        assert np.array_equal(dense, dense.T)
        for k in range(K):
            assert np.all(np.diff(col[row_start[k]:row_start[k + 1]]) > 0)
        # the rows of a component are interleaved with the others: no component of more than 16 rows is a run of rows
        for g in c['groups']:
            assert len(g) <= 16 or g[-1] - g[0] > len(g) - 1, name
    # the components of 65 rows and more are dense: every run of theirs takes a second trip of the lane loop
    c = cd.case('all')
    runs = np.diff(c['csr'][0])
    for g in c['groups']:
        if len(g) >= 65:
            assert runs[g].min() > 64, len(g)
    single = {n: int(c['rows_of'][n][0]) for n in ('single-no-diagonal', 'single-zero-diagonal')}
    row_start, col, val = c['csr']
    run = lambda i: slice(row_start[i], row_start[i + 1])       # noqa: E731
    assert single['single-no-diagonal'] not in col[run(single['single-no-diagonal'])] and runs[single['single-no-diagonal']] > 0
    assert val[run(single['single-zero-diagonal'])][col[run(single['single-zero-diagonal'])] == single['single-zero-diagonal']] == 0.


# -- exactness -----------------------------------------------------------------------------------------------------------------
def test_every_exact_component_is_exact_and_well_conditioned():
    """The three bounds of the mirror per component; L0 X0 = I in integers; every pivot the square of a power of two.  cond_2
    <= 1e4 as in the scenes of tests/test_events_errors_cpu.py for every component that is not singular -- but the three of
    the bar family: a last pivot of 2^-46 IS a condition number of 2^46 n, that is what they are for; they are exact all the
    same, and on the host fallback their bar is vacuous (recorded below)."""
    worst = {}
    for name, (kind, _, _) in cd.COMPONENTS.items():
        if kind == 'single':
            continue
        c, e = cd.component(name), cd.exactness(name)
        assert e['pivots'] and max(e['cholesky'], e['inverse'], e['squares']) < 2 ** 53, (name, e)
        assert e['identity'] is (True if kind == 'exact' else None), name
        assert np.array_equal(c['G'], c['G'].T) and np.all(np.diag(c['G']) > 0)
        if kind == 'exact':
            kappa = float(np.linalg.cond(c['G']))
            worst[name] = kappa
            assert np.all(np.isfinite(c['d'])) and np.all(c['d'] > 0)
            if not name.startswith('bar'):
                assert kappa <= 1e4, (name, kappa)
    print('cond_2: ' + ', '.join(f'{n} {k:.3g}' for n, k in worst.items()))
    assert all(worst[n] > 2. ** 44 for n in ('bar-16-finite', 'bar-64-finite'))
    # the three sensitivities: dense L with sparse X, sparse L with dense X, and the two mixed
    fill = lambda M: np.count_nonzero(M) / (len(M) * (len(M) + 1) / 2)       # noqa: E731
    L, X = cd.component('ones-65')['L0'], cd.component('ones-65')['X0']
    assert fill(L) == 1. and np.count_nonzero(X) == 2 * 65 - 1
    L, X = cd.component('bidiagonal-64')['L0'], cd.component('bidiagonal-64')['X0']
    assert fill(X) == 1. and np.count_nonzero(L) == 2 * 64 - 1
    L, X = cd.component('kron-33')['L0'], cd.component('kron-33')['X0']
    assert 0.1 < fill(L) < 0.9 and 0.1 < fill(X) < 0.9
    # the bar: 2^-46 against 64 * 2^-52 * (1 + 2^-46) and 16 * 2^-52 * (1 + 2^-46); 2^-44 against the former
    G = cd.component('bar-64-singular')['G']
    assert G[63, 63] == 1. + 2. ** -46 and not 2. ** -46 > cd.singular_bar(64, G[63, 63]) and 2. ** -46 > cd.singular_bar(64, 1.) / 2
    assert 2. ** -46 > cd.singular_bar(16, cd.component('bar-16-finite')['G'][15, 15])
    assert cd.component('bar-64-finite')['G'][63, 63] == 1. + 2. ** -44 and 2. ** -44 > cd.singular_bar(64, 1. + 2. ** -44)
    assert cd.component('bar-16-finite')['d'][0] == 2. + 2. ** 46 and cd.component('bar-16-finite')['d'][15] == 2. ** 46
    # the singular ones: rows j - 1 and j of G are equal
    for n in cd.SINGULAR_SIZES:
        for where, j in (('first', 1), ('middle', n // 2), ('last', n - 1)):
            G = cd.component(f'singular-{n}-{where}')['G']
            assert np.array_equal(G[j], G[j - 1]) and cd.component(f'singular-{n}-{where}')['pivot_at'] == j


def test_the_integer_reference_is_the_inverse_in_exact_rational_arithmetic():
    """The reference of a small component of every family against fractions.Fraction: Gauss-Jordan on G itself."""
    from fractions import Fraction
    for name in ('ones-2', 'ones-16', 'bidiagonal-17', 'kron-20', 'bidiagonal-29', 'ones-32', 'kron-33', 'bar-16-finite'):
        c = cd.component(name)
        n = c['n']
        M = [[Fraction(float(v)) for v in row] + [Fraction(int(i == k)) for k in range(n)] for i, row in enumerate(c['G'])]
        for j in range(n):
            M[j] = [v / M[j][j] for v in M[j]]
            for i in range(n):
                if i != j and M[i][j] != 0:
                    M[i] = [a - M[i][j] * b for a, b in zip(M[i], M[j])]
        assert [M[i][n + i] for i in range(n)] == [Fraction(float(v)) for v in c['d']], name
    blocks = cd.component('blocks-129')
    G = blocks['G'].astype(np.longdouble)
    assert np.allclose(np.diag(np.linalg.inv(blocks['G'])), blocks['d'], rtol=1e-10, atol=0) and G.shape == (129, 129)


# -- the transcription against the reference, and the wrong transcriptions against it -------------------------------------------
@pytest.mark.parametrize('name', list(cd.MATRIX))
def test_the_transcription_reproduces_the_integer_reference_bit_for_bit(name):
    c = cd.case(name)
    t = time.perf_counter()
    d, status = cd.device_model(c)
    print(f'{name}: {c["K"]} rows, {len(c["sizes"])} components, the transcription takes {time.perf_counter() - t:.2f} s')
    assert d.tobytes() == c['d'].tobytes(), (name, _differ(d, c['d']))
    assert np.array_equal(status, c['status']) and np.array_equal(np.isnan(d), ~c['active'])
    assert np.array_equal(np.isinf(d), np.isin(np.arange(c['K']), np.concatenate(
        [g for g, s in zip(c['groups'], c['status']) if s] + [np.zeros(0, dtype=np.int64)])))


def test_the_transcription_of_300_rows_takes_well_under_a_second_and_every_plan_gives_the_same_bits():
    c = cd.case('tiles')
    k = c['names'].index('blocks-300')
    t = time.perf_counter()
    d, status = cd.device_model(c, only=[k])
    took = time.perf_counter() - t
    rows = c['rows_of']['blocks-300']
    print(f'300 rows: {took:.2f} s')
    assert d[rows].tobytes() == c['d'][rows].tobytes() and status[k] == 0 and took < 1.
    for plan, scratch in cd.PLANS.items():
        d, status = cd.device_model(c, scratch_doubles=scratch)
        assert d.tobytes() == c['d'].tobytes() and not status.any(), plan


def test_wrong_transcriptions_differ_on_the_components_named_for_them():
    assert set(cd.DEFECTS) == {
        'cholesky-one-term-short', 'inverse-k<i', 'inverse-read-after-write', 'scatter-first-trip-only',
        'scatter-inactive-column', 'tile-not-zeroed', 'packed-index-j(j+1)/2', 'bar-without-n', 'bar-of-the-factored-pivot',
        'third-tile-from-one-predecessor'}
    for defect, (name, comp) in cd.DEFECTS.items():
        c = cd.case(name)
        k = c['names'].index(comp)
        rows = c['rows_of'][comp]
        right, _ = cd.device_model(c, only=[k])
        assert right[rows].tobytes() == c['d'][rows].tobytes()
        for prefill in (np.nan, 1., 0.):
            if prefill == 0. and defect != 'tile-not-zeroed':
                continue
            d, status = cd.device_model(c, defect=defect, only=[k], prefill=prefill)
            n = _differ(d[rows], c['d'][rows])
            print(f'{defect} (storage prefilled with {prefill}): {comp} of {name} differs in {n} of {len(rows)} rows, status '
                  f'{status[k]} for {c["status"][k]}')
            if prefill == 0.:        # a scratch that happens to hold zeros hides a missing zero fill: the test prefills NaN
                assert n == 0
            else:
                assert n > 0, (defect, name, comp)
    # the bar defects turn the singular component finite; the component with 2^-44 stays finite under the right bar
    c = cd.case('class-64')
    for defect in ('bar-without-n', 'bar-of-the-factored-pivot'):
        d, status = cd.device_model(c, defect=defect, only=[c['names'].index('bar-64-singular')])
        assert status[c['names'].index('bar-64-singular')] == 0 and np.all(np.isfinite(d[c['rows_of']['bar-64-singular']]))
    # a bar of 4 n in the place of n would refuse the 16-row component at 2^-46 and the 64-row one at 2^-44
    assert not 2. ** -46 > 4 * cd.singular_bar(16, 1. + 2. ** -46) and not 2. ** -44 > 4 * cd.singular_bar(64, 1. + 2. ** -44)


# -- the host fallback on the whole matrix -------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cd.MATRIX))
def test_the_host_fallback_runs_the_matrix(name):
    """events_inverse_diag_numpy uses LAPACK: held to the relative bar of tests/errors_reference.py with taps = 0,
    kappa * 4 n^2 * 2^-52 per component, against the integer reference; +inf on the same rows, the same status vector."""
    c = cd.case(name)
    d, info = events_inverse_diag_numpy(c['csr'], c['active'], 2048)
    assert np.array_equal(info['sizes'], c['sizes']) and np.array_equal(info['status'], c['status'])
    assert np.array_equal(np.isnan(d), ~c['active']) and np.array_equal(np.isinf(d), np.isinf(c['d']))
    assert info['n_singular'] == int(c['status'].sum()) and info['largest_component'] == int(c['sizes'][-1])
    worst = (-1., '')
    for g, comp, s in zip(c['groups'], c['names'], c['status']):
        if s:
            continue
        kappa = 1. if len(g) == 1 else float(np.linalg.cond(cd.component(comp)['G']))
        assert kappa <= 1e4 or comp.startswith('bar'), (comp, kappa)
        bar = kappa * 4 * len(g) ** 2 * 2. ** -52
        err = float(np.max(np.abs(d[g] - c['d'][g]) / c['d'][g]))
        worst = max(worst, (err / bar, comp))
        assert err <= bar, (comp, err, bar)
    print(f'{name}, host: closest to its bar {worst[1]} at {worst[0]:.3g} of it')
    with pytest.raises(ValueError, match=rf'{int(c["sizes"][-1])} rows.*max_component={int(c["sizes"][-1]) - 1}'):
        events_inverse_diag_numpy(c['csr'], c['active'], int(c['sizes'][-1]) - 1)


# -- the component graphs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', cd.GRAPHS + ('random-dense',))
def test_the_graph_cases_on_the_host(name):
    """The labels of the mirror's min-label hooking give the components of the breadth-first search, within
    4 ceil(log2 K) rounds; the host fallback gives d inside the bar of errors_reference; cond_2 <= 1e4."""
    c = cd.graph_case(name)
    ref, K = c['ref'], c['K']
    assert np.nanmax(ref['kappa']) <= 1e4 and K <= 1025
    label, rounds = cd.hooking(c)
    print(f'{name}: K {K}, sizes {sorted(set(c["sizes"].tolist()))}, cond <= {np.nanmax(ref["kappa"]):.3g}, {rounds} rounds of hooking')
    assert rounds <= 4 * int(np.ceil(np.log2(K))) and (rounds == 0) == (name == 'diagonal-only')
    for g in c['groups']:
        assert np.all(label[g] == g[0])
    assert len(set(label[c['active']].tolist())) == len(c['groups'])
    d, info = events_inverse_diag_numpy(c['csr'], c['active'], 2048)
    on = c['active']
    assert np.array_equal(info['sizes'], c['sizes']) and not info['status'].any() and np.all(np.isnan(d[~on]))
    assert np.all(np.abs(d[on] - ref['d'][on]) <= ref['bar'][on] * ref['d'][on])
    if name == 'three-equal':
        assert c['sizes'].tolist() == [16, 16, 16] and [int(g[0]) for g in c['groups']] == [0, 1, 2]
    if name == 'star-hub-last':
        assert c['sizes'].tolist() == [300] and np.diff(c['csr'][0])[-1] == 300
    if name == 'random-dense':
        assert c['sizes'].tolist() == list(cd.DENSE_SIZES) and (~on).sum() == 6 and er.N_LDS < 257
