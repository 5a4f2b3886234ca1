"""
CPU guard of the scoring kernel matrix: the host mirror of the seven kernels that score events (tests/scoring_dispatch.py) is
held to the sources it restates, the cases of tests/test_hip_scoring_matrix.py are held to executing every named branch at
several CU counts, each item of the list the matrix was built for (N1-N4, S1-S3, T1, K1-K4, Q1-Q2, L1-L4, A1-A4) through a
case named for it, and the mirror's models of the kernels are held to the float64 references.  The wrong models -- the
references with one defect each -- show that the case named for a branch could catch the defect: no kernel is broken for it.
No GPU, no build: the sources are read as text.
"""
import os
import re
import time

import numpy as np
import pytest

import alternatives_reference as aref
import events_dispatch as ed
import landscape_reference as lref
import pursuit_reference as pur
import scoring_dispatch as sc
from conftest import ROOT

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')
CUS = (256, 304, 64, 8)
DTYPES = ('f32', 'f64')
SENTINEL = -12345.5
SLOWEST = {}


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def _reached(name, cu):
    """{kernel: names} over both element types, timed."""
    t = time.perf_counter()
    out = {}
    for dt in DTYPES if sc.kind_of(name) == 'score' else DTYPES[:1]:
        for kernel, names in sc.reached(name, cu, dt).items():
            out[kernel] = out.get(kernel, set()) | names
    SLOWEST[name] = max(SLOWEST.get(name, 0.), time.perf_counter() - t)
    return out


# -- the mirror against the sources --------------------------------------------------------------------------------------------
def test_constants_and_rules_are_those_of_the_sources():
    """The lines the mirror restates.  When one of them changes, tests/scoring_dispatch.py and its cases have to be looked at
    again."""
    events_h, walk = _read(CSRC, 'events.h'), _read(CSRC, 'event_walk.h')
    pursuit, events = _read(CSRC, 'pursuit.hip'), _read(CSRC, 'events.hip')
    landscape, alternatives = _read(CSRC, 'landscape.hip'), _read(CSRC, 'alternatives.hip')
    assert sc.THREADS == int(re.search(r'constexpr int kEventThreads = (\d+);', events_h).group(1))
    assert 'return (unsigned)std::max<long long>(1, std::min<long long>(blocks, (long long)ctx->num_cu * per_cu));' in events_h
    for src in (pursuit, landscape, alternatives):
        assert 'constexpr int kWaves = kEventThreads / 64;' in src
    for src in (landscape, alternatives):
        assert sc.PATCH_MAX == int(re.search(r'constexpr int kPatchMax = (\d+);', src).group(1))
    assert sc.BATCH == aref.BATCH == int(re.search(r'constexpr int kBatch = (\d+);', alternatives).group(1))
    assert sc.PER_CU['landscape'] == int(re.search(r'#define TNMF_LANDSCAPE_BLOCKS_PER_CU (\d+)', landscape).group(1))
    assert sc.PER_CU['alternatives'] == int(re.search(r'#define TNMF_ALTERNATIVES_BLOCKS_PER_CU (\d+)', alternatives).group(1))
    for line in ('for (int t = threadIdx.x; t < taps; t += kEventThreads) sq += (double)w[t] * (double)w[t];',
                 'for (int e = blockIdx.x * kEventThreads + threadIdx.x; e < entries; e += gridDim.x * kEventThreads) {',
                 'if (!o.single() || oy0 < 0 || ox0 < 0 || oy0 + g.Ay > g.Dy || ox0 + g.Ax > g.Dx) {',
                 'const dim3 grid(events_grid(ctx, cdiv(entries, kEventThreads), 8), (unsigned)f.g.P);',
                 'if (Hs == Sx && per_sample <= 0x7fffffffLL && per_sample % kV == 0) {',
                 'rows = planes / P, brows = 1, Sx = Hs = (int)per_sample;',
                 'const int cpr = cdiv(Sx, kV);',
                 'const unsigned grid = events_grid(ctx, (rows * cpr + kEventThreads - 1) / kEventThreads, 8);',
                 'const bool aligned = aligned16(a) && aligned16(gain) && Hs % kV == 0;',
                 'const long long row_step = stride / cpr;',
                 'const int chunk_step = (int)(stride - row_step * cpr), brow_step = (int)(row_step % brows);',
                 'if (kAligned && x0 + kV <= Sx) {',
                 'for (int i = 0; i < kV && x0 + i < Sx; ++i) dst[i] = score_of(src[i], bs[i]);',
                 'row += row_step, chunk += chunk_step, brow += brow_step;',
                 'if (chunk >= cpr) chunk -= cpr, ++row, ++brow;',
                 'if (brow >= brows) brow -= brows;',
                 'const unsigned tgrid = events_grid(ctx, (n_taken + kEventThreads - 1) / kEventThreads, 8);',
                 'if (f < 0 || f >= entries) continue;',
                 'gain[(size_t)row * Hs + (f - row * Sx)] = (T)0;',
                 'for (long long e = (long long)blockIdx.x * kWaves + wave; e < n_picked; e += (long long)gridDim.x * kWaves) {',
                 'const int4 v = make_int4((int)(np / g.P), (int)(np % g.P), u / Sx, u % Sx);   // sample, plane, uy, ux',
                 'const bool live = a > 0. && b > 0.;',
                 'const unsigned grid = events_grid(ctx, (n_picked + kWaves - 1) / kWaves, 64);'):
        assert line in pursuit, line
    assert 'const unsigned grid = events_grid(ctx, (n_events + kWaves - 1) / kWaves);' in events
    assert 'gain[e] = fma(hh, b, hv * a);' in events
    for line in ('const long long cells = (long long)g.C * (g.Ay + 2 * ry) * (g.Ax + 2);',
                 'const int patch = stage && cells <= kPatchMax ? (int)cells : 0;',
                 'const unsigned grid = events_grid(ctx, (n_events + kWaves - 1) / kWaves, TNMF_LANDSCAPE_BLOCKS_PER_CU);',
                 'for (long long e = (long long)blockIdx.x * kWaves + wave; e < n_events; e += (long long)gridDim.x * kWaves) {',
                 'if (patch <= 0) return false;', 'for (int i = lane; i < cells; i += 64) {',
                 'const int Py = g.Ay + 2 * ry, Px = g.Ax + 2;',
                 'const double *at = mine + c * (int)uPP + (jy + 1) * Px + (jx + 1);',
                 'const int c = t / uAx, jx = t - c * g.Ax;   // (Ay == 1)',
                 'if ((unsigned)uy < (unsigned)Sy && (unsigned)ux < (unsigned)Sx) {   // (wave-uniform; else zeros)'):
        assert line in landscape, line
    for line in ('const long long cells = (long long)g.C * g.Ay * g.Ax;',
                 'const int patch = stage && cells <= kPatchMax ? (int)cells : 0;',
                 'const unsigned grid = events_grid(ctx, (n_events + kWaves - 1) / kWaves, TNMF_ALTERNATIVES_BLOCKS_PER_CU);',
                 'return axis_whole(mode, uy, g.Ay, Sy, g.Dy) && axis_whole(mode, ux, g.Ax, Sx, g.Dx);',
                 'for (int j = lane; j < n_alt; j += 64) {', 'for (int j0 = 0; j0 < n_alt; j0 += kBatch) {',
                 'const int live = min(kBatch, n_alt - j0);',
                 'const T *w0 = W + (size_t)(v.y / block * block + v.y % stride) * taps;        // the first candidate'):
        assert line in alternatives, line
    for line in ('if ((unsigned)y < (unsigned)g.Dy && (unsigned)x < (unsigned)g.Dx) f(t, c, y, x);',
                 'if ((unsigned)lx < (unsigned)g.Ax) phi += (double)w[cAA + ly * g.Ax + lx];'):
        assert line in walk, line
    # axis_whole: with the image table, in modes.h
    assert '#include "modes.h"' in walk and 'axis_whole' not in walk.split('#pragma once')[1]
    assert _read(CSRC, 'modes.h').count('return o >= 0 && o + a <= D;') == 1


def test_known_answers_of_the_rules():
    assert sc.events_grid(10, 256, 64) == 10 and sc.events_grid(10 ** 9, 256, 64) == 16384 and sc.events_grid(0, 256, 8) == 1
    assert sc.events_grid(3000, 256, 8) == 2048 and sc.events_grid(3000, 304, 4) == 1216 and sc.events_grid(5, 8, 4) == 5
    # the patches of the four limit geometries
    got = [sc.cells(k, sc.spec_of(n)[0]) for k, n in (('landscape', 'landscape-limit-fits'), ('landscape', 'landscape-limit-over'),
                                                      ('alternatives', 'alternatives-limit-fits'),
                                                      ('alternatives', 'alternatives-limit-over'))]
    assert got == [2048, 2112, 2048, 2112]
    assert [sc.patch('landscape', sc.spec_of(n)[0]) for n in ('landscape-limit-fits', 'landscape-limit-over')] == [2048, 0]
    assert [sc.patch('alternatives', sc.spec_of(n)[0]) for n in ('alternatives-limit-fits', 'alternatives-limit-over')] == [2048, 0]
    assert sc.cells('landscape', (1, 2, 1, (1030,), (1022,), 'valid')) == 2048       # the 1-D limit of the present tests
    # the score: 2 x 3 x 5 x 64 floats, contiguous: one row of 960 per sample, 240 chunks; 480 for doubles
    plan = sc.score_plan('f32', 2, 3, 5, 64, 0, 0, 0, 256)
    assert (plan['collapsed'], plan['rows'], plan['brows'], plan['Sx'], plan['cpr'], plan['aligned']) == (True, 2, 1, 960, 240, True)
    assert (plan['grid'], plan['row_step'], plan['chunk_step'], plan['brow_step']) == (2, 2, 32, 0)
    assert sc.score_plan('f64', 2, 3, 5, 64, 0, 0, 0, 256)['cpr'] == 480
    for dt, unit in (('f32', 4), ('f64', 2)):     # a pointer one element in breaks the alignment, one 16-byte unit in keeps it
        plan = lambda a_off, gain_off: sc.score_plan(dt, 2, 3, 5, 64, 0, a_off, gain_off, 256)     # noqa: E731
        assert not plan(1, 0)['aligned'] and not plan(0, 1)['aligned'] and plan(unit, 0)['aligned'] and plan(0, unit)['aligned']
    # 2 x 3 x 5 x 7: 105 entries per sample are no multiple of 4 or 2: 30 rows of 2 (4) chunks, the width breaks the alignment
    for dt, cpr in (('f32', 2), ('f64', 4)):
        plan = sc.score_plan(dt, 2, 3, 5, 7, 0, 0, 0, 256)
        assert (plan['collapsed'], plan['rows'], plan['brows'], plan['cpr'], plan['aligned']) == (False, 30, 15, cpr, False)
        assert (plan['grid'], plan['row_step'], plan['chunk_step'], plan['brow_step']) == (1, 256 // cpr, 0, 256 // cpr % 15)
    plan = sc.score_plan('f32', 2, 3, 5, 7, 1, 0, 0, 256)                             # padded to 8: aligned, not contiguous
    assert (plan['collapsed'], plan['aligned'], plan['Hs']) == (False, True, 8)
    # the long rows at 256 CUs: 2 x (256 * 8192 + 12) floats, 524291 chunks a row against 524288 threads
    plan = sc.score_case('score-long-rows', 'f32', 256, data=False)['plan']
    assert (plan['rows'], plan['cpr'], plan['grid'], plan['stride'], plan['row_step'], plan['chunk_step']) == \
        (2, 524291, 2048, 524288, 0, 524288)
    assert plan['per_sample'] > 256 * 8192
    walk = sc.score_walk(plan)
    assert len(walk) == 3 and sum(len(p[0]) for p in walk) == 2 * 524291
    # the wave assignment: row e goes to wave e mod (grid * 4)
    assert sc.row_grid('landscape', 4133, 256) == 1024 and sc.wave_of(4096, 1024) == 0 and sc.wave_of(4132, 1024) == 36
    assert sc.row_grid('pick', 65573, 256) == 16384 and sc.wave_of(65536 + 5, 16384) == 5
    assert sc.row_grid('alternatives', 165, 8) == 32 and sc.wave_of(128, 32) == 0
    assert sc.batches(1) == [(0, 1)] and sc.batches(5) == [(0, 4), (4, 1)] and sc.batches(66)[-1] == (64, 2)
    assert sc.first_candidate(5, 3, 2) == 1 and sc.first_candidate(4, 3, 1) == 3 and sc.first_candidate(7, 2, 2) == 5


# -- coverage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cu', CUS)
def test_every_branch_is_reached_and_every_case_reaches_what_it_names(cu):
    union = {kernel: set() for kernel in sc.BRANCHES}
    for name in sc.MATRIX:
        got = _reached(name, cu)
        for kernel, names in got.items():
            union[kernel] |= names
        for kernel, names in sc.MATRIX[name][2].items():
            assert set(names) <= got[kernel], (name, kernel, cu, sorted(set(names) - got[kernel]))
    for kernel, names in sc.BRANCHES.items():
        missing = set(names) - union[kernel] - set(sc.NOT_REACHED.get(kernel, ()))
        assert not missing, (kernel, cu, sorted(missing))
    assert sc.NOT_REACHED == {'score': ('not-reached: needs 2^31 elements',)}
    slow = max(SLOWEST, key=SLOWEST.get)
    print(f'{cu} CUs: the slowest case of the mirror is {slow!r}, {SLOWEST[slow]:.2f} s')


def test_every_element_type_of_a_score_case_reaches_what_it_names():
    for name in sc.names_of('score'):
        for dt in DTYPES:
            for cu in CUS:
                got = sc.reached(name, cu, dt)
                for kernel, names in sc.MATRIX[name][2].items():
                    assert set(names) <= got[kernel], (name, dt, cu, kernel, sorted(set(names) - got[kernel]))


@pytest.mark.parametrize('cu', (256, 8))
def test_dropping_the_case_named_for_an_item_loses_it(cu):
    got = {name: _reached(name, cu) for name in sc.MATRIX}
    seen = set()
    for kernel, items in sc.NEW.items():
        for item in items:
            reach = tuple(n for n in sc.MATRIX if item in got[n].get(kernel, ()))
            claim = tuple(n for n in sc.MATRIX if item in sc.MATRIX[n][2].get(kernel, ()))
            assert claim and set(claim) <= set(reach), (kernel, item)
            if len(reach) > 1:       # recorded beside the cases: sc.ALSO
                assert sc.ALSO.get((kernel, item)) == reach, (kernel, item, reach)
                seen.add((kernel, item))
            else:
                assert reach == claim, (kernel, item, reach, claim)
    assert seen == set(sc.ALSO)


def test_the_in_one_wave_cases_order_their_rows_for_the_cu_count():
    for cu in CUS:
        c = sc.events_case('stride-4', cu)
        K = len(c['rows'])
        grid = sc.row_grid('landscape', K, cu)
        G = grid * sc.WAVES
        assert K == cu * 16 + 37 and grid == cu * 4 == sc.row_grid('alternatives', K, cu)
        for rule in (sc.landscape_staged, sc.alternatives_staged):
            paths = sc._paths(rule, c['geo'], c['rows'])
            for e in range(37):
                assert sc.wave_of(e, grid) == sc.wave_of(e + G, grid) == e
                assert (paths[e], paths[e + G]) == (('s', 'w'), ('w', 's'), ('s', 's'))[e % 3]


def test_the_staged_rules_are_those_of_the_references():
    rows_seen = 0
    for name in sc.names_of('events'):
        c = sc.events_case(name)
        geo, rows, good = c['geo'], c['pool_rows'], sc.in_range(c['geo'], c['pool_rows'])
        for kernel, rule, ref in (('landscape', sc.landscape_staged, lref.staged), ('alternatives', sc.alternatives_staged,
                                                                                      aref.staged)):
            mine = sc._paths(rule, geo, rows) == 's'
            assert np.array_equal(mine[good], ref(geo, rows[good, 2:])), (name, kernel)
            rows_seen += int(good.sum())
    assert rows_seen > 1000


# -- exactness -----------------------------------------------------------------------------------------------------------------
def test_every_reference_value_is_exact():
    """Times sc.DENOMINATOR every reference value of every case is an integer below 2^53, and within the mirror's bound."""
    for name in sc.names_of('events'):
        c = sc.events_case(name)
        t = time.perf_counter()
        for kernel in c['kernels']:
            for x in sc.events_reference(name, kernel):
                y = x * sc.DENOMINATOR
                assert np.array_equal(y, np.round(y)) and np.abs(y).max() <= sc.magnitude_bound(c['geo']) < 2 ** 53, (name, kernel)
        SLOWEST[name] = max(SLOWEST.get(name, 0.), time.perf_counter() - t)
        for x in (c['W'], c['V'], c['R']):
            assert np.array_equal(x, np.round(x)) and x.min() >= 0 and x.max() <= 3
        assert np.array_equal(2 * c['h'], np.round(2 * c['h'])) and c['h'].min() >= 0 and c['h'].max() <= 3
    for name in sc.norms_names():
        b = sc.norms_reference(sc.norms_geometry(name, 8), sc.dictionary(name, 8))
        assert np.array_equal(b, np.round(b)) and b.max() < 2 ** 53
    slow = max(SLOWEST, key=SLOWEST.get)
    print(f'the slowest case with its references is {slow!r}, {SLOWEST[slow]:.2f} s')
    # the planted zeros
    a, b, _ = sc.events_reference('zero-tap', 'pick')
    rows = sc.events_case('zero-tap')['pool_rows']
    corner = np.flatnonzero((rows == (0, 0, 0, 0)).all(axis=1))[0]
    assert b[corner] == 0 and not sc.dictionary('zero-tap')[2].any() and sc.dictionary('zero-tap')[0].any()


def test_the_norms_of_a_long_table_are_built_as_the_reference_tabulates_them():
    """The stride case's reference -- the ends of a small table of the same atom, the whole-plane norm between them -- against
    pursuit_reference.Table at a length small enough to tabulate."""
    W = sc.dictionary('norms-stride')
    for D in (25, 40, 200):
        geo = (1, 1, 1, (D,), (3,), 'valid')
        full = pur.Table(W, (D,), 'valid').norms()
        long_ = np.repeat(np.sum(W.reshape(1, -1) ** 2, axis=1)[:, None], D + 2, axis=1)
        small = pur.Table(W, (12,), 'valid').norms()
        long_[:, :6], long_[:, -6:] = small[:, :6], small[:, -6:]
        assert np.array_equal(full, long_), D
        assert np.array_equal(sc.norms_model(geo, W, 8).reshape(1, -1), full)
    big = sc.norms_reference(sc.norms_geometry('norms-stride', 8), W)
    assert big.shape == (1, 1, 8 * 2048 + 519) and np.array_equal(big[0, 0, :6], small[0, :6])
    assert np.all(big[0, 0, 2:-2] == big[0, 0, 6]) and big[0, 0, 0] < big[0, 0, 6]


# -- the models against the references, and the wrong models against the models ------------------------------------------------
def _differ(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return int(np.sum(~((x == y) | (np.isnan(x) & np.isnan(y)))))


@pytest.mark.parametrize('name', [n for n in sc.norms_names() if n != 'norms-stride'])
def test_the_norms_model_is_the_reference(name):
    geo, W = sc.norms_geometry(name), sc.dictionary(name)
    want = sc.norms_reference(geo, W)
    assert np.array_equal(sc.norms_model(geo, W), want)
    # the seams of the shortcut: on either side of one the model and the reference agree, and the table has both sides
    short = sc.norms_shortcut(geo)
    seams = int(np.sum(short[:, 1:] != short[:, :-1]) + np.sum(short[1:] != short[:-1]))
    assert seams > 0 or geo[5] == 'full' or name == 'widest-circular', name     # ('full': every shift is whole)


def test_wrong_norms_differ_on_the_cases_named_for_them():
    for name, defect, cu in (('norms-taps-300', 'first-256-taps', 256), ('norms-stride', 'one-entry-pass', 8),
                             ('norms-seams', 'far-side-shortcut', 256), ('widest-circular', 'separate-squares', 256),
                             ('widest-reflect', 'separate-squares', 256)):
        geo, W = sc.norms_geometry(name, cu), sc.dictionary(name, cu)
        want = sc.norms_reference(geo, W)
        n = _differ(sc.norms_model(geo, W, cu, defect), want)
        print(f'{name}: {defect} differs in {n} of {want.size} entries')
        assert n > 0, f'{name}: {defect} differs in {n} of {want.size} entries'
    geo, W = sc.norms_geometry('norms-stride', 8), sc.dictionary('norms-stride')
    assert _differ(sc.norms_model(geo, W, 8), sc.norms_reference(geo, W)) == 0
    assert _differ(sc.norms_model(geo, W, 8, 'one-entry-pass'), sc.norms_reference(geo, W)) == 517 + 2
    # the defect of the far side touches exactly the shifts that are clipped there and nowhere else
    geo = sc.norms_geometry('norms-seams')
    terms = sc.norms_terms(geo)
    far_only = (terms[3] | terms[4]) & ~terms[:3].any(axis=0)
    got = sc.norms_model(geo, sc.dictionary('norms-seams'), defect='far-side-shortcut')
    assert far_only.sum() > 0 and np.all((got != sc.norms_reference(geo, sc.dictionary('norms-seams')))[:, far_only])


@pytest.mark.parametrize('name', ['taps-65', 'widest-circular', 'zero-tap'])
def test_the_pick_model_is_the_reference_and_a_swapped_decode_differs(name):
    c = sc.events_case(name)
    geo, idx = c['geo'], sc.flat_indices(c['geo'], c['rows'])
    rows, a, b, mag = sc.pick_model(geo, c['W'], c['V'], c['R'], idx)
    want = tuple(x[c['pick']] for x in sc.events_reference(name, 'pick'))
    assert np.array_equal(a, want[0]) and np.array_equal(b, want[1]) and np.array_equal(mag, want[2])
    k = len(geo[4])
    good = c['good']
    assert np.array_equal(rows[good][:, [0, 1] + list(range(4 - k, 4))], c['rows'][good]) and np.all(rows[~good] == -1)
    wrong = sc.pick_decode(geo, idx, 'swapped-decode')
    n = int(np.sum((wrong != rows).any(axis=1)))
    assert n > 0, f'{name}: the swapped decode differs in {n} of {len(rows)} rows'
    print(f'{name}: the swapped decode differs in {n} of {len(rows)} rows')


def test_a_swapped_decode_differs_on_the_case_named_for_it():
    c = sc.events_case('stride-64', 8)
    geo, idx = c['geo'], sc.flat_indices(c['geo'], c['rows'])
    assert geo[0] != geo[2] and geo[2] & (geo[2] - 1)
    n = int(np.sum((sc.pick_decode(geo, idx, 'swapped-decode') != sc.pick_decode(geo, idx)).any(axis=1)))
    assert n > len(idx) // 2, f'the swapped decode differs in {n} of {len(idx)} rows'


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', sc.names_of('score'))
def test_the_score_model_is_the_numpy_expression(name, dt):
    """At 8 CUs: the walk covers every chunk of the map exactly once, and nothing else."""
    c = sc.score_case(name, dt, 8)
    plan = c['plan']
    N, P, Sy, Sx = plan['shape']
    walk = sc.score_walk(plan)
    visits = np.concatenate([r * plan['cpr'] + ch for r, ch, _, _, _ in walk])
    assert len(visits) == plan['rows'] * plan['cpr'] == len(np.unique(visits)) and visits.max() == len(visits) - 1
    for r, ch, br, _, _ in walk:
        assert np.all(ch < plan['cpr']) and np.array_equal(br, r % plan['brows'])
    store = np.full((N, P, Sy, plan['Hs0']), SENTINEL, dtype=sc.NP[dt])
    store[..., :Sx] = c['a']
    got = sc.score_model(store, c['b'], plan, SENTINEL).reshape(store.shape)
    assert got[..., :Sx].tobytes() == c['untaken'].tobytes() and np.all(got[..., Sx:] == SENTINEL)
    taken = sc.taken_model(got.reshape(-1), plan, c['taken'], 8).reshape(store.shape)
    assert taken[..., :Sx].tobytes() == c['want'].tobytes() and np.all(taken[..., Sx:] == SENTINEL)


def test_wrong_scores_differ_on_the_cases_named_for_them():
    for name, defect in (('score-lines-stride', 'end-chunk-whole'), ('score-lines-stride', 'no-chunk-carry'),
                         ('score-narrow', 'end-chunk-whole')):
        for dt in DTYPES:
            c = sc.score_case(name, dt, 8)
            plan = c['plan']
            N, P, Sy, Sx = plan['shape']
            store = np.full((N, P, Sy, plan['Hs0']), SENTINEL, dtype=sc.NP[dt])
            store[..., :Sx] = c['a']
            right = sc.score_model(store, c['b'], plan, SENTINEL)
            n = _differ(sc.score_model(store, c['b'], plan, SENTINEL, defect), right)
            print(f'{name} {dt}: {defect} differs in {n} of {right.size} elements')
            assert n > 0, f'{name} {dt}: {defect} differs in {n} of {right.size} elements'
    c = sc.score_case('taken-stride', 'f32', 8)
    flat = np.full(c['plan']['entries'] // c['plan']['Sx'] * c['plan']['Hs'], 1., dtype=np.float32)
    n = _differ(sc.taken_model(flat, c['plan'], c['taken'], 8, 'one-pass'), sc.taken_model(flat, c['plan'], c['taken'], 8))
    assert n == 5, f'a taken loop of one pass differs in {n} elements'


def test_the_landscape_model_is_the_reference_and_a_narrow_patch_differs():
    for name in ('landscape-limit-fits', 'stride-4', 'taps-65', 'one-tap'):
        c = sc.events_case(name)
        geo, rows, h = c['geo'], c['pool_rows'], c['pool_h']
        staged = np.flatnonzero(sc._paths(sc.landscape_staged, geo, rows) == 's')[:4]
        assert len(staged) >= 1, name
        want = sc.events_reference(name, 'landscape')
        differ = 0
        for e in staged:
            got = sc.landscape_staged_model(geo, c['W'], c['V'], c['R'], rows[e], h[e])
            assert all(np.array_equal(x, y[e]) for x, y in zip(got, want)), (name, e)
            wrong = sc.landscape_staged_model(geo, c['W'], c['V'], c['R'], rows[e], h[e], 'narrow-patch')
            differ += sum(_differ(x, y[e]) for x, y in zip(wrong, want))
        print(f'{name}: a patch indexed with Px = Ax + 1 differs in {differ} of {3 * len(staged) * want[0].shape[1]} sums')
        if len(geo[4]) == 2:
            assert differ > 0, f'{name}: a patch indexed with Px = Ax + 1 differs in {differ} sums'


def test_the_alternatives_model_is_the_reference_and_its_wrong_models_differ():
    for name, defect in (('one-tap', 'full-last-batch'), ('stride-4', 'full-last-batch'), ('taps-64', 'full-last-batch'),
                         ('zero-fill', 'fill-one-wave'), ('zero-tap', None), ('widest-circular', None)):
        c = sc.events_case(name, 8)
        geo, rows, h, n_alt = c['geo'], c['rows'], c['h'], c['n_alt']
        K = len(rows)
        want = tuple(x[c['pick']] for x in sc.events_reference(name, 'alternatives'))
        got = sc.alternatives_model(geo, c['W'], c['V'], c['R'], rows, h, n_alt, c['stride'])
        for x, y in zip(got, want):
            assert np.array_equal(x[:K * n_alt].reshape(K, n_alt), y) and np.isnan(x[K * n_alt:]).all(), name
        if defect:
            wrong = sc.alternatives_model(geo, c['W'], c['V'], c['R'], rows, h, n_alt, c['stride'], defect=defect)
            n = sum(_differ(x, y) for x, y in zip(wrong, got))
            print(f'{name}: {defect} differs in {n} of {3 * len(got[0])} elements')
            assert n > 0, f'{name}: {defect} differs in {n} of {3 * len(got[0])} elements'
    # the zero fill that stops at lane 63 leaves the candidates 64 and 65 of every refused row unwritten
    c = sc.events_case('zero-fill')
    wrong = sc.alternatives_model(c['geo'], c['W'], c['V'], c['R'], c['pool_rows'], c['pool_h'], 66, 1, defect='fill-one-wave')
    bad = ~sc.in_range(c['geo'], c['pool_rows'])
    assert bad.sum() == 6 and int(np.isnan(wrong[0][:len(bad) * 66]).sum()) == 2 * 6
