"""
CPU guard of the events kernel matrix: the host mirror of k_events_render, k_events_update, k_events_grad_W and
k_events_grad_W_sum (tests/events_dispatch.py) is held to the sources it restates, and the cases of
tests/test_hip_events_matrix.py are held to executing every named branch of the four kernels, each item of the list the
matrix was built for (R1-R5, U1-U3, G1-G3) through a case named for it.  No GPU, no build: the sources are read as text.
"""
import os
import re

import numpy as np
import pytest

import events_dispatch as ed
import events_reference as eref
import test_hip_events as old
import test_hip_events_matrix as gm
import test_hip_events_w as old_w
from conftest import ROOT
from tnmf_amd import _lib

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


# -- the mirror against the sources ---------------------------------------------------------------------------------------------
def test_constants_are_those_of_the_sources():
    events_h, events_hip, header = _read(CSRC, 'events.h'), _read(CSRC, 'events.hip'), _read('include', 'tnmf_hip.h')
    assert ed.THREADS == int(re.search(r'constexpr int kEventThreads = (\d+);', events_h).group(1))
    assert ed.CHAN == int(re.search(r'constexpr int kChan = (\d+);', events_hip).group(1))
    assert 'constexpr int kWaves = kEventThreads / 64;' in events_hip and ed.WAVES == ed.THREADS // 64
    assert ed.SEGMENT == int(re.search(r'#define TNMF_EVENTS_SEGMENT (\d+)', header).group(1)) == _lib.EVENT_SEGMENT
    assert ed.CELL_1D == int(re.search(r'#define TNMF_EVENTS_CELL_1D (\d+)', header).group(1))
    assert ed.CELL_2D == int(re.search(r'#define TNMF_EVENTS_CELL_2D (\d+)', header).group(1))
    assert _lib.EVENT_CELLS == {1: ed.events_tile(1)[1:], 2: ed.events_tile(2)}
    assert ed.CELL_2D ** 2 == ed.THREADS == ed.CELL_1D


def test_mirrored_rules_are_those_of_the_sources():
    """The lines the mirror restates.  When one of them changes, tests/events_dispatch.py and the cases of the matrix have
    to be looked at again."""
    src = _read(CSRC, 'events.hip')
    for line in ('for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {',
                 'const bool inside = y < g.Dy && x < g.Dx;',
                 'const int cy1 = min((tile_y * g.ty + g.ty + g.Ay - 2) / g.ty, g.ncy - 1);',
                 'const int cx1 = min((tile_x * g.tx + g.tx + g.Ax - 2) / g.tx, g.ncx - 1);',
                 'for (int c0 = 0; c0 < g.C; c0 += kChan) {',
                 'for (int cy = tile_y; cy <= cy1; ++cy) {',
                 'const int i0 = max(cell_start[row + tile_x], 0), i1 = min(cell_start[row + cx1 + 1], n_images);',
                 'for (int base = i0; base < i1; base += kEventThreads) {',
                 'if (c0 + cc < g.C) acc[cc] += hv * w[(size_t)cc * AA];',
                 'for (long long e = (long long)blockIdx.x * kWaves + wave; e < n_events; e += (long long)gridDim.x * kWaves) {',
                 'const int ns = (c + TNMF_EVENTS_SEGMENT - 1) / TNMF_EVENTS_SEGMENT;',
                 'count = min(TNMF_EVENTS_SEGMENT, a + c - first);',
                 'const int L = max(1, kEventThreads / taps);   // sub-lanes per tap',
                 'for (int t0 = 0; t0 < taps; t0 += kEventThreads) {',
                 'const bool active = t < taps && sub < L;',
                 'for (int i = sub; i < count; i += L) {',
                 'const int chunks = (taps + kEventThreads - 1) / kEventThreads;',
                 # (the grid rule lives in events.h, below; per_cu is its default here)
                 'const unsigned grid = events_grid(ctx, (long long)g.N * nty * ntx);',
                 'const unsigned grid = events_grid(ctx, (n_events + kWaves - 1) / kWaves);',
                 'long long events_grad_W_slabs(long long n_events, int P) { return n_events / TNMF_EVENTS_SEGMENT + P; }',
                 'dim3((unsigned)n_slabs), dim3(kEventThreads)',
                 'const dim3 grid((unsigned)((long long)cdiv(taps, kEventThreads) * g.P));'):
        assert line in src, line
    assert src.count('const unsigned grid = events_grid(ctx, (n_events + kWaves - 1) / kWaves);') == 2   # update, gain
    events_h = _read(CSRC, 'events.h')
    for line in ('inline unsigned events_grid(const tnmf_hip_ctx *ctx, long long blocks, int per_cu = 64) {',
                 'return (unsigned)std::max<long long>(1, std::min<long long>(blocks, (long long)ctx->num_cu * per_cu));'):
        assert line in events_h, line
    # the occurrence walk the wave kernels share: the image table and the lane loop, and one call per wave kernel with a
    # lane's first tap and stride
    walk, modes = _read(CSRC, 'event_walk.h'), _read(CSRC, 'modes.h')
    for line in ('if (mode == TNMF_MODE_CIRCULAR && u >= S - (a - 1)) {',
                 'if (mode == TNMF_MODE_REFLECT && u >= 1 && u <= a - 1) {'):
        assert modes.count(line) == 1, line   # (axis_images: the image table, in modes.h and nowhere else)
    assert '#include "modes.h"' in walk and 'TNMF_MODE_' not in walk and 'axis_images(mode, u, ' not in walk
    assert 'for (int t = first; t < taps; t += step) {' in walk
    assert src.count('for_each_tap(g, o, lane, 64, [&](int t, int c, int y, int x) {') == 2   # k_events_update, k_events_gain
    assert src.count('for_each_tap(') == 2 and 'axis_images(mode, u' not in src
    api = _read(CSRC, 'api.hip')
    for line in ('g->ncy = cdiv(g->Dy + g->Ay - 1, g->ty), g->ncx = cdiv(g->Dx + g->Ax - 1, g->tx);',
                 'if (!mode_known(mode)) return TNMF_E_GEOM;',
                 'S[0] = mode_shift_len(mode, g.Dy, g.Ay), S[1] = mode_shift_len(mode, g.Dx, g.Ax);',
                 'return mode_axis_ok(mode, S[0], g.Ay) && mode_axis_ok(mode, S[1], g.Ax) ? TNMF_OK : TNMF_E_GEOM;'):
        assert line in api, line
    for line in ('return mode == TNMF_MODE_VALID ? D + a - 1 : (mode == TNMF_MODE_FULL ? D - a + 1 : D);',
                 'return S >= 1 && (mode != TNMF_MODE_CIRCULAR || a - 1 <= S) && (mode != TNMF_MODE_REFLECT || a - 1 < S);'):
        assert modes.count(line) == 1, line
    backend = _read('tnmf_amd', 'backends', 'HIP.py')
    for line in ('nc = [-(-(d + a - 1) // c) for d, a, c in zip(self._sample_shape, self.atom_shape, cells)]',
                 "key = key * nc[i] + torch.div(q[:, i], cells[i], rounding_mode='floor')",
                 'workspace = torch.empty((K // _lib.EVENT_SEGMENT + n_planes) * 2 * taps, dtype=torch.float64,'):
        assert line in backend, line


def _cases():
    """name -> (geometry, sample, plane, shift): the matrix, then the cases the suite had before it."""
    out = {name: ed.matrix_case(name)[:4] for name in ed.MATRIX}
    for name in old.CASES:
        out['old:' + name] = old.case(name)[:4]
    for name in old_w.OWN:
        out['old:' + name] = old_w.wcase(name)[:4]
    return out


@pytest.mark.parametrize('name', list(ed.MATRIX) + ['old:circular', 'old:reflect', 'old:full', 'old:1d', 'old:few-taps'])
def test_the_image_table_is_the_references(name):
    """The mirror's images per event are those of tests/events_reference.py (which the kernels are held to)."""
    geo, sample, plane, shift = _cases()[name]
    N, C, P, D, A, mode = geo
    S = eref.shift_shape(D, A, mode)
    assert ed.shift_shape(geo)[-len(S):] == tuple(S)
    ny, nx, images = ed.image_table(geo, shift)
    rows = np.arange(len(sample)) if len(sample) <= 2000 else np.arange(0, len(sample), 37)
    mine = {}
    for e, qy, qx in images.tolist():
        mine.setdefault(e, []).append((qy, qx) if len(A) == 2 else (qx,))
    for e in rows.tolist():
        want = eref.images(shift[e], A, S, mode)
        assert sorted(mine[e]) == sorted(want) and ny[e] * nx[e] == len(want), (name, e)


# -- the matrix against the mirror ----------------------------------------------------------------------------------------------
def test_the_cases_together_reach_every_branch():
    """The union over the matrix and the earlier cases is the full list of names, kernel by kernel."""
    union = {kernel: set() for kernel in ed.BRANCHES}
    for geo, sample, plane, shift in _cases().values():
        for kernel, names in ed.reached(geo, sample, plane, shift).items():
            union[kernel] |= names
    for kernel, names in ed.BRANCHES.items():
        assert union[kernel] == set(names), (kernel, sorted(set(names) - union[kernel]))


def test_every_new_item_is_reached_by_a_case_named_for_it():
    """Each name that stands for R1-R5, U1-U3, G1-G3 is claimed by at least one case of the matrix, every case reaches what
    it claims, and no earlier case reached it (or the matrix would not have needed the case)."""
    claimed = {kernel: {} for kernel in ed.BRANCHES}
    for name, (_, claims) in ed.MATRIX.items():
        geo, sample, plane, shift = ed.matrix_case(name)[:4]
        got = ed.reached(geo, sample, plane, shift)
        assert claims, name
        for kernel, names in claims.items():
            for b in names:
                assert b in ed.NEW[kernel], (name, kernel, b)
                assert b in got[kernel], f'{name} no longer reaches {kernel}: {b}'
                claimed[kernel].setdefault(b, []).append(name)
    for kernel, names in ed.NEW.items():
        for b in names:
            assert claimed[kernel].get(b), f'no case of the matrix is named for {kernel}: {b}'
    assert {b[:2] for names in ed.NEW.values() for b in names} == {f'{k}{i}' for k, n in (('R', 5), ('U', 3), ('G', 3))
                                                                   for i in range(1, n + 1)}
    before = {kernel: set() for kernel in ed.BRANCHES}
    for name, (geo, sample, plane, shift) in _cases().items():
        if name.startswith('old:'):
            for kernel, names in ed.reached(geo, sample, plane, shift).items():
                before[kernel] |= names
    for kernel, names in ed.NEW.items():
        # (idle lanes in the update were reached through 'few-taps' of the W tests, whose gradient tests do not run the
        # update on integers; samples narrower than a tile through the 8 x 9 sample of 'full-atom-as-large-as-the-sample',
        # the complement of R5's whole tiles; a plane of whole segments in front of another by the accident of a draw: plane 1
        # of '2d-valid' happens to hold 64 of its events)
        assert before[kernel] & set(names) <= {'U1:idle-lanes', 'R5:narrower-than-a-tile', 'G3:whole-segments-then-a-plane',
                                               'G3:offset-crosses-whole-segments'}, (kernel, before[kernel])


def test_the_quoted_figures():
    """What the comments of the matrix say about its cases."""
    geo, sample, plane, shift = ed.matrix_case('pile-up')[:4]
    counts = ed.cell_counts(geo, sample, shift)
    assert counts.shape == (1, 2, 2) and counts[0, 0].sum() == 600 and counts[0, 1].sum() == 0     # 256 + 256 + 88
    assert np.array_equal(ed.plane_counts(*[ed.matrix_case('empty-planes')[i] for i in (0, 2)]), ed.EMPTY_PLANES_COUNTS)
    for name, taps, L in (('tall-atom', 2160, 1), ('long-atom-1d', 300, 1), ('one-tap', 1, 256), ('taps-128', 128, 2),
                          ('taps-256', 256, 1), ('channels', 144, 1)):
        N, C, P, D, A, mode = ed.geometry_of(name)
        assert C * int(np.prod(A)) == taps and ed.sub_lanes(taps) == L, name
    for mode, name in (('circular', 'widest-circular'), ('reflect', 'widest-reflect')):
        geo, sample, plane, shift = ed.matrix_case(name)[:4]
        ny, nx, _ = ed.image_table(geo, shift)
        assert geo[5] == mode and np.any(ny * nx == 4)
        assert np.all(ny == 2) if mode == 'circular' else np.all((ny == 2) == (shift[:, 0] >= 1))


@pytest.mark.parametrize('num_cu', [64, 256, 304])
def test_the_stride_cases_stride_on_any_cu_count(num_cu):
    for name, kernel, branch in (('many-tiles', 'render', 'R4:tile-loop-strides'),
                                 ('many-events', 'update', 'U2:event-loop-strides')):
        geo, sample, plane, shift = ed.matrix_case(name, num_cu)[:4]
        assert branch in ed.reached(geo, sample, plane, shift, num_cu)[kernel]
        assert branch not in ed.reached(geo, sample, plane, shift, 2 * num_cu)[kernel]
    geo, sample, _, _ = ed.matrix_case('many-tiles', num_cu)[:4]
    assert sample.max() == geo[0] - 1 and np.count_nonzero(sample >= num_cu * 64) >= 37   # the second round has events


@pytest.mark.parametrize('name', list(ed.MATRIX))
def test_the_integer_problems_are_exact_in_both_element_types(name):
    """Distinct events, integer operands, a render below 2^20 and a gradient below 2^52 (asserted where they are built)."""
    geo, sample, plane, shift, h, W = ed.matrix_case(name)
    rows = np.column_stack([sample, plane, shift])
    assert len(np.unique(rows, axis=0)) == len(rows)
    assert not np.array_equal(rows, rows[np.lexsort(rows.T[::-1])]), 'given in shuffled order'
    assert set(np.unique(h)) <= {1., 2., 3., 4.} and set(np.unique(W)) <= {0., 1., 2., 3.}
    V, R, want = gm.integer_problem(name)
    assert np.array_equal(R, np.round(R)) and np.array_equal(want, np.round(want))
    assert R.max() < 2 ** 20 and want.max() < 2 ** 52 and set(np.unique(V)) <= {0., 1., 2., 3.}
