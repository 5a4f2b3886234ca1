"""
CPU guard of tests/patches_dispatch.py: its constants are those of tnmf_amd/csrc/patches.h, patches.hip and the header, read
as text; the launch rules it mirrors are the ones the sources spell out; its cases reach every branch it names.  No GPU.
"""
import os
import re

import numpy as np

import patches_dispatch as pd
import patches_reference as pref
from conftest import ROOT
from tnmf_amd import _lib

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _flat(text):
    return re.sub(r'\s+', ' ', text)


def test_the_constants_are_those_of_the_sources():
    h, hip = _read(CSRC, 'patches.h'), _read(CSRC, 'patches.hip')
    header, events_h = _read(ROOT, 'include', 'tnmf_hip.h'), _read(CSRC, 'events.h')
    assert pd.PER_CU == int(re.search(r'#define TNMF_PATCHES_BLOCKS_PER_CU (\d+)', h).group(1))
    assert pd.BLOCK == int(re.search(r'constexpr int kMomentBlock = (\d+);', h).group(1))
    assert pd.DEPTH == int(re.search(r'constexpr int kMomentDepth = (\d+);', h).group(1))
    assert pd.STAGE_MAX == int(re.search(r'#define TNMF_PATCH_STAGE_MAX (\d+)', header).group(1)) == _lib.PATCH_STAGE_MAX
    assert pd.SEGMENT == int(re.search(r'#define TNMF_EVENTS_SEGMENT (\d+)', header).group(1)) == _lib.EVENT_SEGMENT
    assert pd.SEGMENT % pd.DEPTH == 0, 'the chunks of the backend begin where the MFMAs do'
    assert 'constexpr int kWaves = kEventThreads / 64;' in hip
    assert pd.WAVES * 64 == int(re.search(r'constexpr int kEventThreads = (\d+);', events_h).group(1))
    for name, code in _lib.PATCH_SOURCES.items():
        assert code == int(re.search(r'#define TNMF_PATCH_%s (\d+)' % name.upper(), header).group(1))
    assert tuple(_lib.PATCH_SOURCES) == pref.SOURCES


def test_the_launch_conventions():
    h, hip = _flat(_read(CSRC, 'patches.h')), _flat(_read(CSRC, 'patches.hip'))
    assert 'int events_patches(tnmf_hip_ctx *ctx, const EventFrame &f, ' in h
    assert hip.count('events_grid(') == 1
    assert 'events_grid(ctx, (n_events + kWaves - 1) / kWaves, TNMF_PATCHES_BLOCKS_PER_CU)' in hip
    assert hip.count(', s, g, f.mode, f.Sy, f.Sx, ') == 1
    assert 'k_events_patches<T>' in hip and 'k_events_patches<float>' not in hip and 'k_events_patches<double>' not in hip
    assert hip.count('with_dtype(') == 1
    assert 'for_each_tap(g, o, lane, 64, ' in hip and 'phi_at(g, o, w, c * AA, y, x)' in hip
    assert 'residual_without(V[at], R[at], hv, ' in hip and '#include "event_walk.h"' in hip
    assert not re.search(r'atomic\w*\s*\(', hip), 'no atomics'
    assert '__builtin_amdgcn_mfma_f64_16x16x4f64(ya[u], yb[u], acc, 0, 0, 0)' in hip
    assert 'const size_t lds = fold_ptr ? (size_t)kWaves * taps * sizeof(double) : 0;' in hip
    assert 'if (fold_ptr && !patches_stage_fits(taps)) return TNMF_E_GEOM;' in hip
    assert 'inline bool patches_stage_fits(long long taps) { return taps <= TNMF_PATCH_STAGE_MAX; }' in h
    assert 'const int nb = cdiv(D, kMomentBlock), pairs = nb * (nb + 1) / 2;' in hip
    assert 'r0 = b > a ? (a & ~(kMomentDepth - 1)) : b; r0 < b; r0 += kMomentDepth' in hip
    api = _flat(_read(CSRC, 'api.hip'))
    assert api.count('int tnmf_hip_events_patches(') == 1 and api.count('int tnmf_hip_patch_moments(') == 1
    assert 'patches.hip' in _read(CSRC, 'Makefile')


def test_the_mirror_of_the_launches():
    assert pd.patches_launch(0, 2, 1, (3, 4), False, 256) is None and pd.patches_launch(5, 0, 1, (3, 4), True, 256) is None
    assert pd.patches_launch(5, 2, 1, (3, 4), False, 256) == (2, 0)
    assert pd.patches_launch(5, 2, 3, (5, 5), True, 256) == (2, 4 * 75 * 8)
    assert pd.patches_launch(pd.GRID_STRIDE_ROWS, 2, 1, (5,), False, 256) == (256 * pd.PER_CU, 0)
    assert pd.patches_launch(5, 2, 1, (2049,), True, 256) == 'geom' and pd.patches_launch(5, 2, 1, (2048,), True, 256) != 'geom'
    assert pd.patches_launch(5, 2, 1, (2049,), False, 256) == (2, 0)
    assert pd.moments_launch(5, 6) == (1, 1, 6, 2) and pd.moments_launch(75, 6) == (5, 15, 90, 23)
    for nb in (1, 2, 5):
        pairs = [pd.block_pair(i, nb) for i in range(nb * (nb + 1) // 2)]
        assert pairs == [(I, J) for I in range(nb) for J in range(I, nb)]
    assert pd.fours(0, 0) == [] and pd.fours(5, 5) == [] and pd.fours(5, 6) == [4] and pd.fours(3, 9) == [0, 4, 8]
    assert pd.fours(4, 69) == list(range(4, 69, 4))


def test_the_cases_reach_every_branch():
    seen = set()
    for name, (N, C, P, D, A, mode, tables) in pd.PATCH_CASES.items():
        rows, h = pd.patch_rows(name)
        assert len(rows) == len(h) and (len(rows) <= 320 or name == 'grid-stride')
        assert np.array_equal(h, h.astype(np.float32).astype(np.float64)) and h.min() > 0
        mine = pd.launch_branches(len(rows), C, A, 256)
        for row in rows:
            mine |= pd.row_branches(N, C, P, D, A, mode, row)
        seen |= mine
        if name != 'grid-stride':
            assert 'row-out-of-range' in mine and (~pref.in_range(rows, N, P, pref.shift_shape(D, A, mode))).sum() == 7
            good = rows[pref.in_range(rows, N, P, pref.shift_shape(D, A, mode))]
            assert len(np.unique(good, axis=0)) < len(good), 'duplicates'
        if mode in ('circular', 'reflect') and len(D) == 2:
            assert {'two-images', 'four-images', 'single-whole'} <= mine, name
        if mode == 'valid':
            assert {'single-clipped', 'single-whole'} <= mine, name
        if mode == 'full':
            assert mine & set(pd.PATCH_BRANCHES) == {'row-out-of-range', 'single-whole', 'taps-below-64'}, name
        if mode == 'reflect':
            assert 'reflect-overlap' in mine, name
        for T in tables:
            assert P % {None: 1, 'T1': 1, 'flip': 2, 'rot90': 4, 'rot8': 8}[T] == 0
    assert seen >= set(pd.PATCH_BRANCHES), set(pd.PATCH_BRANCHES) - seen
    assert {len(D) for _, _, _, D, _, _, _ in pd.PATCH_CASES.values()} == {1, 2}
    assert {C for _, C, *_ in pd.PATCH_CASES.values()} >= {1, 3}
    assert {m for *_, m, _ in pd.PATCH_CASES.values()} == {'valid', 'full', 'circular', 'reflect'}
    assert {t for *_, ts in pd.PATCH_CASES.values() for t in ts} == {None, 'flip', 'rot90', 'rot8', 'T1'}
    got = set()
    for D in pd.MOMENT_D:
        got |= pd.moment_branches(D, pd.MOMENT_RUNS, with_bad_entry=D == 25)
    assert got == set(pd.MOMENT_BRANCHES)
