"""
The host mirror of the triggered-sums launch (tests/triggered_dispatch.py) without a GPU: its constants and formulas are
those of tnmf_amd/csrc/triggered.h / triggered.hip read as text, and its cases cross every edge it names.
"""
import os
import re

import triggered_dispatch as td
from conftest import ROOT


def _flat(name):
    return re.sub(r'\s+', ' ', open(os.path.join(ROOT, 'tnmf_amd', 'csrc', name)).read())


def test_the_constants_are_the_kernels():
    h, hip = _flat('triggered.h'), _flat('triggered.hip')
    for name, value in (('kTrigThreads', td.THREADS), ('kTrigBlock', td.BLOCK), ('kTrigChunk', td.CHUNK),
                        ('kTrigTile1Float', td.TILE1['f32']), ('kTrigTile1Double', td.TILE1['f64']), ('kTrigTileX', td.TILE_X),
                        ('kTrigTileYFloat', td.TILE_Y['f32']), ('kTrigTileYDouble', td.TILE_Y['f64']), ('kTrigPad', td.PAD),
                        ('kTrigMaxWindow1', td.MAX_WINDOW[1]), ('kTrigMaxWindow2', td.MAX_WINDOW[2]),
                        ('kTrigTargetGroups', td.TARGET_GROUPS)):
        assert f'constexpr int {name} = {value};' in h, name
    assert f'constexpr size_t kTrigPartialCap = (size_t){td.PARTIAL_CAP >> 20} << 20;' in h
    for line in ('p.Wy = Ay + 2 * my, p.Wx = Ax + 2 * mx;', 'p.offy = -(Ay - 1) - my, p.offx = -(Ax - 1) - mx;',
                 'p.TY = ndim == 1 ? 1 : dtype == 0 ? kTrigTileYFloat : kTrigTileYDouble;',
                 'p.TX = ndim == 2 ? kTrigTileX : dtype == 0 ? kTrigTile1Float : kTrigTile1Double;',
                 'p.nbp = cdiv(P, kTrigBlock);', 'p.nxb = cdiv(p.Wx, kTrigBlock);', 'p.cells = F * p.Wy * p.nxb;',
                 'p.CB = std::min(p.nxb, kTrigChunk);', 'p.CJ = std::min(p.Wy, kTrigChunk / p.CB);', 'p.CJ = cdiv(p.Wy, cdiv(p.Wy, p.CJ));',
                 'p.YC = p.TX + kTrigBlock * p.CB;', 'p.chunks_x = cdiv(p.nxb, p.CB);', 'p.chunks_y = cdiv(p.Wy, p.CJ);',
                 'p.CF = std::min(F, kTrigChunk / (p.CB * p.CJ));', 'p.chunks_f = cdiv(F, p.CF);',
                 'p.chunks = p.chunks_f * p.chunks_y * p.chunks_x;', 'p.split = p.CF * p.CJ * p.CB < kWaves ? 1 : 0;',
                 'const long long want = (kTrigTargetGroups + units - 1) / units;',
                 'p.ipg = std::max<long long>(1, (p.seglen + strips - 1) / strips);',
                 'p.strips = (int)std::max<long long>(1, (p.seglen + p.ipg - 1) / p.ipg);',
                 'p.lds = ((size_t)p.TY * kTrigBlock * (p.TX + kTrigPad) + (size_t)p.CF * (p.TY + p.CJ - 1) * p.YC) * esize(dtype);',
                 'return align_up((size_t)p.nseg * p.strips * p.nbp * p.cells * 256 * sizeof(double), 256);',
                 'const int e = kTrigChunk / (cb * cj) * (TY + cj - 1) * (TX + kTrigBlock * cb);',
                 'for (int j = 0; j < NV; ++j) b[j] = (double)yrow[4 * gx + boff[j]];',
                 'acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[j], acc[j], 0, 0, 0);'):
        assert line in hip, line
    assert 'atomic' not in hip.replace('No atomics', '')   # the sums are ordered
    # the work buffer is the caller's: neither file names a buffer of the context
    assert not re.search(r'ctx->|ensure_', h + hip)
    from tnmf_amd import _lib
    assert _lib.TRIGGERED_MAX_WINDOW == td.MAX_WINDOW
    # the limits admit what the interface promises
    assert td.MAX_WINDOW[1] >= 2048 and td.MAX_WINDOW[2] >= 64


def test_the_plan():
    p = td.plan(256, 32, 1, (256, 256), (12, 12), (6, 6), False, 'f32')   # config 3, the default margin: window 24 x 24
    assert (p['Sy'], p['Wy'], p['Wx'], p['nbp'], p['nxb'], p['cells']) == (267, 24, 24, 2, 2, 48)
    assert (p['CB'], p['CJ'], p['chunks'], p['split']) == (2, 12, 2, 0)
    assert (p['tiles'], p['strips'], p['ipg']) == (67 * 5, 511, 168) and p['groups'] == 511 * 4
    assert p['work_bytes'] == 511 * 2 * 48 * 2048 and p['lds'] <= 64 * 1024
    p = td.plan(256, 32, 1, (256, 256), (12, 12), (0, 0), False, 'f32')   # margin 0: one chunk of 12 cells
    assert (p['cells'], p['CB'], p['CJ'], p['chunks']) == (12, 1, 12, 1)
    p = td.plan(2, 3, 1, (37,), (5,), (0,), False, 'f32')                # one cell: the waves split the pixels
    assert (p['cells'], p['split'], p['chunks']) == (1, 1, 1)
    for dt in ('f32', 'f64'):
        for D, A, m in (((3000,), (8,), (1020,)), ((40, 40), (8, 8), (28, 28)), ((40, 40), (8, 8), (60, 60)), ((40, 40), (2, 100), (31, 0))):
            p = td.plan(2, 3, 2, D, A, m, False, dt)
            assert p['lds'] <= 64 * 1024
            assert p['patch'] <= td.patch_max(p['TY'], p['TX'])          # the register stage of the patch holds it
            cells = td.cells_computed(p)                                  # every cell, once
            assert sorted(cells) == [(f, jy, jxb) for f in range(2) for jy in range(p['Wy']) for jxb in range(p['nxb'])]
            assert all(len(td.chunk_cells(p, c)) <= td.CHUNK for c in range(p['chunks']))
    assert td.plan(0, 3, 1, (9, 11), (3, 4), (1, 1), False, 'f32')['work_bytes'] == 0


def test_the_matrix_reaches_every_branch_in_both_precisions():
    for dt in ('f32', 'f64'):
        got = set()
        for name, case in td.MATRIX.items():
            for per_sample in (False, True):
                p = td.plan(*case, per_sample, dt)
                assert p['lds'] <= 64 * 1024 and p['groups'] <= 40000 and p['work_bytes'] <= 128 << 20, name
                got |= td.reached(*case, per_sample, dt)
        assert got == set(td.BRANCHES), (dt, set(td.BRANCHES) ^ got)
    r = lambda name, per, dt: td.reached(*td.MATRIX[name], per, dt)   # noqa: E731
    assert 'split' in r('1d-window-is-atom', False, 'f32') and 'split' in r('2d-window-is-atom', False, 'f64')
    assert {'cell-ragged', 'blocks-several', 'last-block-ragged', 'fields-several'} <= r('1d-window-34', False, 'f32')
    assert 'window-wider-than-sample' in r('1d-window-wider-than-sample', False, 'f32')
    assert 'no-sample' in r('2d-no-sample', False, 'f32')
    assert 'chunks-several-y' in r('2d-chunks-y', False, 'f32') and 'cell-full' in r('2d-chunks-y', False, 'f32')
    assert 'chunks-several-x' in r('1d-chunks-x', False, 'f64')
    assert {'waves-idle', 'chunk-ragged'} <= r('2d-last-chunk-small', False, 'f32')
    assert {'chunk-several-fields', 'chunks-several-f', 'chunk-fields-ragged'} <= r('1d-fields-ragged', False, 'f32')
    assert 'chunk-several-fields' in r('1d-window-34', False, 'f64')
    assert 'last-block-full' in r('2d-planes-16', False, 'f32') and 'blocks-several' in r('2d-planes-32', False, 'f64')
    for dt in ('f32', 'f64'):
        assert {'strip-several-items', 'strip-ragged', 'strip-straddles-samples'} <= r('strips-several-items', False, dt)
        assert {'strips-several', 'per-sample'} <= r('strips-several-items', True, dt)
    assert 'x-below-tile' in r('1d-255', False, 'f32') and 'x-below-tile' in r('1d-127', False, 'f64')
    assert 'x-above-tile' in r('1d-257', False, 'f32') and 'x-above-tile' in r('1d-129', False, 'f64')
    assert 'y-below-tile' in r('2d-3x63', False, 'f32') and 'y-below-tile' in r('2d-1x63', False, 'f64')
    assert 'y-above-tile' in r('2d-5x65', False, 'f32') and 'y-above-tile' in r('2d-5x65', False, 'f64')
