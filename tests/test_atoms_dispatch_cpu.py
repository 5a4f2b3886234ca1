"""CPU guard of tests/atoms_dispatch.py: its constants are those of atoms.h / atoms.hip, and the shapes of its matrix -- the
ones tests/test_hip_atom_gains.py runs -- reach every branch of the kernel.  Sources read as text; no GPU."""
import os
import re

import atoms_dispatch as ad
from conftest import ROOT

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')


def _flat(name):
    return re.sub(r'\s+', ' ', open(os.path.join(CSRC, name)).read())


def test_the_constants_are_the_kernels():
    h, hip = _flat('atoms.h'), _flat('atoms.hip')
    assert f'constexpr int kAtomThreads = {ad.THREADS};' in h and f'constexpr int kAtomPix = {ad.PIX};' in h
    assert f'constexpr int kAtomTileY = {ad.TILE_Y}, kAtomTileX = {ad.TILE_X};' in h
    assert 'constexpr int kAtomTile1D = kAtomThreads * kAtomPix;' in h
    assert f'constexpr int kAtomChannels = {ad.CHANNELS};' in h and f'constexpr int kAtomChunk = {ad.CHUNK};' in h
    assert f'constexpr int kStage = {ad.STAGE};' in hip and 'if (lds > 60 * 1024) return TNMF_E_UNSUPPORTED;' in hip
    for line in ('p.NB = cdiv(g.Ax, kAtomPix);', 'p.NBO = cdiv(g.Ax + 1, kAtomPix);', 'p.SW = p.TX + kAtomPix * p.NBO;',
                 'p.SH = p.TY + g.Ay - 1;', 'p.slots = p.tiles_y * p.tiles_x * p.chunks;',
                 'const bool pre_ok = nel <= kStage * kAtomThreads;', 'if (g.Dy == 1 && g.Ay == 1) {'):
        assert line in hip, line


def test_the_plan():
    p = ad.plan(1, (256, 256), (12, 12))
    assert (p['tiles_y'], p['tiles_x'], p['NB'], p['NBO'], p['SW'], p['SH'], p['slots']) == (16, 4, 3, 4, 80, 27, 64)
    p = ad.plan(5, (50,), (7,))
    assert (p['TY'], p['TX'], p['CH'], p['chunks'], p['NB'], p['NBO'], p['SW'], p['SH']) == (1, 1024, 4, 2, 2, 2, 1032, 1)


def test_the_matrix_reaches_every_branch():
    got = set()
    for name, case in ad.MATRIX.items():
        N, C, M, D, A, group = case
        assert M % group == 0 and ad.plan(C, D, A)['SH'] * ad.plan(C, D, A)['SW'] * 8 <= ad.LDS_LIMIT, name
        got |= ad.reached(*case)
    assert got == set(ad.BRANCHES), set(ad.BRANCHES) - got
    assert 'stage-loop' in ad.reached(*ad.MATRIX['tall-atom']) and 'atoms-flush-inside' in ad.reached(*ad.MATRIX['1d-many-atoms'])
    assert {'below-halo-y', 'below-halo-x', 'group-is-M'} <= ad.reached(*ad.MATRIX['below-halo'])
    assert {'ragged-y', 'ragged-x', 'several-tiles-y', 'several-tiles-x'} <= ad.reached(*ad.MATRIX['tile-plus-one'])
    assert ad.reached(*ad.MATRIX['one-tile']) >= {'one-tile', 'taps-shifted-run-extra', 'stage-registers', 'group-1'}
