"""CPU guard of tests/atom_gram_dispatch.py: its constants are those of atom_gram.h / atom_gram.hip with the kernel text it
includes (atom_gram_kernel.h, atom_walk.h), and the shapes of its matrix -- the ones tests/test_hip_atom_gram.py runs -- reach
every branch of the kernel in both precisions.  Sources read as text; no GPU."""
import os
import re

import atom_gram_dispatch as gd
from conftest import ROOT

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')


def _flat(name):
    return re.sub(r'\s+', ' ', open(os.path.join(CSRC, name)).read())


def test_the_constants_are_the_kernels():
    # (the kernel is built from atom_gram.hip and the body, constants and aliases it includes)
    h, hip = _flat('atom_gram.h'), ' '.join(_flat(name) for name in ('atom_gram.hip', 'atom_gram_kernel.h', 'atom_walk.h'))
    assert 'constexpr int kGramTilePix = kAtomThreads * kAtomPix;' in h and gd.TILE_PIX == 1024
    assert f'constexpr int kGramStride = kGramTilePix + {gd.STRIDE - gd.TILE_PIX};' in h
    assert f'constexpr int kGramStripTiles = {gd.STRIP_TILES};' in h
    assert f'constexpr size_t kGramLds = {gd.LDS // 1024} * 1024;' in h
    assert f'constexpr int kStage = {gd.ad.STAGE};' in hip and 'constexpr int kWaves = kAtomThreads / 64;' in hip
    for line in ('p.ap = atom_terms_plan(g);', 'const size_t h_bytes = align_up((size_t)p.ap.SH * p.ap.SW * es, 32);',
                 'return ((size_t)cap * kGramStride + kGramTilePix) * es + halves * h_bytes + (size_t)cap * kWaves * '
                 'sizeof(double);',
                 'p.cap = Mo > 16 && lds_of(32, 1) <= kGramLds ? 32 : lds_of(16, 1) <= kGramLds ? 16 : 0;',
                 'p.halves = p.cap == 32 && lds_of(32, 2) <= kGramLds ? 2 : 1;',
                 'p.hb = p.cap / 2;', 'p.nbk = p.cap ? std::max(2, cdiv(Mo, p.hb)) : 2;',
                 'p.pairs = p.nbk * (p.nbk - 1) / 2;', 'p.strips = cdiv(p.tiles, kGramStripTiles);',
                 'p.wg_doubles = (size_t)p.cap * p.cap + p.cap;', 'if (p.cap == 0) return TNMF_E_UNSUPPORTED;',
                 'const bool pre_ok = nel <= kStage * kAtomThreads;',
                 '__builtin_amdgcn_mfma_f64_16x16x4f64(aop[bi], bop[bj], acc[u], 0, 0, 0);'):
        assert line in hip, line
    # no floating-point atomics: the sums are ordered
    assert 'atomic' not in hip.replace('No atomics', '')


def test_the_plan():
    p = gd.plan(1, 32, (256, 256), (12, 12), 1, 'f32')   # config 3
    assert (p['cap'], p['nbk'], p['pairs'], p['tiles'], p['strips']) == (32, 2, 1, 64, 4)
    assert p['halves'] == 2 and p['lds'] == (32 * 1040 + 1024) * 4 + 2 * 27 * 80 * 4 + 32 * 4 * 8 == 155520 <= gd.LDS
    assert 256 * p['strips'] * p['pairs'] * p['wg_doubles'] * 8 == 8650752          # partial sums: 8.25 MiB
    p = gd.plan(1, 32, (256, 256), (12, 12), 1, 'f64')
    assert (p['cap'], p['hb'], p['halves'], p['nbk'], p['pairs']) == (16, 8, 1, 4, 6) and p['lds'] == 159104 <= gd.LDS
    p = gd.plan(1, 32, (256, 256), (12, 12), 4, 'f32')   # 8 atoms x rot90
    assert (p['cap'], p['Mo'], p['pairs']) == (16, 8, 1)
    assert gd.plan(1, 1, (16, 16), (200, 200), 1, 'f64')['cap'] == 0      # 215 rows of 268 doubles of H: nothing fits
    assert gd.plan(1, 20, (16, 16), (70, 70), 1, 'f32')['cap'] == 16      # 85 x 136 floats of H: 16 atoms fit, 32 do not


def test_the_matrix_reaches_every_branch_in_both_precisions():
    for dt in ('f32', 'f64'):
        got = set()
        for name, case in (gd.ALL if dt == 'f32' else gd.MATRIX).items():
            N, C, M, D, A, group = case
            p = gd.plan(C, M, D, A, group, dt)
            assert M % group == 0 and p['cap'] and p['lds'] <= gd.LDS and N <= 3, name
            assert p['tiles'] <= 17 and gd.chain(C, M, D, A, group, dt) <= 2 ** 16, name
            got |= gd.reached(*case, dt)
        f32_only = {'cap-32', 'halves-2-even', 'halves-2-odd', 'cap-32-one-half'}   # (32 parked rows of doubles do not fit)
        want = set(gd.BRANCHES) - (f32_only if dt == 'f64' else set())
        assert got == want, (dt, want ^ got)
    r = lambda name, dt: gd.reached(*gd.ALL[name], dt)   # noqa: E731
    assert {'cap-32', 'several-pairs', 'last-block-ragged'} <= r('atoms-33', 'f32')
    assert {'cap-16', 'several-pairs', 'last-block-ragged'} <= r('atoms-33', 'f64')
    assert {'cap-32', 'one-pair-both-blocks', 'mfma-rows-ragged', 'halves-2-odd'} <= r('atoms-17', 'f32')
    assert {'halves-2-even', 'halves-2-odd'} <= r('atoms-33', 'f32') and 'cap-32-one-half' in r('wide-atom-20', 'f32')
    assert gd.plan(*gd.F32_ONLY['wide-atom-20'][1:], 'f64')['cap'] == 0
    assert {'cap-16', 'several-pairs'} <= r('atoms-17', 'f64')
    assert {'cap-16', 'one-pair-both-blocks', 'mfma-rows-full'} <= r('atoms-16', 'f32')
    assert {'cap-32', 'mfma-rows-full'} <= r('atoms-32', 'f32') and 'several-pairs' in r('atoms-32', 'f64')
    assert {'several-strips', 'strip-ragged', 'group-is-M'} <= r('strip-boundary', 'f32')
    assert {'several-strips', 'strip-ragged', 'tile-1d'} <= r('1d-strip-boundary', 'f64')
    assert 'stage-loop' in r('tall-atom', 'f32') and {'below-halo-y', 'below-halo-x'} <= r('below-halo', 'f32')
    assert gd.plan(1, 33, (9, 70), (3, 4), 1, 'f32')['pairs'] == 3 and gd.plan(1, 33, (9, 70), (3, 4), 1, 'f64')['pairs'] == 10
