"""
Host mirror of the launch of tnmf_amd/csrc/atom_gram.hip (k_atom_taps, k_atom_gram, k_atom_gram_finalize), restated in plain
Python in the manner of tests/atoms_dispatch.py, so that tests/test_hip_atom_gram.py can choose the smallest problems that
execute every branch of the kernel and tests/test_atom_gram_dispatch_cpu.py can check without a GPU that the choice covers
them.  The pixel tile, the halo and the tap runs are those of atoms_dispatch.plan().
"""
import atoms_dispatch as ad
from atoms_dispatch import cdiv

TILE_PIX = ad.THREADS * ad.PIX   # atom_gram.h, kGramTilePix: pixels of a tile
STRIDE = TILE_PIX + 16           # kGramStride: elements per parked row
STRIP_TILES = 16                 # kGramStripTiles: tiles whose sums stay in one workgroup's accumulators
LDS = 160 * 1024                 # kGramLds
WAVES = ad.THREADS // 64
ESIZE = {'f32': 4, 'f64': 8}


def align_up(x, a):
    return cdiv(x, a) * a


def plan(C, M, D, A, group, dt):
    """atom_gram_plan: the plan of atoms_dispatch plus dict(cap, hb, halves, nbk, pairs, tiles, strips, lds, wg_doubles)."""
    p = ad.plan(C, D, A)
    Mo, es = M // group, ESIZE[dt]
    h_bytes = align_up(p['SH'] * p['SW'] * es, 32)

    def lds_of(cap, halves):
        return (cap * STRIDE + TILE_PIX) * es + halves * h_bytes + cap * WAVES * 8

    cap = 32 if Mo > 16 and lds_of(32, 1) <= LDS else 16 if lds_of(16, 1) <= LDS else 0
    halves = 2 if cap == 32 and lds_of(32, 2) <= LDS else 1   # two halves of 256 threads build different atoms at once
    p.update(cap=cap, hb=cap // 2, Mo=Mo, halves=halves)
    p['nbk'] = max(2, cdiv(Mo, p['hb'])) if cap else 2
    p['pairs'] = p['nbk'] * (p['nbk'] - 1) // 2
    p['tiles'] = p['tiles_y'] * p['tiles_x']
    p['strips'] = cdiv(p['tiles'], STRIP_TILES)
    p['lds'] = lds_of(cap, halves)
    p['wg_doubles'] = cap * cap + cap
    return p


def chain(C, M, D, A, group, dt):
    """The longest chain of double additions behind one entry of B: 256 products per wave, tile and channel over the strip
    (128 with two halves), the waves, the strips."""
    p = plan(C, M, D, A, group, dt)
    waves = WAVES * p['halves']
    return TILE_PIX // waves * min(p['tiles'], STRIP_TILES) * C + waves + p['strips']


BRANCHES = (
    'tile-1d', 'tile-2d',
    'one-tile', 'several-tiles-one-strip', 'several-strips',   # the accumulators live over one tile / several; the finalize adds
    'strip-ragged',                                            # the last strip has fewer tiles than the others
    'ragged-y', 'ragged-x',                                    # pixels of the last tile outside the sample
    'below-halo-y', 'below-halo-x',                            # D < A - 1: the tile's rows / columns of H end inside the halo
    'channels-1', 'channels-several',                          # the channel loop: one trip, more
    'taps-shifted-run-extra', 'taps-runs-equal',               # NBO == NB + 1 (Ax a multiple of 4) / NBO == NB
    'stage-registers', 'stage-loop',                           # SH * SW <= kStage * 256 or not
    'group-1', 'group-several', 'group-is-M',
    'cap-16', 'cap-32',                                        # one 16 x 16 block of atom pairs per wave, or three
    'halves-1', 'halves-2-even', 'halves-2-odd',               # 256 threads; 512 in two halves, and one half idle on the last atom
    'cap-32-one-half',                                         # 32 rows fit, a second tile of H does not
    'one-pair-second-block-empty', 'one-pair-both-blocks',     # Mo <= cap / 2; cap / 2 < Mo <= cap
    'several-pairs', 'last-block-ragged',                      # Mo > cap: the walk over pairs of blocks; Mo % (cap / 2) != 0
    'mfma-rows-ragged', 'mfma-rows-full',                      # parked rows that stay zero next to live ones, or none
)


def reached(N, C, M, D, A, group, dt):
    p = plan(C, M, D, A, group, dt)
    Dy, Dx = (1, D[0]) if len(D) == 1 else D
    Ay, Ax = (1, A[0]) if len(A) == 1 else A
    Mo = p['Mo']
    out = {'tile-1d' if p['TY'] == 1 else 'tile-2d'}
    out.add('one-tile' if p['tiles'] == 1 else 'several-tiles-one-strip' if p['strips'] == 1 else 'several-strips')
    if p['strips'] > 1 and p['tiles'] % STRIP_TILES:
        out.add('strip-ragged')
    if Dy % p['TY']:
        out.add('ragged-y')
    if Dx % p['TX']:
        out.add('ragged-x')
    if Ay > 1 and Dy < Ay - 1:
        out.add('below-halo-y')
    if Dx < Ax - 1:
        out.add('below-halo-x')
    out.add('channels-1' if C == 1 else 'channels-several')
    out.add('taps-shifted-run-extra' if p['NBO'] > p['NB'] else 'taps-runs-equal')
    out.add('stage-registers' if p['SH'] * p['SW'] <= ad.STAGE * ad.THREADS else 'stage-loop')
    out.add('group-1' if group == 1 else 'group-is-M' if group == M else 'group-several')
    out.add(f'cap-{p["cap"]}')
    nbk, hb = p['nbk'], p['hb']
    staged = {min(hb, Mo - i * hb) + max(0, min(hb, Mo - j * hb)) for i in range(nbk) for j in range(i + 1, nbk)}
    if p['halves'] == 1:
        out.add('halves-1')
        if p['cap'] == 32:
            out.add('cap-32-one-half')
    else:
        out |= {'halves-2-odd' if k % 2 else 'halves-2-even' for k in staged}
    if Mo <= p['hb']:
        out.add('one-pair-second-block-empty')
    elif Mo <= p['cap']:
        out.add('one-pair-both-blocks')
    else:
        out.add('several-pairs')
        if Mo % p['hb']:
            out.add('last-block-ragged')
    out.add('mfma-rows-full' if Mo % p['cap'] == 0 else 'mfma-rows-ragged')
    assert out <= set(BRANCHES), out - set(BRANCHES)
    return out


# name -> (N, C, M, D, A, group): the smallest shapes that reach every branch, in float32 and in float64 (a parked row of
# doubles is twice the bytes: 16 atoms per workgroup, so 17 and 33 atoms walk 3 and 10 pairs of blocks there)
MATRIX = {
    'one-tile': (2, 1, 3, (16, 64), (3, 4), 1),
    'tile-plus-one': (2, 3, 3, (17, 65), (5, 5), 1),          # ragged in both, four tiles, three channels
    'tile-plus-one-y': (2, 1, 6, (17, 64), (3, 4), 2),        # group 2 of M = 6
    'tile-plus-one-x': (2, 1, 2, (16, 65), (3, 3), 1),
    'tile-minus-one': (3, 1, 5, (15, 63), (3, 4), 5),         # group equals M: one atom
    'below-halo': (2, 3, 4, (3, 2), (5, 5), 2),
    'atom-12x12': (2, 1, 8, (20, 70), (12, 12), 4),           # group 4 of M = 8
    'tall-atom': (2, 1, 3, (9, 10), (20, 8), 1),              # 35 x 76 elements of H per tile: beyond the register stage
    'channels-5': (2, 5, 3, (9, 10), (3, 4), 1),
    'atoms-16': (2, 1, 16, (9, 10), (3, 4), 1),               # exactly one block of the matrix cores
    'atoms-17': (2, 1, 17, (17, 65), (3, 3), 1),              # two blocks, one atom in the second (float64: three pairs)
    'atoms-32': (1, 1, 32, (9, 10), (3, 3), 1),               # float32: every parked row live
    'atoms-33': (2, 1, 33, (9, 70), (3, 4), 1),               # a pair of blocks with a ragged second; two tiles
    'atoms-33-group-2': (1, 1, 66, (9, 10), (2, 3), 2),
    'strip-boundary': (1, 1, 2, (257, 64), (3, 4), 2),        # 17 tiles: a strip of 16 and one of 1
    '1d-50': (3, 3, 3, (50,), (7,), 1),
    '1d-tile-plus-one': (2, 1, 5, (TILE_PIX + 1,), (7,), 1),
    '1d-strip-boundary': (1, 1, 2, (STRIP_TILES * TILE_PIX + 1,), (5,), 1),
}
# float32 only: 45 x 96 elements of H fit beside 32 parked rows once, not twice (in float64 not beside 16)
F32_ONLY = {'wide-atom-20': (1, 1, 20, (9, 10), (30, 30), 1)}
ALL = dict(MATRIX, **F32_ONLY)
