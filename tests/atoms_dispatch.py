"""
Host mirror of the launch of tnmf_amd/csrc/atoms.hip (k_atom_taps, k_atom_terms, k_atom_terms_finalize), restated in plain
Python in the manner of tests/direct_dispatch.py, so that tests/test_hip_atom_gains.py can choose the smallest problems that
execute every branch of the kernel and tests/test_atoms_dispatch_cpu.py can check without a GPU that the choice covers them.
"""
THREADS = 256          # atoms.h, kAtomThreads
PIX = 4                # kAtomPix: adjacent pixels per thread along x
TILE_Y, TILE_X = 16, 64   # kAtomTileY, kAtomTileX: the pixel tile on two shift axes
TILE_1D = THREADS * PIX   # kAtomTile1D: on one
CHANNELS = 4           # kAtomChannels: channels per chunk
CHUNK = 64             # kAtomChunk: atoms whose wave sums wait in LDS
STAGE = 10             # atoms.hip, kStage: tile elements per thread in the register stage
LDS_LIMIT = 60 * 1024  # launch_atom_terms


def cdiv(a, b):
    return -(-a // b)


def plan(C, D, A):
    """atom_terms_plan: dict(TY, TX, tiles_y, tiles_x, CH, chunks, NB, NBO, SW, SH, slots)."""
    Dy, Dx = (1, D[0]) if len(D) == 1 else D
    Ay, Ax = (1, A[0]) if len(A) == 1 else A
    TY, TX = (1, TILE_1D) if Dy == 1 and Ay == 1 else (TILE_Y, TILE_X)
    p = dict(TY=TY, TX=TX, tiles_y=cdiv(Dy, TY), tiles_x=cdiv(Dx, TX), CH=min(C, CHANNELS))
    p['chunks'] = cdiv(C, p['CH'])
    p['NB'], p['NBO'] = cdiv(Ax, PIX), cdiv(Ax + 1, PIX)
    p['SW'], p['SH'] = TX + PIX * p['NBO'], TY + Ay - 1
    p['slots'] = p['tiles_y'] * p['tiles_x'] * p['chunks']
    return p


BRANCHES = (
    'tile-1d', 'tile-2d',
    'one-tile', 'several-tiles-y', 'several-tiles-x',   # the finalize adds one slot / several
    'ragged-y', 'ragged-x',                              # pixels of the last tile outside the sample
    'below-halo-y', 'below-halo-x',                      # D < A - 1: the tile's rows / columns of H end inside the halo
    'channels-1', 'channels-3', 'channel-chunks',        # CH, and C > kAtomChannels: a second chunk with channels past the last
    'taps-shifted-run-extra', 'taps-runs-equal',         # NBO == NB + 1 (Ax a multiple of 4) / NBO == NB
    'stage-registers', 'stage-loop',                     # SH * SW <= kStage * 256 or not
    'group-1', 'group-several', 'group-is-M',
    'atoms-flush-at-end', 'atoms-flush-inside',          # M / group <= kAtomChunk or not
)


def reached(N, C, M, D, A, group):
    p = plan(C, D, A)
    Dy, Dx = (1, D[0]) if len(D) == 1 else D
    Ay, Ax = (1, A[0]) if len(A) == 1 else A
    out = {'tile-1d' if p['TY'] == 1 else 'tile-2d'}
    if p['tiles_y'] * p['tiles_x'] == 1:
        out.add('one-tile')
    if p['tiles_y'] > 1:
        out.add('several-tiles-y')
    if p['tiles_x'] > 1:
        out.add('several-tiles-x')
    if Dy % p['TY']:
        out.add('ragged-y')
    if Dx % p['TX']:
        out.add('ragged-x')
    if Ay > 1 and Dy < Ay - 1:
        out.add('below-halo-y')
    if Dx < Ax - 1:
        out.add('below-halo-x')
    out.add('channel-chunks' if p['chunks'] > 1 else f'channels-{C}' if C in (1, 3) else 'channels-other')
    out.discard('channels-other')
    out.add('taps-shifted-run-extra' if p['NBO'] > p['NB'] else 'taps-runs-equal')
    out.add('stage-registers' if p['SH'] * p['SW'] <= STAGE * THREADS else 'stage-loop')
    out.add('group-1' if group == 1 else 'group-is-M' if group == M else 'group-several')
    out.add('atoms-flush-inside' if M // group > CHUNK else 'atoms-flush-at-end')
    assert out <= set(BRANCHES), out - set(BRANCHES)
    return out


# name -> (N, C, M, D, A, group): the smallest shapes that reach every branch
MATRIX = {
    'one-tile': (2, 1, 3, (16, 64), (3, 4), 1),
    'tile-plus-one': (2, 3, 3, (17, 65), (5, 5), 1),         # ragged in both, four tiles
    'tile-plus-one-y': (2, 1, 5, (17, 64), (3, 4), 1),
    'tile-plus-one-x': (3, 3, 5, (16, 65), (5, 5), 5),       # group equals M
    'tile-minus-one': (3, 1, 5, (15, 63), (3, 4), 1),
    'below-halo': (2, 3, 4, (3, 2), (5, 5), 4),
    'atom-12x12': (2, 1, 8, (20, 70), (12, 12), 4),          # group 4 of M = 8
    'tall-atom': (2, 1, 3, (9, 10), (20, 8), 1),             # 35 x 76 elements of H per tile: beyond the register stage
    'channels-5': (2, 5, 3, (9, 10), (3, 4), 1),
    '1d-50': (3, 3, 3, (50,), (7,), 1),
    '1d-tile-plus-one': (2, 1, 5, (TILE_1D + 1,), (7,), 1),
    '1d-many-atoms': (2, 1, 70, (50,), (7,), 1),
}
