"""
Host mirror of the launch of tnmf_amd/csrc/correlogram.hip (correlogram_plan, k_correlogram, k_correlogram_finalize), restated
in plain Python in the manner of tests/atom_gram_dispatch.py, so that tests/test_hip_correlogram.py can choose the smallest
problems that execute every branch of the kernel and tests/test_correlogram_cpu.py can check without a GPU that the choice
covers them: block pairs, tile extents, lag chunks, strips.
"""
THREADS = 256          # correlogram.h, kCorrThreads
BLOCK = 16             # kCorrBlock: planes per block
CHUNK = 32             # kCorrChunk: lags per chunk
WAVES = THREADS // 64
TILE1 = {'f32': 256, 'f64': 128}   # kCorrTile1Float, kCorrTile1Double: TX with one shift axis
TILE_X = 64                        # kCorrTileX
TILE_Y = {'f32': 4, 'f64': 2}      # kCorrTileYFloat, kCorrTileYDouble
PAD = 4                # kCorrPad
MAX_LAG = {1: 1023, 2: 63}         # kCorrMaxLag1, kCorrMaxLag2
TARGET_GROUPS = 2048   # kCorrTargetGroups
PARTIAL_CAP = 256 << 20            # kCorrPartialCap
ESIZE = {'f32': 4, 'f64': 8}


def cdiv(a, b):
    return -(-a // b)


def plan(N, P, S, L, per_sample, dt):
    """correlogram_plan for lags within the limits: dict of its fields."""
    ndim = len(S)
    assert len(L) == ndim and all(0 <= x <= MAX_LAG[ndim] for x in L)
    Sy, Sx = (1, S[0]) if ndim == 1 else S
    Ly, Lx = (0, L[0]) if ndim == 1 else L
    p = dict(P=P, Sy=Sy, Sx=Sx, Ly=Ly, Lx=Lx, Lye=min(Ly, Sy - 1), Lxe=min(Lx, Sx - 1))
    p['TY'] = 1 if ndim == 1 else TILE_Y[dt]
    p['TX'] = TILE1[dt] if ndim == 1 else TILE_X
    p['tiles_y'], p['tiles_x'] = cdiv(Sy, p['TY']), cdiv(Sx, p['TX'])
    p['tiles'] = p['tiles_y'] * p['tiles_x']
    p['nb'] = cdiv(P, BLOCK)
    p['pairs'] = p['nb'] ** 2
    p['c0'], p['cr'] = cdiv(p['Lxe'] + 1, CHUNK), cdiv(2 * p['Lxe'] + 1, CHUNK)
    p['chunks'] = p['c0'] + p['Lye'] * p['cr']
    p['nh'] = p['Lxe'] + 1 + p['Lye'] * (2 * p['Lxe'] + 1)
    p['nseg'] = N if per_sample else 1
    p['seglen'] = p['tiles'] if per_sample else N * p['tiles']
    units = p['nseg'] * p['pairs'] * p['chunks']
    want = cdiv(TARGET_GROUPS, units)
    cap = max(1, PARTIAL_CAP // (p['nseg'] * p['pairs'] * p['nh'] * 256 * 8))
    strips = max(1, min(want, cap, p['seglen']))
    p['ipg'] = cdiv(p['seglen'], strips)
    p['strips'] = cdiv(p['seglen'], p['ipg'])
    p['groups'] = units * p['strips']
    p['lds'] = p['TY'] * BLOCK * (2 * p['TX'] + CHUNK + 2 * PAD) * ESIZE[dt]
    p['partial_bytes'] = p['nseg'] * p['strips'] * p['pairs'] * p['nh'] * 256 * 8
    return p


def chunk(p, c):
    """corr_chunk: (dy, first dx, lags) of lag chunk c."""
    if c < p['c0']:
        dy, dx0 = 0, c * CHUNK
    else:
        dy, dx0 = 1 + (c - p['c0']) // p['cr'], -p['Lxe'] + (c - p['c0']) % p['cr'] * CHUNK
    return dy, dx0, min(CHUNK, p['Lxe'] - dx0 + 1)


def lags_computed(p):
    """Every lag (dy, dx) the chunks hold, in the order of the partial sums."""
    return [(dy, dx0 + l) for dy, dx0, nl in (chunk(p, c) for c in range(p['chunks'])) for l in range(nl)]


BRANCHES = (
    'axes-1', 'axes-2',
    'one-tile', 'several-tiles',
    'x-below-tile', 'x-at-tile', 'x-above-tile',               # Sx == TX - 1, Sx % TX == 0, Sx % TX == 1 beyond one tile
    'y-below-tile', 'y-at-tile', 'y-above-tile',               # the same for the rows of a two-axis tile
    'lag-0-only', 'lag-clamped-x', 'lag-clamped-y',            # one lag; a lag asked for at or beyond the extent: zeros
    'lag-extent-minus-1',                                      # the longest lag with a term: one pixel along the axis
    'chunk-full', 'chunk-ragged',                              # 32 lags in a chunk, or fewer
    'waves-idle',                                              # a chunk with fewer than 4 lags: waves with none
    'row0-several-chunks', 'row-several-chunks',               # dy == 0: more than 32 dx >= 0; dy > 0: more than 32 dx
    'rows-dy-positive', 'window-left-of-plane',                # chunks with dy > 0; windows that start at a negative column
    'blocks-1', 'blocks-several', 'last-block-ragged', 'last-block-full',
    'lag-0-skipped-below-diagonal',                            # I > J: lag 0 is the transposed pair's
    'strip-one-item', 'strip-several-items', 'strip-ragged',   # items per workgroup; the last strip shorter
    'strip-straddles-samples',                                 # a strip whose items belong to two samples
    'strips-several', 'strips-1',
    'per-sample', 'summed',
)


def reached(N, P, S, L, per_sample, dt):
    p = plan(N, P, S, L, per_sample, dt)
    ndim = len(S)
    out = {'axes-1' if ndim == 1 else 'axes-2', 'per-sample' if per_sample else 'summed'}
    out.add('one-tile' if p['tiles'] == 1 else 'several-tiles')

    def extent(s, t, name):
        if s == t - 1:
            out.add(name + '-below-tile')
        if s % t == 0:
            out.add(name + '-at-tile')
        if s > t and s % t == 1:
            out.add(name + '-above-tile')
    extent(p['Sx'], p['TX'], 'x')
    if ndim == 2:
        extent(p['Sy'], p['TY'], 'y')
    if p['nh'] == 1:
        out.add('lag-0-only')
    if p['Lx'] > p['Lxe']:
        out.add('lag-clamped-x')
    if p['Ly'] > p['Lye']:
        out.add('lag-clamped-y')
    if (p['Lxe'] == p['Sx'] - 1 and p['Sx'] > 1) or (p['Lye'] == p['Sy'] - 1 and p['Sy'] > 1):
        out.add('lag-extent-minus-1')
    for c in range(p['chunks']):
        dy, dx0, nl = chunk(p, c)
        out.add('chunk-full' if nl == CHUNK else 'chunk-ragged')
        if nl < WAVES:
            out.add('waves-idle')
        if dy > 0:
            out.add('rows-dy-positive')
        if dx0 < 0:
            out.add('window-left-of-plane')
    if p['c0'] > 1:
        out.add('row0-several-chunks')
    if p['Lye'] > 0 and p['cr'] > 1:
        out.add('row-several-chunks')
    out.add('blocks-1' if p['nb'] == 1 else 'blocks-several')
    if p['nb'] > 1:
        out.add('lag-0-skipped-below-diagonal')
    out.add('last-block-ragged' if P % BLOCK else 'last-block-full')
    out.add('strip-one-item' if p['ipg'] == 1 else 'strip-several-items')
    if p['seglen'] % p['ipg']:
        out.add('strip-ragged')
    if not per_sample and any(s * p['ipg'] // p['tiles'] != (min(p['seglen'], (s + 1) * p['ipg']) - 1) // p['tiles']
                              for s in range(p['strips'])):
        out.add('strip-straddles-samples')
    out.add('strips-1' if p['strips'] == 1 else 'strips-several')
    assert out <= set(BRANCHES), out - set(BRANCHES)
    return out


# name -> (N, P, S, L): the smallest shapes that reach every branch, in float32 and in float64, summed and per sample
MATRIX = {}
for _L in (0, 5, 69, 200):
    MATRIX[f'1d-70-lag-{_L}'] = (2, 3, (70,), (_L,))
MATRIX['1d-1500-lag-1023'] = (1, 2, (1500,), (1023,))          # 32 chunks of 32 lags; six (float64: twelve) tiles
for _L in ((0, 0), (3, 0), (0, 4), (11, 11), (18, 36), (31, 31)):
    MATRIX[f'2d-19x37-lag-{_L[0]}-{_L[1]}'] = (3, 5, (19, 37), _L)
for _P in (16, 17, 33, 48):                                     # diagonal and off-diagonal block pairs, a ragged last block
    MATRIX[f'2d-planes-{_P}'] = (1, _P, (9, 21), (2, 3))
MATRIX.update({
    # one below, at and one above each tile extent (256 and 128 pixels along one axis; 4 and 2 rows, 64 columns on two)
    '1d-127': (2, 2, (127,), (3,)), '1d-128': (2, 2, (128,), (3,)), '1d-129': (2, 2, (129,), (3,)),
    '1d-255': (2, 2, (255,), (3,)), '1d-256': (2, 2, (256,), (3,)), '1d-257': (2, 2, (257,), (3,)),
    '2d-1x63': (2, 2, (1, 63), (1, 2)), '2d-3x63': (2, 2, (3, 63), (1, 2)), '2d-4x64': (2, 2, (4, 64), (1, 2)),
    '2d-5x65': (2, 2, (5, 65), (1, 2)),
    # strips of several (sample, tile) items: the accumulators live over tiles and over samples; a shorter last strip
    'strips-several-items': (3, 5, (66, 37), (63, 0)),
})
