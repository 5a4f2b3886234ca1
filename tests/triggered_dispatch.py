"""
Host mirror of the launch of tnmf_amd/csrc/triggered.hip (triggered_plan, k_triggered, k_triggered_finalize), restated in
plain Python in the manner of tests/correlogram_dispatch.py, so that tests/test_hip_triggered.py can choose the smallest
problems that execute every branch of the kernel and tests/test_triggered_cpu.py can check without a GPU that the choice
covers them: cells, chunks, strips, tiles, work bytes.
"""
THREADS = 256          # triggered.h, kTrigThreads
BLOCK = 16             # kTrigBlock: planes per block, window columns per cell
CHUNK = 32             # kTrigChunk: cells per chunk
WAVES = THREADS // 64
TILE1 = {'f32': 256, 'f64': 128}   # kTrigTile1Float, kTrigTile1Double: TX with one shift axis
TILE_X = 64                        # kTrigTileX
TILE_Y = {'f32': 4, 'f64': 2}      # kTrigTileYFloat, kTrigTileYDouble
PAD = 4                # kTrigPad
MAX_WINDOW = {1: 4096, 2: 128}     # kTrigMaxWindow1, kTrigMaxWindow2
TARGET_GROUPS = 2048   # kTrigTargetGroups
PARTIAL_CAP = 256 << 20            # kTrigPartialCap
ESIZE = {'f32': 4, 'f64': 8}


def cdiv(a, b):
    return -(-a // b)


def plan(N, P, F, D, A, m, per_sample, dt):
    """triggered_plan for windows within the limits: dict of its fields."""
    ndim = len(D)
    assert len(A) == len(m) == ndim and all(a + 2 * x <= MAX_WINDOW[ndim] for a, x in zip(A, m))
    Dy, Dx = (1, D[0]) if ndim == 1 else D
    Ay, Ax = (1, A[0]) if ndim == 1 else A
    my, mx = (0, m[0]) if ndim == 1 else m
    p = dict(P=P, F=F, Dy=Dy, Dx=Dx, Sy=Dy + Ay - 1, Sx=Dx + Ax - 1, Wy=Ay + 2 * my, Wx=Ax + 2 * mx,
             offy=-(Ay - 1) - my, offx=-(Ax - 1) - mx)
    p['TY'] = 1 if ndim == 1 else TILE_Y[dt]
    p['TX'] = TILE1[dt] if ndim == 1 else TILE_X
    p['tiles_y'], p['tiles_x'] = cdiv(p['Sy'], p['TY']), cdiv(p['Sx'], p['TX'])
    p['tiles'] = p['tiles_y'] * p['tiles_x']
    p['nbp'] = cdiv(P, BLOCK)
    p['nxb'] = cdiv(p['Wx'], BLOCK)
    p['cells'] = F * p['Wy'] * p['nxb']
    p['CB'] = min(p['nxb'], CHUNK)
    p['CJ'] = min(p['Wy'], CHUNK // p['CB'])
    p['CJ'] = cdiv(p['Wy'], cdiv(p['Wy'], p['CJ']))   # as many chunks along jy, of even size
    p['CF'] = min(F, CHUNK // (p['CB'] * p['CJ']))
    p['YC'] = p['TX'] + BLOCK * p['CB']
    p['chunks_x'], p['chunks_y'] = cdiv(p['nxb'], p['CB']), cdiv(p['Wy'], p['CJ'])
    p['chunks_f'] = cdiv(F, p['CF'])
    p['chunks'] = p['chunks_f'] * p['chunks_y'] * p['chunks_x']
    p['split'] = int(p['CF'] * p['CJ'] * p['CB'] < WAVES)
    p['nseg'] = N if per_sample else 1
    p['seglen'] = p['tiles'] if per_sample else N * p['tiles']
    units = max(1, p['nseg'] * p['nbp'] * p['chunks'])
    want = cdiv(TARGET_GROUPS, units)
    cap = max(1, PARTIAL_CAP // max(1, p['nseg'] * p['nbp'] * p['cells'] * 256 * 8))
    strips = max(1, min(want, cap, p['seglen']))
    p['ipg'] = max(1, cdiv(p['seglen'], strips))
    p['strips'] = max(1, cdiv(p['seglen'], p['ipg']))
    p['groups'] = p['nseg'] * p['nbp'] * p['chunks'] * p['strips']
    p['lds'] = (p['TY'] * BLOCK * (p['TX'] + PAD) + p['CF'] * (p['TY'] + p['CJ'] - 1) * p['YC']) * ESIZE[dt]
    p['patch'] = p['CF'] * (p['TY'] + p['CJ'] - 1) * p['YC']
    p['work_bytes'] = 0 if N == 0 else cdiv(p['nseg'] * p['strips'] * p['nbp'] * p['cells'] * 256 * 8, 256) * 256
    return p


def patch_max(TY, TX):
    """trig_patch_max: the most elements of a staged patch of Y over the chunk shapes the plan chooses."""
    return max(CHUNK // (cb * cj) * (TY + cj - 1) * (TX + BLOCK * cb)
               for cb in range(1, CHUNK + 1) for cj in range(1, CHUNK // cb + 1))


def chunk_cells(p, c):
    """The cells (f, jy, jxb) of chunk c, in the order of the workgroup's local cells."""
    cx, cy, cf = c % p['chunks_x'], c // p['chunks_x'] % p['chunks_y'], c // (p['chunks_x'] * p['chunks_y'])
    f0, jy0, jxb0 = cf * p['CF'], cy * p['CJ'], cx * p['CB']
    nf, nj, nb = min(p['CF'], p['F'] - f0), min(p['CJ'], p['Wy'] - jy0), min(p['CB'], p['nxb'] - jxb0)
    return [(f0 + l // (nj * nb), jy0 + l % (nj * nb) // nb, jxb0 + l % nb) for l in range(nf * nj * nb)]


def cells_computed(p):
    return [cell for c in range(p['chunks']) for cell in chunk_cells(p, c)]


BRANCHES = (
    'axes-1', 'axes-2',
    'one-tile', 'several-tiles',
    'x-below-tile', 'x-at-tile', 'x-above-tile',               # Sx == TX - 1, Sx % TX == 0, Sx % TX == 1 beyond one tile
    'y-below-tile', 'y-at-tile', 'y-above-tile',               # the same for the rows of a two-axis tile
    'split', 'cells-over-waves',                               # fewer than 4 cells in a chunk: the waves split the pixels
    'waves-idle',                                              # a (last) chunk of an unsplit plan with fewer than 4 cells
    'cell-full', 'cell-ragged',                                # Wx a multiple of 16, or not
    'chunk-full', 'chunk-ragged',                              # CJ * CB cells in a chunk, or fewer
    'chunks-1', 'chunks-several-y', 'chunks-several-x', 'fields-several',
    'chunk-several-fields', 'chunks-several-f', 'chunk-fields-ragged',   # CF > 1; more fields than a chunk holds; F % CF
    'window-wider-than-sample', 'window-left-of-sample', 'window-right-of-sample',
    'blocks-1', 'blocks-several', 'last-block-ragged', 'last-block-full',
    'strip-one-item', 'strip-several-items', 'strip-ragged',   # items per workgroup; the last strip shorter
    'strip-straddles-samples',                                 # a strip whose items belong to two samples
    'strips-several', 'strips-1',
    'per-sample', 'summed', 'no-sample',
)


def reached(N, P, F, D, A, m, per_sample, dt):
    p = plan(N, P, F, D, A, m, per_sample, dt)
    ndim = len(D)
    out = {'axes-1' if ndim == 1 else 'axes-2', 'per-sample' if per_sample else 'summed'}
    if N == 0:
        return out | {'no-sample'}
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
    out.add('split' if p['split'] else 'cells-over-waves')
    out.add('cell-ragged' if p['Wx'] % BLOCK else 'cell-full')
    for c in range(p['chunks']):
        n = len(chunk_cells(p, c))
        out.add('chunk-full' if n == p['CF'] * p['CJ'] * p['CB'] else 'chunk-ragged')
        if n < WAVES and not p['split']:
            out.add('waves-idle')
    if p['chunks'] == 1:
        out.add('chunks-1')
    if p['chunks_y'] > 1:
        out.add('chunks-several-y')
    if p['chunks_x'] > 1:
        out.add('chunks-several-x')
    if F > 1:
        out.add('fields-several')
    if p['CF'] > 1:
        out.add('chunk-several-fields')
    if p['chunks_f'] > 1:
        out.add('chunks-several-f')
    if F % p['CF']:
        out.add('chunk-fields-ragged')
    if p['Wx'] > p['Dx'] or p['Wy'] > p['Dy']:
        out.add('window-wider-than-sample')
    if p['offx'] < 0 or p['offy'] < 0:
        out.add('window-left-of-sample')
    if p['Wx'] - 1 + p['offx'] > 0:
        out.add('window-right-of-sample')
    out.add('blocks-1' if p['nbp'] == 1 else 'blocks-several')
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


# name -> (N, P, F, D, A, m): the issue's cases, then the smallest shapes that reach every other branch
MATRIX = {
    '1d-window-is-atom': (2, 3, 1, (37,), (5,), (0,)),
    '1d-window-34': (3, 17, 2, (300,), (8,), (13,)),
    '1d-window-wider-than-sample': (1, 1, 1, (6,), (3,), (9,)),
    '2d-window-is-atom': (2, 5, 1, (9, 11), (3, 4), (0, 0)),
    '2d-window-13x20': (3, 18, 3, (20, 70), (5, 6), (4, 7)),
    '2d-mostly-outside': (1, 2, 1, (4, 5), (2, 2), (6, 6)),
    '2d-no-sample': (0, 3, 1, (9, 11), (3, 4), (1, 1)),
    # one below, at and one above each tile extent of the padded planes (256 and 128 pixels along one axis; 4 and 2 rows,
    # 64 columns on two)
    '1d-127': (2, 2, 1, (125,), (3,), (2,)), '1d-128': (2, 2, 1, (126,), (3,), (2,)), '1d-129': (2, 2, 1, (127,), (3,), (2,)),
    '1d-255': (2, 2, 1, (253,), (3,), (2,)), '1d-256': (2, 2, 1, (254,), (3,), (2,)), '1d-257': (2, 2, 1, (255,), (3,), (2,)),
    '2d-1x63': (2, 2, 1, (1, 62), (1, 2), (1, 1)), '2d-3x63': (2, 2, 1, (2, 62), (2, 2), (1, 1)),
    '2d-4x64': (2, 2, 1, (3, 63), (2, 2), (1, 1)), '2d-5x65': (2, 2, 1, (4, 64), (2, 2), (1, 1)),
    # planes: one full block, two full blocks
    '2d-planes-16': (1, 16, 1, (9, 21), (2, 3), (1, 1)), '2d-planes-32': (1, 32, 1, (9, 21), (2, 3), (1, 1)),
    # more than one chunk along jy (window 40 x 16: CJ = 32), along jx (one axis, window 16 * 33 + 2), a full cell
    '2d-chunks-y': (1, 2, 1, (10, 20), (4, 4), (18, 6)),
    '1d-chunks-x': (1, 2, 1, (700,), (6,), (262,)),
    # a last chunk of an unsplit plan with fewer than 4 cells: 11 fields of 3 cells (10 fields a chunk, then 1)
    '2d-last-chunk-small': (1, 2, 11, (8, 20), (3, 4), (0, 0)),
    # strips of several (sample, tile) items: the accumulators live over tiles and over samples; a shorter last strip
    'strips-several-items': (5, 100, 1, (33, 400), (2, 3), (1, 2)),
    # more fields than a chunk holds, the last chunk with fewer: window 128 = 8 cells, 4 fields a chunk, 5 fields
    '1d-fields-ragged': (1, 2, 5, (200,), (8,), (60,)),
}
