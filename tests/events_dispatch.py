"""
Host mirror of the launches and the control flow of the five events kernels -- k_events_render, k_events_update,
k_events_grad_W, k_events_grad_W_sum (tnmf_amd/csrc/events.hip) and, through the lists they are given, HIP_Backend.event_list
and event_plane_list -- restated in plain Python, so that the tests can choose small problems that execute every branch of
them (tests/test_hip_events_matrix.py) and a CPU test can check that the choice covers them all
(tests/test_events_dispatch_cpu.py).  "Every branch" means: every loop that can take a second pass takes one, every clamp
clamps, every guard is met from both sides, every seam of the sub-lane scheme of the W gradient is stood on -- the names
of BRANCHES below.

A geometry is (N, C, P, D, A, mode): samples, channels, planes of the dictionary, sample shape, atom shape (1-D:
one-element D and A), reconstruction mode.  The events are (sample [K], plane [K], shift [K, k]).
"""
import zlib

import numpy as np

import events_reference as eref

NUM_CU = 256            # compute units of one MI355X (what events_grid() reads from ctx->num_cu there)

THREADS = 256           # events.h, kEventThreads
CHAN = 4                # events.hip, kChan
WAVES = THREADS // 64   # events.hip, kWaves
SEGMENT = 64            # include/tnmf_hip.h, TNMF_EVENTS_SEGMENT
CELL_1D, CELL_2D = 256, 16   # include/tnmf_hip.h, TNMF_EVENTS_CELL_1D / _2D

BRANCHES = {
    'render': (
        'one-image', 'two-images', 'four-images',   # event_list: the images an event stands for
        'image-clipped',                  # the jy / jx test: an image whose footprint leaves the sample
        'threads-outside',                # `inside`: a tile with threads outside the sample
        'R5:whole-tiles',                 # `inside`: 2-D, several tiles per axis, none with a thread outside the sample
        'R5:narrower-than-a-tile',        # `inside`: Dx < tx: every tile row has threads outside
        'channels-below-a-group',         # C < kChan: the guard c0 + cc < C in the first pass
        'R1:second-channel-pass',         # the c0 loop: C > kChan
        'R1:partial-last-channel-group',  # the guard c0 + cc < C: C > kChan and C % kChan != 0
        'R2:three-cell-rows',             # the cy loop: cy1 - tile_y >= 2 (Ay >= ty + 2)
        'R2:three-cell-columns',          # i0 .. i1: cx1 - tile_x >= 2 (Ax >= tx + 2): a run over three cells
        'cy1-clamped', 'cx1-clamped',     # cy1 / cx1: the min() with ncy - 1 / ncx - 1 decides
        'empty-run', 'one-chunk',         # the `base` loop over chunks takes no pass / one pass
        'R3:second-chunk',                # the `base` loop: a run of more than kEventThreads images: s_img / s_h are reused
        'R3:partial-chunk-after-a-full',  # `mine < i1`, `count`: ... whose last chunk is partial
        'R4:tile-loop-strides',           # the tile loop: more tiles than workgroups
    ),
    'update': (
        'one-image', 'two-images', 'four-images', 'image-clipped',   # event_walk.h: Occurrence, for_each_tap
        'U1:one-tap',                     # for_each_tap(lane, 64), taps == 1: lane 0 alone gathers
        'U1:idle-lanes',                  # ... taps < 64: lanes without a tap take part in the butterfly
        'lane-loop-strides',              # ... taps > 64
        'U2:event-loop-strides',          # the event loop: more events than waves
        'U3:widest-circular',             # api.hip events_shift_shape: A - 1 == S on an axis, every shift has two images
        'U3:widest-reflect',              # ... A - 1 == S - 1
    ),
    'grad_W': (
        'one-image', 'two-images', 'four-images', 'image-clipped',   # the staging (axis_images), the iy / ix loops
        'L==1', 'L-2..63', 'L>=64',       # L: sub-lanes per tap
        'idle-threads',                   # `active`: threads with sub >= L or t >= taps
        'G1:taps-128', 'G1:taps-256',     # L == 2 / L == 1 and no idle thread
        'tap-loop-strides',               # the t0 loop: taps > kEventThreads
        'G1:three-tap-passes',            # the t0 loop: taps > 2 * kEventThreads
        'G1:L-exceeds-segment',           # the `i = sub` loop, L > TNMF_EVENTS_SEGMENT: sub-lanes that own no event
        'full-segment', 'partial-segment',   # `count` of the segment
        'plane-of-several-segments',      # `first` of the segment
        'slab-beyond-the-last-segment',   # `plane < 0`
        'G2:empty-plane-in-front',        # the plane walk: acc crosses a plane without segments before the first populated one
        'G2:empty-plane-between',         # ... between two populated ones
        'G3:whole-segments-then-a-plane',   # `count`: count % SEGMENT == 0 with a populated plane behind
    ),
    'grad_W_sum': (
        'plane-without-slabs', 'one-slab', 'several-slabs',   # the s0 .. s1 loop
        'G2:offset-crosses-an-empty-plane',   # the pp loop: s0 of a populated plane behind an empty one
        'G3:offset-crosses-whole-segments',   # ... behind a plane of whole segments
        'several-chunks',                 # `chunks`: taps > kEventThreads
        'threads-beyond-the-taps',        # `t >= taps`
    ),
}

# the items of the issue this matrix was built for: R1-R5, U1-U3, G1-G3 -> the names above that stand for them
NEW = {kernel: tuple(b for b in names if b[0] in 'RUG' and b[1].isdigit() and b[2] == ':')
       for kernel, names in BRANCHES.items()}


def cdiv(a, b):
    return -(-a // b)


def events_tile(ndim):
    """events.h events_tile -> (ty, tx)."""
    return (CELL_2D, CELL_2D) if ndim == 2 else (1, CELL_1D)


def dims(geometry):
    """(Dy, Dx, Ay, Ax) as EventGeo holds them (api.hip events_geo): a signal is one row."""
    _, _, _, D, A, _ = geometry
    return (1, D[0], 1, A[0]) if len(A) == 1 else (D[0], D[1], A[0], A[1])


def shift_shape(geometry):
    """(Sy, Sx): api.hip events_shift_shape, with its limits asserted."""
    mode = geometry[5]
    Dy, Dx, Ay, Ax = dims(geometry)
    S = []
    for d, a in ((Dy, Ay), (Dx, Ax)):
        s = d + a - 1 if mode == 'valid' else d - a + 1 if mode == 'full' else d
        assert s >= 1 and not (mode == 'circular' and a - 1 > s) and not (mode == 'reflect' and a - 1 >= s), geometry
        S.append(s)
    return tuple(S)


def grid_for(blocks, num_cu=NUM_CU):
    """events.h events_grid, per_cu = 64."""
    return max(1, min(blocks, num_cu * 64))


def axis_images(mode, u, a, S):
    """event_walk.h axis_images on an array of shifts -> (q0, q1, two): the padded positions, and where the second exists."""
    u = np.asarray(u, dtype=np.int64)
    none = np.zeros(u.shape, dtype=bool)
    if mode == 'valid':
        return u, u, none
    q0 = u + a - 1
    if mode == 'circular':
        return q0, u - (S - (a - 1)), u >= S - (a - 1)
    if mode == 'reflect':
        return q0, (a - 1) - u, (u >= 1) & (u <= a - 1)
    return q0, q0, none


def image_table(geometry, shift):
    """-> (ny [K], nx [K], images [I, 3] = (event, qy, qx)): every image of every event (HIP_Backend.event_list)."""
    mode = geometry[5]
    Dy, Dx, Ay, Ax = dims(geometry)
    Sy, Sx = shift_shape(geometry)
    shift = np.asarray(shift, dtype=np.int64).reshape(-1, len(geometry[4]))
    uy = shift[:, 0] if shift.shape[1] == 2 else np.zeros(len(shift), dtype=np.int64)
    ux = shift[:, -1]
    assert np.all((uy >= 0) & (uy < Sy) & (ux >= 0) & (ux < Sx)), 'shifts outside the shift shape'
    qy0, qy1, two_y = axis_images(mode, uy, Ay, Sy)
    qx0, qx1, two_x = axis_images(mode, ux, Ax, Sx)
    every = np.ones(len(shift), dtype=bool)
    rows = []
    for qy, my in ((qy0, every), (qy1, two_y)):
        for qx, mx in ((qx0, every), (qx1, two_x)):
            e = np.flatnonzero(my & mx)
            rows.append(np.stack([e, qy[e], qx[e]], axis=1))
    return 1 + two_y.astype(int), 1 + two_x.astype(int), np.concatenate(rows)


def _image_branches(geometry, shift):
    Dy, Dx, Ay, Ax = dims(geometry)
    ny, nx, images = image_table(geometry, shift)
    out = set()
    for n, name in ((1, 'one-image'), (2, 'two-images'), (4, 'four-images')):
        if np.any(ny * nx == n):
            out.add(name)
    qy, qx = images[:, 1], images[:, 2]
    if np.any((qy - (Ay - 1) < 0) | (qy > Dy - 1) | (qx - (Ax - 1) < 0) | (qx > Dx - 1)):
        out.add('image-clipped')
    return out, images


def cell_counts(geometry, sample, shift):
    """[N, ncy, ncx]: the images per cell -- the cell keys of HIP_Backend.event_list, cell_start as run lengths."""
    N, _, _, _, A, _ = geometry
    Dy, Dx, Ay, Ax = dims(geometry)
    ty, tx = events_tile(len(A))
    ncy, ncx = cdiv(Dy + Ay - 1, ty), cdiv(Dx + Ax - 1, tx)                 # api.hip events_geo
    _, _, images = image_table(geometry, shift)
    key = (np.asarray(sample, dtype=np.int64)[images[:, 0]] * ncy + images[:, 1] // ty) * ncx + images[:, 2] // tx
    return np.bincount(key, minlength=N * ncy * ncx).reshape(N, ncy, ncx)


def render_branches(geometry, sample, plane, shift, num_cu=NUM_CU):
    """The branches of k_events_render (events.hip) and its launch (events_render) on this list executes."""
    N, C, _, _, A, _ = geometry
    Dy, Dx, Ay, Ax = dims(geometry)
    ty, tx = events_tile(len(A))
    ncy, ncx = cdiv(Dy + Ay - 1, ty), cdiv(Dx + Ax - 1, tx)                 # api.hip events_geo
    out, _ = _image_branches(geometry, shift)
    counts = cell_counts(geometry, sample, shift)
    start = np.concatenate([np.zeros((N, ncy, 1), dtype=np.int64), np.cumsum(counts, axis=2)], axis=2)
    nty, ntx = cdiv(Dy, ty), cdiv(Dx, tx)                                   # events_render
    tiles = N * nty * ntx
    if tiles > grid_for(tiles, num_cu):                                     # the tile loop, grid_for
        out.add('R4:tile-loop-strides')
    if Dy % ty or Dx % tx:                                                  # `inside`
        out.add('threads-outside')
    elif len(A) == 2 and nty > 1 and ntx > 1:
        out.add('R5:whole-tiles')
    if Dx < tx:
        out.add('R5:narrower-than-a-tile')
    if C < CHAN:                                                            # the c0 loop and its guard
        out.add('channels-below-a-group')
    if C > CHAN:
        out.add('R1:second-channel-pass')
        if C % CHAN:
            out.add('R1:partial-last-channel-group')
    for tile_y in range(nty):
        for tile_x in range(ntx):
            cy_free, cx_free = (tile_y * ty + ty + Ay - 2) // ty, (tile_x * tx + tx + Ax - 2) // tx   # cy1, cx1
            cy1, cx1 = min(cy_free, ncy - 1), min(cx_free, ncx - 1)
            if cy_free > ncy - 1:
                out.add('cy1-clamped')
            if cx_free > ncx - 1:
                out.add('cx1-clamped')
            if cy1 - tile_y >= 2:
                out.add('R2:three-cell-rows')
            if cx1 - tile_x >= 2:
                out.add('R2:three-cell-columns')
            for cy in range(tile_y, cy1 + 1):                               # the cy loop: one run per cell row, per sample
                run = start[:, cy, cx1 + 1] - start[:, cy, tile_x]
                if np.any(run == 0):
                    out.add('empty-run')
                if np.any((run > 0) & (run <= THREADS)):
                    out.add('one-chunk')
                if np.any(run > THREADS):
                    out.add('R3:second-chunk')
                if np.any((run > THREADS) & (run % THREADS != 0)):
                    out.add('R3:partial-chunk-after-a-full')
    return out


def update_branches(geometry, sample, plane, shift, num_cu=NUM_CU):
    """The branches of k_events_update (events.hip) and its launch (events_update) on this list executes."""
    _, C, _, _, A, mode = geometry
    _, _, Ay, Ax = dims(geometry)
    Sy, Sx = shift_shape(geometry)
    out, _ = _image_branches(geometry, shift)
    taps = C * Ay * Ax                                                      # k_events_update
    if taps == 1:
        out.add('U1:one-tap')
    if taps < 64:
        out.add('U1:idle-lanes')
    if taps > 64:
        out.add('lane-loop-strides')
    blocks = cdiv(len(sample), WAVES)                                       # events_update
    if blocks > grid_for(blocks, num_cu):                                   # the event loop
        out.add('U2:event-loop-strides')
    for a, s in ((Ay, Sy), (Ax, Sx)):                                       # api.hip events_shift_shape: the limits
        if mode == 'circular' and a > 1 and a - 1 == s:
            out.add('U3:widest-circular')
        if mode == 'reflect' and a > 1 and a - 1 == s - 1:
            out.add('U3:widest-reflect')
    return out


def sub_lanes(taps):
    """k_events_grad_W, L."""
    return max(1, THREADS // taps)


def plane_counts(geometry, plane):
    """Events per plane: plane_start of HIP_Backend.event_plane_list as run lengths (events.hip plane_run)."""
    return np.bincount(np.asarray(plane, dtype=np.int64), minlength=geometry[2])


def events_grad_W_slabs(n_events, P):
    """events.hip events_grad_W_slabs."""
    return n_events // SEGMENT + P


def grad_W_branches(geometry, sample, plane, shift, num_cu=NUM_CU):
    """The branches of k_events_grad_W (events.hip), one workgroup per slab (events_grad_W)."""
    _, C, P, _, _, _ = geometry
    _, _, Ay, Ax = dims(geometry)
    out, _ = _image_branches(geometry, shift)
    taps = C * Ay * Ax
    L = sub_lanes(taps)
    out.add('L==1' if L == 1 else 'L-2..63' if L < 64 else 'L>=64')
    if (L > 1 and L * taps < THREADS) or (L == 1 and taps % THREADS):       # `active`
        out.add('idle-threads')
    if taps == 128:
        out.add('G1:taps-128')
    if taps == 256:
        out.add('G1:taps-256')
    if taps > THREADS:                                                      # the t0 loop
        out.add('tap-loop-strides')
    if taps > 2 * THREADS:
        out.add('G1:three-tap-passes')
    counts = plane_counts(geometry, plane)
    if len(sample) and L > SEGMENT:                                         # the `i = sub` loop
        out.add('G1:L-exceeds-segment')
    segments = [cdiv(int(c), SEGMENT) for c in counts]                      # ns of the plane walk
    if sum(segments) < events_grad_W_slabs(len(sample), P):                 # `plane < 0`
        out.add('slab-beyond-the-last-segment')
    if any(c >= SEGMENT for c in counts):
        out.add('full-segment')
    if any(c % SEGMENT for c in counts):
        out.add('partial-segment')
    if any(s > 1 for s in segments):
        out.add('plane-of-several-segments')
    live = [p for p in range(P) if counts[p] > 0]
    if live and live[0] > 0:
        out.add('G2:empty-plane-in-front')
    if any(b - a > 1 for a, b in zip(live, live[1:])):
        out.add('G2:empty-plane-between')
    if any(counts[p] % SEGMENT == 0 for p in live[:-1]):
        out.add('G3:whole-segments-then-a-plane')
    return out


def grad_W_sum_branches(geometry, sample, plane, shift, num_cu=NUM_CU):
    """The branches of k_events_grad_W_sum (events.hip), one thread per (plane, tap) (events_grad_W)."""
    _, C, P, _, _, _ = geometry
    _, _, Ay, Ax = dims(geometry)
    taps = C * Ay * Ax
    counts = plane_counts(geometry, plane)
    out = set()
    for p in range(P):
        ns = cdiv(int(counts[p]), SEGMENT)
        out.add('plane-without-slabs' if ns == 0 else 'one-slab' if ns == 1 else 'several-slabs')
        if ns and any(counts[q] == 0 for q in range(p)):
            out.add('G2:offset-crosses-an-empty-plane')
        if ns and any(counts[q] > 0 and counts[q] % SEGMENT == 0 for q in range(p)):
            out.add('G3:offset-crosses-whole-segments')
    if taps > THREADS:                                                      # `chunks`
        out.add('several-chunks')
    if taps % THREADS:                                                      # `t >= taps`
        out.add('threads-beyond-the-taps')
    return out


MIRRORS = {'render': render_branches, 'update': update_branches, 'grad_W': grad_W_branches,
           'grad_W_sum': grad_W_sum_branches}


def reached(geometry, sample, plane, shift, num_cu=NUM_CU):
    """{kernel: the set of names of BRANCHES[kernel] this problem executes}."""
    out = {kernel: mirror(geometry, sample, plane, shift, num_cu) for kernel, mirror in MIRRORS.items()}
    for kernel, names in out.items():
        assert names <= set(BRANCHES[kernel]), (kernel, names - set(BRANCHES[kernel]))
    return out


# -- the matrix of tests/test_hip_events_matrix.py ----------------------------------------------------------------------------
# name -> (geometry with N possibly a function of the CU count, {kernel: the items of the issue the case is there for}).
# The two stride cases are sized from the CU count of the device the test runs on; the counts quoted are for 256 CUs.
MATRIX = {
    # R1: six channels are a full group of four and a partial one of two
    'channels': (lambda cu: (2, 6, 3, (20, 23), (4, 6), 'valid'),
                 {'render': ('R1:second-channel-pass', 'R1:partial-last-channel-group')}),
    # R1, R2: an 18 x 20 atom reaches three cell rows and three cell columns; G1: 2160 taps are nine passes of the tap loop
    'tall-atom': (lambda cu: (2, 6, 3, (40, 50), (18, 20), 'valid'),
                  {'render': ('R1:second-channel-pass', 'R2:three-cell-rows', 'R2:three-cell-columns'),
                   'grad_W': ('G1:three-tap-passes',)}),
    # R2 in 1-D: 300 taps reach three cells of 256 positions; G1: 300 taps are two passes, the second partial
    'long-atom-1d': (lambda cu: (2, 1, 2, (600,), (300,), 'valid'),
                     {'render': ('R2:three-cell-columns',)}),
    # R3: 600 events in one cell row of a 24 x 24 sample: the tile's run is three chunks, 256 + 256 + 88
    'pile-up': (lambda cu: (1, 1, 4, (24, 24), (3, 3), 'valid'),
                {'render': ('R3:second-chunk', 'R3:partial-chunk-after-a-full')}),
    # R4: one tile per sample and 37 more samples than workgroups; R5: samples narrower than a tile
    'many-tiles': (lambda cu: (cu * 64 + 37, 1, 2, (3, 5), (2, 2), 'valid'),
                   {'render': ('R4:tile-loop-strides', 'R5:narrower-than-a-tile')}),
    # R5: 2 x 3 tiles, no thread outside the sample
    'whole-tiles': (lambda cu: (2, 2, 3, (32, 48), (5, 7), 'full'),
                    {'render': ('R5:whole-tiles',)}),
    # U1: one tap, 63 idle lanes in the butterfly; G1: L == 256 sub-lanes on segments of 64 events
    'one-tap': (lambda cu: (3, 1, 4, (100, 100), (1, 1), 'valid'),
                {'update': ('U1:one-tap', 'U1:idle-lanes'), 'grad_W': ('G1:L-exceeds-segment',)}),
    # U2: 300 more events than the waves of the grid (cu * 64 workgroups of four)
    'many-events': (lambda cu: (2, 1, 4, (100, 100), (1, 2), 'valid'),
                    {'update': ('U2:event-loop-strides',)}),
    # U3: Ay - 1 == Sy: every shift has two images in y
    'widest-circular': (lambda cu: (2, 2, 3, (5, 7), (6, 4), 'circular'),
                        {'update': ('U3:widest-circular',)}),
    # U3: Ay - 1 == Sy - 1: every shift but 0 has its mirror image in y
    'widest-reflect': (lambda cu: (2, 2, 3, (6, 7), (6, 4), 'reflect'),
                       {'update': ('U3:widest-reflect',)}),
    # G1: the seams of the sub-lane scheme without an idle thread
    'taps-128': (lambda cu: (2, 2, 3, (20, 20), (8, 8), 'valid'), {'grad_W': ('G1:taps-128',)}),
    'taps-256': (lambda cu: (2, 4, 3, (20, 20), (8, 8), 'valid'), {'grad_W': ('G1:taps-256',)}),
    # G2, G3: counts per plane [0, 64, 0, 128, 5, 0]
    'empty-planes': (lambda cu: (2, 2, 6, (20, 23), (4, 6), 'valid'),
                     {'grad_W': ('G2:empty-plane-in-front', 'G2:empty-plane-between', 'G3:whole-segments-then-a-plane'),
                      'grad_W_sum': ('G2:offset-crosses-an-empty-plane', 'G3:offset-crosses-whole-segments')}),
}

EMPTY_PLANES_COUNTS = (0, SEGMENT, 0, 2 * SEGMENT, 5, 0)


def geometry_of(name, num_cu=NUM_CU):
    return MATRIX[name][0](num_cu)


def _draw(rng, dims_, count):
    """`count` distinct rows of the index space `dims_`, as an int64 array [count, len(dims_)]."""
    flat = rng.choice(int(np.prod(dims_)), count, replace=False)
    return np.stack(np.unravel_index(flat, dims_), axis=1).astype(np.int64)


_CASES = {}


def matrix_case(name, num_cu=NUM_CU):
    """-> (geometry, sample, plane, shift, integer strengths 1..4, integer W in 0..3), read-only float64 / int64: distinct
    rows in shuffled order, as tests/test_hip_events.py::case gives them."""
    if (name, num_cu) in _CASES:
        return _CASES[name, num_cu]
    N, C, P, D, A, mode = geo = geometry_of(name, num_cu)
    S = eref.shift_shape(D, A, mode)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    space = (N, P) + tuple(S)
    if name == 'pile-up':
        # shifts (= padded positions, 'valid') inside the cell row 0 .. 15: one run of the tile at the origin.  All of them in
        # the rows 0 .. 5, so their footprints end at pixel row 5: the two waves that own the pixel rows 8 .. 15 find nothing
        # to add, are done with a chunk long before the other two and, without the barrier in front of the staging, would
        # overwrite it under them
        rows = _draw(rng, (1, P, 6, S[1]), 600)
    elif name == 'many-tiles':
        # the last samples included: the tiles of the second round of the tile loop
        rows = {(N - 1 - i, i % P, i % S[0], (2 * i) % S[1]) for i in range(40)}
        rows |= {tuple(r) for r in _draw(rng, space, 500).tolist()}
        rows = np.array(sorted(rows), dtype=np.int64)
    elif name == 'many-events':
        rows = _draw(rng, space, num_cu * 64 * WAVES + 300)
    elif name == 'empty-planes':
        rows = np.concatenate([np.insert(_draw(rng, (N,) + tuple(S), c), 1, pl, axis=1)
                               for pl, c in enumerate(EMPTY_PLANES_COUNTS) if c])
    else:
        count = {'tall-atom': 320, 'long-atom-1d': 60, 'one-tap': 300, 'taps-128': 150, 'taps-256': 150}.get(name, 40)
        rows = {tuple(r) for r in _draw(rng, space, count).tolist()}
        # the corners of the shift range; for the widest atoms: the wrap / mirror zone of both axes and its edges
        rows |= {(0, 1) + tuple(c * (s - 1) for c, s in zip(corner, S)) for corner in np.ndindex(*(2,) * len(S))}
        if name.startswith('widest'):
            rows |= {(1, 0) + tuple(min(a, s) - 1 for a, s in zip(A, S)), (1, 2, 0, 0), (0, 2, 1, 1), (1, 1, S[0] - 1, 3)}
        rows = np.array(sorted(rows), dtype=np.int64)
    assert len(np.unique(rows, axis=0)) == len(rows)
    rows = rows[rng.permutation(len(rows))]
    out = (geo, rows[:, 0], rows[:, 1], rows[:, 2:], rng.integers(1, 5, len(rows)).astype(np.float64),
           rng.integers(0, 4, (P, C) + A).astype(np.float64))
    for a in out[1:]:
        a.setflags(write=False)
    _CASES[name, num_cu] = out
    return out
