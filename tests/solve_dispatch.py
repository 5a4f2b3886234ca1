"""
Host mirror of the launches and the control flow of the nine kernels of tnmf_amd/csrc/solve.hip -- k_events_pairs,
k_events_gram, k_events_project, k_nnls_rows, _scale, _start, _step, _reduce -- and of the host loop events_nnls, restated in
plain Python in the manner of tests/events_dispatch.py, so that tests/test_hip_solve_matrix.py can choose small problems that
execute every branch of them and tests/test_solve_dispatch_cpu.py can check without a GPU that the choice covers them all.

Two matrices.  MATRIX: lists of events, (N, C, P, D, A, mode) with their rows, for the pairs, the Gram matrix and the
projection -- integer W and V in 0..3, so every G_ij and c_i is an integer and exact in double in any order.  SYSTEMS:
synthetic CSR systems for the solver, which sees K-vectors and a matrix only: integer, symmetric, non-negative entries,
every row strictly diagonally dominant (Gershgorin: lambda_min >= 1), L = max_i sum_j |G_ij| a power of two attained by the
hub rows alone, so that 1 / L and (G y - c) / L are exact.

A note on P4.  The header calls the pairs a superset because "the overlap of a candidate may lie wholly outside the sample".
For rows inside the contract that cannot happen: on every axis each image meets the sample, two images closer than the atom
extent meet each other, and three intervals that meet pairwise have a point in common.  A candidate with the value exactly 0
exists all the same -- where every product under the overlap has a zero tap of W -- and that is what 'zero-tap' plants.
"""
import zlib

import numpy as np

import events_dispatch as ed
import events_reference as eref
import solve_reference as sr
from events_dispatch import cdiv, cell_counts, dims, grid_for, image_table

NUM_CU = ed.NUM_CU
THREADS = ed.THREADS                # events.h, kEventThreads
WAVES = THREADS // 64               # solve.hip, kWaves
ROW_LANES = 16                      # solve.hip, kRowLanes
ROWS_PER_BLOCK = THREADS // ROW_LANES   # solve.hip, kRowsPerBlock

BRANCHES = {
    'pairs': (
        'one-image', 'two-images', 'four-images',   # the lists: the images an event stands for
        'P1:image-loop-strides',            # the `a` loop: more images than waves in the grid
        'P1:second-round-finds-pairs',      # ... and an image of the second round has a hit
        'P2:empty-run', 'P2:run-within-a-pass',     # the `base` loop takes no pass / one pass
        'P2:run-above-64-partial-last-pass',        # ... a second pass, `b < i1` false in some lanes of the last
        'P3:cy0-clamped', 'P3:cx0-clamped', 'P3:cy1-clamped', 'P3:cx1-clamped',   # the max() / min() decides
        'P3:three-cell-rows', 'P3:three-cell-columns',   # cy1 - cy0 >= 2, cx1 - cx0 >= 2
        'P4:pair-through-several-image-pairs',      # count exceeds the number of unique keys
        'P4:zero-valued-candidate',         # a candidate whose value is exactly 0: in the pairs, not in the CSR
        'no-hit-in-a-pass', 'hit-in-a-pass',        # `if (!m) continue`
        'P5:capacity-inside-a-ballot-group',        # `slot < capacity` true and false among the hits of one ballot
        'P6:image-event-out-of-range', 'P6:image-position-negative', 'P6:image-cell-beyond',   # the guards on `me`
        'P6:image-sample-out-of-range',
        'P6:other-event-out-of-range',      # `(unsigned)im.w < (unsigned)K` in `hit`
    ),
    'gram': (
        'M1:one-tap', 'M1:taps-below-64', 'M1:taps-64', 'M1:taps-above-64-partial',   # for_each_tap(lane, 64)
        'M2:one-image', 'M2:two-images', 'M2:four-images',   # Occurrence of either row: the loops of for_each_tap and phi_at
        'M2:widest-circular', 'M2:widest-reflect',  # A - 1 == S / A - 1 == S - 1: the images of one event overlap each other
        'M2:own-images-overlap',            # ... G_ii carries the cross terms of two images of row i
        'M3:pair-loop-strides',             # the `p` loop: more pairs than waves in the grid
        'M4:row-without-inside-tap',        # G_ii == 0
        'diagonal', 'off-diagonal',
    ),
    'project': (
        'C1:one-tap', 'C1:taps-below-64', 'C1:taps-64', 'C1:taps-above-64-partial',
        'C2:one-image', 'C2:two-images', 'C2:four-images', 'C2:widest-circular', 'C2:widest-reflect',
        'C3:event-loop-strides',            # the `e` loop: more events than waves in the grid
        'C4:row-without-inside-tap',        # c_i == 0 whatever the sample holds
    ),
    'nnls_rows': (                          # k_nnls_rows and k_nnls_step walk a row the same way
        'S1:row-empty', 'S1:row-1..15', 'S1:row-16', 'S1:row-17..32', 'S1:row-above-32',   # passes of the kRowLanes loop
        'S2:one-block', 'S2:several-blocks', 'S2:partial-last-block',                      # i < K
        'S5:row-without-diagonal', 'S5:diagonal-not-positive',                             # act_i = 0
        'S6:col-skipped', 'S6:row-start-negative', 'S6:row-start-above-nnz', 'S6:row-start-decreases',   # csr_run, the col guard
    ),
    'nnls_scale': (
        'S2:one-pass', 'S2:second-pass', 'S2:partial-last-pass',     # the i loop of the one workgroup
        'S3:L-beyond-the-first-pass', 'S3:cmax-beyond-the-first-pass',   # ... what only a later pass sees
        'S3:cmax-in-the-last-partial-block',
    ),
    'nnls_start': (
        'S2:one-block', 'S2:second-block', 'S2:partial-last-block',
        'S5:start-nan', 'S5:start-negative', 'S5:start-zero', 'S5:start-positive',
        'S5:inactive-row-with-positive-start',
    ),
    'nnls_step': (
        'S1:row-empty', 'S1:row-1..15', 'S1:row-16', 'S1:row-17..32', 'S1:row-above-32',
        'S2:partial-last-block',
        'S3:hub-in-the-last-partial-block',  # a row that attains L (and has more than 32 entries) where i < K cuts the block
        'S4:beta-zero', 'S4:beta-positive',
        'projection-decides', 'projection-idle',    # fmax(..., 0)
        'S5:inactive-row',
    ),
    'nnls_reduce': (
        'S2:one-pass', 'S2:second-pass',    # the i loop: more than kEventThreads block entries (K > 4096)
        'S3:pg-max-beyond-the-first-pass',  # the start's largest |pg| in a block only the second pass reads
        'S3:restart-term-beyond-the-first-pass',
        'S4:restart', 'S4:no-restart',      # s_a[0] > 0, both ways
    ),
    'nnls_host': (
        'max-iterations-0', 'converges', 'stops-at-max-iterations',
        'S7:check-every-1', 'S7:check-every-7', 'S7:check-every-above-max-iterations',
        'S7:max-iterations-not-a-multiple', 'S7:history-capacity-short', 'S7:history-null',
    ),
}

NEW = {kernel: tuple(b for b in names if b[0] in 'PMCS' and b[1].isdigit() and b[2] == ':')
       for kernel, names in BRANCHES.items()}


# -- the lists -------------------------------------------------------------------------------------------------------------------
def cells_of(geometry):
    """(ty, tx, ncy, ncx): api.hip events_geo."""
    Dy, Dx, Ay, Ax = dims(geometry)
    ty, tx = ed.events_tile(len(geometry[4]))
    return ty, tx, cdiv(Dy + Ay - 1, ty), cdiv(Dx + Ax - 1, tx)


def lists_of(geometry, sample, plane, shift):
    """(images [I, 4] = (plane, qy, qx, event) sorted by (sample, cell), cell_start [cells + 1], events [K, 4]): the lists of
    HIP_Backend.event_list -- a stable sort of the images in the order image combination, then event."""
    N = geometry[0]
    ty, tx, ncy, ncx = cells_of(geometry)
    sample, plane = np.asarray(sample, dtype=np.int64), np.asarray(plane, dtype=np.int64)
    shift = np.asarray(shift, dtype=np.int64).reshape(len(sample), -1)
    _, _, images = image_table(geometry, shift)
    e, qy, qx = images[:, 0], images[:, 1], images[:, 2]
    key = (sample[e] * ncy + qy // ty) * ncx + qx // tx
    order = np.argsort(key, kind='stable')
    img = np.stack([plane[e], qy, qx, e], axis=1)[order]
    cell_start = np.searchsorted(key[order], np.arange(N * ncy * ncx + 1))
    assert np.array_equal(np.diff(cell_start), cell_counts(geometry, sample, shift).reshape(-1))
    zero = np.zeros_like(sample)
    events = np.stack([sample, plane, shift[:, 0] if shift.shape[1] == 2 else zero, shift[:, -1]], axis=1)
    return img, cell_start, events


def pairs_walk(geometry, img, cell_start, events, K, which=None):
    """k_events_pairs, wave by wave, on raw lists -> (the keys i * K + j it appends, duplicates included, in the mirror's
    order; the hits of every ballot with a hit; the names of BRANCHES['pairs'] the walk executes).  ``which``: the images
    walked (all of them by default)."""
    N = geometry[0]
    _, _, Ay, Ax = dims(geometry)
    ty, tx, ncy, ncx = cells_of(geometry)
    img, cell_start, events = np.asarray(img), np.asarray(cell_start), np.asarray(events)
    n_images = len(img)
    keys, groups, names = [], [], set()
    for a in (range(n_images) if which is None else which):
        _, qy, qx, e = (int(v) for v in img[a])
        if not 0 <= e < K:
            names.add('P6:image-event-out-of-range')
            continue
        if qy < 0 or qx < 0:
            names.add('P6:image-position-negative')
            continue
        if qy // ty >= ncy or qx // tx >= ncx:
            names.add('P6:image-cell-beyond')
            continue
        n = int(events[e, 0])
        if not 0 <= n < N:
            names.add('P6:image-sample-out-of-range')
            continue
        free = (qy - (Ay - 1), qx - (Ax - 1), (qy + Ay - 1) // ty, (qx + Ax - 1) // tx)
        cy0, cx0 = max(free[0] // ty, 0), max(free[1] // tx, 0)     # (a negative quotient ends at 0 whichever way it rounds)
        cy1, cx1 = min(free[2], ncy - 1), min(free[3], ncx - 1)
        for flag, name in ((free[0] < 0, 'P3:cy0-clamped'), (free[1] < 0, 'P3:cx0-clamped'), (free[2] > ncy - 1, 'P3:cy1-clamped'),
                           (free[3] > ncx - 1, 'P3:cx1-clamped'), (cy1 - cy0 >= 2, 'P3:three-cell-rows'),
                           (cx1 - cx0 >= 2, 'P3:three-cell-columns')):
            if flag:
                names.add(name)
        for ry in range(cy0, cy1 + 1):
            row = (n * ncy + ry) * ncx
            i0, i1 = max(int(cell_start[row + cx0]), 0), min(int(cell_start[row + cx1 + 1]), n_images)
            run = i1 - i0
            if run <= 64 or run % 64:
                names.add('P2:empty-run' if run <= 0 else 'P2:run-within-a-pass' if run <= 64 else
                          'P2:run-above-64-partial-last-pass')
            for base in range(i0, i1, 64):
                chunk = img[base:min(base + 64, i1)]
                other = chunk[:, 3]
                if np.any((other < 0) | (other >= K)):
                    names.add('P6:other-event-out-of-range')
                hit = (other >= 0) & (other < K) & (other > e) & (np.abs(chunk[:, 1] - qy) < Ay) & (np.abs(chunk[:, 2] - qx) < Ax)
                if not hit.any():
                    names.add('no-hit-in-a-pass')
                    continue
                names.add('hit-in-a-pass')
                groups.append(int(hit.sum()))
                keys.extend((e * K + other[hit]).tolist())
    return np.array(keys, dtype=np.int64), groups, names


def taps_of(geometry):
    _, _, Ay, Ax = dims(geometry)
    return geometry[1] * Ay * Ax


def _tap_names(prefix, taps):
    return {f'{prefix}1:one-tap' if taps == 1 else f'{prefix}1:taps-below-64' if taps < 64 else f'{prefix}1:taps-64' if taps == 64
            else f'{prefix}1:taps-above-64-partial' if taps % 64 else f'{prefix}1:taps-64'}


def _occurrence_names(prefix, geometry, shift):
    mode = geometry[5]
    _, _, Ay, Ax = dims(geometry)
    Sy, Sx = ed.shift_shape(geometry)
    ny, nx, _ = image_table(geometry, shift)
    out = {f'{prefix}2:{name}' for n, name in ((1, 'one-image'), (2, 'two-images'), (4, 'four-images')) if np.any(ny * nx == n)}
    for a, s in ((Ay, Sy), (Ax, Sx)):                       # api.hip events_shift_shape: the limits
        if mode == 'circular' and a > 1 and a - 1 == s:
            out.add(f'{prefix}2:widest-circular')
        if mode == 'reflect' and a > 1 and a - 1 == s - 1:
            out.add(f'{prefix}2:widest-reflect')
    return out


def blank_rows(geometry, plane, shift, W):
    """[K] bool: the rows whose occurrence has no non-zero tap inside the sample."""
    D = geometry[3]
    shift = np.asarray(shift).reshape(len(plane), -1)
    return np.array([not any(w != 0 for _, w in eref.pixels(W, D, geometry[5], 0, pl, u)) for pl, u in zip(plane, shift)],
                    dtype=bool)


def own_images_overlap(geometry, shift):
    """Some event has two images whose footprints share a pixel of the sample."""
    Dy, Dx, Ay, Ax = dims(geometry)
    _, _, images = image_table(geometry, shift)
    boxes = {}
    for e, qy, qx in images.tolist():
        boxes.setdefault(e, []).append((max(qy - Ay + 1, 0), min(qy, Dy - 1), max(qx - Ax + 1, 0), min(qx, Dx - 1)))
    for b in boxes.values():
        for i in range(len(b)):
            for j in range(i + 1, len(b)):
                if max(b[i][0], b[j][0]) <= min(b[i][1], b[j][1]) and max(b[i][2], b[j][2]) <= min(b[i][3], b[j][3]):
                    return True
    return False


def reached(geometry, sample, plane, shift, W=None, num_cu=NUM_CU, capacity=None, lists=None, walk=True):
    """{'pairs' | 'gram' | 'project': the names of BRANCHES this list executes}.  ``lists``: raw (images, cell_start, events)
    in the place of the ones the backend builds; ``walk=False``: the launches alone (a list too long for the wave-by-wave
    mirror -- then only the images of the second round are walked)."""
    K = len(sample)
    img, cell_start, events = lists_of(geometry, sample, plane, shift) if lists is None else lists
    n_images = len(img)
    pairs = {name for name in ed._image_branches(geometry, shift)[0] if name != 'image-clipped'}
    blocks = cdiv(n_images, WAVES)                                          # events_pairs
    grid = grid_for(blocks, num_cu)
    second = range(grid * WAVES, n_images)
    keys, groups, names = pairs_walk(geometry, img, cell_start, events, K, None if walk else second)
    pairs |= names
    if blocks > grid:
        pairs.add('P1:image-loop-strides')
        if len(pairs_walk(geometry, img, cell_start, events, K, second)[0]):
            pairs.add('P1:second-round-finds-pairs')
    if walk and len(keys) > len(np.unique(keys)):
        pairs.add('P4:pair-through-several-image-pairs')
    if capacity is not None and len(groups) == 1 and 0 < capacity < groups[0]:   # (one ballot: no order of arrival to win)
        pairs.add('P5:capacity-inside-a-ballot-group')
    taps = taps_of(geometry)
    gram = _tap_names('M', taps) | _occurrence_names('M', geometry, shift) | {'diagonal'}
    project = _tap_names('C', taps) | _occurrence_names('C', geometry, shift)
    if walk and len(keys):
        gram.add('off-diagonal')
    n_pairs = K + len(np.unique(keys))                                      # HIP.py gram_event_list: the diagonal, then i < j
    if cdiv(n_pairs, WAVES) > grid_for(cdiv(n_pairs, WAVES), num_cu):       # events_gram
        gram.add('M3:pair-loop-strides')
    if cdiv(K, WAVES) > grid_for(cdiv(K, WAVES), num_cu):                   # events_project
        project.add('C3:event-loop-strides')
    if walk and own_images_overlap(geometry, shift):
        gram.add('M2:own-images-overlap')
    if W is not None and walk:
        blank = blank_rows(geometry, plane, shift, W)
        if blank.any():
            gram.add('M4:row-without-inside-tap')
            project.add('C4:row-without-inside-tap')
            i, j = np.divmod(np.unique(keys), max(K, 1))
            if np.any(blank[i] | blank[j]):
                pairs.add('P4:zero-valued-candidate')
    out = {'pairs': pairs, 'gram': gram, 'project': project}
    for kernel, got in out.items():
        assert got <= set(BRANCHES[kernel]), (kernel, got - set(BRANCHES[kernel]))
    return out


# -- the matrix of lists ---------------------------------------------------------------------------------------------------------
STRIDE_ROWS = lambda cu: cu * 64 * WAVES + 300      # 300 more rows (images, in 'valid') than the waves of the grid


def _stride_samples(cu):
    return cdiv(STRIDE_ROWS(cu), 16)                # 16 of a sample's 84 places are rows: a well-conditioned Gram matrix


MATRIX = {
    # P1, M3, C3: 300 more rows than the grid has waves, on thousands of 40-sample signals under a 3-tap atom, about 16 rows
    # to a signal
    'stride': (lambda cu: (_stride_samples(cu), 1, 2, (40,), (3,), 'valid'),
               {'pairs': ('P1:image-loop-strides', 'P1:second-round-finds-pairs'), 'gram': ('M3:pair-loop-strides',),
                'project': ('C3:event-loop-strides',)}),
    # P2: 150 rows in the upper cell row of sample 0, three in the lower one; sample 1 has rows that reach its empty lower row
    'runs': (lambda cu: (2, 1, 2, (30, 12), (3, 3), 'valid'),
             {'pairs': ('P2:empty-run', 'P2:run-within-a-pass', 'P2:run-above-64-partial-last-pass')}),
    # P3: an 18 x 20 atom reaches three cell rows and three cell columns, every clamp decides; M1 / C1: 360 taps
    'tall-atom': (lambda cu: (2, 1, 2, (40, 50), (18, 20), 'valid'),
                  {'pairs': ('P3:cy0-clamped', 'P3:cx0-clamped', 'P3:cy1-clamped', 'P3:cx1-clamped', 'P3:three-cell-rows',
                             'P3:three-cell-columns'),
                   'gram': ('M1:taps-above-64-partial',), 'project': ('C1:taps-above-64-partial',)}),
    # P3 in 1-D: 300 taps reach three cells of 256
    'long-atom-1d': (lambda cu: (2, 1, 2, (600,), (300,), 'valid'), {'pairs': ('P3:three-cell-columns',)}),
    # P4, M2, C2: the widest geometries of the events matrix: every shift has two images in y that overlap each other
    'widest-circular': (ed.MATRIX['widest-circular'][0],
                        {'pairs': ('P4:pair-through-several-image-pairs',),
                         'gram': ('M2:widest-circular', 'M2:own-images-overlap', 'M2:two-images', 'M2:four-images'),
                         'project': ('C2:widest-circular', 'C2:two-images', 'C2:four-images')}),
    'widest-reflect': (ed.MATRIX['widest-reflect'][0],
                       {'pairs': ('P4:pair-through-several-image-pairs',),
                        'gram': ('M2:widest-reflect', 'M2:own-images-overlap', 'M2:one-image', 'M2:two-images', 'M2:four-images'),
                        'project': ('C2:widest-reflect', 'C2:one-image')}),
    # M1 / C1: the seams of the lane loop
    'one-tap': (lambda cu: (2, 1, 4, (9, 10), (1, 1), 'valid'), {'gram': ('M1:one-tap',), 'project': ('C1:one-tap',)}),
    'taps-64': (lambda cu: (2, 4, 3, (10, 11), (4, 4), 'full'), {'gram': ('M1:taps-64',), 'project': ('C1:taps-64',)}),
    # M4, C4, P4: the corner shift of plane 0 has one tap inside the sample, and W holds a 0 there
    'zero-tap': (lambda cu: (2, 2, 3, (6, 7), (2, 3), 'valid'),
                 {'pairs': ('P4:zero-valued-candidate',), 'gram': ('M4:row-without-inside-tap', 'M1:taps-below-64'),
                  'project': ('C4:row-without-inside-tap', 'C1:taps-below-64')}),
    # P5: row 0 in the middle of four rows that are close to it and not to each other: one ballot of four hits
    'ballot': (lambda cu: (1, 1, 1, (20, 20), (4, 4), 'valid'), {'pairs': ('P5:capacity-inside-a-ballot-group',)}),
    # P6: the lists of 'zero-tap' with images and one row doctored (doctored())
    'doctored': (lambda cu: (2, 2, 3, (6, 7), (2, 3), 'valid'),
                 {'pairs': ('P6:image-event-out-of-range', 'P6:image-position-negative', 'P6:image-cell-beyond',
                            'P6:image-sample-out-of-range', 'P6:other-event-out-of-range')}),
}
BALLOT_CAPACITY = 2


def geometry_of(name, num_cu=NUM_CU):
    return MATRIX[name][0](num_cu)


_CASES = {}


def matrix_case(name, num_cu=NUM_CU):
    """-> (geometry, sample, plane, shift, integer W in 0..3, integer V in 0..3), read-only: distinct rows in shuffled order
    (but 'ballot': the row in the middle is row 0)."""
    if (name, num_cu) in _CASES:
        return _CASES[name, num_cu]
    N, C, P, D, A, mode = geo = geometry_of(name, num_cu)
    S = eref.shift_shape(D, A, mode)
    rng = np.random.default_rng(zlib.crc32(('solve ' + name).encode()))
    space = (N, P) + tuple(S)
    W = rng.integers(0, 4, (P, C) + A).astype(np.float64)
    if name == 'stride':
        rows = ed._draw(rng, space, STRIDE_ROWS(num_cu))
    elif name == 'runs':
        rows = np.concatenate([ed._draw(rng, (1, P, 14, S[1]), 150),                                    # 150 in cell row 0
                               np.array([(0, 0, 20, 3), (0, 1, 22, 9), (0, 1, 25, 4)]),               # 3 in cell row 1
                               np.array([(1, 0, 14, 2), (1, 1, 15, 2), (1, 0, 3, 9)])])               # sample 1: none below
    elif name in ('widest-circular', 'widest-reflect'):
        _, s, pl, sh, _, W = ed.matrix_case(name)
        rows = np.column_stack([s, pl, sh])
        W = np.array(W)
    elif name == 'ballot':
        rows = np.array([(0, 0, 10, 10), (0, 0, 7, 7), (0, 0, 7, 13), (0, 0, 13, 7), (0, 0, 13, 13)])
        W = np.maximum(W, 1.)
    else:
        count = {'tall-atom': 60, 'long-atom-1d': 40, 'one-tap': 80, 'taps-64': 50}.get(name, 40)
        rows = {tuple(r) for r in ed._draw(rng, space, count).tolist()}
        rows |= {(0, 1) + tuple(c * (s - 1) for c, s in zip(corner, S)) for corner in np.ndindex(*(2,) * len(S))}
        if name in ('zero-tap', 'doctored'):
            # the blank rows (0, 0, 0, 0) and (1, 0, 0, 0), and rows close to the first: candidates with the value exactly 0
            W[0, :, -1, -1] = 0.
            rows |= {(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 2, 0, 1), (0, 0, 1, 0), (0, 0, 0, 1), (0, 2, 1, 2)}
        rows = np.array(sorted(rows), dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    assert len(np.unique(rows, axis=0)) == len(rows)
    if name != 'ballot':
        rows = rows[rng.permutation(len(rows))]
    V = rng.integers(0, 4, (N, C) + D).astype(np.float64)
    out = (geo, rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2:].copy(), W, V)
    for a in out[1:]:
        a.setflags(write=False)
    _CASES[name, num_cu] = out
    return out


def doctored(num_cu=NUM_CU):
    """-> (images, cell_start, events, the events whose images and row are left alone) of 'doctored': the lists of the case
    with four images and one row put outside the contract, each in its own way.  The images stay where the sort put them."""
    geo, sample, plane, shift, _, _ = matrix_case('doctored', num_cu)
    K = len(sample)
    _, _, ncy, ncx = cells_of(geo)
    ty, tx = ed.events_tile(2)
    img, cell_start, events = (np.array(a) for a in lists_of(geo, sample, plane, shift))
    victims = [int(e) for e in np.flatnonzero(sample == 0)[:5]]
    at = [int(np.flatnonzero(img[:, 3] == e)[0]) for e in victims]
    img[at[0], 3] = K + 3                    # an event index of at least K
    img[at[1], 1] = -2                       # a negative position
    img[at[2], 2] = ncx * tx + 1             # a cell beyond ncx
    img[at[3], 1] = ncy * ty                 # a cell beyond ncy
    events[victims[4], 0] = geo[0] + 1       # its event's sample at least N
    clean = np.setdiff1d(np.arange(K), victims)
    return img, cell_start, events, clean


# -- the solver ------------------------------------------------------------------------------------------------------------------
BANDS = {'narrow': (5, 3, 2), 'wide': (8, 7, 6)}
SCALE = {'narrow': 128, 'wide': 256}       # L, a power of two: attained by the hub rows, and by no other


def nnls_system(K, band='narrow', seed=0):
    """-> dict(K, csr=(row_start, col, val), c, start, L, hubs, margin): a synthetic system for the solver, integers throughout.
    A band of three neighbours on either side; rows that gather 9, 13 and 36 far links of value 1 (16, 20 and 43 entries with
    the band and the diagonal: one pass of the row loop exactly, two, three) where K has room for them; one row without any
    entry (row 5, K >= 64).  The diagonal is the row's off-diagonal sum plus 1..3 -- Gershgorin: lambda_min >= 1 --, at a hub
    L minus that sum.  The hubs sit at K - 1 and, where they exist, at 300 and 4099; max |c| at K - 2; the start's largest
    |pg| at K - 3."""
    rng = np.random.default_rng(1000 * K + seed + (7 if band == 'wide' else 0))
    L = SCALE[band]
    off = {}

    def link(i, j, v):
        assert i != j and (i, j) not in off
        off[i, j] = off[j, i] = v
    empty = 5 if K >= 64 else None
    for i in range(K):
        for d, v in enumerate(BANDS[band], start=1):
            if i + d < K and empty not in (i, i + d):
                link(i, i + d, v)
    hubs = [h for h in (300, 4099, K - 1) if 40 <= h < K and K >= 64]
    hubs = sorted(set(hubs))
    gather = [(h, 36) for h in hubs]
    if K >= 64:
        gather += [(20, 9), (40, 13)]
    for h, count in gather:
        free = [j for j in range(K) if abs(j - h) > 3 and j != empty and (h, j) not in off and all(abs(j - g) > 3 for g, _ in gather)]
        for j in rng.choice(free, count, replace=False).tolist():
            link(h, int(j), 1)
    rows = [[] for _ in range(K)]
    for (i, j), v in off.items():
        rows[i].append((j, v))
    total = np.array([sum(v for _, v in r) for r in rows], dtype=np.int64)
    diag = total + rng.integers(1, 4, K)
    tops = hubs if hubs else [K - 1]
    for h in tops:                              # the rows that attain L (without hubs: the last row, by its diagonal)
        diag[h] = L - total[h]
    assert np.all(diag > total) and np.all((diag + total)[np.setdiff1d(np.arange(K), tops)] < L)
    row_start, col, val = [0], [], []
    for i in range(K):
        entries = sorted(rows[i] + ([(i, int(diag[i]))] if i != empty else []))
        col += [j for j, _ in entries]
        val += [v for _, v in entries]
        row_start.append(len(col))
    c = rng.integers(-30, 90, K).astype(np.float64)
    start = rng.integers(0, 4, K).astype(np.float64)       # zeros among them
    if K >= 2:
        c[K - 2] = 200.
    if K >= 3:
        start[K - 3] = 40.
    if empty is not None:
        start[empty] = 3.                      # an inactive row with a positive start
    out = dict(K=K, csr=(np.array(row_start, dtype=np.int64), np.array(col, dtype=np.int64), np.array(val, dtype=np.float64)),
               c=c, start=start, L=float(L), hubs=tops, margin=float(np.min(np.delete(diag - total, empty) if empty is not None
                                                                             else diag - total)), empty=empty)
    for a in out['csr'] + (c, start):
        a.setflags(write=False)
    return out


def doctor_csr(system):
    """-> (row_start, col, val, the sanitised triple's reference arguments): the system's CSR put outside the contract -- a
    column of -1 and one of K in place of two entries, a negative row_start, one above nnz, one that decreases -- with 64
    entries of slack behind it (NaN values under valid columns: a run that is not clamped reads them).  nnz is the length
    WITHOUT the slack."""
    K = system['K']
    row_start, col, val = (np.array(a) for a in system['csr'])
    nnz = len(val)
    col[row_start[7] + 1] = -1
    col[row_start[9] + 2] = K
    row_start[0] = -3                          # row 0 begins at max(-3, 0)
    row_start[30] = row_start[29] - 2          # decreases: row 29 is empty, row 30 begins two entries early
    row_start[K] = nnz + 40                    # row K - 1 ends at nnz
    slack = 64
    col = np.concatenate([col, np.arange(slack) % K])
    val = np.concatenate([val, np.full(slack, np.nan)])
    return row_start, col, val, nnz


def row_lengths(K, row_start, nnz):
    """csr_run: the clamped run of every row."""
    a = np.minimum(np.maximum(np.asarray(row_start[:-1]), 0), nnz)
    b = np.minimum(np.maximum(np.asarray(row_start[1:]), a), nnz)
    return a, b


def solver_reached(K, row_start, col, val, nnz, c, start, tol, max_iterations, check_every, history_capacity, follow=0):
    """{kernel: names} of one tnmf_hip_events_nnls call.  ``follow``: the iterations whose restart tests are looked at
    (sr.nnls_iterates)."""
    row_start, col, val = np.asarray(row_start), np.asarray(col), np.asarray(val)
    out = {k: set() for k in BRANCHES if k.startswith('nnls')}
    a, b = row_lengths(K, row_start, nnz)
    blocks, rem = cdiv(K, ROWS_PER_BLOCK), K % ROWS_PER_BLOCK
    rows = out['nnls_rows']
    for n in (b - a).tolist():
        rows.add('S1:row-empty' if n == 0 else 'S1:row-1..15' if n < ROW_LANES else 'S1:row-16' if n == ROW_LANES else
                 'S1:row-17..32' if n <= 2 * ROW_LANES else 'S1:row-above-32')
    out['nnls_step'] |= set(rows)
    rows.add('S2:one-block' if blocks == 1 else 'S2:several-blocks')
    if rem:
        rows.add('S2:partial-last-block')
        out['nnls_step'].add('S2:partial-last-block')
    if np.any(row_start[:-1] < 0) or np.any(row_start[1:] < 0):
        rows.add('S6:row-start-negative')
    if np.any(row_start > nnz):
        rows.add('S6:row-start-above-nnz')
    if np.any(np.maximum(row_start[1:], 0) < np.minimum(np.maximum(row_start[:-1], 0), nnz)):
        rows.add('S6:row-start-decreases')
    r, cc, vv = sr.csr_entries(K, row_start, col[:nnz], val[:nnz])
    if len(r) < int(np.sum(b - a)):
        rows.add('S6:col-skipped')
    has = np.bincount(r[r == cc], minlength=K) > 0
    diag = np.bincount(r[r == cc], weights=vv[r == cc], minlength=K)
    rowabs = np.bincount(r, weights=np.abs(vv), minlength=K)
    if np.any(~has):
        rows.add('S5:row-without-diagonal')
    if np.any(has & (diag <= 0)):
        rows.add('S5:diagonal-not-positive')
    act = diag > 0
    scale = out['nnls_scale']
    scale.add('S2:one-pass' if K <= THREADS else 'S2:second-pass')
    if K % THREADS:
        scale.add('S2:partial-last-pass')
    L, cmax = rowabs.max(), np.abs(c).max()
    if K > THREADS and not np.any(rowabs[:THREADS] == L):
        scale.add('S3:L-beyond-the-first-pass')
    if K > THREADS and not np.any(np.abs(c[:THREADS]) == cmax):
        scale.add('S3:cmax-beyond-the-first-pass')
    last_block = np.arange(K) >= (K // ROWS_PER_BLOCK) * ROWS_PER_BLOCK
    if rem and np.all(last_block[np.abs(c) == cmax]):
        scale.add('S3:cmax-in-the-last-partial-block')
    first = out['nnls_start']
    first.add('S2:one-block' if K <= THREADS else 'S2:second-block')
    if K % THREADS:
        first.add('S2:partial-last-block')
    with np.errstate(invalid='ignore'):
        for flag, name in ((np.isnan(start), 'S5:start-nan'), (start < 0, 'S5:start-negative'), (start == 0, 'S5:start-zero'),
                           (start > 0, 'S5:start-positive'), (~act & (start > 0), 'S5:inactive-row-with-positive-start')):
            if np.any(flag):
                first.add(name)
    step, reduce_, host = out['nnls_step'], out['nnls_reduce'], out['nnls_host']
    if np.any(~act):
        step.add('S5:inactive-row')
    if rem and np.any(last_block & (rowabs == L) & ((b - a) > 2 * ROW_LANES)):
        step.add('S3:hub-in-the-last-partial-block')
    reduce_.add('S2:one-pass' if blocks <= THREADS else 'S2:second-pass')
    its = sr.nnls_iterates((row_start, col[:nnz], val[:nnz]), c, start, max(follow, 1))
    if blocks > THREADS:
        x0, _, _, _, _ = its[0]
        g = np.bincount(r, weights=vv * x0[cc], minlength=K) - c
        pg = np.where(act, np.where(x0 > 0, np.abs(g), np.maximum(-g, 0.)), 0.)
        block_of = np.arange(K) // ROWS_PER_BLOCK
        if np.all(block_of[pg == pg.max()] >= THREADS):
            reduce_.add('S3:pg-max-beyond-the-first-pass')
        x1 = its[1][0]
        if np.any((x1 != x0)[block_of >= THREADS]):     # (beta = 0: y = x, the term is -(x1 - x0)^2)
            reduce_.add('S3:restart-term-beyond-the-first-pass')
    steps = min(follow, max_iterations)
    for k, (x, _, restarted, _, _) in enumerate(its[:steps]):
        reduce_.add('S4:restart' if restarted else 'S4:no-restart')
        following = its[k + 1][0]
        step.add('projection-decides' if np.any(act & (following == 0)) else 'projection-idle')
    if steps >= 1:
        step.add('S4:beta-zero')
    if steps >= 3 and not (its[0][2] and its[1][2]):   # (the first two coefficients are 0 whatever the test says)
        step.add('S4:beta-positive')
    if max_iterations == 0:
        host.add('max-iterations-0')
    kkts = [k for _, k, _, _, _ in its]
    checks = [it for it in range(max_iterations + 1) if it % check_every == 0 or it == max_iterations]
    known = [it for it in checks if it < len(kkts)]
    done = next((it for it in known if kkts[it] <= tol), None)
    if done is not None:
        host.add('converges')
        checks = [it for it in checks if it <= done]
    elif max_iterations < len(kkts):
        host.add('stops-at-max-iterations')
    if check_every == 1:
        host.add('S7:check-every-1')
    if check_every == 7:
        host.add('S7:check-every-7')
    if check_every > max_iterations > 0:
        host.add('S7:check-every-above-max-iterations')
    if max_iterations % check_every:
        host.add('S7:max-iterations-not-a-multiple')
    if history_capacity is None:
        host.add('S7:history-null')
    elif history_capacity < len(checks):
        host.add('S7:history-capacity-short')
    for kernel, got in out.items():
        assert got <= set(BRANCHES[kernel]), (kernel, got - set(BRANCHES[kernel]))
    return out


TOL = 1e-8
SIZES = (1, 15, 16, 17, 256, 257, 4096, 4137)      # S2
BIG = 4137                                           # above 4096 and no multiple of 16: 259 blocks, the last of nine rows

# name -> (K, band, what is done to the system, (max_iterations, check_every, history_capacity), the items it is there for)
SYSTEMS = {}
for _K in SIZES:
    SYSTEMS[f'K-{_K}'] = (_K, 'narrow', None, (400, 1, 401), {})
SYSTEMS['K-1'][4].update({'nnls_rows': ('S2:one-block', 'S1:row-1..15'), 'nnls_step': ('S1:row-1..15',)})
SYSTEMS['K-15'][4].update({'nnls_rows': ('S2:partial-last-block',)})
SYSTEMS['K-16'][4].update({'nnls_rows': ('S2:one-block',)})
SYSTEMS['K-17'][4].update({'nnls_rows': ('S2:several-blocks', 'S2:partial-last-block'), 'nnls_step': ('S2:partial-last-block',)})
SYSTEMS['K-256'][4].update({'nnls_scale': ('S2:one-pass',), 'nnls_start': ('S2:one-block',),
                            'nnls_rows': ('S1:row-empty', 'S1:row-16', 'S1:row-17..32', 'S1:row-above-32'),
                            'nnls_step': ('S1:row-empty', 'S1:row-16', 'S1:row-17..32', 'S1:row-above-32')})
SYSTEMS['K-257'][4].update({'nnls_scale': ('S2:second-pass', 'S2:partial-last-pass', 'S3:L-beyond-the-first-pass'),
                            'nnls_start': ('S2:second-block', 'S2:partial-last-block')})
SYSTEMS['K-4096'][4].update({'nnls_reduce': ('S2:one-pass',)})
SYSTEMS['K-4137'][4].update({'nnls_reduce': ('S2:second-pass', 'S3:pg-max-beyond-the-first-pass',
                                             'S3:restart-term-beyond-the-first-pass', 'S4:restart', 'S4:no-restart'),
                             'nnls_scale': ('S3:L-beyond-the-first-pass', 'S3:cmax-beyond-the-first-pass',
                                            'S3:cmax-in-the-last-partial-block'),
                             'nnls_step': ('S3:hub-in-the-last-partial-block', 'S4:beta-zero', 'S4:beta-positive'),
                             'nnls_host': ('S7:check-every-1',)})
SYSTEMS['wide-4137'] = (BIG, 'wide', None, (400, 1, 401),
                        {'nnls_reduce': ('S2:second-pass', 'S4:restart', 'S4:no-restart')})
SYSTEMS['starts'] = (257, 'narrow', 'starts', (400, 1, 401),
                     {'nnls_start': ('S5:start-nan', 'S5:start-negative', 'S5:start-zero', 'S5:start-positive',
                                     'S5:inactive-row-with-positive-start'),
                      'nnls_rows': ('S5:row-without-diagonal', 'S5:diagonal-not-positive'),
                      'nnls_step': ('S5:inactive-row',)})
SYSTEMS['doctored-csr'] = (257, 'narrow', 'csr', (400, 1, 401),
                           {'nnls_rows': ('S6:col-skipped', 'S6:row-start-negative', 'S6:row-start-above-nnz',
                                          'S6:row-start-decreases')})
SYSTEMS['every-7'] = (257, 'narrow', None, (45, 7, 3),
                      {'nnls_host': ('S7:check-every-7', 'S7:max-iterations-not-a-multiple', 'S7:history-capacity-short')})
SYSTEMS['every-above'] = (257, 'narrow', None, (5, 9, None),
                          {'nnls_host': ('S7:check-every-above-max-iterations', 'S7:history-null')})
SYSTEMS['no-iterations'] = (BIG, 'narrow', None, (0, 1, 4), {'nnls_host': ('max-iterations-0',)})

_SYSTEMS = {}


def system_case(name):
    """-> dict(K, row_start, col, val, nnz, c, start, L, margin, params): the arrays as the solver is given them (col and val
    may be longer than nnz: doctor_csr's slack), read-only."""
    if name in _SYSTEMS:
        return _SYSTEMS[name]
    K, band, doctor, params, _ = SYSTEMS[name]
    s = nnls_system(K, band)
    row_start, col, val = s['csr']
    nnz, start = len(val), s['start']
    if doctor == 'csr':
        row_start, col, val, nnz = doctor_csr(s)
    if doctor == 'starts':
        start, val = np.array(start), np.array(val)
        start[[3, 60, 100]] = np.nan
        start[[4, 61, 256]] = -2.
        start[7], start[8] = 0., 5.
        val[row_start[8] + int(np.flatnonzero(col[row_start[8]:row_start[9]] == 8)[0])] = 0.   # a diagonal of 0: inactive
    out = dict(K=K, row_start=np.asarray(row_start), col=np.asarray(col), val=np.asarray(val), nnz=nnz, c=s['c'],
               start=np.asarray(start), L=s['L'], margin=s['margin'], params=params, hubs=s['hubs'], empty=s['empty'])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _SYSTEMS[name] = out
    return out


_ITERATES = {}


def reference_iterates(name, n=400):
    """sr.nnls_iterates of the case in CSR order, up to the first iterate with kkt <= TOL (at most n), cached."""
    if name not in _ITERATES:
        s = system_case(name)
        its = sr.nnls_iterates((s['row_start'], s['col'][:s['nnz']], s['val'][:s['nnz']]), s['c'], s['start'], n)
        done = next((k for k, it in enumerate(its) if it[1] <= TOL), n)
        _ITERATES[name] = its[:done + 2]         # (the iterate accepted and the one the extra launch pair computes)
    return _ITERATES[name]


def system_reached(name):
    s = system_case(name)
    max_iterations, check_every, capacity = s['params']
    follow = len(reference_iterates(name)) - 2
    return solver_reached(s['K'], s['row_start'], s['col'], s['val'], s['nnz'], s['c'], s['start'], TOL, max_iterations,
                          check_every, capacity, follow=follow)


# Level (c) of the GPU test, the kkt history wherever the reference's kkt is at least 1e-6.  Measured on the CPU
# (tests/test_solve_dispatch_cpu.py prints it): two float64 evaluations of the reference that sum the rows in different
# orders, CSR order against dense, diverge by at most ORDER_DIVERGENCE relative over the cases; the GPU's lane split and
# fused multiply-adds are a third order of the same sums and the iteration contracts, so a hundred times that is allowed.
ORDER_DIVERGENCE = 5e-11        # (the largest of the cases: 4.83e-11, 'K-4137')
KKT_HISTORY_BAR = 100 * ORDER_DIVERGENCE
# The iterates themselves, relative to the largest strength, between the same two orders: at most 9.42e-16 ('K-4137').
ORDER_DIVERGENCE_X = 1e-15
ITERATE_BAR = 100 * ORDER_DIVERGENCE_X
