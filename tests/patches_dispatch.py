"""
The host mirror of the two launches of tnmf_amd/csrc/patches.hip -- which branch of k_events_patches a row takes, the grid
and the LDS of its launch, the work units of k_patch_moments -- and the smallest cases that reach every branch.
tests/test_patches_dispatch_cpu.py holds the constants to the sources read as text and the cases to the branches;
tests/test_hip_patches.py runs the cases on the device.
"""
import numpy as np

import patches_reference as pref

WAVES = 4                 # kEventThreads / 64
PER_CU = 8                # TNMF_PATCHES_BLOCKS_PER_CU
STAGE_MAX = 2048          # TNMF_PATCH_STAGE_MAX
BLOCK, DEPTH = 16, 4      # kMomentBlock, kMomentDepth
SEGMENT = 64              # TNMF_EVENTS_SEGMENT: the unit of the backend's chunks

PATCH_BRANCHES = ('row-out-of-range', 'single-whole', 'single-clipped', 'two-images', 'four-images', 'reflect-overlap',
                  'taps-below-64', 'taps-not-a-multiple-of-64', 'taps-above-128', 'event-loop-strides')
MOMENT_BRANCHES = ('atom-without-rows', 'one-row', 'rows-not-a-multiple-of-4', 'run-not-aligned-to-4', 'more-than-a-segment',
                   'one-block', 'last-block-partial', 'several-blocks', 'entry-out-of-range')


def patches_launch(n_events, N, C, A, with_table, num_cu):
    """-> (grid, LDS bytes) of the launch, None when nothing is launched, 'geom' when the staged patch does not fit."""
    taps = C * int(np.prod(A))
    if with_table and taps > STAGE_MAX:
        return 'geom'
    if n_events <= 0 or N <= 0:
        return None
    return max(1, min(-(-n_events // WAVES), num_cu * PER_CU)), (WAVES * taps * 8 if with_table else 0)


def row_branches(N, C, P, D, A, mode, row):
    """The branches of k_events_patches the row (n, p, *u) takes (the sources and the table are arguments of the launch)."""
    S = pref.shift_shape(D, A, mode)
    if not pref.in_range([row], N, P, S)[0]:
        return {'row-out-of-range'}
    per_axis = [pref.axis_images(int(u), a, s, mode) for u, a, s in zip(row[2:], A, S)]
    n_images = int(np.prod([len(q) for q in per_axis]))
    out = set()
    if n_images == 1:
        whole = all(q[0] - (a - 1) >= 0 and q[0] + 1 <= d for q, a, d in zip(per_axis, A, D))
        out.add('single-whole' if whole else 'single-clipped')
    else:
        out.add('two-images' if n_images == 2 else 'four-images')
    if mode == 'reflect' and any(1 <= int(u) <= a - 1 for u, a in zip(row[2:], A)):
        out.add('reflect-overlap')
    return out


def launch_branches(n_events, C, A, num_cu):
    taps = C * int(np.prod(A))
    out = {'taps-below-64' if taps < 64 else 'taps-above-128' if taps > 128 else 'taps-not-a-multiple-of-64' if taps % 64
           else 'taps-a-multiple-of-64'}
    if -(-n_events // WAVES) > num_cu * PER_CU:
        out.add('event-loop-strides')
    return out


# -- the cases of tnmf_hip_events_patches: name -> (N, C, P, D, A, mode, the transforms whose tables the case runs) ----------
# P is a multiple of every T; 'T1' is the table of one map (a magnification by 2: weighted entries and pixels without an
# entry), 'rot8' transforms.rotations((5, 5), 8)
PATCH_CASES = {
    'valid-2d': (2, 1, 4, (9, 11), (3, 4), 'valid', (None,)),          # clipped at every border; taps 12
    'full-2d': (2, 1, 4, (9, 11), (3, 4), 'full', (None,)),
    'circular-2d': (2, 1, 4, (9, 11), (3, 4), 'circular', (None,)),    # 2 and 4 images
    'reflect-2d': (2, 1, 4, (9, 11), (3, 4), 'reflect', (None,)),      # images that overlap inside the sample
    'c3-5x5': (2, 3, 8, (9, 11), (5, 5), 'circular', (None, 'rot90', 'rot8', 'T1')),   # taps 75
    '12x12': (2, 1, 4, (13, 14), (12, 12), 'reflect', (None, 'rot90')),               # taps 144
    '1d-5': (2, 1, 4, (40,), (5,), 'circular', (None, 'flip')),                       # one shift axis, taps 5
    '1d-valid': (2, 2, 2, (40,), (5,), 'valid', (None,)),
    'grid-stride': (2, 1, 2, (40,), (5,), 'reflect', (None,)),         # more rows than one pass of the grid takes
}
GRID_STRIDE_ROWS = 9000    # > 4 * PER_CU * 256: beyond one pass on any device of up to 256 CUs


def patch_rows(name):
    """-> (rows [K, 2 + k] int64 with rows out of range in place, strengths float32-representable), shuffled."""
    N, C, P, D, A, mode, _ = PATCH_CASES[name]
    S = pref.shift_shape(D, A, mode)
    rng = np.random.default_rng(sorted(PATCH_CASES).index(name))

    def random_rows(count):
        return np.column_stack([rng.integers(N, size=count), rng.integers(P, size=count)]
                               + [rng.integers(s, size=count) for s in S]).astype(np.int64)
    if name == 'grid-stride':
        rows = random_rows(GRID_STRIDE_ROWS)
    else:
        every = np.array([(1, P - 1) + u for u in np.ndindex(*S)], dtype=np.int64)   # every zone of every axis
        if len(every) > 160:
            every = every[rng.choice(len(every), 160, replace=False)]
        corners = np.array([(0, 0) + tuple(c * (s - 1) for c, s in zip(corner, S)) for corner in np.ndindex(*(2,) * len(S))])
        rows = np.concatenate([every, corners, random_rows(40)])
        rows = np.concatenate([rows, rows[:5]])                                     # duplicates
        bad = rows[5:12].copy()                                                     # rows outside the contract
        bad[0, 0], bad[1, 0], bad[2, 1], bad[3, 1], bad[4, 2], bad[5, -1], bad[6, 2] = N, -1, P, -2, S[0], S[-1], -5
        rows = np.concatenate([rows, bad])
    h = (rng.random(len(rows)) + 0.5).astype(np.float32).astype(np.float64)
    if name != 'grid-stride':
        h[len(rows) - 12:len(rows) - 7] = h[:5]                                     # (the duplicates: strengths too)
    order = rng.permutation(len(rows))
    return rows[order], h[order]


# -- the cases of tnmf_hip_patch_moments ---------------------------------------------------------------------------------------
MOMENT_D = (5, 16, 25, 48, 75)
# rows per atom: none, one, three (not a multiple of the MFMA depth), a segment and one -- and, from the runs before it not
# adding up to a multiple of four, runs that do not begin at a multiple of four
MOMENT_RUNS = (0, 1, 3, SEGMENT + 1, 0, 6)


def moments_launch(D, n_atoms):
    """-> (blocks per side, pairs of blocks, work units, grid)."""
    nb = -(-D // BLOCK)
    pairs = nb * (nb + 1) // 2
    return nb, pairs, n_atoms * pairs, -(-n_atoms * pairs // WAVES)


def block_pair(pair, nb):
    """(I, J), I <= J, of index ``pair`` in the order (0,0) (0,1) .. (0,nb-1) (1,1) .."""
    I = 0
    while pair >= nb - I:
        pair -= nb - I
        I += 1
    return I, I + pair


def fours(a, b):
    """The positions at which k_patch_moments begins its MFMAs over the run [a, b)."""
    return list(range(a - a % DEPTH, b, DEPTH)) if b > a else []


def moment_branches(D, runs, with_bad_entry=False):
    out = set()
    start = np.concatenate([[0], np.cumsum(runs)])
    for a, b in zip(start[:-1], start[1:]):
        n = b - a
        out |= {'atom-without-rows'} if n == 0 else set()
        out |= {'one-row'} if n == 1 else set()
        out |= {'rows-not-a-multiple-of-4'} if n % DEPTH else set()
        out |= {'run-not-aligned-to-4'} if n and a % DEPTH else set()
        out |= {'more-than-a-segment'} if n > SEGMENT else set()
    nb = -(-D // BLOCK)
    out.add('one-block' if nb == 1 else 'several-blocks')
    if D % BLOCK:
        out.add('last-block-partial')
    if with_bad_entry:
        out.add('entry-out-of-range')
    return out
