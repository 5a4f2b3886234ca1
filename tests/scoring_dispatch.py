"""
Host mirror of the launches and the control flow of the seven kernels that score events -- k_events_gain
(tnmf_amd/csrc/events.hip), k_events_norms, k_pursuit_score, k_pursuit_taken, k_pursuit_pick (pursuit.hip),
k_events_landscape (landscape.hip) and k_events_alternatives (alternatives.hip) -- restated in plain Python in the manner of
tests/events_dispatch.py and tests/solve_dispatch.py, so that tests/test_hip_scoring_matrix.py can choose small problems that
execute every branch of them and tests/test_scoring_dispatch_cpu.py can check without a GPU that the choice covers them all.

Three kinds of cases in one MATRIX, name -> (kind, lambda num_cu: spec, {kernel: the items the case is there for}):
  'norms'   spec = a geometry (N, C, P, D, A, mode); the table of one dictionary of integers.
  'score'   spec = (N, P, Sy, Sx, pad, a_off, gain_off, in_place, n_taken): a map of [N, P, Sy, Sx] with rows Sx + pad apart,
            the pointers a_off / gain_off elements behind a 16-byte boundary; both element types (kV = 4 and 2).
  'events'  spec = (geometry, (n_alt, stride), kernels, rows): a list of rows for the pick, the gain, the landscape and the
            alternatives, drawn (with repeats where the list has to be long) from a pool of distinct places.

Every events and norms case is integer-valued: W, V and R in 0..3, strengths multiples of 1/2 in 0..3.  Every product and every
double sum is then an integer or a dyadic rational with denominator at most 8, far below 2^53 (magnitude_bound), exact in any
order: the device must equal the float64 references bit for bit.

The wrong models at the end are the references with one defect each, in plain numpy: tests/test_scoring_dispatch_cpu.py
asserts that each differs from the right answer on the case named for the branch -- the proof that the case could catch it.
"""
import zlib

import numpy as np

import alternatives_reference as aref
import events_dispatch as ed
import events_gain_reference as gref
import landscape_reference as lref
import pursuit_reference as pur
import solve_dispatch as sd
from events_dispatch import cdiv, dims, shift_shape

NUM_CU = ed.NUM_CU
THREADS = ed.THREADS                # events.h, kEventThreads
WAVES = THREADS // 64               # kWaves of pursuit.hip, landscape.hip, alternatives.hip, events.hip
PATCH_MAX = 2048                    # landscape.hip and alternatives.hip, kPatchMax
BATCH = 4                           # alternatives.hip, kBatch
PER_CU = {'norms': 8, 'score': 8, 'taken': 8, 'pick': 64, 'gain': 64, 'landscape': 4, 'alternatives': 4}
DENOMINATOR = 8                     # every reference value times this is an integer
NOT_REACHED = {'score': ('not-reached: needs 2^31 elements',)}   # per_sample > 0x7fffffff: an 8 GB map

BRANCHES = {
    'norms': (
        'taps<256', 'taps==256',            # for (t = threadIdx.x; t < taps; t += kEventThreads): one pass
        'N1:second-tap-pass',               # ... taps > kEventThreads
        'N1:partial-last-tap-pass',         # ... and taps % kEventThreads != 0
        'entries<256', 'partial-last-block',   # e < entries cuts the first / the last workgroup
        'N2:entry-loop-strides',            # e += gridDim.x * kEventThreads: cdiv(entries, 256) > num_cu * 8
        'N3:not-single', 'N3:oy0<0', 'N3:ox0<0', 'N3:bottom-clipped', 'N3:right-clipped',   # !o.single() || oy0 < 0 || ox0 < 0
        'N3:shortcut',                      # || oy0 + g.Ay > g.Dy || ox0 + g.Ax > g.Dx: each term alone, and none
        'one-image', 'two-images', 'four-images',   # for_each_tap / phi_at: o.ny * o.nx
        'N4:widest-circular', 'N4:widest-reflect',  # A - 1 == S / A - 1 == S - 1 on an axis
        'N4:own-images-overlap',            # phi_at adds two taps on one pixel: b carries the cross term
        'N4:full-S==1',                     # 'full' with the atom as long as the sample on an axis
        'C>1', 'P==1', 'P>1',               # c * AA; blockIdx.y
    ),
    'score': (
        'aligned',                          # aligned16(a) && aligned16(gain) && Hs % kV == 0
        'S1:a-misaligned', 'S1:gain-misaligned',    # ... one pointer alone decides
        'a-and-gain-misaligned',            # ... both: a view of a larger buffer, scored in place
        'Hs-breaks-alignment',              # ... Hs % kV != 0
        'collapsed-to-one-row',             # Hs == Sx && per_sample <= 0x7fffffff && per_sample % kV == 0
        'S2:not-collapsed-per_sample%kV',   # ... contiguous, and per_sample % kV != 0 decides
        'whole-chunk', 'row-end-chunk',     # kAligned && x0 + kV <= Sx
        'Sx<kV',                            # cpr == 1 and the chunk is partial
        'S3:row_step==0',                   # stride / cpr == 0 and the loop takes a second pass: a row longer than the grid
        'row_step>0',                       # ... a second pass that moves on by whole rows
        'chunk-carry',                      # if (chunk >= cpr) chunk -= cpr, ++row, ++brow; -- before a chunk that is visited
        'brow-wraps',                       # if (brow >= brows) brow -= brows; -- likewise
        'in-place',                         # gain == a
        'not-reached: needs 2^31 elements',   # per_sample > 0x7fffffff
    ),
    'taken': (
        'below-range', 'above-range',       # if (f < 0 || f >= entries) continue;
        'duplicate-index',                  # two threads store the same zero
        'padded-rows',                      # Hs != Sx: row * Hs + (f - row * Sx)
        'collapsed-view',                   # Sx = Hs = per_sample: row is the sample
        'T1:loop-strides',                  # i += gridDim.x * kEventThreads: cdiv(n_taken, 256) > num_cu * 8
    ),
    'pick': (
        'one-image', 'two-images', 'four-images', 'image-clipped',   # Occurrence, for_each_tap
        'K1:one-tap', 'K1:taps-64', 'K1:taps-65',   # for_each_tap(lane, 64): one lane; every lane once; lane 0 twice
        'lane-loop-strides',                # taps > 64
        'K2:event-loop-strides',            # e += gridDim.x * kWaves: cdiv(n, 4) > num_cu * 64
        'K3:widest-circular', 'K3:widest-reflect', 'K3:full-S==1',
        'index-below-range', 'index-above-range',   # if (f < 0 || f >= entries)
        'first-entry', 'last-entry',        # f == 0, f == entries - 1
        'P-not-a-power-of-two',             # np / g.P, np % g.P
        'a<0', 'a==0',                      # live = a > 0. && b > 0.
        'K4:b==0',                          # ... a clipped shift of a plane with non-zero taps that shows only zero taps
        'mag-null',                         # if (mag)
    ),
    'gain': (
        'Q1:one-tap', 'Q1:taps-64', 'Q1:taps-65',
        'Q2:widest-circular', 'Q2:widest-reflect', 'Q2:full-S==1',
        'event-loop-strides',               # cdiv(n, 4) > num_cu * 64
        'row-out-of-range',                 # (unsigned)v.x >= (unsigned)g.N || ...
        'h==0', 'mag-null',
    ),
    'landscape': (
        'staged', 'walk',                   # landscape_staged()
        'L1:staged-after-walk-in-one-wave', 'L1:walk-after-staged-in-one-wave',   # consecutive passes of the event loop
        'L1:staged-after-staged',           # ... the patch is reused
        'L2:patch-limit-2d-fits',           # cells <= kPatchMax with cells == kPatchMax, two shift axes
        'L2:patch-limit-2d-does-not-fit',   # ... one column more: patch = 0, rows that would be staged walk
        'cells<64', 'cell-loop-strides',    # for (i = lane; i < cells; i += 64)
        'L3:one-tap', 'L3:taps-64', 'L3:taps-65',
        'neighbour-outside-the-shift-shape',   # (unsigned)uy < (unsigned)Sy && (unsigned)ux < (unsigned)Sx
        'L4:widest-circular', 'L4:widest-reflect',
        'L4:full-S==1',                     # only the centre neighbour exists
        'ry==0', 'ry==1',                   # nb = ry ? 9 : 3
        '1d-C>1',                           # c = t / uAx of the 1-D staged loop
        'row-out-of-range', 'event-loop-strides',   # cdiv(n, 4) > num_cu * TNMF_LANDSCAPE_BLOCKS_PER_CU
        'mag-null',
    ),
    'alternatives': (
        'staged', 'walk',                   # alternatives_staged()
        'live==1', 'live==2', 'live==3', 'live==4',   # live = min(kBatch, n_alt - j0)
        'several-batches',                  # j0 += kBatch takes a second pass
        'A1:zero-fill-beyond-a-wave',       # for (j = lane; j < n_alt; j += 64) of a refused row, n_alt > 64
        'stride>1', 'p%stride!=0',          # v.y / block * block + v.y % stride
        'second-block',                     # v.y / block > 0
        'A2:patch-limit-2d-fits', 'A2:patch-limit-2d-does-not-fit',
        'A3:one-tap', 'A3:taps-64', 'A3:taps-65',
        'A4:widest-circular', 'A4:widest-reflect',
        'staged-after-walk-in-one-wave', 'walk-after-staged-in-one-wave',
        'event-loop-strides', 'row-out-of-range', 'mag-null',
    ),
}

NEW = {kernel: tuple(b for b in names if b[0] in 'NSTKQLA' and b[1].isdigit() and b[2] == ':')
       for kernel, names in BRANCHES.items()}


# -- the launch rules ----------------------------------------------------------------------------------------------------------
def events_grid(blocks, num_cu=NUM_CU, per_cu=64):
    """events.h events_grid."""
    return max(1, min(blocks, num_cu * per_cu))


def wave_of(e, grid):
    """The wave (blockIdx.x * kWaves + wave) that takes row e of a one-wave-per-row kernel launched with `grid` workgroups."""
    return e % (grid * WAVES)


def row_grid(kernel, n_rows, num_cu=NUM_CU):
    """The grid of a one-wave-per-row kernel: pick, gain, landscape, alternatives."""
    return events_grid(cdiv(n_rows, WAVES), num_cu, PER_CU[kernel])


def taps_of(geo):
    _, _, Ay, Ax = dims(geo)
    return geo[1] * Ay * Ax


def magnitude_bound(geo):
    """The largest value a sum of a case of this geometry can take, times DENOMINATOR: at most 4 * taps terms; |w| <= 3,
    |V - R| <= 3, phi <= 4 * 3, h <= 3, so |d_e| <= 3 + 3 * 12 and a term of the gain is at most h^2 / 2 * 3 * 12 + h * 9."""
    terms = 4 * taps_of(geo)
    return DENOMINATOR * terms * max(3 * (3 + 3 * 12), 4.5 * 3 * 12 + 3 * 9)


# -- the occurrence of a shift: event_walk.h -----------------------------------------------------------------------------------
def occurrence(geo, uy, ux):
    """Occurrence -> (qy, qx): the padded positions of the images on either axis, one or two each."""
    mode = geo[5]
    _, _, Ay, Ax = dims(geo)
    Sy, Sx = shift_shape(geo)

    def axis(u, a, S):
        q0, q1, two = ed.axis_images(mode, np.array([u]), a, S)
        return [int(q0[0])] + ([int(q1[0])] if two[0] else [])
    return axis(uy, Ay, Sy), axis(ux, Ax, Sx)


def for_each_tap(geo, occ, first=0, step=1):
    """for_each_tap -> (t, c, y, x) of the taps first, first + step, ... of every image, in (iy, ix) order, inside the sample."""
    Dy, Dx, Ay, Ax = dims(geo)
    AA, taps = Ay * Ax, taps_of(geo)
    for qy in occ[0]:
        for qx in occ[1]:
            oy, ox = qy - (Ay - 1), qx - (Ax - 1)
            for t in range(first, taps, step):
                c, r = divmod(t, AA)
                jy, jx = divmod(r, Ax)
                y, x = oy + jy, ox + jx
                if 0 <= y < Dy and 0 <= x < Dx:
                    yield t, c, y, x


def phi_at(geo, occ, w, c, y, x):
    """phi_at: every image that covers the pixel, in image order; w the taps of the plane, flat."""
    _, _, Ay, Ax = dims(geo)
    phi = 0.
    for qy in occ[0]:
        ly = y - (qy - (Ay - 1))
        if not 0 <= ly < Ay:
            continue
        for qx in occ[1]:
            lx = x - (qx - (Ax - 1))
            if 0 <= lx < Ax:
                phi += w[c * Ay * Ax + ly * Ax + lx]
    return phi


def image_parts(geo, w, occ):
    """The images of the occurrence, each clipped to the sample, as dense [C, Dy, Dx] arrays."""
    Dy, Dx, Ay, Ax = dims(geo)
    w = np.asarray(w, dtype=np.float64).reshape(geo[1], Ay, Ax)
    parts = []
    for qy in occ[0]:
        for qx in occ[1]:
            oy, ox = qy - (Ay - 1), qx - (Ax - 1)
            y0, y1, x0, x1 = max(oy, 0), min(oy + Ay, Dy), max(ox, 0), min(ox + Ax, Dx)
            img = np.zeros((geo[1], Dy, Dx))
            if y0 < y1 and x0 < x1:
                img[:, y0:y1, x0:x1] = w[:, y0 - oy:y1 - oy, x0 - ox:x1 - ox]
            parts.append(img)
    return parts


def axis_whole(geo, axis, u):
    """axis_whole: the shift u on one axis is in range and its occurrence is one image wholly inside the sample."""
    mode = geo[5]
    D, A, S = dims(geo)[axis], dims(geo)[2 + axis], shift_shape(geo)[axis]
    if not 0 <= u < S:
        return False
    q0, _, two = ed.axis_images(mode, np.array([u]), A, S)
    o = int(q0[0]) - (A - 1)
    return not two[0] and o >= 0 and o + A <= D


def cells(kernel, geo):
    """The doubles of the patch a wave of the staged path would stage: events_landscape / events_alternatives, `cells`."""
    _, _, Ay, Ax = dims(geo)
    ry = 1 if len(geo[4]) == 2 else 0
    return geo[1] * (Ay + 2 * ry) * (Ax + 2) if kernel == 'landscape' else geo[1] * Ay * Ax


def patch(kernel, geo):
    """`patch`: the cells where they fit kPatchMax, else 0 -- every row walks."""
    n = cells(kernel, geo)
    return n if n <= PATCH_MAX else 0


def landscape_staged(geo, uy, ux):
    ry = 1 if len(geo[4]) == 2 else 0
    if patch('landscape', geo) <= 0:
        return False
    return (all(axis_whole(geo, 0, uy + d) for d in range(-ry, ry + 1))
            and all(axis_whole(geo, 1, ux + d) for d in (-1, 0, 1)))


def alternatives_staged(geo, uy, ux):
    if patch('alternatives', geo) <= 0:
        return False
    return axis_whole(geo, 0, uy) and axis_whole(geo, 1, ux)


def batches(n_alt):
    """The batch loop of the alternatives -> [(j0, live)]."""
    return [(j0, min(BATCH, n_alt - j0)) for j0 in range(0, n_alt, BATCH)]


def first_candidate(p, n_alt, stride):
    block = n_alt * stride
    return p // block * block + p % stride


# -- norms ---------------------------------------------------------------------------------------------------------------------
TERMS = ('N3:not-single', 'N3:oy0<0', 'N3:ox0<0', 'N3:bottom-clipped', 'N3:right-clipped')


def norms_terms(geo):
    """[5, Sy, Sx] bool: the five terms of the shortcut test of k_events_norms at every shift."""
    mode = geo[5]
    Dy, Dx, Ay, Ax = dims(geo)
    Sy, Sx = shift_shape(geo)
    qy, _, two_y = ed.axis_images(mode, np.arange(Sy), Ay, Sy)
    qx, _, two_x = ed.axis_images(mode, np.arange(Sx), Ax, Sx)
    oy0, ox0 = (qy - (Ay - 1))[:, None], (qx - (Ax - 1))[None, :]
    full = np.ones((Sy, Sx), dtype=bool)
    return np.stack([two_y[:, None] | two_x[None, :], (oy0 < 0) & full, (ox0 < 0) & full, (oy0 + Ay > Dy) & full,
                     (ox0 + Ax > Dx) & full])


def norms_shortcut(geo):
    """[Sy, Sx] bool: the shifts whose norm is the plane's sum of squares, taken once."""
    return ~norms_terms(geo).any(axis=0)


def widest_names(prefix, geo):
    mode = geo[5]
    _, _, Ay, Ax = dims(geo)
    out = set()
    for a, s in zip((Ay, Ax), shift_shape(geo)):
        if mode == 'circular' and a > 1 and a - 1 == s:
            out.add(f'{prefix}:widest-circular')
        if mode == 'reflect' and a > 1 and a - 1 == s - 1:
            out.add(f'{prefix}:widest-reflect')
        if mode == 'full' and a > 1 and s == 1:
            out.add(f'{prefix}:full-S==1')
    return out


def norms_branches(geo, num_cu=NUM_CU):
    _, C, P, _, _, _ = geo
    Sy, Sx = shift_shape(geo)
    taps, entries = taps_of(geo), Sy * Sx
    out = {'taps<256' if taps < THREADS else 'taps==256' if taps == THREADS else 'N1:second-tap-pass'}
    if taps > THREADS and taps % THREADS:
        out.add('N1:partial-last-tap-pass')
    blocks = cdiv(entries, THREADS)                                         # events_norms
    if entries < THREADS:
        out.add('entries<256')
    if entries % THREADS:
        out.add('partial-last-block')
    if blocks > events_grid(blocks, num_cu, PER_CU['norms']):
        out.add('N2:entry-loop-strides')
    terms = norms_terms(geo)
    for i, name in enumerate(TERMS):
        if np.any(terms[i] & (terms.sum(axis=0) == 1)):                     # this term true, the other four false
            out.add(name)
    if np.any(~terms.any(axis=0)):
        out.add('N3:shortcut')
    every = np.array(list(np.ndindex(Sy, Sx)), dtype=np.int64)[:, 2 - len(geo[4]):]
    if entries <= 4096:
        out |= {n for n in ed._image_branches(geo, every)[0] if n != 'image-clipped'}
        if sd.own_images_overlap(geo, every):
            out.add('N4:own-images-overlap')
    else:
        out.add('one-image')
    out |= widest_names('N4', geo)
    out.add('P==1' if P == 1 else 'P>1')
    if C > 1:
        out.add('C>1')
    return out


def norms_model(geo, W, num_cu=NUM_CU, defect=None):
    """k_events_norms, entry by entry -> b [P, Sy, Sx] (NaN where nothing is written).  ``defect``: 'first-256-taps' (the
    square-sum loop takes one pass), 'one-entry-pass' (the entry loop does not stride), 'far-side-shortcut' (the test leaves
    out the two far-side terms), 'separate-squares' (phi_at squares the images one by one)."""
    P = geo[2]
    Sy, Sx = shift_shape(geo)
    entries = Sy * Sx
    grid = events_grid(cdiv(entries, THREADS), num_cu, PER_CU['norms'])
    last = min(entries, grid * THREADS) if defect == 'one-entry-pass' else entries
    terms = norms_terms(geo).reshape(5, entries)
    if defect == 'far-side-shortcut':
        terms = terms[:3]
    walked = terms.any(axis=0)
    out = np.full((P, entries), np.nan)
    for p in range(P):
        w = np.asarray(W[p], dtype=np.float64).reshape(-1)
        whole = float(np.sum(w[:THREADS] ** 2 if defect == 'first-256-taps' else w ** 2))
        out[p, :last] = whole
        for e in np.flatnonzero(walked[:last]):
            parts = image_parts(geo, w, occurrence(geo, *divmod(int(e), Sx)))
            out[p, e] = sum(float(np.sum(q * q)) for q in parts) if defect == 'separate-squares' else float(np.sum(sum(parts) ** 2))
    return out.reshape(P, Sy, Sx)


def norms_reference(geo, W):
    """The float64 reference table b [P, Sy, Sx].  A 1-D table too long to tabulate is built from the table of the same atom
    on a sample of 4 * A pixels: its first and last 2 * A shifts at the ends, the whole-plane norm between them."""
    _, _, P, D, A, mode = geo
    S = shift_shape(geo)[2 - len(A):]
    if int(np.prod(S)) <= 4096:
        return pur.Table(W, D, mode).norms().reshape((P,) + shift_shape(geo))
    assert len(A) == 1 and D[0] > 8 * A[0]
    small = pur.Table(W, (4 * A[0],), mode).norms()
    out = np.repeat(np.sum(np.asarray(W, dtype=np.float64).reshape(P, -1) ** 2, axis=1)[:, None], S[0], axis=1)
    out[:, :2 * A[0]], out[:, -2 * A[0]:] = small[:, :2 * A[0]], small[:, -2 * A[0]:]
    return out.reshape((P,) + shift_shape(geo))


# -- score and taken -----------------------------------------------------------------------------------------------------------
ITEM = {'f32': 4, 'f64': 8}
NP = {'f32': np.float32, 'f64': np.float64}


def score_plan(dt, N, P, Sy, Sx, pad, a_off, gain_off, num_cu=NUM_CU):
    """pursuit_score_t: the view, the chunks and the steps of the walk of one call."""
    kV = 16 // ITEM[dt]
    Hs = Sx + pad
    planes = N * P
    out = dict(dt=dt, kV=kV, shape=(N, P, Sy, Sx), Hs0=Hs, entries=planes * Sy * Sx)
    rows, per_sample, brows = planes * Sy, P * Sy * Sx, P * Sy
    out['contiguous'] = Hs == Sx
    out['collapsed'] = Hs == Sx and per_sample <= 0x7fffffff and per_sample % kV == 0
    if out['collapsed']:
        rows, brows, Sx, Hs = planes // P, 1, per_sample, per_sample
    cpr = cdiv(Sx, kV)
    grid = events_grid(cdiv(rows * cpr, THREADS), num_cu, PER_CU['score'])
    stride = grid * THREADS
    row_step = stride // cpr
    out.update(rows=rows, brows=brows, Sx=Sx, Hs=Hs, cpr=cpr, grid=grid, stride=stride, row_step=row_step,
               chunk_step=stride - row_step * cpr, brow_step=row_step % brows, per_sample=per_sample,
               a_aligned=a_off * ITEM[dt] % 16 == 0, gain_aligned=gain_off * ITEM[dt] % 16 == 0)
    out['aligned'] = out['a_aligned'] and out['gain_aligned'] and Hs % kV == 0
    return out


def score_walk(plan, carry=True, limit=64):
    """k_pursuit_score, every thread at once, pass by pass -> [(row, chunk, brow, carried, wrapped)] of the chunks visited:
    arrays over the threads that are still inside the map; carried / wrapped: the step in front of the visit took the
    carry / the wrap."""
    rows, brows, cpr = plan['rows'], plan['brows'], plan['cpr']
    first = np.arange(plan['stride'], dtype=np.int64)
    row = first // cpr
    chunk, brow = first - row * cpr, row % brows
    carried = wrapped = np.zeros(len(first), dtype=bool)
    out = []
    while np.any(row < rows) and len(out) < limit:
        live = row < rows
        out.append((row[live], chunk[live], brow[live], carried[live], wrapped[live]))
        row, chunk, brow = row + plan['row_step'], chunk + plan['chunk_step'], brow + plan['brow_step']
        carried = chunk >= cpr
        if carry:
            chunk, row, brow = np.where(carried, chunk - cpr, chunk), row + carried, brow + carried
        wrapped = brow >= brows
        brow = np.where(wrapped, brow - brows, brow)
    return out


def score_expression(a, b, dt):
    """The map as numpy evaluates it: one double product and quotient, rounded once."""
    a64 = np.asarray(a, dtype=np.float64)
    with np.errstate(all='ignore'):
        return np.where((a64 > 0) & (b > 0), (a64 * a64 / (2. * b)).astype(NP[dt]), NP[dt](0)).astype(NP[dt])


def score_model(store, b, plan, sentinel, defect=None):
    """k_pursuit_score on the flat storage of the map (rows Hs apart) and the flat table -> the flat storage of the gains over
    `sentinel`.  ``defect``: 'end-chunk-whole' (the chunk that holds the end of a row is taken as a whole one),
    'no-chunk-carry' (chunk >= cpr is not carried into the row)."""
    dt, kV, Sx, Hs = plan['dt'], plan['kV'], plan['Sx'], plan['Hs']
    store, b = np.asarray(store).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    out = np.full(len(store), sentinel, dtype=NP[dt])
    for row, chunk, brow, _, _ in score_walk(plan, carry=defect != 'no-chunk-carry'):
        x0 = chunk * kV
        whole = plan['aligned'] & ((x0 + kV <= Sx) | (defect == 'end-chunk-whole'))
        for i in range(kV):
            ok = whole | (x0 + i < Sx)
            at, bt = row * Hs + x0 + i, brow * Sx + x0 + i
            ok &= (at < len(store)) & (bt < len(b))
            out[at[ok]] = score_expression(store[at[ok]], b[bt[ok]], dt)
    return out


def score_branches(plan, in_place=False):
    kV, Sx = plan['kV'], plan['Sx']
    out = set()
    if plan['aligned']:
        out.add('aligned')
    elif plan['Hs'] % kV:
        out.add('Hs-breaks-alignment')
    elif plan['gain_aligned'] and not plan['a_aligned']:
        out.add('S1:a-misaligned')
    elif plan['a_aligned'] and not plan['gain_aligned']:
        out.add('S1:gain-misaligned')
    else:
        out.add('a-and-gain-misaligned')
    if plan['collapsed']:
        out.add('collapsed-to-one-row')
    elif plan['contiguous'] and plan['per_sample'] <= 0x7fffffff:
        out.add('S2:not-collapsed-per_sample%kV')
    if plan['aligned'] and Sx >= kV:
        out.add('whole-chunk')
    if Sx % kV:
        out.add('row-end-chunk')
    if Sx < kV:
        out.add('Sx<kV')
    walk = score_walk(plan)
    if len(walk) > 1:
        out.add('S3:row_step==0' if plan['row_step'] == 0 else 'row_step>0')
    if any(p[3].any() for p in walk):
        out.add('chunk-carry')
    if any(p[4].any() for p in walk):
        out.add('brow-wraps')
    if in_place:
        out.add('in-place')
    return out


def taken_branches(plan, taken, num_cu=NUM_CU):
    taken = np.asarray(taken, dtype=np.int64)
    out = set()
    if np.any(taken < 0):
        out.add('below-range')
    if np.any(taken >= plan['entries']):
        out.add('above-range')
    inside = taken[(taken >= 0) & (taken < plan['entries'])]
    if len(np.unique(inside)) < len(inside):
        out.add('duplicate-index')
    if plan['Hs'] != plan['Sx']:
        out.add('padded-rows')
    if plan['collapsed']:
        out.add('collapsed-view')
    blocks = cdiv(len(taken), THREADS)
    if blocks > events_grid(blocks, num_cu, PER_CU['taken']):
        out.add('T1:loop-strides')
    return out


def taken_model(gain, plan, taken, num_cu=NUM_CU, defect=None):
    """k_pursuit_taken on the flat storage.  ``defect``: 'one-pass' (the loop does not stride)."""
    taken = np.asarray(taken, dtype=np.int64)
    if defect == 'one-pass':
        taken = taken[:events_grid(cdiv(len(taken), THREADS), num_cu, PER_CU['taken']) * THREADS]
    f = taken[(taken >= 0) & (taken < plan['entries'])]
    row = f // plan['Sx']
    out = np.array(gain)
    out[row * plan['Hs'] + (f - row * plan['Sx'])] = 0
    return out


# -- the one-wave-per-row kernels ----------------------------------------------------------------------------------------------
def in_range(geo, rows):
    """[K] bool: the rows inside the contract."""
    N, _, P, _, A, _ = geo
    S = shift_shape(geo)[2 - len(A):]
    rows = np.asarray(rows, dtype=np.int64)
    return ((rows[:, 0] >= 0) & (rows[:, 0] < N) & (rows[:, 1] >= 0) & (rows[:, 1] < P)
            & np.all((rows[:, 2:] >= 0) & (rows[:, 2:] < np.array(S)), axis=1))


def flat_indices(geo, rows):
    """The rows as flat C-order indices of [N, P, *S] for the pick; the rows outside the contract as indices out of range."""
    N, _, P, _, A, _ = geo
    S = shift_shape(geo)[2 - len(A):]
    rows = np.asarray(rows, dtype=np.int64)
    good = in_range(geo, rows)
    entries = N * P * int(np.prod(S))
    idx = np.empty(len(rows), dtype=np.int64)
    idx[good] = np.ravel_multi_index(tuple(rows[good].T), (N, P) + tuple(S))
    idx[~good] = np.resize(np.array([-1, entries, entries + 5, 2 ** 40, -2 ** 40], dtype=np.int64), int((~good).sum()))
    return idx


def pick_decode(geo, idx, defect=None):
    """k_pursuit_pick: the row (n, p, uy, ux) of every flat index, -1 for an index out of range.  ``defect``:
    'swapped-decode' ((np % P, np / P) in the place of (np / P, np % P))."""
    N, _, P, _, _, _ = geo
    Sy, Sx = shift_shape(geo)
    plane = Sy * Sx
    f = np.asarray(idx, dtype=np.int64)
    out = np.full((len(f), 4), -1, dtype=np.int64)
    ok = (f >= 0) & (f < N * P * plane)
    npl, u = np.divmod(f[ok], plane)
    n, p = (npl % P, npl // P) if defect == 'swapped-decode' else (npl // P, npl % P)
    out[ok] = np.stack([n, p, u // Sx, u % Sx], axis=1)
    return out


def pick_model(geo, W, V, R, idx, defect=None):
    """k_pursuit_pick through the restated walk -> (rows [K, 4], a, b, mag)."""
    N, C, P, _, _, _ = geo
    Dy, Dx, _, _ = dims(geo)
    rows = pick_decode(geo, idx, defect)
    d = (np.asarray(V, dtype=np.float64) - np.asarray(R, dtype=np.float64)).reshape(N, C, Dy, Dx)
    out = np.zeros((3, len(rows)))
    for e, (n, p, uy, ux) in enumerate(rows.tolist()):
        if n < 0 or n >= N or p >= P:
            continue
        w = np.asarray(W[p], dtype=np.float64).reshape(-1)
        occ = occurrence(geo, uy, ux)
        for t, c, y, x in for_each_tap(geo, occ):
            wd = w[t] * d[n, c, y, x]
            out[:, e] += wd, w[t] * phi_at(geo, occ, w, c, y, x), abs(wd)
    return rows, out[0], out[1], out[2]


def tap_names(prefix, taps):
    name = {1: 'one-tap', 64: 'taps-64', 65: 'taps-65'}.get(taps)
    return {f'{prefix}:{name}'} if name else set()


def _shifts2(geo, rows):
    """(uy, ux) of the rows: one shift axis as uy = 0."""
    rows = np.asarray(rows, dtype=np.int64)
    return (rows[:, 2] if rows.shape[1] == 4 else np.zeros(len(rows), dtype=np.int64)), rows[:, -1]


def _strides(kernel, n_rows, num_cu):
    return cdiv(n_rows, WAVES) > row_grid(kernel, n_rows, num_cu)


def pick_branches(geo, rows, num_cu=NUM_CU, W=None, ab=None):
    """``ab``: the reference (a, b) of the rows, for the names that depend on the values."""
    N, _, P, _, A, _ = geo
    rows = np.asarray(rows, dtype=np.int64)
    good = in_range(geo, rows)
    idx = flat_indices(geo, rows)
    entries = N * P * int(np.prod(shift_shape(geo)))
    out = set(ed._image_branches(geo, rows[good, 2:])[0]) | tap_names('K1', taps_of(geo)) | widest_names('K3', geo) | {'mag-null'}
    if taps_of(geo) > 64:
        out.add('lane-loop-strides')
    if _strides('pick', len(rows), num_cu):
        out.add('K2:event-loop-strides')
    for flag, name in ((idx < 0, 'index-below-range'), (idx >= entries, 'index-above-range'), (idx == 0, 'first-entry'),
                       (idx == entries - 1, 'last-entry')):
        if np.any(flag):
            out.add(name)
    if P & (P - 1):
        out.add('P-not-a-power-of-two')
    if ab is not None:
        a, b = ab
        if np.any(a[good] < 0):
            out.add('a<0')
        if np.any(a[good] == 0):
            out.add('a==0')
        uy, ux = _shifts2(geo, rows)
        clipped = norms_terms(geo)[1:].any(axis=0)[np.where(good, uy, 0), np.where(good, ux, 0)]
        live_plane = np.array([bool(np.any(W[p])) if g else False for p, g in zip(rows[:, 1], good)])
        if np.any(good & (b == 0) & clipped & live_plane):
            out.add('K4:b==0')
    return out


def gain_branches(geo, rows, h, num_cu=NUM_CU):
    good = in_range(geo, rows)
    out = tap_names('Q1', taps_of(geo)) | widest_names('Q2', geo) | {'mag-null'}
    if _strides('gain', len(rows), num_cu):
        out.add('event-loop-strides')
    if np.any(~good):
        out.add('row-out-of-range')
    if np.any(np.asarray(h)[good] == 0):
        out.add('h==0')
    return out


def _paths(rule, geo, rows):
    """[K] of 's' (staged), 'w' (walk), 'x' (refused), the rule evaluated once per distinct place."""
    rows = np.asarray(rows, dtype=np.int64)
    good = in_range(geo, rows)
    uy, ux = _shifts2(geo, rows)
    places, inverse = np.unique(np.stack([uy, ux], axis=1), axis=0, return_inverse=True)
    st = np.array([rule(geo, int(y), int(x)) for y, x in places], dtype=bool)[inverse.reshape(-1)]
    return np.where(good, np.where(st, 's', 'w'), 'x')


def _same_wave(paths, grid):
    """The (earlier, later) paths of consecutive passes of one wave."""
    G = grid * WAVES
    return set(zip(paths[:-G].tolist(), paths[G:].tolist())) if len(paths) > G else set()


def landscape_branches(geo, rows, num_cu=NUM_CU):
    k = len(geo[4])
    Sy, Sx = shift_shape(geo)
    rows = np.asarray(rows, dtype=np.int64)
    paths = _paths(landscape_staged, geo, rows)
    out = tap_names('L3', taps_of(geo)) | {'mag-null', 'ry==1' if k == 2 else 'ry==0'}
    out |= {n for n in widest_names('L4', geo) if n != 'L4:full-S==1'}
    if geo[5] == 'full' and Sy == 1 and Sx == 1 and np.any(paths == 'w'):
        out.add('L4:full-S==1')
    n = cells('landscape', geo)
    if np.any(paths == 's'):
        out |= {'staged', 'cells<64' if n < 64 else 'cell-loop-strides'}
        if k == 1 and geo[1] > 1:
            out.add('1d-C>1')
        if k == 2 and n == PATCH_MAX:
            out.add('L2:patch-limit-2d-fits')
    if np.any(paths == 'w'):
        out.add('walk')
        uy, ux = _shifts2(geo, rows)
        w = paths == 'w'
        if np.any(w & ((ux == 0) | (ux == Sx - 1) | ((k == 2) & ((uy == 0) | (uy == Sy - 1))))):
            out.add('neighbour-outside-the-shift-shape')
        if k == 2 and n > PATCH_MAX and any(
                p == 'w' and all(axis_whole(geo, 0, int(y) + d) and axis_whole(geo, 1, int(x) + d) for d in (-1, 0, 1))
                for p, y, x in zip(paths, uy, ux)):        # a row whose geometry stages it walks: the patch decides
            out.add('L2:patch-limit-2d-does-not-fit')
    if np.any(paths == 'x'):
        out.add('row-out-of-range')
    grid = row_grid('landscape', len(rows), num_cu)
    if _strides('landscape', len(rows), num_cu):
        out.add('event-loop-strides')
    pairs = _same_wave(paths, grid)
    for pair, name in ((('w', 's'), 'L1:staged-after-walk-in-one-wave'), (('s', 'w'), 'L1:walk-after-staged-in-one-wave'),
                       (('s', 's'), 'L1:staged-after-staged')):
        if pair in pairs:
            out.add(name)
    return out


def alternatives_branches(geo, rows, n_alt, stride, num_cu=NUM_CU):
    k = len(geo[4])
    rows = np.asarray(rows, dtype=np.int64)
    assert n_alt >= 1 and stride >= 1 and geo[2] % (n_alt * stride) == 0
    paths = _paths(alternatives_staged, geo, rows)
    good = paths != 'x'
    out = tap_names('A3', taps_of(geo)) | {'mag-null'} | {n for n in widest_names('A4', geo) if n != 'A4:full-S==1'}
    if good.any():
        out |= {f'live=={live}' for _, live in batches(n_alt)}
        if n_alt > BATCH:
            out.add('several-batches')
    n = cells('alternatives', geo)
    if np.any(paths == 's'):
        out.add('staged')
        if k == 2 and n == PATCH_MAX:
            out.add('A2:patch-limit-2d-fits')
    if np.any(paths == 'w'):
        out.add('walk')
        if k == 2 and n > PATCH_MAX and n - geo[1] * dims(geo)[2] <= PATCH_MAX:
            uy, ux = _shifts2(geo, rows)
            if any(p == 'w' and axis_whole(geo, 0, int(y)) and axis_whole(geo, 1, int(x)) for p, y, x in zip(paths, uy, ux)):
                out.add('A2:patch-limit-2d-does-not-fit')
    if np.any(~good):
        out.add('row-out-of-range')
        if n_alt > 64:
            out.add('A1:zero-fill-beyond-a-wave')
    if stride > 1:
        out.add('stride>1')
        if np.any(rows[good, 1] % stride):
            out.add('p%stride!=0')
    if np.any(rows[good, 1] // (n_alt * stride) > 0):
        out.add('second-block')
    grid = row_grid('alternatives', len(rows), num_cu)
    if _strides('alternatives', len(rows), num_cu):
        out.add('event-loop-strides')
    pairs = _same_wave(paths, grid)
    if ('w', 's') in pairs:
        out.add('staged-after-walk-in-one-wave')
    if ('s', 'w') in pairs:
        out.add('walk-after-staged-in-one-wave')
    return out


def landscape_staged_model(geo, W, V, R, row, h, defect=None):
    """The staged path of k_events_landscape for one row, through the patch -> (a, b, mag) [3^k].  ``defect``:
    'narrow-patch' (the neighbours are read with Px = Ax + 1)."""
    _, C, _, _, A, mode = geo
    Dy, Dx, Ay, Ax = dims(geo)
    ry = 1 if len(A) == 2 else 0
    n, p = int(row[0]), int(row[1])
    uy, ux = (int(row[2]), int(row[3])) if ry else (0, int(row[2]))
    w = np.asarray(W[p], dtype=np.float64).reshape(-1)
    oy = (uy - (Ay - 1) if mode == 'valid' else uy) - ry
    ox = (ux - (Ax - 1) if mode == 'valid' else ux) - 1
    Py, Px = Ay + 2 * ry, Ax + 2
    V, R = (np.asarray(x, dtype=np.float64).reshape(-1, C, Dy, Dx) for x in (V, R))
    mine = np.zeros(C * Py * Px)
    for i in range(C * Py * Px):
        c, r = divmod(i, Py * Px)
        py, px = divmod(r, Px)
        jy, jx = py - ry, px - 1
        phi = w[c * Ay * Ax + jy * Ax + jx] if 0 <= jy < Ay and 0 <= jx < Ax else 0.
        mine[i] = h * phi + (V[n, c, oy + py, ox + px] - R[n, c, oy + py, ox + px])
    nb = 9 if ry else 3
    a, m = np.zeros(nb), np.zeros(nb)
    Pw = Ax + 1 if defect == 'narrow-patch' else Px
    for t in range(C * Ay * Ax):
        c, r = divmod(t, Ay * Ax)
        jy, jx = divmod(r, Ax)
        at = c * Py * Px + (jy + ry) * Pw + (jx + 1)
        for k in range(nb):
            d = mine[at + ((k // 3 - 1) * Pw + (k % 3 - 1) if ry else k - 1)]
            a[k] += w[t] * d
            m[k] += abs(w[t] * d)
    return a, np.full(nb, float(np.sum(w * w))), m


def alternatives_model(geo, W, V, R, rows, h, n_alt, stride, slack=BATCH, defect=None):
    """The batch loop and the refusal of k_events_alternatives, row by row in row order -> (a, b, mag), each flat
    [K * n_alt + slack] over NaN.  ``defect``: 'full-last-batch' (the last batch takes live = kBatch: its surplus sums are
    stored behind the row), 'fill-one-wave' (the zero fill of a refused row stops at lane 63)."""
    _, C, P, _, _, _ = geo
    Dy, Dx, _, _ = dims(geo)
    rows = np.asarray(rows, dtype=np.int64)
    good = in_range(geo, rows)
    V, R = (np.asarray(x, dtype=np.float64).reshape(-1, C, Dy, Dx) for x in (V, R))
    out = np.full((3, len(rows) * n_alt + slack), np.nan)
    uy, ux = _shifts2(geo, rows)
    for e in range(len(rows)):
        if not good[e]:
            out[:, e * n_alt:e * n_alt + (min(n_alt, 64) if defect == 'fill-one-wave' else n_alt)] = 0.
            continue
        n, p = int(rows[e, 0]), int(rows[e, 1])
        occ = occurrence(geo, int(uy[e]), int(ux[e]))
        de = (V[n] - R[n]) + h[e] * sum(image_parts(geo, W[p], occ))
        first = first_candidate(p, n_alt, stride)
        for j0, live in batches(n_alt):
            for j in range(BATCH if defect == 'full-last-batch' else live):
                q = first + (j0 + j) * stride
                parts = image_parts(geo, W[q], occ) if q < P else [np.zeros_like(de)]
                phi = sum(parts)
                out[:, e * n_alt + j0 + j] = (float(np.sum(phi * de)), float(np.sum(phi * phi)),
                                              float(sum(np.sum(np.abs(q_ * de)) for q_ in parts)))
    return out[0], out[1], out[2]


# -- the matrix ----------------------------------------------------------------------------------------------------------------
STRIDE_ROWS = lambda cu, kernel: cu * PER_CU[kernel] * WAVES + 37      # 37 more rows than the grid has waves
EVENT_KERNELS = ('pick', 'gain', 'landscape', 'alternatives')


def _ev(geo, alt=(1, 1), kernels=EVENT_KERNELS, rows=None):
    return lambda cu: (geo, alt, kernels, rows(cu) if rows else None)


MATRIX = {
    # -- norms ---------------------------------------------------------------------------------------------------------------
    # N2: 517 + 2 more shifts than num_cu * 8 workgroups hold threads
    'norms-stride': ('norms', lambda cu: (1, 1, 1, (cu * 2048 + 517,), (3,), 'valid'),
                     {'norms': ('N2:entry-loop-strides', 'P==1')}),
    # N1: 300 taps, a second pass of 44; the shifts 0 .. 20 lie wholly inside: their norm is the sum of all 300 squares
    'norms-taps-300': ('norms', lambda cu: (1, 1, 2, (320,), (300,), 'circular'),
                       {'norms': ('N1:second-tap-pass', 'N1:partial-last-tap-pass', 'N3:shortcut')}),
    'norms-taps-256': ('norms', lambda cu: (1, 2, 2, (200,), (128,), 'valid'), {'norms': ('taps==256', 'C>1')}),
    # N3: in 'valid' each border clips alone where the other axis is inside; the seams lie inside the table
    'norms-seams': ('norms', lambda cu: (1, 2, 2, (9, 11), (3, 4), 'valid'),
                    {'norms': ('N3:oy0<0', 'N3:ox0<0', 'N3:bottom-clipped', 'N3:right-clipped', 'N3:shortcut', 'entries<256')}),
    # N3: a mirrored shift u in 1 .. a - 1 with u + a <= D has two images and its first one wholly inside
    'norms-reflect': ('norms', lambda cu: (1, 2, 2, (12, 14), (4, 4), 'reflect'),
                      {'norms': ('N3:not-single', 'one-image', 'two-images', 'four-images')}),
    # -- score and taken -----------------------------------------------------------------------------------------------------
    # S3: a contiguous map of two samples whose one row per sample holds more chunks than the grid has threads, in place
    'score-long-rows': ('score', lambda cu: (2, 2, 1, cu * 4096 + 6, 0, 0, 0, True, 7),
                        {'score': ('S3:row_step==0', 'in-place', 'collapsed-to-one-row', 'chunk-carry', 'brow-wraps')}),
    # rows padded to whole 16-byte units, 2.6 times the chunks the grid has threads (f64: 5.1 times): the carries and the wraps
    # of a view that is not collapsed
    'score-lines-stride': ('score', lambda cu: (4, 1, cu * 20, 261, 3, 0, 0, False, 7),
                           {'score': ('row_step>0', 'chunk-carry', 'brow-wraps', 'whole-chunk', 'row-end-chunk', 'aligned'),
                            'taken': ('padded-rows',)}),
    # S1: views one element into an aligned buffer; rows, row stride and the other pointer aligned
    'score-a-misaligned': ('score', lambda cu: (2, 3, 5, 64, 0, 1, 0, False, 7),
                           {'score': ('S1:a-misaligned',), 'taken': ('collapsed-view',)}),
    'score-gain-misaligned': ('score', lambda cu: (2, 3, 5, 64, 0, 0, 1, False, 7), {'score': ('S1:gain-misaligned',)}),
    # ... and the same view scored in place
    'score-view-in-place': ('score', lambda cu: (2, 3, 5, 64, 0, 1, 1, True, 7), {'score': ('a-and-gain-misaligned', 'in-place')}),
    # S2: contiguous, an odd number of entries per sample: no collapse, and the odd width breaks the alignment
    'score-odd': ('score', lambda cu: (2, 3, 5, 7, 0, 0, 0, False, 7),
                  {'score': ('S2:not-collapsed-per_sample%kV', 'Hs-breaks-alignment')}),
    'score-narrow': ('score', lambda cu: (2, 3, 5, 1, 3, 0, 0, False, 7), {'score': ('Sx<kV',)}),
    # T1: five more indices than num_cu * 8 workgroups hold threads, drawn with repeats from a small padded map; the last
    # five are met nowhere else
    'taken-stride': ('score', lambda cu: (2, 2, 3, 10, 2, 0, 0, False, cu * 2048 + 5),
                     {'taken': ('T1:loop-strides', 'below-range', 'above-range', 'duplicate-index', 'padded-rows')}),
    # -- pick, gain, landscape, alternatives ---------------------------------------------------------------------------------
    # K2: 37 more rows than num_cu * 64 workgroups have waves
    'stride-64': ('events', _ev((2, 2, 3, (12, 14), (3, 3), 'reflect'), (3, 1), ('pick', 'gain')),
                  {'pick': ('K2:event-loop-strides', 'P-not-a-power-of-two', 'first-entry', 'last-entry', 'index-below-range',
                            'index-above-range'),
                   'gain': ('event-loop-strides', 'row-out-of-range')}),
    # L1: 37 more rows than num_cu * 4 workgroups have waves; the first 37 rows and their successors in the same waves are
    # ordered (staged, walk, staged, ...) against (walk, staged, staged, ...)
    'stride-4': ('events', _ev((2, 2, 6, (12, 14), (3, 3), 'reflect'), (3, 2), ('landscape', 'alternatives')),
                 {'landscape': ('L1:staged-after-walk-in-one-wave', 'L1:walk-after-staged-in-one-wave', 'L1:staged-after-staged',
                                'event-loop-strides'),
                  'alternatives': ('staged-after-walk-in-one-wave', 'walk-after-staged-in-one-wave', 'event-loop-strides',
                                   'stride>1', 'p%stride!=0', 'live==3')}),
    # K1, Q1, L3, A3: the seams of the lane loop
    'one-tap': ('events', _ev((2, 1, 5, (9, 10), (1, 1), 'valid'), (5, 1)),
                {'pick': ('K1:one-tap',), 'gain': ('Q1:one-tap',), 'landscape': ('L3:one-tap', 'cells<64'),
                 'alternatives': ('A3:one-tap', 'live==4', 'live==1', 'several-batches')}),
    'taps-64': ('events', _ev((2, 4, 4, (10, 11), (4, 4), 'circular'), (2, 2)),
                {'pick': ('K1:taps-64',), 'gain': ('Q1:taps-64',), 'landscape': ('L3:taps-64',),
                 'alternatives': ('A3:taps-64', 'live==2')}),
    'taps-65': ('events', _ev((2, 5, 6, (40,), (13,), 'reflect'), (3, 1)),
                {'pick': ('K1:taps-65', 'lane-loop-strides'), 'gain': ('Q1:taps-65',),
                 'landscape': ('L3:taps-65', 'ry==0', '1d-C>1'), 'alternatives': ('A3:taps-65', 'second-block')}),
    # K3, Q2, L4, A4, N4: the widest geometries of the events matrix: every shift has two images in y that overlap
    'widest-circular': ('events', _ev(ed.MATRIX['widest-circular'][0](NUM_CU), (3, 1)),
                        {'pick': ('K3:widest-circular', 'two-images', 'four-images'), 'gain': ('Q2:widest-circular',),
                         'landscape': ('L4:widest-circular',), 'alternatives': ('A4:widest-circular',),
                         'norms': ('N4:widest-circular', 'N4:own-images-overlap')}),
    'widest-reflect': ('events', _ev(ed.MATRIX['widest-reflect'][0](NUM_CU), (3, 1)),
                       {'pick': ('K3:widest-reflect',), 'gain': ('Q2:widest-reflect',), 'landscape': ('L4:widest-reflect',),
                        'alternatives': ('A4:widest-reflect',), 'norms': ('N4:widest-reflect', 'N4:own-images-overlap')}),
    # 'full' with the atom as large as the sample: one shift, only the centre neighbour exists
    'full-one-shift': ('events', _ev((2, 2, 3, (6, 9), (6, 9), 'full'), (3, 1)),
                       {'landscape': ('L4:full-S==1',), 'pick': ('K3:full-S==1',), 'gain': ('Q2:full-S==1',)}),
    # ... as long as the sample on the first axis: one row of shifts
    'full-one-row': ('events', _ev((2, 2, 3, (6, 9), (6, 4), 'full'), (3, 1), ('pick', 'gain')),
                     {'pick': ('K3:full-S==1',), 'gain': ('Q2:full-S==1',), 'norms': ('N4:full-S==1',)}),
    # K4: the corner shift of plane 0 shows one tap per channel, and W holds a 0 there; plane 2 is all zero
    'zero-tap': ('events', _ev((2, 2, 3, (6, 7), (2, 3), 'valid'), (3, 1)),
                 {'pick': ('K4:b==0', 'a==0', 'a<0', 'image-clipped'), 'gain': ('h==0',),
                  'landscape': ('neighbour-outside-the-shift-shape', 'row-out-of-range', 'ry==1'),
                  'alternatives': ('row-out-of-range',)}),
    # L2: C * (Ay + 2) * (Ax + 2) = 2 * 32 * 32 = 2048 doubles, and one column more
    'landscape-limit-fits': ('events', _ev((1, 2, 1, (33, 34), (30, 30), 'valid'), (1, 1), ('landscape',)),
                             {'landscape': ('L2:patch-limit-2d-fits', 'cell-loop-strides', 'staged', 'walk')}),
    'landscape-limit-over': ('events', _ev((1, 2, 1, (33, 35), (30, 31), 'valid'), (1, 1), ('landscape',)),
                             {'landscape': ('L2:patch-limit-2d-does-not-fit',)}),
    # A2: C * Ay * Ax = 2 * 32 * 32 = 2048 doubles, and one column more
    'alternatives-limit-fits': ('events', _ev((1, 2, 2, (34, 35), (32, 32), 'valid'), (2, 1), ('alternatives',)),
                                {'alternatives': ('A2:patch-limit-2d-fits', 'staged', 'walk')}),
    'alternatives-limit-over': ('events', _ev((1, 2, 2, (34, 36), (32, 33), 'valid'), (2, 1), ('alternatives',)),
                                {'alternatives': ('A2:patch-limit-2d-does-not-fit',)}),
    # A1: a refused row of 66 candidates: the zero fill takes a second pass of two lanes
    'zero-fill': ('events', _ev((2, 1, 66, (6, 7), (2, 2), 'valid'), (66, 1), ('alternatives',)),
                  {'alternatives': ('A1:zero-fill-beyond-a-wave',)}),
}
# the norms of the events cases that stand for an item of the norms
NORMS_OF_EVENTS = ('widest-circular', 'widest-reflect', 'full-one-row')

# the items more than one case reaches: every case that does (the CPU test holds this list to the mirror).  Each clipping term
# of N3 is alone wherever the other axis lies inside, so every table with a border has some; 'norms-seams' is the case that
# has all four and the seams inside one small table.
ALSO = {
    ('norms', 'N3:not-single'): ('norms-reflect', 'widest-reflect'),
    ('norms', 'N3:ox0<0'): ('norms-stride', 'norms-taps-256', 'norms-seams'),
    ('norms', 'N3:bottom-clipped'): ('norms-seams', 'norms-reflect'),
    ('norms', 'N3:right-clipped'): ('norms-stride', 'norms-taps-256', 'norms-seams', 'norms-reflect', 'widest-reflect'),
    ('norms', 'N3:shortcut'): ('norms-stride', 'norms-taps-300', 'norms-taps-256', 'norms-seams', 'norms-reflect', 'widest-reflect',
                               'full-one-row'),
    ('norms', 'N4:own-images-overlap'): ('norms-reflect', 'widest-circular', 'widest-reflect'),
    ('pick', 'K3:full-S==1'): ('full-one-shift', 'full-one-row'),
    ('gain', 'Q2:full-S==1'): ('full-one-shift', 'full-one-row'),
}


def kind_of(name):
    return MATRIX[name][0]


def spec_of(name, num_cu=NUM_CU):
    return MATRIX[name][1](num_cu)


def names_of(kind):
    return [n for n in MATRIX if MATRIX[n][0] == kind]


def norms_names():
    return names_of('norms') + list(NORMS_OF_EVENTS)


def norms_geometry(name, num_cu=NUM_CU):
    spec = spec_of(name, num_cu)
    return spec if kind_of(name) == 'norms' else spec[0]


def _integers(name, shape, what):
    rng = np.random.default_rng(zlib.crc32(f'scoring {name} {what}'.encode()))
    return rng.integers(0, 4, shape).astype(np.float64)


_W = {}


def dictionary(name, num_cu=NUM_CU):
    """W [P, C, *A]: integers in 0..3 (the same whatever the CU count), with the zero taps the case needs."""
    if name not in _W:
        _, C, P, _, A, _ = norms_geometry(name, num_cu)
        W = _integers(name, (P, C) + tuple(A), 'W')
        if name == 'zero-tap':
            W[(0, slice(None)) + (-1,) * len(A)] = 0.       # the tap the first corner of 'valid' shows
            W[2] = 0.                                        # an all-zero plane
        if name.startswith('norms-seams'):
            W[:, :, -1, :], W[:, :, :, -1] = np.maximum(W[:, :, -1, :], 1.), np.maximum(W[:, :, :, -1], 1.)   # (clipped taps count)
        W.setflags(write=False)
        _W[name] = W
    return _W[name]


_CASES = {}


def score_case(name, dt, num_cu=NUM_CU, data=True):
    """-> dict(plan, in_place, taken, and with ``data`` a [N, P, Sy, Sx] in the element type with negative values, zeros, NaN and
    +inf, b [P, Sy, Sx] with zeros, want [N, P, Sy, Sx]: the numpy expression with the taken entries zeroed)."""
    key = (name, dt, num_cu, data)
    if key in _CASES:
        return _CASES[key]
    N, P, Sy, Sx, pad, a_off, gain_off, in_place, n_taken = spec_of(name, num_cu)
    plan = score_plan(dt, N, P, Sy, Sx, pad, a_off, gain_off, num_cu)
    rng = np.random.default_rng(zlib.crc32(f'scoring {name}'.encode()))
    size = N * P * Sy * Sx
    if n_taken <= 7:
        taken = np.array([-1, 0, size - 1, size, 2 ** 40, 7 % size, size // 2], dtype=np.int64)[:n_taken]
    else:       # the first half of the map with repeats and indices out of range, then five entries of the second half
        taken = rng.integers(0, size // 2, n_taken).astype(np.int64)
        taken[[3, 11, n_taken - 9]], taken[[5, 13, n_taken - 8]] = (-1, -2 ** 40, -7), (size, 2 ** 40, size + 3)
        taken[-5:] = size // 2 + 3 + 2 * np.arange(5)
    out = dict(plan=plan, in_place=in_place, taken=taken, a_off=a_off, gain_off=gain_off)
    if data:
        a = (rng.standard_normal((N, P, Sy, Sx)) * 3.).astype(NP[dt])
        flat = a.reshape(-1)
        flat[rng.integers(size, size=max(2, size // 9))] = 0.
        flat[rng.integers(size, size=max(2, size // 17))] = np.nan
        flat[rng.integers(size, size=max(2, size // 19))] = np.inf
        a[0, 0, 0, 0], a[N - 1, P - 1, Sy - 1, Sx - 1] = 2.5, 1.25
        if n_taken > 7:
            flat[taken[-5:]] = 1.5 + np.arange(5)
        b = rng.random((P, Sy, Sx)) + 0.01
        b.reshape(-1)[rng.integers(b.size, size=max(2, b.size // 11))] = 0.
        b[0, 0, 0], b[P - 1, Sy - 1, Sx - 1] = 0.75, 0.5
        if n_taken > 7:
            b.reshape(-1)[taken[-5:] % b.size] = 0.5
        want = score_expression(a, b, dt)
        untaken = want.copy()
        want.reshape(-1)[taken[(taken >= 0) & (taken < size)]] = 0
        for x in (a, b, want, untaken):
            x.setflags(write=False)
        out.update(a=a, b=b, want=want, untaken=untaken)
    _CASES[key] = out
    return out


def _places(geo):
    """name -> shift: landscape_reference.places() without its zones, every place clamped into the shift shape (the widest
    geometries have an atom longer than the sample)."""
    _, _, _, D, A, mode = geo
    k = len(A)
    S = shift_shape(geo)[2 - k:]
    first = [a - 1 if mode == 'valid' else 0 for a in A]        # the shift whose occurrence starts at pixel 0
    out = {'interior': tuple(f + (d - a) // 2 for f, d, a in zip(first, D, A)), 'near': tuple(f + 1 for f in first),
           'edge': tuple(first), 'far': tuple(f + d - a - 1 for f, d, a in zip(first, D, A))}
    for i, corner in enumerate(np.ndindex(*(2,) * k)):
        out[f'corner{i}'] = tuple(c * (s - 1) for c, s in zip(corner, S))
    for i in range(k):
        for name, x in (('rim-lo', 0), ('rim-hi', S[i] - 1)):
            out[f'{name}{i}'] = tuple(x if j == i else S[j] // 2 for j in range(k))
    if mode in ('reflect', 'circular'):                          # the zones of two images on every axis, and beside them
        out['zone'] = tuple(1 if mode == 'reflect' else s - 1 for s in S)
        out['zone-one-axis'] = tuple((1 if mode == 'reflect' else S[j] - 1) if j == k - 1 else S[j] // 2 for j in range(k))
        out['beside-zone'] = tuple(a if mode == 'reflect' else s - a for s, a in zip(S, A))
    return {n: tuple(int(min(max(x, 0), s - 1)) for x, s in zip(u, S)) for n, u in out.items()}


def _pool(name, geo, rng):
    """The distinct places of an events case with their strengths: (rows [M, 2 + k], h [M]); rows outside the contract among
    them.  The first two are a place every path rule stages and one every rule walks, where the geometry has both."""
    N, C, P, D, A, mode = geo
    k = len(A)
    S = shift_shape(geo)[2 - k:]
    at = _places(geo)
    special = [(0, P - 1) + at['interior']]
    walks = [u for n, u in at.items() if not alternatives_staged(geo, *((0,) * (2 - k) + u))]
    special.append((N - 1, min(1, P - 1)) + (walks[0] if walks else at['corner0']))
    special += [(i % N, (3 * i + 1) % P) + u for i, u in enumerate(at.values())]
    special += [(0, 0) + (0,) * k, (N - 1, P - 1) + tuple(s - 1 for s in S)]          # the first and the last entry
    count = {'stride-64': 250, 'stride-4': 90, 'landscape-limit-fits': 0, 'landscape-limit-over': 0,
             'alternatives-limit-fits': 0, 'alternatives-limit-over': 0, 'zero-fill': 6}.get(name, 40)
    if name.endswith(('-fits', '-over')):
        keep = ('interior', 'near', 'edge', 'far', 'corner0', f'corner{2 ** k - 1}', 'rim-lo0', 'rim-hi1')
        special = [(0, i % P) + at[n] for i, n in enumerate(keep)]
    if name == 'zero-tap':
        special += [(0, 0, 0, 0), (1, 0, 0, 0), (0, 2, 3, 3), (1, 2, 0, 0), (0, 1, 0, 0)]
    if name.startswith('widest'):
        special += [(1, 1) + u for u in np.ndindex(*S)]                                # every shift of one plane of one sample
    space = (N, P) + tuple(S)
    drawn = ed._draw(rng, space, min(count, int(np.prod(space)))).tolist() if count else []
    rows = list(dict.fromkeys([tuple(r) for r in special] + [tuple(r) for r in drawn]))
    bad = [[N, 0] + [0] * k, [-1, 0] + [0] * k, [0, P] + [0] * k, [0, -2] + [0] * k, [N - 1, P - 1] + [S[0]] + [0] * (k - 1),
           [N - 1, P - 1] + [0] * (k - 1) + [-1]]
    rows = np.array(rows + bad, dtype=np.int64)
    h = rng.integers(0, 7, len(rows)) / 2.
    h[:2] = 1.5, 2.5
    h[3] = 0.
    return rows, h


def events_case(name, num_cu=NUM_CU):
    """-> dict(geo, n_alt, stride, kernels, rows [K, 2 + k], h [K], W, V, R, good [K], pool_rows, pool_h, pick [K]): rows =
    pool_rows[pick].  W, V, R and the pool do not depend on the CU count; the length and the order of the list do."""
    if (name, num_cu) in _CASES:
        return _CASES[name, num_cu]
    geo, (n_alt, stride), kernels, _ = spec_of(name, num_cu)
    N, C, P, D, A, mode = geo
    rng = np.random.default_rng(zlib.crc32(f'scoring {name} rows'.encode()))
    pool_rows, pool_h = _pool(name, geo, rng)
    M = len(pool_rows)
    if name in ('stride-64', 'stride-4'):
        K = STRIDE_ROWS(num_cu, kernels[0])
        assert K >= M
        pick = np.concatenate([np.arange(M), rng.integers(0, M, K - M)])
        pick = pick[rng.permutation(K)]
        if name == 'stride-4':      # the waves that take a second row: (staged, walk, staged)[e % 3] then (walk, staged, staged)
            G = row_grid('landscape', K, num_cu) * WAVES
            assert K - G == 37
            e = np.arange(37)
            pick[:37], pick[G:] = np.array([0, 1, 0])[e % 3], np.array([1, 0, 0])[e % 3]
    else:
        pick = rng.permutation(M)
    last = np.flatnonzero(in_range(geo, pool_rows[pick]))[-1]      # a row inside the contract comes last: what it stores
    pick[[last, -1]] = pick[[-1, last]]                            # behind itself lands behind the outputs
    V, R = _integers(name, (N, C) + tuple(D), 'V'), _integers(name, (N, C) + tuple(D), 'R')
    out = dict(geo=geo, n_alt=n_alt, stride=stride, kernels=kernels, rows=pool_rows[pick], h=pool_h[pick],
               W=dictionary(name, num_cu), V=V, R=R, good=in_range(geo, pool_rows[pick]), pool_rows=pool_rows, pool_h=pool_h,
               pick=pick)
    for x in out.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    _CASES[name, num_cu] = out
    return out


_REFERENCES = {}


def events_reference(name, kernel):
    """The float64 reference of the POOL of the case, computed once (it does not depend on the CU count) -> for 'pick'
    (a, b, mag), for 'gain' (gain, mag), for 'landscape' and 'alternatives' (a, b, mag) [M, 3^k] / [M, n_alt]; zeros for the
    rows outside the contract.  Index it with the case's ``pick``."""
    if (name, kernel) not in _REFERENCES:
        c = events_case(name)
        geo, rows, h, W, V, R = c['geo'], c['pool_rows'], c['pool_h'], c['W'], c['V'], c['R']
        good = in_range(geo, rows)
        sample, plane, shift = rows[:, 0], rows[:, 1], rows[:, 2:]
        if kernel == 'pick':
            out = np.zeros((3, len(rows)))
            out[:, good] = pur.exact(V, R, W, geo[5], rows[good])
            out = tuple(out)
        elif kernel == 'gain':
            out = gref.closed_form(V, R, W, geo[5], sample, plane, shift, h)
        elif kernel == 'landscape':
            out = lref.landscape(V, R, W, geo[5], sample, plane, shift, h)
        else:
            out = aref.alternatives(V, R, W, geo[5], sample, plane, shift, h, c['n_alt'], c['stride'])
        out = tuple(np.asarray(x) + 0. for x in out)          # (a sum of exact zeros may carry a sign in numpy: +0 here)
        for x in out:
            x.setflags(write=False)
        _REFERENCES[name, kernel] = out
    return _REFERENCES[name, kernel]


def pick_outputs(a, b, dt):
    """(strength in the element type, gain) of the pick from the exact sums, as numpy evaluates them in float64."""
    live = (a > 0) & (b > 0)
    safe = np.where(live, b, 1.)
    return np.where(live, (a / safe).astype(NP[dt]), NP[dt](0)).astype(NP[dt]), np.where(live, a * a / (2. * safe), 0.)


def reached(name, num_cu=NUM_CU, dt='f32'):
    """{kernel: the names of BRANCHES[kernel] the case executes at this CU count} (a score case: in this element type)."""
    kind = kind_of(name)
    out = {}
    if kind == 'norms' or name in NORMS_OF_EVENTS:
        out['norms'] = norms_branches(norms_geometry(name, num_cu), num_cu)
    if kind == 'score':
        c = score_case(name, dt, num_cu, data=False)
        out['score'] = score_branches(c['plan'], c['in_place'])
        out['taken'] = taken_branches(c['plan'], c['taken'], num_cu)
    if kind == 'events':
        c = events_case(name, num_cu)
        geo, rows = c['geo'], c['rows']
        assert magnitude_bound(geo) < 2 ** 53
        if 'pick' in c['kernels']:
            a, b, _ = events_reference(name, 'pick')
            out['pick'] = pick_branches(geo, rows, num_cu, c['W'], (a[c['pick']], b[c['pick']]))
        if 'gain' in c['kernels']:
            out['gain'] = gain_branches(geo, rows, c['h'], num_cu)
        if 'landscape' in c['kernels']:
            out['landscape'] = landscape_branches(geo, rows, num_cu)
        if 'alternatives' in c['kernels']:
            out['alternatives'] = alternatives_branches(geo, rows, c['n_alt'], c['stride'], num_cu)
    for kernel, got in out.items():
        assert got <= set(BRANCHES[kernel]), (kernel, got - set(BRANCHES[kernel]))
    return out
