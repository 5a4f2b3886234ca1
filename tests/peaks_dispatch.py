"""
Host mirror of the launch and the control flow of k_find_peaks in its plain form, the one the product runs
(tnmf_amd/csrc/peaks.hip: launch(), k_find_peaks<T, false>, examine(), floor_to(); the geometry of api.hip
tnmf_hip_find_peaks) -- restated in plain Python, so that the tests can choose small inputs that execute every branch of it
(tests/test_hip_peaks_matrix.py) and a CPU test can check that the choice covers them all
(tests/test_peaks_dispatch_cpu.py).  "Every branch" means: both grid loops stride, each of the two thinning tests is live
with and without the other, the window walk takes every shape it has (lanes along x only, several window rows per slab,
several steps along x, several batches of slabs), and the threshold is rounded down on the way to float32 -- the names of
BRANCHES below.  The tiled form (-DTNMF_PEAKS_TILED, examine_tile) is an A/B flavour outside the product build and is
not mirrored.

An input is H[N, P, *S] with one, two or three shift axes; `radius` has one entry per shift axis.
"""
from collections import namedtuple

import numpy as np

NUM_CU = 256          # compute units of one MI355X (what launch() reads from ctx->num_cu there)

WAVES = 4             # peaks.hip:29, kWaves
ROWS_PER_WAVE = 4     # peaks.hip:30, kRowsPerWave
BLOCK_ROWS = WAVES * ROWS_PER_WAVE   # peaks.hip:31, kBlockRows
SLAB_BATCH = 4        # peaks.hip:32, kSlabBatch
GX_CAP = 1024         # peaks.hip:265
GY_CAP = 65535        # peaks.hip:267

BRANCHES = (
    'one-shift-axis-folded',          # :260-263 the planes of a signal become the rows of one plane
    'two-shift-axes', 'three-shift-axes',
    'row-padded',                     # Hs > Sx
    'group>1',                        # :108-109, :157
    'P1:plane-loop-strides',          # :154 more planes than gridDim.y
    'P1:plane-loop-strides-in-a-group',   # :157 ... with group > 1: qc of a plane the workgroup did not start on
    'P1:qc-changes-across-the-stride',    # :157 ... and that plane has another place in its group than the first
    'P2:row-block-loop-strides',      # :158 more than 1024 blocks of 16 rows
    'several-column-tiles',           # :160 Sx > 64
    'no-thinning', 'both-thinnings',  # :193, :197
    'P3:vertical-thinning-only',      # :197 alone: rx == 0, a window one entry wide (lw == 0, 64 window rows per slab)
    'P3:horizontal-thinning-only',    # :193 alone, with two shift axes: ry == 0
    'P4:window-of-3',                 # :248-249 rx == 1: lw == 2
    'P4:window-of-2',                 # :247 Sx == 2: lw == 1
    'several-window-rows-per-slab',   # :94 rpi > 1
    'several-slab-batches',           # :114 n_rows > kSlabBatch * rpi
    'wide-1d-window',                 # :112 the xs loop steps, one shift axis
    'P5:wide-2d-window',              # :112 ... with two shift axes: rpi == 1 and several window rows
    'P6:threshold-rounded-down',      # :239 (float)t > t: floor_to<float> steps to the predecessor
    'threshold-exact',                # :239 not taken
)

Launch = namedtuple('Launch', 'lw rpi xs_steps j0_batches gx gy fold plane_loop_strides row_loop_strides '
                              'thin_x thin_y planes rpp width n_rows qc_changes')


def cdiv(a, b):
    return -(-a // b)


def launch(shape, radius, group=1, stride=None, num_cu=NUM_CU):
    """What launch() (peaks.hip:243-274) does with H of `shape` = (N, P, *S), rows `stride` entries apart:

      lw, rpi       log2 of the lanes along x in a slab, window rows per slab (:246-249, :94)
      xs_steps, j0_batches   steps of the xs loop and batches of the j0 loop over a full (unclipped) window (:112, :114)
      gx, gy, fold  the grid, and whether one shift axis was folded into the rows of one plane (:260-267)
      plane_loop_strides, row_loop_strides   whether `plane += gridDim.y` / `rb += gridDim.x * kBlockRows` are taken
      thin_x, thin_y   which of the two thinning tests are live (:193, :197)
      qc_changes    group > 1 and a workgroup meets a plane whose place in its group is not that of its first plane"""
    N, P, S = shape[0], shape[1], tuple(shape[2:])
    assert 1 <= len(S) <= 3 and len(radius) == len(S) and group >= 1 and P % group == 0
    Sz, Sy, Sx = (1,) * (3 - len(S)) + S                                      # api.hip tnmf_hip_find_peaks: S[k], r[k]
    rz, ry, rx = [min(r, s - 1) for r, s in zip((0,) * (3 - len(S)) + tuple(radius), (Sz, Sy, Sx))]
    assert stride is None or stride >= Sx
    width = min(2 * rx + 1, Sx)                                                # :247
    lw = 0
    while lw < 6 and (1 << lw) < width:                                        # :248-249
        lw += 1
    wpad, rpi = 1 << lw, 64 >> lw                                              # :94
    planes = N * P
    n_rows = min(2 * ry + 1, Sy)                                               # :98 of a candidate away from the edges
    fold = Sz == 1 and Sy == 1 and group == 1 and planes <= 0x7fffffff         # :260
    if fold:
        Sy, planes = planes, 1                                                 # :261-262
    rpp = Sz * Sy                                                              # :264
    gx = min(cdiv(rpp, BLOCK_ROWS), GX_CAP)                                    # :265
    budget = max(1, num_cu * 64 // gx)                                         # :266
    gy = max(1, min(planes, budget, GY_CAP))                                   # :267
    plane_loop_strides = planes > gy                                           # :154
    qc_changes = plane_loop_strides and group > 1 and (gy % P) % group != 0   # :157
    return Launch(lw=lw, rpi=rpi, xs_steps=cdiv(width, wpad), j0_batches=cdiv(n_rows, SLAB_BATCH * rpi), gx=gx, gy=gy,
                  fold=fold, plane_loop_strides=plane_loop_strides, row_loop_strides=cdiv(rpp, BLOCK_ROWS) > gx,
                  thin_x=rx >= 1, thin_y=ry >= 1 and Sz == 1, planes=planes, rpp=rpp, width=width, n_rows=n_rows,
                  qc_changes=qc_changes)


def threshold_rounds_down(threshold, dtype):
    """peaks.hip:237-241, floor_to<float>: whether the nextafterf branch is taken."""
    return dtype in (0, 'f32') and float(np.float32(threshold)) > float(threshold)


def reached(shape, radius, group=1, stride=None, threshold=0., dtype=0, num_cu=NUM_CU):
    """The names of BRANCHES one call executes."""
    k = len(shape) - 2
    c = launch(shape, radius, group, stride, num_cu)
    out = {'one-shift-axis-folded' if c.fold else 'two-shift-axes' if k <= 2 else 'three-shift-axes'}
    out.add('P6:threshold-rounded-down' if threshold_rounds_down(threshold, dtype) else 'threshold-exact')
    if stride is not None and stride > shape[-1]:
        out.add('row-padded')
    if group > 1:
        out.add('group>1')
    if c.plane_loop_strides:
        out.add('P1:plane-loop-strides')
        if group > 1:
            out.add('P1:plane-loop-strides-in-a-group')
        if c.qc_changes:
            out.add('P1:qc-changes-across-the-stride')
    if c.row_loop_strides:
        out.add('P2:row-block-loop-strides')
    if shape[-1] > 64:
        out.add('several-column-tiles')
    if c.thin_x and c.thin_y:
        out.add('both-thinnings')
    elif c.thin_y:
        assert c.lw == 0 and c.rpi == 64 and c.width == 1
        out.add('P3:vertical-thinning-only')
    elif c.thin_x and k == 2:
        out.add('P3:horizontal-thinning-only')
    elif not c.thin_x:
        out.add('no-thinning')
    if c.width == 3:
        assert c.lw == 2
        out.add('P4:window-of-3')
    if c.width == 2:
        assert c.lw == 1
        out.add('P4:window-of-2')
    if c.rpi > 1 and c.n_rows > 1:
        out.add('several-window-rows-per-slab')
    if c.j0_batches > 1:
        out.add('several-slab-batches')
    if c.xs_steps > 1:
        assert c.rpi == 1
        out.add('P5:wide-2d-window' if k >= 2 and c.n_rows > 1 else 'wide-1d-window')
    assert out <= set(BRANCHES), out - set(BRANCHES)
    return out


NEW = tuple(b for b in BRANCHES if b[0] == 'P' and b[1].isdigit())


def plane_stride_samples(num_cu=NUM_CU):
    """The fewest samples of 240 planes that are more planes than launch() gives workgroups (one block of rows each)."""
    return num_cu * 64 // 240 + 1


# The calls of tests/test_hip_peaks_matrix.py on tie_rich inputs: name -> (shape as a function of the CU count, seed,
# row stride, threshold, radius, group, the items of the issue the call is there for).  Counts quoted for 256 CUs.
MATRIX = {
    # P1: 16 560 planes of 5 rows on 16 384 workgroups; in groups of four the stride of 16 384 planes keeps every plane's
    # place in its group (16 384 % 240 = 64), in groups of three it does not
    'plane-stride': (lambda cu: (plane_stride_samples(cu), 240, 5, 9), 11, None, 0., (1, 1), 1, ('P1:plane-loop-strides',)),
    'plane-stride-group-4': (lambda cu: (plane_stride_samples(cu), 240, 5, 9), 11, None, 0., (1, 1), 4,
                             ('P1:plane-loop-strides-in-a-group',)),
    'plane-stride-group-3': (lambda cu: (plane_stride_samples(cu), 240, 5, 9), 11, None, 0., (1, 1), 3,
                             ('P1:plane-loop-strides-in-a-group', 'P1:qc-changes-across-the-stride')),
    # P2: 16 896 signals folded into the rows of one plane: 1056 blocks of 16 rows on 1024 workgroups
    'row-stride': (lambda cu: (132, 128, 20), 12, None, 0., (2,), 1, ('P2:row-block-loop-strides',)),
    # P3: one thinning test without the other
    'vertical-only': (lambda cu: (2, 3, 40, 150), 13, None, 0., (4, 0), 1, ('P3:vertical-thinning-only',)),
    'horizontal-only': (lambda cu: (2, 3, 40, 150), 13, None, 0., (0, 4), 1, ('P3:horizontal-thinning-only',)),
    # P4: windows three and two entries wide
    'narrow-3': (lambda cu: (2, 3, 33, 70), 14, None, 0., (2, 1), 1, ('P4:window-of-3',)),
    'narrow-2': (lambda cu: (2, 3, 33, 2), 15, None, 0., (1, 1), 1, ('P4:window-of-2',)),
    # P5: a window of 3 x 81 entries: two steps along x, one window row per slab
    'wide-2d': (lambda cu: (2, 4, 20, 200), 16, 256, 0., (1, 40), 2, ('P5:wide-2d-window',)),
}

# threshold-ulp (P6) and nan-inf (P7) are inputs of their own: tests/test_hip_peaks_matrix.py builds them
ULP_SHAPE, ULP_THRESHOLD = (2, 3, 21, 70), 0.1
NAN_INF_SHAPE, NAN_INF_CALLS = (2, 3, 33, 70), (((2, 3), 1), ((1, 40), 3), ((0, 0), 1))


def call_of(name, num_cu=NUM_CU):
    """-> (shape, seed, stride, threshold, radius, group) of a call of the matrix on this CU count."""
    shape, seed, stride, threshold, radius, group, _ = MATRIX[name]
    return shape(num_cu), seed, stride, threshold, radius, group
