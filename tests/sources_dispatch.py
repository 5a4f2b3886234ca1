"""
Host mirror of the launch of tnmf_amd/csrc/sources.hip (k_source_wsum, k_atom_sources) and of the tables that
tnmf_hip_atom_sources completes (tnmf_amd/csrc/api.hip), restated in plain Python and numpy in the manner of
tests/scoring_dispatch.py, so that tests/test_hip_sources_matrix.py can choose the smallest problems that execute every
branch of the two kernels and tests/test_sources_dispatch_cpu.py can check without a GPU that the choice covers them.

The walk itself is that of tests/atoms_dispatch.py (``plan``); what sources.hip adds to it is restated here: whether a
thread's four pixels move as one aligned 16-byte unit (``vec``), the channel instance and the channels of each chunk, the
register stage, the grid of the channel sums, the layout of the work buffer and the completed tables.

What is planted in the operands (``operands``, ``integer_operands``), so that pixels of every kind exist:
  * every layout with unlisted planes, sample 1, the pixels of ``hidden_block``: the listed planes of Hp are zero over the
    windows of those pixels and the first unlisted plane is positive there -- only the hidden group explains them: label 0
    (not -1), share 0, every mask 0, total > 0;
  * layout 'hidden-heavy': the unlisted planes of Hp times 8 -- a hidden group of several planes that outweighs the source;
  * random operands, sample 0, the last two pixels of every row: every plane of Hp is zero over their windows -- nobody
    explains them: label -1, share 0, every mask 0 with eps = 0 as well;
  * integer operands: planes 0 and 1 alike (a tie that the lowest index wins under 'each') and, in sample 0, the first
    columns of every plane zero (the construction of tests/test_hip_sources.py).

The wrong models at the end are the reference with one defect each, in plain numpy: tests/test_sources_dispatch_cpu.py
asserts that each differs from the right answer on the case named for it by more than 100 times the bound the GPU test
applies there -- the proof that the case could catch it.
"""
import functools

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import sources_reference as sref
from atoms_dispatch import CHANNELS, LDS_LIMIT, PIX, STAGE, THREADS, cdiv, plan

NUM_CU = 256                       # compute units of one MI355X (ctx->num_cu there)
WSUM_PER_CU = 8                    # launch_atom_sources: the grid of k_source_wsum is at most num_cu * 8 workgroups
EMIT = {'contribution': 0, 'mask': 1, 'masked': 2, 'dominant': 3}   # include/tnmf_hip.h, TNMF_SOURCES_*
ESIZE = {'f32': 4, 'f64': 8}
NP = {'f32': np.float32, 'f64': np.float64}
U = {'f32': 2. ** -24, 'f64': 2. ** -53}
DTYPES = ('f32', 'f64')
EPS = 1e-9
LAYOUTS = ('each', 'interleaved', 'all', 'scattered', 'hidden-heavy')
DEVICE_LIMIT = 64 << 20            # bytes a case may allocate on the device

# what the matrix does not execute, and why
NOT_REACHED = (
    'not-reached: N * slots > 2^31',          # atom_terms_check refuses it: 2^31 workgroups, no output of that size fits
    'not-reached: out beyond 2^31 elements',  # `at` is size_t throughout; 8 GB of output for one test
)

BRANCHES = (
    # stores and loads: put / get of k_atom_sources
    'vec', 'pixelwise:Dx%4', 'pixelwise:out-misaligned', 'pixelwise:V-misaligned',
    'vec:thread-outside-x',        # xb >= g.Dx under vec: the guard inside put and get is false
    'vec:row-outside-y',           # y >= g.Dy under vec: row_in is false
    'vec:several-tiles', 'vec:1d',
    'vec:stage-loop',              # pre_ok == false
    'vec:below-halo',              # D < A - 1 on an axis
    # instances
    'CH1:f32', 'CH2:f32', 'CH3:f32', 'CH4:full:f32', 'CH4:short-second-chunk:f32', 'DOM:f32',
    'CH1:f64', 'CH2:f64', 'CH3:f64', 'CH4:full:f64', 'CH4:short-second-chunk:f64', 'DOM:f64',
    # groups
    'hidden:empty', 'hidden:one-plane', 'hidden:several-and-largest',
    'pixel:only-hidden-explains', 'pixel:nobody-explains',
    'source:planes-descending-and-scattered', 'S==1', 'S==1:rest-hidden', 'S==M',
    'tie:lowest-index-wins',
    # emit
    'emit:contribution', 'emit:mask', 'emit:masked', 'emit:dominant', 'eps==0', 'eps~total',
    # k_source_wsum
    'wsum:one-block', 'wsum:partial-last-block', 'wsum:grid-stride', 'wsum:C==1',
) + NOT_REACHED


# -- the launch rules ----------------------------------------------------------------------------------------------------------
def dims(D, A):
    Dy, Dx = (1, D[0]) if len(D) == 1 else D
    Ay, Ax = (1, A[0]) if len(A) == 1 else A
    return Dy, Dx, Ay, Ax


def vec(Dx, out_offset, V_offset, esize):
    """launch_atom_sources, `vec`: ``out_offset`` / ``V_offset`` are the elements by which the pointers lie behind a
    boundary of kAtomPix elements."""
    unit = PIX * esize
    return Dx % PIX == 0 and out_offset * esize % unit == 0 and V_offset * esize % unit == 0


def instance(C, emit):
    """-> (CH, DOM) of the k_atom_sources instance; the dominant source walks one channel, the channel sums."""
    return (1, True) if emit == 'dominant' else (min(C, CHANNELS), False)


def chunk_channels(C):
    """nc of every chunk: g.C - c0 < CH ? g.C - c0 : CH."""
    CH = min(C, CHANNELS)
    return [min(CH, C - c0) for c0 in range(0, C, CH)]


def pre_ok(C, D, A):
    p = plan(C, D, A)
    return p['SH'] * p['SW'] <= STAGE * THREADS


def wsum_grid(M, A, num_cu=NUM_CU):
    """-> (n_sum, blocks of one pass over it, grid)."""
    n_sum = M * int(np.prod(A))
    return n_sum, cdiv(n_sum, THREADS), min(cdiv(n_sum, THREADS), num_cu * WSUM_PER_CU)


def align_up(x, a):
    return cdiv(x, a) * a


def taps_bytes(C, M, D, A, dt):
    """atom_terms_taps_bytes."""
    return align_up(M * C * dims(D, A)[2] * 2 * plan(C, D, A)['NBO'] * PIX * ESIZE[dt], 256)


def work(C, M, D, A, dt, S, emit):
    """atom_sources_work: dict(taps_off, wsum_off, order_off, start_off, total).  The taps are sized for all C channels,
    for 'dominant' as well."""
    w = dict(taps_off=0, wsum_off=taps_bytes(C, M, D, A, dt))
    wsum = M * int(np.prod(A)) * ESIZE[dt] if emit == 'dominant' else 0
    w['order_off'] = w['wsum_off'] + align_up(wsum, 256)
    w['start_off'] = w['order_off'] + align_up(M * 4, 256)
    w['total'] = w['start_off'] + align_up((S + 2) * 4, 256)
    return w


def tables(sets, M):
    """The two tables as tnmf_hip_atom_sources completes them -> (order [M], start [S + 2]): the listed planes first, the
    unlisted ascending, start[S + 1] = M."""
    order = [m for s in sets for m in s]
    assert len(set(order)) == len(order) and all(0 <= m < M for m in order) and all(len(s) for s in sets)
    start = list(np.cumsum([0] + [len(s) for s in sets]))
    order += [m for m in range(M) if m not in set(order)]
    return np.array(order, dtype=np.int32), np.array(start + [M], dtype=np.int32)


def plane_sets(M, layout):
    """The layouts of tests/test_hip_sources.py -- every plane on its own; the even and the odd planes with the last plane
    unlisted; one source of all planes, from the last to the first -- and two more: the planes (M - 1, 2) and (0), the
    rest hidden; plane 0 alone, the rest hidden."""
    if layout == 'each':
        return [[m] for m in range(M)]
    if layout == 'interleaved':
        return [list(range(0, M - 1, 2)), list(range(1, M - 1, 2))]
    if layout == 'all':
        return [list(range(M - 1, -1, -1))]
    if layout == 'scattered':
        return [[M - 1, 2], [0]]
    assert layout == 'hidden-heavy'
    return [[0]]


def hidden_planes(M, sets):
    listed = {m for s in sets for m in s}
    return [m for m in range(M) if m not in listed]


def hidden_block(D):
    """The pixels [0, b) per axis that only hidden planes explain: up to 2 rows of 6 pixels -- a thread's four pixels and
    half of the next thread's -- and at most half of an axis."""
    return tuple(min(b, max(1, d // 2)) for b, d in zip((2, 6)[2 - len(D):], D))


# -- the cases -----------------------------------------------------------------------------------------------------------------
TWO = ('each', 'scattered')
# name -> (N, C, lambda num_cu: M, D, A, layouts, dtypes): the smallest shapes that reach every branch
MATRIX = {
    'vec-ragged': (2, 2, lambda cu: 6, (17, 68), (3, 4), LAYOUTS, DTYPES),       # four tiles, xb >= Dx and y >= Dy under vec
    'vec-c4': (2, 4, lambda cu: 5, (5, 8), (3, 3), TWO, DTYPES),                 # nc == CH == 4, one chunk
    'vec-c5': (2, 5, lambda cu: 7, (9, 12), (3, 4), LAYOUTS, DTYPES),            # a second chunk of one channel under vec
    'vec-stage-loop': (2, 1, lambda cu: 5, (9, 12), (20, 8), ('interleaved', 'hidden-heavy'), DTYPES),   # 35 x 76 > 2560
    'vec-below-halo': (2, 2, lambda cu: 5, (3, 4), (5, 7), ('all', 'scattered'), DTYPES),
    'vec-1d': (2, 3, lambda cu: 7, (1028,), (7,), LAYOUTS, DTYPES),              # two 1-D tiles, threads past Dx
    'pixel-c3': (2, 3, lambda cu: 5, (5, 10), (3, 3), TWO, DTYPES),              # Dx % 4 != 0: pixel by pixel
    # M * 1024 > num_cu * 8 * 256: the last plane's channel sums are written by the second pass of the grid
    'wsum-stride': (1, 2, lambda cu: 2 * cu + 1, (2, 4), (32, 32), ('scattered',), DTYPES),
}
# the runs of tests/test_hip_sources_matrix.py beyond (case, layout, dtype, emit) at aligned pointers and EPS
INTEGER_CASES = ('vec-ragged', 'vec-c5', 'vec-1d')       # small integers, layouts TWO: exact
IDENTITY_CASES = ('vec-ragged', 'vec-c5', 'vec-1d')      # the two store paths, bit for bit
OFFSETS = ((0, 0), (1, 0), (0, 1))                       # (out, V): elements behind an aligned boundary
EPS_CASES = (('vec-ragged', 'interleaved'), ('vec-1d', 'scattered'))   # eps = 0 and eps = the median total


def geometry(name, num_cu=NUM_CU):
    N, C, M, D, A, _, _ = MATRIX[name]
    return N, C, M(num_cu), D, A


def counts(M, A, sets):
    """(n_g [S], n_max): multiply-adds behind a pixel of each source, and the most of any group, the hidden one included."""
    nA = int(np.prod(A))
    n_g = np.array([len(s) * nA for s in sets])
    return n_g, max(int(n_g.max()), (M - sum(len(s) for s in sets)) * nA)


def device_bytes(name, layout, dt, num_cu=NUM_CU):
    """What one call of the case holds on the device: H, W, V, out with its two frames, label, share, the work buffer."""
    N, C, M, D, A = geometry(name, num_cu)
    S, e, px = len(plane_sets(M, layout)), ESIZE[dt], int(np.prod(D))
    Hp = N * M * int(np.prod([d + a - 1 for d, a in zip(D, A)]))
    return (e * (Hp + M * C * int(np.prod(A)) + N * C * px + 1 + N * S * C * px + 2 * 4097 + N * px) + 4 * N * px
            + max(work(C, M, D, A, dt, S, emit)['total'] for emit in EMIT))


def stray_stores(name, layout, num_cu=NUM_CU):
    """What the aligned store of `put` would touch without its `xb < g.Dx` test -- on paper only, such a kernel is never
    run: the threads with y < Dy and xb >= Dx store kAtomPix elements at ``at(gi, c)`` all the same -> (the number of those
    elements that belong to other pixels of `out`, the number beyond its end, the farthest of them behind the end)."""
    N, C, M, D, A = geometry(name, num_cu)
    Dy, Dx, _, _ = dims(D, A)
    p, S = plan(C, D, A), len(plane_sets(M, layout))
    assert Dx % PIX == 0
    xb = np.arange(Dx, p['tiles_x'] * p['TX'], PIX)                            # the threads outside, every row alike
    planes, y = np.arange(N * S * C)[:, None, None, None], np.arange(Dy)[None, :, None, None]
    off = (planes * Dy + y) * Dx + xb[None, None, :, None] + np.arange(PIX)[None, None, None, :]
    n_out = N * S * C * Dy * Dx
    beyond = off[off >= n_out]
    return int(np.sum(off < n_out)), len(beyond), int(beyond.max() - n_out + 1) if len(beyond) else 0


def runs(num_cu=NUM_CU):
    """Every call of the GPU matrix -> (name, layout, dt, emit, out_offset, V_offset, eps kind, operand kind)."""
    for name, (_, _, _, _, _, layouts, dtypes) in MATRIX.items():
        for layout in layouts:
            for dt in dtypes:
                for emit in EMIT:
                    yield name, layout, dt, emit, 0, 0, 'default', 'random'
    for name in INTEGER_CASES + ('wsum-stride',):
        for layout in TWO if name in INTEGER_CASES else MATRIX[name][5]:
            for dt in DTYPES:
                for emit, eps in (('contribution', 'default'), ('dominant', 'default'), ('mask', 'zero')):
                    yield name, layout, dt, emit, 0, 0, eps, 'integer'
    for name in IDENTITY_CASES:
        for dt in DTYPES:
            for emit in ('contribution', 'masked'):
                for out_offset, V_offset in OFFSETS:
                    yield name, 'interleaved', dt, emit, out_offset, V_offset, 'default', 'random'
    for name, layout in EPS_CASES:
        for dt in DTYPES:
            for emit in EMIT:
                for eps in ('zero', 'median'):
                    yield name, layout, dt, emit, 0, 0, eps, 'random'


def reached(name, layout, dt, emit, out_offset=0, V_offset=0, eps='default', kind='random', num_cu=NUM_CU):
    """The names of BRANCHES that one call executes."""
    N, C, M, D, A = geometry(name, num_cu)
    Dy, Dx, Ay, Ax = dims(D, A)
    sets = plane_sets(M, layout)
    S, hidden = len(sets), hidden_planes(M, sets)
    CH, dom = instance(C, emit)
    p = plan(1 if dom else C, D, A)
    assert p['SH'] * p['SW'] * ESIZE[dt] <= LDS_LIMIT and N * p['slots'] <= 0x7fffffff, name
    out = {f'emit:{emit}'}
    if dom:
        out.add(f'DOM:{dt}')
        n_sum, blocks, grid = wsum_grid(M, A, num_cu)
        out.add('wsum:one-block' if blocks == 1 else 'wsum:grid-stride' if blocks > grid else 'wsum:several-blocks')
        out.discard('wsum:several-blocks')
        if blocks > 1 and n_sum % THREADS:
            out.add('wsum:partial-last-block')
        if C == 1:
            out.add('wsum:C==1')
    else:
        nc = chunk_channels(C)
        if CH < CHANNELS:
            out.add(f'CH{CH}:{dt}')
        elif len(nc) == 1:
            out.add(f'CH4:full:{dt}')          # C == 4: nc == CH and no second chunk
        elif nc[-1] < CH:
            out.add(f'CH4:short-second-chunk:{dt}')
        if vec(Dx, out_offset, V_offset, ESIZE[dt]):
            out.add('vec')
            if Dx % p['TX']:
                out.add('vec:thread-outside-x')
            if Dy % p['TY']:
                out.add('vec:row-outside-y')
            if p['tiles_y'] * p['tiles_x'] > 1:
                out.add('vec:several-tiles')
            if p['TY'] == 1:
                out.add('vec:1d')
            if not pre_ok(C, D, A):
                out.add('vec:stage-loop')
            if Dx < Ax - 1 or (Ay > 1 and Dy < Ay - 1):
                out.add('vec:below-halo')
        else:
            out.add('pixelwise:Dx%4' if Dx % PIX else 'pixelwise:out-misaligned' if out_offset % PIX
                    else 'pixelwise:V-misaligned')
    out.add('hidden:empty' if not hidden else 'hidden:one-plane' if len(hidden) == 1 else 'hidden:several')
    out.discard('hidden:several')
    if S == 1:
        out |= {'S==1'} | ({'S==1:rest-hidden'} if hidden else set())
    if S == M:
        out.add('S==M')
    if any(a > b for s in sets for a, b in zip(s, s[1:])) and S > 1 and max(sets[0]) > min(sets[1]):
        out.add('source:planes-descending-and-scattered')
    if eps != 'default':
        out.add('eps==0' if eps == 'zero' else 'eps~total')
    # what depends on the operands: read from the reference
    want = reference(name, layout, dt, 'default', kind, num_cu)
    rc, tc = want['contribution'].sum(axis=2), want['total'].sum(axis=1)
    if np.any((tc > 0) & (rc.max(axis=1) == 0)):
        out.add('pixel:only-hidden-explains')
    if np.any(tc == 0):
        out.add('pixel:nobody-explains')
    if len(hidden) > 1 and np.mean(tc - rc.sum(axis=1) > rc.max(axis=1)) > 0.75:
        out.add('hidden:several-and-largest')
    if dom and S > 1 and np.any((rc[:, 0] == rc.max(axis=1)) & (rc[:, 1] == rc[:, 0]) & (rc[:, 0] > 0)):
        out.add('tie:lowest-index-wins')
    assert out <= set(BRANCHES), out - set(BRANCHES)
    return out


# -- operands and references ---------------------------------------------------------------------------------------------------
def rounded(x, dt):
    return np.asarray(x).astype(NP[dt]).astype(np.float64)


def _plant_hidden_pixels(Hp, D, A, sets, value):
    """Sample 1, the pixels of hidden_block(D): the listed planes zero over their windows, the first hidden plane `value`."""
    M = Hp.shape[1]
    hidden = hidden_planes(M, sets)
    if not hidden:
        return
    region = tuple(slice(0, b + a - 1) for b, a in zip(hidden_block(D), A))
    for m in range(M):
        if m not in hidden:
            Hp[(1, m) + region] = 0.
    Hp[(1, hidden[0]) + region] = value(Hp[(1, hidden[0]) + region].shape)


@functools.lru_cache(maxsize=None)
def operands(name, dt, layout, num_cu=NUM_CU):
    """-> dict of read-only float64 arrays holding values of the element type: padded activations Hp (values >= 0.1 or
    exactly 0, whole planes of zeros among them), W >= 0.1, V >= 0.1; with the plants of the module docstring."""
    N, C, M, D, A = geometry(name, num_cu)
    sets = plane_sets(M, layout)
    rng = np.random.default_rng(sum(map(ord, name + layout)) + 1)
    Hp = (rng.random((N, M) + tuple(d + a - 1 for d, a in zip(D, A))) + 0.1) * (rng.random((N, M) + (1,) * len(D)) > 0.15)
    Hp = Hp * (rng.random(Hp.shape) > 0.3)
    if layout == 'hidden-heavy':
        Hp[:, hidden_planes(M, sets)] *= 8.
    if N > 1:
        _plant_hidden_pixels(Hp, D, A, sets, lambda shape: rng.random(shape) + 0.1)
        Hp[0, ..., -(A[-1] + 1):] = 0.                  # the last two pixels of every row of sample 0: nobody
    out = dict(Hp=rounded(Hp, dt), W=rounded(rng.random((M, C) + A) + 0.1, dt), V=rounded(rng.random((N, C) + D) + 0.1, dt))
    for x in out.values():
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def integer_operands(name, layout, num_cu=NUM_CU):
    """The construction of tests/test_hip_sources.py, integer_operands: small integers, every sum exact in float32; planes
    0 and 1 alike, a block of pixels nobody explains; and the pixels that only hidden planes explain.  Values in 0..3, in
    0..1 where the atom has more than 256 taps (every sum below 2^24)."""
    N, C, M, D, A = geometry(name, num_cu)
    sets = plane_sets(M, layout)
    top = 4 if int(np.prod(A)) <= 256 else 2
    rng = np.random.default_rng(11)
    Hp = rng.integers(0, top, (N, M) + tuple(d + a - 1 for d, a in zip(D, A))).astype(np.float64)
    Hp *= rng.random(Hp.shape) > 0.5
    W = rng.integers(0, top, (M, C) + A).astype(np.float64)
    W[1], Hp[:, 1] = W[0], Hp[:, 0]
    if N > 1:
        Hp[0, ..., : A[-1] + 3] = 0.
        _plant_hidden_pixels(Hp, D, A, sets, lambda shape: np.full(shape, top - 1.))
    V = rng.integers(0, 9, (N, C) + D).astype(np.float64)
    out = dict(Hp=Hp, W=W, V=V)
    for x in out.values():
        x.setflags(write=False)
    return out


def fast_parts(W, Hp):
    """atoms_reference.parts_valid(W, Hp, 1) as one contraction over sliding windows: [N, M, C, *D], float64."""
    W, Hp = np.asarray(W, dtype=np.float64), np.asarray(Hp, dtype=np.float64)
    k = W.ndim - 2
    win = sliding_window_view(Hp, W.shape[2:], axis=tuple(range(2, 2 + k)))
    Wf = W[(Ellipsis,) + (slice(None, None, -1),) * k]
    return np.einsum('nmyxab,mcab->nmcyx' if k == 2 else 'nmxa,mca->nmcx', win, Wf, optimize=True)


def finish(parts, parts_c, V, sets, eps, defect=None, CH=CHANNELS):
    """sources_reference.outputs from the per-plane parts [N, M, C, *D] and the parts of the channel sums [N, M, *D] --
    the walk on sum_c W that the dominant source takes.  ``defect``: one of WRONG."""
    N, M, C = parts.shape[:3]
    order, start = tables(sets, M)
    S = len(sets)
    start = start.copy()
    if defect == 'boundary-off-by-one':
        start[1:S + 1] -= 1
    groups = [order[start[k]:start[k + 1]] for k in range(S + 1)]
    r = np.stack([parts[:, g].sum(axis=1) for g in groups[:S]], axis=1)
    rc = np.stack([parts_c[:, g].sum(axis=1) for g in groups[:S]], axis=1)
    hidden, hidden_c = (0. if defect == 'total-without-hidden' else x[:, groups[S]].sum(axis=1) for x in (parts, parts_c))
    total, tc = r.sum(axis=1) + hidden, rc.sum(axis=1) + hidden_c
    e = 0. if defect == 'eps-dropped' else eps
    den = (total + e)[:, None]
    if defect == 'total-of-sample-0':
        den = np.broadcast_to(den[:1], den.shape)
    mask = np.divide(r, den, out=np.zeros(r.shape), where=den != 0)
    V = np.asarray(V, dtype=np.float64)
    if defect == 'masked-times-first-channel-V':
        V = V[:, [c // CH * CH for c in range(C)]]
    label = np.full(tc.shape, -1, dtype=np.int32)
    best = np.zeros(tc.shape)
    for g in range(S):
        better = (rc[:, g] >= best if defect == 'tie-last' else rc[:, g] > best) if g else np.ones(tc.shape, dtype=bool)
        label[better], best[better] = g, rc[:, g][better]
    label[(best if defect == 'label-minus-one-on-best' else tc) == 0] = -1
    tden = (total[:, 0] if defect == 'share-over-channel-0' else tc) + e
    share = np.divide(best, tden, out=np.zeros(tc.shape), where=tden != 0)
    return dict(contribution=r, mask=mask, masked=V[:, None] * mask, label=label, share=share, total=total)


# defect -> (case, layout, operand kind, eps kind, the outputs that must show it)
WRONG = {
    'total-without-hidden': ('vec-ragged', 'hidden-heavy', 'random', 'default', ('mask', 'masked', 'share')),
    'tie-last': ('vec-ragged', 'each', 'integer', 'default', ('label',)),
    'label-minus-one-on-best': ('vec-c5', 'scattered', 'integer', 'default', ('label',)),
    'wsum-drops-last-channel': ('vec-ragged', 'interleaved', 'random', 'default', ('share',)),
    'share-over-channel-0': ('vec-c4', 'scattered', 'random', 'default', ('share',)),
    'masked-times-first-channel-V': ('vec-c4', 'each', 'random', 'default', ('masked',)),
    'second-chunk-reads-first': ('vec-c5', 'interleaved', 'random', 'default', ('contribution', 'mask', 'masked')),
    'total-of-sample-0': ('vec-1d', 'each', 'random', 'default', ('mask', 'masked')),
    'boundary-off-by-one': ('vec-1d', 'scattered', 'random', 'default', ('contribution', 'mask', 'masked', 'share')),
    'eps-dropped': ('vec-ragged', 'interleaved', 'random', 'median', ('mask', 'masked', 'share')),
    'wsum-missing-tail': ('wsum-stride', 'scattered', 'integer', 'default', ('label', 'share')),
}


def ops_of(name, dt, layout, kind='random', num_cu=NUM_CU):
    return operands(name, dt, layout, num_cu) if kind == 'random' else integer_operands(name, layout, num_cu)


def eps_of(name, layout, dt, eps, kind='random', num_cu=NUM_CU):
    """The eps of a run as the element type holds it: EPS, 0, or the median of the reference's totals."""
    if eps == 'median':
        return float(NP[dt](np.median(reference(name, layout, dt, 'default', kind, num_cu)['total'])))
    return float(NP[dt](EPS if eps == 'default' else 0.))


def outputs(name, layout, dt, eps='default', kind='random', num_cu=NUM_CU, defect=None):
    """The reference through ``fast_parts`` and ``finish`` -- and, with ``defect``, the wrong model of that name (at
    num_cu compute units, for the defect that depends on them)."""
    N, C, M, D, A = geometry(name, num_cu)
    ops = ops_of(name, dt, layout, kind, num_cu)
    W = np.array(ops['W'])
    if defect == 'second-chunk-reads-first':
        W = W[:, [c % CHANNELS for c in range(C)]]
    Ws = (W[:, :-1] if defect == 'wsum-drops-last-channel' else W).sum(axis=1, keepdims=True)
    if defect == 'wsum-missing-tail':            # (flat element i = plane * prod(A) + a of k_source_wsum)
        Ws.reshape(-1)[num_cu * WSUM_PER_CU * THREADS:] = 0.
    return finish(fast_parts(W, ops['Hp']), fast_parts(Ws, ops['Hp'])[:, :, 0], ops['V'], plane_sets(M, layout),
                  eps_of(name, layout, dt, eps, kind, num_cu), defect, min(C, CHANNELS))


@functools.lru_cache(maxsize=None)
def reference(name, layout, dt, eps='default', kind='random', num_cu=NUM_CU):
    """sources_reference.outputs on the case's operands, float64, read-only.  The case of many planes of 1024 taps goes
    through the one contraction of ``fast_parts`` (tests/test_sources_dispatch_cpu.py holds the two to each other)."""
    N, C, M, D, A = geometry(name, num_cu)
    if M * int(np.prod(A)) > 4096:
        want = outputs(name, layout, dt, eps, kind, num_cu)
    else:
        ops = ops_of(name, dt, layout, kind, num_cu)
        want = sref.outputs(ops['W'], ops['Hp'], ops['V'], plane_sets(M, layout), eps_of(name, layout, dt, eps, kind, num_cu))
    for x in want.values():
        x.setflags(write=False)
    return want


# -- the bounds of tests/test_hip_sources.py, derived there --------------------------------------------------------------------
def bounds(want, C, M, A, sets, dt, exact=False):
    """emit -> the bound on |got - want|, elementwise.  ``exact`` (integer operands): 0 for the contribution, 2 u for the
    share -- only total + eps and the division round."""
    u, S, k = U[dt], len(sets), len(A)
    n_g, n_max = counts(M, A, sets)
    per_source = n_g.reshape((1, S, 1) + (1,) * k)
    if exact:
        return dict(contribution=np.zeros(want['contribution'].shape), share=2 * u * want['share'])
    return dict(contribution=(per_source + 8) * u * np.abs(want['contribution']),
                mask=(per_source + n_max + S + 8) * u * np.abs(want['mask']),
                masked=(per_source + n_max + S + 8) * u * np.abs(want['masked']),
                share=(int(n_g.max()) + n_max + S + 8 + 2 * (C - 1)) * u * want['share'])


def label_violations(label, want, C, M, A, sets, dt):
    """The pixels whose label differs from the reference's beyond the near-tie rule of tests/test_hip_sources.py: a label may
    differ only where the chosen source is within rounding of the largest.  A total of 0 is a sum of zeros, exact in
    any element type: there the label is -1 and nothing else."""
    _, n_max = counts(M, A, sets)
    rc, tc = want['contribution'].sum(axis=2), want['total'].sum(axis=1)
    differ = label != want['label']
    chosen = np.take_along_axis(rc, np.maximum(label, 0)[:, None].astype(np.int64), axis=1)[:, 0]
    near = (label >= 0) & (tc > 0) & (rc.max(axis=1) - chosen <= 2 * (n_max + C + 8) * U[dt] * rc.max(axis=1))
    return int(np.sum(differ & ~near))
