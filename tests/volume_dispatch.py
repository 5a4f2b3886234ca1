"""
Host mirror of the three-shift-axis family: the kernels of tnmf_amd/csrc/volume.hip and the vol_api_*
entries of tnmf_amd/csrc/api.hip, restated in plain Python so that the tests can choose the smallest cases that reach every
branch -- the tap blocks and the lane loop of k_vol_corr_H, every bound of its chunk count, the arms of the entries that
take a reconstruction, the index maps of k_vol_pad / k_vol_fold at their limits, the terms of k_vol_lateral, the refusals
of to_vol (tests/test_hip_volume_matrix.py) -- and a CPU test can check that they do (tests/test_volume_dispatch_cpu.py).

A geometry is (N, C, D, M, A) with three-component D and A, as in the other mirrors.  A cell is (group, name).
"""
from collections import namedtuple

kVolBlock = 256                 # volume.hip: threads per workgroup, voxels per tile
kVolTaps = 8                    # volume.hip: taps ax one pass of k_vol_corr_H keeps in registers
WAVES = kVolBlock // 64         # the waves of a workgroup take the rows of its chunk in turn
P_CAP = 1024                    # volume.hip: vol_corr_H_chunks
WG_PER_CU = 4                   # volume.hip: 4L * ctx->num_cu
ROWS_PER_CHUNK = 8              # volume.hip: rows / 8
GRID_PER_CU = 32                # volume.hip: num_cu * 32, the cap of the pad / fold / lateral grid
LIM = 0x7fffffff                # volume.hip: vol_fits
kEnergyPartials = 2048          # generic.h
kMaxTaps = 127                  # generic.h
CUS = (256, 304)                # compute units of the devices the cells are evaluated at
MODES = ('valid', 'full', 'circular', 'reflect')
ESIZE = {'f': 4, 'd': 8}
DTYPES = ('f', 'd')

Vol = namedtuple('Vol', 'N M C D A H')


def cdiv(a, b):
    return (a + b - 1) // b


def align_up(a, b):
    return cdiv(a, b) * b


def prod(t):
    out = 1
    for x in t:
        out *= x
    return out


# ----------------------------------------------------------------------------------------------------------------------
# api.hip: to_vol
# ----------------------------------------------------------------------------------------------------------------------
def to_vol(geometry, dtype=0, h_row_stride=0, null=False):
    """(error or None, Vol or None), the refusals in the library's order: the pointer, the dtype, N / M / C, then each
    axis in turn, the row stride last.  H = D + A - 1; a row stride is accepted only when it IS the row length."""
    if null:
        return 'E_NULL', None
    if dtype not in (0, 1):
        return 'E_DTYPE', None
    N, C, D, M, A = geometry
    if N < 0 or M <= 0 or C <= 0:
        return 'E_GEOM', None
    H = []
    for i in range(3):
        if D[i] <= 0 or A[i] <= 0:
            return 'E_GEOM', None
        H.append(D[i] + A[i] - 1)
    if h_row_stride > 0 and h_row_stride != H[2]:
        return 'E_STRIDE', None
    return None, Vol(N, M, C, tuple(D), tuple(A), tuple(H))


def vol(geometry):
    err, v = to_vol(geometry)
    assert err is None, (geometry, err)
    return v


def vol_fits(v):
    """volume.hip: vol_fits -- every index inside one volume is an int."""
    vox, hvox, avox = prod(v.D), prod(v.H), prod(v.A)
    tiles = cdiv(hvox, kVolBlock)
    return vox < LIM and hvox < LIM and avox * v.M * v.C < LIM and tiles * v.N * max(v.M, v.C) < LIM


# ----------------------------------------------------------------------------------------------------------------------
# volume.hip: the W gradient (k_vol_corr_H, k_vol_corr_H_finalize)
# ----------------------------------------------------------------------------------------------------------------------
def corr_H_entries(v):
    return v.M * v.C * v.A[0] * v.A[1]


def corr_H_rows(v):
    return v.N * v.D[0] * v.D[1]


def vol_corr_H_chunks(v, cus):
    """volume.hip: vol_corr_H_chunks -- four workgroups per compute unit, no chunk below eight rows, at most 1024."""
    P = cdiv(WG_PER_CU * cus, corr_H_entries(v))
    P = min(P, corr_H_rows(v) // ROWS_PER_CHUNK, P_CAP)
    return max(P, 1)


def chunk_bounds(v, P):
    """[(r0, r1)] of every chunk p: rows * p / P."""
    rows = corr_H_rows(v)
    return [(rows * p // P, rows * (p + 1) // P) for p in range(P)]


def waves_with_rows(v, P):
    """Waves of the workgroup of the smallest chunk that get a row at all (r = r0 + wave < r1)."""
    return min(WAVES, min(r1 - r0 for r0, r1 in chunk_bounds(v, P)))


def tap_blocks(ax):
    """nt of every pass of `for (a0 = 0; a0 < A[2]; a0 += kVolTaps)`."""
    return [min(kVolTaps, ax - a0) for a0 in range(0, ax, kVolTaps)]


def lane_trips(dx):
    """Trips of `for (x = lane; x < D[2]; x += 64)` of lane 0, and the lanes that take the last one."""
    return cdiv(dx, 64), (dx - 1) % 64 + 1


def grids(v, cus, P=None):
    """The launch grids of the family (workgroups of 256 threads)."""
    P = vol_corr_H_chunks(v, cus) if P is None else P
    n = v.M * v.C * prod(v.A)
    return {'reconstruct': cdiv(prod(v.D), kVolBlock) * v.N * v.C,
            'corr_W': cdiv(prod(v.H), kVolBlock) * v.N * v.M,
            'corr_H': corr_H_entries(v) * P,
            'finalize': cdiv(n, kVolBlock)}


def strided_grid(total, cus):
    """Pad, fold and lateral terms: (blocks, passes of the grid-stride loop)."""
    if total == 0:
        return 0, 0
    blocks = min(cdiv(total, kVolBlock), cus * GRID_PER_CU)
    return blocks, cdiv(total, blocks * kVolBlock)


def vol_scratch(v, T, cus, extra=0):
    """api.hip: vol_scratch -- [R of the slice | energy partials + result | partial sums of the W gradient] (+ extra)."""
    r = align_up(v.N * v.C * prod(v.D) * ESIZE[T], 256)
    e = align_up((kEnergyPartials + 8) * 8, 256)
    p = align_up(vol_corr_H_chunks(v, cus) * v.M * v.C * prod(v.A) * 2 * 8, 256)
    return {'R': (0, r), 'red': (r, e), 'part': (r + e, p), 'total': r + e + p + extra}


# ----------------------------------------------------------------------------------------------------------------------
# volume.hip: the reconstruction modes (vol_pad_src, vol_pad_dup, vol_pad_fold)
# ----------------------------------------------------------------------------------------------------------------------
def vol_pad_src(j, S, a, mode):
    """Activation copied to padded position j, or -1."""
    l = a - 1
    if mode == 'full':
        u = j - l
        return u if 0 <= u < S else -1
    if j >= l:
        return j - l
    return S - l + j if mode == 'circular' else l - j


def vol_pad_dup(u, S, a, mode):
    """Second padded copy of activation u, or -1."""
    l = a - 1
    if mode == 'circular':
        return u - (S - l) if u >= S - l else -1
    if mode == 'reflect':
        return l - u if 1 <= u <= l else -1
    return -1


def mode_S(d, a, mode):
    """Activation length of one axis: the `S` line of vol_pad_fold and of vol_api_update_H_ex."""
    return d + a - 1 if mode == 'valid' else (d - a + 1 if mode == 'full' else d)


def pad_fold_guard(D, A, mode):
    """vol_pad_fold: None, or 'E_GEOM' -- per axis: S < 1, 'circular' wraps at most once, 'reflect' without the edge."""
    for d, a in zip(D, A):
        S = mode_S(d, a, mode)
        if S < 1:
            return 'E_GEOM'
        if mode == 'circular' and a - 1 > S:
            return 'E_GEOM'
        if mode == 'reflect' and a - 1 >= S:
            return 'E_GEOM'
    return None


def axis_class(d, a, mode):
    """The state of one padded axis (as lateral_dispatch.mode_axis names them)."""
    S, l = mode_S(d, a, mode), a - 1
    if l == 0:
        return 'l0'
    if mode == 'full':
        return 'full_S1' if S == 1 else ('full_long' if l > S else 'full')
    if mode == 'circular':
        return 'circ_all' if l == S else ('circ_all_but_one' if l == S - 1 else 'circ')
    return 'refl_max' if l == S - 1 else 'refl'


AXIS_CLASSES = {'full': ('l0', 'full', 'full_S1', 'full_long'),
                'circular': ('l0', 'circ', 'circ_all_but_one', 'circ_all'),
                'reflect': ('l0', 'refl', 'refl_max')}


# ----------------------------------------------------------------------------------------------------------------------
# api.hip: the arms of the entries
# ----------------------------------------------------------------------------------------------------------------------
def grad_H_arm(v, R_given):
    """vol_api_grad_H: (arm, kernels)."""
    if v.N == 0:
        return 'empty', ()
    if R_given:
        return 'R_given', ('k_vol_corr_W',)
    return 'R_null', ('k_vol_reconstruct', 'k_vol_corr_W')


def grad_W_arm(v, r_scratch, r_is_valid):
    """vol_api_grad_W: (arm, kernels).  An empty slice still runs the correlation: every sum is zero."""
    tail = ('k_vol_corr_H', 'k_vol_corr_H_finalize')
    if v.N == 0:
        return 'empty', tail
    if r_is_valid:
        return 'valid_R', tail
    return ('caller_scratch' if r_scratch else 'library_scratch'), ('k_vol_reconstruct',) + tail


def update_H_arm(v, r_scratch, r_is_valid):
    """vol_api_update_H: (arm or error, kernels)."""
    if v.N == 0:
        return 'empty', ()
    if not r_scratch and r_is_valid:
        return 'E_NULL', ()
    if r_is_valid:
        return 'valid_R', ('k_vol_corr_W<fused>',)
    return ('caller_scratch' if r_scratch else 'library_scratch'), ('k_vol_reconstruct', 'k_vol_corr_W<fused>')


def cross_factor(M, cross):
    """The `xc` line: cross / (M - 1), only when there is another atom."""
    return cross / (M - 1) if cross > 0 and M > 1 else 0.0


def update_H_ex_arm(v, mode, inhibition=0., cross=0., klen=(1, 1, 1), mode_code=None):
    """vol_api_update_H_ex: (error or None, kernels, xc).  The refusals in the library's order; the guards of the pad
    come after the lateral-term kernels have run on the library's work arrays (H itself is untouched)."""
    code = MODES.index(mode) if mode_code is None else mode_code
    if code < 0 or code > 3:
        return 'E_UNSUPPORTED', (), 0.
    if v.N == 0:
        return None, (), 0.
    if inhibition < 0 or cross < 0:
        return 'E_GEOM', (), 0.
    lateral = inhibition > 0 or cross > 0
    if lateral and any(k < 1 or k > kMaxTaps or k % 2 == 0 for k in klen):
        return 'E_UNSUPPORTED', (), 0.
    xc = cross_factor(v.M, cross)
    if mode == 'valid' and not lateral:
        return None, update_H_arm(v, True, False)[1], xc
    if any(mode_S(d, a, mode) < 1 for d, a in zip(v.D, v.A)):
        return 'E_GEOM', (), xc
    kernels = ('k_convolve_axis',) * 3 + ('k_vol_lateral',) if lateral else ()
    if mode == 'valid':
        return None, kernels + ('k_vol_reconstruct', 'k_vol_corr_W', 'k_mu_update_extra'), xc
    if pad_fold_guard(v.D, v.A, mode):
        return 'E_GEOM', kernels, xc
    return None, kernels + ('k_vol_pad', 'k_vol_reconstruct', 'k_vol_corr_W', 'k_vol_fold', 'k_vol_fold',
                            'k_mu_update_extra'), xc


def lateral_class(M, inhibition, cross):
    if not (inhibition > 0 or cross > 0):
        return 'none'
    if cross > 0 and M == 1:
        return 'M_1_cross_dropped'
    return 'both' if inhibition > 0 and cross > 0 else ('inh_only' if inhibition > 0 else 'cross_only')


# ----------------------------------------------------------------------------------------------------------------------
# cells
# ----------------------------------------------------------------------------------------------------------------------
def tap_class(ax):
    b = tap_blocks(ax)
    full = sum(1 for nt in b if nt == kVolTaps)
    rag = b[-1] if b[-1] < kVolTaps else 0
    return f'taps_{full}_full_{"plus_1" if rag == 1 else ("plus_ragged" if rag else "exact")}'


TAP_CELLS = ('taps_0_full_plus_ragged', 'taps_1_full_exact', 'taps_1_full_plus_1', 'taps_2_full_exact', 'taps_2_full_plus_ragged')
LANE_CELLS = ('lanes_64', 'lanes_65', 'lanes_3_trips')
CHUNK_CELLS = ('P_cap_1024', 'P_by_entries', 'P_by_rows', 'P_1_entries_gt_4cu', 'P_1_rows_lt_8', 'idle_waves', 'chunks_ragged',
               'two_channels_two_blocks', 'empty_slice', 'last_slice')
TILE_CELLS = ('vox_256', 'vox_257', 'atom_longer_than_sample_on_two_axes', 'one_voxel_atoms')
ARM_CELLS = tuple(('grad_W', a) for a in ('valid_R', 'caller_scratch', 'library_scratch', 'empty_caller_scratch')) + tuple(
    ('grad_H', a) for a in ('R_given', 'R_null')) + tuple(('update_H', a) for a in ('valid_R', 'caller_scratch', 'library_scratch'))
PAD_CELLS = tuple(c for cs in AXIS_CLASSES.values() for c in cs if c != 'l0') + (
    'l0_next_to_padded', 'grid_stride_pad', 'grid_stride_fold', 'adjoint', 'refused_circular', 'refused_reflect',
    'refused_full_S_lt_1')
LATERAL_CELLS = tuple(f'{m}_{t}' for m in MODES for t in ('none', 'inh_only', 'cross_only', 'both')) + (
    'M_1_cross_dropped', 'parabolic_kernels', 'random_kernels', 'no_r_scratch', 'r_scratch', 'tap')
ENTRIES = ('reconstruct', 'grad_H', 'grad_W', 'update_H', 'update_H_ex', 'pad_H')
TO_VOL_REFUSALS = {'dtype_2': 'E_DTYPE', 'N_negative': 'E_GEOM', 'M_0': 'E_GEOM', 'D_0': 'E_GEOM', 'stride_plus_1': 'E_STRIDE'}
REFUSAL_CELLS = tuple(f'{e}_{r}' for e in ENTRIES for r in TO_VOL_REFUSALS) + (
    'stride_equal_accepted', 'bad_mode', 'even_klen', 'context_works_afterwards')


def required():
    req = {('corr_H', c) for c in TAP_CELLS + LANE_CELLS + CHUNK_CELLS}
    req |= {('tiles', c) for c in TILE_CELLS}
    req |= {('arm',) + c for c in ARM_CELLS}
    req |= {('pad', c) for c in PAD_CELLS}
    req |= {('lateral', c) for c in LATERAL_CELLS}
    req |= {('refusal', c) for c in REFUSAL_CELLS}
    return req


# Refusals no call can reach.
UNREACHABLE = {
    ('refusal', 'corr_H_grid'): 'entries * P > 2^31 - 1 (vol_corr_H): vol_fits holds entries below 2^31 - 1, and P is at most '
                                'cdiv(4 * CUs, entries), which is 1 for any entries above 4 * CUs',
}

# What the matrix leaves out, with the reason (tests/test_volume_dispatch_cpu.py checks the list is exact).
NOT_COVERED = {
    ('refusal', 'vol_fits'): 'a volume of 2^31 - 1 voxels would hand real pointers to an entry whose only protection is the guard '
                             'under test; the arithmetic of the guard is held on the mirror instead '
                             '(test_vol_fits_at_its_four_boundaries)',
    ('refusal', 'workspace'): 'TNMF_E_WORKSPACE of vol_scratch / ensure_hwork needs a device whose memory is exhausted, which '
                              'a test on a shared machine must not bring about',
}

# ----------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_hip_volume_matrix.py
# ----------------------------------------------------------------------------------------------------------------------
# kind 'prim': geometry; P = the chunk count the case was chosen for (an int, or {CUs: P}); slices: the empty and the
#              last-sample slice are run as well
# kind 'pad':  geometry (C is 1), mode
# kind 'ex':   geometry, mode, terms = the lateral classes run, kernels 'random' | 'parabolic'
Case = namedtuple('Case', 'kind geometry mode P slices terms kernels')


def prim(geometry, P, slices=False):
    return Case('prim', geometry, 'valid', P, slices, (), None)


def pad(geometry, mode):
    return Case('pad', geometry, mode, None, False, (), None)


def ex(geometry, mode, terms, kernels='random'):
    return Case('ex', geometry, mode, None, False, tuple(terms), kernels)


ALL_TERMS = ('none', 'inh_only', 'cross_only', 'both')
STRENGTHS = {'none': (0., 0.), 'inh_only': (0.1, 0.), 'cross_only': (0., 0.05), 'both': (0.1, 0.05)}   # the project's usual
EX = (2, 2, (4, 5, 6), 3, (2, 3, 2))
EX_M1 = (2, 1, (4, 5, 6), 1, (2, 3, 2))

MATRIX = {
    # ---- k_vol_corr_H: the tap blocks, the lane loop
    't7': prim((2, 1, (3, 4, 20), 2, (2, 2, 7)), 3),
    't8': prim((2, 1, (3, 4, 20), 2, (2, 2, 8)), 3),
    't9_c2': prim((2, 2, (3, 4, 20), 2, (1, 2, 9)), 3, slices=True),
    't16_d64': prim((1, 1, (2, 5, 64), 3, (2, 1, 16)), 1),
    't19_d65': prim((2, 1, (3, 3, 65), 2, (2, 2, 19)), 2, slices=True),
    'd130': prim((1, 2, (2, 3, 130), 2, (1, 2, 3)), 1),
    # ---- vol_corr_H_chunks
    'p_cap': prim((2, 1, (64, 65, 8), 1, (1, 1, 3)), 1024),
    'p_entries': prim((3, 2, (3, 4, 5), 5, (6, 10, 2)), {256: 2, 304: 3}),
    'p_one': prim((1, 4, (4, 4, 3), 8, (7, 6, 2)), 1),
    'p_rows3': prim((1, 1, (1, 3, 2), 1, (1, 1, 1)), 1),
    'p_ragged': prim((2, 1, (13, 1, 9), 2, (2, 1, 3)), 3),
    # ---- tiles of one thread per voxel
    'vox256': prim((1, 1, (4, 8, 8), 2, (2, 2, 2)), 4),
    'vox257': prim((1, 1, (1, 1, 257), 2, (1, 1, 2)), 1),
    'long_atom': prim((2, 1, (2, 3, 4), 2, (5, 3, 9)), 1),
    # ---- k_vol_pad / k_vol_fold
    'pad_circ_all': pad((2, 1, (2, 3, 4), 3, (3, 4, 5)), 'circular'),
    'pad_refl_max': pad((2, 1, (3, 4, 5), 3, (3, 4, 5)), 'reflect'),
    'pad_full_s1': pad((2, 1, (4, 2, 4), 3, (4, 1, 2)), 'full'),
    'pad_full_mixed': pad((2, 1, (7, 5, 5), 2, (3, 1, 4)), 'full'),
    'pad_circ_mixed': pad((2, 1, (5, 4, 3), 2, (3, 4, 1)), 'circular'),
    'pad_refl_mixed': pad((2, 1, (5, 4, 3), 2, (3, 4, 1)), 'reflect'),
    'pad_large': pad((4, 1, (60, 60, 60), 4, (3, 1, 2)), 'circular'),
    'pad_circ_refused': pad((2, 1, (2, 3, 4), 3, (3, 4, 6)), 'circular'),
    'pad_refl_refused': pad((2, 1, (3, 4, 5), 3, (3, 5, 5)), 'reflect'),
    'pad_full_refused': pad((2, 1, (3, 4, 5), 3, (3, 4, 6)), 'full'),
    # ---- vol_api_update_H_ex
    **{f'ex_{m}': ex(EX, m, ALL_TERMS) for m in MODES},
    'ex_parabolic': ex(EX, 'circular', ('both',), 'parabolic'),
    'ex_m1': ex(EX_M1, 'valid', ('M_1_cross_dropped',)),
    'ex_m1_reflect': ex(EX_M1, 'reflect', ('M_1_cross_dropped',)),
}
REFUSAL_GEOMETRY = (2, 2, (3, 4, 5), 3, (2, 2, 3))


def chosen_P(case, cus):
    return case.P[cus] if isinstance(case.P, dict) else case.P


def reached(case, cus, backend_only=False):
    """The cells one case reaches on a device of `cus` compute units.  backend_only: through the forms HIP.py makes alone
    (it always brings its own R_scratch and never a finished reconstruction) -- what the older tests could reach."""
    out = set()
    v = vol(case.geometry)
    if case.kind == 'prim':
        P = vol_corr_H_chunks(v, cus)
        entries, rows = corr_H_entries(v), corr_H_rows(v)
        by_entries = cdiv(WG_PER_CU * cus, entries)
        out.add(('corr_H', tap_class(v.A[2])))
        trips, _ = lane_trips(v.D[2])
        for name, hit in (('lanes_64', v.D[2] == 64), ('lanes_65', v.D[2] == 65), ('lanes_3_trips', trips >= 3),
                          ('P_cap_1024', P == P_CAP and by_entries >= P_CAP and rows // ROWS_PER_CHUNK > P_CAP),
                          ('P_by_entries', 1 < P == by_entries < rows // ROWS_PER_CHUNK),
                          ('P_by_rows', 1 < P == rows // ROWS_PER_CHUNK < min(by_entries, P_CAP)),
                          ('P_1_entries_gt_4cu', entries > WG_PER_CU * cus and rows // ROWS_PER_CHUNK > 1),
                          ('P_1_rows_lt_8', rows < ROWS_PER_CHUNK),
                          ('idle_waves', waves_with_rows(v, P) < WAVES),
                          ('chunks_ragged', rows % P != 0),
                          ('two_channels_two_blocks', v.C > 1 and len(tap_blocks(v.A[2])) > 1),
                          ('empty_slice', case.slices), ('last_slice', case.slices and v.N > 1)):
            if hit:
                out.add(('corr_H', name))
        for name, hit in (('vox_256', prod(v.D) == kVolBlock), ('vox_257', prod(v.D) == kVolBlock + 1),
                          ('atom_longer_than_sample_on_two_axes', sum(a > d for a, d in zip(v.A, v.D)) >= 2),
                          ('one_voxel_atoms', prod(v.A) == 1)):
            if hit:
                out.add(('tiles', name))
        # every primitive case is run through every arm of the entries that take a reconstruction
        forms = ((True, False),) if backend_only else ((False, False), (True, False), (True, True))
        out |= {('arm', 'grad_W', grad_W_arm(v, s, r)[0]) for s, r in forms}
        out |= {('arm', 'grad_H', grad_H_arm(v, r)[0]) for r in ((False,) if backend_only else (False, True))}
        out |= {('arm', 'update_H', update_H_arm(v, s, r)[0]) for s, r in forms}
        if case.slices and not backend_only:
            out.add(('arm', 'grad_W', 'empty_caller_scratch'))
    elif case.kind == 'pad':
        guard = pad_fold_guard(v.D, v.A, case.mode)
        if guard:
            S = [mode_S(d, a, case.mode) for d, a in zip(v.D, v.A)]
            out.add(('pad', 'refused_full_S_lt_1' if min(S) < 1 else 'refused_' + case.mode))
            return out
        classes = [axis_class(d, a, case.mode) for d, a in zip(v.D, v.A)]
        out |= {('pad', c) for c in classes if c != 'l0'}
        if 'l0' in classes and len(set(classes)) > 1:
            out.add(('pad', 'l0_next_to_padded'))
        S = [mode_S(d, a, case.mode) for d, a in zip(v.D, v.A)]
        if strided_grid(v.N * v.M * prod(v.H), cus)[1] > 1:
            out.add(('pad', 'grid_stride_pad'))
        if strided_grid(v.N * v.M * prod(S), cus)[1] > 1:
            out.add(('pad', 'grid_stride_fold'))
        if not backend_only:
            out.add(('pad', 'adjoint'))
    else:
        for t in case.terms:
            inh, cross = STRENGTHS['both' if t == 'M_1_cross_dropped' else t]
            err, kernels, xc = update_H_ex_arm(v, case.mode, inh, cross, (3, 3, 3))
            assert err is None, (case, t)
            cls = lateral_class(v.M, inh, cross)
            assert cls == t, (case, t, cls)
            out.add(('lateral', cls if cls == 'M_1_cross_dropped' else f'{case.mode}_{cls}'))
            assert (xc == 0.) == (cls in ('none', 'inh_only', 'M_1_cross_dropped'))
        out.add(('lateral', case.kernels + '_kernels'))
        out |= {('lateral', c) for c in (('r_scratch',) if backend_only else ('no_r_scratch', 'r_scratch'))}
        if case.mode == 'valid' and 'both' in case.terms:
            out.add(('lateral', 'tap'))
    return out


def reached_by(matrix, cus, backend_only=False):
    """{cell: [case ids]} over the matrix and the refusals of to_vol, which every matrix carries."""
    got = {}
    for cid, case in matrix.items():
        for cell in reached(case, cus, backend_only):
            got.setdefault(cell, []).append(cid)
    if backend_only:
        return got
    for e in ENTRIES:
        for r, err in TO_VOL_REFUSALS.items():
            if refused_geometry(r)[3] == err:
                got[('refusal', f'{e}_{r}')] = ['refusals']
    G = REFUSAL_GEOMETRY
    if to_vol(G, 0, vol(G).H[2])[0] is None:
        got[('refusal', 'stride_equal_accepted')] = ['refusals']
    if update_H_ex_arm(vol(G), 'valid', mode_code=4)[0] == 'E_UNSUPPORTED' and update_H_ex_arm(vol(G), 'valid', mode_code=-1)[0]:
        got[('refusal', 'bad_mode')] = ['refusals']
    if update_H_ex_arm(vol(G), 'valid', 0.1, 0., (3, 4, 3))[0] == 'E_UNSUPPORTED':
        got[('refusal', 'even_klen')] = ['refusals']
    got[('refusal', 'context_works_afterwards')] = ['refusals']
    return got


def refused_geometry(name):
    """(geometry, dtype code, row stride, the error to_vol answers) of one refusal, on REFUSAL_GEOMETRY."""
    N, C, D, M, A = REFUSAL_GEOMETRY
    G, dtype, stride = REFUSAL_GEOMETRY, 0, 0
    if name == 'dtype_2':
        dtype = 2
    elif name == 'N_negative':
        G = (-1, C, D, M, A)
    elif name == 'M_0':
        G = (N, C, D, 0, A)
    elif name == 'D_0':
        G = (N, C, (D[0], 0, D[2]), M, A)
    elif name == 'stride_plus_1':
        stride = D[2] + A[2]
    else:
        raise KeyError(name)
    return G, dtype, stride, to_vol(G, dtype, stride)[0]


def missing(matrix=None, cus=CUS):
    """The required cells the matrix does not reach at every one of `cus`."""
    matrix = MATRIX if matrix is None else matrix
    out = set()
    for cu in cus:
        got = reached_by(matrix, cu)
        out |= {c for c in required() if c not in got}
    return sorted(out)


def sole_carriers(matrix=None, cus=CUS):
    """{case id: [required cells only it carries at one of `cus`]}."""
    matrix = MATRIX if matrix is None else matrix
    out = {}
    for cu in cus:
        for cell, cids in reached_by(matrix, cu).items():
            if cell in required() and len(cids) == 1 and cids[0] in matrix and cell not in out.get(cids[0], []):
                out.setdefault(cids[0], []).append(cell)
    return out
