"""
Host mirror of the H half step in full: the route of update_H_2d (tnmf_amd/csrc/api.hip) through the
lateral-term kernels of tnmf_amd/csrc/inhibit.hip (k_inhibition, k_mu_update_extra, k_fold_update) and the pad / fold
kernels of tnmf_amd/csrc/generic.hip (k_pad_H, k_fold_H), restated in plain Python so that the tests can choose cases that
reach every k_inhibition instance, both staging forms, the LDS arm above 64 KiB, every refusal and every route
(tests/test_hip_lateral_matrix.py), and a CPU test can check that the choice covers them all
(tests/test_lateral_dispatch_cpu.py).  Which kernel FAMILY takes the reconstruction and the correlation with W is not
restated here: direct_dispatch, split_dispatch and fft_dispatch answer that.

A case is (geometry, dtype, path, mode, taps, strengths, layout, kernels): geometry = (N, C, D, M, A) as in
direct_dispatch; dtype 'f' / 'd'; path 'generic', 'mfma', 'fft' or 'auto'; mode one of MODES; taps = the inhibition
kernel's length per shift axis; strengths = (inhibition, cross-atom inhibition); layout 'contig' or 'padded' (rows of H
padded to whole 128-byte lines, 'valid' mode only); kernels 'random' (asymmetric) or 'parabolic' (the reference's own).
"""
from collections import namedtuple

import direct_dispatch as dd
import fft_dispatch as fd
from split_dispatch import use_split_under_auto

# inhibit.hip / generic.h constants (tests/test_lateral_dispatch_cpu.py holds them to the source)
kTY, kTX, kThreads = 32, 32, 256        # inhibit.hip:17
kPre = 16                               # inhibit.hip:96   register stage: values per thread
kBatch = 8                              # inhibit.hip:147  loads per batch of the other staging form
kMaxTaps = 127                          # generic.h:5
LDS_PLAIN, LDS_MAX = 64 * 1024, 160 * 1024      # inhibit.hip:330 (attribute arm above), :317 (refused above)
PLANE_LIMIT = 1 << 31                   # inhibit.hip:319  bytes of one plane behind a buffer descriptor
BLOCKS_LIMIT = 0x7fffffff               # inhibit.hip:327
COMPILED = ((23, 23), (17, 17), (31, 31))       # inhibit.hip:337-339, the INH_LAUNCH chain; everything else runs <0, 0>
HW_ALIGN = 1 << 20                      # api.hip:115  ensure_buffer rounds the work buffer to whole MiB

MODES = ('valid', 'full', 'circular', 'reflect')
ESIZE = dd.ESIZE
cdiv = dd.cdiv

Case = namedtuple('Case', 'geometry dtype path mode taps strengths layout kernels')


def align_up(a, b):
    return cdiv(a, b) * b


def padded_ld(Hx):
    """Row stride of the row-padded activations the tests build: whole 32-element lines, one more where Hx fills its
    lines exactly (test_hip_direct_matrix.padded)."""
    return (Hx // 32 + 1) * 32


# ----------------------------------------------------------------------------------------------------------------------
# inhibit.hip: k_inhibition
# ----------------------------------------------------------------------------------------------------------------------
Inhibition = namedtuple('Inhibition', 'inst SH SW nel staging npre lds attr tiles_y tiles_x blocks remap error why')


def _inh_refused(error, why):
    return Inhibition(None, 0, 0, 0, None, 0, 0, False, 0, 0, 0, None, error, why)


def inhibition(T, n, M, rows, ld, ly, lx):
    """launch_inhibition (inhibit.hip:348-355) and launch_inhibition_t (:312-344) for n samples of M planes of
    rows x ld elements: the instance (T, LYC, LXC), the LDS tile, the staging form and the grid; where it refuses, the
    error and which guard gave it."""
    if ly < 1 or lx < 1 or ly > kMaxTaps or lx > kMaxTaps:                         # :351
        return _inh_refused('E_UNSUPPORTED', 'kMaxTaps')
    if ly % 2 == 0 or lx % 2 == 0:                                                 # :351
        return _inh_refused('E_UNSUPPORTED', 'odd')
    if n <= 0:                                                                     # :352
        return None
    ry, rx = (ly - 1) // 2, (lx - 1) // 2                                          # :314
    SH, SW = kTY + 2 * ry, (kTX + 2 * rx + 8) | 1                                  # :315 (kernel: :58)
    lds = (SH * SW + SH * (kTX + 1)) * ESIZE[T]                                    # :316
    if lds > LDS_MAX:                                                              # :317
        return _inh_refused('E_UNSUPPORTED', 'lds')
    if rows * ld * ESIZE[T] >= PLANE_LIMIT:                                        # :319
        return _inh_refused('E_UNSUPPORTED', 'plane')
    tiles_y, tiles_x = cdiv(rows, kTY), cdiv(ld, kTX)                              # :325
    blocks = n * tiles_y * tiles_x                                                 # :326
    if blocks > BLOCKS_LIMIT:                                                      # :327
        return _inh_refused('E_GEOM', 'blocks')
    inst = (T,) + ((ly, lx) if (ly, lx) in COMPILED else (0, 0))                   # :337-340
    nel = SH * SW                                                                  # :97
    staging = 'prefetch' if nel <= kPre * kThreads else 'batched'                  # :98
    npre = cdiv(nel, kThreads)                                                     # :140
    # :68-69: workgroups below the last multiple of eight are dealt to the XCDs, the rest keep their index
    remap = 'none' if blocks < 8 else ('whole' if blocks % 8 == 0 else 'tail')
    return Inhibition(inst, SH, SW, nel, staging, npre, lds, lds > LDS_PLAIN, tiles_y, tiles_x, blocks, remap, None, None)


def all_inhibition_instances():
    return {(T,) + c for T in dd.DTYPES for c in COMPILED + ((0, 0),)}


# ----------------------------------------------------------------------------------------------------------------------
# generic.hip: the reconstruction modes (launch_pad_fold, :1073-1095; pad_src / pad_dup, :1010-1026)
# ----------------------------------------------------------------------------------------------------------------------
Axis = namedtuple('Axis', 'S l dup error')


def mode_axis(d, a, mode):
    """One shift axis of a mode: activation length S, pad l = a - 1, the class of its duplicate-position table and the
    refusal of launch_pad_fold (E_GEOM).  Classes: 'l0' (one-tap atoms: nothing padded), 'full' / 'full_S1' (one
    activation) / 'full_long' (pad longer than the activations), 'circ' / 'circ_all_but_one' (l = S - 1) / 'circ_all'
    (l = S, the largest one wrap allows), 'refl' / 'refl_max' (l = S - 1, the largest a mirror without the edge allows)."""
    l = a - 1
    if mode == 'valid':
        return Axis(d + l, l, 'identity', None)
    S = d - a + 1 if mode == 'full' else d                                         # :1069-1071
    if S < 1:                                                                      # :1076
        return Axis(S, l, None, 'E_GEOM')
    if mode == 'circular' and l > S:                                               # :1079
        return Axis(S, l, None, 'E_GEOM')
    if mode == 'reflect' and l >= S:                                               # :1082
        return Axis(S, l, None, 'E_GEOM')
    if l == 0:
        return Axis(S, l, 'l0', None)
    if mode == 'full':
        return Axis(S, l, 'full_S1' if S == 1 else ('full_long' if l > S else 'full'), None)
    if mode == 'circular':
        return Axis(S, l, 'circ_all' if l == S else ('circ_all_but_one' if l == S - 1 else 'circ'), None)
    return Axis(S, l, 'refl_max' if l == S - 1 else 'refl', None)


def mode_axes(geometry, mode):
    """(y axis, x axis) of a mode; a 1-D problem is one row (its y axis: S = 1, l = 0, class 'row')."""
    g = dd.geo(geometry)
    y = Axis(1, 0, 'row', None) if g.one_d else mode_axis(g.Dy, g.Ay, mode)
    return y, mode_axis(g.Dx, g.Ax, mode)


DUP_CLASSES = {'full': ('l0', 'full', 'full_S1', 'full_long'),
               'circular': ('l0', 'circ', 'circ_all_but_one', 'circ_all'),
               'reflect': ('l0', 'refl', 'refl_max')}


# ----------------------------------------------------------------------------------------------------------------------
# api.hip: update_H_2d (:888-961)
# ----------------------------------------------------------------------------------------------------------------------
Plan = namedtuple('Plan', 'route family error why inh kernels regrow hw_bytes copied axes edges')

ROUTES = ('epilogue', 'fallback', 'modes', 'plain', 'refused')


def _taps2(geometry, taps):
    """:911-912: a 1-D problem has the x kernel only; its y kernel is the one tap 1."""
    return (1, taps[0]) if len(geometry[4]) == 1 else (taps[0], taps[1])


def family(geometry, T, path, primitive, padded):
    """Family of a primitive: direct_dispatch for its paths, the FFT family under path='fft' (api.hip:225, :250)."""
    if path == 'fft':
        assert fd.fft_has(geometry, T) and not fd.one_d(geometry), geometry
        return 'fft'
    c = dd.cell(geometry, T, path, primitive, padded)
    return c.family if c.family != 'refused' else ('refused', c.error)


def plan(case, n_call=None, terms='both', hw_bytes=0):
    """What one fused_update_H call of the backend does on n_call samples (default: all) of `case`, with the strengths
    of `terms` ('both', 'inh', 'cross' or 'none') and a work buffer of hw_bytes:

      route    'epilogue' (the lateral term inside the fused kernel of `family`), 'fallback' (unfused gradient of `family`,
               then k_mu_update_extra), 'modes' (pad -> unfused gradient -> fold-update), 'plain' ('valid' mode without
               lateral terms: the fused kernel of `family` alone) or 'refused' (error, why)
      inh      the Inhibition launch (None: no lateral term)
      kernels  the kernels of inhibit.hip / generic.hip the call runs, as instances
      regrow   the fall-back grows the work buffer and computes E a second time (api.hip:930-935)
      hw_bytes the work buffer after the call
      copied   HIP.py stepped a contiguous copy (path='mfma' answers E_STRIDE to row-padded H: _call_H)
      axes     per shift axis (S, l, duplicate class) of the mode
      edges    the edge classes of k_inhibition this call meets (INHIBITION_EDGES)"""
    geometry, T, path, mode, taps, strengths, layout, _ = case
    N, C, D, M, A = geometry
    n = N if n_call is None else n_call
    geometry = (n, C, D, M, A)
    g = dd.geo(geometry)
    es = ESIZE[T]
    inh, cross = {'both': strengths, 'inh': (strengths[0], 0.), 'cross': (0., strengths[1]), 'none': (0., 0.)}[terms]
    lateral = inh > 0 or cross > 0                                                 # :896
    ly, lx = _taps2(geometry, taps) if lateral else (1, 1)
    padded = layout == 'padded'
    assert not (padded and (mode != 'valid' or g.one_d)), 'row-padded activations: valid mode on two shift axes'
    copied = False

    def refused(error, why, hw=hw_bytes, axes=None):
        return Plan('refused', None, error, why, None, frozenset(), False, hw, copied, axes, frozenset())

    def grown(hw, want):                                                           # :111-134
        return hw if want <= hw else align_up(want, HW_ALIGN)

    if mode == 'valid':
        if padded and path == 'mfma':
            # do_reconstruct answers E_STRIDE (:235) after E has been computed; nothing of H has been written and HIP.py
            # repeats the call on a contiguous copy
            probe = inhibition(T, n, M, g.Hy, padded_ld(g.Hx), ly, lx) if lateral else None
            if probe is None or probe.error is None:
                copied, padded = True, False
                if lateral:
                    hw_bytes = grown(hw_bytes, align_up(n * M * g.Hy * padded_ld(g.Hx) * es, 256))
        Hs = padded_ld(g.Hx) if padded else g.Hx
        nE = align_up(n * M * g.Hy * Hs * es, 256)                                 # :916
        nG = align_up(n * M * g.Hy * g.Hx * es, 256)                               # :917
        launch = None
        kernels = set()
        if lateral:
            hw_bytes = grown(hw_bytes, nE)                                         # :920
            launch = inhibition(T, n, M, g.Hy, Hs, ly, lx)                         # :922
            if launch.error:
                return refused(launch.error, launch.why, hw_bytes)
            kernels.add(('k_inhibition',) + launch.inst)
        fam = family(geometry, T, path, 'reconstruct', padded)                    # :924
        if isinstance(fam, tuple):
            return refused(fam[1], 'reconstruct', hw_bytes)
        if not lateral:
            fam = family(geometry, T, path, 'update_H', padded)
            if isinstance(fam, tuple):
                return refused(fam[1], 'update_H', hw_bytes)
            return Plan('plain', fam, None, None, None, frozenset(), False, hw_bytes, copied, None, frozenset())
        # do_corr_W with the extra term (:243-269)
        route = None
        if path == 'fft':                                                          # :246
            route = 'fallback'
        elif path == 'auto' and T == 'f' and use_split_under_auto(geometry) and Hs % 32 == 0 and not g.one_d:
            route, fam = 'epilogue', 'split'                                       # :253-257, split_kernels.h:948
        elif not padded and dd.use_mfma(g, T, path, 'update_H'):                   # :259-260
            route = 'fallback'
        elif path == 'mfma':                                                       # :265-266
            route = 'fallback'
        else:                                                                      # :267-268
            if dd.generic_corr_W(g, T, True) is None:
                return refused('E_UNSUPPORTED', 'generic_corr_W', hw_bytes)
            route, fam = 'epilogue', 'generic'
        regrow = False
        if route == 'fallback':
            regrow = hw_bytes < nE + 2 * nG                                        # :930
            hw_bytes = grown(hw_bytes, nE + 2 * nG)
            fam = family(geometry, T, path, 'grad_H', padded)                     # :937
            if isinstance(fam, tuple):
                return refused(fam[1], 'grad_H', hw_bytes)
            kernels.add(('k_mu_update_extra', T))                                  # :939
        return Plan(route, fam, None, None, launch, frozenset(kernels), regrow, hw_bytes, copied, None,
                    inhibition_edges(launch, g.Hy, g.Hx, ly, lx, M, inh, cross, padded, route, regrow))

    # reconstruction modes (:942-960)
    ay, ax = axes = mode_axes(geometry, mode)
    if (not g.one_d and ay.S < 1) or ax.S < 1:                                     # :947
        return refused('E_GEOM', 'shift', axes=axes)
    Sy, Sx = ay.S, ax.S
    nP = align_up(n * M * g.Hy * g.Hx * es, 256)                                   # :948
    nE = align_up(n * M * Sy * Sx * es, 256) if lateral else 0                     # :949
    hw_bytes = grown(hw_bytes, 3 * nP + nE)                                        # :950
    if ay.error or ax.error:                                                       # :954, launch_pad_fold
        return refused('E_GEOM', 'pad', hw_bytes, axes)
    kernels = {('k_pad_H', T), ('k_fold_update', T)}                               # :954, :960
    for prim in ('reconstruct', 'grad_H'):                                         # :955, :957
        fam = family(geometry, T, path, prim, False)
        if isinstance(fam, tuple):
            return refused(fam[1], prim, hw_bytes, axes)
    launch = None
    if lateral:
        launch = inhibition(T, n, M, Sy, Sx, ly, lx)                               # :958
        if launch.error:
            return refused(launch.error, launch.why, hw_bytes, axes)
        kernels.add(('k_inhibition',) + launch.inst)
    edges = inhibition_edges(launch, Sy, Sx, ly, lx, M, inh, cross, False, 'modes', False) if lateral else frozenset()
    return Plan('modes', fam, None, None, launch, frozenset(kernels), False, hw_bytes, copied, axes, edges)


# The edge classes of k_inhibition.  Those of GEOMETRY_EDGES every instance can meet; STAGING_EDGES follow from the tap
# counts, which the compile-time instances fix (possible_edges).
GEOMETRY_EDGES = ('rows_below_32', 'rows_mod32_exact', 'rows_mod32_ragged', 'ld_mod32_exact', 'ld_mod32_ragged',
                  'remap_none', 'remap_tail', 'remap_whole', 'kernel_taller_than_plane', 'kernel_wider_than_plane',
                  'inh_only', 'cross_only', 'both_terms', 'M_1_cross_dropped', 'padded_H')
STAGING_EDGES = ('one_row', 'prefetch', 'batched', 'batched_npre_mod8_exact', 'batched_npre_mod8_ragged', 'lds_above_64K',
                 'lds_below_64K')
ROUTE_EDGES = ('epilogue', 'fallback_regrow', 'fallback_plain', 'modes')
INHIBITION_EDGES = GEOMETRY_EDGES + STAGING_EDGES


def inhibition_edges(launch, rows, cols, ly, lx, M, inh, cross, padded, route, regrow):
    e = set()
    ry, rx = (ly - 1) // 2, (lx - 1) // 2
    ld = padded_ld(cols) if padded else cols
    dd._flag(e, 'rows_below_32', rows < kTY)
    dd._flag(e, 'one_row', rows == 1 and ly == 1)
    dd._flag(e, 'rows_mod32_exact', rows % kTY == 0)
    dd._flag(e, 'rows_mod32_ragged', rows > kTY and rows % kTY != 0)
    dd._flag(e, 'ld_mod32_exact', ld % kTX == 0)
    dd._flag(e, 'ld_mod32_ragged', ld % kTX != 0)
    e.add('remap_' + launch.remap)
    dd._flag(e, 'kernel_taller_than_plane', ly > 1 and ry >= rows)
    dd._flag(e, 'kernel_wider_than_plane', rx >= cols)
    dd._flag(e, 'inh_only', inh > 0 and not cross > 0)
    dd._flag(e, 'cross_only', cross > 0 and not inh > 0 and M > 1)
    dd._flag(e, 'both_terms', inh > 0 and cross > 0 and M > 1)
    dd._flag(e, 'M_1_cross_dropped', cross > 0 and M == 1)                         # api.hip:913: xc = 0 for one atom
    dd._flag(e, 'padded_H', padded)
    e.add(launch.staging)
    if launch.staging == 'batched':
        e.add('batched_npre_mod8_exact' if launch.npre % kBatch == 0 else 'batched_npre_mod8_ragged')
    e.add('lds_above_64K' if launch.attr else 'lds_below_64K')
    e.add({'epilogue': 'epilogue', 'modes': 'modes', 'fallback': 'fallback_regrow' if regrow else 'fallback_plain'}[route])
    return frozenset(e)


def possible_edges(inst):
    """The edge classes an instance can meet at all.  The compile-time instances fix the tap counts, hence the LDS tile:
    <23, 23> and <17, 17> always prefetch, <31, 31> (62 x 71 = 4402 elements, 18 loads per thread) always stages in
    ragged batches, none of them needs more than 64 KiB in either dtype, and none has one-tap rows."""
    T, LY, LX = inst
    if (LY, LX) == (0, 0):
        return set(INHIBITION_EDGES)
    fixed = inhibition(T, 1, 1, 32, 32, LY, LX)
    staging = {fixed.staging, 'lds_above_64K' if fixed.attr else 'lds_below_64K'}
    if fixed.staging == 'batched':
        staging.add('batched_npre_mod8_exact' if fixed.npre % kBatch == 0 else 'batched_npre_mod8_ragged')
    return set(GEOMETRY_EDGES) | staging


# Instances and refusals no case can reach.
UNREACHABLE = {}

# What the matrix leaves out, with the reason (tests/test_lateral_dispatch_cpu.py checks the list is exact).
NOT_COVERED = {
    ('refusal', 'plane'): 'a plane of 2^31 bytes behind one buffer descriptor (inhibit.hip:319) is 2 GiB of activations '
                          'per atom and sample: not a test',
    ('refusal', 'blocks'): 'more than 2^31 - 1 workgroups (inhibit.hip:327) need as many 32 x 32 tiles: beyond the memory '
                           'of the device',
}

REFUSALS = ('odd', 'kMaxTaps', 'lds', 'plane', 'blocks', 'pad')

# ----------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_hip_lateral_matrix.py.  Strengths: DOMINATED cases take theirs from STRENGTHS (chosen on the
# float64 oracle so that the lateral term is at least 0.9 of every denominator -- the test measures and asserts it);
# USUAL is the project's 0.1 / 0.05.  A dominated case takes the smallest power of ten at which the oracle's smallest share,
# over random and spot operands and the three combinations of terms, reaches 0.9 (short kernels on short 1-D activations
# need the largest).
# ----------------------------------------------------------------------------------------------------------------------
USUAL = (0.1, 0.05)


def _both(name, geometry, path, mode, taps, strengths, layout='contig', kernels='random', dtypes=dd.DTYPES):
    return {f'{name}-{T}': Case(geometry, T, path, mode, taps, strengths, layout, kernels) for T in dtypes}


MATRIX = {}
for _l, _a in ((17, 9), (23, 12), (31, 16)):
    # the compile-time instances, each in both dtypes: a plane smaller than the kernel's radius with one atom (three
    # workgroups), whole tiles behind row-padded storage (eight workgroups), and the reference's own parabolic kernels
    # of an _a x _a atom on ragged tiles (twelve workgroups: eight remapped, four not)
    MATRIX.update(_both(f'c{_l}_tiny', (3, 1, (4, 5), 1, (3, 3)), 'generic', 'valid', (_l, _l), (10., 10.)))
    MATRIX.update(_both(f'c{_l}_whole', (2, 1, (60, 40), 3, (5, 6)), 'generic', 'valid', (_l, _l), (10., 10.), 'padded'))
    MATRIX.update(_both(f'c{_l}_parabolic', (3, 1, (41 - _a, 46 - _a), 4, (_a, _a)), 'generic', 'valid', (_l, _l), (10., 10.),
                        kernels='parabolic'))
# the run-time instance
MATRIX.update(_both('rt_13x9', (3, 1, (30, 41), 4, (4, 5)), 'generic', 'valid', (13, 9), (10., 10.)))
MATRIX.update(_both('rt_13x9_usual', (3, 1, (30, 41), 4, (4, 5)), 'generic', 'valid', (13, 9), USUAL))
MATRIX.update(_both('rt_9x13_padded', (4, 1, (29, 41), 4, (4, 5)), 'generic', 'valid', (9, 13), (10., 10.), 'padded'))
MATRIX.update(_both('rt_parabolic', (2, 1, (20, 30), 3, (5, 6)), 'generic', 'valid', (9, 11), (10., 10.), kernels='parabolic'))
MATRIX.update(_both('rt_tiny_m1', (2, 1, (3, 4), 1, (2, 2)), 'generic', 'valid', (11, 15), (10., 10.)))
MATRIX.update(_both('rt_1d', (2, 1, (70,), 3, (6,)), 'generic', 'valid', (11,), (100., 100.)))
MATRIX.update(_both('rt_1d_long', (9, 2, (40,), 2, (3,)), 'generic', 'valid', (127,), (10., 10.)))
MATRIX.update(_both('rt_29_batched', (2, 1, (30, 20), 3, (3, 4)), 'generic', 'valid', (29, 29), (10., 10.)))   # 17 loads
MATRIX.update(_both('rt_41x43_batched', (2, 1, (30, 20), 3, (3, 4)), 'generic', 'valid', (41, 43), (10., 10.)))  # 24 loads
MATRIX.update(_both('rt_1x63', (2, 1, (12, 70), 3, (2, 3)), 'generic', 'valid', (1, 63), (10., 10.)))
# the LDS arm: the last lengths below 64 KiB and the first above, the longest that run, the first refused
MATRIX.update(_both('lds_77', (1, 1, (20, 24), 2, (3, 3)), 'generic', 'valid', (77, 77), (10., 10.), dtypes=('f',)))
MATRIX.update(_both('lds_79', (1, 1, (20, 24), 2, (3, 3)), 'generic', 'valid', (79, 79), (10., 10.), dtypes=('f',)))
MATRIX.update(_both('lds_127', (1, 1, (20, 24), 2, (3, 3)), 'generic', 'valid', (127, 127), (10., 10.), dtypes=('f',)))
MATRIX.update(_both('lds_39', (1, 1, (20, 24), 2, (3, 3)), 'generic', 'valid', (39, 39), (10., 10.), dtypes=('d',)))
MATRIX.update(_both('lds_41', (1, 1, (20, 24), 2, (3, 3)), 'generic', 'valid', (41, 41), (10., 10.), dtypes=('d',)))
MATRIX.update(_both('lds_91', (1, 1, (20, 24), 2, (3, 3)), 'generic', 'valid', (91, 91), (10., 10.), dtypes=('d',)))
MATRIX.update(_both('lds_93_refused', (1, 1, (20, 24), 2, (3, 3)), 'generic', 'valid', (93, 93), (10., 10.), dtypes=('d',)))
MATRIX.update(_both('lds_127x75_refused', (1, 1, (20, 24), 2, (3, 3)), 'generic', 'valid', (127, 75), (10., 10.), dtypes=('d',)))
MATRIX.update(_both('taps_even_refused', (1, 1, (20, 24), 2, (3, 3)), 'generic', 'valid', (5, 4), (10., 10.)))
MATRIX.update(_both('taps_129_refused', (1, 1, (20, 24), 2, (3, 3)), 'generic', 'valid', (3, 129), (10., 10.)))
# the routes of update_H_2d: families without an epilogue for the extra term (f32 MFMA, FFT), small (the first work buffer
# holds the gradients too) and at sizes where the fall-back has to grow it and compute E again; the split kernel's epilogue
# on row-padded activations and its refusal of contiguous ones (the fall-back then takes its unfused gradient)
MATRIX.update(_both('route_mfma', (3, 1, (36, 40), 4, (5, 6)), 'mfma', 'valid', (13, 9), (10., 10.), dtypes=('f',)))
MATRIX.update(_both('route_mfma_usual', (3, 1, (36, 40), 4, (5, 6)), 'mfma', 'valid', (13, 9), USUAL, dtypes=('f',)))
MATRIX.update(_both('route_mfma_padded', (3, 1, (36, 40), 4, (5, 6)), 'mfma', 'valid', (13, 9), (10., 10.), 'padded', dtypes=('f',)))
MATRIX.update(_both('route_mfma_regrow', (4, 1, (80, 80), 8, (7, 7)), 'mfma', 'valid', (13, 9), (10., 10.), dtypes=('f',)))
MATRIX.update(_both('route_fft', (3, 1, (36, 40), 4, (5, 6)), 'fft', 'valid', (13, 9), (10., 10.)))
MATRIX.update(_both('route_fft_usual', (3, 1, (36, 40), 4, (5, 6)), 'fft', 'valid', (13, 9), USUAL))
MATRIX.update(_both('route_fft_padded', (3, 1, (36, 40), 4, (5, 6)), 'fft', 'valid', (9, 13), (10., 10.), 'padded'))
MATRIX.update({'route_fft_regrow-f': Case((4, 1, (80, 80), 8, (7, 7)), 'f', 'fft', 'valid', (13, 9), (10., 10.), 'contig', 'random'),
               'route_fft_regrow-d': Case((2, 1, (80, 80), 8, (7, 7)), 'd', 'fft', 'valid', (13, 9), (10., 10.), 'contig', 'random')})
MATRIX.update(_both('route_split_padded', (2, 1, (60, 60), 8, (12, 12)), 'auto', 'valid', (23, 23), USUAL, 'padded', 'parabolic', ('f',)))
MATRIX.update(_both('route_split_padded_dom', (2, 1, (60, 60), 8, (12, 12)), 'auto', 'valid', (13, 9), (10., 10.), 'padded', dtypes=('f',)))
MATRIX.update(_both('route_split_contig', (2, 1, (60, 60), 8, (12, 12)), 'auto', 'valid', (13, 9), (10., 10.), dtypes=('f',)))
# the reconstruction modes: the duplicate-position tables at their edges, on one and two shift axes
MATRIX.update(_both('m_full_long', (2, 1, (20, 9), 3, (12, 3)), 'generic', 'full', (7, 5), (10., 10.)))
MATRIX.update(_both('m_full_s1', (2, 1, (8, 12), 3, (8, 4)), 'generic', 'full', (7, 5), (100., 100.)))
MATRIX.update(_both('m_full_l0', (2, 2, (9, 12), 3, (1, 4)), 'generic', 'full', (7, 5), (1000., 1000.)))
MATRIX.update(_both('m_circ_max', (2, 1, (10, 13), 3, (10, 5)), 'generic', 'circular', (7, 5), (100., 100.)))
MATRIX.update(_both('m_circ_all', (2, 1, (6, 9), 3, (7, 3)), 'generic', 'circular', (5, 7), (100., 100.)))
MATRIX.update(_both('m_circ_l0', (2, 1, (9, 12), 3, (1, 5)), 'generic', 'circular', (7, 5), (100., 100.)))
MATRIX.update(_both('m_circ_usual', (3, 1, (36, 40), 4, (5, 6)), 'generic', 'circular', (13, 9), USUAL))
MATRIX.update(_both('m_refl_max', (2, 1, (10, 13), 3, (10, 5)), 'generic', 'reflect', (7, 5), (100., 100.)))
MATRIX.update(_both('m_refl_l0', (2, 1, (9, 12), 3, (4, 1)), 'generic', 'reflect', (7, 5), (100., 100.)))
MATRIX.update(_both('m_refl_mfma', (3, 1, (36, 40), 4, (5, 6)), 'mfma', 'reflect', (13, 9), (10., 10.), dtypes=('f',)))
MATRIX.update(_both('m_refl_refused', (2, 1, (10, 13), 3, (11, 5)), 'generic', 'reflect', (7, 5), (10., 10.)))
MATRIX.update(_both('m_circ_refused', (2, 1, (6, 9), 3, (8, 3)), 'generic', 'circular', (7, 5), (10., 10.)))
MATRIX.update(_both('m1_full_long', (3, 1, (20,), 3, (12,)), 'generic', 'full', (9,), (1000., 1000.)))
MATRIX.update(_both('m1_full_s1', (3, 1, (9,), 3, (9,)), 'generic', 'full', (5,), (100., 100.)))
MATRIX.update(_both('m1_circ_max', (3, 1, (14,), 3, (14,)), 'generic', 'circular', (9,), (1000., 1000.)))
MATRIX.update(_both('m1_circ_l0', (3, 2, (14,), 3, (1,)), 'generic', 'circular', (9,), (10000., 10000.)))
MATRIX.update(_both('m1_refl_max', (3, 1, (14,), 3, (14,)), 'generic', 'reflect', (9,), (1000., 1000.)))
MATRIX.update(_both('m1_refl', (3, 1, (40,), 3, (6,)), 'generic', 'reflect', (9,), (1000., 1000.)))


def n_calls(case):
    """Samples per call of the GPU test: the whole batch, and one-sample slices where the batch has them."""
    N = case.geometry[0]
    return (N,) + ((1,) if N > 1 else ())


def reached(matrix):
    """What the GPU test's calls on the cases of `matrix` reach: ({kernel instance or ('refusal', why): {edge: [case
    ids]}}).  Per case: two whole-batch steps on a fresh backend (the second on the grown work buffer), one-sample slices,
    each of them with both terms, inhibition alone and cross inhibition alone; the modes without lateral terms too."""
    out = {}

    def note(key, edge, cid):
        out.setdefault(key, {}).setdefault(edge, [])
        if cid not in out[key][edge]:
            out[key][edge].append(cid)

    for cid, case in matrix.items():
        hw = 0
        for n in (n_calls(case)[0],) + n_calls(case):          # (the first call twice)
            for terms in ('both', 'inh', 'cross') + (('none',) if case.mode != 'valid' else ()):
                p = plan(case, n, terms, hw)
                hw = p.hw_bytes
                if p.route == 'refused':
                    note(('refusal', p.why), p.error, cid)
                    continue
                for k in p.kernels:
                    note(k, 'reached', cid)
                    if k[0] == 'k_inhibition':
                        for e in p.edges:
                            note(k, e, cid)
                    if k[0] == 'k_fold_update':
                        for ax in p.axes:
                            note(k, ax.dup, cid)
                        note(k, 'lateral' if p.inh else 'no_lateral', cid)
        if case.mode != 'valid' and plan(case).why not in ('pad', 'shift'):
            note(('k_fold_H', case.dtype), 'reached', cid)      # (the unfused gradients of the mode: HIP.py _fold)
        if convolves(case):
            note(('k_convolve_axis', case.dtype), 'reached', cid)   # (be.convolve_multi_1d with the case's kernels)
    return out


def convolves(case):
    """The GPU test holds be.convolve_multi_1d (k_convolve_axis, the front end's fall-back) to the oracle with the case's
    kernels: 'valid' mode, tap counts launch_convolve_axis takes (generic.hip:988)."""
    return case.mode == 'valid' and all(t % 2 == 1 and t <= kMaxTaps for t in case.taps)


def required():
    """Every cell the matrix has to reach: (key, edge) as reached() names them."""
    need = set()
    for inst in all_inhibition_instances():
        need |= {(('k_inhibition',) + inst, e) for e in possible_edges(inst)}
    for T in dd.DTYPES:
        need |= {(('k_inhibition', T, 0, 0), r) for r in ROUTE_EDGES}
        need |= {((k, T), 'reached') for k in ('k_mu_update_extra', 'k_fold_update', 'k_pad_H', 'k_fold_H', 'k_convolve_axis')}
        need |= {(('k_fold_update', T), c) for cs in DUP_CLASSES.values() for c in cs}
        need |= {(('k_fold_update', T), c) for c in ('row', 'lateral', 'no_lateral')}
    need |= {(('refusal', why), 'E_GEOM' if why in ('blocks', 'pad') else 'E_UNSUPPORTED') for why in REFUSALS}
    return need


def missing(matrix):
    """The required cells `matrix` does not reach and NOT_COVERED does not excuse."""
    got = reached(matrix)
    return sorted((k, e) for k, e in required() if e not in got.get(k, {}) and k not in NOT_COVERED and k not in UNREACHABLE)


def sole_carriers(matrix):
    """{case id: [(key, edge), ...]}: the required cells only that case reaches."""
    out = {}
    for k, edges in reached(matrix).items():
        for e, cids in edges.items():
            if len(cids) == 1 and (k, e) in required():
                out.setdefault(cids[0], []).append((k, e))
    return out
