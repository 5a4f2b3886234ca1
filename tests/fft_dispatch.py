"""
Host mirror of the FFT kernel family's dispatch: which transform lengths a problem takes, which kernel instances
(kernel name + template arguments) each primitive launches under path='fft' and under path='hybrid' / 'auto', with which
tiles, groups and paddings -- restated in plain Python from tnmf_amd/csrc/fft.hip, fft_kernels.h, fft_mixed.hip,
fft_spectral.hip and api.hip, so that the tests can choose geometries that reach every instance and every edge of the
family (tests/test_hip_fft_matrix.py) and a CPU test can check that the choice covers them all
(tests/test_fft_dispatch_cpu.py).

A geometry is (N, C, D, M, A): samples, channels, sample shape, atoms, atom shape (1-D: one-element D and A).
dtype is 'f' (float32) or 'd' (float64); path is 'fft' or 'hybrid' ('auto' dispatches like 'hybrid' once it takes the
family at all: use_fft_under_auto()).
"""
from collections import namedtuple

NUM_CU = 256    # compute units of one MI355X (what the launchers read from ctx->num_cu)

LENS_Y = (32, 48, 64, 96, 144, 192, 270, 288, 384, 576)           # fft.hip:28  kLensY
LENS_X = (32, 48, 64, 96, 144, 192, 270, 288, 384, 540, 576)      # fft.hip:29  kLensX
F64_MAX_LEN = 288                                                 # fft.hip:35, :39; fft_len.hip:14
MIX_MAX_GROUPS = 128                                              # fft.hip:30  kMixMaxGroups
MIX_COLS = 16                                                     # fft_mixed.hip:47  kMixCols
MIX_MAX_AY = 16                                                   # fft_mixed.hip:555-560, MIX_SWITCH
MIX_W2_MAX_AY = 12                                                # fft_mixed.hip:506
MIX_GROUPS = 4                                                    # fft_mixed.hip:495  GROUPS
MIX_R_1D_MAX_C, MIX_W_1D_MAX_C = 3, 4                             # fft_mixed.hip:556, :559
MIX_STRIP_ROWS = {1: 16 * 8, 3: 8 * 8}                            # fft_mixed.hip:236, :243  S * STRIPS per CG
SPEC_CG, SPEC_NS, SPEC_MS, SPEC_THREADS = 4, 4, 4, 256            # fft_spectral.hip:16-20
WINDOW_BUDGET = 8 << 30                                           # fft.hip:109

PATHS = ('fft', 'hybrid')
DTYPES = ('f', 'd')
PRIMITIVES = ('reconstruct', 'grad_H', 'update_H', 'grad_W', 'update_W')


def cdiv(a, b):
    return -(-a // b)


def align_up(a, b):
    return cdiv(a, b) * b


def pick_len(h, dtype, along_x, tall=False):
    """fft.hip:32-41: the shortest length that holds h; float64 is instantiated up to 288; 0 when none does."""
    for L in (LENS_X if along_x or tall else LENS_Y):
        if L >= h and (dtype == 'f' or L <= F64_MAX_LEN):
            return L
    return 0


def tall_columns(path):
    """fft.hip:44: the column direction takes the x-only length (540) whenever the path cannot ask for k_fft_grad_H."""
    return path != 'fft'


class LenCfg:
    """fft_kernels.h:20-33, struct LenCfg<L>, and the per-dtype tile rules of fft_run_typed (:740, :762)."""

    def __init__(self, L):
        self.L = L
        self.col_tile = 8 if L > 384 else 16                                   # :22
        self.col_threads = 480 if L in (270, 540) else (512 if L > 192 else 256)   # :25
        assert (L * self.col_tile) % self.col_threads == 0 and (L * 16) % self.col_threads == 0   # :26
        self.col_elems = L * self.col_tile // self.col_threads                 # :27
        self.row_pairs = 8 if L > 288 else 16                                  # :28
        self.row_threads = 256                                                 # :29
        self.mu_pairs = 4 if L > 288 else 8                                    # :30
        self.mu_threads = 512 if L // 2 + 1 > 256 else 256                     # :31
        self.wide_tile = 16                                                    # :37-40  ColTile<L, true>
        self.wide_elems = L * 16 // self.col_threads

    def NB(self, dtype):
        """:740: float64 tiles of the longer transforms hold half the row pairs."""
        return self.row_pairs // 2 if dtype == 'd' and self.L > 144 else self.row_pairs

    def NBM(self, dtype):
        """:762: likewise for the fused update kernel (kFftRowsMu)."""
        return self.mu_pairs // 2 if dtype == 'd' and self.L > 144 else self.mu_pairs


def _dims(geometry):
    """(Dy, Dx, Ay, Ax, Hy, Hx) as the library's Geo holds them: a 1-D problem is one row."""
    _, _, D, _, A = geometry
    Dy, Dx, Ay, Ax = (1, D[0], 1, A[0]) if len(A) == 1 else (D[0], D[1], A[0], A[1])
    return Dy, Dx, Ay, Ax, Dy + Ay - 1, Dx + Ax - 1


def one_d(geometry):
    return _dims(geometry)[0] == 1 and _dims(geometry)[2] == 1


def mixed_has_reconstruct(geometry, dtype):
    """fft_mixed.hip:555-557."""
    C = geometry[1]
    Ay = _dims(geometry)[2]
    return dtype == 'f' and Ay <= MIX_MAX_AY and (C == 1 or (one_d(geometry) and C <= MIX_R_1D_MAX_C))


def mixed_has_grad_W(geometry, dtype):
    """fft_mixed.hip:558-560."""
    C = geometry[1]
    Ay = _dims(geometry)[2]
    return dtype == 'f' and Ay <= MIX_MAX_AY and (C == 1 or (one_d(geometry) and C <= MIX_W_1D_MAX_C))


def fft_has(geometry, dtype):
    """fft.hip:535-543: 1-D signals need both mixed forms (float32, up to three channels); 2-D ones a length per axis."""
    _, _, _, _, Hy, Hx = _dims(geometry)
    if one_d(geometry):
        return pick_len(Hx, dtype, True) != 0 and mixed_has_reconstruct(geometry, dtype) and mixed_has_grad_W(geometry, dtype)
    return pick_len(Hy, dtype, False) != 0 and pick_len(Hx, dtype, True) != 0


def use_fft_under_auto(geometry, dtype):
    """api.hip:149-155 under path='auto': float32 problems of 2^19 activations or more."""
    N, _, _, M, _ = geometry
    _, _, _, _, Hy, Hx = _dims(geometry)
    return dtype == 'f' and fft_has(geometry, dtype) and N * M * Hy * Hx >= 1 << 19


def family(geometry, dtype, path, primitive):
    """Which family a primitive runs on: 'fft', 'direct' (the H gradient and H update of 'hybrid': api.hip:250-267),
    'refused' (1-D H primitives under path='fft': fft.hip:684, :711) or None (the family does not take the problem)."""
    if not fft_has(geometry, dtype):
        return None
    if primitive in ('grad_H', 'update_H'):
        if path != 'fft':
            return 'direct'
        return 'refused' if one_d(geometry) else 'fft'
    return 'fft'


Layout = namedtuple('Layout', 'Ly Lx KX KXP resident ngroups nper chunk mgroups mper sT '
                              'sSH sS sD T SH SV VT SW TWr total_no_window total')   # (byte sizes per sample, byte offsets)


def sample_groups(N, M, tiles):
    """fft.hip:77-84 -> (ngroups, nper)."""
    ng = max(1, min(cdiv(2048, M * tiles), 16, N))
    nper = cdiv(N if N > 0 else 1, ng)
    return cdiv(N if N > 0 else 1, nper), nper


def make_layout(geometry, dtype, path, n_call=None, budget=WINDOW_BUDGET):
    """fft.hip:86-156 for a call on n_call samples (default: all) of the resident problem `geometry`."""
    N, C, _, M, _ = geometry
    n = N if n_call is None else n_call
    _, _, _, _, Hy, Hx = _dims(geometry)
    Ly = pick_len(Hy, dtype, False, tall_columns(path))                         # :87
    Lx = pick_len(Hx, dtype, True)                                              # :88
    assert Ly and Lx, geometry
    KX = Lx // 2 + 1                                                            # :92
    KXP = align_up(KX, 16)                                                      # :93
    csz = 8 if dtype == 'f' else 16                                             # :94
    tiles = cdiv(KX, 8 if Ly > 384 else 16)                                     # :95
    ngroups, nper = sample_groups(n, M, tiles)                                  # :98
    sT = M * Hy * KXP * csz                                                     # :101
    chunk_full = max(1, min(budget // (2 * sT), N))                             # :111-113
    chunk = n if chunk_full > n and n > 0 else chunk_full                       # :114
    mg = max(1, min(cdiv(1024, chunk * cdiv(KX, 16) * 2), M))                   # :115-117
    mper = cdiv(M, mg)                                                          # :118
    resident = not (mixed_has_reconstruct(geometry, dtype) and mixed_has_grad_W(geometry, dtype))   # :131
    # the workspace, in the order fft.hip takes it: sizes follow the resident sample count N, never the call's
    Dy, _, Ay, Ax, _, _ = _dims(geometry)
    Nf = N if N > 0 else 1                                                      # :100
    sSH, sS, sD = M * Ly * KXP * csz, C * Ly * KXP * csz, C * Dy * KXP * csz    # :102-104
    nSW = M * C * Ly * KXP * csz                                                # :120
    at = [0]

    def take(nbytes):                                                           # :122-126
        o = at[0]
        at[0] += align_up(nbytes, 256)
        return o

    T = take(Nf * sT + 64 * KXP * csz)                                          # :128
    SH = take(Nf * sSH if resident else 0)                                      # :132
    SV = take(Nf * sS)                                                          # :133
    take(Nf * sS)                                                               # :134  SR
    take(Nf * sD)                                                               # :135  Ts
    VT = take(Nf * sD)                                                          # :136
    take(Nf * sD)                                                               # :137  RT
    SW = take(nSW)                                                              # :138
    take(nSW)                                                                   # :139  SWf
    take(2 * M * C * Ay * KXP * csz)                                            # :140  TW
    TWr = take(M * C * Ay * KXP * csz)                                          # :141
    take(2 * M * C * Ay * Ax * (csz // 2))                                      # :142  Wt
    nG = max(nSW * sample_groups(N, M, tiles)[0], MIX_MAX_GROUPS * M * C * Ay * KXP * csz)   # :145
    take(nG)                                                                    # :146  Gn
    take(nG)                                                                    # :147  Gp
    take(nSW * 2)                                                               # :148  Gs
    take(2 * M * C * Ay * Ax * (csz // 2))                                      # :149  Wo
    total_no_window = at[0]                                                     # :150
    take(chunk_full * sT)                                                       # :152  Tn
    take(chunk_full * sT)                                                       # :153  Tp
    return Layout(Ly, Lx, KX, KXP, resident, ngroups, nper, chunk, cdiv(M, mper), mper, sT,
                  sSH, sS, sD, T, SH, SV, VT, SW, TWr, total_no_window, at[0])


def mix_groups(N, C, M, Ay, KX, num_cu=NUM_CU):
    """fft.hip:748-767 and :782-788 -> (ng, nper, ngpad) of the mixed W gradient."""
    slots = 2 * 4 * num_cu                                                      # :749
    per_group_block = (cdiv(M, 2) if C == 1 and Ay <= 12 else M) * cdiv(KX, 16)   # :750
    best, best_cost = 32, 1e30
    cand = 32
    while cand <= MIX_MAX_GROUPS:                                               # :753
        ng = min(N, cand)
        ng = cdiv(N, cdiv(N, ng))
        rounds = per_group_block * cdiv(ng, 4) / slots                          # :757
        whole = 1.0 if rounds <= 1.0 else float(int(rounds + 0.999999))         # :758
        cost = whole / rounds + 0.03 * (cand // 32)                             # :760
        if cost < best_cost - 1e-9:
            best, best_cost = cand, cost
        cand *= 2
    ng = min(N, best)                                                           # :785
    nper = cdiv(N, ng)                                                          # :786
    ng = cdiv(N, nper)                                                          # :787
    return ng, nper, align_up(ng, 4)                                            # :788


def mix_span(nper, M, Hy, KXP):
    """fft_mixed.hip:509: the largest per-lane byte offset of k_mix_grad_W2; it must stay below 2^31 (:510)."""
    return ((MIX_GROUPS - 1) * nper * M + 2) * Hy * KXP * 8


def spectral_groups(N, C, M, Ly, KXP, ngroups_layout, num_cu=NUM_CU):
    """fft.hip:805-809 -> (ngroups, nper) of the resident-spectrum W gradient."""
    blocks = cdiv(M, 4) * cdiv(Ly * KXP, 256) * cdiv(C, 4)
    ng = max(1, min(cdiv(8 * num_cu, blocks), ngroups_layout))
    nper = cdiv(N, ng)
    return cdiv(N, nper), nper


def grad_H_class(C):
    """fft_kernels.h:788-792: CH = C for one to four channels (held in registers), 0 for more (reloaded per atom)."""
    return C if C <= 4 else 0


def contract_R_cg(C):
    """fft_kernels.h:779 (k_fft_contract_R, diagnostic builds only)."""
    return C if C <= 3 else 4


def grad_W_cg(C, L):
    """fft_kernels.h:796 (k_fft_grad_W, diagnostic builds only)."""
    return C if C <= 2 else (3 if LenCfg(L).col_elems <= 9 else 2)


def spectral_cg(C):
    """fft_spectral.hip:128, :156."""
    return min(C, SPEC_CG)


# ---- what a call launches ------------------------------------------------------------------------------------------------
# An instance is a tuple: the kernel name followed by its template arguments, dtype first.

def _prev_len(L, lens):
    i = lens.index(L)
    return lens[i - 1] if i else 0


def _fit_edges(axis, H, L, lens):
    """exact fit (no zero padding: a linear convolution computed circularly is one off from wrapping round), one short,
    and the smallest H that still picks this length (lengths above the shortest)."""
    out = set()
    if H == L:
        out.add(axis + '_exact')
    if H == L - 1:
        out.add(axis + '_one_short')
    if H == _prev_len(L, lens) + 1 and L != lens[0]:
        out.add(axis + '_min')
    return out


class _Cells(dict):
    def hit(self, inst, *edges):
        self.setdefault(inst, set()).update(e for e in edges if e)


def _row_launch(out, kernel, dtype, Lx, planes, rows, edges, NB=None):
    """One launch of a row kernel on [planes][rows] real rows: fft_kernels.h:749-755 (planes of one row are handed over as
    the rows of one plane), tiles of 2 NB rows (two real rows = one complex sequence)."""
    cfg = LenCfg(Lx)
    nb = cfg.NB(dtype) if NB is None else NB
    if kernel in ('k_fft_rows_fwd', 'k_fft_rows_inv') and rows == 1 and planes > 1:   # :749
        rows, planes = planes, 1
    out.hit((kernel, dtype, Lx), 'odd_rows' if rows % 2 else None, 'row_tile_partial' if rows % (2 * nb) else None,
            'row_tiles_several' if rows > 2 * nb else None, *edges)


def cells(geometry, dtype, path, primitives=PRIMITIVES, n_call=None, num_cu=NUM_CU):
    """{instance: edge classes met} for the primitives of one backend on `geometry` (n_call: samples of a mini-batch
    slice).  Empty when the family does not take the problem.  Edge classes:

      x_exact, x_one_short, x_min / y_...   H == L, H == L - 1, H == (next shorter length) + 1 on the axis the kernel
                                            transforms (mixed and spectral kernels: the axes of the transforms around them)
      kx_tail_16, kx_tail_8                 a partial last tile of kx columns (KX = L/2 + 1 never fills 16- or 8-wide tiles)
      odd_rows, row_tile_partial, row_tiles_several   row kernels: the pair packing with a last single row, a last tile that
                                            is partly empty, more than one tile per plane
      M_odd                                 k_mix_grad_W2: the second atom of the last block repeats the first
      M_mod4, N_mod4, C_mod4, C_gt4         spectral kernels: partial atom quads / sample quads / channel groups, several groups
      C_gt4 on k_fft_grad_H                 the CH = 0 class
      nper_tail, ngpad                      W gradients: N not a multiple of nper; padding groups that must write zeros
      mper_tail                             k_fft_grad_H: M not a multiple of mper
      rows_tail                             k_mix_grad_W / k_mix_grad_W2: Dy not a multiple of the row block (AY rows / one ring
                                            period): the rows past the data must contribute nothing
      strip_tail, strip_blocks              k_mix_reconstruct: Dy not a multiple of the strip block (128 rows), several blocks
      slice_last, slice_interior            a mini-batch slice can be the last sample / an interior one (N >= 3)
    """
    out = _Cells()
    N, C, _, M, _ = geometry
    if not fft_has(geometry, dtype):
        return out
    n = N if n_call is None else n_call
    Dy, Dx, Ay, Ax, Hy, Hx = _dims(geometry)
    l = make_layout(geometry, dtype, path, n_call)
    cx, cy = LenCfg(l.Lx), LenCfg(l.Ly)
    T = dtype
    d1 = one_d(geometry)
    xfit = _fit_edges('x', Hx, l.Lx, LENS_X)
    yfit = _fit_edges('y', Hy, l.Ly, LENS_X if tall_columns(path) else LENS_Y)
    sl = {'slice_last', 'slice_interior'} if N >= 3 else set()
    kx16 = 'kx_tail_16' if l.KX % 16 else None
    mixed_R, mixed_W = mixed_has_reconstruct(geometry, dtype), mixed_has_grad_W(geometry, dtype)

    def rows(kernel, planes, nrows, NB=None):
        _row_launch(out, kernel, T, l.Lx, planes, nrows, xfit | sl, NB)

    def cols(kernel):
        out.hit((kernel, T, l.Ly), 'kx_tail_%d' % cy.col_tile if l.KX % cy.col_tile else None, *(yfit | sl))

    def spectra_W():                                                            # fft.hip:319-335
        out.hit(('k_fft_prep_W', T))
        rows('k_fft_rows_fwd', M * C, Ay)
        cols('k_fft_cols_fwd')

    def spectra_of_H():                                                         # fft.hip:523-531
        rows('k_fft_rows_fwd', n * M, Hy)
        cols('k_fft_cols_fwd')

    def planes_VR(full):                                                        # fft.hip:468-493, :273-291
        rows('k_fft_rows_fwd', n * C, Dy)
        if full:
            cols('k_fft_cols_fwd')

    for prim in primitives:
        if family(geometry, dtype, path, prim) != 'fft':
            continue
        if prim in ('reconstruct', 'update_H', 'update_W'):                     # every fused step reconstructs first
            rows('k_fft_rows_fwd', n * M, Hy)                                   # rows_of_H, fft.hip:597
            if mixed_R:                                                         # fft.hip:608-616
                out.hit(('k_fft_prep_W', T))
                rows('k_fft_rows_fwd', M * C, Ay)
                if d1:                                                          # fft_mixed.hip:226-233
                    out.hit(('k_mix_reconstruct_1d', T, 3, 16), kx16, *(xfit | sl), 'row_tile_partial' if n % 16 else None)
                else:                                                           # :235-239 (C == 1: CG = 1, S = 16)
                    blk = MIX_STRIP_ROWS[1]
                    out.hit(('k_mix_reconstruct', T, Ay, 1, 16, 8), kx16, *(xfit | sl),
                            'strip_tail' if Dy % blk else None, 'strip_blocks' if Dy > blk else None)
            else:                                                               # fft.hip:617-640
                spectra_W()
                spectra_of_H()
                out.hit(('k_spec_contract_R', T, spectral_cg(C)), *(xfit | yfit | sl), 'N_mod4' if n % SPEC_NS else None,
                        'C_mod4' if C % SPEC_CG else None, 'C_gt4' if C > SPEC_CG else None)
                cols('k_fft_cols_inv')
            rows('k_fft_rows_inv', n * C, Dy)                                   # fft.hip:641-651
        if prim in ('grad_H', 'update_H'):                                      # fft.hip:657-662, :682-742
            spectra_W()
            planes_VR(True)
            planes_VR(True)
            assert l.chunk >= n, 'the window loop (chunk < N) is NOT_COVERED: no geometry of a test may need it'
            out.hit(('k_fft_grad_H', T, l.Ly, grad_H_class(C)), kx16, *(yfit | sl),
                    'mper_tail' if M % l.mper else None, 'C_gt4' if C > 4 else None)
            if prim == 'grad_H':
                rows('k_fft_rows_inv2', n * M, Hy)
            else:
                rows('k_fft_rows_mu', n * M, Hy, cx.NBM(T))
        if prim in ('grad_W', 'update_W'):                                      # fft.hip:769-873
            rows('k_fft_rows_fwd', n * M, Hy)
            if mixed_W:
                planes_VR(False)
                planes_VR(False)
                ng, nper, ngpad = mix_groups(n, C, M, Ay, l.KX, num_cu)
                edges = [kx16, 'nper_tail' if n % nper else None, 'ngpad' if ngpad > ng else None, *(xfit | sl)]
                if d1:                                                          # fft_mixed.hip:497-504
                    out.hit(('k_mix_grad_W_1d', T, 4, MIX_GROUPS), *edges)
                elif Ay <= MIX_W2_MAX_AY and C == 1 and mix_span(nper, M, Hy, l.KXP) < 1 << 31:   # :506-517
                    ring = (Ay + 4 + 7) // 8 * 8                                # :348  RS: rows per period of the rings
                    out.hit(('k_mix_grad_W2', T, Ay, MIX_GROUPS), 'M_odd' if M % 2 else None,
                            'rows_tail' if Dy % ring else None, *edges)
                else:                                                           # :519-522 (rows in blocks of AY: :292)
                    out.hit(('k_mix_grad_W', T, Ay, 1, MIX_GROUPS), 'rows_tail' if Dy % Ay else None, *edges)
                out.hit(('k_fft_sum_groups', 'f'))                              # fft.hip:792
            else:
                planes_VR(True)
                planes_VR(True)
                spectra_of_H()
                ngroups, nper = spectral_groups(n, C, M, l.Ly, l.KXP, l.ngroups, num_cu)
                out.hit(('k_spec_grad_W', T, spectral_cg(C)), *(xfit | yfit | sl), 'M_mod4' if M % SPEC_MS else None,
                        'C_mod4' if C % SPEC_CG else None, 'C_gt4' if C > SPEC_CG else None,
                        'nper_tail' if n % nper else None)
                out.hit(('k_fft_sum_groups', T))
                cols('k_fft_cols_inv')
            rows('k_fft_rows_inv', 2 * M * C, Ay)                               # fft.hip:848-857
            out.hit(('k_fft_flip_out', T))
    return out


# ---- the universe of instances -------------------------------------------------------------------------------------------

ROW_KERNELS = ('k_fft_rows_fwd', 'k_fft_rows_inv', 'k_fft_rows_inv2', 'k_fft_rows_mu')
COL_KERNELS = ('k_fft_cols_fwd', 'k_fft_cols_inv')
GRAD_H_CLASSES = (1, 2, 3, 4, 0)


def lens_of(dtype, lens):
    return tuple(L for L in lens if dtype == 'f' or L <= F64_MAX_LEN)


def _diag_contract_R():
    return {('k_fft_contract_R', T, L, cg) for T in DTYPES for L in lens_of(T, LENS_X) for cg in (1, 2, 3, 4)}


def _diag_grad_W():
    return {('k_fft_grad_W', T, L, cg) for T in DTYPES for L in lens_of(T, LENS_X) for cg in (1, 2, 3)
            if cg <= 2 or cg == grad_W_cg(3, L)}


def _none():
    return set()


# Instances (and launch parameters) the product build cannot run: every launch site sits behind a tnmf_diag_env() read,
# which common.h compiles to "unset" unless the library is built with -DTNMF_DIAG.  `guard` names the function of fft.hip
# whose tnmf_diag_env read decides; tests/test_fft_dispatch_cpu.py checks both from the source text.
UNREACHABLE = {
    'k_fft_contract_R': dict(
        instances=_diag_contract_R, op='kFftContractR', guard='use_resident', env='TNMF_FFT_NO_RESIDENT',
        reason='launched from the else branch of `if (use_resident(l))` in fft_reconstruct; that branch is entered only when '
               'the mixed reconstruct does not take the problem, and then Lay::resident is true: use_resident() is false '
               'only when TNMF_FFT_NO_RESIDENT is read'),
    'k_fft_grad_W': dict(
        instances=_diag_grad_W, op='kFftGradW', guard='use_resident', env='TNMF_FFT_NO_RESIDENT',
        reason='likewise in fft_grad_W: the column-transform W gradient runs only when use_resident() is switched off'),
    'forced_mix_groups': dict(
        instances=_none, op=None, guard='fft_grad_W', env='TNMF_MIX_GROUPS',
        reason='a group count of the mixed W gradient other than the one mix_groups() computes'),
    'forced_no_mixed': dict(
        instances=_none, op=None, guard='use_mixed', env='TNMF_FFT_NO_MIXED',
        reason='one-channel float32 problems with atoms of up to 16 rows on the resident-spectrum kernels (the kernels '
               'themselves are reached with taller atoms and with several channels)'),
}

# Reachable in the product build, but only at sizes no test of this suite runs.  Nothing else belongs here.
NOT_COVERED = {
    'h_update_window_loop': dict(
        instances=_none,
        reason='fft_grad_H / fft_update_H walk the samples in windows of Lay::chunk (fft.hip:690, :723); chunk < N needs more '
               'than 8 GB of gradient row spectra (2 * N * M * Hy * KXP * 8 bytes), and the budget can be lowered only '
               'through TNMF_FFT_WINDOW_MB in the diagnostic build'),
    'mix_grad_W_span_fallback': dict(
        instances=lambda: {('k_mix_grad_W', 'f', ay, 1, MIX_GROUPS) for ay in range(1, MIX_W2_MAX_AY + 1)},
        reason='launch_mix_grad_W (fft_mixed.hip:509-510) falls back to the single-atom kernel for atoms of up to 12 rows '
               'when the per-lane offsets of k_mix_grad_W2 would pass 2^31 bytes: (3 * nper * M + 2) * Hy * KXP * 8, i.e. '
               'nper * M >= 511 at Hy = 576, KXP = 304 -- tens of GB of activations'),
}

# Compiled, but no launch site of ANY build can select them: findings of the mirror, reported in DESIGN.md; not part of
# the universe (there is nothing to run).
COMPILED_NOT_DISPATCHED = {
    'k_fft_grad_H<T, 540, 480, CH>': 'a column length of 540 is picked only when path != fft (tall_columns) and '
                                     'k_fft_grad_H runs only when path == fft',
    'k_mix_reconstruct<T, AY, 3, 8, 8>': 'the three-channel 2-D form of launch_mix_reconstruct (fft_mixed.hip:240-247): '
                                         'mixed_has_reconstruct admits several channels for 1-D signals only, which take '
                                         'k_mix_reconstruct_1d',
    'k_mix_grad_W<T, AY <= 12, 1, 4> with C > 1': 'the C != 1 way into the single-atom kernel (fft_mixed.hip:510): '
                                                  'mixed_has_grad_W admits several channels for 1-D signals only, which '
                                                  'take k_mix_grad_W_1d',
}


def universe():
    """Every kernel instance a launch site of the sources can select: kernel x length x dtype x template class.
    Row kernels take the lengths of kLensX; the plain column kernels those of kLensY and, under every path but 'fft',
    540 as well (tall_columns); k_fft_grad_H runs under path='fft' alone, hence on kLensY."""
    out = set()
    for T in DTYPES:
        for L in lens_of(T, LENS_X):
            out.update((k, T, L) for k in ROW_KERNELS)
            out.update((k, T, L) for k in COL_KERNELS)          # (kLensX is kLensY plus 540)
        for L in lens_of(T, LENS_Y):
            out.update(('k_fft_grad_H', T, L, ch) for ch in GRAD_H_CLASSES)
        for cg in range(1, SPEC_CG + 1):
            out.update({('k_spec_contract_R', T, cg), ('k_spec_grad_W', T, cg)})
        out.update({('k_fft_prep_W', T), ('k_fft_sum_groups', T), ('k_fft_flip_out', T)})
    for ay in range(1, MIX_MAX_AY + 1):                         # MIX_SWITCH: float only
        out.add(('k_mix_reconstruct', 'f', ay, 1, 16, 8))
        out.add(('k_mix_grad_W2', 'f', ay, MIX_GROUPS) if ay <= MIX_W2_MAX_AY else ('k_mix_grad_W', 'f', ay, 1, MIX_GROUPS))
    out.update({('k_mix_reconstruct_1d', 'f', 3, 16), ('k_mix_grad_W_1d', 'f', 4, MIX_GROUPS)})
    for ent in list(UNREACHABLE.values()) + list(NOT_COVERED.values()):
        out.update(ent['instances']())
    return out


def excused():
    out = set()
    for ent in list(UNREACHABLE.values()) + list(NOT_COVERED.values()):
        out.update(ent['instances']())
    return out


def reached(matrix, paths=PATHS, dtypes=DTYPES):
    """{instance: edge classes} over a dict of geometries, both dtypes and both paths; whole batch and a one-sample slice
    (the calls of tests/test_hip_fft_matrix.py)."""
    out = _Cells()
    for g in matrix.values():
        for T in dtypes:
            for p in paths:
                for n_call in (None, 1):
                    for inst, edges in cells(g, T, p, n_call=n_call).items():
                        out.hit(inst, *edges)
    return out


# Which edge classes apply to which kernel (tests/test_fft_dispatch_cpu.py requires each to be met in each dtype the kernel
# has; the fit edges besides on every transform length, see there).
_FIT_X = ('x_exact', 'x_one_short', 'x_min')
_FIT_Y = ('y_exact', 'y_one_short', 'y_min')
_SLICES = ('slice_last', 'slice_interior')
_ROWS = _FIT_X + _SLICES + ('odd_rows', 'row_tile_partial', 'row_tiles_several')
EDGES = {
    'k_fft_rows_fwd': _ROWS, 'k_fft_rows_inv': _ROWS, 'k_fft_rows_inv2': _ROWS, 'k_fft_rows_mu': _ROWS,
    'k_fft_cols_fwd': _FIT_Y + _SLICES + ('kx_tail_16', 'kx_tail_8'),
    'k_fft_cols_inv': _FIT_Y + _SLICES + ('kx_tail_16', 'kx_tail_8'),
    'k_fft_grad_H': _FIT_Y + _SLICES + ('kx_tail_16', 'mper_tail', 'C_gt4'),
    'k_spec_contract_R': _FIT_X + _FIT_Y + _SLICES + ('N_mod4', 'C_mod4', 'C_gt4'),
    'k_spec_grad_W': _FIT_X + _FIT_Y + _SLICES + ('M_mod4', 'C_mod4', 'C_gt4', 'nper_tail'),
    'k_mix_reconstruct': _FIT_X + _SLICES + ('kx_tail_16', 'strip_tail', 'strip_blocks'),
    'k_mix_reconstruct_1d': _FIT_X + _SLICES + ('kx_tail_16', 'row_tile_partial'),
    'k_mix_grad_W2': _FIT_X + _SLICES + ('kx_tail_16', 'M_odd', 'nper_tail', 'ngpad', 'rows_tail'),
    'k_mix_grad_W': _FIT_X + _SLICES + ('kx_tail_16', 'nper_tail', 'ngpad', 'rows_tail'),
    'k_mix_grad_W_1d': _FIT_X + _SLICES + ('kx_tail_16', 'nper_tail', 'ngpad'),
    'k_fft_prep_W': (), 'k_fft_sum_groups': (), 'k_fft_flip_out': (),
}


# The geometries of tests/test_hip_fft_matrix.py: (N, C, D, M, A).  The grid y<Ly>_c<C>_x<Lx> crosses every column length
# with every channel class of k_fft_grad_H (C = 1, 2, 3, 4 and more) and walks the row lengths through exact fit, one
# short and the shortest row that picks the length; the column lengths likewise down each row of the grid (C = 2: exact,
# 3: one short, 4: shortest).  Rows up to 288 also run in float64; 385 <= Hy <= 540 takes 576 under path='fft' and 540
# under 'hybrid'.  The one-channel geometries walk the atom heights 1..16 of the mixed kernels.
MATRIX = {
    'y32_c1_x288':    (3, 1, (5, 270), 3, (13, 2)),
    'y32_c2_x288':    (3, 2, (26, 285), 19, (7, 3)),
    'y32_c3_x288':    (3, 3, (20, 285), 5, (12, 4)),
    'y32_c4_x270':    (3, 4, (13, 189), 6, (17, 5)),
    'y32_c5_x270':    (3, 5, (16, 264), 7, (3, 6)),
    'y48_c1_x270':    (3, 1, (27, 264), 8, (14, 7)),
    'y48_c2_x192':    (3, 2, (36, 138), 3, (13, 8)),
    'y48_c3_x192':    (3, 3, (30, 190), 4, (18, 2)),
    'y48_c4_x192':    (3, 4, (30, 190), 5, (4, 3)),
    'y48_c6_x144':    (3, 6, (34, 94), 6, (9, 4)),
    'y64_c1_x144':    (3, 1, (43, 139), 7, (15, 5)),
    'y64_c2_x144':    (3, 2, (46, 139), 8, (19, 6)),
    'y64_c3_x96':     (3, 3, (59, 59), 3, (5, 7)),
    'y64_c4_x96':     (3, 4, (40, 88), 4, (10, 8)),
    'y64_c5_x96':     (3, 5, (44, 95), 5, (15, 2)),
    'y96_c1_x64':     (3, 1, (81, 47), 6, (1, 3)),
    'y96_c2_x64':     (3, 2, (91, 60), 7, (6, 4)),
    'y96_c3_x64':     (3, 3, (85, 60), 8, (11, 5)),
    'y96_c4_x48':     (3, 4, (50, 28), 3, (16, 6)),
    'y96_c5_x48':     (3, 5, (81, 41), 4, (2, 7)),
    'y144_c1_x48':    (3, 1, (119, 41), 5, (2, 8)),
    'y144_c2_x32':    (3, 2, (133, 30), 6, (12, 2)),
    'y144_c3_x32':    (3, 3, (127, 30), 7, (17, 3)),
    'y144_c4_x32':    (3, 4, (95, 24), 8, (3, 4)),
    'y144_c5_x32':    (3, 5, (115, 24), 3, (8, 5)),
    'y192_c1_x32':    (3, 1, (167, 24), 4, (3, 6)),
    'y192_c2_x32':    (3, 2, (175, 11), 5, (18, 7)),
    'y192_c3_x32':    (3, 3, (188, 11), 6, (4, 8)),
    'y192_c4_x32':    (3, 4, (137, 18), 7, (9, 2)),
    'y192_c6_x32':    (3, 6, (157, 18), 8, (14, 3)),
    'y270_c1_x32':    (3, 1, (228, 18), 3, (4, 4)),
    'y270_c2_x32':    (3, 2, (266, 18), 4, (5, 5)),
    'y270_c3_x32':    (3, 3, (260, 18), 5, (10, 6)),
    'y270_c4_x32':    (3, 4, (179, 18), 6, (15, 7)),
    'y270_c5_x32':    (3, 5, (213, 18), 7, (20, 8)),
    'y288_c1_x32':    (3, 1, (275, 25), 8, (5, 2)),
    'y288_c2_x32':    (3, 2, (278, 25), 3, (11, 3)),
    'y288_c3_x32':    (3, 3, (272, 25), 4, (16, 4)),
    'y288_c4_x32':    (3, 4, (270, 25), 5, (2, 5)),
    'y288_c5_x32':    (3, 5, (274, 12), 6, (7, 6)),
    'y384_c1_x384':   (3, 1, (332, 378), 3, (6, 7)),
    'y384_c2_x384':   (3, 2, (368, 376), 4, (17, 8)),
    'y384_c3_x384':   (3, 3, (381, 288), 3, (3, 2)),
    'y384_c4_x540':   (3, 4, (282, 538), 4, (8, 3)),
    'y384_c5_x540':   (3, 5, (326, 536), 3, (13, 4)),
    'y576_c1_x540':   (3, 1, (554, 381), 4, (7, 5)),
    'y576_c2_x576':   (3, 2, (573, 571), 3, (4, 6)),
    'y576_c3_x576':   (3, 3, (567, 569), 4, (9, 7)),
    'y576_c4_x576':   (3, 4, (372, 534), 3, (14, 8)),
    'y576_c5_x32':    (3, 5, (522, 26), 4, (19, 2)),
    'y576_c2b_x32':   (3, 2, (535, 26), 3, (5, 3)),
    'mix_a8_strips':  (3, 1, (150, 20), 5, (8, 5)),   # two strip blocks, the second partial
    'mix_a9_n129':    (129, 1, (12, 20), 3, (9, 4)),   # nper = 2: N % nper != 0 (two-atom kernel)
    'mix_a10':        (3, 1, (130, 9), 4, (10, 3)),   # a second strip block of two rows
    'mix_a11':        (3, 1, (20, 39), 7, (11, 9)),   # Hx = 47: one short of 48
    'mix_a12':        (3, 1, (30, 21), 6, (12, 12)),
    'mix_a16_n129':   (129, 1, (10, 14), 3, (16, 3)),   # single-atom kernel with nper = 2
    'tall_atoms_c1':  (3, 1, (30, 25), 5, (20, 6)),   # atoms taller than 16 rows: spectral kernels with one channel
    'spec_n35_c2':    (35, 2, (10, 12), 3, (4, 5)),   # spectral W gradient: nper = 3, N % nper != 0
    'd1_c1':          (3, 1, (90,), 5, (7,)),   # Hx = 96: exact
    'd1_c2':          (19, 2, (180,), 4, (12,)),   # Hx = 191
    'd1_c3':          (129, 3, (270,), 3, (20,)),   # Hx = 289: the shortest row that takes 384; nper = 2
}


def _length_of(inst):
    """The transform length in an instance of a per-length kernel, else None."""
    return inst[2] if inst[0] in ROW_KERNELS + COL_KERNELS + ('k_fft_grad_H',) else None


def coverage_gaps(matrix):
    """What `matrix` does not reach, as a sorted list of strings (empty: complete):
      * instances of universe() - excused();
      * per kernel and dtype, the edge classes of EDGES (kx_tail_8 in float32 only: the 8-wide tiles belong to 540 and 576);
      * per kernel, dtype and transform length, the three fit edges on the axis the kernel transforms (no 'min' at 32);
      * rows_tail on every atom height of the mixed W-gradient kernels."""
    got = reached(matrix)
    want = universe() - excused()
    gaps = ['instance %r' % (i,) for i in want - set(got)] + ['not in the universe %r' % (i,) for i in set(got) - want]
    for kernel, edges in EDGES.items():
        for T in DTYPES:
            insts = [i for i in want if i[0] == kernel and i[1] == T]
            if not insts:
                continue
            met = set().union(*(got.get(i, set()) for i in insts))
            gaps += ['edge %s on %s<%s>' % (e, kernel, T) for e in edges
                     if e not in met and not (e == 'kx_tail_8' and T == 'd')]
            axis = 'x' if kernel in ROW_KERNELS else 'y'
            for L in sorted({_length_of(i) for i in insts} - {None}):
                met = set().union(*(got.get(i, set()) for i in insts if _length_of(i) == L))
                gaps += ['edge %s_%s on %s<%s, %d>' % (axis, e, kernel, T, L) for e in ('exact', 'one_short', 'min')
                         if axis + '_' + e not in met and not (e == 'min' and L == LENS_X[0])]
    for inst in want:                    # every atom height is its own unrolled row loop
        if inst[0] in ('k_mix_grad_W', 'k_mix_grad_W2') and inst in got and 'rows_tail' not in got[inst]:
            gaps.append('edge rows_tail on %r' % (inst,))
    return sorted(gaps)
