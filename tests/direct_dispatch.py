"""
Host mirror of the dispatch of the direct kernels: which kernel of tnmf_amd/csrc/mfma.hip (float32 on the matrix cores)
or tnmf_amd/csrc/generic.hip (both dtypes, any shape) runs a primitive, with which template arguments, how much LDS and
how many workgroups -- restated in plain Python from api.hip, mfma.hip and generic.hip, so that the tests can choose
geometries that reach every instance and every edge of every kernel (tests/test_hip_direct_matrix.py) and a CPU test can
check that the choice covers them all (tests/test_direct_dispatch_cpu.py).

A geometry is (N, C, D, M, A): samples, channels, sample shape, atoms, atom shape (1-D: one-element D and A).  A dtype
is 'f' (float32) or 'd' (float64).  Names: in the library corr_W is the correlation WITH W -- the H gradient ('grad_H')
and the fused H update ('update_H'); corr_H is the W gradient ('grad_W').
"""
from collections import namedtuple

from fft_dispatch import use_fft_under_auto
from split_dispatch import use_split_under_auto

NUM_CU = 256    # compute units of one MI355X (ctx->num_cu; mfma_has_corr_H plans with 256 whatever the device)
kBlock = 256    # mfma.hip:25, generic.hip:14

DTYPES = ('f', 'd')
PATHS = ('mfma', 'generic', 'auto')
PRIMITIVES = ('reconstruct', 'grad_H', 'update_H', 'grad_W')
ESIZE = {'f': 4, 'd': 8}

# mfma.hip constants the plans use (tests/test_direct_dispatch_cpu.py holds them to the source)
CW_TY, CW_TX, CW_RB, CW_XSTR = 16, 32, 4, 64      # :75
CP_TY, CP_RB, CP_XE4 = 8, 2, 3                    # :228
CH_RH = 4                                         # :522
RC_RBK = 4                                        # :759
# generic.hip
kSmallTY, kSmallTX, kSmallQ = 2, 32, 4            # :176
kMaxShiftsPerThread = 4                           # :361

# The contraction lengths the project's bars (2e-5 / 1e-10 of the output's maximum) were stated for and are held at by
# test_matrix_core_kernels_at_baseline_sizes: C*Ay*Ax of the H gradient, M*Ay*Ax of reconstruct, the N*Dy*Dx pixels of
# the W gradient (512 x 512, summed in chunks of at most 32K float32 terms, then in double).
K_HELD = {'grad_H': 768, 'update_H': 768, 'reconstruct': 16384, 'grad_W': 512 * 512}

Geo = namedtuple('Geo', 'N C Dy Dx Ay Ax M Hy Hx one_d')


def cdiv(a, b):
    return -(-a // b)


def geo(geometry):
    """api.hip:22-44, to_geo: a 1-D problem is one row."""
    N, C, D, M, A = geometry
    Dy, Dx, Ay, Ax = (1, D[0], 1, A[0]) if len(A) == 1 else (D[0], D[1], A[0], A[1])
    return Geo(N, C, Dy, Dx, Ay, Ax, M, Dy + Ay - 1, Dx + Ax - 1, len(A) == 1)


def contraction(geometry, primitive):
    """Terms of one output element's sum."""
    g = geo(geometry)
    return {'grad_H': g.C * g.Ay * g.Ax, 'update_H': g.C * g.Ay * g.Ax, 'reconstruct': g.M * g.Ay * g.Ax,
            'grad_W': g.N * g.Dy * g.Dx}[primitive]


# ----------------------------------------------------------------------------------------------------------------------
# mfma.hip
# ----------------------------------------------------------------------------------------------------------------------
def mfma_common(g, T):
    """mfma.hip:1127-1132."""
    if T != 'f':
        return False
    if g.Dy == 1 or g.Ay == 1:          # 1-D signals run on the generic kernels
        return False
    return g.Ax <= 32 and g.Ay <= 32


def mfma_has_reconstruct(g, T, hx_guard=True):
    """mfma.hip:1134-1138.  hx_guard=False is the rule before the guard: 16-byte loads from min(x, Hx - 4) on rows
    narrower than four floats."""
    if not mfma_common(g, T):
        return False
    if hx_guard and g.Hx < 4:
        return False
    return 3 <= g.Ay <= 16


def mfma_has_corr_W(g, T):
    """mfma.hip:1140-1144: the one-tile form's LDS (window + W of one channel) within 64 KiB."""
    if not mfma_common(g, T):
        return False
    lds_w = (2 * (CW_TY + g.Ay - 1) * CW_XSTR + g.Ay * ((g.Ax + 1) & ~1) * 32) * 4
    return lds_w <= 64 * 1024


ReconPlan = namedtuple('ReconPlan', 'CB NB cgroups xblocks MB chunks lds')


def plan_reconstruct(g):
    """mfma.hip:1052-1074 and the LAUNCH_RC switch of mfma_reconstruct (:1201-1207)."""
    Axp4 = (g.Ax + 3) & ~3
    nbq = Axp4 >> 2
    CB = 1 if (2 <= nbq <= 4 and g.M <= 32) else min(g.C, 4)
    HST = 64 + Axp4
    ring = 4 * CB * 256 * 4
    per_atom = (CB * Axp4 * 16 + RC_RBK * HST) * 4
    MB = max(1, min((72 * 1024 - ring) // per_atom, 32, g.M))
    NB = nbq if (CB == 1 and 2 <= nbq <= 4) else 0
    return ReconPlan(CB, NB, cdiv(g.C, CB), cdiv(g.Dx, 64), MB, cdiv(g.M, MB), ring + per_atom * MB)


CorrHPlan = namedtuple('CorrHPlan', 'NT JG MT TW AST XSTW rblocks cblocks items P P_free nch_max lds')


def plan_corr_H(g, num_cu=NUM_CU):
    """mfma.hip:1082-1120."""
    nA = g.Ay * g.Ax
    J = g.C * nA
    tiles = cdiv(J, 16)
    JG = cdiv(tiles, 12)
    NT = cdiv(tiles, JG)
    MT = cdiv(g.M, 32)
    cblocks = cdiv(g.Hx, 72)
    TW = (cdiv(g.Hx, cblocks) + 3) & ~3
    XSTW = (TW + 31) & ~31
    AST = CH_RH * TW
    while AST & 31 != 2:
        AST += 1
    rblocks = cdiv(g.Hy, CH_RH)
    items = g.N * rblocks * cblocks
    P_free = max((2 * num_cu) // (MT * JG), 1)
    P = max(P_free, (items * 2 * TW + 32767) // 32768)      # one f32 chain below ~32K terms
    P = min(P, items, 8192)
    XST = XSTW + g.Ax + 1
    plane = (CH_RH + g.Ay - 1) * XST
    ZL = TW + XST + 8
    nch_max = 1
    for jg in range(JG):
        c0 = (jg * NT * 16) // nA
        c1 = min(((jg + 1) * NT * 16 - 1) // nA, g.C - 1)
        nch_max = max(nch_max, c1 - c0 + 1)
    stage = (32 * AST + 2 * (nch_max * plane + ZL)) * 4
    red = 4 * 2 * 4 * 64 * 4
    return CorrHPlan(NT, JG, MT, TW, AST, XSTW, rblocks, cblocks, items, P, P_free, nch_max, max(stage, red))


def mfma_has_corr_H(g, T):
    """mfma.hip:1146-1152 (planned for 256 compute units whatever the device)."""
    if not mfma_common(g, T):
        return False
    pl = plan_corr_H(g, 256)
    return pl.lds <= 80 * 1024 and pl.NT <= 12 and pl.TW <= 72 and g.Hx >= 4 and g.Dx >= 4


CorrWPlan = namedtuple('CorrWPlan', 'persist NE NBP wpieces lds tiles_y tiles_x MT ntiles P')


def persist_accepts(C, Ay, Ax, Dx=4):
    """The condition of the persistent form (mfma.hip:1235-1239): (accepted, window pieces, LDS bytes)."""
    Axp = (Ax + 1) & ~1
    SH = CP_TY + Ay - 1
    lds_p = (2 * SH * CW_XSTR + C * Ay * Axp * 32) * 4
    wpieces = SH * ((CW_TX + Axp - 1 + 3) // 4)
    return lds_p <= 52 * 1024 and wpieces <= CP_XE4 * kBlock and Dx >= 4, wpieces, lds_p


def persist_instance(wpieces, Ax):
    """The LAUNCH_CP chain of mfma_corr_W (mfma.hip:1248-1274): (NE, NBP)."""
    ne = cdiv(wpieces, kBlock)
    nbp = ((Ax + 1) & ~1) >> 1
    if ne <= 1 and nbp in (3, 4, 5, 6):
        return (1, nbp)
    if ne <= 2 and nbp == 8:
        return (2, 8)
    if ne <= 1:
        return (1, 0)
    return (2, 0) if ne == 2 else (3, 0)


def plan_corr_W(g, num_cu=NUM_CU):
    """mfma.hip:1231-1291, mfma_corr_W: the persistent form where W of all channels fits beside an 8-row window, else one
    tile of 16 rows per workgroup."""
    ok, wpieces, lds_p = persist_accepts(g.C, g.Ay, g.Ax, g.Dx)
    MT = cdiv(g.M, 32)
    tiles_x = cdiv(g.Hx, CW_TX)
    if ok:
        tiles_y = cdiv(g.Hy, CP_TY)
        ntiles = g.N * tiles_y * tiles_x
        P = min(max((2 * num_cu) // MT, 1), ntiles)
        NE, NBP = persist_instance(wpieces, g.Ax)
        return CorrWPlan(True, NE, NBP, wpieces, lds_p, tiles_y, tiles_x, MT, ntiles, P)
    tiles_y = cdiv(g.Hy, CW_TY)
    lds = (2 * (CW_TY + g.Ay - 1) * CW_XSTR + g.Ay * ((g.Ax + 1) & ~1) * 32) * 4
    ntiles = g.N * tiles_y * tiles_x
    return CorrWPlan(False, 0, 0, wpieces, lds, tiles_y, tiles_x, MT, ntiles, ntiles * MT)


# ----------------------------------------------------------------------------------------------------------------------
# generic.hip
# ----------------------------------------------------------------------------------------------------------------------
Tile = namedtuple('Tile', 'TY TX tiles_y tiles_x')


def make_tile(rows, cols):
    """generic.hip:21-36: 1 x 256 for one row, 8 x 32 for wide or short planes, 16 x 16 for narrow tall ones."""
    if rows == 1:
        TY, TX = 1, kBlock
    elif cols >= 32 or rows < 16:
        TY, TX = 8, 32
    else:
        TY, TX = 16, 16
    return Tile(TY, TX, cdiv(rows, TY), cdiv(cols, TX))


def reconstruct_small_lds(g, T, q):
    """generic.hip:267-270."""
    return (q * ((kSmallTY + g.Ay - 1) * (kSmallTX + g.Ax - 1) + g.Ay * g.Ax) + q * 64) * ESIZE[T]


def reconstruct_is_small(g, T, t):
    """generic.hip:273-278."""
    blocks = g.N * g.C * t.tiles_y * t.tiles_x
    return blocks < 64 and g.M >= kSmallQ and g.Dy > 1 and reconstruct_small_lds(g, T, kSmallQ) <= 64 * 1024


def generic_reconstruct(g, T):
    """generic.hip:797-826, launch_reconstruct: (kernel instance, tile, LDS) or None where it refuses (64 KiB)."""
    t = make_tile(g.Dy, g.Dx)
    lds = ((t.TY + g.Ay - 1) * (t.TX + g.Ax - 1) + g.Ay * g.Ax) * ESIZE[T]
    if lds > 64 * 1024:
        return None
    if reconstruct_is_small(g, T, t):
        if g.M > 8 and reconstruct_small_lds(g, T, 16) <= 64 * 1024:
            q = 16
        elif g.M > 4 and reconstruct_small_lds(g, T, 8) <= 64 * 1024:
            q = 8
        else:
            q = 4
        return ('k_reconstruct_small', T, q), Tile(kSmallTY, kSmallTX, cdiv(g.Dy, kSmallTY), cdiv(g.Dx, kSmallTX)), \
            reconstruct_small_lds(g, T, q)
    return ('k_reconstruct', T), t, lds


def generic_corr_W(g, T, fused):
    """generic.hip:828-844, launch_corr_W."""
    t = make_tile(g.Hy, g.Hx)
    lds = (2 * (t.TY + g.Ay - 1) * (t.TX + g.Ax - 1) + g.Ay * g.Ax) * ESIZE[T]
    if lds > 64 * 1024:
        return None
    return ('k_corr_W', T, fused), t, lds


def generic_corr_H_chunks(g, num_cu=NUM_CU):
    """generic.hip:880-888."""
    t = make_tile(g.Dy, g.Dx)
    items = g.N * t.tiles_y * t.tiles_x
    P = (num_cu * 8 + g.M * g.C - 1) // (g.M * g.C)
    return min(max(P, 1), items, 4096)


def generic_corr_H(g, T):
    """generic.hip:846-862, launch_corr_H: (instance, tile, LDS, threads per group, groups, shifts per thread)."""
    t = make_tile(g.Dy, g.Dx)
    nA = g.Ay * g.Ax
    if nA > kBlock * kMaxShiftsPerThread:
        return None
    gs = min(nA, kBlock)
    G = kBlock // gs
    lds = max(((t.TY + g.Ay - 1) * (t.TX + g.Ax - 1) + 2 * t.TY * t.TX) * ESIZE[T], G * nA * 2 * 8)
    if lds > 64 * 1024:
        return None
    return ('k_corr_H', T), t, lds, gs, G, cdiv(nA, gs)


# ----------------------------------------------------------------------------------------------------------------------
# api.hip
# ----------------------------------------------------------------------------------------------------------------------
def use_mfma(g, T, path, primitive):
    """api.hip:168-175."""
    if path in ('generic', 'fft'):
        return False
    if primitive == 'reconstruct':
        return mfma_has_reconstruct(g, T)
    if primitive in ('grad_H', 'update_H'):
        return mfma_has_corr_W(g, T)
    return mfma_has_corr_H(g, T)


def use_split(geometry, T, path):
    """api.hip:159-166 for the paths of this matrix: never under 'mfma' or 'generic'; under 'auto' float32 calls of 2^16
    activations or more that the split kernel covers and finds worth it."""
    return path == 'auto' and T == 'f' and use_split_under_auto(geometry)


Cell = namedtuple('Cell', 'family kernel inst error edges info')


def _refused(error='E_UNSUPPORTED'):
    return Cell('refused', None, None, error, frozenset(), None)


def cell(geometry, dtype, path, primitive, padded=False, num_cu=NUM_CU):
    """What one primitive runs on: do_reconstruct (api.hip:222-238), do_corr_W (:243-269), do_corr_H_partials (:272-283).

      family  'mfma', 'generic', 'split', 'fft' (path='auto' at 2^19 activations and more) or 'refused'
      kernel  the kernel's name; inst = (name, template arguments...): an element of all_instances()
      error   where refused: 'E_UNSUPPORTED', or 'E_STRIDE' for row-padded H in front of a family that wants it contiguous
      edges   the edge classes of the kernel this call meets (names: EDGES[kernel])
      info    the plan (ReconPlan, CorrWPlan, CorrHPlan or the generic tuple)
    padded: H with h_row_stride > Hx (the g.Hs == g.Hx conditions)."""
    assert dtype in DTYPES and path in PATHS and primitive in PRIMITIVES
    g = geo(geometry)
    fused = primitive == 'update_H'
    if path == 'auto' and primitive in ('reconstruct', 'grad_W') and use_fft_under_auto(geometry, dtype):
        return Cell('fft', None, None, None, frozenset(), None)                  # :225, :299
    if primitive in ('grad_H', 'update_H') and use_split(geometry, dtype, path):
        return Cell('split', 'k_split_corr_W', None, None, frozenset(), None)    # :253
    contiguous_ok = (not padded) or primitive == 'grad_H'                        # :231, :259 (!fused ||), :274
    if contiguous_ok and use_mfma(g, dtype, path, primitive):
        return _mfma_cell(g, primitive, fused, num_cu)
    if path == 'mfma':                                                           # :235, :265-266, :279
        return _refused('E_STRIDE' if padded and primitive != 'grad_H' else 'E_UNSUPPORTED')
    return _generic_cell(g, dtype, primitive, fused, padded, num_cu)


def _mfma_cell(g, primitive, fused, num_cu):
    e = set()
    if primitive == 'reconstruct':
        pl = plan_reconstruct(g)
        Axp4 = (g.Ax + 3) & ~3
        HST = 64 + Axp4
        e |= {f'rowgroups_{((g.Ay - 1) >> 2) + 1}'}
        e |= {f'Ay_{g.Ay}'} if g.Ay in (3, 4, 5, 16) else set()
        _flag(e, 'partial_channel_group', g.C % pl.CB != 0)
        _flag(e, 'atom_chunks_partial', pl.chunks > 1 and g.M % pl.MB != 0)
        _flag(e, 'odd_chunk', pl.MB % 2 == 1)
        _flag(e, 'Dx_mod64_1to3', g.Dx % 64 in (1, 2, 3))
        _flag(e, 'Dx_mod64_exact', g.Dx % 64 == 0)
        _flag(e, 'right_border', (pl.xblocks - 1) * 64 + HST > g.Hx)
        _flag(e, 'interior_block', HST <= g.Hx)
        _flag(e, 'Ax_not_mult4', g.Ax % 4 != 0)
        _flag(e, 'smallest_plane', g.Hx == 4)
        _flag(e, 'partial_row_block', (g.Dy + 3 + 4 * ((g.Ay - 1) >> 2)) % RC_RBK != 0)
        return Cell('mfma', 'k_mfma_reconstruct', ('k_mfma_reconstruct', pl.CB, pl.NB), None, frozenset(e), pl)
    if primitive == 'grad_W':
        pl = plan_corr_H(g, num_cu)
        J = g.C * g.Ay * g.Ax
        _flag(e, 'straddles_channels', pl.JG > 1 and pl.nch_max > 1)
        _flag(e, 'zero_strip', J % 16 != 0)
        _flag(e, 'ragged_column_blocks', pl.cblocks > 1 and pl.cblocks * pl.TW != g.Hx)
        _flag(e, 'edge_cols', pl.cblocks * pl.TW != g.Hx)
        _flag(e, 'exact_cols', pl.cblocks * pl.TW == g.Hx)
        _flag(e, 'partial_rows', g.Hy % CH_RH != 0)
        _flag(e, 'partial_atom_tile', g.M % 32 != 0)
        _flag(e, 'item_loop', pl.items > pl.P)
        _flag(e, 'P_clamped_to_items', pl.P == pl.items and pl.items < pl.P_free)
        _flag(e, 'one_sample', g.N == 1)
        _flag(e, 'several_channels', g.C > 1)
        return Cell('mfma', 'k_mfma_corr_H', ('k_mfma_corr_H', pl.NT), None, frozenset(e), pl)
    pl = plan_corr_W(g, num_cu)
    _flag(e, 'partial_atom_tile', g.M % 32 != 0)
    _flag(e, 'edge_cols', g.Hx % 32 != 0)
    _flag(e, 'edge_cols_1to3', g.Hx % 32 in (1, 2, 3))
    _flag(e, 'exact_cols', g.Hx % 32 == 0)
    _flag(e, 'odd_Ax', g.Ax % 2 == 1)
    _flag(e, 'several_channels', g.C > 1)
    if pl.persist:
        _flag(e, 'partial_rows', g.Hy % CP_TY != 0)
        _flag(e, 'Dx_4to7', 4 <= g.Dx <= 7)
        _flag(e, 'tile_loop_partial', pl.ntiles > pl.P and pl.ntiles % pl.P != 0)
        return Cell('mfma', 'k_mfma_corr_W_persist', ('k_mfma_corr_W_persist', fused, pl.NE, pl.NBP), None,
                    frozenset(e), pl)
    _flag(e, 'partial_rows', g.Hy % CW_TY != 0)
    _flag(e, 'Dx_below_4', g.Dx < 4)
    _flag(e, 'W_image_too_large', g.Dx >= 4)        # (the persistent form refused on its LDS bound or its piece count)
    return Cell('mfma', 'k_mfma_corr_W', ('k_mfma_corr_W', fused), None, frozenset(e), pl)


def _flag(edges, name, on):
    if on:
        edges.add(name)


def _generic_cell(g, T, primitive, fused, padded, num_cu):
    e = set()
    if primitive == 'reconstruct':
        got, rows, cols = generic_reconstruct(g, T), g.Dy, g.Dx
    elif primitive == 'grad_W':
        got, rows, cols = generic_corr_H(g, T), g.Dy, g.Dx
    else:
        got, rows, cols = generic_corr_W(g, T, fused), g.Hy, g.Hx
    if got is None:
        return _refused()
    inst, t = got[0], got[1]
    full = make_tile(rows, cols)
    e.add(f'tile_{full.TY}x{full.TX}')
    _flag(e, f'tile_{full.TY}x{full.TX}_ragged', rows % full.TY != 0 and cols % full.TX != 0 if rows > 1
          else cols % full.TX != 0)
    _flag(e, 'padded_H', padded)
    _flag(e, 'one_d', g.one_d)
    if T == 'f' and g.Dy > 1 and g.Ay > 1:
        # float32 problems on two shift axes that the MFMA family hands over
        _flag(e, 'handover_Hx_below_4', g.Hx < 4)
        _flag(e, 'handover_Dx_below_4', g.Dx < 4)
        _flag(e, 'handover_Ay_2', primitive == 'reconstruct' and g.Ay == 2)
        _flag(e, 'handover_Ay_above_16', primitive == 'reconstruct' and g.Ay > 16)
        _flag(e, 'handover_32x32', primitive in ('grad_H', 'update_H') and (g.Ay, g.Ax) == (32, 32))
    if primitive == 'reconstruct':
        _flag(e, 'small_M_4', inst[0] == 'k_reconstruct_small' and g.M == 4)
    if primitive == 'grad_W':
        _, _, _, gs, G, shifts = got
        _flag(e, 'several_groups', G > 1)
        _flag(e, f'shifts_{shifts}', shifts > 1)
        P = generic_corr_H_chunks(g, num_cu)
        _flag(e, 'item_loop', g.N * full.tiles_y * full.tiles_x > P)
    return Cell('generic', inst[0], inst, None, frozenset(e), got)


# What a call of the backend runs, in order (HIP.py -> api.hip): the gradients and the fused steps reconstruct first.
API_CALLS = {
    'reconstruct': ('reconstruct',),
    'grad_H': ('reconstruct', 'grad_H'),         # tnmf_hip_grad_H without R (api.hip:716-731)
    'update_H': ('reconstruct', 'update_H'),     # update_H_2d (api.hip:924-926)
    'grad_W': ('reconstruct', 'grad_W'),         # grad_W_2d (api.hip:1022-1026)
}


def api_family(geometry, dtype, path, call, padded=False):
    """ctx->last_path after the backend's `call`: the family of the last primitive it runs, or 'refused' with the error
    as soon as one of them is: (family, error)."""
    last = None
    for prim in API_CALLS[call]:
        last = cell(geometry, dtype, path, prim, padded)
        if last.family == 'refused':
            return 'refused', last.error
    return last.family, None


# ----------------------------------------------------------------------------------------------------------------------
# instances
# ----------------------------------------------------------------------------------------------------------------------
PERSIST_ARMS = ((1, 3), (1, 4), (1, 5), (1, 6), (2, 8), (1, 0), (2, 0), (3, 0))     # LAUNCH_CP arms, in order
RECONSTRUCT_INSTANCES = ((1, 0), (1, 2), (1, 3), (1, 4), (2, 0), (3, 0), (4, 0))    # SET_LDS / LAUNCH_RC
CORR_H_NT = tuple(range(1, 13))                                                     # SET_LDS / LAUNCH_CH


def all_instances(family=None):
    """Every instance of the direct kernels the sources instantiate."""
    mfma = {('k_mfma_corr_W_persist', f, ne, nbp) for f in (True, False) for ne, nbp in PERSIST_ARMS}
    mfma |= {('k_mfma_corr_W', f) for f in (True, False)}
    mfma |= {('k_mfma_corr_H', nt) for nt in CORR_H_NT}
    mfma |= {('k_mfma_reconstruct', cb, nb) for cb, nb in RECONSTRUCT_INSTANCES}
    gen = set()
    for T in DTYPES:
        gen |= {('k_reconstruct', T), ('k_corr_H', T)}
        gen |= {('k_reconstruct_small', T, q) for q in (4, 8, 16)}
        gen |= {('k_corr_W', T, f) for f in (True, False)}
    return {'mfma': mfma, 'generic': gen, None: mfma | gen}[family]


def persist_arms_reached():
    """Every (NE, NBP) some accepted geometry selects: the whole accepted domain Ay, Ax <= 32 (mfma_common) at one
    channel -- the LDS bound only tightens with C, the piece count does not depend on it."""
    arms = {}
    for Ay in range(2, 33):
        for Ax in range(1, 33):
            ok, wpieces, _ = persist_accepts(1, Ay, Ax)
            if ok:
                arms.setdefault(persist_instance(wpieces, Ax), (Ay, Ax))
    return arms


# Instances no accepted geometry selects.  k_mfma_corr_W_persist<*, 3, 0> needs more than 512 window pieces
# ((Ay + 7) * ceil((31 + Axp) / 4)), i.e. Ay >= 26 with Ax >= 21, whose LDS footprint (101 KiB at the least, with one
# channel) is beyond the 52 KiB the persistent form accepts -- by enumeration in tests/test_direct_dispatch_cpu.py.  The
# arm stays in the source as the catch-all of the chain.
UNREACHABLE = {
    ('k_mfma_corr_W_persist', True, 3, 0): 'more than 512 window pieces need a W image beyond the 52 KiB bound',
    ('k_mfma_corr_W_persist', False, 3, 0): 'more than 512 window pieces need a W image beyond the 52 KiB bound',
}

# What the matrix leaves out, with the reason (tests/test_direct_dispatch_cpu.py checks the list is exact).
NOT_COVERED = {}

# The edge classes each kernel has to meet somewhere in the matrix.
EDGES = {
    'k_mfma_corr_W_persist': ('partial_atom_tile', 'partial_rows', 'edge_cols', 'edge_cols_1to3', 'exact_cols', 'odd_Ax',
                              'Dx_4to7', 'several_channels', 'tile_loop_partial'),
    'k_mfma_corr_W': ('partial_atom_tile', 'partial_rows', 'edge_cols', 'exact_cols', 'odd_Ax', 'Dx_below_4',
                      'W_image_too_large', 'several_channels'),
    'k_mfma_corr_H': ('straddles_channels', 'zero_strip', 'ragged_column_blocks', 'edge_cols', 'exact_cols', 'partial_rows',
                      'partial_atom_tile', 'item_loop', 'P_clamped_to_items', 'one_sample', 'several_channels'),
    'k_mfma_reconstruct': ('partial_channel_group', 'atom_chunks_partial', 'odd_chunk', 'Dx_mod64_1to3', 'Dx_mod64_exact',
                           'right_border', 'interior_block', 'Ay_3', 'Ay_4', 'Ay_5', 'Ay_16', 'rowgroups_1', 'rowgroups_2',
                           'rowgroups_3', 'rowgroups_4', 'Ax_not_mult4', 'smallest_plane', 'partial_row_block'),
}
GENERIC_EDGES = {
    'reconstruct': ('tile_1x256_ragged', 'tile_8x32_ragged', 'tile_16x16_ragged', 'padded_H', 'one_d', 'small_M_4',
                    'handover_Hx_below_4', 'handover_Dx_below_4', 'handover_Ay_2', 'handover_Ay_above_16'),
    'grad_H': ('tile_1x256_ragged', 'tile_8x32_ragged', 'tile_16x16_ragged', 'padded_H', 'one_d', 'handover_32x32'),
    'update_H': ('tile_1x256_ragged', 'tile_8x32_ragged', 'tile_16x16_ragged', 'padded_H', 'one_d', 'handover_32x32'),
    'grad_W': ('tile_1x256_ragged', 'tile_8x32_ragged', 'tile_16x16_ragged', 'padded_H', 'one_d', 'several_groups',
               'shifts_2', 'shifts_3', 'shifts_4', 'item_loop', 'handover_Hx_below_4', 'handover_Dx_below_4'),
}

# ----------------------------------------------------------------------------------------------------------------------
# The geometries of tests/test_hip_direct_matrix.py: (N, C, D, M, A).  Counts quoted for 256 compute units.
# ----------------------------------------------------------------------------------------------------------------------
MATRIX = {
    'p13': (2, 1, (21, 37), 33, (5, 6)),            # persist<1,3>; reconstruct<1,2> in chunks of 32 + 1; NT 2
    'p14_c2': (2, 2, (20, 30), 8, (7, 7)),          # persist<1,4>, odd Ax, two channels; NT 7 over both channels
    'p15_loop': (3, 1, (60, 70), 200, (8, 10)),     # persist<1,5>, tile loop: 81 tiles on P = 73; reconstruct<1,3> in
                                                    # seven chunks; NT 5 with 102 work items on P = 73
    'p16_c3': (2, 3, (25, 53), 20, (9, 12)),        # persist<1,6>, Hx = 64 (exact fit); NT 11 x JG 2 straddling channels
    'p28': (2, 1, (22, 49), 31, (11, 16)),          # persist<2,8>, Hx = 64; reconstruct<1,4> in chunks of 30 + 1; NT 11
    'p28_c2': (2, 2, (23, 19), 12, (4, 15)),        # persist<2,8> with two channels, Hx = 33; reconstruct<1,4>, Ay = 4
    'p10': (2, 1, (20, 20), 5, (3, 3)),             # persist<1,0>, NT 1, reconstruct<1,0>, Ay = 3, a chunk of five atoms
    'p10_w': (2, 1, (26, 5), 6, (16, 13)),          # persist<2,0> (Ax 13 on a tall atom), Dx = 5 (clamped window load), Ay = 16
    'p20_tall': (1, 1, (30, 30), 4, (24, 2)),       # persist<2,0> by a tall atom; NT 3; reconstruct on the generic kernel
    'p20_wide': (1, 1, (20, 64), 9, (10, 29)),      # persist<2,0> by a wide atom; NT 10 x JG 2; reconstruct<1,0>, Dx % 64 = 0
    'p20_c2': (2, 2, (17, 36), 7, (5, 29)),         # persist<1,0> with two channels; Hx = 64; reconstruct<2,0>, Ay = 5
    'r40': (2, 4, (30, 27), 40, (6, 8)),            # reconstruct<4,0>, three chunks (17 + 17 + 6); NT 12 over four channels
    'r40_c5': (2, 5, (18, 65), 9, (4, 3)),          # reconstruct<4,0> with C % CB = 1 and Dx % 64 = 1; NT 4 over five channels
    'r20': (2, 2, (19, 130), 34, (13, 4)),          # reconstruct<2,0>, Dx % 64 = 2, three column blocks; NT 7; cblocks 2
    'r30': (2, 3, (24, 40), 40, (12, 12)),          # reconstruct<3,0>; one-tile H gradient (W image of three channels); JG 3
    't_c5': (2, 5, (24, 130), 40, (9, 12)),         # one-tile H gradient; NT 12 x JG 3, cblocks 2; reconstruct<4,0> with C = 5
    't_16': (1, 3, (17, 49), 32, (16, 16)),         # one-tile H gradient, Hx = 64 exact, Hy % 16 = 0, M % 32 = 0; one sample
    't_narrow': (2, 1, (20, 3), 4, (8, 2)),         # Hx = 4, Dx = 3: one-tile H gradient, the smallest reconstruct plane
    't_narrow_c2': (3, 2, (18, 2), 33, (5, 7)),     # Dx = 2 with odd Ax, two channels, partial atom tile
    'nt2': (2, 1, (37, 76), 16, (5, 5)),            # NT 2; cblocks 2 with TW = 40 exact
    'nt5': (2, 1, (30, 70), 8, (9, 8)),             # NT 5; cblocks 2, TW 40 over Hx = 77
    'nt6': (2, 3, (33, 31), 7, (5, 6)),             # NT 6, three channels in one column group
    'nt8': (1, 1, (33, 140), 70, (11, 11)),         # NT 8; cblocks 3, TW 52 (ragged); one sample; M % 32 = 6
    'nt9': (2, 1, (29, 44), 12, (12, 12)),          # NT 9 (J % 16 = 0)
    'nt11': (2, 1, (25, 30), 10, (13, 13)),         # NT 11 (J = 169)
    'h_hx3': (2, 1, (20, 3), 5, (3, 1)),            # Hx = 3: the shape the Hx >= 4 guard hands to the generic kernels
    'h_hx1': (3, 1, (17, 1), 6, (4, 1)),            # Hx = 1
    'h_ay2': (2, 1, (18, 40), 9, (2, 7)),           # Ay = 2: reconstruct on the generic kernel, gradients on the MFMA ones
    'h_ay17': (2, 1, (20, 24), 5, (17, 16)),        # Ay = 17 (272 shifts: two per thread in the generic W gradient)
    'h_24': (1, 1, (30, 28), 4, (24, 24)),          # 576 shifts: three per thread; k_reconstruct_small<4>; 16 x 16 tile
    'h_32': (2, 1, (40, 36), 6, (32, 32)),          # 32 x 32 atoms: 1024 shifts; reconstruct and the H gradient handed over
    'g_small8': (1, 2, (12, 40), 7, (3, 5)),        # k_reconstruct_small<8> (M in 5..8)
    'g_small16': (3, 1, (32, 32), 10, (7, 7)),      # k_reconstruct_small<16>: the mini-batch of the stochastic schedules
    'g_tall': (2, 1, (37, 19), 3, (6, 5)),          # 16 x 16 tile on reconstruct and W gradient, ragged both ways
    'g_1d': (2, 1, (1000,), 8, (20,)),              # 1-D: the 1 x 256 tile, four ragged column tiles
    'g_1d_c3': (5, 3, (300,), 3, (1,)),             # 1-D with one-tap atoms, three channels
    'g_1d_long': (2, 1, (700,), 5, (300,)),         # 1-D with 300-tap atoms: two shifts per thread
}


def corner_spots(Hs):
    """The activations of the 'corners' operands: the corners and the centre of a shift plane of shape Hs (1-D: both ends
    and the centre); plane (n, m) carries spot j when n + m + j is even."""
    ends = [(0, h - 1) for h in Hs]
    spots = [(x,) for x in ends[0]] if len(Hs) == 1 else [(y, x) for y in ends[0] for x in ends[1]]
    spots.append(tuple(h // 2 for h in Hs))
    return spots


def matrix_cases():
    """(geometry id, dtype, path) of the GPU matrix: path='generic' in both dtypes everywhere; path='mfma' in float32 where
    the family runs at least one primitive; path='auto' where its mix of families is neither of those and stays on the
    direct kernels (the hand-over shapes: below 2^16 activations, so neither the split kernel nor the FFT family)."""
    out = []
    for gid, G in MATRIX.items():
        fam = {p: tuple(cell(G, 'f', p, prim).family for prim in PRIMITIVES) for p in PATHS}
        if 'mfma' in fam['mfma']:
            out.append((gid, 'f', 'mfma'))
        out += [(gid, 'f', 'generic'), (gid, 'd', 'generic')]
        if fam['auto'] not in (fam['mfma'], fam['generic']) and set(fam['auto']) <= {'mfma', 'generic'}:
            out.append((gid, 'f', 'auto'))
    return out
