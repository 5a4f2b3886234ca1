"""
Host mirror of the split (3 x bf16) H-update dispatch: which instance of k_split_corr_W<FUSED, MULTI, AY, NR4, EXTRA>
runs a problem, on which MFMA form, with how many waves, how much LDS and how many workgroups -- restated in plain
Python from tnmf_amd/csrc/split.hip and tnmf_amd/csrc/split_kernels.h, so that the tests can choose geometries that
reach every instance and every edge of the kernel (tests/test_hip_split_matrix.py) and a CPU test can check that the
choice covers them all (tests/test_split_dispatch_cpu.py).

A geometry is (N, C, D, M, A): samples, channels, sample shape, atoms, atom shape (1-D: one-element D and A).
"""
from collections import namedtuple

NUM_CU = 256    # compute units of one MI355X (what launch() reads from ctx->num_cu there)

# split.hip, TNMF_SPLIT_SHAPES: (atom rows AY, runs of four taps per atom row NR4), in dispatch order (ties go to the first)
SHAPES = ((12, 3), (9, 3), (16, 4), (7, 2), (8, 2), (5, 2), (1, 4), (1, 8), (1, 16))

KINDS = ('grad', 'fused', 'extra')      # unfused gradient, fused update, fused update + lateral terms (EXTRA)


def split_plane_bytes(rows, wstr):
    """split_kernels.h:62."""
    return ((rows * wstr * 2 - 64 + 255) // 256) * 256 + 64


class SplitCfg:
    """split_kernels.h:68-114, struct SplitCfg<AY, NR4>: the compile-time geometry of one instantiation."""

    def __init__(self, AY, NR4):
        self.AY, self.NR4 = AY, NR4
        self.ONE_D = AY == 1                                                   # :70
        self.WSTR = 4 * NR4 + 28                                               # :72
        self.NP = (AY + 1) // 2                                                # :74
        self.NSLOT = NR4 // 2 if self.ONE_D else self.NP * NR4                 # :75
        self.KB = (self.NSLOT + 1) // 2                                        # :76
        self.NKB16 = (AY * NR4 + 7) // 8                                       # :90-91
        self.wimg16, self.wimg32 = self.NKB16 * 6 * 1024, self.KB * 3 * 1024   # :92
        has16 = self.m16(True) or self.m16(False)
        self.wimg = self.wimg16 if has16 and self.wimg16 > self.wimg32 else self.wimg32   # :93
        lds4 = self.wimg + 24 * split_plane_bytes(8 + AY, self.WSTR)          # :101
        lds8 = self.wimg + 24 * split_plane_bytes(16 + AY, self.WSTR)         # :102
        self.WAVES = 8 if (not self.ONE_D and lds4 > 80 * 1024 and lds8 <= 160 * 1024) else 4   # :103
        self.kBlock, self.TY = 64 * self.WAVES, 2 * self.WAVES                # :104 (SP_RB = 2)
        self.planeB = split_plane_bytes(self.TY + AY, self.WSTR)              # :106, :108
        self.lds = self.wimg + 24 * self.planeB                                # :109-110

    def m16(self, multi):
        """split_kernels.h:87 (product build): the 16x16x32 form for 16 x 16 atoms always, for 12 x 12 with several channels."""
        return (self.AY == 16 and self.NR4 == 4) or (self.AY == 12 and self.NR4 == 3 and multi)


def kb_of(AY, NR4):
    """k blocks of an instantiation as split_pick counts them (split.hip:28, :52)."""
    return (((AY + 1) // 2) * NR4 + 1) // 2


def one_d(geometry):
    return len(geometry[4]) == 1


def _dims(geometry):
    """(Dy, Dx, Ay, Ax) as the library's Geo holds them: a 1-D problem is one row."""
    _, _, D, _, A = geometry
    return (1, D[0], 1, A[0]) if len(A) == 1 else (D[0], D[1], A[0], A[1])


def split_pick(geometry):
    """split.hip:22-36: the covering instantiation with the fewest k blocks, (AY, NR4); None when none covers."""
    Dy, _, Ay, Ax = _dims(geometry)
    if Dy == 1 and Ay == 1:                                                    # :23
        return (1, 4 if Ax <= 16 else (8 if Ax <= 32 else 16))
    nr4 = (Ax + 3) // 4
    best, best_kb = None, 1 << 30
    for AY, NR4 in SHAPES:                                                     # :26-34
        if AY > 1 and AY >= Ay and NR4 >= nr4 and kb_of(AY, NR4) < best_kb:
            best, best_kb = (AY, NR4), kb_of(AY, NR4)
    return best


def split_has_corr_W(geometry, only_if_worth=False):
    """split.hip:38-58 (float32), without the 2^31-byte offset guard (the tests stay far below it)."""
    Dy, Dx, Ay, Ax = _dims(geometry)
    if Dy == 1 and Ay == 1:
        return Ax <= 64 and Dx >= 4                                            # :42
    if Dy == 1 or Ay == 1 or Ax > 16 or Ay > 16 or Dx < 4:                     # :44-45
        return False
    pick = split_pick(geometry)
    if pick is None:
        return False
    return not (only_if_worth and 6 * kb_of(*pick) > Ay * Ax)                 # :50-55


def use_split_under_auto(geometry):
    """api.hip use_split() under path='auto' (float32): 2^16 activations or more, and worth it."""
    N, _, D, M, A = geometry
    size = N * M
    for d, a in zip(D, A):
        size *= d + a - 1
    return size >= 1 << 16 and split_has_corr_W(geometry, only_if_worth=True)


Cell = namedtuple('Cell', 'inst form multi extra waves block lds TY P tiles '
                          'partial_atom_tile partial_rows edge_cols tile_loop_partial refused')


def cell(geometry, kind, num_cu=NUM_CU):
    """What path='split' runs for one call `kind` ('grad', 'fused' or 'extra') on `geometry` = (N, C, D, M, A), with
    row-padded activations (H rows padded to whole 32-float tiles, as the EXTRA epilogue requires):

      inst    (FUSED, MULTI, AY, NR4, EXTRA): the template arguments of k_split_corr_W that run.  'extra' on a 1-D problem
              is refused (launch(), split_kernels.h:948) and the fallback's unfused gradient runs: refused=True, and
              inst is the gradient instance.
      form    '16x16x32', '32x32' or '1d' (the 32x32x16 MFMA with the rows of a tile being samples)
      waves, block, lds   waves and threads per workgroup, dynamic LDS bytes (SplitCfg)
      TY, P, tiles        rows per tile, workgroups per atom tile, (row block, column tile) tiles (launch())
    and the edge flags: a partial atom tile (M % 32), a partial row block (Hy % TY; 1-D: N % TY), a last column tile of
    one to three pixels or a row narrower than eight (Hx % 32 in 1..3, Hx < 8), and the persistent tile loop with a
    partial last round (tiles > P, tiles % P != 0)."""
    assert kind in KINDS
    N, C, D, M, A = geometry
    pick = split_pick(geometry)
    assert pick is not None and split_has_corr_W(geometry), geometry
    cfg = SplitCfg(*pick)
    multi = C > 1                                                              # launch(): g.C > 1 selects MULTI
    refused = kind == 'extra' and cfg.ONE_D                                    # split_kernels.h:948
    fused = kind != 'grad' and not refused
    extra = kind == 'extra' and not refused
    # split_kernels.h:269: M16 = m16(MULTI) && !(EXTRA && MULTI) -- the same rule picks the W image at :964
    if cfg.ONE_D:
        form = '1d'
    else:
        form = '16x16x32' if cfg.m16(multi) and not (extra and multi) else '32x32'
    Hy = 1 if cfg.ONE_D else D[0] + A[0] - 1
    Hx = D[-1] + A[-1] - 1
    # launch(), split_kernels.h:971-979
    MT = -(-M // 32)
    tiles_y = -(-N // cfg.TY) if cfg.ONE_D else -(-Hy // cfg.TY)
    tiles_x = -(-Hx // 32)
    nrowblocks = tiles_y if cfg.ONE_D else N * tiles_y
    tiles = nrowblocks * tiles_x
    per_cu = 2 if cfg.lds <= 80 * 1024 else 1                                  # :976
    P = min(max((per_cu * num_cu) // MT, 1), tiles)                            # :977-979
    rows = N if cfg.ONE_D else Hy
    return Cell(inst=(fused, multi, cfg.AY, cfg.NR4, extra), form=form, multi=multi, extra=extra, waves=cfg.WAVES,
                block=cfg.kBlock, lds=cfg.lds, TY=cfg.TY, P=P, tiles=tiles,
                partial_atom_tile=M % 32 != 0, partial_rows=rows % cfg.TY != 0,
                edge_cols=Hx % 32 in (1, 2, 3) or Hx < 8,
                tile_loop_partial=tiles > P and tiles % P != 0, refused=refused)


def all_instances():
    """Every k_split_corr_W instance prepare_one() sets attributes for (split_kernels.h:1028-1043): per instantiation the
    four (FUSED, MULTI) combinations without EXTRA, and the two fused ones with EXTRA on 2-D instantiations."""
    out = set()
    for AY, NR4 in SHAPES:
        for fused in (True, False):
            for multi in (True, False):
                out.add((fused, multi, AY, NR4, False))
        if AY != 1:
            for multi in (True, False):
                out.add((True, multi, AY, NR4, True))
    return out


# The geometries of tests/test_hip_split_matrix.py: (N, C, D, M, A).  Tile-loop counts quoted for 256 compute units.
MATRIX = {
    's12_c1': (3, 1, (60, 70), 200, (12, 12)),      # tile loop: 81 tiles on P = 73
    's12_c4': (2, 4, (30, 53), 40, (11, 10)),       # window ring wraps (C > 3); 16x16x32 form, 32x32 under EXTRA
    's9_c1': (2, 1, (41, 55), 33, (9, 9)),
    's9_c5': (2, 5, (24, 30), 20, (9, 12)),
    's16_c1': (2, 1, (40, 36), 20, (16, 16)),       # EXTRA on the 16x16x32 form (one channel)
    's16_c1_big': (2, 1, (60, 66), 300, (15, 13)),  # tile loop on eight-wave workgroups: 30 tiles on P = 25
    's16_c2': (2, 2, (25, 50), 35, (13, 16)),       # Hx % 32 == 1
    's7_c1': (3, 1, (33, 4), 17, (7, 7)),           # the narrowest sample (Dx = 4)
    's7_c4': (2, 4, (30, 27), 12, (6, 8)),
    's8_c1': (2, 1, (26, 62), 64, (8, 8)),
    's8_c3': (2, 3, (29, 63), 9, (8, 5)),           # Hx % 32 == 3
    's5_c1': (2, 1, (40, 4), 33, (5, 4)),           # Hx = 7
    's5_c2': (2, 2, (19, 70), 40, (4, 5)),
    'd4_c1': (9, 1, (130,), 40, (16,)),
    'd4_c3': (10, 3, (61,), 20, (11,)),
    'd8_c1': (13, 1, (150,), 48, (17,)),
    'd8_c4': (11, 4, (97,), 9, (30,)),
    'd16_c1': (5, 1, (40,), 33, (64,)),
    'd16_c2': (20, 2, (200,), 70, (50,)),
    'd4_loop': (48, 1, (274,), 300, (16,)),         # 1-D tile loop: 60 tiles on P = 51; Hx % 32 == 1
}
