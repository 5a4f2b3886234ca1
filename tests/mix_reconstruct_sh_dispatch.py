"""
Host mirror of the dispatch of k_mix_reconstruct_sh, the one-channel 2-D mixed reconstruct of large calls that stages the
row spectra through LDS: which calls it takes (fft_mixed.hip: mixed_reconstruct_sh_takes), what its grid looks like and
which edges of the kernel a call meets -- restated in plain Python on top of tests/fft_dispatch.py, so that
tests/test_hip_mix_reconstruct_sh.py can choose the smallest geometries that cross the threshold and still reach every edge,
and a CPU test (tests/test_mix_reconstruct_sh_dispatch_cpu.py) can hold the restatement to the sources and the choice to
the edges.

A geometry is (N, C, D, M, A) as in fft_dispatch; n_call is the number of samples of one call on a slice of it.
"""
import fft_dispatch as fd

RSH_STRIPS = 16            # fft.h  TNMF_MIX_RSH_STRIPS / kMixRShStrips: strips of 16 output rows per workgroup
RSH_TILES = 1              # fft.h  TNMF_MIX_RSH_TILES / kMixRShTiles: LDS tiles per workgroup
RSH_PER_CU = 3             # fft.h  TNMF_MIX_RSH_PER_CU / kMixRShPerCU: workgroups per CU (of four waves: waves per SIMD)
RSH_MAX_AY = 12            # fft.h  kMixRShMaxAy
RSH_MIN_BYTES = 24 << 20   # fft.h  kMixRShMinBytes: row spectra of H of the call
RSH_S = 16                 # fft_mixed.hip  k_mix_reconstruct_sh: S output rows per thread
RSH_BLOCK = RSH_S * RSH_STRIPS   # output rows per workgroup


def tile_rows(Ay):
    """fft_mixed.hip  k_mix_reconstruct_sh: ROWS, the rows of T a workgroup stages per atom."""
    return RSH_BLOCK + Ay - 1


def lds_bytes(Ay):
    """fft_mixed.hip  k_mix_reconstruct_sh: TILES tiles of ROWS rows at a pitch of 17 entries (rounded up to 16 bytes) plus
    the atom's Ay rows of W spectra."""
    trows = (tile_rows(Ay) * 17 + 1) // 2 * 2
    return RSH_TILES * (trows + Ay * 16) * 8


def workgroups_per_cu(Ay, lds_per_cu=160 << 10):
    """fft_mixed.hip  launch_mix_reconstruct: unused dynamic LDS tops a workgroup up to just over a (RSH_PER_CU + 1)-th
    of the CU's LDS, so that RSH_PER_CU workgroups fit and no more."""
    hold = lds_per_cu // (RSH_PER_CU + 1) + 1
    return lds_per_cu // max(lds_bytes(Ay), hold)


def spectra_bytes(geometry, n_call=None):
    """Row spectra of H of one call: N * M * Hy * KXP * 8 bytes."""
    N, _, _, M, _ = geometry
    Hy = fd._dims(geometry)[4]
    return (N if n_call is None else n_call) * M * Hy * fd.make_layout(geometry, 'f', 'hybrid').KXP * 8


def rsh_takes(geometry, dtype='f', n_call=None):
    """fft_mixed.hip  mixed_reconstruct_sh_takes, behind use_mixed(): float32, one channel, 2-D, atoms up to 12 rows, a
    plane's bytes below 2^31, and at least RSH_MIN_BYTES of row spectra."""
    C = geometry[1]
    Ay, Hy = fd._dims(geometry)[2], fd._dims(geometry)[4]
    if not (fd.fft_has(geometry, dtype) and fd.mixed_has_reconstruct(geometry, dtype)):
        return False
    KXP = fd.make_layout(geometry, dtype, 'hybrid').KXP
    return (C == 1 and Ay <= RSH_MAX_AY and not fd.one_d(geometry) and Hy * KXP * 8 < 1 << 31
            and spectra_bytes(geometry, n_call) >= RSH_MIN_BYTES)


def rsh_grid(geometry, n_call=None):
    """(kx tiles, row blocks, samples) of the launch."""
    N = geometry[0]
    Dy = fd._dims(geometry)[0]
    KX = fd.make_layout(geometry, 'f', 'hybrid').KX
    return fd.cdiv(KX, fd.MIX_COLS), fd.cdiv(Dy, RSH_BLOCK), N if n_call is None else n_call


def reconstruct_kernel(geometry, n_call=None):
    """The kernel the mixed reconstruct of a float32 call runs on (None: not a mixed call)."""
    if rsh_takes(geometry, 'f', n_call):
        return 'k_mix_reconstruct_sh'
    names = {i[0] for i in fd.cells(geometry, 'f', 'hybrid', n_call=n_call) if i[0].startswith('k_mix_reconstruct')}
    assert len(names) <= 1
    return names.pop() if names else None


def under_threshold(geometry, n_call=None):
    """The largest number of samples per call at which the same problem stays on k_mix_reconstruct."""
    n = geometry[0] if n_call is None else n_call
    while n > 1 and rsh_takes(geometry, 'f', n):
        n -= 1
    assert not rsh_takes(geometry, 'f', n)
    return n


def edges(geometry, n_call=None):
    """The edge classes of k_mix_reconstruct_sh a call meets."""
    N, _, _, M, _ = geometry
    Dy, _, Ay, _, Hy, _ = fd._dims(geometry)
    lay = fd.make_layout(geometry, 'f', 'hybrid')
    gx, gy, _ = rsh_grid(geometry, n_call)
    out = {'ay_%d' % Ay}
    if lay.KX % 16:
        out.add('kx_tail')              # partial last kx tile: column clamped, not stored
    if gx > 1:
        out.add('kx_tiles')             # more than one kx tile: the loader's column offset
    if Dy < RSH_BLOCK:
        out.add('rows_short')           # fewer rows than one row block
    if Dy % RSH_BLOCK:
        out.add('rows_tail')            # the last row block stores fewer rows
    else:
        out.add('rows_whole')           # every strip of the last block stores all its rows
    if gy > 1:
        out.add('row_blocks')           # several row blocks: the tile's first row
    if gy > 1 and Dy % RSH_BLOCK and Dy % RSH_BLOCK <= RSH_BLOCK // 2:
        out.add('row_block_short')      # ... the last one with whole strips that store nothing
    if (gy - 1) * RSH_BLOCK + tile_rows(Ay) > Hy:
        out.add('rows_past_plane')      # tile rows past the plane (on the last plane of the call too): clamped
    if M < 8:
        out.add('atoms_few')            # fewer atoms than the eight-atom chunk of k_mix_reconstruct
    if M % 8:
        out.add('atoms_tail')           # no multiple of it
    out.add('atoms_odd' if M % 2 else 'atoms_even')   # the LDS tile the last atom is read from
    if n_call is not None and n_call < N:
        out.add('slice')                # a slice of the bound samples: the spectra of the slice
    return out


# the GPU cases: (N, C, D, M, A) of the bound problem, samples per call (None: all)
CASES = {
    'ay12_two_blocks_m9': ((15, 1, (300, 100), 9, (12, 12)), None),
    'ay9_short_plane_m5': ((164, 1, (40, 120), 5, (9, 9)), None),
    'ay5_one_block_m12': ((16, 1, (256, 60), 12, (5, 8)), None),
    'ay1_rows258_m16': ((16, 1, (258, 47), 16, (1, 3)), None),
    'slices_of_a_binding': ((45, 1, (300, 100), 9, (12, 12)), 15),
}
EDGES = ('ay_1', 'ay_5', 'ay_9', 'ay_12', 'kx_tail', 'kx_tiles', 'rows_short', 'rows_tail', 'rows_whole', 'row_blocks',
         'row_block_short', 'rows_past_plane', 'atoms_few', 'atoms_tail', 'atoms_odd', 'atoms_even', 'slice')
