"""
Host mirror of the dispatch of k_mix_grad_W3, the three-multiply mixed W gradient of large calls: which calls it takes
(fft_mixed.hip: mixed_grad_W3_takes), into how many sample groups it splits them (fft.hip: mix_groups_w3) and what its
grid looks like -- restated in plain Python on top of tests/fft_dispatch.py, so that tests/test_hip_mix_grad_w3.py can
choose the smallest geometries that cross the threshold and still reach every edge of the kernel, and a CPU test
(tests/test_mix_grad_w3_dispatch_cpu.py) can hold the restatement to the sources and the choice to the edges.

A geometry is (N, C, D, M, A) as in fft_dispatch; n_call is the number of samples of one call on a slice of it.
"""
import fft_dispatch as fd

W3_ATOMS = 16            # fft.h  kMixW3Atoms: atoms per workgroup
W3_MAX_AY = 12           # fft.h  kMixW3MaxAy
W3_MIN_BYTES = 24 << 20  # fft.h  kMixW3MinBytes: row spectra of H of the call
W3_CHUNK = 16            # fft_mixed.hip  k_mix_grad_W3: RS = CH = 16 rows per ring period / LDS chunk


def w3_waves(Ay):
    """fft.h  mix_w3_waves: workgroups per CU of k_mix_grad_W3<float, Ay> (the compiler's resource report)."""
    return 3 if Ay >= 8 else (4 if Ay >= 4 else (5 if Ay >= 2 else 7))


def w3_span(Hy, KXP):
    """fft_mixed.hip  mixed_grad_W3_takes: the largest per-lane byte offset (atom slot 15, last row) stays below 2^31."""
    return W3_ATOMS * Hy * KXP * 8


def spectra_bytes(geometry, n_call=None):
    """Row spectra of H of one call: N * M * Hy * KXP * 8 bytes."""
    N, _, _, M, _ = geometry
    Hy = fd._dims(geometry)[4]
    return (N if n_call is None else n_call) * M * Hy * fd.make_layout(geometry, 'f', 'hybrid').KXP * 8


def w3_takes(geometry, dtype='f', n_call=None):
    """fft_mixed.hip  mixed_grad_W3_takes, behind use_mixed(): float32, one channel, 2-D, atoms up to 12 rows, the span,
    and at least W3_MIN_BYTES of row spectra."""
    C = geometry[1]
    Ay, Hy = fd._dims(geometry)[2], fd._dims(geometry)[4]
    if not (fd.fft_has(geometry, dtype) and fd.mixed_has_grad_W(geometry, dtype)):
        return False
    KXP = fd.make_layout(geometry, dtype, 'hybrid').KXP
    return (C == 1 and Ay <= W3_MAX_AY and not fd.one_d(geometry) and w3_span(Hy, KXP) < 1 << 31
            and spectra_bytes(geometry, n_call) >= W3_MIN_BYTES)


def w3_groups(N, M, Ay, KX, num_cu=fd.NUM_CU):
    """fft.hip  mix_groups_w3 and the lines of fft_grad_W that follow it -> (groups, nper)."""
    slots3 = w3_waves(Ay) * num_cu
    per_group = fd.cdiv(M, W3_ATOMS) * fd.cdiv(KX, 16)
    best, best_cost = 1, 1e30
    for cand in range(min(N, fd.MIX_MAX_GROUPS), 0, -1):
        ng = fd.cdiv(N, fd.cdiv(N, cand))
        rounds = per_group * ng / slots3
        whole = 1.0 if rounds <= 1.0 else float(int(rounds + 0.999999))
        cost3 = whole / rounds + 0.03 * ng / 32.0
        if cost3 < best_cost - 1e-9:
            best, best_cost = ng, cost3
    nper = fd.cdiv(N, best)
    return fd.cdiv(N, nper), nper


def w3_grid(geometry, n_call=None):
    """(atom blocks, kx tiles, groups, nper) of the launch."""
    N, _, _, M, _ = geometry
    n = N if n_call is None else n_call
    KX = fd.make_layout(geometry, 'f', 'hybrid').KX
    ng, nper = w3_groups(n, M, fd._dims(geometry)[2], KX)
    return fd.cdiv(M, W3_ATOMS), fd.cdiv(KX, 16), ng, nper


def grad_W_kernel(geometry, n_call=None):
    """The kernel the mixed W gradient of a float32 call runs on (None: not a mixed call)."""
    if w3_takes(geometry, 'f', n_call):
        return 'k_mix_grad_W3'
    names = {i[0] for i in fd.cells(geometry, 'f', 'hybrid', n_call=n_call) if i[0].startswith('k_mix_grad_W')}
    assert len(names) <= 1
    return names.pop() if names else None


def edges(geometry, n_call=None):
    """The edge classes of k_mix_grad_W3 a call meets."""
    N, _, _, M, _ = geometry
    n = N if n_call is None else n_call
    Dy, _, Ay = fd._dims(geometry)[:3]
    lay = fd.make_layout(geometry, 'f', 'hybrid')
    gx, gy, ng, nper = w3_grid(geometry, n_call)
    out = {'ay_%d' % Ay}
    if M % W3_ATOMS:
        out.add('atom_tail')            # atom slots past M: clamped, not stored
    if gx > 1:
        out.add('atom_blocks')          # more than one block of 16 atoms: descriptor bases off atom 0
    if lay.KX % 16:
        out.add('kx_tail')              # partial last kx tile: clamped, not stored
    if nper > 1:
        out.add('samples_per_group')    # the V^/R^ chunk stream runs on into the next sample
    if nper > 1 and Dy > W3_CHUNK:
        out.add('chunks_across_samples')   # ... after the last of several chunks, into the other LDS buffer
    if n % nper:
        out.add('nper_tail')            # the last group holds fewer samples
    if Dy % W3_CHUNK:
        out.add('rows_tail')            # the last chunk of a plane leaves the ring period early
    if Dy < W3_CHUNK:
        out.add('rows_short')           # fewer rows than one ring period / LDS chunk
    if Dy > W3_CHUNK:
        out.add('chunks')               # more than one chunk per plane: both LDS buffers
    if (gx * gy * ng) % 8:
        out.add('xcd_remainder')        # workgroups past the last whole multiple of eight keep their place
    if n_call is not None and n_call < N:
        out.add('slice')                # a slice of the bound samples: bases off the binding's start
    return out


# the GPU cases: (N, C, D, M, A) of the bound problem, samples per call (None: all)
CASES = {
    'atom_tail_ay12': ((47, 1, (52, 70), 17, (12, 12)), None),
    'two_blocks_ay9': ((33, 1, (40, 120), 32, (9, 9)), None),
    'short_planes_ay5': ((130, 1, (5, 250), 19, (5, 8)), None),
    'ay1_rows81': ((51, 1, (81, 47), 16, (1, 3)), None),
    'slices_of_a_binding': ((141, 1, (52, 70), 17, (12, 12)), 47),
    # (more than 128 samples of more than one chunk each: the chunk stream crosses from a sample into the next)
    'two_samples_per_group_ay3': ((130, 1, (20, 30), 35, (3, 3)), None),
}
EDGES = ('ay_1', 'ay_5', 'ay_9', 'ay_12', 'atom_tail', 'atom_blocks', 'kx_tail', 'samples_per_group',
         'chunks_across_samples', 'ay_3', 'nper_tail', 'rows_tail', 'rows_short', 'chunks', 'xcd_remainder', 'slice')
