"""
CPU guard of k_mix_grad_W3's dispatch: the host mirror (tests/mix_grad_w3_dispatch.py) is held to the C++ lines it
restates, every geometry of the FFT matrix (tests/fft_dispatch.py: MATRIX) is shown to stay on the kernel the older mirror
and the GPU matrix say it runs on, and the cases of tests/test_hip_mix_grad_w3.py are held to crossing the threshold and to
meeting every edge of the new kernel between them.  No GPU, no build: the sources are read as text.
"""
import os

import fft_dispatch as fd
import mix_grad_w3_dispatch as w3
import test_hip_parity as old
from conftest import ROOT

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_mirror_restates_the_sources():
    """The constants, the selection rule, the group-count rule and the launch as the mirror restates them."""
    hdr = _read('fft.h')
    for line in ('#define TNMF_MIX_W3_WAVES 3',
                 'constexpr int kMixW3Atoms = %d, kMixW3Waves = TNMF_MIX_W3_WAVES, kMixW3MaxAy = %d;' % (w3.W3_ATOMS, w3.W3_MAX_AY),
                 'constexpr long kMixW3MinBytes = 24L << 20;',
                 'const int w = Ay >= 8 ? 3 : (Ay >= 4 ? 4 : (Ay >= 2 ? 5 : 7));',
                 'return kMixW3Waves < 3 ? kMixW3Waves : w;'):
        assert line in hdr, line
    assert w3.W3_MIN_BYTES == 24 << 20 and [w3.w3_waves(a) for a in range(1, 13)] == [7, 5, 5, 4, 4, 4, 4, 3, 3, 3, 3, 3]
    mixed = _read('fft_mixed.hip')
    for line in ('const long span = (long)kMixW3Atoms * g.Hy * KXP * 8;',
                 'const long spectra = (long)g.N * g.M * g.Hy * KXP * 8;',
                 'return g.C == 1 && g.Ay <= kMixW3MaxAy && !(g.Dy == 1 && g.Ay == 1) && span < (1L << 31) && spectra >= kMixW3MinBytes;',
                 'if constexpr (AY <= kMixW3MaxAy) {',
                 'if (mixed_grad_W3_takes(g, KXP)) {',
                 'const int gx = cdiv(g.M, kMixW3Atoms), gy = cdiv(KX, kMixCols), gz = ngroups;',
                 'hipLaunchKernelGGL((k_mix_grad_W3<T, AY>), dim3((unsigned)(gx * gy * gz)), dim3(kMixCols * kMixW3Atoms),',
                 '__global__ __launch_bounds__(kMixCols *kMixW3Atoms, kMixW3Waves) TNMF_MIX_NO_DS_PAIRING void k_mix_grad_W3(',
                 'constexpr int NA = kMixW3Atoms, RS = %d, CH = RS, NT = kMixCols * NA;' % w3.W3_CHUNK,
                 'static_assert(AY + 4 <= RS && sizeof(cplx<T>) == 8 && NT == 2 * CH * (kMixCols / 2), "ring depth, float spectra");'):
        assert line in mixed, line
    # the new branch comes first and falls through to the older kernels; the 1-D form is decided before either
    launch = mixed[mixed.index('int launch_mix_grad_W('):]
    assert launch.index('k_mix_grad_W_1d<T, 4, GROUPS>') < launch.index('if (mixed_grad_W3_takes(g, KXP)) {') \
        < launch.index('hipLaunchKernelGGL((k_mix_grad_W2<T, AY, GROUPS>)') < launch.index('hipLaunchKernelGGL((k_mix_grad_W<T, AY, 1, GROUPS>)')
    src = _read('fft.hip')
    for line in ('const long slots3 = (long)mix_w3_waves(g.Ay) * (ctx->num_cu > 0 ? ctx->num_cu : 256);',
                 'const long per_group = (long)cdiv(g.M, kMixW3Atoms) * cdiv(l.KX, 16);',
                 'for (int cand = g.N < kMixMaxGroups ? g.N : kMixMaxGroups; cand >= 1; --cand) {',
                 'const int ng = cdiv(g.N, cdiv(g.N, cand));',
                 'const double rounds = (double)(per_group * ng) / (double)slots3;',
                 'const double cost3 = whole / rounds + 0.03 * ng / 32.0;',
                 'int nparts = ngpad, nper_call = nper;',
                 'if (mixed_grad_W3_takes(g, l.KXP)) {',
                 'nper_call = cdiv(g.N, mix_groups_w3(ctx, g, l));',
                 'nparts = cdiv(g.N, nper_call);',
                 'CHECK(mixed_grad_W(g, c.T, c.VT, c.RT, at(ctx, l.Gn), at(ctx, l.Gp), l.KX, l.KXP, nparts, nper_call, s));'):
        assert line in src, line
    assert src.count('mixed_grad_W3_takes(') == 1 and mixed.count('mixed_grad_W3_takes(') == 2   # one rule, asked twice
    # mix_groups() and the older kernels' group lines are what they were (tests/test_fft_dispatch_cpu.py pins them too)
    assert 'const long slots = 2L * 4 * (ctx->num_cu > 0 ? ctx->num_cu : 256);' in src
    assert 'const int ngpad = (int)align_up((size_t)ng, 4);' in src


def test_group_rule_fills_the_chip_at_the_flagship_shape():
    """Config 3 (256 x 1 x 256^2, 32 atoms 12 x 12): 2 atom blocks x 9 kx tiles x 128 groups = 2304 workgroups = three
    rounds of 3 x 256 resident ones; the partial sums fit the kMixMaxGroups slots of the workspace for any call."""
    g3 = (256, 1, (256, 256), 32, (12, 12))
    assert w3.w3_takes(g3) and w3.w3_grid(g3) == (2, 9, 128, 2)
    assert 2 * 9 * 128 == 3 * (w3.w3_waves(12) * fd.NUM_CU)
    for n in (1, 2, 3, 47, 128, 129, 130, 255, 256, 257, 1000):
        for M, Ay, KX in ((17, 12, 49), (32, 9, 73), (19, 5, 136), (16, 1, 33), (64, 12, 289)):
            ng, nper = w3.w3_groups(n, M, Ay, KX)
            assert 1 <= ng <= fd.MIX_MAX_GROUPS and ng == fd.cdiv(n, nper) and (ng - 1) * nper < n   # no group is empty


def _older_shapes():
    shapes = [(g, None) for g in fd.MATRIX.values()] + [(g, 1) for g in fd.MATRIX.values()]
    shapes += [(tuple(s[:5]), None) for s in old.FFT_SHAPES + old.HYBRID_SHAPES + old.ONE_D_SHAPES + old.SHAPES]
    return shapes


def test_matrix_geometries_stay_on_their_kernels():
    """Every geometry of MATRIX, whole and in one-sample slices, and every shape of the older lists that names no sample
    count of its own stays below the threshold: the mirror of tests/fft_dispatch.py and the GPU matrix keep describing what
    runs.  The largest one-channel geometry with atoms up to 12 rows is y576_c1_x540 at 14.6 MB; the threshold is 25.2 MB."""
    for g, n in _older_shapes():
        assert not w3.w3_takes(g, 'f', n), (g, n)
        if fd.fft_has(g, 'f') and fd.mixed_has_grad_W(g, 'f'):
            assert w3.grad_W_kernel(g, n) in ('k_mix_grad_W', 'k_mix_grad_W2', 'k_mix_grad_W_1d'), g
    cand = {k: w3.spectra_bytes(g) for k, g in fd.MATRIX.items()
            if g[1] == 1 and not fd.one_d(g) and fd._dims(g)[2] <= w3.W3_MAX_AY and fd.fft_has(g, 'f')}
    top = max(cand, key=cand.get)
    assert top == 'y576_c1_x540' and cand[top] == 14622720 < w3.W3_MIN_BYTES
    # the BASELINE geometries of tests/test_hip_parity.py / test_hip_scale.py: config 3 runs the new kernel from four samples
    # on (37 MB); config 2 (9 x 9 atoms, 128^2) does not at 2 or 16 samples; several channels and 16-row atoms never do
    c2, c3, c4, c5 = old.BASELINE_SHAPES
    assert [w3.w3_takes((n,) + tuple(c3)) for n in (2, 4, 16)] == [False, True, True]
    assert not any(w3.w3_takes((n,) + tuple(s)) for n in (2, 4, 16, 256) for s in (c4, c5))
    assert [w3.w3_takes((n,) + tuple(c2)) for n in (2, 16, 19)] == [False, False, True]


def test_gpu_cases_cross_the_threshold_and_meet_every_edge():
    """Each case of tests/test_hip_mix_grad_w3.py runs k_mix_grad_W3 -- none by more than a third of the threshold, so
    the oracle's work stays small -- and between them they meet every edge class of the kernel."""
    met = set()
    for cid, (g, n) in w3.CASES.items():
        assert w3.grad_W_kernel(g, n) == 'k_mix_grad_W3', cid
        assert w3.W3_MIN_BYTES <= w3.spectra_bytes(g, n) < w3.W3_MIN_BYTES * 4 // 3, cid
        assert fd.family(g, 'f', 'hybrid', 'grad_W') == 'fft', cid
        met |= w3.edges(g, n)
    assert met == set(w3.EDGES), (met ^ set(w3.EDGES))
    # the edges the issue names for its cases
    e = {cid: w3.edges(g, n) for cid, (g, n) in w3.CASES.items()}
    assert {'atom_tail', 'kx_tail', 'ay_12', 'rows_tail'} <= e['atom_tail_ay12'] and fd.make_layout(w3.CASES['atom_tail_ay12'][0], 'f', 'hybrid').KX == 49
    assert {'atom_blocks', 'ay_9'} <= e['two_blocks_ay9'] and fd.make_layout(w3.CASES['two_blocks_ay9'][0], 'f', 'hybrid').Lx == 144
    assert {'rows_short', 'ay_5', 'nper_tail', 'samples_per_group'} <= e['short_planes_ay5']
    assert fd.make_layout(w3.CASES['short_planes_ay5'][0], 'f', 'hybrid').Lx == 270
    assert {'ay_1', 'rows_tail', 'chunks'} <= e['ay1_rows81']
    assert 'slice' in e['slices_of_a_binding'] and w3.CASES['slices_of_a_binding'][0][0] == 3 * 47
    assert {'chunks_across_samples', 'ay_3'} <= e['two_samples_per_group_ay3']
    # two samples fewer and the first case falls back to k_mix_grad_W2
    g = w3.CASES['atom_tail_ay12'][0]
    assert w3.grad_W_kernel((45,) + g[1:]) == 'k_mix_grad_W2'
