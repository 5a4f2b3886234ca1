"""
CPU guard of k_mix_reconstruct_sh's dispatch: the host mirror (tests/mix_reconstruct_sh_dispatch.py) is held to the C++
lines it restates, every geometry of the FFT matrix (tests/fft_dispatch.py: MATRIX) and every case of the W gradient's
large-call kernel below the threshold is shown to stay on the kernel the older mirror and the GPU matrix say it runs on, and
the cases of tests/test_hip_mix_reconstruct_sh.py are held to crossing the threshold and to meeting every edge of the new
kernel between them.  No GPU, no build: the sources are read as text.
"""
import os

import fft_dispatch as fd
import mix_grad_w3_dispatch as w3
import mix_reconstruct_sh_dispatch as rsh
import test_hip_parity as old
from conftest import ROOT

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_mirror_restates_the_sources():
    """The constants, the selection rule, the launch and the kernel's shape as the mirror restates them."""
    hdr = _read('fft.h')
    for line in ('#define TNMF_MIX_RSH_STRIPS %d' % rsh.RSH_STRIPS,
                 '#define TNMF_MIX_RSH_TILES %d' % rsh.RSH_TILES,
                 '#define TNMF_MIX_RSH_PER_CU %d' % rsh.RSH_PER_CU,
                 'constexpr int kMixRShStrips = TNMF_MIX_RSH_STRIPS, kMixRShTiles = TNMF_MIX_RSH_TILES, kMixRShPerCU = TNMF_MIX_RSH_PER_CU;',
                 'constexpr int kMixRShWaves = kMixRShPerCU * kMixRShStrips / 16, kMixRShMaxAy = %d;' % rsh.RSH_MAX_AY,
                 'constexpr long kMixRShMinBytes = 24L << 20;',
                 'return kMixRShTiles * (((16 * kMixRShStrips + Ay - 1) * 17 + 1) / 2 * 2 + Ay * 16) * 8u;',
                 'constexpr int mix_rsh_waves(int Ay) { return kMixRShWaves; }',
                 'bool mixed_reconstruct_sh_takes(const Geo &g, int KXP);'):
        assert line in hdr, line
    assert rsh.RSH_MIN_BYTES == 24 << 20 == w3.W3_MIN_BYTES
    mixed = _read('fft_mixed.hip')
    for line in ('const long plane = (long)g.Hy * KXP * 8;',
                 'const long spectra = (long)g.N * g.M * g.Hy * KXP * 8;',
                 'return g.C == 1 && g.Ay <= kMixRShMaxAy && !(g.Dy == 1 && g.Ay == 1) && plane < (1L << 31) && spectra >= kMixRShMinBytes;',
                 '#ifdef TNMF_MIX_NO_RSH',
                 'if constexpr (AY <= kMixRShMaxAy) {',
                 'if (mixed_reconstruct_sh_takes(g, KXP)) {',
                 'hipLaunchKernelGGL((k_mix_reconstruct_sh<T, AY, kMixRShStrips, kMixRShTiles>),',
                 'dim3(tiles, (unsigned)cdiv(g.Dy, 16 * kMixRShStrips), (unsigned)g.N),',
                 'constexpr unsigned tiles_lds = mix_rsh_lds_bytes(AY), hold = (160u << 10) / (kMixRShPerCU + 1) + 1;',
                 'dim3(kMixCols * kMixRShStrips), tiles_lds < hold ? hold - tiles_lds : 0u, s,',
                 '__global__ __launch_bounds__(kMixCols *STRIPS, kMixRShWaves) TNMF_MIX_NO_DS_PAIRING void k_mix_reconstruct_sh(',
                 'constexpr int S = %d, NT = kMixCols * STRIPS, ROWS = S * STRIPS + AY - 1, PITCH = kMixCols + 1;' % rsh.RSH_S,
                 'constexpr int TROWS = (ROWS * PITCH + 1) / 2 * 2, TILE = TROWS + AY * kMixCols;',
                 '__shared__ __align__(16) cplx<T> tile[TILES][TILE];'):
        assert line in mixed, line
    # one rule of its own, asked once; the W gradient's rule is not involved (tests/test_mix_grad_w3_dispatch_cpu.py counts it)
    assert mixed.count('mixed_reconstruct_sh_takes(') == 2 and 'mixed_reconstruct_sh_takes(' not in _read('fft.hip')
    rule = mixed[mixed.index('bool mixed_reconstruct_sh_takes('):mixed.index('int mixed_reconstruct(')]
    assert 'mixed_grad_W3_takes' not in rule
    # the new branch comes after the 1-D form and before the register forms, which are what they were
    launch = mixed[mixed.index('int launch_mix_reconstruct('):mixed.index('// ---- W gradient')]
    assert launch.index('k_mix_reconstruct_1d<T, 3, SAMPLES>') < launch.index('if (mixed_reconstruct_sh_takes(g, KXP)) {') \
        < launch.index('constexpr int S = 16, STRIPS = 8;') < launch.index('hipLaunchKernelGGL((k_mix_reconstruct<T, AY, 1, S, STRIPS>)') \
        < launch.index('constexpr int S = 8, STRIPS = 8;') < launch.index('hipLaunchKernelGGL((k_mix_reconstruct<T, AY, 3, S, STRIPS>)')


def test_occupancy_the_header_states():
    """One tile of the tallest atom is the 37 856 bytes the compiler reports; topped up by the launch, three workgroups of
    four waves fit a CU's 160 KiB and a fourth does not, for every atom height: three waves per SIMD, which is what
    __launch_bounds__ asks for.  At config 3 the grid is then a whole number of rounds."""
    assert rsh.lds_bytes(12) == 37856 and all(rsh.lds_bytes(a) <= rsh.lds_bytes(12) for a in range(1, 13))
    assert all(rsh.workgroups_per_cu(a) == rsh.RSH_PER_CU for a in range(1, 13))
    assert rsh.RSH_STRIPS * fd.MIX_COLS == 4 * 64            # a wave per SIMD and workgroup
    gx, gy, n = rsh.rsh_grid((256, 1, (256, 256), 32, (12, 12)))
    assert (gx, gy, n) == (9, 1, 256) and gx * gy * n == 3 * (rsh.RSH_PER_CU * fd.NUM_CU)


def _older_shapes():
    shapes = [(g, None) for g in fd.MATRIX.values()] + [(g, 1) for g in fd.MATRIX.values()]
    shapes += [(tuple(s[:5]), None) for s in old.FFT_SHAPES + old.HYBRID_SHAPES + old.ONE_D_SHAPES + old.SHAPES]
    return shapes


def test_older_geometries_stay_on_their_kernels():
    """Every geometry of MATRIX, whole and in one-sample slices, and every shape of the older lists stays below the
    threshold, so the mirror of tests/fft_dispatch.py and the GPU matrix keep describing what runs; the cases of
    tests/mix_grad_w3_dispatch.py are taken exactly when they reach the (common) threshold."""
    for g, n in _older_shapes():
        assert not rsh.rsh_takes(g, 'f', n), (g, n)
        if fd.fft_has(g, 'f') and fd.mixed_has_reconstruct(g, 'f'):
            assert rsh.reconstruct_kernel(g, n) in ('k_mix_reconstruct', 'k_mix_reconstruct_1d'), g
    cand = {k: rsh.spectra_bytes(g) for k, g in fd.MATRIX.items()
            if g[1] == 1 and not fd.one_d(g) and fd._dims(g)[2] <= rsh.RSH_MAX_AY and fd.fft_has(g, 'f')}
    top = max(cand, key=cand.get)
    assert top == 'y576_c1_x540' and cand[top] == 14622720 < rsh.RSH_MIN_BYTES
    for cid, (g, n) in w3.CASES.items():
        below = w3.spectra_bytes(g, n) < rsh.RSH_MIN_BYTES
        assert rsh.rsh_takes(g, 'f', n) == (not below), cid
        for k in range(1, (g[0] if n is None else n) + 1):
            if w3.spectra_bytes(g, k) < rsh.RSH_MIN_BYTES:
                assert not rsh.rsh_takes(g, 'f', k), (cid, k)


def test_baseline_configurations():
    """Config 3 (256 x 1 x 256^2, 32 atoms 12 x 12) is taken from the sample count where its spectra cross the threshold:
    9.8 MB per sample, three samples; configs 4 and 5 (three channels) never, at any sample count."""
    c2, c3, c4, c5 = old.BASELINE_SHAPES
    per_sample = rsh.spectra_bytes((1,) + tuple(c3))
    assert per_sample == 32 * 267 * 144 * 8
    first = fd.cdiv(rsh.RSH_MIN_BYTES, per_sample)
    assert first == 3
    for n in range(1, 300):
        assert rsh.rsh_takes((n,) + tuple(c3)) == (n >= first), n
        assert not rsh.rsh_takes((n,) + tuple(c4)) and not rsh.rsh_takes((n,) + tuple(c5)), n
    assert rsh.rsh_grid((256,) + tuple(c3)) == (9, 1, 256)
    assert [rsh.rsh_takes((n,) + tuple(c2)) for n in (2, 16, 19)] == [False, False, True]


def test_gpu_cases_cross_the_threshold_and_meet_every_edge():
    """Each case of tests/test_hip_mix_reconstruct_sh.py runs k_mix_reconstruct_sh -- none by more than a third of the
    threshold, so the oracle's work stays small -- and between them they meet every edge class of the kernel."""
    met = set()
    for cid, (g, n) in rsh.CASES.items():
        assert rsh.reconstruct_kernel(g, n) == 'k_mix_reconstruct_sh', cid
        assert rsh.RSH_MIN_BYTES <= rsh.spectra_bytes(g, n) < rsh.RSH_MIN_BYTES * 4 // 3, cid
        assert fd.family(g, 'f', 'hybrid', 'reconstruct') == 'fft', cid
        assert rsh.reconstruct_kernel(g, rsh.under_threshold(g, n)) == 'k_mix_reconstruct', cid
        met |= rsh.edges(g, n)
    assert met == set(rsh.EDGES), (met ^ set(rsh.EDGES))
    e = {cid: rsh.edges(g, n) for cid, (g, n) in rsh.CASES.items()}
    # the edges the issue names for its cases
    assert {'ay_12', 'kx_tail', 'row_blocks', 'row_block_short', 'rows_past_plane', 'atoms_tail', 'atoms_odd'} <= e['ay12_two_blocks_m9']
    assert fd.make_layout(rsh.CASES['ay12_two_blocks_m9'][0], 'f', 'hybrid').KX == 73
    assert {'ay_9', 'rows_short', 'atoms_few', 'rows_past_plane'} <= e['ay9_short_plane_m5']
    assert {'ay_5', 'rows_whole', 'atoms_even'} <= e['ay5_one_block_m12'] and 'row_blocks' not in e['ay5_one_block_m12']
    assert {'ay_1', 'rows_tail', 'row_blocks', 'row_block_short'} <= e['ay1_rows258_m16']
    assert 'slice' in e['slices_of_a_binding'] and rsh.CASES['slices_of_a_binding'][0][0] == 3 * 15
    # one sample fewer and the first case falls back to k_mix_reconstruct
    g = rsh.CASES['ay12_two_blocks_m9'][0]
    assert rsh.reconstruct_kernel((14,) + g[1:]) == 'k_mix_reconstruct'
