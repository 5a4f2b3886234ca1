"""
CPU guard of the FFT kernel matrix: the host mirror of the dispatch (tests/fft_dispatch.py) is held to the C++ it restates,
the geometries of tests/test_hip_fft_matrix.py are held to reaching every kernel instance the product build can run and
every edge of every kernel, the tables of what cannot be reached are held to the source text, and the comparison helpers
of the GPU file are shown to fail on a shifted or mis-scaled result.  No GPU, no build: the sources are read as text.
"""
import os
import re

import numpy as np
import pytest

import fft_dispatch as fd
import test_hip_fft_matrix as gm
import test_hip_parity as old
from conftest import ROOT

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _ints(text):
    return tuple(int(v) for v in re.findall(r'\d+', text))


# ---- the mirror agrees with the sources ------------------------------------------------------------------------------------

def test_length_tables_agree():
    """The objects the Makefile builds, the declarations of fft.h, the lookup switch and the two length tables of fft.hip
    and the mirror's tuples are the same lists; a length missing from one of them fails here, not when a library with an
    undefined symbol is loaded."""
    src = _read('fft.hip')
    m = re.search(r'^FFTLENS\s*:=(.*)$', _read('Makefile'), re.M)
    assert m and _ints(m.group(1)) == fd.LENS_X
    assert _ints(re.search(r'const int kLensY\[\] = \{(.*?)\};', src).group(1)) == fd.LENS_Y
    assert _ints(re.search(r'const int kLensX\[\] = \{(.*?)\};', src).group(1)) == fd.LENS_X
    assert set(fd.LENS_X) - set(fd.LENS_Y) == {540}
    body = src[src.index('fft_run_fn lookup(int L)'):]
    body = body[:body.index('default:')]
    cases = re.findall(r'case (\d+): return fft_run_(\d+);', body)
    assert tuple(int(a) for a, _ in cases) == fd.LENS_X and all(a == b for a, b in cases)
    assert tuple(int(v) for v in re.findall(r'^TNMF_FFT_DECL\((\d+)\);', _read('fft.h'), re.M)) == fd.LENS_X
    assert 'if constexpr (L <= %d) return fft_run_typed<double, L>(op, a, s);' % fd.F64_MAX_LEN in _read('fft_len.hip')
    assert src.count('if (L >= h && (dtype == 0 || L <= %d)) return L;' % fd.F64_MAX_LEN) == 2
    assert 'bool tall_columns(const tnmf_hip_ctx *ctx) { return ctx->path != TNMF_PATH_FFT; }' in src
    assert 'constexpr int kMixMaxGroups = %d;' % fd.MIX_MAX_GROUPS in src


def test_mixed_dispatch_agrees():
    """MIX_SWITCH instantiates the atom heights 1..16 in float, the two-atom kernel stops at 12, and mixed_has_* admit one
    channel (1-D signals: three / four)."""
    src = _read('fft_mixed.hip')
    body = src[src.index('#define MIX_SWITCH(FN, ...)'):]
    body = body[:body.index('default: return TNMF_E_UNSUPPORTED;')]
    cases = re.findall(r'case (\d+): return FN<float, (\d+)>\(__VA_ARGS__\);', body)
    assert [int(a) for a, _ in cases] == list(range(1, fd.MIX_MAX_AY + 1)) and all(a == b for a, b in cases)
    assert body.count('case ') == fd.MIX_MAX_AY
    for line in ('return dtype == 0 && g.Ay <= 16 && (g.C == 1 || (g.Dy == 1 && g.Ay == 1 && g.C <= 3));',
                 'return dtype == 0 && g.Ay <= 16 && (g.C == 1 || (g.Dy == 1 && g.Ay == 1 && g.C <= 4));',
                 'constexpr int kMixCols = 16;',
                 'constexpr int GROUPS = 4;',
                 'if constexpr (AY <= 12) {',
                 'const long span = ((long)(GROUPS - 1) * nper * g.M + 2) * g.Hy * KXP * 8;',
                 'if (g.C == 1 && span < (1L << 31)) {',
                 'constexpr int MA = 2, VS = 8, RS = (AY + 4 + VS - 1) / VS * VS, P = VS - 1;',
                 'for (int yb = 0; yb < Dy; yb += AY) {',
                 'constexpr int SAMPLES = 16;',
                 'constexpr int S = 16, STRIPS = 8;',
                 'constexpr int S = 8, STRIPS = 8;',
                 'hipLaunchKernelGGL((k_mix_reconstruct_1d<T, 3, SAMPLES>)',
                 'hipLaunchKernelGGL((k_mix_reconstruct<T, AY, 1, S, STRIPS>)',
                 'hipLaunchKernelGGL((k_mix_grad_W_1d<T, 4, GROUPS>)',
                 'hipLaunchKernelGGL((k_mix_grad_W2<T, AY, GROUPS>)',
                 'hipLaunchKernelGGL((k_mix_grad_W<T, AY, 1, GROUPS>)'):
        assert line in src, line
    assert (fd.MIX_MAX_AY, fd.MIX_W2_MAX_AY, fd.MIX_R_1D_MAX_C, fd.MIX_W_1D_MAX_C, fd.MIX_COLS, fd.MIX_GROUPS) == (16, 12, 3, 4, 16, 4)
    assert fd.MIX_STRIP_ROWS == {1: 128, 3: 64}


def test_lencfg_and_ladders_agree():
    """The LenCfg<L> constants, the per-dtype tile rules and the channel ladders of fft_run_typed as the mirror restates
    them, and the mirror's values for every length."""
    src = _read('fft_kernels.h')
    for line in ('static constexpr int col_tile = L > 384 ? 8 : 16;',
                 'static constexpr int col_threads = (L == 270 || L == 540) ? 480 : (L > 192 ? 512 : 256);',
                 'static constexpr int col_elems = L * col_tile / col_threads;',
                 'static constexpr int row_pairs = L > 288 ? 8 : 16;',
                 'static constexpr int row_threads = 256;',
                 'static constexpr int mu_pairs = L > 288 ? 4 : 8;',
                 'static constexpr int mu_threads = L / 2 + 1 > 256 ? 512 : 256;',
                 'static constexpr int v = WIDE ? 16 : LenCfg<L>::col_tile;',
                 'constexpr int NB = (sizeof(T) == 8 && L > 144) ? Cfg::row_pairs / 2 : Cfg::row_pairs;',
                 'constexpr int NBM = (sizeof(T) == 8 && L > 144) ? Cfg::mu_pairs / 2 : Cfg::mu_pairs;',
                 'if ((op == kFftRowsFwd || op == kFftRowsInv) && a->rows == 1 && a->planes > 1) {',
                 'const dim3 rgrid((unsigned)cdiv(a->rows, 2 * NB), (unsigned)a->planes);',
                 'const int cg = a->C <= 3 ? a->C : 4;',
                 'const int cg = a->C <= 2 ? a->C : (Cfg::col_elems <= 9 ? 3 : 2);',
                 'const dim3 grid((unsigned)a->planes, wide_tiles, 2u * (unsigned)a->mgroups);'):
        assert line in src, line
    ladder = src[src.index('case kFftGradH: {'):src.index('case kFftGradW: {')]
    assert re.findall(r'if \(a->C == (\d)\) TNMF_FFT_LAUNCH\(\(k_fft_grad_H<T, L, NTC, (\d)>\)', ladder) == [(str(c), str(c)) for c in (1, 2, 3, 4)]
    assert ladder.count('k_fft_grad_H<') == 5 and 'TNMF_FFT_LAUNCH((k_fft_grad_H<T, L, NTC, 0>), grid, NTC, wide_lds);' in ladder
    assert [fd.grad_H_class(c) for c in range(1, 8)] == [1, 2, 3, 4, 0, 0, 0] and set(fd.GRAD_H_CLASSES) == {0, 1, 2, 3, 4}
    assert [fd.contract_R_cg(c) for c in range(1, 7)] == [1, 2, 3, 4, 4, 4]
    assert [fd.grad_W_cg(c, 288) for c in range(1, 6)] == [1, 2, 3, 3, 3] and [fd.grad_W_cg(c, 384) for c in range(1, 6)] == [1, 2, 2, 2, 2]
    assert [fd.spectral_cg(c) for c in range(1, 7)] == [1, 2, 3, 4, 4, 4]
    want = {  # L: col_tile, col_threads, col_elems, row_pairs, mu_pairs, mu_threads
        32: (16, 256, 2, 16, 8, 256), 48: (16, 256, 3, 16, 8, 256), 64: (16, 256, 4, 16, 8, 256),
        96: (16, 256, 6, 16, 8, 256), 144: (16, 256, 9, 16, 8, 256), 192: (16, 256, 12, 16, 8, 256),
        270: (16, 480, 9, 16, 8, 256), 288: (16, 512, 9, 16, 8, 256), 384: (16, 512, 12, 8, 4, 256),
        540: (8, 480, 9, 8, 4, 512), 576: (8, 512, 9, 8, 4, 512)}
    for L in fd.LENS_X:
        c = fd.LenCfg(L)
        assert (c.col_tile, c.col_threads, c.col_elems, c.row_pairs, c.mu_pairs, c.mu_threads) == want[L], L
        assert (c.NB('f'), c.NB('d')) == (c.row_pairs, c.row_pairs // 2 if L > 144 else c.row_pairs)
        assert (L // 2 + 1) % 16 != 0 and ((L // 2 + 1) % 8 != 0 or c.col_tile == 16), 'the last kx tile is always partial'
    spec = _read('fft_spectral.hip')
    for line in ('constexpr int kSpecThreads = 256;', 'constexpr int kSpecCG = 4;', 'constexpr int kSpecNS = 4;',
                 'constexpr int kSpecMS = 4;', 'const int cg = g.C < kSpecCG ? g.C : kSpecCG;'):
        assert line in spec, line
    assert spec.count('const int cg = g.C < kSpecCG ? g.C : kSpecCG;') == 2
    for macro in ('SPEC_R', 'SPEC_G'):
        assert re.findall(r'case (\d): %s\(T, (\d)\); break;' % macro, spec) == [('1', '1'), ('2', '2'), ('3', '3')]
        assert 'default: %s(T, 4); break;' % macro in spec


def test_layout_and_dispatch_rules_are_those_of_the_source():
    """The lines of fft.hip and api.hip the mirror restates.  When one of them changes, tests/fft_dispatch.py and the
    matrix's geometries have to be looked at again."""
    src = _read('fft.hip')
    for line in ('int ng = cdiv(2048, g.M * tiles);',
                 'if (ng > 16) ng = 16;',
                 'l->Ly = pick_len(g.Hy, dtype, false, tall_columns(ctx));',
                 'l->Lx = pick_len(g.Hx, dtype, true);',
                 'l->KX = l->Lx / 2 + 1;',
                 'l->KXP = (int)align_up((size_t)l->KX, 16);',
                 'const int tiles = cdiv(l->KX, l->Ly > 384 ? 8 : 16);',
                 'size_t budget = (size_t)8 << 30;',
                 'long chunk_full = (long)(budget / (2 * l->sT));',
                 'l->sT = (size_t)g.M * g.Hy * kxp * c;',
                 'int mg = cdiv(1024, l->chunk * cdiv(l->KX, 16) * 2);',
                 'l->mper = cdiv(g.M, mg);',
                 'l->resident = !(use_mixed(g, dtype, false) && use_mixed(g, dtype, true));',
                 'return !off && (grad_W ? mixed_has_grad_W(g, dtype) : mixed_has_reconstruct(g, dtype));',
                 'return l.resident && !off;',
                 'return pick_len(g.Hx, dtype, true) != 0 && mixed_has_reconstruct(g, dtype) && mixed_has_grad_W(g, dtype);',
                 'return pick_len(g.Hy, dtype, false) != 0 && pick_len(g.Hx, dtype, true) != 0;',
                 'const long slots = 2L * 4 * (ctx->num_cu > 0 ? ctx->num_cu : 256);',
                 'const long per_group_block = (long)(g.C == 1 && g.Ay <= 12 ? cdiv(g.M, 2) : g.M) * cdiv(l.KX, 16);',
                 'for (int cand = 32; cand <= kMixMaxGroups; cand *= 2) {',
                 'const double cost = whole / rounds + 0.03 * (cand / 32);',
                 'const int ngpad = (int)align_up((size_t)ng, 4);',
                 'const long blocks = (long)cdiv(g.M, 4) * (((long)l.Ly * l.KXP + 255) / 256) * cdiv(g.C, 4);',
                 'int ng = (int)((8L * ctx->num_cu + blocks - 1) / blocks);',
                 'for (int n0 = 0; n0 < g.N; n0 += l.chunk) {'):
        assert line in src, line
    assert src.count('if (g.Dy == 1 && g.Ay == 1) return TNMF_E_UNSUPPORTED;') == 2   # fft_grad_H, fft_update_H
    api = _read('api.hip')
    for line in ('if (ctx->path == TNMF_PATH_HYBRID) return fft_has(g, dtype);',
                 'return (size_t)g.N * g.M * g.Hy * g.Hx >= ((size_t)1 << 19);',
                 'return fused ? fft_update_H(ctx, g, dtype, V, R, W, Hio, reg, s) : fft_grad_H(ctx, g, dtype, V, R, W, neg, pos, s);',
                 'return ctx->path == TNMF_PATH_FFT || use_fft_hybrid(ctx, g, dtype);'):
        assert line in api, line


def test_mirror_values_at_the_baseline_geometries():
    """Figures the sources quote, from the mirror: the transform lengths of the BASELINE shift widths (267, 527), the
    padded spectrum rows, and the 540-long columns of the default dispatch."""
    g5 = (4, 3, (512, 512), 64, (16, 16))
    assert fd.make_layout(g5, 'f', 'fft')[:4] == (576, 540, 271, 272)
    assert fd.make_layout(g5, 'f', 'hybrid')[:4] == (540, 540, 271, 272)
    g3 = (4, 1, (256, 256), 32, (12, 12))
    assert fd.make_layout(g3, 'f', 'fft')[:4] == (270, 270, 136, 144)
    assert fd.make_layout(g3, 'd', 'fft')[:4] == (270, 270, 136, 144) and not fd.fft_has(g5, 'd')
    assert not fd.make_layout(g3, 'f', 'hybrid').resident and fd.make_layout(g5, 'f', 'hybrid').resident
    assert fd.make_layout(g3, 'd', 'hybrid').resident


# ---- what cannot be reached ---------------------------------------------------------------------------------------------------

def _block_after(text, start):
    """(begin, end) of the brace block that opens at the first '{' at or after `start`."""
    i = text.index('{', start)
    depth = 0
    for j in range(i, len(text)):
        depth += (text[j] == '{') - (text[j] == '}')
        if depth == 0:
            return i, j
    raise AssertionError('unbalanced braces')


def _function_body(text, signature):
    return text[slice(*_block_after(text, text.index(signature)))]


def test_unreachable_instances_sit_behind_diagnostic_reads():
    """UNREACHABLE holds only what a tnmf_diag_env() read decides, and the product build compiles that read to "unset":
    every launch of kFftContractR / kFftGradW is in the else branch of `if (use_resident(l))`, use_resident() is
    `l.resident && !off` with `off` a tnmf_diag_env read, and the branches are entered only when the mixed form of the
    same primitive does not take the problem -- in which case Lay::resident is true (checked over a grid of shapes)."""
    common = _read('common.h')
    diag, product = common[common.index('#ifdef TNMF_DIAG'):].split('#else')[:2]
    assert 'tnmf_diag_env(const char *name) { return getenv(name); }' in diag
    assert 'static inline const char *tnmf_diag_env(const char *) { return nullptr; }' in product[:product.index('#endif')]
    src = _read('fft.hip')
    for key, ent in fd.UNREACHABLE.items():
        guard = _function_body(src, {'use_resident': 'bool use_resident(const Lay &l)', 'use_mixed': 'bool use_mixed(const Geo &g, int dtype, bool grad_W) {',
                                     'fft_grad_W': 'int fft_grad_W('}[ent['guard']])
        reads = [ln for ln in guard.splitlines() if '"%s"' % ent['env'] in ln]
        assert len(reads) == 1 and 'tnmf_diag_env("%s")' % ent['env'] in reads[0], key
        assert src.count('"%s"' % ent['env']) == 1, key     # read nowhere else
        if not ent['op']:
            assert not ent['instances'](), key
            continue
        # every launch of the op: inside the else block of an `if (use_resident(l))`
        sites = [m.start() for m in re.finditer(r'colf\(%s\b' % ent['op'], src)]
        assert len(sites) == 1, (key, sites)
        elses = []
        for m in re.finditer(r'if \(use_resident\(l\)\) \{', src):
            _, end = _block_after(src, m.start())
            assert src[end:end + 8] == '} else {', src[end:end + 20]
            elses.append(_block_after(src, end + 1))
        assert len(elses) == 2 and sum(b < sites[0] < e for b, e in elses) == 1, key
        # the kernels are launched by that op alone
        kern = _read('fft_kernels.h')
        launches = [m.start() for m in re.finditer(r'TNMF_FFT_LAUNCH\(\(%s<' % key, kern)]
        case = kern.index('case %s: {' % ent['op'])
        assert launches and all(case < p < _block_after(kern, case)[1] for p in launches), key
        assert all(i[0] == key for i in ent['instances']())
    assert 'static const bool off = tnmf_diag_env("TNMF_FFT_NO_RESIDENT") != nullptr;' in _function_body(src, 'bool use_resident(const Lay &l)')
    # the else branches are entered only without the mixed form, and then the spectra are resident
    for C in range(1, 7):
        for A in ((1, 3), (5, 5), (16, 2), (17, 4)):
            for T in fd.DTYPES:
                g = (3, C, (30, 30), 4, A)
                if not (fd.mixed_has_reconstruct(g, T) and fd.mixed_has_grad_W(g, T)):
                    assert fd.make_layout(g, T, 'fft').resident
                assert fd.mixed_has_reconstruct(g, T) == fd.mixed_has_grad_W(g, T)   # 2-D: one rule
    # compiled for every length: what the diagnostic ops would launch
    assert len(fd.UNREACHABLE['k_fft_contract_R']['instances']()) == 4 * (11 + 8)
    assert len(fd.UNREACHABLE['k_fft_grad_W']['instances']()) == 2 * (11 + 8) + (9 + 7)   # cg = 3 where col_elems <= 9: not at 192 and 384


def test_not_covered_is_the_window_loop_and_the_span_fallback_and_nothing_else():
    """NOT_COVERED: the window loop of the H update (chunk < N) and the 2^31-byte fallback of launch_mix_grad_W.  The
    mirror confirms that no geometry of the matrix or of the older shape lists comes near either, and what it would take."""
    assert set(fd.NOT_COVERED) == {'h_update_window_loop', 'mix_grad_W_span_fallback'}
    shapes = list(fd.MATRIX.values()) + [tuple(s[:5]) for s in old.FFT_SHAPES + old.HYBRID_SHAPES + old.ONE_D_SHAPES + old.SHAPES]
    shapes += [(n,) + tuple(s) for s in old.BASELINE_SHAPES for n in (2, 4, 16)]
    # (the shard sizes of configs 4 and 5 that test_full_shard_sizes_of_configs_4_and_5 runs under the default dispatch)
    shapes += [(32, 3, (256, 256), 32, (12, 12)), (32, 3, (512, 512), 64, (16, 16))]
    for g in shapes:
        for T in fd.DTYPES:
            if not fd.fft_has(g, T):
                continue
            l = fd.make_layout(g, T, 'fft')
            assert l.chunk == g[0] and 2 * g[0] * l.sT <= fd.WINDOW_BUDGET, g
            if fd.mixed_has_grad_W(g, T) and not fd.one_d(g):
                _, nper, _ = fd.mix_groups(g[0], g[1], g[3], fd._dims(g)[2], l.KX)
                assert fd.mix_span(nper, g[3], fd._dims(g)[4], l.KXP) < 1 << 28, g    # an eighth of the limit at most
    # under the default dispatch the H update of a problem of any size is a direct kernel: the loop needs path='fft'
    assert fd.family((32, 3, (512, 512), 64, (16, 16)), 'f', 'hybrid', 'update_H') == 'direct'
    # what it takes: more than 8 GB of neg/pos row spectra; config 5 (Hy = 527, KXP = 272, 64 atoms) from 59 samples on
    g = (59, 3, (512, 512), 64, (16, 16))
    assert fd.make_layout(g, 'f', 'fft').chunk == 58 and fd.make_layout((58,) + g[1:], 'f', 'fft').chunk == 58
    # the span: nper * M >= 511 at the longest transforms (Hy = 576, KXP = 304)
    assert fd.mix_span(1, 510, 576, 304) < 1 << 31 <= fd.mix_span(1, 511, 576, 304)
    assert 511 * 576 * 304 * 8 * 128 > 50 << 30          # nper samples in each of 128 groups: > 50 GB of row spectra
    assert fd.NOT_COVERED['mix_grad_W_span_fallback']['instances']() == {('k_mix_grad_W', 'f', ay, 1, 4) for ay in range(1, 13)}


# ---- the matrix is complete ---------------------------------------------------------------------------------------------------

def test_universe_is_enumerated():
    """kernel x length x dtype x template class: 4 row kernels on 11 + 8 lengths, 2 plain column kernels likewise,
    k_fft_grad_H in 5 channel classes on 10 + 8 lengths, 2 spectral kernels x 4 channel groups x 2 dtypes, 3 helpers x 2, the
    mixed kernels (16 + 12 + 4 + 2), and the excused ones."""
    want = fd.universe() - fd.excused()
    count = lambda k: sum(1 for i in want if i[0] == k)  # noqa: E731
    assert [count(k) for k in fd.ROW_KERNELS] == [19] * 4 and [count(k) for k in fd.COL_KERNELS] == [19] * 2
    assert count('k_fft_grad_H') == 5 * 18 and count('k_spec_contract_R') == count('k_spec_grad_W') == 8
    assert (count('k_mix_reconstruct'), count('k_mix_grad_W2'), count('k_mix_grad_W')) == (16, 12, 4)
    assert len(want) == 260 and len(fd.universe()) == 260 + 76 + 48 + 12 + 6
    assert set(fd.EDGES) == {i[0] for i in want}


def test_matrix_reaches_every_instance_and_every_edge():
    """universe - UNREACHABLE - NOT_COVERED is exactly what MATRIX reaches over both dtypes and both paths, every edge
    class is met on every kernel it applies to (both tile widths of the column kernels included), and the fit edges on
    every transform length."""
    assert fd.coverage_gaps(fd.MATRIX) == []
    got = fd.reached(fd.MATRIX)
    assert set(got) == fd.universe() - fd.excused()
    for k in fd.COL_KERNELS:       # both tile widths, on both 8-wide lengths
        for L in (540, 576):
            assert 'kx_tail_8' in got[(k, 'f', L)] and fd.LenCfg(L).col_tile == 8
    print('%d geometries, %d instances, %d (instance, edge class) pairs' % (len(fd.MATRIX), len(got), sum(len(e) for e in got.values())))


@pytest.mark.parametrize('gid,lost', [
    ('y96_c5_x48', ["instance ('k_fft_grad_H', 'd', 96, 0)", "instance ('k_fft_grad_H', 'f', 96, 0)"]),
    ('tall_atoms_c1', ["instance ('k_spec_contract_R', 'f', 1)", "instance ('k_spec_grad_W', 'f', 1)"]),
    ('y576_c2b_x32', ['edge y_one_short on k_fft_cols_fwd<f, 540>', 'edge y_one_short on k_fft_cols_inv<f, 540>']),
    ('mix_a16_n129', ['edge nper_tail on k_mix_grad_W<f>', "instance ('k_mix_grad_W', 'f', 16, 1, 4)", "instance ('k_mix_reconstruct', 'f', 16, 1, 16, 8)"]),
])
def test_a_removed_geometry_is_missed_by_name(gid, lost):
    """Without a geometry that is the only one to reach something, the coverage check names the lost cells."""
    rest = {k: v for k, v in fd.MATRIX.items() if k != gid}
    assert fd.coverage_gaps(rest) == lost


def test_matrix_geometries_run_where_the_mirror_says():
    """The family takes every geometry in float32, the 1-D ones in float32 alone and with three channels at most, and
    float64 exactly where both lengths stay within 288; every 2-D geometry has an interior sample."""
    for gid, g in fd.MATRIX.items():
        assert fd.fft_has(g, 'f'), gid
        Hy, Hx = fd._dims(g)[4:]
        assert fd.fft_has(g, 'd') == (not fd.one_d(g) and max(Hy, Hx) <= 288), gid
        assert g[0] >= 3, gid
        for p in fd.PATHS:
            assert fd.family(g, 'f', p, 'grad_W') == fd.family(g, 'f', p, 'reconstruct') == 'fft'
        assert fd.family(g, 'f', 'hybrid', 'update_H') == 'direct'
        assert fd.family(g, 'f', 'fft', 'update_H') == ('refused' if fd.one_d(g) else 'fft')
    assert not fd.fft_has((3, 4, (100,), 4, (9,)), 'f') and fd.fft_has((3, 3, (100,), 4, (9,)), 'f')
    assert fd.mixed_has_grad_W((3, 4, (100,), 4, (9,)), 'f') and not fd.mixed_has_reconstruct((3, 4, (100,), 4, (9,)), 'f')
    assert len(gm.CASES) == sum(fd.fft_has(g, T) for g in fd.MATRIX.values() for T in fd.DTYPES) * 2


# ---- what the older shape lists reached -------------------------------------------------------------------------------------

def _old_lists():
    """(list name, geometry, dtypes, paths) as the tests of test_hip_parity.py run them on the FFT family."""
    for s in old.FFT_SHAPES:
        yield 'FFT_SHAPES', tuple(s[:5]), s[5], ('fft',)
    for s in old.HYBRID_SHAPES:
        yield 'HYBRID_SHAPES', tuple(s), 'f', ('hybrid',)
    for s in old.ONE_D_SHAPES:
        yield 'ONE_D_SHAPES', tuple(s), 'f', ('hybrid',)
    for s in old.BASELINE_SHAPES:
        yield 'BASELINE_SHAPES', (2,) + tuple(s), 'f', ('fft',)
        yield 'BASELINE_SHAPES', (16 if s[2] == 16 else 4,) + tuple(s), 'f', ('hybrid',)
    for s in old.SHAPES:                      # path='auto': the family only from 2^19 activations on
        if fd.use_fft_under_auto(tuple(s), 'f'):
            yield 'SHAPES', tuple(s), 'f', ('hybrid',)


def old_lists_reach():
    got = fd._Cells()
    for _, g, dtypes, paths in _old_lists():
        for T in dtypes:
            for p in paths:
                for n_call in (None, 1):
                    for inst, edges in fd.cells(g, T, p, n_call=n_call).items():
                        got.hit(inst, *edges)
    return got


def test_what_the_older_shape_lists_did_not_reach():
    """The gap this matrix closes, from the mirror (the table of DESIGN.md): of the 260 instances the lists of
    test_hip_parity.py that name a transform length reach 152; none of SHAPES is large enough for path='auto' to take the
    family."""
    got = old_lists_reach()
    want = fd.universe() - fd.excused()
    assert set(got) <= want
    assert not any(name == 'SHAPES' for name, *_ in _old_lists())
    missed = want - set(got)
    lens = lambda k, T: sorted(i[2] for i in missed if i[0] == k and i[1] == T)  # noqa: E731
    assert lens('k_fft_rows_fwd', 'f') == [288, 576] and lens('k_fft_rows_fwd', 'd') == [288]
    assert lens('k_fft_rows_mu', 'f') == [288, 384, 576] and lens('k_fft_rows_inv2', 'f') == [288, 384, 576]
    assert lens('k_fft_cols_fwd', 'f') == [192] and lens('k_fft_cols_fwd', 'd') == [192, 288]
    assert lens('k_fft_cols_inv', 'f') == [192, 384] and lens('k_fft_cols_inv', 'd') == [192, 288]
    heights = lambda k: sorted(i[2] for i in missed if i[0] == k)  # noqa: E731
    assert heights('k_mix_reconstruct') == [2, 3, 4, 6, 8, 10, 11, 13, 14, 15]
    assert heights('k_mix_grad_W2') == [2, 3, 4, 6, 8, 10, 11] and heights('k_mix_grad_W') == [13, 14, 15]
    assert {i[3] for i in want if i[0] == 'k_fft_grad_H'} - {i[3] for i in got if i[0] == 'k_fft_grad_H'} == {4}
    assert sum(1 for i in missed if i[0] == 'k_fft_grad_H') == 90 - 23      # 13 of 50 in float32, 10 of 40 in float64
    assert {i[2] for i in missed if i[0] == 'k_fft_grad_H' and i[3] == 1} == {192, 270, 288, 576}
    assert not any(i[0].startswith('k_spec') or i[0].endswith('_1d') for i in missed)
    assert len(got) == 152 and len(missed) == 108
    # exact fit: one row (48, HYBRID_SHAPES) and no column; no length at its shortest H on either axis in float64
    exact = sorted({(i[0], i[2]) for i, e in got.items() if 'x_exact' in e and i[0] in fd.ROW_KERNELS})
    assert exact == [('k_fft_rows_fwd', 48), ('k_fft_rows_inv', 48)]
    assert not any('y_exact' in e for e in got.values())
    # the transform lengths the corrected comments of FFT_SHAPES and HYBRID_SHAPES quote
    assert [fd.make_layout(tuple(s[:5]), 'f', 'fft')[:2] for s in old.FFT_SHAPES] == [
        (48, 64), (48, 48), (48, 96), (32, 32), (96, 96), (32, 48), (64, 64), (144, 144), (144, 192), (270, 270), (384, 540)]
    assert [fd.make_layout(tuple(s), 'f', 'hybrid')[:2] for s in old.HYBRID_SHAPES] == [
        (144, 384), (96, 48), (48, 540), (288, 48), (32, 32), (64, 64)]


# ---- the comparison helpers of the GPU file bite -------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', ['f', 'd'])
def test_comparison_helpers_fail_on_a_shifted_or_scaled_result(dtype):
    """relmax at the bars of the GPU matrix: the oracle's own array passes; shifted by one element along either axis, or
    with one plane scaled by 1 + 1e-4, it fails at every bar in use (primitive, fused, chained) -- on random operands and
    on the structured ones, whose footprint check besides names a leak into the empty region."""
    tol = gm.TOL[dtype]
    g = fd.MATRIX['y64_c3_x96']
    for kind in ('random', 'corners'):
        V, Wn, Hn = gm.operands('y64_c3_x96', kind)
        R = gm.orc.reconstruct(Wn, Hn, 'contract')
        assert gm.relmax(R, R) == 0 and gm.relmax(R.astype(np.float32 if dtype == 'f' else np.float64), R) < tol
        bad = [np.roll(R, 1, axis=-1), np.roll(R, 1, axis=-2), R.copy()]
        bad[2][np.unravel_index(R.argmax(), R.shape)[:2]] *= 1 + 1e-4          # the plane that holds the maximum
        for b in bad:
            assert gm.relmax(b, R) >= 4 * tol, (kind, gm.relmax(b, R))
            with pytest.raises(AssertionError):
                gm.check('R', b, R, tol)
        if kind == 'corners':
            assert (R == 0).mean() > 0.3                     # the region no placed atom reaches
            gm.check_empty_region(R, R, tol)
            leak = R.copy()
            leak[R == 0] = 2 * tol * R.max()
            with pytest.raises(AssertionError, match='empty region'):
                gm.check_empty_region(leak, R, tol)
            for b in bad[:2]:
                with pytest.raises(AssertionError, match='empty region'):
                    gm.check_empty_region(b, R, tol)
    assert g == (3, 3, (59, 59), 3, (5, 7))
