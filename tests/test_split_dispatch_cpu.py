"""
CPU guard of the split (3 x bf16) kernel matrix: the host mirror of the dispatch (tests/split_dispatch.py) is held to
the C++ it restates, and the geometries of tests/test_hip_split_matrix.py are held to reaching every instance of
k_split_corr_W and every edge of every MFMA form.  No GPU, no build: the sources are read as text.
"""
import os
import re

import pytest

import split_dispatch as sd
from conftest import ROOT

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _source_shapes():
    m = re.search(r'^#define TNMF_SPLIT_SHAPES\(X\)(.*)$', _read('split.hip'), re.M)
    assert m, 'TNMF_SPLIT_SHAPES not found in split.hip'
    return tuple((int(a), int(b)) for a, b in re.findall(r'X\(\s*(\d+)\s*,\s*(\d+)\s*\)', m.group(1)))


def _makefile_shapes():
    m = re.search(r'^SPLIT_SHAPES\s*:=(.*)$', _read('Makefile'), re.M)
    assert m, 'SPLIT_SHAPES not found in the Makefile'
    return tuple(tuple(int(v) for v in s.split('_')) for s in m.group(1).split())


def test_shape_lists_agree():
    """The instantiations split.hip dispatches to, the objects the Makefile builds and the mirror's list are the same, in
    the same order (the order breaks ties in split_pick).  A Makefile without a shape still links a library, with an
    undefined symbol that fails only when the library is loaded."""
    assert _source_shapes() == sd.SHAPES
    assert _makefile_shapes() == sd.SHAPES


def test_prepare_one_lists_the_mirrors_instances():
    """prepare_one() (split_kernels.h) sets attributes for four (FUSED, MULTI) instances per instantiation and two more
    with EXTRA on 2-D instantiations: the 48 instances the matrix must reach."""
    src = _read('split_kernels.h')
    body = src[src.index('int prepare_one()'):]
    body = body[:body.index('#undef SPLIT_ATTR')]
    plain, guarded = body.split('if constexpr (!SplitCfg<AY, NR4>::ONE_D)')
    call = r'SPLIT_ATTR\((true|false), (true|false), (true|false)\);'
    as_set = lambda text: {tuple(v == 'true' for v in c) for c in re.findall(call, text)}  # noqa: E731
    assert as_set(plain) == {(f, m, False) for f in (True, False) for m in (True, False)}
    assert as_set(guarded) == {(True, m, True) for m in (True, False)}
    want = {(f, m, AY, NR4, e) for AY, NR4 in sd.SHAPES for f, m, e in as_set(plain) | (set() if AY == 1 else as_set(guarded))}
    assert sd.all_instances() == want and len(want) == 48


def test_mirrored_rules_are_those_of_the_source():
    """The lines of split_kernels.h the mirror restates (the form, the waves, the workgroups per CU, the grid).  When one
    of them changes, tests/split_dispatch.py and the matrix's geometries have to be looked at again."""
    src = _read('split_kernels.h')
    for line in ('static constexpr bool m16(bool multi) { return (AY == 16 && NR4 == 4) || (AY == 12 && NR4 == 3 && multi); }',
                 'M16 = Cfg::m16(MULTI) && !(EXTRA && MULTI);',
                 'static constexpr int WAVES = (!ONE_D && lds4 > 80 * 1024 && lds8 <= 160 * 1024) ? 8 : 4;',
                 'static constexpr int kBlock = 64 * WAVES, TY = SP_RB * WAVES;',
                 'const int per_cu = Cfg::lds <= 80 * 1024 ? 2 : 1;',
                 'long P = ((long)per_cu * ctx->num_cu) / MT;',
                 'if (P > ntiles) P = ntiles;',
                 'if (extra && (!fused || g.Hs % SP_TX != 0 || Cfg::ONE_D)) return TNMF_E_UNSUPPORTED;',
                 'if (Cfg::m16(g.C > 1) && !(fused && extra && g.C > 1))'):
        assert line in src, line
    assert 'const int kb = (((AY_ + 1) / 2) * NR4_ + 1) / 2;' in _read('split.hip')


def test_instantiation_constants():
    """SplitCfg of the instantiations as the comments of split_kernels.h describe them: eight-wave workgroups (one per CU)
    for 16 x 16 atoms only, four-wave ones (two per CU) everywhere else, all within the 160 KB of LDS of a CU."""
    for AY, NR4 in sd.SHAPES:
        cfg = sd.SplitCfg(AY, NR4)
        assert cfg.WAVES == (8 if (AY, NR4) == (16, 4) else 4), (AY, NR4)
        assert (cfg.lds <= 80 * 1024) == (cfg.WAVES == 4), (AY, NR4, cfg.lds)
        assert cfg.lds <= 160 * 1024 and cfg.planeB % 256 == 64
        assert (cfg.TY + AY - 1) * (cfg.WSTR // 4) <= cfg.kBlock   # one staging item per thread (static_assert)


@pytest.mark.parametrize('A,want', [((10, 10), (12, 3)), ((13, 14), (16, 4)), ((6, 6), (7, 2)), ((8, 8), (8, 2)),
                                    ((9, 12), (9, 3)), ((4, 5), (5, 2)), ((16,), (1, 4)), ((30,), (1, 8)), ((50,), (1, 16))])
def test_picks_of_the_source_comments(A, want):
    """split_pick: the smallest covering instantiation (6 x 6 ties 7_2 with 8_2 at four k blocks: the first listed wins)."""
    D = (40,) if len(A) == 1 else (40, 40)
    assert sd.split_pick((2, 1, D, 8, A)) == want


def test_small_atoms_on_large_instantiations_are_not_worth_it_under_auto():
    """3 x 16 atoms are covered only by 16_4 (16 k blocks for 48 taps): path='split' runs them, 'auto' does not."""
    g = (4, 1, (128, 128), 32, (3, 16))
    assert sd.split_has_corr_W(g) and not sd.split_has_corr_W(g, only_if_worth=True)
    assert not sd.use_split_under_auto(g)
    assert sd.use_split_under_auto((4, 1, (128, 128), 32, (10, 10)))
    assert not sd.use_split_under_auto((1, 1, (20, 20), 8, (10, 10)))   # below 2^16 activations


def test_matrix_reaches_every_instance():
    """Every (instantiation x call kind x channel count) instance is reached by some geometry of the GPU matrix -- an
    instantiation added to TNMF_SPLIT_SHAPES without a geometry fails here."""
    reached = {sd.cell(g, kind).inst for g in sd.MATRIX.values() for kind in sd.KINDS}
    assert reached == sd.all_instances(), sorted(sd.all_instances() - reached)


def test_matrix_reaches_every_edge_of_every_form():
    """Each MFMA form meets each edge class at least once: a partial atom tile, a partial row block, a last column tile of
    one to three pixels (or a row narrower than eight), the persistent tile loop with a partial last round; and on
    several channels the ring of three window copies wraps (C > 3)."""
    edges = ('partial_atom_tile', 'partial_rows', 'edge_cols', 'tile_loop_partial')
    met = {}
    for g in sd.MATRIX.values():
        for kind in sd.KINDS:
            c = sd.cell(g, kind)
            for e in edges:
                met.setdefault((c.form, e), False)
                met[(c.form, e)] |= getattr(c, e)
    assert {f for f, _ in met} == {'16x16x32', '32x32', '1d'}
    assert all(met.values()), sorted(k for k, v in met.items() if not v)
    # every form with several channels, the ring wrapping on each
    for form in ('16x16x32', '32x32', '1d'):
        assert any(sd.cell(g, kind).form == form and g[1] > 3 for g in sd.MATRIX.values() for kind in sd.KINDS), form
    # the last column tile with one, two and three pixels, and the narrowest sample
    hx = {g[2][-1] + g[4][-1] - 1 for g in sd.MATRIX.values() if not sd.one_d(g)}
    assert {1, 2, 3} <= {h % 32 for h in hx} and min(g[2][-1] for g in sd.MATRIX.values()) == 4


def test_tile_loop_geometries_loop():
    """The counts quoted in the matrix: (tiles, workgroups per atom tile) on 256 compute units."""
    for gid, tiles, P in (('s12_c1', 81, 73), ('s16_c1_big', 30, 25), ('d4_loop', 60, 51)):
        c = sd.cell(sd.MATRIX[gid], 'fused')
        assert (c.tiles, c.P) == (tiles, P) and c.tile_loop_partial, (gid, c)
    assert sd.cell(sd.MATRIX['s16_c1_big'], 'fused').waves == 8


def test_matrix_geometries_are_split_problems():
    """Every geometry runs on the split kernel under path='split', and the EXTRA cells are the ones the issue names: the
    16x16x32 form with one channel, the 32x32 form forced back with several."""
    for g in sd.MATRIX.values():
        assert sd.split_has_corr_W(g), g
    assert sd.cell(sd.MATRIX['s16_c1'], 'extra').form == '16x16x32'
    assert sd.cell(sd.MATRIX['s16_c2'], 'extra').form == '32x32'
    assert sd.cell(sd.MATRIX['s16_c2'], 'fused').form == '16x16x32'
    assert sd.cell(sd.MATRIX['s12_c4'], 'fused').form == '16x16x32'
    assert sd.cell(sd.MATRIX['s12_c1'], 'fused').form == '32x32'
    assert all(sd.cell(g, 'extra').refused == sd.one_d(g) for g in sd.MATRIX.values())
