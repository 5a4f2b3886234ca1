"""
CPU guard of the sources matrix: the host mirror tests/sources_dispatch.py is held to the sources it restates
(tnmf_amd/csrc/sources.hip, atoms.h, api.hip, include/tnmf_hip.h, read as text), the cases of
tests/test_hip_sources_matrix.py are held to executing every named branch at several CU counts, the planted pixels are held to
existing in the reference, and the wrong models -- the reference with one defect each -- are held to differing from it on the
case named for them by more than 100 times the bound the GPU test applies there: no kernel is broken for it.  No GPU, no build.
"""
import os
import re

import numpy as np
import pytest

import atoms_dispatch as ad
import sources_dispatch as sd
import sources_reference as sref
from conftest import ROOT
from tnmf_amd import _lib
from tnmf_amd.sources_host import source_tables

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')
CUS = (64, 256, 304)


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


# -- the mirror against the sources --------------------------------------------------------------------------------------------
def test_constants_and_rules_are_those_of_the_sources():
    """The lines the mirror restates.  When one of them changes, tests/sources_dispatch.py and its cases have to be looked at
    again."""
    src, atoms_h, api, header = _read(CSRC, 'sources.hip'), _read(CSRC, 'atoms.h'), _read(CSRC, 'api.hip'), \
        _read('include', 'tnmf_hip.h')
    assert ad.STAGE == int(re.search(r'constexpr int kStage = (\d+);', src).group(1))
    for name, value in (('kAtomPix', sd.PIX), ('kAtomThreads', sd.THREADS), ('kAtomChannels', sd.CHANNELS)):
        assert value == int(re.search(rf'constexpr int {name} = (\d+);', atoms_h).group(1)), name
    codes = {name.lower(): int(code) for name, code in re.findall(r'#define TNMF_SOURCES_(\w+) (\d+)', header)}
    assert codes == sd.EMIT == _lib.SOURCE_OUTPUTS
    for line in ('const bool vec = g.Dx % kAtomPix == 0 && reinterpret_cast<uintptr_t>(out) % (kAtomPix * esize(dtype)) == 0 &&\n'
                 '                     reinterpret_cast<uintptr_t>(V) % (kAtomPix * esize(dtype)) == 0;',
                 '(unsigned)std::min<size_t>((n_sum + kAtomThreads - 1) / kAtomThreads, (size_t)ctx->num_cu * 8);',
                 'const size_t n_sum = (size_t)g.M * g.Ay * g.Ax;',
                 'for (size_t i = (size_t)blockIdx.x * kAtomThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kAtomThreads) {',
                 'const int nc = g.C - c0 < CH ? g.C - c0 : CH;',
                 'const bool pre_ok = nel <= kStage * kAtomThreads;',
                 'if (xb < g.Dx) *reinterpret_cast<Quad<T> *>(q) = Quad<T>{v[0], v[1], v[2], v[3]};',
                 'const Quad<T> w = xb < g.Dx ? *reinterpret_cast<const Quad<T> *>(q) : Quad<T>(T(0));',
                 'if (gi < S && (gi == 0 || rv[px] > best[px])) {',
                 'end = gi <= S ? start[gi + 1] : -1;',
                 'label[o] = total[0][px] > T(0) ? arg[px] : -1;',
                 'if (dom) g.C = 1;',
                 'w.wsum_off = atom_terms_taps_bytes(g, dtype);',
                 'const size_t wsum = emit == TNMF_SOURCES_DOMINANT ? (size_t)g.M * g.Ay * g.Ax * esize(dtype) : 0;',
                 'w.order_off = w.wsum_off + align_up(wsum, 256);',
                 'w.start_off = w.order_off + align_up((size_t)g.M * sizeof(int), 256);',
                 'w.total = w.start_off + align_up((size_t)(n_sources + 2) * sizeof(int), 256);'):
        assert line in src, line
    assert re.search(r'atomic\w*\s*\(', src) is None          # one writer per output element
    for line in ('if (!listed[m]) order[fill++] = m;', 'start[n_sources + 1] = g.M;',
                 'if (g.N == 0) return TNMF_OK;'):
        assert line in api, line
    assert 'return align_up((size_t)g.M * g.C * g.Ay * 2 * atom_terms_plan(g).NBO * kAtomPix * esize(dtype), 256);' in \
        _read(CSRC, 'atoms.hip')


def test_known_answers_of_the_rules():
    # vec: four floats are 16 bytes, four doubles 32; one element off either pointer, or a ragged width, ends it
    for e in (4, 8):
        assert sd.vec(68, 0, 0, e) and sd.vec(68, 4, 8, e)
        assert not sd.vec(68, 1, 0, e) and not sd.vec(68, 0, 1, e) and not sd.vec(66, 0, 0, e) and not sd.vec(68, 2, 0, e)
    assert [sd.instance(c, 'mask') for c in (1, 2, 3, 4, 5)] == [(1, False), (2, False), (3, False), (4, False), (4, False)]
    assert sd.instance(5, 'dominant') == (1, True)
    assert [sd.chunk_channels(c) for c in (1, 2, 3, 4, 5, 8)] == [[1], [2], [3], [4], [4, 1], [4, 4]]
    # the plans of the cases
    p = sd.plan(2, (17, 68), (3, 4))
    assert (p['tiles_y'], p['tiles_x'], p['CH'], p['chunks']) == (2, 2, 2, 1)
    p = sd.plan(1, (9, 12), (20, 8))
    assert (p['SH'], p['SW']) == (35, 76) and 35 * 76 > 2560 and not sd.pre_ok(1, (9, 12), (20, 8))
    assert sd.pre_ok(2, (17, 68), (3, 4)) and sd.pre_ok(3, (1028,), (7,))
    p = sd.plan(3, (1028,), (7,))
    assert (p['TY'], p['TX'], p['tiles_x']) == (1, 1024, 2)
    p = sd.plan(5, (9, 12), (3, 4))
    assert (p['CH'], p['chunks'], p['slots']) == (4, 2, 2)
    # the channel sums: 513 planes of 1024 taps against 2048 workgroups of 256
    assert sd.wsum_grid(513, (32, 32), 256) == (525312, 2052, 2048)
    assert sd.wsum_grid(5, (3, 3), 256) == (45, 1, 1) and sd.wsum_grid(5, (20, 8), 256) == (800, 4, 4)
    assert sd.wsum_grid(2 * 64 + 1, (32, 32), 64)[1:] == (516, 512)
    # the work buffer: 6 planes of 2 channels of 3 rows of 2 * 2 runs of 4 floats = 2304 bytes
    assert sd.taps_bytes(2, 6, (17, 68), (3, 4), 'f32') == 2304
    assert sd.work(2, 6, (17, 68), (3, 4), 'f32', 2, 'mask') == dict(taps_off=0, wsum_off=2304, order_off=2304,
                                                                       start_off=2560, total=2816)
    assert sd.work(2, 6, (17, 68), (3, 4), 'f32', 2, 'dominant') == dict(taps_off=0, wsum_off=2304, order_off=2304 + 512,
                                                                           start_off=2304 + 768, total=2304 + 1024)
    # the tables
    order, start = sd.tables([[5, 2], [0]], 6)
    assert order.tolist() == [5, 2, 0, 1, 3, 4] and start.tolist() == [0, 2, 3, 6]
    order, start = sd.tables([[m] for m in range(3)], 3)
    assert order.tolist() == [0, 1, 2] and start.tolist() == [0, 1, 2, 3, 3]
    for M in (5, 6, 7):
        for layout in sd.LAYOUTS:
            sets = sd.plane_sets(M, layout)
            listed, first = source_tables(sets)
            order, start = sd.tables(sets, M)
            assert np.array_equal(order[:len(listed)], listed) and np.array_equal(start[:-1], first)
            assert sorted(order.tolist()) == list(range(M)) and order[len(listed):].tolist() == sd.hidden_planes(M, sets)


# -- coverage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cu', CUS)
def test_every_branch_is_reached_and_no_case_is_large(cu):
    union = set()
    per_case = {}
    for name, layout, dt, emit, out_offset, V_offset, eps, kind in sd.runs(cu):
        got = sd.reached(name, layout, dt, emit, out_offset, V_offset, eps, kind, cu)
        union |= got
        per_case.setdefault(name, set()).update(got)
        assert sd.device_bytes(name, layout, dt, cu) <= sd.DEVICE_LIMIT, (name, layout, dt)
    missing = set(sd.BRANCHES) - union - set(sd.NOT_REACHED)
    assert not missing, (cu, sorted(missing))
    # what each case of the matrix is there for
    for name, names in (('vec-ragged', ('vec:thread-outside-x', 'vec:row-outside-y', 'vec:several-tiles', 'CH2:f32', 'vec',
                                        'pixelwise:out-misaligned', 'pixelwise:V-misaligned', 'hidden:several-and-largest',
                                        'pixel:only-hidden-explains', 'pixel:nobody-explains', 'S==1:rest-hidden',
                                        'tie:lowest-index-wins', 'source:planes-descending-and-scattered')),
                        ('vec-c4', ('CH4:full:f32', 'CH4:full:f64', 'wsum:one-block')),
                        ('vec-c5', ('CH4:short-second-chunk:f32', 'vec')),
                        ('vec-stage-loop', ('vec:stage-loop', 'CH1:f32', 'wsum:C==1', 'wsum:partial-last-block')),
                        ('vec-below-halo', ('vec:below-halo',)),
                        ('vec-1d', ('vec:1d', 'vec:thread-outside-x', 'vec:several-tiles', 'CH3:f32')),
                        ('pixel-c3', ('pixelwise:Dx%4',)),
                        ('wsum-stride', ('wsum:grid-stride', 'DOM:f32', 'DOM:f64', 'vec:stage-loop'))):
        assert set(names) <= per_case[name], (name, cu, sorted(set(names) - per_case[name]))
    assert 'vec' not in per_case['pixel-c3']
    # the stride case strides by exactly one plane's worth and a bit
    N, C, M, D, A = sd.geometry('wsum-stride', cu)
    n_sum, blocks, grid = sd.wsum_grid(M, A, cu)
    assert blocks > grid == cu * 8 and 0 < n_sum - grid * sd.THREADS <= int(np.prod(A))


def test_the_layouts_keep_the_three_of_the_first_tests_and_every_case_has_room():
    assert sd.plane_sets(5, 'each') == [[0], [1], [2], [3], [4]]
    assert sd.plane_sets(5, 'interleaved') == [[0, 2], [1, 3]] and sd.plane_sets(6, 'interleaved') == [[0, 2, 4], [1, 3]]
    assert sd.plane_sets(5, 'all') == [[4, 3, 2, 1, 0]]
    assert sd.plane_sets(7, 'scattered') == [[6, 2], [0]] and sd.plane_sets(7, 'hidden-heavy') == [[0]]
    for name in sd.MATRIX:
        N, C, M, D, A = sd.geometry(name)
        assert name == 'wsum-stride' or (N == 2 and 5 <= M <= 7)
        assert len(sd.hidden_planes(M, sd.plane_sets(M, 'scattered'))) >= 2
        for c in (C, 1):
            p = sd.plan(c, D, A)
            assert p['SH'] * p['SW'] * 8 <= ad.LDS_LIMIT, name


def test_an_aligned_store_without_its_guard_would_be_seen():
    """Argued from the mirror, never run: without `xb < g.Dx` in the aligned branch of `put`, the threads outside the
    sample store onto other pixels' elements -- whose rightful values the comparison with the reference then misses -- and,
    from the last rows of the last plane, behind the end of `out`, within the 4096 elements of pattern the GPU test keeps
    there and checks."""
    for name in sd.IDENTITY_CASES:
        assert 'vec:thread-outside-x' in sd.reached(name, 'interleaved', 'f32', 'masked')
        inside, beyond, farthest = sd.stray_stores(name, 'interleaved')
        print(f'{name}: {inside} stray elements inside out, {beyond} behind it, the farthest {farthest} elements behind')
        assert inside > 0 and beyond > 0 and farthest <= 4096
    # vec-ragged: tile column 1 holds the pixels 64 .. 67 of 68: 15 threads a row lie outside, and the last row's reach 60 behind
    assert sd.stray_stores('vec-ragged', 'interleaved') == (2 * 2 * 2 * 17 * 15 * 4 - 60, 60, 60)


# -- the references ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n in sd.MATRIX if n != 'wsum-stride'])
def test_the_contraction_is_the_reference(name):
    """``outputs`` (one contraction over sliding windows, then ``finish``) against sources_reference.outputs: the same
    bits on integers, the same to rounding on random operands; the reference of the stride case rests on this."""
    layouts = sd.MATRIX[name][5]
    for layout in layouts:
        for kind in ('random', 'integer'):
            want, got = sd.reference(name, layout, 'f32', 'default', kind), sd.outputs(name, layout, 'f32', 'default', kind)
            assert set(want) == set(got)
            for key in want:
                if kind == 'integer' or key == 'label':
                    assert np.array_equal(want[key], got[key]), (name, layout, kind, key)
                else:
                    np.testing.assert_allclose(got[key], want[key], rtol=1e-13, atol=0, err_msg=f'{name} {layout} {key}')


def test_the_stride_case_is_exact_and_below_2_to_24():
    for cu in CUS:
        N, C, M, D, A = sd.geometry('wsum-stride', cu)
        ops = sd.integer_operands('wsum-stride', 'scattered', cu)
        assert M == 2 * cu + 1 and ops['W'].max() == 1 and ops['Hp'].max() == 1
        want = sd.reference('wsum-stride', 'scattered', 'f32', 'default', 'integer', cu)
        assert 0 < want['total'].sum(axis=1).max() < 2 ** 24
        assert np.array_equal(want['total'], np.round(want['total']))
        # plane by plane, as atoms_reference.parts_valid does it, on the first and the last plane
        for m in (0, M - 1):
            one = sref.source_sums(ops['W'][m:m + 1], ops['Hp'][:, m:m + 1], [[0]])[0][:, 0]
            assert np.array_equal(one, sd.fast_parts(ops['W'][m:m + 1], ops['Hp'][:, m:m + 1])[:, 0])
        assert np.any(want['label'] == 0) and np.all(want['label'] >= 0)


# -- the wrong models ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('defect', list(sd.WRONG))
def test_each_wrong_model_differs_on_the_case_named_for_it_by_100_bounds(defect):
    name, layout, kind, eps, keys = sd.WRONG[defect]
    assert (name, layout) in [(n, l) for n, l, *_ in sd.runs()]
    for dt in sd.DTYPES:
        N, C, M, D, A = sd.geometry(name)
        sets = sd.plane_sets(M, layout)
        right = sd.reference(name, layout, dt, eps, kind)
        wrong = sd.outputs(name, layout, dt, eps, kind, defect=defect)
        bound = sd.bounds(right, C, M, A, sets, dt, exact=kind == 'integer')
        shown = {}
        for key in keys:
            if key == 'label':
                # integer operands: the GPU test asks for equal labels
                assert kind == 'integer'
                shown[key] = int(np.sum(wrong['label'] != right['label']))
                assert shown[key] > 0, (defect, dt, key)
                continue
            err = np.abs(wrong[key] - right[key])
            assert key in bound, (defect, key)
            worst = float(np.max(np.divide(err, bound[key], out=np.where(err > 0, np.inf, 0.), where=bound[key] > 0)))
            shown[key] = worst
            assert worst > 100., (defect, dt, key, worst)
        print(f'{defect} on {name} {layout} {dt}: ' + ', '.join(
            f'{k} {v} labels' if k == 'label' else f'{k} {v:.3g} bounds' for k, v in shown.items()))
    # the model without a defect is the reference
    got = sd.outputs(name, layout, 'f64', eps, kind)
    right = sd.reference(name, layout, 'f64', eps, kind)
    assert np.array_equal(got['label'], right['label'])
    np.testing.assert_allclose(got['masked'], right['masked'], rtol=1e-13, atol=0)


def test_the_wrong_models_are_the_list_of_the_mirror():
    assert list(sd.WRONG) == ['total-without-hidden', 'tie-last', 'label-minus-one-on-best', 'wsum-drops-last-channel',
                              'share-over-channel-0', 'masked-times-first-channel-V', 'second-chunk-reads-first',
                              'total-of-sample-0', 'boundary-off-by-one', 'eps-dropped', 'wsum-missing-tail']
    # the tail that a one-pass k_source_wsum leaves out at 256 CUs is the last plane, which source 0 holds
    N, C, M, D, A = sd.geometry('wsum-stride', 256)
    assert 256 * 8 * 256 == (M - 1) * int(np.prod(A)) and sd.plane_sets(M, 'scattered')[0][0] == M - 1


# -- the planted pixels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['random', 'integer'])
@pytest.mark.parametrize('name', [n for n in sd.MATRIX if n != 'wsum-stride'])
def test_the_planted_pixels_exist_in_the_reference(name, kind):
    N, C, M, D, A = sd.geometry(name)
    for layout in sd.MATRIX[name][5] if kind == 'random' else sd.TWO:
        want = sd.reference(name, layout, 'f32', 'default', kind)
        sets = sd.plane_sets(M, layout)
        tc = want['total'].sum(axis=1)
        nobody = tc == 0
        assert nobody.any() and np.all(want['label'][nobody] == -1) and np.all(want['share'][nobody] == 0)
        assert np.all(want['mask'][np.broadcast_to(nobody[:, None, None], want['mask'].shape)] == 0)
        if kind == 'random':      # sample 0, the last two pixels of every row
            assert np.all(nobody[0, ..., -2:]) and not nobody[1].any()
        if sd.hidden_planes(M, sets):
            block = (1,) + tuple(slice(0, b) for b in sd.hidden_block(D))
            assert np.all(tc[block] > 0) and np.all(want['label'][block] == 0) and np.all(want['share'][block] == 0)
            assert np.all(want['mask'][(1, slice(None), slice(None)) + block[1:]] == 0)
            assert np.all(want['total'][(1, slice(None)) + block[1:]] > 0)
        if kind == 'integer' and layout == 'each':
            rc = want['contribution'].sum(axis=2)
            assert np.any((rc[:, 0] == rc[:, 1]) & (rc[:, 0] > 0) & (want['label'] == 0))
        if layout == 'hidden-heavy':
            assert np.mean(tc - want['contribution'].sum(axis=(1, 2)) > want['contribution'].sum(axis=(1, 2))) > 0.75
