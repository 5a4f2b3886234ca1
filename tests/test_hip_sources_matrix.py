"""
The sources kernels, every branch of them: k_source_wsum and k_atom_sources (tnmf_amd/csrc/sources.hip) through the C ABI on
the cases of sources_dispatch.MATRIX, which are chosen with the host mirror tests/sources_dispatch.py so that together they
execute every named branch (tests/test_sources_dispatch_cpu.py checks that without a GPU, and that each case could catch the
defect it is there for).  The case that has to stride is sized from the CU count of the device the test runs on.

The bounds are those derived in the docstring of tests/test_hip_sources.py -- (n_g + 8) u for the contribution,
(n_g + n_max + S + 8) u for mask and masked, (max n_g + n_max + S + 8 + 2 (C - 1)) u for the share, against
sources_reference.outputs in float64 on operands rounded to the element type; nothing is measured.  With integer operands the
contributions and the labels are exact and the share is within 2 u.  Every call writes into buffers filled with a pattern:
4096 or 4097 elements in front of and behind ``out`` keep it, and so do the outputs the call's emit does not name.  Every test
prints the largest ratio of an error to its bound.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import sources_dispatch as sd
import test_hip_atom_gains as gains
from test_atom_gains_cpu import _AtomStub
from test_hip_atom_gains import DTYPES, NP, PATTERN, U, context, dev, p
from test_hip_sources import plane_sets, ratio
from tnmf_amd import _lib
from tnmf_amd.backends.HIP import HIP_Backend
from tnmf_amd.sources_host import source_tables
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

pytestmark = pytest.mark.gpu

FRAME = 4096
CASES = [(name, layout) for name, case in sd.MATRIX.items() for layout in case[5]]
SIGNALS = ('contribution', 'mask', 'masked')


def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def run(geo, dt, ops, sets, emit, eps=sd.EPS, out_offset=0, V_offset=0, stream=None, ctx=None, batch=None):
    """One call of tnmf_hip_atom_sources on outputs filled with PATTERN (labels: -7) -> dict(code, out [N, S, C, *D],
    label, share, front, back).  ``out`` begins FRAME + out_offset elements into its buffer and V V_offset elements into
    its own: elements behind an aligned boundary.  ``stream``: the operands are made and the call is made on it.
    ``batch``: the N of the call, where it is not the case's."""
    N, C, M, D, A = geo
    lib, own, _ = context()
    tdt = torch.float32 if dt == 'f32' else torch.float64
    S, n_out, n_V = len(sets), N * len(sets) * C * int(np.prod(D)), N * C * int(np.prod(D))
    frame = FRAME + out_offset
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        H, W = dev(ops['Hp'], dt), dev(ops['W'], dt)
        V = torch.empty(n_V + sd.PIX, dtype=tdt, device='cuda')[V_offset:V_offset + n_V]
        V.copy_(torch.from_numpy(np.array(ops['V'], dtype=NP[dt]).reshape(-1)))
        order, start = (torch.from_numpy(x).cuda() for x in source_tables(sets))
        buf = torch.full((n_out + 2 * frame,), PATTERN, dtype=tdt, device='cuda')
        out = buf[frame:frame + n_out]
        label = torch.full((N,) + D, -7, dtype=torch.int32, device='cuda')
        share = torch.full((N,) + D, PATTERN, dtype=tdt, device='cuda')
        e, unit = sd.ESIZE[dt], sd.PIX * sd.ESIZE[dt]
        assert out.data_ptr() % unit == out_offset * e % unit and V.data_ptr() % unit == V_offset * e % unit
        g = _lib.make_geom(N if batch is None else batch, M, C, D, A, DTYPES.index(dt), 0)
        code = lib.tnmf_hip_atom_sources(own if ctx is None else ctx, ctypes.byref(g), S, p(order), int(order.numel()),
                                         p(start), sd.EMIT[emit], eps, p(V), p(W), p(H), p(out), p(label), p(share),
                                         None if stream is None else ctypes.c_void_p(stream.cuda_stream))
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    whole = buf.cpu().numpy()
    return dict(code=code, out=whole[frame:frame + n_out].reshape((N, S, C) + D), front=whole[:frame], back=whole[-frame:],
                label=label.cpu().numpy(), share=share.cpu().numpy())


def untouched(got, emit):
    """The frames keep the pattern, and so does every output the emit does not name; what it names is written throughout."""
    ok = bool(np.all(got['front'] == PATTERN) and np.all(got['back'] == PATTERN))
    signals_kept = bool(np.all(got['out'] == PATTERN))
    dominant_kept = bool(np.all(got['label'] == -7) and np.all(got['share'] == PATTERN))
    if emit is None:
        return ok and signals_kept and dominant_kept
    if emit == 'dominant':
        return ok and signals_kept and not np.any(got['label'] == -7) and not np.any(got['share'] == PATTERN)
    return ok and dominant_kept and not np.any(got['out'] == PATTERN)


def judge(what, geo, dt, ops, sets, want, eps, exact=False, **how):
    """The four emits of one case against the reference ``want`` -> {emit: largest error / bound}; the ranges and the labels
    are asserted here."""
    N, C, M, D, A = geo
    bound = sd.bounds(want, C, M, A, sets, dt, exact)
    worst = {}
    for emit in SIGNALS:
        got = run(geo, dt, ops, sets, emit, eps, **how)
        assert got['code'] == 0 and untouched(got, emit), (what, emit)
        if emit in bound:
            worst[emit] = ratio(got['out'], want[emit], bound[emit])
        if emit == 'mask':
            assert np.all(got['out'] >= 0) and np.all(got['out'] <= 1)        # no tolerance: r_g <= total in the pass's sums
        if emit == 'masked':
            assert np.all(got['out'] >= 0) and np.all(got['out'] <= ops['V'][:, None].astype(NP[dt]))
    got = run(geo, dt, ops, sets, 'dominant', eps, **how)
    assert got['code'] == 0 and untouched(got, 'dominant'), what
    worst['share'] = ratio(got['share'], want['share'], bound['share'])
    if exact:
        np.testing.assert_array_equal(got['label'], want['label'])
    else:
        assert sd.label_violations(got['label'], want, C, M, A, sets, dt) == 0, what
    print(f'sources matrix {what} {dt}: largest error / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    return worst


def test_the_mirror_is_asked_about_this_device():
    """The stride case strides at the CU count of this device; the layouts are those of tests/test_hip_sources.py."""
    cu = device_cus()
    print(f'{cu} compute units')
    assert 'wsum:grid-stride' in sd.reached('wsum-stride', 'scattered', 'f32', 'dominant', num_cu=cu)
    for layout in ('each', 'interleaved', 'all'):
        assert plane_sets(6, layout) == sd.plane_sets(6, layout) and plane_sets(7, layout) == sd.plane_sets(7, layout)


# -- 1. every case, both element types, all four emits, within the derived bound -----------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name,layout', CASES)
def test_every_case_within_the_derived_bound(name, layout, dt):
    cu = device_cus()
    geo = sd.geometry(name, cu)
    ops, sets = sd.operands(name, dt, layout, cu), sd.plane_sets(geo[2], layout)
    want = sd.reference(name, layout, dt, 'default', 'random', cu)
    worst = judge(f'{name} {layout}', geo, dt, ops, sets, want, sd.eps_of(name, layout, dt, 'default', 'random', cu))
    assert max(worst.values()) <= 1., worst


# -- 2. integer operands: exact contributions and labels, the planted pixels ---------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('layout', sd.TWO)
@pytest.mark.parametrize('name', sd.INTEGER_CASES)
def test_integer_operands_are_exact_and_the_planted_pixels_answer_as_the_reference(name, layout, dt):
    geo = N, C, M, D, A = sd.geometry(name)
    ops, sets = sd.integer_operands(name, layout), sd.plane_sets(M, layout)
    want = sd.reference(name, layout, dt, 'default', 'integer')
    assert want['total'].sum(axis=1).max() < 2 ** 24
    tc, rc = want['total'].sum(axis=1), want['contribution'].sum(axis=2)
    nobody = tc == 0
    assert nobody.any() and np.all(want['label'][nobody] == -1)
    if layout == 'each':
        assert np.any((rc[:, 0] == rc[:, 1]) & (rc[:, 0] > 0) & (want['label'] == 0))     # a planted tie, the lowest index wins
    else:
        only_hidden = (tc > 0) & (rc.max(axis=1) == 0)
        assert only_hidden.any() and np.all(want['label'][only_hidden] == 0) and np.all(want['share'][only_hidden] == 0)
    got = run(geo, dt, ops, sets, 'contribution')
    assert got['code'] == 0 and untouched(got, 'contribution')
    np.testing.assert_array_equal(got['out'], want['contribution'])
    if layout == 'each':
        np.testing.assert_array_equal(got['out'].astype(np.float64).sum(axis=1), want['total'])   # a partition adds up to R
    dom = run(geo, dt, ops, sets, 'dominant')
    assert dom['code'] == 0 and untouched(dom, 'dominant')
    np.testing.assert_array_equal(dom['label'], want['label'])
    worst = ratio(dom['share'], want['share'], 2 * U[dt] * want['share'])
    print(f'sources matrix {name} {layout} {dt} integer operands: share, largest error / (2 u share): {worst:.3f}')
    assert worst <= 1.
    # with eps = 0: the masks of a pixel nobody explains, and of one that only hidden planes explain, are 0
    mask = run(geo, dt, ops, sets, 'mask', eps=0.)
    assert mask['code'] == 0 and np.all(mask['out'] <= 1)
    zero = np.broadcast_to(((rc.max(axis=1) == 0))[:, None, None], mask['out'].shape)
    assert np.all(mask['out'][zero] == 0) and np.all(mask['out'][~zero] >= 0)
    np.testing.assert_array_equal(mask['out'] == 0, want['contribution'] == 0)


@pytest.mark.parametrize('dt', DTYPES)
def test_the_channel_sums_beyond_one_pass_of_the_grid(dt):
    """wsum-stride: more planes of 1024 taps than num_cu * 8 workgroups of 256 threads cover; integers in 0..1, every sum
    below 2^24 and exact.  Two runs give the same bits."""
    cu = device_cus()
    name, layout = 'wsum-stride', 'scattered'
    geo = N, C, M, D, A = sd.geometry(name, cu)
    assert M * 1024 > cu * 8 * 256
    ops, sets = sd.integer_operands(name, layout, cu), sd.plane_sets(M, layout)
    want = sd.reference(name, layout, dt, 'default', 'integer', cu)
    assert ops['W'].max() == 1 and ops['Hp'].max() == 1 and 0 < want['total'].sum(axis=1).max() < 2 ** 24
    first, second = run(geo, dt, ops, sets, 'dominant'), run(geo, dt, ops, sets, 'dominant')
    assert first['code'] == 0 and untouched(first, 'dominant')
    np.testing.assert_array_equal(first['label'], want['label'])
    worst = ratio(first['share'], want['share'], 2 * U[dt] * want['share'])
    print(f'sources matrix {name} {dt}, {M} planes at {cu} compute units: share, largest error / (2 u share): {worst:.3f}')
    assert worst <= 1.
    assert first['label'].tobytes() == second['label'].tobytes() and first['share'].tobytes() == second['share'].tobytes()
    a, b = run(geo, dt, ops, sets, 'contribution'), run(geo, dt, ops, sets, 'contribution')
    np.testing.assert_array_equal(a['out'], want['contribution'])
    assert a['out'].tobytes() == b['out'].tobytes()


# -- 3. the two store paths give the same bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', sd.IDENTITY_CASES)
def test_aligned_and_pixelwise_stores_give_identical_bytes(name, dt):
    geo = N, C, M, D, A = sd.geometry(name)
    layout = 'interleaved'
    ops, sets = sd.operands(name, dt, layout), sd.plane_sets(M, layout)
    paths = [sd.reached(name, layout, dt, 'masked', o, v) for o, v in sd.OFFSETS]
    assert 'vec' in paths[0] and 'pixelwise:out-misaligned' in paths[1] and 'pixelwise:V-misaligned' in paths[2]
    for emit in ('contribution', 'masked'):
        got = [run(geo, dt, ops, sets, emit, out_offset=o, V_offset=v) for o, v in sd.OFFSETS]
        for g, (o, v) in zip(got, sd.OFFSETS):
            assert g['code'] == 0 and len(g['front']) == FRAME + o and untouched(g, emit), (emit, o, v)
        assert got[0]['out'].tobytes() == got[1]['out'].tobytes() == got[2]['out'].tobytes(), emit


# -- 4. eps --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('eps', ['zero', 'median'])
@pytest.mark.parametrize('name,layout', sd.EPS_CASES)
def test_eps_of_zero_and_eps_comparable_to_the_totals(name, layout, eps, dt):
    geo = N, C, M, D, A = sd.geometry(name)
    ops, sets = sd.operands(name, dt, layout), sd.plane_sets(M, layout)
    want = sd.reference(name, layout, dt, eps, 'random')
    value = sd.eps_of(name, layout, dt, eps)
    assert value == 0. if eps == 'zero' else 0.1 < value / np.median(want['total']) < 10.
    worst = judge(f'{name} {layout} eps={value:.3g}', geo, dt, ops, sets, want, value)
    assert max(worst.values()) <= 1., worst
    if eps == 'zero':
        nobody = want['total'] == 0
        assert nobody.any()
        for emit in ('mask', 'masked'):
            got = run(geo, dt, ops, sets, emit, eps=0.)
            assert np.all(got['out'][np.broadcast_to(nobody[:, None], got['out'].shape)] == 0)
        dom = run(geo, dt, ops, sets, 'dominant', eps=0.)
        assert np.all(dom['share'][nobody.all(axis=1)] == 0) and np.all(dom['label'][nobody.all(axis=1)] == -1)


# -- 5. around the call --------------------------------------------------------------------------------------------------------
def test_the_shared_work_buffer_survives_interleaved_calls():
    """tnmf_hip_atom_terms, the sources, tnmf_hip_atom_terms on one context: the taps, the tables and the channel sums live
    in the buffer the atom terms keep their partial sums and taps in."""
    name, dt = 'tile-plus-one', 'f32'
    terms_ops = gains.operands(name, dt, 'real')
    geo = sd.geometry('vec-c5')
    ops, sets = sd.operands('vec-c5', dt, 'scattered'), sd.plane_sets(geo[2], 'scattered')
    fresh = HIP_Backend()
    alone = {emit: run(geo, dt, ops, sets, emit, ctx=fresh._ctx) for emit in ('masked', 'dominant')}
    code, before = gains.call(name, dt, terms_ops)
    assert code == 0
    between = {emit: run(geo, dt, ops, sets, emit) for emit in ('masked', 'dominant')}
    code, after = gains.call(name, dt, terms_ops)
    assert code == 0 and before.tobytes() == after.tobytes()
    for emit in alone:
        assert alone[emit]['code'] == between[emit]['code'] == 0
        for key in ('out', 'label', 'share'):
            assert alone[emit][key].tobytes() == between[emit][key].tobytes(), (emit, key)
    assert not np.any(between['masked']['out'] == PATTERN) and not np.any(between['dominant']['label'] == -7)


@pytest.mark.parametrize('emit', list(sd.EMIT))
def test_an_empty_batch_returns_ok_and_writes_nothing(emit):
    geo = sd.geometry('vec-ragged')
    ops, sets = sd.operands('vec-ragged', 'f32', 'interleaved'), sd.plane_sets(geo[2], 'interleaved')
    got = run(geo, 'f32', ops, sets, emit, batch=0)
    assert got['code'] == 0 and untouched(got, None)


@pytest.mark.parametrize('dt', DTYPES)
def test_a_stream_other_than_the_default_gives_the_same_bytes(dt):
    geo = sd.geometry('vec-ragged')
    ops, sets = sd.operands('vec-ragged', dt, 'scattered'), sd.plane_sets(geo[2], 'scattered')
    stream = torch.cuda.Stream()
    for emit in ('masked', 'dominant'):
        default, other = run(geo, dt, ops, sets, emit), run(geo, dt, ops, sets, emit, stream=stream)
        assert default['code'] == other['code'] == 0 and untouched(other, emit)
        for key in ('out', 'label', 'share'):
            assert default[key].tobytes() == other[key].tobytes(), (emit, key)


def test_float32_with_two_channels_through_the_front_end():
    """The only way to k_atom_sources<float, 2> through HIP_Backend._atom_sources: a float32 fit of two channels; against
    the float64 host fallback on the same (W, H), within the float32 bounds."""
    shape_V, M, A = (2, 2, 20, 68), 3, (5, 5)
    V = (np.random.default_rng(0).random(shape_V) + 0.05).astype(np.float32)
    np.random.seed(42)
    hip = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip')
    hip.fit(V, n_iterations=2, sparsity_H=0.1)
    np.random.seed(42)
    cpu = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend=_AtomStub('valid'))
    cpu.fit(V.astype(np.float64), n_iterations=0)
    cpu._W[...] = hip.W
    cpu._H[...] = hip._backend.to_ndarray(hip._H)
    cpu._expand_W()
    assert hip._backend.supports_sources and not getattr(cpu._backend, 'supports_sources', False)
    C, nA, u = shape_V[1], int(np.prod(A)), U['f32']
    worst = {}
    for sources in (None, [[M - 1], [0]]):
        sets = [[m] for m in range(M)] if sources is None else sources
        S, n_max = len(sets), nA * max(1, M - len(sets))
        tag = '' if sources is None else ' (two sources)'
        for output in SIGNALS:
            got, want = hip.separate(sources, output=output), cpu.separate(sources, output=output)
            assert got.dtype == np.float32 and want.dtype == np.float64 and got.shape == want.shape == (2, S) + shape_V[1:]
            n = (nA + 8) if output == 'contribution' else (nA + n_max + S + 8)
            worst[output + tag] = ratio(got, want, n * u * np.abs(want))
            if output == 'mask':
                assert np.all(got >= 0) and np.all(got <= 1)
            if output == 'masked':
                assert np.all(got >= 0) and np.all(got <= V[:, None])
        label, share = hip.dominant_source(sources)
        want_label, want_share = cpu.dominant_source(sources)
        rc = cpu.separate(sources, output='contribution').sum(axis=2)
        differ = label != want_label                          # the near-tie rule of tests/test_hip_sources.py
        chosen = np.take_along_axis(rc, np.maximum(label, 0)[:, None].astype(np.int64), axis=1)[:, 0]
        assert np.all(label[differ] >= 0)
        assert np.all((rc.max(axis=1) - chosen)[differ] <= 2 * (n_max + C + 8) * u * rc.max(axis=1)[differ])
        worst['share' + tag] = ratio(share, want_share, (nA + n_max + S + 8 + 2 * (C - 1)) * u * want_share)
    print('separate float32, C = 2: largest difference to the float64 fallback / bound: '
          + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1., worst
