"""
The seven kernels that score events, every branch of them: k_events_gain (tnmf_amd/csrc/events.hip), k_events_norms,
k_pursuit_score, k_pursuit_taken, k_pursuit_pick (pursuit.hip), k_events_landscape (landscape.hip) and k_events_alternatives
(alternatives.hip) through the C ABI on the cases of scoring_dispatch.MATRIX, which are chosen with the host mirror
tests/scoring_dispatch.py so that together they execute every named branch (tests/test_scoring_dispatch_cpu.py checks that
without a GPU).  The cases that have to stride are sized from the CU count of the device the test runs on, and the mirror is
asked whether they stride there.

Everything is EXACT.  W, V and R are integers in 0..3 and the strengths multiples of 1/2, so every product and every double sum
is an integer or a multiple of 1/8 far below 2^53, the same in any order: a, b, mag, the gains, the norms and the decoded rows
equal the float64 references bit for bit, and one dropped, doubled or misplaced tap fails.  The pick's strength and gain are
one IEEE division of exact operands: the numpy expression in float64.  The score is one correctly rounded product and
quotient: the numpy expression, on any data.  Every output lies in a buffer with poisoned slack around it, which must stay as
it was.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import scoring_dispatch as sc
from test_hip_events import DTYPES, NP, dev, p
from test_hip_events_gain import SENTINEL, events_of
from test_hip_events_matrix import backend, device_cus
from tnmf_amd import _lib

pytestmark = pytest.mark.gpu

SLACK = 2                       # poisoned rows behind every output of the one-wave-per-row kernels
EVENTS = sc.names_of('events')


def context():
    """Any initialised backend: the entries take their geometry per call."""
    be = backend(2, 2, 3, (20, 23), (4, 6), 'circular', 'f32')
    return be._lib, be._ctx


def torch_type(dt):
    return getattr(torch, np.dtype(NP[dt]).name)


def bits(x):
    return np.ascontiguousarray(x).tobytes()


@pytest.mark.parametrize('name', list(sc.MATRIX))
def test_the_case_reaches_its_branches_on_this_device(name):
    """What the case is there for, by the mirror, with the CU count of this device -- the stride cases stride here."""
    cu = device_cus()
    print(f'{name}: {cu} compute units')
    for dt in DTYPES if sc.kind_of(name) == 'score' else DTYPES[:1]:
        got = sc.reached(name, cu, dt)
        for kernel, names in sc.MATRIX[name][2].items():
            assert set(names) <= got[kernel], (name, dt, kernel, cu, sorted(set(names) - got[kernel]))


# -- norms ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def norms_want(name):
    cu = device_cus()
    want = sc.norms_reference(sc.norms_geometry(name, cu), sc.dictionary(name, cu))
    want.setflags(write=False)
    return want


def norms_call(geo, W, dt, N):
    lib, ctx = context()
    _, C, P, D, A, mode = geo
    entries = P * int(np.prod(sc.shift_shape(geo)))
    b = torch.full((entries + 8,), float('nan'), dtype=torch.float64, device='cuda')
    g = _lib.make_geom(N, P, C, D, A, DTYPES.index(dt))
    Wd = dev(W, dt)                                                                     # (held until the call has run)
    code = lib.tnmf_hip_events_norms(ctx, ctypes.byref(g), _lib.MODES[mode], p(Wd), p(b), None)
    torch.cuda.synchronize()
    b = b.cpu().numpy()
    return code, b[:entries], b[entries:]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', sc.norms_names())
def test_the_norms_are_the_reference_bit_for_bit(name, dt):
    cu = device_cus()
    geo, W = sc.norms_geometry(name, cu), sc.dictionary(name, cu)
    want = norms_want(name).reshape(-1)
    code, b, behind = norms_call(geo, W, dt, 2)
    assert code == 0 and not np.isnan(b).any(), ('every element is written', np.flatnonzero(np.isnan(b))[:8])
    assert np.isnan(behind).all(), 'nothing is written behind the table'
    wrong = np.flatnonzero(b != want)
    assert bits(b) == bits(want), (name, len(wrong), wrong[:8].tolist(), b[wrong[:8]].tolist(), want[wrong[:8]].tolist())
    # either side of every seam of the shortcut: the last shift that takes the plane's norm and the first that is walked
    short = np.broadcast_to(sc.norms_shortcut(geo), (geo[2],) + sc.shift_shape(geo)).reshape(-1)
    if 'N3:shortcut' in sc.MATRIX[name][2].get('norms', ()):
        whole = np.sum(W.reshape(geo[2], -1) ** 2, axis=1)
        assert short.any() and not short.all() and np.array_equal(b[short], np.repeat(whole, short.sum() // geo[2]))
    code, again, _ = norms_call(geo, W, dt, 0)                                   # the table does not depend on the samples
    assert code == 0 and bits(again) == bits(b), 'the same bits again'


# -- score and taken -----------------------------------------------------------------------------------------------------------
def score_call(c, dt, a_buf, gain_buf, taken):
    """One tnmf_hip_pursuit_score call on the views of the case into the two buffers."""
    lib, ctx = context()
    plan = c['plan']
    N, P, Sy, Sx = plan['shape']
    Hs, size = plan['Hs0'], N * P * Sy * plan['Hs0']
    D, A = ((Sy, Sx), (1, 1)) if Sy > 1 else ((Sx,), (1,))
    g = _lib.make_geom(N, P, 1, D, A, DTYPES.index(dt), 0 if Hs == Sx else Hs)
    a_view, gain_view = a_buf[c['a_off']:c['a_off'] + size], gain_buf[c['gain_off']:c['gain_off'] + size]
    td = None if taken is None else torch.from_numpy(np.array(taken)).cuda()
    code = lib.tnmf_hip_pursuit_score(ctx, ctypes.byref(g), p(a_view), p(c['bd']), p(gain_view), p(td),
                                      0 if taken is None else len(taken), None)
    torch.cuda.synchronize()
    return code


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', sc.names_of('score'))
def test_score_and_taken_are_the_numpy_expression_bit_for_bit(name, dt):
    """The map lies in a buffer with one spare 16-byte unit: a misaligned view starts one element in.  The pad columns, the
    spare unit and, where the call is not in place, the map itself stay as they were."""
    c = dict(sc.score_case(name, dt, device_cus()))
    plan = c['plan']
    N, P, Sy, Sx = plan['shape']
    Hs, kV = plan['Hs0'], plan['kV']
    size = N * P * Sy * Hs
    assert c['a_off'] < kV and c['gain_off'] < kV
    c['bd'] = torch.from_numpy(np.array(c['b'])).cuda()
    padded = np.full((N, P, Sy, Hs), SENTINEL, dtype=NP[dt])
    padded[..., :Sx] = c['a']

    def fresh(off, fill):
        buf = torch.full((size + kV,), SENTINEL, dtype=torch_type(dt), device='cuda')
        if fill:
            buf[off:off + size] = torch.from_numpy(padded.reshape(-1)).cuda()
        assert buf.data_ptr() % 16 == 0 and (buf[off:].data_ptr() % 16 == 0) == (off == 0)
        return buf

    def check(buf, off, want, what):
        got = buf.cpu().numpy()
        inside = got[off:off + size].reshape(N, P, Sy, Hs)
        wrong = np.flatnonzero(inside[..., :Sx].reshape(-1) != want.reshape(-1))
        assert bits(inside[..., :Sx]) == bits(want), (name, dt, what, len(wrong), wrong[:8].tolist())
        assert np.all(inside[..., Sx:] == SENTINEL), (what, 'pad columns are not written')
        assert np.all(got[:off] == SENTINEL) and np.all(got[off + size:] == SENTINEL), (what, 'the spare unit is not written')

    for taken, want in ((c['taken'], c['want']), (None, c['untaken'])):
        a_buf = fresh(c['a_off'], True)
        gain_buf = a_buf if c['in_place'] else fresh(c['gain_off'], False)
        assert score_call(c, dt, a_buf, gain_buf, taken) == 0
        check(gain_buf, c['gain_off'], want, 'first run')
        if not c['in_place']:
            check(a_buf, c['a_off'], c['a'], 'the map is read only')
            first = bits(gain_buf.cpu().numpy())
            gain_buf.fill_(SENTINEL)
            assert score_call(c, dt, a_buf, gain_buf, taken) == 0
            assert bits(gain_buf.cpu().numpy()) == first, 'the same bits again'
            if c['a_off'] == c['gain_off']:     # in place on the map
                assert score_call(c, dt, a_buf, a_buf, taken) == 0
                check(a_buf, c['a_off'], want, 'in place')
    assert np.count_nonzero(c['want']) >= 1 and not np.isnan(c['want']).any()
    inside = c['taken'][(c['taken'] >= 0) & (c['taken'] < plan['entries'])]
    assert np.any(c['untaken'].reshape(-1)[inside] != 0), 'the list zeroes entries that scored'
    if len(c['taken']) > 7:        # T1: the five entries only the second pass of the loop meets
        assert np.all(c['untaken'].reshape(-1)[c['taken'][-5:]] > 0) and not c['want'].reshape(-1)[c['taken'][-5:]].any()


# -- pick, gain, landscape, alternatives ---------------------------------------------------------------------------------------
def case(name):
    return sc.events_case(name, device_cus())


def want_of(name, kernel):
    c = case(name)
    return tuple(x[c['pick']] for x in sc.events_reference(name, kernel))


def operands(name, dt):
    c = case(name)
    k = len(c['geo'][4])
    return dev(c['W'], dt), events_of(c['rows'], k), dev(c['h'], dt), dev(c['V'], dt), dev(c['R'], dt)


def geom(geo, dt):
    N, C, P, D, A, _ = geo
    return _lib.make_geom(N, P, C, D, A, DTYPES.index(dt))


def poisoned(K, width=None, dtype=torch.float64):
    return torch.full((K + SLACK,) if width is None else (K + SLACK, width), float('nan'), dtype=dtype, device='cuda')


def split(t, K):
    """(the K rows that are written, the slack behind them) on the host."""
    x = t.cpu().numpy()
    return x[:K], x[K:]


def same(got, want, what):
    wrong = np.flatnonzero((got != want).reshape(-1))
    assert bits(got) == bits(np.asarray(want, dtype=got.dtype)), (what, len(wrong), wrong[:8].tolist(),
                                                                  got.reshape(-1)[wrong[:8]].tolist(),
                                                                  np.asarray(want).reshape(-1)[wrong[:8]].tolist())


def pick_call(name, dt, with_mag=True):
    c = case(name)
    geo = c['geo']
    lib, ctx = context()
    idx = sc.flat_indices(geo, c['rows'])
    K = len(idx)
    Wd, _, _, Vd, Rd = operands(name, dt)
    at = torch.from_numpy(idx).cuda()
    ev = torch.full((K + SLACK, 4), -7, dtype=torch.int32, device='cuda')
    h, gain = poisoned(K, dtype=torch_type(dt)), poisoned(K)
    mag = poisoned(K) if with_mag else None
    g = geom(geo, dt)
    code = lib.tnmf_hip_pursuit_pick(ctx, ctypes.byref(g), _lib.MODES[geo[5]], p(Wd), p(at), K, p(Vd), p(Rd), p(ev), p(h),
                                     p(gain), p(mag), None)
    torch.cuda.synchronize()
    assert code == 0
    return idx, [split(t, K) for t in (ev, h, gain) + ((mag,) if with_mag else ())]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', [n for n in EVENTS if 'pick' in sc.spec_of(n)[2]])
def test_the_pick_is_the_reference_bit_for_bit(name, dt):
    c = case(name)
    geo, good = c['geo'], c['good']
    a, b, want_mag = want_of(name, 'pick')
    idx, outs = pick_call(name, dt)
    (ev, ev_b), (h, h_b), (gain, gain_b), (mag, mag_b) = outs
    assert np.all(ev_b == -7) and np.isnan(h_b).all() and np.isnan(gain_b).all() and np.isnan(mag_b).all(), 'behind the outputs'
    assert not np.isnan(h).any() and not np.isnan(gain).any() and not np.isnan(mag).any(), 'every element is written'
    same(ev, sc.pick_decode(geo, idx).astype(np.int32), 'the decoded rows')
    k = len(geo[4])
    assert np.array_equal(ev[good][:, [0, 1] + list(range(4 - k, 4))], c['rows'][good]) and np.all(ev[~good] == -1)
    want_h, want_gain = sc.pick_outputs(a, b, dt)
    same(mag, want_mag, 'mag')
    same(h, want_h, 'strength = NP[dt](a / b)')
    same(gain, want_gain, 'gain = a * a / (2. * b)')
    assert not h[~good].any() and not gain[~good].any() and not mag[~good].any()
    if 'K4:b==0' in sc.MATRIX[name][2].get('pick', ()):
        dead = good & (b == 0)
        assert dead.any() and not h[dead].any() and not gain[dead].any()
    _, again = pick_call(name, dt)
    assert all(bits(x[0]) == bits(y[0]) for x, y in zip(again, outs)), 'the same bits again'
    _, bare = pick_call(name, dt, with_mag=False)
    assert len(bare) == 3 and all(bits(x[0]) == bits(y[0]) and bits(x[1]) == bits(y[1]) for x, y in zip(bare, outs)), 'without mag'


def gain_call(name, dt, with_mag=True):
    c = case(name)
    geo = c['geo']
    lib, ctx = context()
    K = len(c['rows'])
    Wd, ev, hd, Vd, Rd = operands(name, dt)
    gain = poisoned(K)
    mag = poisoned(K) if with_mag else None
    g = geom(geo, dt)
    code = lib.tnmf_hip_events_gain(ctx, ctypes.byref(g), _lib.MODES[geo[5]], p(Wd), p(ev), p(hd), K, p(Vd), p(Rd), p(gain),
                                    p(mag), None)
    torch.cuda.synchronize()
    assert code == 0
    return [split(t, K) for t in (gain,) + ((mag,) if with_mag else ())]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', [n for n in EVENTS if 'gain' in sc.spec_of(n)[2]])
def test_the_gain_is_the_closed_form_bit_for_bit(name, dt):
    c = case(name)
    good = c['good']
    want, want_mag = want_of(name, 'gain')
    outs = gain_call(name, dt)
    (gain, gain_b), (mag, mag_b) = outs
    assert np.isnan(gain_b).all() and np.isnan(mag_b).all(), 'behind the outputs'
    assert not np.isnan(gain).any() and not np.isnan(mag).any(), 'every element is written'
    same(gain, want, 'gain')
    same(mag, want_mag, 'mag')
    assert not gain[~good].any() and not mag[~good].any() and np.count_nonzero(gain) > 0
    dead = good & (c['h'] == 0)
    assert not gain[dead].any() and not mag[dead].any()
    again = gain_call(name, dt)
    assert all(bits(x[0]) == bits(y[0]) for x, y in zip(again, outs)), 'the same bits again'
    bare = gain_call(name, dt, with_mag=False)
    assert len(bare) == 1 and bits(bare[0][0]) == bits(gain) and np.isnan(bare[0][1]).all(), 'without mag'


def landscape_call(geo, dt, Wd, ev, hd, Vd, Rd, with_mag=True):
    lib, ctx = context()
    K, nb = len(ev), 3 ** len(geo[4])
    outs = [poisoned(K, nb) for _ in range(3 if with_mag else 2)]
    g = geom(geo, dt)
    code = lib.tnmf_hip_events_landscape(ctx, ctypes.byref(g), _lib.MODES[geo[5]], p(Wd), p(ev), p(hd), K, p(Vd), p(Rd),
                                         p(outs[0]), p(outs[1]), p(outs[2]) if with_mag else None, None)
    torch.cuda.synchronize()
    assert code == 0
    return [split(t, K) for t in outs]


def alternatives_call(geo, dt, n_alt, stride, Wd, ev, hd, Vd, Rd, with_mag=True):
    lib, ctx = context()
    K = len(ev)
    outs = [poisoned(K, n_alt) for _ in range(3 if with_mag else 2)]
    g = geom(geo, dt)
    code = lib.tnmf_hip_events_alternatives(ctx, ctypes.byref(g), _lib.MODES[geo[5]], p(Wd), p(ev), p(hd), K, p(Vd), p(Rd),
                                            n_alt, stride, p(outs[0]), p(outs[1]), p(outs[2]) if with_mag else None, None)
    torch.cuda.synchronize()
    assert code == 0
    return [split(t, K) for t in outs]


def check_sums(call, name, kernel):
    c = case(name)
    good = c['good']
    want = want_of(name, kernel)
    outs = call(True)
    for (got, behind), ref, what in zip(outs, want, ('a', 'b', 'mag')):
        assert np.isnan(behind).all(), (what, 'behind the output')
        assert not np.isnan(got).any(), (what, 'every element is written', np.argwhere(np.isnan(got))[:8].tolist())
        same(got, ref, what)
        assert not got[~good].any()
    assert np.count_nonzero(outs[0][0]) > 0
    again = call(True)
    assert all(bits(x[0]) == bits(y[0]) for x, y in zip(again, outs)), 'the same bits again'
    bare = call(False)
    assert len(bare) == 2 and all(bits(x[0]) == bits(y[0]) and np.isnan(x[1]).all() for x, y in zip(bare, outs)), 'without mag'
    return outs


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', [n for n in EVENTS if 'landscape' in sc.spec_of(n)[2]])
def test_the_landscape_is_the_reference_bit_for_bit(name, dt):
    c = case(name)
    geo, ops = c['geo'], operands(name, dt)
    (a, _), (b, _), _ = check_sums(lambda with_mag: landscape_call(geo, dt, *ops, with_mag=with_mag), name, 'landscape')
    paths = sc._paths(sc.landscape_staged, geo, c['rows'])
    claims = sc.MATRIX[name][2].get('landscape', ())
    if 'staged' in claims or any(n.startswith('L1') for n in claims):
        assert np.any(paths == 's') and np.any(paths == 'w')
    if 'L4:full-S==1' in claims:       # only the centre neighbour exists
        centre = (a.shape[1] - 1) // 2
        assert b[c['good'], centre].all() and not np.delete(b, centre, axis=1).any()


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', [n for n in EVENTS if 'alternatives' in sc.spec_of(n)[2]])
def test_the_alternatives_are_the_reference_bit_for_bit(name, dt):
    c = case(name)
    geo, ops = c['geo'], operands(name, dt)
    check_sums(lambda with_mag: alternatives_call(geo, dt, c['n_alt'], c['stride'], *ops, with_mag=with_mag), name,
               'alternatives')
    paths = sc._paths(sc.alternatives_staged, geo, c['rows'])
    claims = sc.MATRIX[name][2].get('alternatives', ())
    if 'staged' in claims or 'staged-after-walk-in-one-wave' in claims:
        assert np.any(paths == 's') and np.any(paths == 'w')
    if 'A1:zero-fill-beyond-a-wave' in claims:
        assert c['n_alt'] > 64 and np.any(paths == 'x')


# -- the staged rows forced onto the walk --------------------------------------------------------------------------------------
def far_shift(geo, gap):
    """The shift whose occurrence ends `gap` pixels in front of the far border of the sample on every axis."""
    _, _, _, D, A, mode = geo
    return [(a - 1 if mode == 'valid' else 0) + d - a - gap for d, a in zip(D, A)]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', ['landscape-limit-fits', 'stride-4'])
def test_a_staged_landscape_row_equals_the_same_row_on_the_walk(name, dt):
    """An atom one pixel from the far border of the sample takes the staged path.  Cut the last row and column of pixels off V
    and R and the same atom over the same pixels sits ON the border: its far neighbours are clipped, the row walks.  The
    neighbours both problems have -- the offsets <= 0 on every axis -- see the same pixels: bit for bit the same sums."""
    c = case(name)
    geo = c['geo']
    N, C, P, D, A, mode = geo
    k = len(D)
    cut = (N, C, P, tuple(d - 1 for d in D), A, mode)
    row = np.array([[0, P - 1] + far_shift(geo, 1)], dtype=np.int64)
    uy, ux = sc._shifts2(geo, row)
    assert sc.landscape_staged(geo, int(uy[0]), int(ux[0])) and not sc.landscape_staged(cut, int(uy[0]), int(ux[0]))
    assert sc.in_range(cut, row)[0]
    crop = (slice(None), slice(None)) + (slice(None, -1),) * k
    h = np.array([1.5])
    shared = [j for j, delta in enumerate(sc.lref.deltas(k)) if max(delta) <= 0]
    out = {}
    for which, g, V, R in (('staged', geo, c['V'], c['R']), ('walk', cut, c['V'][crop], c['R'][crop])):
        got = landscape_call(g, dt, dev(c['W'], dt), events_of(row, k), dev(h, dt), dev(V, dt), dev(R, dt))
        want = sc.lref.landscape(V, R, c['W'], mode, row[:, 0], row[:, 1], row[:, 2:], h)
        for (x, _), y, what in zip(got, want, ('a', 'b', 'mag')):
            same(x, y + 0., f'{which} {what}')
        out[which] = [x[0][0] for x in got]
    assert len(shared) == 2 ** k
    for x, y in zip(out['staged'], out['walk']):
        assert bits(x[shared]) == bits(y[shared])
    assert out['staged'][1].all() and np.count_nonzero(out['walk'][1]) == 3 ** k


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', ['alternatives-limit-fits', 'stride-4'])
def test_a_staged_alternatives_row_equals_the_same_row_on_the_walk(name, dt):
    """An atom whose last pixel is the last pixel of the sample takes the staged path.  Cut that last row and column of pixels
    off V and R and the same atom hangs over the border: the walk.  With planes whose last row and column of taps are zero
    both see the same pixels under the same taps -- the clipped taps add exact zeros on the staged path."""
    c = case(name)
    geo = c['geo']
    N, C, P, D, A, mode = geo
    k = len(D)
    cut = (N, C, P, tuple(d - 1 for d in D), A, mode)
    row = np.array([[0, P - 1] + far_shift(geo, 0)], dtype=np.int64)
    uy, ux = sc._shifts2(geo, row)
    assert sc.alternatives_staged(geo, int(uy[0]), int(ux[0])) and not sc.alternatives_staged(cut, int(uy[0]), int(ux[0]))
    assert sc.in_range(cut, row)[0]
    W = np.array(c['W'])
    W[:, :, -1, :] = 0.
    W[:, :, :, -1] = 0.
    crop = (slice(None), slice(None)) + (slice(None, -1),) * k
    h = np.array([1.5])
    out = {}
    for which, g, V, R in (('staged', geo, c['V'], c['R']), ('walk', cut, c['V'][crop], c['R'][crop])):
        got = alternatives_call(g, dt, c['n_alt'], c['stride'], dev(W, dt), events_of(row, k), dev(h, dt), dev(V, dt), dev(R, dt))
        want = sc.aref.alternatives(V, R, W, mode, row[:, 0], row[:, 1], row[:, 2:], h, c['n_alt'], c['stride'])
        for (x, _), y, what in zip(got, want, ('a', 'b', 'mag')):
            same(x, y + 0., f'{which} {what}')
        out[which] = [x[0][0] for x in got]
    for x, y in zip(out['staged'], out['walk']):
        assert bits(x) == bits(y)
    assert out['staged'][1].all()
