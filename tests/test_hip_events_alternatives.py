"""
The alternatives of events on the GPU: tnmf_hip_events_alternatives through the C ABI, and ``detection_alternatives`` /
``relabel_detections`` on ``backend='hip'``, against tests/alternatives_reference.py evaluated in extended precision on the SAME
V, W, strengths and on the R the device rendered, read back.

The bars are those tests/test_hip_events_landscape.py holds tnmf_hip_events_landscape to (derived there), the sums being the
same ones at delta = 0: per row and candidate |a - ref| <= 8 * taps * 2^-52 * mag, taps = C * prod(A) and mag = sum |w' d_e| the
sum of the magnitudes of the terms of a; b (all its terms are positive: it is its own magnitude) and mag to the same relative
bar.  Here too a sum has at most 4 * taps terms (an occurrence has at most four images).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import alternatives_reference as aref
import events_reference as eref
import landscape_reference as lref
from test_events_alternatives_cpu import cells, holding, planted_det
from test_events_landscape_cpu import key
from test_hip_events import BAR, DTYPES, NP, backend, dev, p
from test_hip_events_gain import SENTINEL, events_of
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF

pytestmark = pytest.mark.gpu

MODES = ['valid', 'full', 'circular', 'reflect']
N = 2
BLOCKS_PER_CU, WAVES = 4, 4        # alternatives.hip: TNMF_ALTERNATIVES_BLOCKS_PER_CU, kWaves
B = aref.BATCH
# tap counts on both sides of a wave: 9, 64 and 105
GEOMETRIES = {'3x3-c1': ((12, 14), (3, 3), 1), '8x8-c1': ((20, 22), (8, 8), 1), '5x7-c3': ((12, 14), (5, 7), 3)}
# (geometry, planes, n_alt, stride): n_alt = 1, one below the batch, the batch, one above it, and 24 = 3 atoms x dihedral
SETS = [('3x3-c1', 24, 24, 1), ('3x3-c1', 24, 3, 8), ('3x3-c1', 2, 1, 1), ('8x8-c1', 2 * (B - 1), B - 1, 1),
        ('8x8-c1', 2 * (B - 1), B - 1, 2), ('8x8-c1', 2 * B, B, 2), ('8x8-c1', B + 1, B + 1, 1), ('5x7-c3', 2 * (B + 1), B + 1, 2),
        ('5x7-c3', 3, 1, 3), ('5x7-c3', B, B, 1)]
assert B == 4 and sorted({s[2] for s in SETS}) == [1, B - 1, B, B + 1, 24] and {s[3] > 1 for s in SETS} == {False, True}


@functools.lru_cache(maxsize=None)
def rows_of_case(name, mode, P):
    """-> (rows [K, 2 + k], h, W, V, good): every place of landscape_reference.places() under planes that run through the
    dictionary, duplicates, a zero strength -- with rows outside the contract between them; float32-representable,
    read-only."""
    D, A, C = GEOMETRIES[name]
    S = eref.shift_shape(D, A, mode)
    k = len(D)
    rng = np.random.default_rng(31)
    W, V = rng.random((P, C) + A) + 0.1, rng.random((N, C) + D) * 2.
    at = lref.places(D, A, mode)
    names = list(at) + ['interior', 'corner0']
    shift = np.array([at[n] for n in names], dtype=np.int64)
    plane = ((5 * np.arange(len(names)) + 1) % P).astype(np.int64)
    plane[-2:] = plane[[names.index('interior'), names.index('corner0')]]
    h = rng.random(len(names)) + 0.5
    h[-2:] = h[[names.index('interior'), names.index('corner0')]]
    h[names.index('far')] = 0.
    rows = np.column_stack([np.ones(len(names), dtype=np.int64), plane, shift])
    extra = np.column_stack([[0, 0, 0], [0, P - 1, P // 2]] + [rng.integers(s, size=3) for s in S])
    rows, h = np.concatenate([rows, extra]).astype(np.int64), np.concatenate([h, [1., 0.5, 2.]])
    bad = np.array([[N, 0] + [0] * k, [-1, 0] + [0] * k, [0, P] + [0] * k, [0, -2] + [0] * k,
                    [1, P - 1] + [S[0]] + [0] * (k - 1), [1, P - 1] + [0] * (k - 1) + [-1]], dtype=np.int64)
    where = np.array([3, 3, 6, 6, 9, 9])
    rows = np.insert(rows, where, bad, axis=0)
    h = np.insert(h, where, 1.)
    good = np.ones(len(rows), dtype=bool)
    good[where + np.arange(len(where))] = False
    assert not np.any([lref.in_range(N, P, S, r[0], r[1], r[2:]) for r in rows[~good]])
    assert np.all([lref.in_range(N, P, S, r[0], r[1], r[2:]) for r in rows[good]])
    f32 = lambda x: np.asarray(x).astype(np.float32).astype(np.float64)   # noqa: E731
    out = (rows, f32(h), f32(W), f32(V), good)
    for x in out:
        x.setflags(write=False)
    return out


def context():
    return backend(2, 2, 3, (20, 23), (4, 6), 'circular', 'f32')            # any context: the entry takes its geometry per call


def launch(geo, dt, n_alt, stride, Wd, ev, hd, Vd, Rd, with_mag=True, fill=float('nan')):
    """-> (code, a, b, mag) of one call on poisoned outputs."""
    n, C, planes, D, A, mode = geo
    be = context()
    K = len(ev)
    a = torch.full((K, n_alt), fill, dtype=torch.float64, device='cuda')
    b = torch.full((K, n_alt), fill, dtype=torch.float64, device='cuda')
    mag = torch.full((K, n_alt), fill, dtype=torch.float64, device='cuda') if with_mag else None
    g = _lib.make_geom(n, planes, C, D, A, DTYPES.index(dt))
    code = be._lib.tnmf_hip_events_alternatives(be._ctx, ctypes.byref(g), _lib.MODES[mode], p(Wd), p(ev), p(hd), K, p(Vd),
                                                p(Rd), n_alt, stride, p(a), p(b), p(mag), None)
    torch.cuda.synchronize()
    return code, a.cpu().numpy(), b.cpu().numpy(), None if mag is None else mag.cpu().numpy()


def device_render(geo, dt, rows, h, W):
    """R of the rows inside the contract as the device renders it, on the device."""
    n, C, planes, D, A, mode = geo
    be = backend(n, C, planes, D, A, mode, dt)
    return be.render_events(dev(W, dt), rows[:, 0], rows[:, 1], rows[:, 2:], np.asarray(h, dtype=NP[dt]))


def geo_of(name, mode, P):
    D, A, C = GEOMETRIES[name]
    return (N, C, P, D, A, mode)


@functools.lru_cache(maxsize=None)
def run(name, P, n_alt, stride, mode, dt):
    """-> (a, b, mag, reference a, b, mag, operands) of the case, the reference on the device's own R."""
    rows, h, W, V, good = rows_of_case(name, mode, P)
    geo = geo_of(name, mode, P)
    Rd = device_render(geo, dt, rows[good], h[good], W)
    operands = (dev(W, dt), events_of(rows, len(geo[3])), dev(h, dt), dev(V, dt), Rd)
    code, a, b, mag = launch(geo, dt, n_alt, stride, *operands)
    assert code == 0
    R = Rd.cpu().numpy().astype(np.float64)
    want = aref.alternatives(V, R, W, mode, rows[:, 0], rows[:, 1], rows[:, 2:], h, n_alt, stride)
    return (a, b, mag) + want + (operands,)


def within_the_bars(a, b, mag, ra, rb, rmag, taps, what):
    bar = 8 * taps * 2. ** -52
    live = rmag > 0
    worst = [float(np.max(e[live] / s[live])) for e, s in ((np.abs(a - ra), rmag), (np.abs(b - rb), rb),
                                                          (np.abs(mag - rmag), rmag))]
    print(f'{what}: taps {taps}; |a - ref| / mag <= {worst[0]:.3g}, |b - ref| / b <= {worst[1]:.3g}, '
          f'|mag - ref| / mag <= {worst[2]:.3g}, bar {bar:.3g}')
    assert np.all(np.abs(a - ra) <= bar * rmag) and np.all(np.abs(b - rb) <= bar * rb)
    assert np.all(np.abs(mag - rmag) <= bar * rmag)
    return bar


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', SETS, ids=lambda s: f'{s[0]}-P{s[1]}-n{s[2]}-s{s[3]}')
def test_parity_with_the_reference(case, mode, dt):
    name, P, n_alt, stride = case
    rows, h, W, V, good = rows_of_case(name, mode, P)
    geo = geo_of(name, mode, P)
    a, b, mag, ra, rb, rmag, operands = run(name, P, n_alt, stride, mode, dt)
    taps = geo[1] * int(np.prod(geo[4]))
    assert not np.isnan(a).any() and not np.isnan(b).any() and not np.isnan(mag).any(), 'every element is written'
    st = aref.staged(geo, rows[:, 2:]) & good
    within_the_bars(a, b, mag, ra, rb, rmag, taps, f'{name} {mode} {dt} n_alt {n_alt} stride {stride}: {len(rows)} rows '
                    f'({int(st.sum())} staged)')
    # rows outside the contract: exactly 0; every candidate of a row inside it has a pixel in the sample
    assert not a[~good].any() and not b[~good].any() and not mag[~good].any() and (~good).sum() == 6
    assert np.all(b[good] > 0)
    # both paths ran (the host mirror of the rule; in 'full' every occurrence is whole: its walk is the patch limit's test)
    assert st.any() and ((good & ~st).sum() >= 4 or mode == 'full')
    # the same bits again, and without mag
    code, a2, b2, mag2 = launch(geo, dt, n_alt, stride, *operands)
    assert code == 0 and a2.tobytes() == a.tobytes() and b2.tobytes() == b.tobytes() and mag2.tobytes() == mag.tobytes()
    code, a3, b3, none = launch(geo, dt, n_alt, stride, *operands, with_mag=False)
    assert code == 0 and none is None and a3.tobytes() == a.tobytes() and b3.tobytes() == b.tobytes()


def test_the_cases_reach_what_they_are_for():
    """Over the cases: rows of one, two and four images, both paths, tap counts on both sides of a wave."""
    assert sorted({GEOMETRIES[n][2] * int(np.prod(GEOMETRIES[n][1])) for n in GEOMETRIES}) == [9, 64, 105]
    for mode in MODES:
        for name, P, n_alt, stride in SETS:
            rows, h, W, V, good = rows_of_case(name, mode, P)
            D, A, C = GEOMETRIES[name]
            S = eref.shift_shape(D, A, mode)
            n_images = {len(eref.images(r[2:], A, S, mode)) for r in rows[good]}
            assert n_images == ({1} if mode in ('valid', 'full') else {1, 2, 4})
            assert np.count_nonzero(h[good] == 0) == 1 and P % (n_alt * stride) == 0
            st = aref.staged(geo_of(name, mode, P), rows[:, 2:]) & good
            assert st.any() and ((good & ~st).any() or mode == 'full')
            # the rows' own planes sit at more than one place of the progression
            assert len({aref.candidates(int(r[1]), n_alt, stride)[1] for r in rows[good]}) > 1 or n_alt == 1


# -- the seam between the paths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', list(GEOMETRIES))
def test_the_seam_between_the_paths(name, dt):
    """An atom whose first pixel is the first pixel of the sample takes the staged path.  Cut that first row and column of
    pixels off V and R and the same atom hangs over the border: the walk.  With planes whose first row and column of taps
    are zero both see the same pixels under the same taps -- the clipped taps add exact zeros on the staged path -- so they
    agree within the bars, and bit for bit, since both paths add the same terms in the same order."""
    D, A, C = GEOMETRIES[name]
    k, mode, P, n_alt, stride = len(D), 'valid', 10, 5, 2
    rng = np.random.default_rng(5)
    W = (rng.random((P, C) + A) + 0.1).astype(np.float32).astype(np.float64)
    W[:, :, 0, :] = 0.
    W[:, :, :, 0] = 0.
    V = (rng.random((N, C) + D) * 2.).astype(np.float32).astype(np.float64)
    R = (V * (0.5 + rng.random(V.shape))).astype(np.float32).astype(np.float64)   # (need not be anyone's render)
    first = [a - 1 for a in A]
    row, cut_row = np.array([[1, 3] + first], dtype=np.int64), np.array([[1, 3] + [f - 1 for f in first]], dtype=np.int64)
    geo, cut = (N, C, P, D, A, mode), (N, C, P, tuple(d - 1 for d in D), A, mode)
    assert aref.staged(geo, row[:, 2:])[0] and not aref.staged(cut, cut_row[:, 2:])[0]
    crop = (slice(None), slice(None)) + (slice(1, None),) * k
    hh = np.array([1.25])
    out = {}
    for which, g, r, v_, r_ in (('staged', geo, row, V, R), ('walk', cut, cut_row, V[crop], R[crop])):
        code, a, b, mag = launch(g, dt, n_alt, stride, dev(W, dt), events_of(r, k), dev(hh, dt), dev(v_, dt), dev(r_, dt))
        assert code == 0
        want = aref.alternatives(v_, r_, W, mode, r[:, 0], r[:, 1], r[:, 2:], hh, n_alt, stride)
        within_the_bars(a, b, mag, *want, C * int(np.prod(A)), f'{name} {dt} {which}')
        out[which] = (a[0], b[0], mag[0])
    for x, y in zip(out['staged'], out['walk']):
        print(f'{name} {dt}: staged - walk {np.abs(x - y).max():.3g}')
        assert x.tobytes() == y.tobytes()
    assert out['staged'][1].all()


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('A', [1024, 1025])
def test_the_patch_limit_of_the_staged_path(A, dt):
    """C * A = 2048 doubles is the largest patch a wave stages -- 64 KiB of LDS for the four waves of a workgroup; with one
    tap more per channel the patch does not fit and every row of the geometry walks.  Either way the same bars hold."""
    geo = n, C, planes, D, _, mode = (1, 2, 2, (1030,), (A,), 'valid')
    assert (C * A <= aref.PATCH_MAX) == (A == 1024) and C * 1024 == aref.PATCH_MAX
    rows = np.array([[0, 0, A - 1 + 3], [0, 1, A - 1], [0, 1, A - 1 + D[0] - A], [0, 0, 0], [0, 1, D[0] + A - 2]],
                    dtype=np.int64)
    assert aref.staged(geo, rows[:, 2:]).tolist() == [A == 1024, A == 1024, A == 1024, False, False]
    rng = np.random.default_rng(A)
    W = (rng.random((planes, C, A)) + 0.1).astype(np.float32).astype(np.float64)
    V = (rng.random((n, C) + D) * 3.).astype(np.float32).astype(np.float64)
    R = (V * (0.5 + rng.random(V.shape))).astype(np.float32).astype(np.float64)
    h = np.array([1.25, 0.5, 2., 1., 0.75])
    operands = (dev(W, dt), events_of(rows, 1), dev(h, dt), dev(V, dt), dev(R, dt))
    code, a, b, mag = launch(geo, dt, 2, 1, *operands)
    assert code == 0 and not np.isnan(a).any() and not np.isnan(b).any() and not np.isnan(mag).any()
    want = aref.alternatives(V, R, W, mode, rows[:, 0], rows[:, 1], rows[:, 2:], h, 2, 1)
    within_the_bars(a, b, mag, *want, C * A, f'A = {A} {dt}')
    assert np.all(want[2] > 0)
    code, a2, b2, mag2 = launch(geo, dt, 2, 1, *operands)
    assert code == 0 and a2.tobytes() == a.tobytes() and b2.tobytes() == b.tobytes() and mag2.tobytes() == mag.tobytes()


# -- the identities with the gains and the landscape ----------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('mode', MODES)
def test_identities_with_the_gains_and_the_landscape_on_the_device(mode, dt):
    name, P, n_alt, stride = '5x7-c3', 2 * (B + 1), B + 1, 2
    rows, h, W, V, good = rows_of_case(name, mode, P)
    n, C, planes, D, A, _ = geo_of(name, mode, P)
    a, b, mag, _, _, rmag, (Wd, ev, hd, Vd, Rd) = run(name, P, n_alt, stride, mode, dt)
    be = context()
    K = len(rows)
    g = _lib.make_geom(n, planes, C, D, A, DTYPES.index(dt))
    gain = torch.empty(K, dtype=torch.float64, device='cuda')
    gmag = torch.empty(K, dtype=torch.float64, device='cuda')
    out = []
    for strengths in (hd, torch.ones_like(hd)):
        assert be._lib.tnmf_hip_events_gain(be._ctx, ctypes.byref(g), _lib.MODES[mode], p(Wd), p(ev), p(strengths), K, p(Vd),
                                            p(Rd), p(gain), p(gmag), None) == 0
        torch.cuda.synchronize()
        out.append((gain.cpu().numpy().copy(), gmag.cpu().numpy().copy()))
    (gain_h, mag_h), (gain_1, mag_1) = out
    la, lb, lm = (torch.empty((K, 9), dtype=torch.float64, device='cuda') for _ in range(3))
    assert be._lib.tnmf_hip_events_landscape(be._ctx, ctypes.byref(g), _lib.MODES[mode], p(Wd), p(ev), p(hd), K, p(Vd), p(Rd),
                                             p(la), p(lb), p(lm), None) == 0
    torch.cuda.synchronize()
    la, lb, lm = (x.cpu().numpy()[:, 4] for x in (la, lb, lm))
    own = np.array([aref.candidates(int(r[1]), n_alt, stride)[1] if ok else 0 for r, ok in zip(rows, good)])
    every = np.arange(K)
    a0, b0, m0, r0 = a[every, own], b[every, own], mag[every, own], rmag[every, own]
    hv = np.asarray(h, dtype=np.float64)
    bar = 8 * C * int(np.prod(A)) * 2. ** -52
    # column j_own against the centre of the landscape: the same sums
    same = [x.tobytes() == y.tobytes() for x, y in ((a0, la), (b0, lb), (m0, lm))]
    print(f'{mode} {dt}: column j_own and the centre of the landscape have equal bits (a, b, mag): {same}; '
          f'|a - a_landscape| / mag <= {np.max(np.abs(a0 - la)[good] / r0[good]):.3g}')
    assert np.all(np.abs(a0 - la) <= 4 * bar * r0) and np.all(np.abs(b0 - lb) <= 4 * bar * b0)
    assert np.all(np.abs(m0 - lm) <= 4 * bar * r0)
    # a_e of the gains, read off a call with strengths 1 against the same R: gain = a_e + b / 2
    a_e = gain_1 - 0.5 * b0
    scale = r0 + hv * b0 + mag_1
    print(f'{mode} {dt}: |a_0 - h b_0 - a_e| / scale <= {np.max(np.abs(a0 - hv * b0 - a_e)[good] / scale[good]):.3g}, '
          f'|h a_e + h^2 b_0 / 2 - gain| / scale <= '
          f'{np.max(np.abs(hv * (a0 - hv * b0) + 0.5 * hv * hv * b0 - gain_h)[good] / (hv * scale + mag_h + 1e-300)[good]):.3g}')
    assert np.all(np.abs(a0 - hv * b0 - a_e) <= 4 * bar * scale)
    assert np.all(np.abs(hv * (a0 - hv * b0) + 0.5 * hv * hv * b0 - gain_h) <= 4 * bar * (hv * scale + mag_h))
    assert np.abs(gain_h[good]).max() > 0


# -- the output contract --------------------------------------------------------------------------------------------------------
def test_many_rows_run_the_grid_stride_loop():
    """8 000 rows, duplicates among them, on the 2 x 2 x 12 x 14 problem: more workgroups' worth than the grid has."""
    geo = n, C, planes, D, A, mode = (2, 2, 8, (12, 14), (3, 3), 'reflect')
    n_alt, stride = 4, 2
    S = eref.shift_shape(D, A, mode)
    rng = np.random.default_rng(8)
    K = 8000
    assert -(-K // WAVES) > torch.cuda.get_device_properties(0).multi_processor_count * BLOCKS_PER_CU
    pool = np.column_stack([rng.integers(n, size=300), rng.integers(planes, size=300)]
                           + [rng.integers(s, size=300) for s in S]).astype(np.int64)
    pick = rng.integers(300, size=K)                                 # 300 places with their strengths, drawn 8 000 times
    rows, h = pool[pick], (rng.integers(0, 4, 300) / 4.)[pick]
    W = (rng.random((planes, C) + A) + 0.1).astype(np.float32).astype(np.float64)
    V = (rng.random((n, C) + D) * 3.).astype(np.float32).astype(np.float64)
    R = (V * (0.5 + rng.random(V.shape))).astype(np.float32).astype(np.float64)
    operands = (dev(W, 'f32'), events_of(rows, 2), dev(h, 'f32'), dev(V, 'f32'), dev(R, 'f32'))
    code, a, b, mag = launch(geo, 'f32', n_alt, stride, *operands)
    assert code == 0 and not np.isnan(a).any() and not np.isnan(b).any() and not np.isnan(mag).any()
    # the reference per DISTINCT (row, strength): the same row against the same R has the same alternatives
    full = np.column_stack([rows.astype(np.float64), h])
    distinct, inverse = np.unique(full, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    d_rows = distinct[:, :-1].astype(np.int64)
    want = tuple(x[inverse] for x in aref.alternatives(V, R, W, mode, d_rows[:, 0], d_rows[:, 1], d_rows[:, 2:],
                                                       distinct[:, -1], n_alt, stride))
    within_the_bars(a, b, mag, *want, C * 9, f'{K} rows')
    st = aref.staged(geo, rows[:, 2:])
    assert st.sum() > 1000 and (~st).sum() > 1000
    code, a2, b2, mag2 = launch(geo, 'f32', n_alt, stride, *operands)
    assert code == 0 and a2.tobytes() == a.tobytes() and b2.tobytes() == b.tobytes() and mag2.tobytes() == mag.tobytes()
    first = np.unique(inverse, return_index=True)[1]
    assert np.array_equal(a, a[first][inverse]) and np.array_equal(b, b[first][inverse])


def test_refused_calls_write_nothing():
    name, mode, P, n_alt, stride = '3x3-c1', 'circular', 24, 3, 8
    rows, h, W, V, good = rows_of_case(name, mode, P)
    n, C, planes, D, A, _ = geo_of(name, mode, P)
    be = context()
    lib, ctx = be._lib, be._ctx
    K = len(rows)
    Wd, hd, Vd, ev = dev(W, 'f32'), dev(h, 'f32'), dev(V, 'f32'), events_of(rows, 2)
    Rd = dev(V * 0.5, 'f32')
    outs = [torch.full((K, 24), SENTINEL, dtype=torch.float64, device='cuda') for _ in range(3)]
    E_NULL, E_DTYPE = -1, -3

    def geom(**kw):
        g = _lib.make_geom(n, planes, C, D, A, 0)
        for key_, val in kw.items():
            setattr(g, key_, val)
        return ctypes.byref(g)

    def call(g, m=_lib.MODES[mode], W_=Wd, ev_=ev, st=hd, k_=K, V_=Vd, R_=Rd, na=n_alt, sd=stride, a_=outs[0], b_=outs[1],
             mg=outs[2], c=ctx):
        return lib.tnmf_hip_events_alternatives(c, g, m, p(W_), p(ev_), p(st), k_, p(V_), p(R_), na, sd, p(a_), p(b_), p(mg),
                                                None)

    assert call(geom(), c=None) == E_NULL and call(None) == E_NULL
    for kw in (dict(W_=None), dict(ev_=None), dict(st=None), dict(V_=None), dict(R_=None), dict(a_=None), dict(b_=None)):
        assert call(geom(), **kw) == E_NULL, kw
    assert call(geom(dtype=2)) == E_DTYPE and call(geom(dtype=-1)) == E_DTYPE
    assert call(geom(ndim=3)) == _lib.E_UNSUPPORTED
    assert call(geom(), k_=(2 ** 31 - 1) // 3 + 1) == _lib.E_UNSUPPORTED and call(geom(), k_=2 ** 31) == _lib.E_UNSUPPORTED
    assert call(geom(), k_=(2 ** 31 - 1) // 24 + 1, na=24, sd=1) == _lib.E_UNSUPPORTED
    for kw in (dict(ndim=0), dict(ndim=4), dict(N=-1), dict(M=0), dict(C=0)):
        assert call(geom(**kw)) == _lib.E_GEOM, kw
    assert call(geom(), m=4) == _lib.E_GEOM and call(geom(), m=-1) == _lib.E_GEOM and call(geom(), k_=-1) == _lib.E_GEOM
    for na, sd in ((0, 1), (-1, 1), (3, 0), (3, -8), (5, 1), (3, 3), (24, 2), (48, 1), (7, 8), (2 ** 16, 2 ** 16)):
        assert call(geom(), na=na, sd=sd) == _lib.E_GEOM, (na, sd)
    assert call(geom(M=25)) == _lib.E_GEOM                             # a block that does not divide the planes
    g = _lib.make_geom(n, planes, C, (1, 14), (3, 3), 0)             # circular: more than one wrap
    assert call(ctypes.byref(g)) == _lib.E_GEOM
    g = _lib.make_geom(n, planes, C, (2, 14), (3, 3), 0)             # reflect: a mirror without the edge
    assert call(ctypes.byref(g), m=_lib.MODES['reflect']) == _lib.E_GEOM
    assert call(ctypes.byref(g), m=_lib.MODES['full']) == _lib.E_GEOM   # full: no shift at all
    # nothing to do: OK, and nothing written -- with every operand NULL as well
    assert call(geom(), k_=0) == 0 and call(geom(N=0)) == 0
    assert call(geom(), k_=0, W_=None, ev_=None, st=None, V_=None, R_=None, a_=None, b_=None, mg=None) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.all(o == SENTINEL)) for o in outs)
    assert call(geom()) == 0                                          # (and the call they were all one step from)
    torch.cuda.synchronize()
    flat = [o.reshape(-1) for o in outs]
    assert not any(bool(torch.any(o[:K * n_alt] == SENTINEL)) for o in flat)
    assert all(bool(torch.all(o[K * n_alt:] == SENTINEL)) for o in flat)   # [K, n_alt] and not an element more


# -- the front end --------------------------------------------------------------------------------------------------------------
def hip_holding(W, V, mode, dt, transforms=None):
    nmf = TransformInvariantNMF(n_atoms=W.shape[0], atom_shape=W.shape[2:], backend='hip', reconstruction_mode=mode,
                                transforms=transforms)
    nmf._W = dev(W, dt)
    np.random.seed(42)
    nmf.fit(np.array(V, dtype=NP[dt]), n_iterations=0, keep_W=True)
    assert np.array_equal(nmf.W.astype(np.float64), W)
    return nmf


@pytest.mark.parametrize('dt', DTYPES)
def test_the_front_end_returns_what_the_float64_host_route_returns(dt):
    sc = cells()
    host = holding(sc['W'], sc['V'], sc['mode'], 'rot90')
    nmf = hip_holding(sc['W'], sc['V'], sc['mode'], dt, 'rot90')
    before = (nmf.H.copy(), nmf.W.copy(), nmf._backend._V_dev.clone())
    start, true = planted_det(sc, sc['wrong']), planted_det(sc, sc['rows'])
    for over, shape in (('transforms', (20, 4)), ('atoms', (20, 2)), ('all', (20, 2, 4))):
        a, b = nmf.detection_alternatives(start, over)
        wa, wb = host.detection_alternatives(start, over)
        assert a.shape == b.shape == shape and a.dtype == b.dtype == np.float64
        print(f'{dt} {over}: |a - host| <= {np.abs(a - wa).max() / np.abs(wa).max():.3g} of max |a|, |b - host| / b <= '
              f'{np.max(np.abs(b - wb) / wb):.3g}')
        assert np.all(np.abs(a - wa) <= BAR[dt] * np.abs(wa).max()) and np.all(np.abs(b - wb) <= BAR[dt] * wb)
    for kw in (dict(), dict(strengths='solve'), dict(over='all')):
        want, want_gains = host.relabel_detections(start, **kw)
        got, gains = nmf.relabel_detections(start, **kw)
        assert isinstance(got, Detections) and gains.dtype == np.float64
        for name in ('sample', 'atom', 'transform', 'shift', 'origin'):
            np.testing.assert_array_equal(getattr(got, name), getattr(want, name))
            np.testing.assert_array_equal(getattr(got, name), getattr(true, name))
        err = np.abs(got.strength.astype(np.float64) - want.strength) / want.strength
        print(f'{dt} {kw}: strengths vs the host route {err.max():.3g}, gains '
              f'{np.max(np.abs(gains - want_gains) / want_gains):.3g}; history {nmf.relabel_history_.tolist()}')
        assert err.max() <= BAR[dt] and np.all(np.abs(gains - want_gains) <= BAR[dt] * want_gains)
        assert nmf.relabel_history_[:, :2].tolist() == host.relabel_history_[:, :2].tolist() == [[20., 20.], [0., 0.]]
        np.testing.assert_allclose(nmf.relabel_history_[:, 2], host.relabel_history_[:, 2], rtol=BAR[dt])
    assert len(set(key(got))) == 20
    assert np.array_equal(nmf.H, before[0]) and np.array_equal(nmf.W, before[1])
    assert torch.equal(nmf._backend._V_dev, before[2])


def test_the_backend_refuses_weights_and_the_front_end_the_rest():
    V = np.random.default_rng(55).random((2, 1, 12, 14)).astype(np.float32) + 0.1

    def refused(nmf, det):
        for call in (lambda: nmf.detection_alternatives(det, 'all'), lambda: nmf.relabel_detections(det, 'all')):
            with pytest.raises(NotImplementedError):
                call()
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend='hip', beta_loss=1.)
    nmf.fit(V, n_iterations=2)
    refused(nmf, nmf.detections(threshold=float(np.quantile(nmf.H, 0.9))))
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend='hip')
    nmf.fit(V, n_iterations=2, weights=np.ones((2, 1, 1, 1), dtype=np.float32))
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)))
    refused(nmf, det)
    with pytest.raises(NotImplementedError):                        # ... nor does the backend take it
        nmf._backend.event_alternatives(None, nmf._W, det.sample, det.atom, det.shift, det.strength, 2, 1)
    np.random.seed(42)
    vol = TransformInvariantNMF(n_atoms=1, atom_shape=(2, 2, 2), backend='hip')
    vol.fit(np.random.default_rng(56).random((1, 1, 5, 5, 5)).astype(np.float32), n_iterations=1)
    refused(vol, vol.detections(threshold=float(np.quantile(vol.H, 0.9))))
