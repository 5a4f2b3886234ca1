"""
The landscape of events on the GPU: tnmf_hip_events_landscape through the C ABI, and ``detection_landscape`` /
``refine_detections`` / ``relocate_detections`` on ``backend='hip'``, against tests/landscape_reference.py evaluated in
extended precision on the SAME V, W, strengths and on the R the device rendered, read back.

The bars are those tests/test_hip_events_gain.py holds tnmf_hip_events_gain to, the sums being of the same kind and length:
per row and neighbour |a - ref| <= 8 * taps * 2^-52 * mag, taps = C * prod(A) and mag = sum |w d_e| the sum of the magnitudes
of the terms of a; b (all its terms are positive: it is its own magnitude) and mag to the same relative bar.  The device adds
at most 4 * taps terms per sum (an occurrence has at most four images) in double, an error of at most 4 * taps * 2^-53 * mag
in any order, with a few roundings per term (V - R, the fma of d_e, the product) on top; the reference rounds once.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import events_reference as eref
import landscape_reference as lref
from test_events_landscape_cpu import GEOMETRIES, holding, key, problem, scene, scene_det
from test_hip_events import BAR, DTYPES, NP, backend, dev, p
from test_hip_events_gain import SENTINEL, events_of, hip_model
from tnmf_amd import _lib
from tnmf_amd.events_host import events_landscape_numpy
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF

pytestmark = pytest.mark.gpu

MODES = ['valid', 'full', 'circular', 'reflect']
N, P = 2, 2
BLOCKS_PER_CU, WAVES = 4, 4        # landscape.hip: TNMF_LANDSCAPE_BLOCKS_PER_CU, kWaves


@functools.lru_cache(maxsize=None)
def rows_of_case(name, mode):
    """-> (rows [K, 2 + k], h, W, V, good): the rows of the CPU test's problem -- every place of landscape_reference.places(),
    duplicates, a zero strength -- with rows outside the contract between them; float32-representable, read-only."""
    V, W, sample, plane, shift, h, names = problem(name, mode)
    D, A, C = GEOMETRIES[name]
    S = eref.shift_shape(D, A, mode)
    k = len(D)
    rows = np.column_stack([sample, plane, shift]).astype(np.int64)
    bad = np.array([[N, 0] + [0] * k, [-1, 0] + [0] * k, [0, P] + [0] * k, [0, -2] + [0] * k,
                    [1, 1] + [S[0]] + [0] * (k - 1), [1, 1] + [0] * (k - 1) + [-1]], dtype=np.int64)
    at = np.array([3, 3, 6, 6, 9, 9])
    rows = np.insert(rows, at, bad, axis=0)
    h = np.insert(h, at, 1.)
    good = np.ones(len(rows), dtype=bool)
    good[at + np.arange(len(at))] = False
    assert not np.any([lref.in_range(N, P, S, r[0], r[1], r[2:]) for r in rows[~good]])
    assert np.all([lref.in_range(N, P, S, r[0], r[1], r[2:]) for r in rows[good]])
    f32 = lambda x: np.asarray(x).astype(np.float32).astype(np.float64)   # noqa: E731
    out = (rows, f32(h), f32(W), f32(V), good)
    for x in out:
        x.setflags(write=False)
    return out


def geo_of(name, mode):
    D, A, C = GEOMETRIES[name]
    return (N, C, P, D, A, mode)


def launch(geo, dt, Wd, ev, hd, Vd, Rd, with_mag=True, fill=float('nan')):
    """-> (code, a, b, mag) of one call on poisoned outputs."""
    n, C, planes, D, A, mode = geo
    be = backend(2, 2, 3, (20, 23), (4, 6), 'circular', 'f32')            # any context: the entry takes its geometry per call
    K, nb = len(ev), 3 ** len(D)
    a = torch.full((K, nb), fill, dtype=torch.float64, device='cuda')
    b = torch.full((K, nb), fill, dtype=torch.float64, device='cuda')
    mag = torch.full((K, nb), fill, dtype=torch.float64, device='cuda') if with_mag else None
    g = _lib.make_geom(n, planes, C, D, A, DTYPES.index(dt))
    code = be._lib.tnmf_hip_events_landscape(be._ctx, ctypes.byref(g), _lib.MODES[mode], p(Wd), p(ev), p(hd), K, p(Vd),
                                             p(Rd), p(a), p(b), p(mag), None)
    torch.cuda.synchronize()
    return code, a.cpu().numpy(), b.cpu().numpy(), None if mag is None else mag.cpu().numpy()


def device_render(geo, dt, rows, h, W):
    """R of the rows inside the contract as the device renders it, on the device."""
    n, C, planes, D, A, mode = geo
    be = backend(n, C, planes, D, A, mode, dt)
    return be.render_events(dev(W, dt), rows[:, 0], rows[:, 1], rows[:, 2:], np.asarray(h, dtype=NP[dt]))


@functools.lru_cache(maxsize=None)
def run(name, mode, dt):
    """-> (a, b, mag, reference a, b, mag) of the case, the reference on the device's own R."""
    rows, h, W, V, good = rows_of_case(name, mode)
    geo = geo_of(name, mode)
    Rd = device_render(geo, dt, rows[good], h[good], W)
    operands = (dev(W, dt), events_of(rows, len(geo[3])), dev(h, dt), dev(V, dt), Rd)
    code, a, b, mag = launch(geo, dt, *operands)
    assert code == 0
    R = Rd.cpu().numpy().astype(np.float64)
    want = lref.landscape(V, R, W, mode, rows[:, 0], rows[:, 1], rows[:, 2:], h)
    return (a, b, mag) + want + (operands,)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(GEOMETRIES))
def test_parity_with_the_reference(name, mode, dt):
    rows, h, W, V, good = rows_of_case(name, mode)
    geo = geo_of(name, mode)
    a, b, mag, ra, rb, rmag, operands = run(name, mode, dt)
    taps = geo[1] * int(np.prod(geo[4]))
    assert not np.isnan(a).any() and not np.isnan(b).any() and not np.isnan(mag).any(), 'every element is written'
    bar = 8 * taps * 2. ** -52
    live = rmag > 0
    worst = [float(np.max(e[live] / s[live])) for e, s in ((np.abs(a - ra), rmag), (np.abs(b - rb), rb),
                                                          (np.abs(mag - rmag), rmag))]
    st = lref.staged(geo, rows[:, 2:]) & good
    print(f'{name} {mode} {dt}: {len(rows)} rows ({int(st.sum())} staged), taps {taps}; |a - ref| / mag <= {worst[0]:.3g}, '
          f'|b - ref| / b <= {worst[1]:.3g}, |mag - ref| / mag <= {worst[2]:.3g}, bar {bar:.3g}')
    assert np.all(np.abs(a - ra) <= bar * rmag) and np.all(np.abs(b - rb) <= bar * rb)
    assert np.all(np.abs(mag - rmag) <= bar * rmag)
    # rows outside the contract and neighbours outside the shift shape: exactly 0
    assert not a[~good].any() and not b[~good].any() and not mag[~good].any() and (~good).sum() == 6
    dead = rb == 0
    assert dead[good].any() and not a[dead].any() and not b[dead].any() and not mag[dead].any()
    # both paths ran (the host mirror of the rule; 5 x 7 in 'reflect' on 12 x 14 has no shift with whole neighbours)
    assert (good & ~st).sum() >= 4
    assert st.any() or (name.startswith('5x7') and mode == 'reflect')
    # the same bits again, and without mag
    code, a2, b2, mag2 = launch(geo, dt, *operands)
    assert code == 0 and a2.tobytes() == a.tobytes() and b2.tobytes() == b.tobytes() and mag2.tobytes() == mag.tobytes()
    code, a3, b3, none = launch(geo, dt, *operands, with_mag=False)
    assert code == 0 and none is None and a3.tobytes() == a.tobytes() and b3.tobytes() == b.tobytes()


def test_the_cases_reach_what_they_are_for():
    """Over the cases: rows of one, two and four images, both paths in every mode, tap counts on both sides of a wave."""
    assert sorted({GEOMETRIES[n][2] * int(np.prod(GEOMETRIES[n][1])) for n in GEOMETRIES}) == [5, 9, 27, 35, 105]
    for mode in MODES:
        for name in GEOMETRIES:
            rows, h, W, V, good = rows_of_case(name, mode)
            D, A, C = GEOMETRIES[name]
            S = eref.shift_shape(D, A, mode)
            n_images = {len(eref.images(r[2:], A, S, mode)) for r in rows[good]}
            assert n_images == ({1} if mode in ('valid', 'full') else {1, 2} if len(D) == 1 else {1, 2, 4})
            assert np.count_nonzero(h[good] == 0) == 1
        assert any((lref.staged(geo_of(n, mode), rows_of_case(n, mode)[0][:, 2:]) & rows_of_case(n, mode)[4]).any()
                   for n in ('1d', '3x3-c1', '5x7-c3'))


# -- the seam between the paths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('mode', ['valid', 'full'])
@pytest.mark.parametrize('name', ['1d', '3x3-c1', '5x7-c3'])
def test_the_seam_between_the_paths(name, mode, dt):
    """An atom one pixel from the border of the sample takes the staged path.  Cut that first row and column of pixels off V
    and R and the same atom over the same pixels sits ON the border: the walk.  The neighbours both problems have -- the
    offsets >= 0 on every axis -- see the same pixels, so they agree within the bars, and bit for bit, since both paths add
    the same terms in the same order."""
    rows, h, W, V, good = rows_of_case(name, mode)
    D, A, C = GEOMETRIES[name]
    k = len(D)
    first = [a - 1 if mode == 'valid' else 0 for a in A]
    row = np.array([[1, 1] + [f + 1 for f in first]], dtype=np.int64)
    geo, cut = (N, C, P, D, A, mode), (N, C, P, tuple(d - 1 for d in D), A, mode)
    cut_row = np.array([[1, 1] + first], dtype=np.int64)
    assert lref.staged(geo, row[:, 2:])[0] and not lref.staged(cut, cut_row[:, 2:])[0]
    rng = np.random.default_rng(5)
    R = (V * (0.5 + rng.random(V.shape))).astype(np.float32).astype(np.float64)   # (need not be anyone's render)
    crop = (slice(None), slice(None)) + (slice(1, None),) * k
    hh = np.array([1.25])
    out = {}
    for which, g, r, v_, r_ in (('staged', geo, row, V, R), ('walk', cut, cut_row, V[crop], R[crop])):
        code, a, b, mag = launch(g, dt, dev(W, dt), events_of(r, k), dev(hh, dt), dev(v_, dt), dev(r_, dt))
        assert code == 0
        ra, rb, rmag = lref.landscape(v_, r_, W, mode, r[:, 0], r[:, 1], r[:, 2:], hh)
        bar = 8 * C * int(np.prod(A)) * 2. ** -52
        assert np.all(np.abs(a - ra) <= bar * rmag) and np.all(np.abs(b - rb) <= bar * rb)
        assert np.all(np.abs(mag - rmag) <= bar * rmag)
        out[which] = (a[0], b[0], mag[0], rmag[0])
    shared = [j for j, delta in enumerate(lref.deltas(k)) if min(delta) >= 0]
    assert len(shared) == 2 ** k
    for x, y in zip(out['staged'][:3], out['walk'][:3]):
        print(f'{name} {mode} {dt}: staged - walk {np.abs(x[shared] - y[shared]).max():.3g}')
        assert np.all(np.abs(x[shared] - y[shared]) <= 2 * bar * out['staged'][3][shared])
        assert x[shared].tobytes() == y[shared].tobytes()
    assert out['staged'][1].all() and np.count_nonzero(out['walk'][1]) == (2 ** k if mode == 'full' else 3 ** k)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('A', [1022, 1023])
def test_the_patch_limit_of_the_staged_path(A, dt):
    """C * (A + 2) = 2048 doubles is the largest patch a wave stages -- 64 KiB of LDS for the four waves of a workgroup; with
    one tap more per channel the patch does not fit and every row of the geometry walks.  Either way the same bars hold."""
    geo = n, C, planes, D, _, mode = (1, 2, 1, (1030,), (A,), 'valid')
    assert (C * (A + 2) <= lref.PATCH_MAX) == (A == 1022) and C * (1022 + 2) == lref.PATCH_MAX
    rows = np.array([[0, 0, A - 1 + 3], [0, 0, A - 1], [0, 0, A - 1 + D[0] - A - 1], [0, 0, 0]], dtype=np.int64)
    assert lref.staged(geo, rows[:, 2:]).tolist() == [A == 1022, False, A == 1022, False]
    rng = np.random.default_rng(A)
    W = (rng.random((planes, C, A)) + 0.1).astype(np.float32).astype(np.float64)
    V = (rng.random((n, C) + D) * 3.).astype(np.float32).astype(np.float64)
    R = (V * (0.5 + rng.random(V.shape))).astype(np.float32).astype(np.float64)
    h = np.array([1.25, 0.5, 2., 1.])
    operands = (dev(W, dt), events_of(rows, 1), dev(h, dt), dev(V, dt), dev(R, dt))
    code, a, b, mag = launch(geo, dt, *operands)
    assert code == 0 and not np.isnan(a).any() and not np.isnan(b).any() and not np.isnan(mag).any()
    ra, rb, rmag = lref.landscape(V, R, W, mode, rows[:, 0], rows[:, 1], rows[:, 2:], h)
    bar = 8 * C * A * 2. ** -52
    live = rmag > 0
    print(f'A = {A} {dt}: |a - ref| / mag <= {np.max(np.abs(a - ra)[live] / rmag[live]):.3g}, |b - ref| / b <= '
          f'{np.max(np.abs(b - rb)[live] / rb[live]):.3g}, bar {bar:.3g}')
    assert np.all(np.abs(a - ra) <= bar * rmag) and np.all(np.abs(b - rb) <= bar * rb)
    assert np.all(np.abs(mag - rmag) <= bar * rmag) and live.sum() == 11 and not a[3, 0] and not b[3, 0]
    code, a2, b2, mag2 = launch(geo, dt, *operands)
    assert code == 0 and a2.tobytes() == a.tobytes() and b2.tobytes() == b.tobytes() and mag2.tobytes() == mag.tobytes()


# -- the identities with the gains ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('mode', MODES)
def test_identities_with_the_gains_on_the_device(mode, dt):
    name = '5x7-c3'
    rows, h, W, V, good = rows_of_case(name, mode)
    n, C, planes, D, A, _ = geo = geo_of(name, mode)
    a, b, mag, _, _, rmag, (Wd, ev, hd, Vd, Rd) = run(name, mode, dt)
    be = backend(2, 2, 3, (20, 23), (4, 6), 'circular', 'f32')
    K = len(rows)
    gain = torch.empty(K, dtype=torch.float64, device='cuda')
    gmag = torch.empty(K, dtype=torch.float64, device='cuda')
    ones = torch.ones_like(hd)
    g = _lib.make_geom(n, planes, C, D, A, DTYPES.index(dt))
    out = []
    for strengths in (hd, ones):
        assert be._lib.tnmf_hip_events_gain(be._ctx, ctypes.byref(g), _lib.MODES[mode], p(Wd), p(ev), p(strengths), K, p(Vd),
                                            p(Rd), p(gain), p(gmag), None) == 0
        torch.cuda.synchronize()
        out.append((gain.cpu().numpy().copy(), gmag.cpu().numpy().copy()))
    (gain_h, mag_h), (gain_1, mag_1) = out
    centre = (a.shape[1] - 1) // 2
    a0, b0 = a[:, centre], b[:, centre]
    hv = np.asarray(h, dtype=np.float64)
    bar = 8 * C * int(np.prod(A)) * 2. ** -52
    # a_e of the gains, read off a call with strengths 1 against the same R: gain = a_e + b / 2
    a_e = gain_1 - 0.5 * b0
    scale = rmag[:, centre] + hv * b0 + mag_1
    print(f'{mode} {dt}: |a_0 - h b_0 - a_e| / scale <= {np.max(np.abs(a0 - hv * b0 - a_e)[good] / scale[good]):.3g}, '
          f'|h a_e + h^2 b_0 / 2 - gain| / scale <= '
          f'{np.max(np.abs(hv * (a0 - hv * b0) + 0.5 * hv * hv * b0 - gain_h)[good] / (hv * scale + mag_h + 1e-300)[good]):.3g}')
    assert np.all(np.abs(a0 - hv * b0 - a_e) <= 4 * bar * scale)
    assert np.all(np.abs(hv * (a0 - hv * b0) + 0.5 * hv * hv * b0 - gain_h) <= 4 * bar * (hv * scale + mag_h))
    assert np.abs(gain_h[good]).max() > 0


# -- the output contract --------------------------------------------------------------------------------------------------------
def test_many_rows_run_the_grid_stride_loop():
    """8 000 rows, duplicates among them, on the 2 x 2 x 12 x 14 problem: more workgroups' worth than the grid has."""
    geo = n, C, planes, D, A, mode = (2, 2, 2, (12, 14), (3, 3), 'reflect')
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
    code, a, b, mag = launch(geo, 'f32', *operands)
    assert code == 0 and not np.isnan(a).any() and not np.isnan(b).any() and not np.isnan(mag).any()
    # the reference per DISTINCT (row, strength): the same row against the same R has the same landscape
    full = np.column_stack([rows.astype(np.float64), h])
    distinct, inverse = np.unique(full, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    d_rows = distinct[:, :-1].astype(np.int64)
    ra, rb, rmag = (x[inverse] for x in lref.landscape(V, R, W, mode, d_rows[:, 0], d_rows[:, 1], d_rows[:, 2:],
                                                       distinct[:, -1]))
    bar = 8 * C * 9 * 2. ** -52
    assert np.all(np.abs(a - ra) <= bar * rmag) and np.all(np.abs(b - rb) <= bar * rb)
    assert np.all(np.abs(mag - rmag) <= bar * rmag)
    st = lref.staged(geo, rows[:, 2:])
    assert st.sum() > 100 and (~st).sum() > 1000
    code, a2, b2, mag2 = launch(geo, 'f32', *operands)
    assert code == 0 and a2.tobytes() == a.tobytes() and b2.tobytes() == b.tobytes() and mag2.tobytes() == mag.tobytes()
    first = np.unique(inverse, return_index=True)[1]
    assert np.array_equal(a, a[first][inverse]) and np.array_equal(b, b[first][inverse])


def test_refused_calls_write_nothing():
    name, mode = '3x3-c3', 'circular'
    rows, h, W, V, good = rows_of_case(name, mode)
    n, C, planes, D, A, _ = geo_of(name, mode)
    be = backend(2, 2, 3, (20, 23), (4, 6), 'circular', 'f32')
    lib, ctx = be._lib, be._ctx
    K = len(rows)
    Wd, hd, Vd, ev = dev(W, 'f32'), dev(h, 'f32'), dev(V, 'f32'), events_of(rows, 2)
    Rd = dev(V * 0.5, 'f32')
    outs = [torch.full((K, 9), SENTINEL, dtype=torch.float64, device='cuda') for _ in range(3)]
    E_NULL, E_DTYPE = -1, -3

    def geom(**kw):
        g = _lib.make_geom(n, planes, C, D, A, 0)
        for key_, val in kw.items():
            setattr(g, key_, val)
        return ctypes.byref(g)

    def call(g, m=_lib.MODES[mode], W_=Wd, ev_=ev, st=hd, k_=K, V_=Vd, R_=Rd, a_=outs[0], b_=outs[1], mg=outs[2], c=ctx):
        return lib.tnmf_hip_events_landscape(c, g, m, p(W_), p(ev_), p(st), k_, p(V_), p(R_), p(a_), p(b_), p(mg), None)

    assert call(geom(), c=None) == E_NULL and call(None) == E_NULL
    for kw in (dict(W_=None), dict(ev_=None), dict(st=None), dict(V_=None), dict(R_=None), dict(a_=None), dict(b_=None)):
        assert call(geom(), **kw) == E_NULL, kw
    assert call(geom(dtype=2)) == E_DTYPE and call(geom(dtype=-1)) == E_DTYPE
    assert call(geom(ndim=3)) == _lib.E_UNSUPPORTED
    assert call(geom(), k_=(2 ** 31 - 1) // 9 + 1) == _lib.E_UNSUPPORTED and call(geom(), k_=2 ** 31) == _lib.E_UNSUPPORTED
    for kw in (dict(ndim=0), dict(ndim=4), dict(N=-1), dict(M=0), dict(C=0)):
        assert call(geom(**kw)) == _lib.E_GEOM, kw
    assert call(geom(), m=4) == _lib.E_GEOM and call(geom(), m=-1) == _lib.E_GEOM and call(geom(), k_=-1) == _lib.E_GEOM
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
    assert not any(bool(torch.any(o == SENTINEL)) for o in outs)


# -- the front end --------------------------------------------------------------------------------------------------------------
def hip_holding(W, V, mode, dt):
    nmf = TransformInvariantNMF(n_atoms=W.shape[0], atom_shape=W.shape[2:], backend='hip', reconstruction_mode=mode)
    nmf._W = dev(W, dt)
    np.random.seed(42)
    nmf.fit(np.array(V, dtype=NP[dt]), n_iterations=0, keep_W=True)
    assert np.array_equal(nmf.W.astype(np.float64), W)
    return nmf


@pytest.mark.parametrize('dt', DTYPES)
def test_refine_and_relocate_return_what_the_numpy_route_returns(dt):
    sc = scene()
    host = holding(sc['W'], sc['V'], sc['mode'])
    nmf = hip_holding(sc['W'], sc['V'], sc['mode'], dt)
    before = (nmf.H.copy(), nmf.W.copy(), nmf._backend._V_dev.clone())
    start, true = scene_det(sc, sc['moved']), scene_det(sc, sc['rows'])
    want, want_gains = host.relocate_detections(start)
    got, gains = nmf.relocate_detections(start)
    assert isinstance(got, Detections) and gains.dtype == np.float64
    for name in ('sample', 'atom', 'transform', 'shift', 'origin'):
        np.testing.assert_array_equal(getattr(got, name), getattr(want, name))
        np.testing.assert_array_equal(getattr(got, name), getattr(true, name))
    err = np.abs(got.strength.astype(np.float64) - want.strength) / want.strength
    print(f'{dt}: strengths vs the host route {err.max():.3g}, gains {np.max(np.abs(gains - want_gains) / want_gains):.3g}; '
          f'history {nmf.relocation_history_.tolist()}')
    assert err.max() <= BAR[dt] and np.all(np.abs(gains - want_gains) <= BAR[dt] * want_gains)
    assert nmf.relocation_history_[:, :2].tolist() == host.relocation_history_[:, :2].tolist() == [[20., 20.], [0., 0.]]
    for det in (true, start):
        off, g0, peak = nmf.refine_detections(det)
        w_off, w_g0, w_peak = host.refine_detections(det)
        print(f'{dt}: offsets vs the host route {np.abs(off - w_off).max():.3g}, peaks {int(peak.sum())} of {len(peak)}')
        assert np.array_equal(peak, w_peak) and np.all(np.abs(off - w_off) <= (1e-6 if dt == 'f32' else 1e-9))
        assert np.all(np.abs(g0 - w_g0) <= BAR[dt] * w_g0.max())
        a, b = nmf.detection_landscape(det)
        assert a.shape == b.shape == (len(det), 3, 3) and a.dtype == b.dtype == np.float64
    assert nmf.refine_detections(true)[2].all() and not nmf.refine_detections(start)[2].all()
    assert np.array_equal(nmf.H, before[0]) and np.array_equal(nmf.W, before[1])
    assert torch.equal(nmf._backend._V_dev, before[2])


def test_with_rot90_the_landscape_is_that_of_the_oriented_atom():
    V = np.random.default_rng(52).random((3, 1, 20, 22)).astype(np.float32)
    nmf = hip_model(V, 2, (4, 4), transforms='rot90')
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.95)), min_distance=1)
    keep = np.sort(np.argsort(-det.strength, kind='stable')[:40])
    det = Detections(*[getattr(det, f)[keep] for f in ('sample', 'atom', 'transform', 'shift', 'origin', 'strength')])
    assert len(set(det.transform.tolist())) > 1
    before = (nmf.H.copy(), nmf.W.copy(), nmf._backend._V_dev.clone())
    W = np.asarray(nmf.transformed_atoms, dtype=np.float64).reshape((-1,) + nmf.W.shape[1:])
    plane = det.atom * 4 + det.transform
    R = nmf.reconstruct_detections(det).astype(np.float64)
    a, b = (x.reshape(len(det), 9) for x in nmf.detection_landscape(det))
    ra, rb, rmag = lref.landscape(V.astype(np.float64), R, W, 'valid', det.sample, plane, det.shift,
                                  det.strength.astype(np.float64))
    bar = 8 * 16 * 2. ** -52
    assert np.all(np.abs(a - ra) <= bar * rmag) and np.all(np.abs(b - rb) <= bar * rb) and rmag.max() > 0
    # the read-outs: the formula on the device's landscape, and the rows of the float64 host route
    off, g0, peak = nmf.refine_detections(det)
    w_off, w_g0, w_peak = lref.refine(a, b, 2)
    assert np.array_equal(off, w_off) and np.array_equal(g0, w_g0) and np.array_equal(peak, w_peak)
    ha, hb = events_landscape_numpy(W, V.shape[2:], 3, 'valid', det.sample, plane, det.shift,
                                    det.strength.astype(np.float64), V.astype(np.float64))
    assert np.all(np.abs(a - ha) <= 1e-5 * np.abs(ha).max()) and np.all(np.abs(b - hb) <= 1e-12 * hb.max())
    moved, gains = nmf.relocate_detections(det, n_iterations=20, max_rounds=3)
    assert len(moved) == len(det) and np.array_equal(moved.atom, det.atom) and np.array_equal(moved.transform, det.transform)
    assert np.abs(moved.shift - det.shift).max() <= 3 and len(set(key(moved))) == len(det)
    E = [0.5 * float(np.sum((V - nmf.reconstruct_detections(d)) ** 2))
         for d in (nmf.refit_detections(det, 20), moved)]
    print(f'rot90: {int(np.any(moved.shift != det.shift, axis=1).sum())} of {len(det)} rows moved, objective {E[0]:.6g} -> '
          f'{E[1]:.6g}; history {nmf.relocation_history_.tolist()}')
    assert E[1] <= E[0] * (1 + 1e-6)
    assert np.array_equal(nmf.H, before[0]) and np.array_equal(nmf.W, before[1])
    assert torch.equal(nmf._backend._V_dev, before[2])


def test_the_backend_refuses_weights_and_the_front_end_the_rest():
    V = np.random.default_rng(55).random((2, 1, 12, 14)).astype(np.float32) + 0.1

    def refused(nmf, det):
        for call in (nmf.detection_landscape, nmf.refine_detections, nmf.relocate_detections):
            with pytest.raises(NotImplementedError):
                call(det)
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
        nmf._backend.event_landscape(None, nmf._W, det.sample, det.atom, det.shift, det.strength)
    np.random.seed(42)
    vol = TransformInvariantNMF(n_atoms=1, atom_shape=(2, 2, 2), backend='hip')
    vol.fit(np.random.default_rng(56).random((1, 1, 5, 5, 5)).astype(np.float32), n_iterations=1)
    refused(vol, vol.detections(threshold=float(np.quantile(vol.H, 0.9))))
