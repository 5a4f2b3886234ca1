"""
Events on the GPU: tnmf_hip_events_render / tnmf_hip_events_update through HIP_Backend and the C ABI, and
``reconstruct_detections`` / ``refit_detections`` on ``backend='hip'``, against the naive float64 reference
tests/events_reference.py and against the dense kernels on the scattered H.

Renders of integer-valued inputs (W in 0..3, strengths 1..4, every sum far below 2^24) are compared EXACTLY in both element
types.  Float-valued renders are held to the project's bars relative to max R (1e-10 float64, 1e-5 float32), refitted
strengths to the same bars per strength.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch

import events_reference as eref
from tnmf_amd import _lib
from tnmf_amd.backends.HIP import HIP_Backend
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF

pytestmark = pytest.mark.gpu

NP = {'f32': np.float32, 'f64': np.float64}
BAR = {'f32': 1e-5, 'f64': 1e-10}
DTYPES = ['f32', 'f64']


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def backend(N, C, P, D, A, mode, dt):
    """An initialised backend of this geometry whose resident samples the tests overwrite (be._V_dev)."""
    np.random.seed(0)
    be = HIP_Backend(reconstruction_mode=mode)
    be.initialize(np.ones((N, C) + D, dtype=NP[dt]), A, P, None, tuple(range(-len(A), 0)))
    return be


def dev(x, dt):
    return torch.from_numpy(np.array(x, dtype=NP[dt])).cuda()   # (a copy: the cases are read-only)


# -- the cases: (N, C, P, D, A, mode) and their events, built once ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """-> (geometry, sample, plane, shift, integer strengths, integer W), read-only."""
    rng = np.random.default_rng(11)
    if name == '2d-valid':
        N, C, P, D, A, mode = 3, 2, 4, (37, 150), (5, 7), 'valid'
    elif name == '1d':
        N, C, P, D, A, mode = 2, 1, 3, (300,), (9,), 'valid'
    elif name == 'full-atom-as-large-as-the-sample':
        N, C, P, D, A, mode = 2, 2, 3, (8, 9), (8, 9), 'full'
    else:
        N, C, P, D, A, mode = 2, 2, 3, (20, 23), (4, 6), name
    S = eref.shift_shape(D, A, mode)
    k = len(D)
    rows = set()
    samples = [0, 2] if name == '2d-valid' else list(range(N))     # 2d-valid: sample 1 has NO events
    for n in samples[:1]:                                            # the corners of the shift range
        for corner in np.ndindex(*(2,) * k):
            rows.add((n, 1) + tuple(c * (s - 1) for c, s in zip(corner, S)))
    if mode == 'circular':                                           # the wrap zone of both axes, one axis, its edge
        rows |= {(0, 2) + tuple(s - 1 for s in S), (1, 0) + tuple(s - (a - 1) for s, a in zip(S, A)),
                 (1, 1, S[0] - 2, 3), (1, 1, 5, S[1] - 1), (0, 0) + tuple(s - a for s, a in zip(S, A))}
    if mode == 'reflect':                                            # the mirror zone of both axes, one axis, its edges
        rows |= {(0, 2, 1, 1), (1, 0) + tuple(a - 1 for a in A), (1, 1, 2, 12), (1, 1, 9, 3), (0, 0) + tuple(A),
                 (0, 0, 0, 2)}
    if name == '2d-valid':
        # 70 events whose footprints all cover pixel (20, 100) of sample 0: more than a wave's worth on one tile
        spots = [(pl, 20 + jy, 100 + jx) for pl in range(P) for jy in range(A[0]) for jx in range(A[1])]
        for i in rng.choice(len(spots), 70, replace=False):
            rows.add((0,) + spots[i])
    target = {'2d-valid': 200 + len(rows), '1d': 60}.get(name, min(40, N * P * int(np.prod(S))))
    while len(rows) < target:
        rows.add((int(rng.choice(samples)), int(rng.integers(P))) + tuple(int(rng.integers(s)) for s in S))
    rows = np.array(sorted(rows), dtype=np.int64)
    rows = rows[rng.permutation(len(rows))]                          # given in shuffled order
    out = ((N, C, P, D, A, mode), rows[:, 0], rows[:, 1], rows[:, 2:], rng.integers(1, 5, len(rows)).astype(np.float64),
           rng.integers(0, 4, (P, C) + A).astype(np.float64))
    for a in out[1:]:
        a.setflags(write=False)
    return out


CASES = ['2d-valid', '1d', 'full-atom-as-large-as-the-sample', 'valid', 'full', 'circular', 'reflect']


@functools.lru_cache(maxsize=None)
def integer_render(name):
    (N, C, P, D, A, mode), sample, plane, shift, h, W = case(name)
    R = eref.render(W, D, N, mode, sample, plane, shift, h)
    assert R.max() < 2 ** 20 and R.any()
    R.setflags(write=False)
    return R


# -- render -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', CASES)
def test_render_of_integers_is_exact(name, dt):
    geo, sample, plane, shift, h, W = case(name)
    be = backend(*geo, dt)
    want = integer_render(name)
    R = be.render_events(dev(W, dt), sample, plane, shift, h)
    assert R.dtype == be._torch_dtype and tuple(R.shape) == want.shape
    assert np.array_equal(R.cpu().numpy().astype(np.float64), want)
    if name == '2d-valid':
        assert not want[1].any() and want[0, :, 20, 100].min() >= 1
    # over a poisoned buffer: every pixel is written, zeros included; and the same bits again
    s, pl, sh, hh = be._check_events(W.shape[0], sample, plane, shift, h)
    images, cell_start, _ = be.event_list(s, pl, sh)
    if name in ('circular', 'reflect'):
        assert images.shape[0] > len(sample)                        # some events stand for several images
    poisoned = torch.full_like(R, float('nan'))
    be.render_event_list(dev(W, dt), images, cell_start, hh, poisoned)
    assert torch.equal(poisoned, R)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', ['2d-valid', 'circular'])
def test_duplicates_add_up_and_no_events_give_zeros(name, dt):
    geo, sample, plane, shift, h, W = case(name)
    be = backend(*geo, dt)
    twice = [np.concatenate([x, x[:30]]) for x in (sample, plane, shift, h)]
    want = integer_render(name) + eref.render(W, geo[3], geo[0], geo[5], sample[:30], plane[:30], shift[:30], h[:30])
    assert np.array_equal(be.render_events(dev(W, dt), *twice).cpu().numpy().astype(np.float64), want)
    none = be.render_events(dev(W, dt), sample[:0], plane[:0], shift[:0], h[:0])
    assert tuple(none.shape) == want.shape and not bool(none.any())
    be._V_dev.fill_(1.)
    assert be.refit_events(None, dev(W, dt), sample[:0], plane[:0], shift[:0], h[:0], 3).shape == (0,)


# -- float-valued problems: render against the dense reconstruct, refit against the reference and the dense half step ----------
@functools.lru_cache(maxsize=None)
def float_problem(name):
    """W, the starting strengths and V = the render of 'true' strengths + 0.1 (positive, well conditioned), in float64 of
    float32-representable values, so that both element types work on the same numbers."""
    geo, sample, plane, shift, _, _ = case(name)
    N, C, P, D, A, mode = geo
    rng = np.random.default_rng(12)
    W = (rng.random((P, C) + A) + 0.1).astype(np.float32).astype(np.float64)
    true = (rng.random(len(sample)) + 0.5).astype(np.float32).astype(np.float64)
    start = (rng.random(len(sample)) + 0.5).astype(np.float32).astype(np.float64)
    start[1] = 0.   # stays 0
    V = (eref.render(W, D, N, mode, sample, plane, shift, true) + 0.1).astype(np.float32).astype(np.float64)
    for a in (W, start, V):
        a.setflags(write=False)
    return W, start, V


@functools.lru_cache(maxsize=None)
def reference_refit(name, sparsity):
    geo, sample, plane, shift, _, _ = case(name)
    W, start, V = float_problem(name)
    out = eref.refit(V, W, geo[5], sample, plane, shift, start, 3, sparsity, 1e-9)
    out.setflags(write=False)
    return out


FLOAT_CASES = ['2d-valid', '1d', 'full', 'circular', 'reflect']


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', FLOAT_CASES)
def test_render_agrees_with_the_dense_reconstruct(name, dt):
    geo, sample, plane, shift, _, _ = case(name)
    N, C, P, D, A, mode = geo
    be = backend(*geo, dt)
    W, start, _ = float_problem(name)
    R = be.render_events(dev(W, dt), sample, plane, shift, start).cpu().numpy().astype(np.float64)
    H = eref.scatter(N, P, eref.shift_shape(D, A, mode), sample, plane, shift, start)
    dense = be.reconstruct(dev(W, dt), dev(H, dt)).cpu().numpy().astype(np.float64)
    want = eref.render(W, D, N, mode, sample, plane, shift, start)
    err_ref, err_dense = np.abs(R - want).max() / want.max(), np.abs(R - dense).max() / want.max()
    print(f'{name} {dt}: render vs reference {err_ref:.3g}, vs dense reconstruct {err_dense:.3g} (of max R)')
    assert err_ref <= BAR[dt] and err_dense <= BAR[dt]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('sparsity', [0., 0.2])
@pytest.mark.parametrize('name', FLOAT_CASES)
def test_three_refit_steps(name, sparsity, dt):
    geo, sample, plane, shift, _, _ = case(name)
    N, C, P, D, A, mode = geo
    be = backend(*geo, dt)
    W, start, V = float_problem(name)
    be._V_dev.copy_(dev(V, dt))
    Wd = dev(W, dt)
    got_t = be.refit_events(None, Wd, sample, plane, shift, start, 3, sparsity=sparsity, eps=1e-9)
    again = be.refit_events(None, Wd, sample, plane, shift, start, 3, sparsity=sparsity, eps=1e-9)
    assert torch.equal(got_t, again), 'a refit is deterministic'
    got = got_t.cpu().numpy().astype(np.float64)
    want = reference_refit(name, sparsity)
    assert got[1] == 0. and want[1] == 0.
    live = want > 0
    err = np.abs(got[live] - want[live]) / want[live]
    # three dense H half steps on the scattered H, read at the support
    H = dev(eref.scatter(N, P, eref.shift_shape(D, A, mode), sample, plane, shift, start), dt)
    for _ in range(3):
        be.fused_update_H(None, Wd, H, sparsity=sparsity, eps=1e-9)
    dense = H.cpu().numpy().astype(np.float64)[(sample, plane) + tuple(shift.T)]
    err_dense = np.abs(got[live] - dense[live]) / want[live]
    print(f'{name} {dt} sparsity {sparsity}: 3 refit steps vs reference {err.max():.3g}, vs dense {err_dense.max():.3g} '
          f'(per strength, relative)')
    assert err.max() <= BAR[dt]
    assert err_dense.max() <= BAR[dt]
    assert np.count_nonzero(H.cpu().numpy()) == int(live.sum())


# -- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    geo, sample, plane, shift, h, W = case('circular')
    N, C, P, D, A, mode = geo
    be = backend(*geo, 'f32')
    lib, ctx = be._lib, be._ctx
    s, pl, sh, hh = be._check_events(P, sample, plane, shift, h)
    images, cell_start, events = be.event_list(s, pl, sh)
    Wd = dev(W, 'f32')
    R = torch.full((N, C) + D, -7., dtype=torch.float32, device='cuda')
    V = torch.ones_like(R)
    hh = hh.clone()
    before = hh.clone()
    I, K = images.shape[0], len(sample)
    E_NULL, E_DTYPE = -1, -3

    def geom(**kw):
        g = _lib.make_geom(N, P, C, D, A, 0)
        for key, val in kw.items():
            setattr(g, key, val)
        return ctypes.byref(g)

    def render(g, W_=Wd, img=images, n_img=I, cs=cell_start, st=hh, k_=K, R_=R, c=ctx):
        return lib.tnmf_hip_events_render(c, g, p(W_), p(img), n_img, p(cs), p(st), k_, p(R_), None)

    def update(g, m=_lib.MODES[mode], W_=Wd, ev=events, st=hh, k_=K, V_=V, R_=R, eps=1e-9, sp=0., c=ctx):
        return lib.tnmf_hip_events_update(c, g, m, p(W_), p(ev), p(st), k_, p(V_), p(R_), eps, sp, None)

    assert render(geom(), c=None) == E_NULL and render(None) == E_NULL
    for kw in (dict(W_=None), dict(cs=None), dict(R_=None), dict(img=None), dict(st=None)):
        assert render(geom(), **kw) == E_NULL, kw
    assert render(geom(dtype=2)) == E_DTYPE and update(geom(dtype=-1)) == E_DTYPE
    assert render(geom(ndim=3)) == _lib.E_UNSUPPORTED and update(geom(ndim=3)) == _lib.E_UNSUPPORTED
    for kw in (dict(ndim=0), dict(ndim=4), dict(N=-1), dict(M=0), dict(C=0)):
        assert render(geom(**kw)) == _lib.E_GEOM and update(geom(**kw)) == _lib.E_GEOM, kw
    assert render(geom(), n_img=-1) == _lib.E_GEOM and render(geom(), k_=-1) == _lib.E_GEOM
    assert render(geom(), n_img=2 ** 31) == _lib.E_UNSUPPORTED
    assert update(geom(), c=None) == E_NULL and update(None) == E_NULL
    for kw in (dict(W_=None), dict(ev=None), dict(st=None), dict(V_=None), dict(R_=None)):
        assert update(geom(), **kw) == E_NULL, kw
    assert update(geom(), m=4) == _lib.E_GEOM and update(geom(), m=-1) == _lib.E_GEOM and update(geom(), k_=-1) == _lib.E_GEOM
    assert update(geom(), eps=-1.) == _lib.E_UNSUPPORTED and update(geom(), sp=float('nan')) == _lib.E_UNSUPPORTED
    g = _lib.make_geom(N, P, C, (4, 23), (6, 6), 0)                 # circular: more than one wrap
    assert update(ctypes.byref(g)) == _lib.E_GEOM
    g = _lib.make_geom(N, P, C, (3, 23), (4, 6), 0)                 # reflect: a mirror without the edge
    assert update(ctypes.byref(g), m=_lib.MODES['reflect']) == _lib.E_GEOM
    g = _lib.make_geom(N, P, C, (3, 23), (4, 6), 0)                 # full: no shift at all
    assert update(ctypes.byref(g), m=_lib.MODES['full']) == _lib.E_GEOM
    torch.cuda.synchronize()
    assert bool(torch.all(R == -7.)) and torch.equal(hh, before)
    # rows outside the contract are skipped, not followed: a wild plane and event, offsets beyond the list
    wild = images.clone()
    wild[0, 0], wild[1, 3], wild[2, 0] = P, K, -1
    loose = cell_start.clone()
    loose[-1] = I + 1000
    assert render(geom(), img=wild, cs=loose) == 0
    keep = np.ones(I, dtype=bool)
    keep[:3] = False
    im = images.cpu().numpy()[keep]
    want = np.zeros((N, C) + D)
    for plane_, qy, qx, e in im:                                    # what the remaining rows place, from the rows themselves
        for c in range(C):
            for jy in range(A[0]):
                for jx in range(A[1]):
                    y, x = qy - (A[0] - 1) + jy, qx - (A[1] - 1) + jx
                    if 0 <= y < D[0] and 0 <= x < D[1]:
                        want[sample[e], c, y, x] += h[e] * W[plane_, c, jy, jx]
    assert np.array_equal(R.cpu().numpy().astype(np.float64), want)
    ev = events.clone()
    ev[0, 0], ev[1, 1], ev[2, 2], ev[3, 3] = N, -1, D[0], -5
    assert update(geom(), ev=ev) == 0
    torch.cuda.synchronize()
    assert torch.equal(hh[:4], before[:4]) and not torch.equal(hh[4:], before[4:])


def test_the_backend_refuses_bad_events():
    geo, sample, plane, shift, h, W = case('reflect')
    N, C, P, D, A, mode = geo
    be = backend(*geo, 'f64')
    Wd = dev(W, 'f64')

    def changed(col, value):
        cols = [np.array(x) for x in (sample, plane, shift, h)]
        cols[col][2] = value
        return cols
    for col, value in ((0, N), (0, -1), (1, P), (1, -1), (2, (D[0], 0)), (2, (0, -1)), (3, -1.), (3, np.nan), (3, np.inf)):
        with pytest.raises(ValueError):
            be.render_events(Wd, *changed(col, value))
        with pytest.raises(ValueError):
            be.refit_events(None, Wd, *changed(col, value), 1)
    with pytest.raises(ValueError):
        be.render_events(Wd, sample.astype(np.float64), plane, shift, h)


# -- end to end -----------------------------------------------------------------------------------------------------------------
def hip_model(V, n_atoms, atom_shape, **kw):
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=n_atoms, atom_shape=atom_shape, backend='hip', **kw)
    nmf.fit(V, n_iterations=5, sparsity_H=0.1)
    return nmf


def check_model(nmf, dt):
    be = nmf._backend
    assert be.supports_events
    mode = be._reconstruction_mode
    W = nmf.transformed_atoms.reshape((-1,) + nmf.W.shape[1:]).astype(np.float64)
    V = np.asarray(nmf.V, dtype=np.float64)
    D, T = V.shape[2:], nmf.n_transforms
    # every positive entry of H: the list reconstructs what H reconstructs
    everything = nmf.detections(threshold=0., min_distance=0)
    R_all, R = nmf.reconstruct_detections(everything), nmf.R
    assert R_all.shape == R.shape and R_all.dtype == R.dtype
    err = np.abs(R_all.astype(np.float64) - R).max() / R.max()
    print(f'{mode} {dt}: reconstruct_detections(all {len(everything)}) vs R {err:.3g} of max R')
    assert err <= BAR[dt]
    # the strongest few: render and refit against the reference
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.95)), min_distance=1)
    assert 10 < len(det) < 1000
    plane = det.atom * T + det.transform
    want = eref.render(W, D, len(V), mode, det.sample, plane, det.shift, det.strength.astype(np.float64))
    got = nmf.reconstruct_detections(det)
    err = np.abs(got - want).max() / want.max()
    print(f'{mode} {dt}: reconstruct_detections({len(det)}) vs reference {err:.3g} of max R')
    assert err <= BAR[dt]
    refit = nmf.refit_detections(det, 3, sparsity_H=0.05)
    assert isinstance(refit, Detections) and refit.strength.dtype == det.strength.dtype
    for name in ('sample', 'atom', 'transform', 'shift', 'origin'):
        np.testing.assert_array_equal(getattr(refit, name), getattr(det, name))
    ref = eref.refit(V, W, mode, det.sample, plane, det.shift, det.strength.astype(np.float64), 3, 0.05, nmf.eps)
    err = np.abs(refit.strength - ref) / ref
    print(f'{mode} {dt}: refit_detections 3 steps vs reference {err.max():.3g} per strength')
    assert err.max() <= BAR[dt]
    # a refit against V explains V at least as well as the strengths it started from (MU does not increase the objective)
    def loss(d):
        return 0.5 * np.sum((V - nmf.reconstruct_detections(d).astype(np.float64)) ** 2)
    assert loss(nmf.refit_detections(det, 10)) <= loss(det) * (1 + 1e-6)
    assert np.array_equal(nmf.reconstruct_detections(refit), nmf.reconstruct_detections(
        dataclasses.replace(det, strength=refit.strength)))


@pytest.mark.parametrize('mode', ['valid', 'circular'])
@pytest.mark.parametrize('which', ['2d-f32', '1d-f64'])
def test_fit_detect_refit_reconstruct(which, mode):
    rng = np.random.default_rng(21)
    if which == '2d-f32':
        V, M, A = rng.random((3, 2, 24, 30)).astype(np.float32), 4, (5, 6)
    else:
        V, M, A = rng.random((4, 1, 120)), 3, (9,)
    check_model(hip_model(V, M, A, reconstruction_mode=mode), which[-3:])


def test_fit_with_rot90_detect_refit_reconstruct():
    V = np.random.default_rng(22).random((3, 1, 20, 22)).astype(np.float32)
    nmf = hip_model(V, 2, (4, 4), transforms='rot90')
    assert nmf.H.shape == (3, 2, 4, 23, 25)
    check_model(nmf, 'f32')


def test_volumes_beta_and_weights_are_refused():
    V = np.random.default_rng(23).random((2, 1, 12, 14)).astype(np.float32) + 0.1
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend='hip', beta_loss=1.)
    nmf.fit(V, n_iterations=2)
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)))
    with pytest.raises(NotImplementedError):
        nmf.refit_detections(det, 1)
    assert nmf.reconstruct_detections(det).shape == V.shape        # a render does not depend on the objective
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend='hip')
    nmf.fit(V, n_iterations=2, weights=np.ones((2, 1, 1, 1), dtype=np.float32))
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)))
    with pytest.raises(NotImplementedError):
        nmf.refit_detections(det, 1)
    with pytest.raises(NotImplementedError):                        # ... nor does the backend take it
        nmf._backend.refit_events(None, nmf._W, det.sample, det.atom, det.shift, det.strength, 1)
    assert nmf.reconstruct_detections(det).shape == V.shape
    np.random.seed(42)
    vol = TransformInvariantNMF(n_atoms=1, atom_shape=(2, 2, 2), backend='hip')
    vol.fit(np.random.default_rng(24).random((1, 1, 5, 5, 5)).astype(np.float32), n_iterations=1)
    det = vol.detections(threshold=float(np.quantile(vol.H, 0.9)))
    for call in (vol.reconstruct_detections, vol.refit_detections):
        with pytest.raises(NotImplementedError):
            call(det)
