"""
Gains of events on the GPU: tnmf_hip_events_gain through the C ABI, and ``detection_gains`` / ``prune_detections`` on
``backend='hip'``, against the closed form of tests/events_gain_reference.py evaluated in float64 on the SAME V, W, strengths
and R -- R is copied to both sides (or read back from the device), so only the order of the additions differs.

The bar per row: |gain - ref| <= 8 * taps * 2^-52 * mag, taps = C * prod(A) and mag the sum of the magnitudes of the terms of
the gain.  Either side adds at most 4 * taps terms per sum (an event has at most four images) in double, an error of at most
4 * taps * 2^-53 * mag each in any order, with a few roundings per term (the difference V - R, the products, phi) on top: the
bar is twice the two together.  mag is held to the same relative bar.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import events_gain_reference as gref
import events_reference as eref
from test_events_gain_cpu import MIN_GAIN, key, planted_model, rows_of
from test_hip_events import BAR, DTYPES, NP, backend, dev, p
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF, event_images

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


def context():
    """Any initialised backend: the entry takes its geometry per call."""
    be = backend(2, 2, 3, (20, 23), (4, 6), 'circular', 'f32')
    return be._lib, be._ctx, be


# -- the cases: (N, C, P, D, A, mode) and their rows, built once --------------------------------------------------------------
GEOMETRIES = {
    'taps-9': (3, 1, 4, (12, 14), (3, 3), 'reflect'),             # fewer taps than lanes
    'taps-75': (3, 3, 4, (12, 14), (5, 5), 'circular'),           # more than a wave's worth, not a multiple of it
    'taps-320': (3, 5, 4, (12, 14), (8, 8), 'valid'),             # more than 256
    '1d-7': (3, 2, 4, (40,), (7,), 'reflect'),
    '1d-300': (3, 1, 4, (320,), (300,), 'circular'),
    'valid': (3, 2, 4, (12, 14), (4, 4), 'valid'),
    'full': (3, 2, 4, (12, 14), (4, 4), 'full'),
    'circular': (3, 2, 4, (12, 14), (4, 4), 'circular'),
    'reflect': (3, 2, 4, (12, 14), (4, 4), 'reflect'),
    'grid-stride': (2, 1, 3, (50,), (2,), 'circular'),            # 70 000 rows: beyond num_cu * 64 blocks of 4 waves
}
MODE_CASES = ['valid', 'full', 'circular', 'reflect']


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (geometry, rows [K, 2 + k] with the rows outside the contract in place, strengths, W, V, R, reference gain, mag):
    float64 arrays of float32-representable values, read-only.  R is the render of the rows plus a perturbation: what the
    entry is given need not be anyone's render."""
    geo = N, C, P, D, A, mode = GEOMETRIES[name]
    S = eref.shift_shape(D, A, mode)
    k = len(D)
    rng = np.random.default_rng(41)

    def random_rows(count):
        return np.column_stack([rng.integers(N, size=count), rng.integers(P, size=count)]
                               + [rng.integers(s, size=count) for s in S]).astype(np.int64)
    if name == 'grid-stride':
        rows = random_rows(70000)
        h = rng.integers(0, 4, len(rows)) / 4.
    else:
        rows = random_rows(40)
        if name in MODE_CASES:   # every shift of one plane of one sample: every zone of both axes
            every = np.array([(1, 2) + u for u in np.ndindex(*S)], dtype=np.int64)
            rows = np.concatenate([every, rows])
        rows = np.concatenate([rows, rows[:5]])                     # duplicates
        h = (rng.random(len(rows)) + 0.5).astype(np.float32).astype(np.float64)
        h[-5:] = h[:5]
        h[[7, len(h) - 7]] = 0.
        if name in MODE_CASES:   # rows outside the contract, between good ones
            rows[10, 0], rows[20, 0], rows[30, 1], rows[31, 1] = N, -1, P, -2
            rows[40, 2], rows[50, 3], rows[51, 2] = S[0], S[1], -5
    order = rng.permutation(len(rows))                              # given in shuffled order
    rows, h = rows[order], h[order]
    W = (rng.random((P, C) + A) + 0.1).astype(np.float32).astype(np.float64)
    V = (rng.random((N, C) + D) * 3.).astype(np.float32).astype(np.float64)
    good = ((rows[:, 0] >= 0) & (rows[:, 0] < N) & (rows[:, 1] >= 0) & (rows[:, 1] < P)
            & np.all((rows[:, 2:] >= 0) & (rows[:, 2:] < np.array(S)), axis=1))
    if name == 'grid-stride':      # (the render of 70 000 rows: that of the distinct places with their strengths added up)
        places, inverse = np.unique(rows, axis=0, return_inverse=True)
        total = np.bincount(inverse.reshape(-1), weights=h, minlength=len(places))
        R = eref.render(W, D, N, mode, places[:, 0], places[:, 1], places[:, 2:], total)
    else:
        R = eref.render(W, D, N, mode, rows[good, 0], rows[good, 1], rows[good, 2:], h[good])
    R = (R * (1. + 0.1 * rng.random(R.shape))).astype(np.float32).astype(np.float64)
    # the reference per DISTINCT (row, strength): the same row against the same R has the same gain
    full = np.column_stack([rows.astype(np.float64), h])
    distinct, inverse = np.unique(full, axis=0, return_inverse=True)
    d_rows = distinct[:, :-1].astype(np.int64)
    gain, mag = gref.closed_form(V, R, W, mode, d_rows[:, 0], d_rows[:, 1], d_rows[:, 2:], distinct[:, -1])
    gain, mag = gain[inverse.reshape(-1)], mag[inverse.reshape(-1)]
    out = (geo, rows, h, W, V, R, gain, mag, good)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def events_of(rows, k):
    """[K, 4] int32 on the device: (n, p, u_0, u_1), one shift axis as (n, p, 0, u_0)."""
    ev = np.zeros((len(rows), 4), dtype=np.int32)
    ev[:, :2] = rows[:, :2]
    ev[:, 4 - k:] = rows[:, 2:]
    return torch.from_numpy(ev).cuda()


def call(name, dt, with_mag=True):
    """-> (code, gain, mag) of one call on poisoned outputs."""
    geo, rows, h, W, V, R, _, _, _ = case(name)
    N, C, P, D, A, mode = geo
    lib, ctx, _ = context()
    K = len(rows)
    gain = torch.full((K,), float('nan'), dtype=torch.float64, device='cuda')
    mag = torch.full((K,), float('nan'), dtype=torch.float64, device='cuda') if with_mag else None
    g = _lib.make_geom(N, P, C, D, A, DTYPES.index(dt))
    Wd, hd, Vd, Rd, ev = dev(W, dt), dev(h, dt), dev(V, dt), dev(R, dt), events_of(rows, len(D))
    code = lib.tnmf_hip_events_gain(ctx, ctypes.byref(g), _lib.MODES[mode], p(Wd), p(ev), p(hd), K, p(Vd), p(Rd), p(gain),
                                    p(mag), None)
    torch.cuda.synchronize()
    return code, gain.cpu().numpy(), None if mag is None else mag.cpu().numpy()


def test_the_cases_reach_what_they_are_for():
    for name in MODE_CASES:
        geo, rows, h, _, _, _, gain, mag, good = case(name)
        N, C, P, D, A, mode = geo
        S = eref.shift_shape(D, A, mode)
        n_images = np.bincount(event_images(rows[good, 2:], A, S, mode)[0], minlength=int(good.sum()))
        assert set(n_images.tolist()) == ({1, 2, 4} if mode in ('circular', 'reflect') else {1})
        assert (~good).sum() == 7 and not gain[~good].any() and not mag[~good].any()
        assert np.count_nonzero(h == 0) == 2 and np.count_nonzero(gain[good]) == good.sum() - 2
    assert [int(np.prod(GEOMETRIES[n][4])) * GEOMETRIES[n][1] for n in ('taps-9', 'taps-75', 'taps-320')] == [9, 75, 320]
    # more rows than one pass of the largest grid takes: num_cu * 64 blocks of 4 waves
    assert len(case('grid-stride')[1]) == 70000 > torch.cuda.get_device_properties(0).multi_processor_count * 64 * 4


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', list(GEOMETRIES))
def test_gain_and_magnitude_against_the_closed_form(name, dt):
    geo, rows, h, W, V, R, want, want_mag, good = case(name)
    taps = geo[1] * int(np.prod(geo[4]))
    code, gain, mag = call(name, dt)
    assert code == 0
    assert not np.isnan(gain).any() and not np.isnan(mag).any(), 'every element is written'
    bar = 8 * taps * 2. ** -52
    err = np.abs(gain - want)
    live = want_mag > 0
    print(f'{name} {dt}: {len(rows)} rows, taps {taps}; |gain - ref| / mag <= {np.max(err[live] / want_mag[live]):.3g}, '
          f'|mag - ref| / mag <= {np.max(np.abs(mag - want_mag)[live] / want_mag[live]):.3g}, bar {bar:.3g}')
    assert np.all(err <= bar * want_mag)
    assert np.all(np.abs(mag - want_mag) <= bar * want_mag)
    assert not gain[~live].any() and not mag[~live].any()          # h = 0 and the rows outside the contract: exactly 0
    assert np.all(mag * (1 + 1e-12) >= np.abs(gain))
    # the same bits again, and without mag
    code2, gain2, mag2 = call(name, dt)
    assert code2 == 0 and gain2.tobytes() == gain.tobytes() and mag2.tobytes() == mag.tobytes()
    code3, gain3, _ = call(name, dt, with_mag=False)
    assert code3 == 0 and gain3.tobytes() == gain.tobytes()


def test_duplicate_rows_have_the_same_gain():
    _, rows, h, _, _, _, _, _, _ = case('circular')
    _, gain, _ = call('circular', 'f64')
    full = np.column_stack([rows.astype(np.float64), h])
    _, first, inverse, counts = np.unique(full, axis=0, return_index=True, return_inverse=True, return_counts=True)
    assert counts.max() >= 2
    assert np.array_equal(gain, gain[first][inverse.reshape(-1)])


# -- refusals -----------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    geo, rows, h, W, V, R, _, _, _ = case('circular')
    N, C, P, D, A, mode = geo
    lib, ctx, _ = context()
    K = len(rows)
    Wd, hd, Vd, Rd, ev = dev(W, 'f32'), dev(h, 'f32'), dev(V, 'f32'), dev(R, 'f32'), events_of(rows, 2)
    gain = torch.full((K,), SENTINEL, dtype=torch.float64, device='cuda')
    mag = torch.full((K,), SENTINEL, dtype=torch.float64, device='cuda')
    E_NULL, E_DTYPE = -1, -3

    def geom(**kw):
        g = _lib.make_geom(N, P, C, D, A, 0)
        for name, val in kw.items():
            setattr(g, name, val)
        return ctypes.byref(g)

    def gains(g, m=_lib.MODES[mode], W_=Wd, ev_=ev, st=hd, k_=K, V_=Vd, R_=Rd, out=gain, mg=mag, c=ctx):
        return lib.tnmf_hip_events_gain(c, g, m, p(W_), p(ev_), p(st), k_, p(V_), p(R_), p(out), p(mg), None)

    assert gains(geom(), c=None) == E_NULL and gains(None) == E_NULL
    for kw in (dict(W_=None), dict(ev_=None), dict(st=None), dict(V_=None), dict(R_=None), dict(out=None)):
        assert gains(geom(), **kw) == E_NULL, kw
    assert gains(geom(dtype=2)) == E_DTYPE and gains(geom(dtype=-1)) == E_DTYPE
    assert gains(geom(ndim=3)) == _lib.E_UNSUPPORTED
    assert gains(geom(), k_=2 ** 31) == _lib.E_UNSUPPORTED
    for kw in (dict(ndim=0), dict(ndim=4), dict(N=-1), dict(M=0), dict(C=0)):
        assert gains(geom(**kw)) == _lib.E_GEOM, kw
    assert gains(geom(), m=4) == _lib.E_GEOM and gains(geom(), m=-1) == _lib.E_GEOM and gains(geom(), k_=-1) == _lib.E_GEOM
    g = _lib.make_geom(N, P, C, (2, 14), (4, 4), 0)                 # circular: more than one wrap
    assert gains(ctypes.byref(g)) == _lib.E_GEOM
    g = _lib.make_geom(N, P, C, (3, 14), (4, 4), 0)                 # reflect: a mirror without the edge
    assert gains(ctypes.byref(g), m=_lib.MODES['reflect']) == _lib.E_GEOM
    g = _lib.make_geom(N, P, C, (3, 14), (4, 4), 0)                 # full: no shift at all
    assert gains(ctypes.byref(g), m=_lib.MODES['full']) == _lib.E_GEOM
    # nothing to do: OK, and nothing written -- with every operand NULL as well
    assert gains(geom(), k_=0) == 0 and gains(geom(N=0)) == 0
    assert gains(geom(), k_=0, W_=None, ev_=None, st=None, V_=None, R_=None, out=None, mg=None) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(gain == SENTINEL)) and bool(torch.all(mag == SENTINEL))
    assert gains(geom()) == 0                                        # (and the call they were all one step from)
    torch.cuda.synchronize()
    assert not bool(torch.any(gain == SENTINEL)) and not bool(torch.any(mag == SENTINEL))


# -- the front end ------------------------------------------------------------------------------------------------------------
def check_model(nmf, dt, n_rows=40):
    """detection_gains against the closed form on the device's own render of the same rows."""
    be = nmf._backend
    mode = be._reconstruction_mode
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.95)), min_distance=1)
    det = rows_of(det, np.sort(np.argsort(-det.strength, kind='stable')[:n_rows]))
    assert len(det) > 10
    W = np.asarray(nmf.transformed_atoms, dtype=np.float64).reshape((-1,) + nmf.W.shape[1:])
    taps = int(np.prod(W.shape[1:]))
    # in the backend's terms: its order of the samples, the planes of the effective dictionary
    sample = det.sample if nmf._shuffle_idx is None else np.argsort(nmf._shuffle_idx)[det.sample]
    plane = det.atom * nmf.n_transforms + det.transform
    V = np.asarray(nmf._V, dtype=np.float64)
    R = nmf.reconstruct_detections(det).astype(np.float64)
    want, mag = gref.closed_form(V, R, W, mode, sample, plane, det.shift, det.strength.astype(np.float64))
    got = nmf.detection_gains(det)
    assert got.dtype == np.float64 and got.shape == (len(det),)
    print(f'{mode} {dt}: detection_gains({len(det)}) |gain - ref| / mag <= {np.max(np.abs(got - want) / mag):.3g}, '
          f'bar {8 * taps * 2. ** -52:.3g}; gains {got.min():.3g} .. {got.max():.3g}')
    assert np.all(np.abs(got - want) <= 8 * taps * 2. ** -52 * mag) and np.abs(want).max() > 0
    assert got.tobytes() == nmf.detection_gains(det).tobytes()
    # what the number means: the objective of the list without the row, minus that of the list (float64 on the host;
    # the bar is that of the CPU test plus the element type's rounding of the two renders)
    loo, E = gref.leave_one_out(V, W, mode, sample, plane, det.shift, det.strength.astype(np.float64))
    assert np.all(np.abs(got - loo) <= (BAR[dt] + 1e-10) * (E + mag))
    return det


def hip_model(V, n_atoms, atom_shape, **kw):
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=n_atoms, atom_shape=atom_shape, backend='hip', **kw)
    nmf.fit(V, n_iterations=5, sparsity_H=0.1)
    return nmf


def test_detection_gains_plain():
    V = np.random.default_rng(51).random((3, 2, 24, 30)).astype(np.float32)
    check_model(hip_model(V, 4, (5, 6)), 'f32')


def test_detection_gains_with_rot90():
    V = np.random.default_rng(52).random((3, 1, 20, 22)).astype(np.float32)
    det = check_model(hip_model(V, 2, (4, 4), transforms='rot90'), 'f32')
    assert len(set(det.transform.tolist())) > 1


def test_detection_gains_under_a_shuffle():
    V = np.random.default_rng(53).random((5, 1, 60))
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(7,), backend='hip')
    nmf.fit(V, batch_size=2, n_epochs=2, sparsity_H=0.1)
    nmf._shuffle_idx = np.array([3, 0, 4, 1, 2])
    det = check_model(nmf, 'f64')
    assert len(set(det.sample.tolist())) > 1


def test_detection_gains_in_reflect_mode():
    V = np.random.default_rng(54).random((2, 2, 16, 18))
    check_model(hip_model(V, 3, (4, 5), reconstruction_mode='reflect'), 'f64')


@pytest.mark.parametrize('dt', DTYPES)
def test_prune_returns_the_rows_of_the_float64_host_path(dt):
    host, det, case_ = planted_model()
    want, want_gains = host.prune_detections(det, MIN_GAIN)
    assert key(want) == key(rows_of(det, case_['true']))
    nmf = TransformInvariantNMF(n_atoms=case_['W'].shape[0], atom_shape=case_['W'].shape[2:], backend='hip')
    nmf._W = dev(case_['W'], dt)
    np.random.seed(42)
    nmf.fit(np.array(case_['V'], dtype=NP[dt]), n_iterations=0, keep_W=True)
    assert np.array_equal(nmf.W.astype(np.float64), case_['W'])
    got, gains = nmf.prune_detections(det, MIN_GAIN)
    assert isinstance(got, Detections) and gains.dtype == np.float64
    for name in ('sample', 'atom', 'transform', 'shift', 'origin'):
        np.testing.assert_array_equal(getattr(got, name), getattr(want, name))
    err = np.abs(got.strength.astype(np.float64) - want.strength) / want.strength
    print(f'{dt}: prune keeps {len(got)} of {len(det)}; strengths vs the host path {err.max():.3g}, gains '
          f'{np.max(np.abs(gains - want_gains) / want_gains):.3g}')
    assert err.max() <= BAR[dt]
    zero, zero_gains = nmf.prune_detections(det, MIN_GAIN, max_rounds=0)
    assert len(zero) == len(det) and zero_gains.shape == (len(det),)


def test_the_backend_refuses_weights_and_the_front_end_the_rest():
    V = np.random.default_rng(55).random((2, 1, 12, 14)).astype(np.float32) + 0.1
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend='hip', beta_loss=1.)
    nmf.fit(V, n_iterations=2)
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)))
    with pytest.raises(NotImplementedError):
        nmf.detection_gains(det)
    with pytest.raises(NotImplementedError):
        nmf.prune_detections(det, 0.1)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend='hip')
    nmf.fit(V, n_iterations=2, weights=np.ones((2, 1, 1, 1), dtype=np.float32))
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)))
    with pytest.raises(NotImplementedError):
        nmf.detection_gains(det)
    with pytest.raises(NotImplementedError):
        nmf.prune_detections(det, 0.1)
    with pytest.raises(NotImplementedError):                        # ... nor does the backend take it
        nmf._backend.event_gains(None, nmf._W, det.sample, det.atom, det.shift, det.strength)
    np.random.seed(42)
    vol = TransformInvariantNMF(n_atoms=1, atom_shape=(2, 2, 2), backend='hip')
    vol.fit(np.random.default_rng(56).random((1, 1, 5, 5, 5)).astype(np.float32), n_iterations=1)
    det = vol.detections(threshold=float(np.quantile(vol.H, 0.9)))
    with pytest.raises(NotImplementedError):
        vol.detection_gains(det)
    with pytest.raises(NotImplementedError):
        vol.prune_detections(det, 0.1)
