"""
Forward selection of events on the GPU: tnmf_hip_events_norms, tnmf_hip_pursuit_score and tnmf_hip_pursuit_pick through the
C ABI, and ``pursue_detections`` on ``backend='hip'``, against tests/pursuit_reference.py in float64 on the same numbers.

The bars.  Sums: with eps = 8 * taps * 2^-52, taps = C * prod(A) -- either side adds at most 4 * taps terms per sum (an event
has at most four images) in double, the derivation of tests/test_hip_events_gain.py -- |b - ref| <= eps * ref (all terms are
non-negative) and |a - ref| <= eps * mag, mag = sum |w (V - R)|.  Through the quotients, to first order:
  h = max(a, 0) / b:      |h - ref| <= eps * (mag + |a|) / b, plus half an ulp of the element type for its one rounding;
  gain = a^2 / (2 b):     |g - ref| <= eps * (|a| * mag / b + a^2 / (2 b)).
The score kernel is one correctly rounded double product and quotient rounded once: bit-identical to the numpy expression.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import events_reference as eref
import pursuit_reference as pur
from test_events_cpu import MODES
from test_hip_events import DTYPES, NP, backend, dev, p
from test_hip_events_gain import MODE_CASES, case as gain_case
from test_pursuit_cpu import NOISY_MIN_GAIN, NOISY_SEEDS, SEEDS, boxes_disjoint, key, noisy, separated, wrapped_scene
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
HALF_ULP = {'f32': 2. ** -24, 'f64': 2. ** -53}


def context():
    """Any initialised backend: the entries take their geometry per call."""
    be = backend(2, 2, 3, (20, 23), (4, 6), 'circular', 'f32')
    return be._lib, be._ctx, be


# -- 1. norms ---------------------------------------------------------------------------------------------------------------------
NORM_SHAPES = {'1d': (2, 3, (40,), (5,)), '2d': (2, 2, (24, 26), (4, 4)), '2d-tall': (1, 2, (6, 300), (6, 3))}


@functools.lru_cache(maxsize=None)
def norm_case(shape, mode):
    """-> (W, reference b): W float32-representable with a zero first row and column in plane 0, so that in 'valid' mode the
    shifts that show only those taps have a norm of exactly 0."""
    C, P, D, A = NORM_SHAPES[shape]
    rng = np.random.default_rng(61)
    W = (rng.random((P, C) + A) + 0.1).astype(np.float32).astype(np.float64)
    W[(0, slice(None)) + (-1,) * len(A)] = 0.        # the tap the first corner of 'valid' shows
    W.setflags(write=False)
    return W, pur.Table(W, D, mode).norms()


def norms_call(W, D, mode, dt, N=2):
    lib, ctx, _ = context()
    P, C, A = W.shape[0], W.shape[1], W.shape[2:]
    S = eref.shift_shape(D, A, mode)
    b = torch.full((P,) + S, float('nan'), dtype=torch.float64, device='cuda')
    g = _lib.make_geom(N, P, C, D, A, DTYPES.index(dt))
    Wd = dev(W, dt)                                                                     # (held until the call has run)
    code = lib.tnmf_hip_events_norms(ctx, ctypes.byref(g), _lib.MODES[mode], p(Wd), p(b), None)
    torch.cuda.synchronize()
    return code, b.cpu().numpy()


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', list(NORM_SHAPES))
def test_norms_against_the_reference(shape, mode, dt):
    C, P, D, A = NORM_SHAPES[shape]     # ('2d-tall': A = D on the first axis -- in 'full' one row of shifts)
    W, want = norm_case(shape, mode)
    code, b = norms_call(W, D, mode, dt)
    assert code == 0 and not np.isnan(b).any(), 'every element is written'
    taps = C * int(np.prod(A))
    err = np.abs(b - want)
    print(f'{shape} {mode} {dt}: |b - ref| / ref <= {np.max(err[want > 0] / want[want > 0]):.3g}, bar {8 * taps * 2. ** -52:.3g}; '
          f'{int(np.sum(want == 0))} zeros')
    assert np.all(err <= 8 * taps * 2. ** -52 * want)
    assert np.all(b[want == 0] == 0)
    if mode == 'valid':
        assert want[(0,) + (0,) * len(D)] == 0 and np.sum(want == 0) >= 1       # such entries exist
    if shape != '2d-tall':      # the shortcut's entries are among them: the middle shift lies wholly inside
        interior = want[(1,) + tuple(s // 2 for s in want.shape[1:])]
        assert abs(interior - float(np.sum(W[1] ** 2))) <= 1e-12 * interior
    code2, b2 = norms_call(W, D, mode, dt, N=0)                                  # the table does not depend on the samples
    assert code2 == 0 and b2.tobytes() == b.tobytes()


# -- 2. score ---------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 63, 64, 65, 130)


def score_case(width, dt, two_axes=True):
    """a [N, P, Sy, width] with negative values, zeros, NaN and +inf; b [P, Sy, width] with zeros; the numpy expression."""
    rng = np.random.default_rng(62 + width)
    N, P, Sy = 2, 3, (5 if two_axes else 1)
    a = (rng.standard_normal((N, P, Sy, width)) * 3.).astype(NP[dt])
    a.reshape(-1)[rng.integers(a.size, size=max(2, a.size // 9))] = 0.
    a.reshape(-1)[rng.integers(a.size, size=max(2, a.size // 17))] = np.nan
    a.reshape(-1)[rng.integers(a.size, size=max(2, a.size // 19))] = np.inf
    a[0, 0, 0, 0], a[1, 2, Sy - 1, width - 1] = 2.5, 1.25          # (live corners)
    b = rng.random((P, Sy, width)) + 0.01
    b.reshape(-1)[rng.integers(b.size, size=max(2, b.size // 11))] = 0.
    b[0, 0, 0], b[2, Sy - 1, width - 1] = 0.75, 0.5
    a64 = a.astype(np.float64)
    with np.errstate(all='ignore'):
        want = np.where((a64 > 0) & (b > 0), (a64 * a64 / (2. * b)).astype(NP[dt]), NP[dt](0))
    taken = np.array([-1, 0, a.size - 1, a.size, 2 ** 40, 7 % a.size, a.size // 2], dtype=np.int64)
    want.reshape(-1)[taken[(taken >= 0) & (taken < a.size)]] = 0.
    return a, b, want.astype(NP[dt]), taken


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('stride', ['contiguous', 'lines', 'odd'])
@pytest.mark.parametrize('width', WIDTHS)
def test_score_is_the_numpy_expression_bit_for_bit(width, stride, dt):
    for two_axes in (True, False):
        a, b, want, taken = score_case(width, dt, two_axes)
        N, P, Sy, _ = a.shape
        # rows padded to whole 16-byte units and beyond ('lines': the 16-byte accesses), or by a width that breaks them
        Hs = {'contiguous': width, 'lines': (width + 3) // 4 * 4 + 4, 'odd': width + (1 if (width + 1) % 4 else 3)}[stride]
        lib, ctx, _ = context()
        store_a = torch.full((N, P, Sy, Hs), SENTINEL, dtype=getattr(torch, np.dtype(NP[dt]).name), device='cuda')
        store_a[..., :width] = torch.from_numpy(a).cuda()
        store_g = torch.full_like(store_a, SENTINEL)
        bd, td = torch.from_numpy(b).cuda(), torch.from_numpy(taken).cuda()
        D, A = ((Sy, width), (1, 1)) if two_axes else ((width,), (1,))
        g = _lib.make_geom(N, P, 1, D, A, DTYPES.index(dt), 0 if stride == 'contiguous' else Hs)
        assert lib.tnmf_hip_pursuit_score(ctx, ctypes.byref(g), p(store_a), p(bd), p(store_g), p(td), len(taken), None) == 0
        torch.cuda.synchronize()
        got = store_g.cpu().numpy()
        assert got[..., :width].tobytes() == want.tobytes(), (two_axes, np.flatnonzero(got[..., :width] != want)[:5])
        assert np.all(got[..., width:] == SENTINEL), 'pad columns are not written'
        assert np.count_nonzero(want) >= 1 and not np.isnan(want).any()
        if a.size > 500:
            assert np.isinf(want).any() and np.isnan(a).any() and np.any(a < 0) and np.any(a == 0) and np.any(b == 0)
        # in place on the map, and without a list
        assert lib.tnmf_hip_pursuit_score(ctx, ctypes.byref(g), p(store_a), p(bd), p(store_a), p(td), len(taken), None) == 0
        torch.cuda.synchronize()
        assert store_a.cpu().numpy().tobytes() == got.tobytes()
        store_a[..., :width] = torch.from_numpy(a).cuda()
        assert lib.tnmf_hip_pursuit_score(ctx, ctypes.byref(g), p(store_a), p(bd), p(store_g), None, 0, None) == 0
        torch.cuda.synchronize()
        inside = taken[(taken >= 0) & (taken < a.size)]
        again = store_g.cpu().numpy()[..., :width].reshape(-1)
        rest = np.ones(a.size, dtype=bool)
        rest[inside] = False
        assert again[rest].tobytes() == want.reshape(-1)[rest].tobytes() and np.any(again[inside] != 0)


def test_score_walks_a_map_larger_than_its_grid():
    """More 16-byte chunks than num_cu * 8 workgroups hold threads: the grid stride, its carries from chunk to row to plane --
    on a contiguous map (one long row per sample), on rows padded to 16 bytes and on rows that break the alignment."""
    rng = np.random.default_rng(63)
    N, P, Sy, Sx = 5, 4, 97, 1531
    assert N * P * Sy * (Sx // 4) > torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    a = (rng.standard_normal((N, P, Sy, Sx)) * 2.).astype(np.float32)
    b = rng.random((P, Sy, Sx)) + 0.01
    b[rng.random(b.shape) < 0.1] = 0.
    a64 = a.astype(np.float64)
    with np.errstate(all='ignore'):
        want = np.where((a64 > 0) & (b > 0), (a64 * a64 / (2. * b)).astype(np.float32), np.float32(0))
    lib, ctx, _ = context()
    bd = torch.from_numpy(b).cuda()
    for Hs in (Sx, 1532, 1533):
        store = torch.full((N, P, Sy, Hs), SENTINEL, dtype=torch.float32, device='cuda')
        store[..., :Sx] = torch.from_numpy(a).cuda()
        out = torch.full_like(store, SENTINEL)
        g = _lib.make_geom(N, P, 1, (Sy, Sx), (1, 1), 0, Hs)
        assert lib.tnmf_hip_pursuit_score(ctx, ctypes.byref(g), p(store), p(bd), p(out), None, 0, None) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got[..., :Sx].tobytes() == want.tobytes() and np.all(got[..., Sx:] == SENTINEL), Hs


# -- 3. pick ----------------------------------------------------------------------------------------------------------------------
PICK_CASES = MODE_CASES + ['taps-9', 'taps-75', 'taps-320', '1d-7']


def pick_call(name, dt, with_mag=True):
    """One call on poisoned outputs for the rows of tests/test_hip_events_gain.py's case: the rows outside the contract go in
    as flat indices out of range.  -> (code, flat indices, events, strength, gain, mag)."""
    geo, rows, _, W, V, R, _, _, good = gain_case(name)
    N, C, P, D, A, mode = geo
    S = eref.shift_shape(D, A, mode)
    entries = N * P * int(np.prod(S))
    idx = np.empty(len(rows), dtype=np.int64)
    idx[good] = np.ravel_multi_index(tuple(rows[good].T), (N, P) + S)
    idx[~good] = np.resize(np.array([-1, entries, entries + 5, 2 ** 40, -2 ** 40], dtype=np.int64), int((~good).sum()))
    lib, ctx, _ = context()
    K = len(idx)
    ev = torch.full((K, 4), -7, dtype=torch.int32, device='cuda')
    h = torch.full((K,), float('nan'), dtype=getattr(torch, np.dtype(NP[dt]).name), device='cuda')
    gain = torch.full((K,), float('nan'), dtype=torch.float64, device='cuda')
    mag = torch.full((K,), float('nan'), dtype=torch.float64, device='cuda') if with_mag else None
    g = _lib.make_geom(N, P, C, D, A, DTYPES.index(dt))
    Wd, Vd, Rd, at = dev(W, dt), dev(V, dt), dev(R, dt), torch.from_numpy(idx).cuda()   # (held until the call has run)
    code = lib.tnmf_hip_pursuit_pick(ctx, ctypes.byref(g), _lib.MODES[mode], p(Wd), p(at), K, p(Vd), p(Rd), p(ev), p(h),
                                     p(gain), p(mag), None)
    torch.cuda.synchronize()
    return code, idx, ev.cpu().numpy(), h.cpu().numpy(), gain.cpu().numpy(), None if mag is None else mag.cpu().numpy()


@functools.lru_cache(maxsize=None)
def pick_reference(name):
    geo, rows, _, W, V, R, _, _, good = gain_case(name)
    a, b, mag = np.zeros((3, len(rows)))
    a[good], b[good], mag[good] = pur.exact(V, R, W, geo[5], rows[good])
    return a, b, mag


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', PICK_CASES)
def test_pick_against_the_reference(name, dt):
    geo, rows, _, W, V, R, _, _, good = gain_case(name)
    N, C, P, D, A, mode = geo
    k = len(D)
    taps = C * int(np.prod(A))
    a, b, want_mag = pick_reference(name)
    code, idx, ev, h, gain, mag = pick_call(name, dt)
    assert code == 0 and not np.isnan(h).any() and not np.isnan(gain).any() and not np.isnan(mag).any()
    want_ev = np.full((len(rows), 4), -1, dtype=np.int32)
    want_ev[good, :2], want_ev[good, 4 - k:] = rows[good, :2], rows[good, 2:]
    if k == 1:
        want_ev[good, 2] = 0
    assert np.array_equal(ev, want_ev)
    assert not h[~good].any() and not gain[~good].any() and not mag[~good].any() and (~good).sum() == (7 if k == 2 and
                                                                                                     name in MODE_CASES else 0)
    eps = 8 * taps * 2. ** -52
    full = (ev, h, gain, mag)
    a, b, want_mag, h, gain, mag = (x[good] for x in (a, b, want_mag, h, gain, mag))
    assert np.all(b > 0) and np.any(a > 0) and np.any(a < 0)
    want_h, want_gain = np.maximum(a, 0.) / b, np.where(a > 0, a * a / (2. * b), 0.)
    bar_h = eps * (want_mag + np.abs(a)) / b + HALF_ULP[dt] * want_h
    bar_gain = eps * (np.abs(a) * want_mag / b + want_gain)
    print(f'{name} {dt}: {int(good.sum())} rows, taps {taps}; |h - ref| / bar <= {np.max(np.abs(h - want_h) / bar_h):.3g}, '
          f'|gain - ref| / bar <= {np.max(np.abs(gain - want_gain) / bar_gain):.3g}, |mag - ref| / mag <= '
          f'{np.max(np.abs(mag - want_mag) / want_mag):.3g}')
    assert np.all(np.abs(h.astype(np.float64) - want_h) <= bar_h)
    assert np.all(np.abs(gain - want_gain) <= bar_gain)
    assert np.all(np.abs(mag - want_mag) <= eps * want_mag)
    clear = a < -eps * want_mag                      # residuals clearly against the row: exactly nothing
    assert clear.any() and not h[clear].any() and not gain[clear].any()
    # the same bits again, and without mag
    again = pick_call(name, dt)
    assert again[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(again[2:], full))
    bare = pick_call(name, dt, with_mag=False)
    assert bare[0] == 0 and bare[5] is None and all(x.tobytes() == y.tobytes() for x, y in zip(bare[2:5], full[:3]))


def test_the_pick_cases_hold_every_kind_of_row():
    from tnmf_amd.TransformInvariantNMF import event_images
    for name in ('circular', 'reflect'):
        geo, rows, _, _, _, _, _, _, good = gain_case(name)
        S = eref.shift_shape(geo[3], geo[4], geo[5])
        n_images = np.bincount(event_images(rows[good, 2:], geo[4], S, geo[5])[0])
        assert set(n_images.tolist()) == {1, 2, 4} and (~good).sum() == 7


# -- 4. end to end ----------------------------------------------------------------------------------------------------------------
def hip_model(W, V, mode, dt, **kw):
    nmf = TransformInvariantNMF(n_atoms=W.shape[0], atom_shape=W.shape[2:], backend='hip', reconstruction_mode=mode, **kw)
    nmf._W = dev(W, dt)
    np.random.seed(42)
    nmf.fit_batch(np.array(V, dtype=NP[dt]), n_iterations=0, keep_W=True)
    assert np.array_equal(nmf.W.astype(np.float64), W)
    return nmf


FAMILIES = {('auto', 'f32'): ('split', 'mfma', 'generic'), ('auto', 'f64'): ('generic',), ('fft', 'f32'): ('fft',),
            ('fft', 'f64'): ('fft',), ('mfma', 'f32'): ('mfma',)}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('path,dt', list(FAMILIES))
def test_separated_scenes_end_to_end(path, dt, mode):
    for seed in SEEDS:
        case, table = separated(seed, mode)
        V, W, rows = case['V'], case['W'], case['rows']
        taps = W.shape[1] * int(np.prod(W.shape[2:]))
        ref = pur.pursue(V, W, mode, 1e-6, table=table)
        nmf = hip_model(W, V, mode, dt, path=path)
        H_before = nmf.H.copy()
        det, gains = nmf.pursue_detections(1e-6, refit_iterations=0, n_iterations=0)
        assert nmf._backend.last_path in FAMILIES[path, dt], nmf._backend.last_path
        assert key(det) == sorted((n, q, 0) + tuple(u) for n, q, *u in rows.tolist())
        hist = nmf.pursuit_history_
        assert np.array_equal(hist[:, :2], ref['history'][:, :2]) and hist[:, 1].tolist() == [10, 0]
        got = np.column_stack([det.sample, det.atom, det.shift])
        a, b, mag = pur.exact(V, np.zeros(V.shape), W, mode, got)
        by_row = {tuple(r): x for r, x in zip(ref['rows'].tolist(), ref['strength'])}
        want_h = np.array([by_row[tuple(r)] for r in got.tolist()])
        eps = 8 * taps * 2. ** -52
        bar_h = eps * (mag + np.abs(a)) / b + HALF_ULP[dt] * want_h
        print(f'{path} {dt} {mode} seed {seed}: {nmf._backend.last_path}; |h - ref| / bar <= '
              f'{np.max(np.abs(det.strength - want_h) / bar_h):.3g}')
        assert np.all(np.abs(det.strength.astype(np.float64) - want_h) <= bar_h)
        assert abs(hist[0, 2] - ref['history'][0, 2]) <= np.sum(eps * (np.abs(a) * mag / b + a * a / (2. * b)))
        assert gains.shape == (10,) and np.all(gains > 1e-3)
        assert np.array_equal(nmf.H, H_before), 'the dense H is left as it is'


@pytest.mark.parametrize('path,dt', list(FAMILIES))
def test_a_circular_event_wrapped_on_both_axes_end_to_end(path, dt):
    """4 images and the whole sample for a box: one event per sample, the only scene of that kind with a known answer."""
    V, W, rows, h = wrapped_scene()
    nmf = hip_model(W, V, 'circular', dt, path=path)
    det, _ = nmf.pursue_detections(1e-6, refit_iterations=0, n_iterations=0)
    assert nmf._backend.last_path in FAMILIES[path, dt]
    assert key(det) == sorted((n, q, 0) + tuple(u) for n, q, *u in rows.tolist())
    assert nmf.pursuit_history_[:, 1].tolist() == [2, 0]
    got = np.column_stack([det.sample, det.atom, det.shift])
    a, b, mag = pur.exact(V, np.zeros(V.shape), W, 'circular', got)
    taps = W.shape[1] * int(np.prod(W.shape[2:]))
    bar_h = 8 * taps * 2. ** -52 * (mag + np.abs(a)) / b + HALF_ULP[dt] * a / b
    assert np.all(np.abs(det.strength.astype(np.float64) - a / b) <= bar_h)


# -- 5. the residual is fresh each round ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('mode', MODES)
def test_with_the_spectrum_cache_enabled_every_round_correlates_its_own_residual(mode, dt):
    """path='fft' with tnmf_hip_ctx_set_cache on.  What a reused spectrum of the residual would do: round 2 ranks by round 1's
    map.  The kept rows are scored again exactly by the pick kernel, so the energy bookkeeping holds whatever map ranked them
    -- it guards the additions, not the map.  A stale map shows in the ROUNDS: with the taken entries zeroed, round 1's map
    offers its runners-up, whose exact gains against the true residual fall below the threshold, so the rows added per round
    and the support differ from the float64 reference's; and in the counters: a hit on the samples' spectra during the call.
    In 'valid' mode the fit's binding is explicit and the residual, a foreign pointer, is never tracked, so there the
    counters hold with or without the invalidation; the hazard is live in the three other modes, where the forced-on cache
    binds implicitly to whatever pointer it is given -- the residual's."""
    for seed in NOISY_SEEDS:
        case, table = noisy(seed, mode)
        V, W = case['V'], case['W']
        nmf = hip_model(W, V, mode, dt, path='fft')
        be = nmf._backend
        _lib.check(be._lib.tnmf_hip_ctx_set_cache(be._ctx, 1), 'tnmf_hip_ctx_set_cache')
        before = be.cache_counters
        det, _ = nmf.pursue_detections(NOISY_MIN_GAIN, refit_iterations=0, n_iterations=0)
        after = be.cache_counters
        hist = nmf.pursuit_history_
        assert be.last_path == 'fft' and len(hist) >= 3
        rows = np.column_stack([det.sample, det.atom, det.shift])
        assert len(np.unique(rows, axis=0)) == len(rows) == int(hist[:, 1].sum())
        first = 0
        for count in hist[:, 1].astype(int):
            assert boxes_disjoint(rows[first:first + count], W.shape[2:], V.shape[2:], table.S, mode)
            first += count
        E = pur.energy(V, W, mode, rows, det.strength.astype(np.float64))
        booked = 0.5 * float(np.sum(V * V)) - float(hist[:, 2].sum())
        print(f'{mode} {dt} seed {seed}: added {hist[:, 1].astype(int).tolist()}, |booked - E| = {abs(booked - E):.3g}')
        assert abs(booked - E) <= NOISY_MIN_GAIN / 100
        ref = pur.pursue(V, W, mode, NOISY_MIN_GAIN, table=table)      # the rounds of a fresh residual every time
        assert hist[:, 1].tolist() == ref['history'][:, 1].tolist()
        assert sorted(map(tuple, rows.tolist())) == sorted(map(tuple, ref['rows'].tolist()))
        # every round transformed its residual: one pass over the samples per round, none of them taken from the cache
        assert after['v_runs'] - before['v_runs'] >= len(hist) and after['v_hits'] == before['v_hits']
    if mode == 'valid':
        # the cache is still on and still the fit's: the second of two H half steps finds the spectra of V
        nmf._update_H()
        mid = be.cache_counters
        nmf._update_H()
        assert be.cache_counters['v_hits'] > mid['v_hits']


# -- 6. refusals ------------------------------------------------------------------------------------------------------------------
E_NULL, E_DTYPE = -1, -3


def test_refused_norms_write_nothing():
    lib, ctx, _ = context()
    C, P, D, A = NORM_SHAPES['2d']
    W = dev(norm_case('2d', 'circular')[0], 'f32')
    b = torch.full((P,) + D, SENTINEL, dtype=torch.float64, device='cuda')

    def geom(**kw):
        g = _lib.make_geom(2, P, C, D, A, 0)
        for name, val in kw.items():
            setattr(g, name, val)
        return ctypes.byref(g)

    def call(g, m=_lib.MODES['circular'], W_=W, out=b, c=ctx):
        return lib.tnmf_hip_events_norms(c, g, m, p(W_), p(out), None)
    assert call(geom(), c=None) == E_NULL and call(None) == E_NULL
    assert call(geom(), W_=None) == E_NULL and call(geom(), out=None) == E_NULL
    assert call(geom(dtype=2)) == E_DTYPE and call(geom(ndim=3)) == _lib.E_UNSUPPORTED
    assert call(geom(M=65536)) == _lib.E_UNSUPPORTED
    for kw in (dict(ndim=0), dict(ndim=4), dict(N=-1), dict(M=0), dict(C=0)):
        assert call(geom(**kw)) == _lib.E_GEOM, kw
    assert call(geom(), m=4) == _lib.E_GEOM and call(geom(), m=-1) == _lib.E_GEOM
    g = _lib.make_geom(2, P, C, (3, 14), (4, 4), 0)                 # full: no shift at all
    assert call(ctypes.byref(g), m=_lib.MODES['full']) == _lib.E_GEOM
    torch.cuda.synchronize()
    assert bool(torch.all(b == SENTINEL))
    assert call(geom()) == 0
    torch.cuda.synchronize()
    assert not bool(torch.any(b == SENTINEL))


def test_refused_scores_write_nothing():
    lib, ctx, _ = context()
    a, b, _, taken = score_case(65, 'f32')
    N, P, Sy, Sx = a.shape
    ad, bd, td = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(taken).cuda()
    out = torch.full_like(ad, SENTINEL)

    def geom(**kw):
        g = _lib.make_geom(N, P, 1, (Sy, Sx), (1, 1), 0)
        for name, val in kw.items():
            setattr(g, name, val)
        return ctypes.byref(g)

    def call(g, a_=ad, b_=bd, out_=out, t_=td, n_=len(taken), c=ctx):
        return lib.tnmf_hip_pursuit_score(c, g, p(a_), p(b_), p(out_), p(t_), n_, None)
    assert call(geom(), c=None) == E_NULL and call(None) == E_NULL
    for kw in (dict(a_=None), dict(b_=None), dict(out_=None), dict(t_=None)):
        assert call(geom(), **kw) == E_NULL, kw
    assert call(geom(dtype=2)) == E_DTYPE and call(geom(ndim=3)) == _lib.E_UNSUPPORTED
    for kw in (dict(ndim=0), dict(ndim=4), dict(N=-1), dict(M=0), dict(h_row_stride=Sx - 1)):
        assert call(geom(**kw)) == _lib.E_GEOM, kw
    assert call(geom(), n_=-1) == _lib.E_GEOM
    assert call(geom(N=0)) == 0                                     # nothing to do
    torch.cuda.synchronize()
    assert bool(torch.all(out == SENTINEL))
    assert call(geom()) == 0
    torch.cuda.synchronize()
    assert not bool(torch.any(out == SENTINEL))


def test_refused_picks_write_nothing():
    geo, rows, _, W, V, R, _, _, good = gain_case('circular')
    N, C, P, D, A, mode = geo
    lib, ctx, _ = context()
    idx = torch.from_numpy(np.ravel_multi_index(tuple(rows[good].T), (N, P) + D)).cuda()
    K = idx.numel()
    Wd, Vd, Rd = dev(W, 'f32'), dev(V, 'f32'), dev(R, 'f32')
    ev = torch.full((K, 4), -7, dtype=torch.int32, device='cuda')
    h = torch.full((K,), SENTINEL, dtype=torch.float32, device='cuda')
    gain = torch.full((K,), SENTINEL, dtype=torch.float64, device='cuda')
    mag = torch.full((K,), SENTINEL, dtype=torch.float64, device='cuda')

    def geom(**kw):
        g = _lib.make_geom(N, P, C, D, A, 0)
        for name, val in kw.items():
            setattr(g, name, val)
        return ctypes.byref(g)

    def call(g, m=_lib.MODES[mode], W_=Wd, i_=idx, k_=K, V_=Vd, R_=Rd, ev_=ev, h_=h, out=gain, mg=mag, c=ctx):
        return lib.tnmf_hip_pursuit_pick(c, g, m, p(W_), p(i_), k_, p(V_), p(R_), p(ev_), p(h_), p(out), p(mg), None)
    assert call(geom(), c=None) == E_NULL and call(None) == E_NULL
    for kw in (dict(W_=None), dict(i_=None), dict(V_=None), dict(R_=None), dict(ev_=None), dict(h_=None), dict(out=None)):
        assert call(geom(), **kw) == E_NULL, kw
    assert call(geom(dtype=2)) == E_DTYPE and call(geom(dtype=-1)) == E_DTYPE
    assert call(geom(ndim=3)) == _lib.E_UNSUPPORTED and call(geom(), k_=2 ** 31) == _lib.E_UNSUPPORTED
    for kw in (dict(ndim=0), dict(ndim=4), dict(N=-1), dict(M=0), dict(C=0)):
        assert call(geom(**kw)) == _lib.E_GEOM, kw
    assert call(geom(), m=4) == _lib.E_GEOM and call(geom(), m=-1) == _lib.E_GEOM and call(geom(), k_=-1) == _lib.E_GEOM
    g = _lib.make_geom(N, P, C, (2, 14), (4, 4), 0)                 # circular: more than one wrap
    assert call(ctypes.byref(g)) == _lib.E_GEOM
    assert call(geom(), k_=0) == 0                                  # nothing to do
    assert call(geom(), k_=0, W_=None, i_=None, V_=None, R_=None, ev_=None, h_=None, out=None, mg=None) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(ev == -7)) and bool(torch.all(h == SENTINEL)) and bool(torch.all(gain == SENTINEL))
    assert bool(torch.all(mag == SENTINEL))
    assert call(geom()) == 0
    torch.cuda.synchronize()
    assert not bool(torch.any(h == SENTINEL)) and not bool(torch.any(gain == SENTINEL)) and bool(torch.all(ev[:, 0] >= 0))


# -- 7. the front end's refusals on the backend -----------------------------------------------------------------------------------
def test_the_backend_refuses_weights():
    V = np.random.default_rng(55).random((2, 1, 12, 14)).astype(np.float32) + 0.1
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend='hip')
    nmf.fit(V, n_iterations=2, weights=np.ones((2, 1, 1, 1), dtype=np.float32))
    with pytest.raises(NotImplementedError):
        nmf.pursue_detections(0.1)
    none = np.zeros(0, dtype=np.int64)
    with pytest.raises(NotImplementedError):
        nmf._backend.pursue_events(None, nmf._W, none, none, np.zeros((0, 2), dtype=np.int64), np.zeros(0), 0.1)
