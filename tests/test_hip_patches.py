"""
Patches on the GPU: tnmf_hip_events_patches and tnmf_hip_patch_moments through the C ABI on the cases of
tests/patches_dispatch.py, against the independent reference tests/patches_reference.py (extended precision, from the
definitions), and ``detection_patches`` / ``atom_patch_moments`` / ``atom_modes`` on ``backend='hip'`` on the planted problem
of tests/test_patches_cpu.py.  Every bound is derived from the roundings of the definition with U = 2^-53 (the docstrings
count them); every test prints the largest ratio of an error to its bound.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch

import patches_dispatch as pd
import patches_reference as pref
from test_hip_events import DTYPES, NP, backend, dev, p
from test_patches_cpu import K0, case, check_additive, check_planted, planted_model, reference, table_of
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF, modes_from_moments

pytestmark = pytest.mark.gpu

U = pref.U
SENTINEL = -12345.5
GROUP_TABLES = (None, 'flip', 'rot90')        # no table, or single entries of weight 1: a permutation


def context():
    """Any initialised backend: the entries take their geometry per call."""
    be = backend(2, 2, 3, (20, 23), (4, 6), 'circular', 'f32')
    return be._lib, be._ctx


def events_of(rows, k):
    """[K, 4] int32 on the device: (n, p, u_0, u_1), one shift axis as (n, p, 0, u_0)."""
    ev = np.zeros((len(rows), 4), dtype=np.int32)
    ev[:, :2] = rows[:, :2]
    ev[:, 4 - k:] = rows[:, 2:]
    return torch.from_numpy(ev).cuda()


@functools.lru_cache(maxsize=None)
def device_table(name, A):
    ptr, src, w, T = table_of(name, A)
    if ptr is None:
        return None, None, None, 1
    return torch.from_numpy(ptr).cuda(), torch.from_numpy(src).cuda(), torch.from_numpy(w).cuda(), T


@functools.lru_cache(maxsize=None)
def folded(name, source, table):
    """(y, bound of y) of the case in the frame of ``table``: the reference and what the device's rounding may add."""
    x, mag, _ = reference(name, source)
    return pref.fold(x, pref.ROUNDINGS[source] * U * mag, case(name)[0][:, 1], table_of(table, pd.PATCH_CASES[name][4]))


def call_patches(name, source, table, dt, fill=float('nan')):
    """-> (code, out [K, C, *A]) of one call on a poisoned output."""
    N, C, P, D, A, mode, _ = pd.PATCH_CASES[name]
    rows, h, W, V, R = case(name)
    lib, ctx = context()
    out = torch.full((len(rows), C) + A, fill, dtype=torch.float64, device='cuda')
    g = _lib.make_geom(N, P, C, D, A, DTYPES.index(dt))
    Wd, hd, Vd, Rd, ev = dev(W, dt), dev(h, dt), dev(V, dt), dev(R, dt), events_of(rows, len(D))
    ptr, src, w, T = device_table(table, A)
    code = lib.tnmf_hip_events_patches(ctx, ctypes.byref(g), _lib.MODES[mode], _lib.PATCH_SOURCES[source], p(Wd), p(ev), p(hd),
                                       len(rows), p(Vd), p(Rd), p(ptr), p(src), p(w), T, p(out), None)
    torch.cuda.synchronize()
    return code, out.cpu().numpy()


# -- 1. tnmf_hip_events_patches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', list(pd.PATCH_CASES))
def test_patches_against_the_definition(name, dt):
    """|x - x_ref| <= c U sum |terms| per element, c the roundings of the definition: the additions of the images (at most 4
    images: 3), for 'residual' the subtraction (+ 1), for 'cleaned' the fma (+ 1) and the additions inside phi (+ 4) -- 3, 4
    and 9; sum |terms| = sum over the images of |V| + |R| + h sum |w|.  Through a table the bound of an element is
    sum |w_k| bound(x[src_k]) and, where the row has several entries or a weight other than 1, (entries + 1) U sum |w x| on
    top.  The inputs are float32-representable, so both element types see the same numbers.  'data' of a single-image row
    under no table or a permutation is (double)V to the bit."""
    N, C, P, D, A, mode, tables = pd.PATCH_CASES[name]
    rows, h, W, V, R = case(name)
    good = pref.in_range(rows, N, P, pref.shift_shape(D, A, mode))
    assert torch.cuda.get_device_properties(0).multi_processor_count <= 256 or name != 'grid-stride'
    for source in (pref.SOURCES if name != 'grid-stride' else ('cleaned',)):
        n_images = reference(name, source)[2]
        for table in tables:
            want, bound = folded(name, source, table)
            code, got = call_patches(name, source, table, dt)
            assert code == 0
            assert not np.isnan(got).any(), 'every element is written'
            assert not got[~good].any(), 'zeros for a row out of range'
            err = np.abs(got - want)
            live = bound > 0
            print(f'{name} {dt} {source} table {table}: {len(rows)} rows, largest error / bound '
                  f'{np.max(err[live] / bound[live]) if live.any() else 0.:.3g}')
            assert np.all(err <= bound)
            if source == 'data' and table in GROUP_TABLES:
                one = n_images == 1
                assert one.any() and got[one].tobytes() == np.asarray(want[one], dtype=np.float64).tobytes()
            code2, again = call_patches(name, source, table, dt, fill=SENTINEL)
            assert code2 == 0 and again.tobytes() == got.tobytes(), 'the same bits run after run'


def test_the_largest_staged_patch_launches():
    """C * prod(A) = TNMF_PATCH_STAGE_MAX doubles with a table: the four waves of a workgroup stage 64 KiB of dynamic LDS,
    the most the launch takes; one double more is refused (test_refused_patches_write_nothing).  A 1-D atom of 2048 taps
    under 'flip', rows clipped at both ends of the 'valid' shift range and one in the middle; bounds as above."""
    N, C, P, D, A, mode = 1, 1, 2, (2060,), (pd.STAGE_MAX,), 'valid'
    assert pd.patches_launch(5, N, C, A, True, 256) == (2, 4 * pd.STAGE_MAX * 8) and 4 * pd.STAGE_MAX * 8 == 64 * 1024
    rng = np.random.default_rng(71)
    rows = np.array([[0, 0, 0], [0, 1, 2047], [0, 0, 2053], [0, 1, 4106], [0, 1, 2053]], dtype=np.int64)
    h = (rng.random(len(rows)) + 0.5).astype(np.float32).astype(np.float64)
    W = (rng.random((P, C) + A) + 0.1).astype(np.float32).astype(np.float64)
    V = (rng.random((N, C) + D) * 3.).astype(np.float32).astype(np.float64)
    R = np.asarray(pref.render(W, D, N, mode, rows, h), dtype=np.float64).astype(np.float32).astype(np.float64)
    lib, ctx = context()
    ptr, src, w, T = device_table('flip', A)
    assert ptr.numel() == 2 * pd.STAGE_MAX + 1
    wanted = {}
    for source in pref.SOURCES:
        x, mag, _ = pref.patches(V, R, W, mode, rows, h, source)
        wanted[source] = pref.fold(x, pref.ROUNDINGS[source] * U * mag, rows[:, 1], table_of('flip', A))
    for dt in DTYPES:
        g = _lib.make_geom(N, P, C, D, A, DTYPES.index(dt))
        Wd, hd, Vd, Rd, ev = dev(W, dt), dev(h, dt), dev(V, dt), dev(R, dt), events_of(rows, 1)
        for source in pref.SOURCES:
            want, bound = wanted[source]
            out = torch.full((len(rows), C) + A, float('nan'), dtype=torch.float64, device='cuda')
            assert lib.tnmf_hip_events_patches(ctx, ctypes.byref(g), _lib.MODES[mode], _lib.PATCH_SOURCES[source], p(Wd), p(ev),
                                               p(hd), len(rows), p(Vd), p(Rd), p(ptr), p(src), p(w), T, p(out), None) == 0
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert not np.isnan(got).any(), 'every element is written'
            err, live = np.abs(got - want), bound > 0
            print(f'2048 taps {dt} {source} table flip: largest error / bound '
                  f'{np.max(err[live] / bound[live]) if live.any() else 0.:.3g}')
            assert np.all(err <= bound) and np.abs(want).max() > 0
            if source == 'data':
                assert got.tobytes() == np.asarray(want, dtype=np.float64).tobytes()


def test_a_backend_initialised_again_with_other_atoms_builds_its_table_again():
    """The fold table of a group name belongs to one atom shape: the backend keys it on both, so after a second
    initialize() with larger atoms the kernel is handed a table of the geometry it is called with.  'data' patches of rows
    wholly inside the sample are a permutation of V: equal to the host path in every bit."""
    from tnmf_amd import patches_host as ph
    from tnmf_amd.backends.HIP import HIP_Backend
    rng = np.random.default_rng(72)
    np.random.seed(0)
    be = HIP_Backend(reconstruction_mode='valid')
    for A in ((3, 3), (6, 6), (4, 4)):
        V = rng.random((2, 1, 20, 22)).astype(np.float32)
        W, _ = be.initialize(V, A, 4, None, (-2, -1))
        K = 12
        sample, plane = rng.integers(2, size=K), rng.integers(4, size=K)
        shift = np.stack([rng.integers(A[0] - 1, 20, size=K), rng.integers(A[1] - 1, 22, size=K)], axis=1)
        h = (rng.random(K) + 0.5).astype(np.float32)
        got = be.event_patches(V, W, sample, plane, shift, h, 'data', 'rot90', 'atom')
        table = be._fold_table('rot90')
        assert table[0].numel() == 4 * A[0] * A[1] + 1 and got.shape == (K, 1) + A
        want = ph.event_patches_numpy(W.cpu().numpy(), (20, 22), 2, 'valid', sample, plane, shift, h, V, 'data', 'rot90', 'atom')
        print(f'atoms {A}: largest difference to the host path {np.abs(got - want).max():.3g} (bound 0: a permutation of V)')
        assert got.tobytes() == want.tobytes() and np.abs(want).max() > 0
    assert len(be._fold_tables) == 3


def test_duplicate_rows_have_the_same_patch():
    rows, h, _, _, _ = case('circular-2d')
    _, got = call_patches('circular-2d', 'cleaned', None, 'f64')
    full = np.column_stack([rows.astype(np.float64), h])
    _, first, inverse, counts = np.unique(full, axis=0, return_index=True, return_inverse=True, return_counts=True)
    assert counts.max() >= 2 and np.array_equal(got, got[first][inverse.reshape(-1)])


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', ['reflect-2d', 'c3-5x5'])
def test_the_identities_with_the_gain_and_the_landscape(name, dt):
    """<W_eff[p], x_e> on the device's own patches (the products summed on the host in extended precision) against the
    device's own scores: for 'residual' the a_e of tnmf_hip_events_gain -- gain is h a + h^2 b / 2 against the R it is given,
    so a = 2 gain(h = 1) - gain(h = 2) / 2 -- and for 'cleaned' a_out[e, delta = 0] of tnmf_hip_events_landscape.  Bound:
    taps U sum |w x| for the patch (c <= 9 <= taps roundings per element) plus the bar those entries are held to, 8 taps 2^-52
    of their own mag (tests/test_hip_events_gain.py, tests/test_hip_events_landscape.py)."""
    N, C, P, D, A, mode, _ = pd.PATCH_CASES[name]
    rows, h, W, V, R = case(name)
    good = pref.in_range(rows, N, P, pref.shift_shape(D, A, mode))
    taps = C * int(np.prod(A))
    lib, ctx = context()
    K = len(rows)
    g = _lib.make_geom(N, P, C, D, A, DTYPES.index(dt))
    Wd, hd, Vd, Rd, ev = dev(W, dt), dev(h, dt), dev(V, dt), dev(R, dt), events_of(rows, len(D))
    Wp = np.where(good[:, None], W[np.clip(rows[:, 1], 0, P - 1)].reshape(K, -1), 0.).astype(pref.LD)
    bar = 8 * taps * 2. ** -52

    def dots(source):
        code, x = call_patches(name, source, None, dt)
        assert code == 0
        x = x.reshape(K, -1).astype(pref.LD)
        return np.sum(Wp * x, axis=1), np.sum(np.abs(Wp * x), axis=1)

    # 'residual' against the gain at strengths 1 and 2
    gains, mags = [], []
    for strength in (1., 2.):
        gain = torch.full((K,), float('nan'), dtype=torch.float64, device='cuda')
        mag = torch.full((K,), float('nan'), dtype=torch.float64, device='cuda')
        hs = dev(np.full(K, strength), dt)
        assert lib.tnmf_hip_events_gain(ctx, ctypes.byref(g), _lib.MODES[mode], p(Wd), p(ev), p(hs), K, p(Vd), p(Rd), p(gain),
                                        p(mag), None) == 0
        torch.cuda.synchronize()
        gains.append(gain.cpu().numpy())
        mags.append(mag.cpu().numpy())
    a_gain = 2. * gains[0] - 0.5 * gains[1]
    dot, scale = dots('residual')
    bound = taps * U * scale + bar * (2. * mags[0] + 0.5 * mags[1]) + U * (2. * np.abs(gains[0]) + 0.5 * np.abs(gains[1]))
    err = np.abs(dot - a_gain).astype(np.float64)
    print(f'{name} {dt}: |<W, x_residual> - a of the gain| / bound {np.max(err[good] / bound[good].astype(np.float64)):.3g}')
    assert np.all(err <= bound) and np.abs(a_gain[good]).max() > 0 and not dot[~good].any()
    # 'cleaned' against the landscape at the centre
    nb = 3 ** len(D)
    a, b, mag = (torch.full((K, nb), float('nan'), dtype=torch.float64, device='cuda') for _ in range(3))
    assert lib.tnmf_hip_events_landscape(ctx, ctypes.byref(g), _lib.MODES[mode], p(Wd), p(ev), p(hd), K, p(Vd), p(Rd), p(a),
                                         p(b), p(mag), None) == 0
    torch.cuda.synchronize()
    a0, m0 = a.cpu().numpy()[:, nb // 2], mag.cpu().numpy()[:, nb // 2]
    dot, scale = dots('cleaned')
    bound = taps * U * scale + bar * m0
    err = np.abs(dot - a0).astype(np.float64)
    print(f'{name} {dt}: |<W, x_cleaned> - a_out of the landscape| / bound '
          f'{np.max(err[good] / bound[good].astype(np.float64)):.3g}')
    assert np.all(err <= bound) and np.abs(a0[good]).max() > 0


def test_refused_patches_write_nothing():
    name = 'c3-5x5'
    N, C, P, D, A, mode, _ = pd.PATCH_CASES[name]
    rows, h, W, V, R = case(name)
    lib, ctx = context()
    K = len(rows)
    Wd, hd, Vd, Rd, ev = dev(W, 'f32'), dev(h, 'f32'), dev(V, 'f32'), dev(R, 'f32'), events_of(rows, 2)
    ptr, src, w, T = device_table('rot90', A)
    out = torch.full((K, C) + A, SENTINEL, dtype=torch.float64, device='cuda')
    E_NULL, E_DTYPE = -1, -3

    def geom(**kw):
        g = _lib.make_geom(N, P, C, D, A, 0)
        for key, val in kw.items():
            setattr(g, key, val)
        return ctypes.byref(g)

    def patches(g, m=_lib.MODES[mode], source=2, W_=Wd, ev_=ev, st=hd, k_=K, V_=Vd, R_=Rd, fp=ptr, fs=src, fw=w, T_=T, o=out,
                c=ctx):
        return lib.tnmf_hip_events_patches(c, g, m, source, p(W_), p(ev_), p(st), k_, p(V_), p(R_), p(fp), p(fs), p(fw), T_,
                                           p(o), None)

    assert patches(geom(), c=None) == E_NULL and patches(None) == E_NULL
    for kw in (dict(W_=None), dict(ev_=None), dict(st=None), dict(V_=None), dict(R_=None), dict(o=None), dict(fs=None),
               dict(fw=None), dict(source=1, R_=None)):
        assert patches(geom(), **kw) == E_NULL, kw
    assert patches(geom(dtype=2)) == E_DTYPE and patches(geom(dtype=-1)) == E_DTYPE
    assert patches(geom(ndim=3)) == _lib.E_UNSUPPORTED
    assert patches(geom(), k_=2 ** 31) == _lib.E_UNSUPPORTED
    assert patches(geom(), k_=(2 ** 31 - 1) // (C * 25) + 1) == _lib.E_UNSUPPORTED      # n_events * C * prod(A) > 2^31 - 1
    for kw in (dict(ndim=0), dict(ndim=4), dict(N=-1), dict(M=0), dict(C=0)):
        assert patches(geom(**kw)) == _lib.E_GEOM, kw
    assert patches(geom(), m=4) == _lib.E_GEOM and patches(geom(), m=-1) == _lib.E_GEOM and patches(geom(), k_=-1) == _lib.E_GEOM
    assert patches(geom(), source=3) == _lib.E_GEOM and patches(geom(), source=-1) == _lib.E_GEOM
    assert patches(geom(), T_=0) == _lib.E_GEOM and patches(geom(), T_=3) == _lib.E_GEOM   # T < 1, M % T != 0
    g = _lib.make_geom(N, P, 83, D, A, 0)                            # 83 * 25 = 2075 doubles: beyond a wave's share of the LDS
    assert patches(ctypes.byref(g)) == _lib.E_GEOM
    g = _lib.make_geom(N, P, C, (2, 14), A, 0)                       # circular: more than one wrap
    assert patches(ctypes.byref(g)) == _lib.E_GEOM
    # nothing to do: OK, and nothing written -- with every operand NULL as well
    assert patches(geom(), k_=0) == 0 and patches(geom(N=0)) == 0
    assert patches(geom(), k_=0, W_=None, ev_=None, st=None, V_=None, R_=None, fp=None, fs=None, fw=None, o=None) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(out == SENTINEL))
    # 'data' needs neither R nor W_eff nor the strengths; and the call they were all one step from
    assert patches(geom(), source=0, R_=None, W_=None, st=None) == 0
    torch.cuda.synchronize()
    assert not bool(torch.any(out == SENTINEL))
    out.fill_(SENTINEL)
    assert patches(geom()) == 0
    torch.cuda.synchronize()
    assert not bool(torch.any(out == SENTINEL))


# -- 2. tnmf_hip_patch_moments -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def moment_case(D):
    """-> (Y [n, D] in list order, h, atom of every row, by_atom, atom_start): the runs of patches_dispatch.MOMENT_RUNS in a
    shuffled list; for D = 25 one entry of by_atom is out of range."""
    rng = np.random.default_rng(D)
    atom = np.repeat(np.arange(len(pd.MOMENT_RUNS)), pd.MOMENT_RUNS)[rng.permutation(sum(pd.MOMENT_RUNS))]
    Y, h = rng.standard_normal((len(atom), D)), rng.random(len(atom)) + 0.5
    by_atom = np.argsort(atom, kind='stable').astype(np.int32)
    start = np.searchsorted(atom[by_atom], np.arange(len(pd.MOMENT_RUNS) + 1)).astype(np.int32)
    return Y, h, atom, by_atom, start


def call_moments(D, Y, h, by_atom, start, accumulate=False, out=None, fill=float('nan')):
    lib, ctx = context()
    M = len(start) - 1
    if out is None:
        out = tuple(torch.full(shape, fill, dtype=torch.float64, device='cuda') for shape in ((M, D, D), (M, D), (M,), (M,)))
    Yd, hd = torch.from_numpy(np.ascontiguousarray(Y)).cuda(), torch.from_numpy(np.ascontiguousarray(h)).cuda()
    ba, st = torch.from_numpy(np.ascontiguousarray(by_atom)).cuda(), torch.from_numpy(np.ascontiguousarray(start)).cuda()
    code = lib.tnmf_hip_patch_moments(ctx, D, M, p(Yd), p(hd), p(ba), p(st), len(by_atom), int(accumulate), *map(p, out), None)
    torch.cuda.synchronize()
    return code, out


def chunked(D, cut):
    """The sorted list of moment_case(D) in two calls, cut at sorted position ``cut``."""
    Y, h, atom, by_atom, start = moment_case(D)
    Ys, hs = Y[by_atom], h[by_atom]
    out = None
    for r0, r1 in ((0, cut), (cut, len(Ys))):
        code, out = call_moments(D, Ys[r0:r1], hs[r0:r1], np.arange(r1 - r0, dtype=np.int32),
                                 np.clip(start - r0, 0, r1 - r0).astype(np.int32), accumulate=r0 > 0, out=out)
        assert code == 0
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize('D', pd.MOMENT_D)
def test_moments_against_the_reference(D):
    """|S - S_ref| <= (K_m + 2) U sum |y_i y_j| and |g - g_ref| <= (K_m + 2) U sum h |y_i|: K_m products and K_m additions
    (the first to the zero the accumulator starts from), in whatever order the matrix core adds the four of one
    instruction.  The chunking contract: a list cut at a multiple of four of the sorted position gives, with accumulate,
    the BITS of the same list in one call -- S, g, s2 and count; any other cut gives the bits of g, s2 and count and S within
    the bound."""
    Y, h, atom, by_atom, start = moment_case(D)
    M, Km = len(pd.MOMENT_RUNS), np.array(pd.MOMENT_RUNS, dtype=np.float64)
    bad = None
    if D == 25:   # an entry out of range: fed as zeros, still counted
        by_atom = by_atom.copy()
        bad = int(start[3]) + 5
        atom = atom.copy()
        atom[by_atom[bad]] = -1
        by_atom[bad] = len(Y) + 3
    code, out = call_moments(D, Y, h, by_atom, start)
    assert code == 0
    S, g, s2, count = [t.cpu().numpy() for t in out]
    assert not any(np.isnan(x).any() for x in (S, g, s2, count)), 'every element is written'
    rS, rg, rs2, _, Sm, gm = pref.moments(Y, h, atom, M)
    eS, eg = np.abs(S - rS), np.abs(g - rg)
    bS, bg = (Km + 2)[:, None, None] * U * Sm, (Km + 2)[:, None] * U * gm
    print(f'D {D}: |S - ref| / bound {np.max(eS[bS > 0] / bS[bS > 0]):.3g}, |g - ref| / bound {np.max(eg[bg > 0] / bg[bg > 0]):.3g}')
    assert np.all(eS <= bS) and np.all(eg <= bg) and np.all(np.abs(s2 - rs2) <= (Km + 2) * U * rs2)
    assert np.array_equal(count, Km)
    assert S.tobytes() == np.ascontiguousarray(S.transpose(0, 2, 1)).tobytes(), 'symmetric to the bit'
    for m in np.flatnonzero(Km == 0):
        assert not S[m].any() and not g[m].any() and s2[m] == 0 and count[m] == 0
    code2, out2 = call_moments(D, Y, h, by_atom, start, fill=SENTINEL)
    assert code2 == 0 and all(a.cpu().numpy().tobytes() == b.tobytes() for a, b in zip(out2, (S, g, s2, count)))
    if bad is not None:
        return
    # the same list sorted, in one call and in two
    whole = chunked(D, len(Y))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, (S, g, s2, count))), 'by_atom is only an indirection'
    aligned = chunked(D, pd.SEGMENT)
    assert pd.SEGMENT % pd.DEPTH == 0 and start[3] < pd.SEGMENT < start[4], 'the cut goes through the long run'
    assert all(a.tobytes() == b.tobytes() for a, b in zip(aligned, (S, g, s2, count)))
    other = chunked(D, pd.SEGMENT - 30 - 1)
    assert (pd.SEGMENT - 31) % pd.DEPTH and all(a.tobytes() == b.tobytes() for a, b in zip(other[1:], (g, s2, count)))
    assert np.all(np.abs(other[0] - rS) <= bS)


def test_refused_moments_write_nothing():
    D = 16
    Y, h, atom, by_atom, start = moment_case(D)
    lib, ctx = context()
    M = len(start) - 1
    out = tuple(torch.full(shape, SENTINEL, dtype=torch.float64, device='cuda') for shape in ((M, D, D), (M, D), (M,), (M,)))
    Yd, hd = torch.from_numpy(Y).cuda(), torch.from_numpy(h).cuda()
    ba, st = torch.from_numpy(by_atom).cuda(), torch.from_numpy(start).cuda()

    def moments(c=ctx, D_=D, M_=M, Y_=Yd, h_=hd, ba_=ba, st_=st, n=len(Y), o=out):
        return lib.tnmf_hip_patch_moments(c, D_, M_, p(Y_), p(h_), p(ba_), p(st_), n, 0, *map(p, o), None)

    assert moments(c=None) == -1
    for kw in (dict(Y_=None), dict(h_=None), dict(ba_=None), dict(st_=None)):
        assert moments(**kw) == -1, kw
    for i in range(4):
        assert moments(o=out[:i] + (None,) + out[i + 1:]) == -1
    assert moments(D_=0) == _lib.E_GEOM and moments(M_=0) == _lib.E_GEOM and moments(n=-1) == _lib.E_GEOM
    assert moments(D_=46341, M_=1) == _lib.E_UNSUPPORTED and moments(D_=1024, M_=2048) == _lib.E_UNSUPPORTED
    assert moments(n=2 ** 31) == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == SENTINEL)) for t in out)
    assert moments(n=0, Y_=None, h_=None, ba_=None) == 0            # no rows: the zeros are written
    torch.cuda.synchronize()
    assert all(not bool(t.any()) for t in out)


# -- 3. the front end ------------------------------------------------------------------------------------------------------------
def hip_planted(transforms, dt):
    return planted_model(transforms, backend='hip', dtype=NP[dt], to_backend=lambda a: torch.from_numpy(a).cuda())


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('transforms', [None, 'rot90'])
def test_the_planted_problem(transforms, dt):
    """The closed form and the bounds of test_patches_cpu.check_planted (derived there), with the element type's rounding."""
    nmf, det, pl = hip_planted(transforms, dt)
    assert np.array_equal(nmf.W[0, 0].astype(np.float64), pl['W0'])
    patches, mom = check_planted(nmf, det, pl, 2. ** (-24 if dt == 'f32' else -53), transforms)
    # the moments are additive: two halves of det sum to det, within the summation bound
    halves = [dataclasses.replace(det, **{f.name: getattr(det, f.name)[sel] for f in dataclasses.fields(Detections)})
              for sel in (slice(0, 11), slice(11, None))]
    parts = [nmf.atom_patch_moments(half) for half in halves]
    y = np.abs(patches.reshape(K0, -1))
    bounds = ((K0 + 2) * U * y.T @ y, (K0 + 2) * U * pl['h'] @ y, (K0 + 2) * U * np.sum(pl['h'] ** 2), 0.)
    check_additive(f'planted {transforms} {dt}', mom, parts, bounds)
    # a list of several chunks (the rows six times over; 'data', which no other row touches): the chunk length does not
    # change a bit
    many = dataclasses.replace(det, **{f.name: np.concatenate([getattr(det, f.name)] * 6)
                                       for f in dataclasses.fields(Detections)})
    assert len(many) > 2 * _lib.EVENT_SEGMENT and nmf._backend.patch_chunk_rows(100) == _lib.EVENT_SEGMENT
    default = nmf.atom_patch_moments(many, source='data')
    short = nmf.atom_patch_moments(many, source='data', max_rows=_lib.EVENT_SEGMENT)
    print(f'planted {transforms} {dt}: {len(many)} rows in chunks of {_lib.EVENT_SEGMENT} against one chunk, largest '
          f'difference {max(float(np.max(np.abs(a - b))) for a, b in zip(default, short)):.3g} (bound 0: the same bits)')
    for a, b in zip(default, short):
        assert a.tobytes() == b.tobytes()
    for got, want in zip(modes_from_moments(*default, 2), nmf.atom_modes(many, n_modes=2, source='data')):
        np.testing.assert_array_equal(got, want.reshape(got.shape))
    np.testing.assert_allclose(default[0], 6. * mom[0], rtol=1e-13)


def test_a_fitted_model_matches_the_reference():
    """detection_patches and atom_patch_moments of a fitted rot90 model in 'reflect' mode against the reference on the
    device's own render of the same rows -- bounds as in test_patches_against_the_definition and
    test_moments_against_the_reference."""
    V = np.random.default_rng(61).random((3, 1, 20, 22)).astype(np.float32)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(4, 4), backend='hip', transforms='rot90', reconstruction_mode='reflect')
    nmf.fit(V, n_iterations=5, sparsity_H=0.1)
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.97)), min_distance=1)
    assert len(det) > 20 and len(set(det.transform.tolist())) > 1
    W = np.asarray(nmf.transformed_atoms, dtype=np.float64).reshape((-1,) + nmf.W.shape[1:])
    rows = np.column_stack([det.sample, det.atom * 4 + det.transform, det.shift])
    h = det.strength.astype(np.float64)
    R = nmf.reconstruct_detections(det).astype(np.float64)
    for source in pref.SOURCES:
        x, mag, _ = pref.patches(V.astype(np.float64), R, W, 'reflect', rows, h, source)
        y, by = pref.fold(x, pref.ROUNDINGS[source] * U * mag, rows[:, 1], table_of('rot90', (4, 4)))
        got = nmf.detection_patches(det, source=source)
        print(f'fitted {source}: {len(det)} rows, largest error / bound {np.max(np.abs(got - y)[by > 0] / by[by > 0]):.3g}')
        assert np.all(np.abs(got - y) <= by) and np.abs(y).max() > 0
        image = nmf.detection_patches(det, source=source, frame='image')
        bx = pref.ROUNDINGS[source] * U * mag
        print(f'fitted {source}, image frame: largest error / bound {np.max(np.abs(image - x)[bx > 0] / bx[bx > 0]):.3g}')
        assert np.all(np.abs(image - x) <= bx)
    S, g, s2, count = nmf.atom_patch_moments(det)
    rS, rg, rs2, rcount, Sm, gm = pref.moments(got, h, det.atom, 2)
    Km = rcount[:, None, None]
    bS, bg, bs = (Km + 2) * U * Sm, (Km[:, 0] + 2) * U * gm, (rcount + 2) * U * rs2
    print(f'fitted moments: rows per atom {rcount.tolist()}, |S - ref| / bound {np.max(np.abs(S - rS)[bS > 0] / bS[bS > 0]):.3g}, '
          f'|g - ref| / bound {np.max(np.abs(g - rg)[bg > 0] / bg[bg > 0]):.3g}, |s2 - ref| / bound '
          f'{np.max(np.abs(s2 - rs2)[bs > 0] / bs[bs > 0]):.3g}')
    assert np.array_equal(count, rcount) and np.all(np.abs(S - rS) <= bS)
    assert np.all(np.abs(g - rg) <= bg) and np.all(np.abs(s2 - rs2) <= bs)


def test_the_refusals_are_those_of_the_list_operations():
    nmf, det, _ = hip_planted(None, 'f32')
    calls = (lambda m, d: m.detection_patches(d), lambda m, d: m.atom_patch_moments(d), lambda m, d: m.atom_modes(d))
    unfitted = TransformInvariantNMF(n_atoms=1, atom_shape=(5, 5), backend='hip')
    V = np.random.default_rng(62).random((2, 1, 12, 14)).astype(np.float32) + 0.1
    np.random.seed(42)
    beta = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend='hip', beta_loss=1.)
    beta.fit(V, n_iterations=2)
    np.random.seed(42)
    weighted = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend='hip')
    weighted.fit(V, n_iterations=2, weights=np.ones((2, 1, 1, 1), dtype=np.float32))
    np.random.seed(42)
    vol = TransformInvariantNMF(n_atoms=1, atom_shape=(2, 2, 2), backend='hip')
    vol.fit(np.random.default_rng(63).random((1, 1, 5, 5, 5)).astype(np.float32), n_iterations=1)
    for call in calls:
        with pytest.raises(RuntimeError):
            call(unfitted, det)
        for model in (beta, weighted, vol):
            with pytest.raises(NotImplementedError):
                call(model, model.detections(threshold=float(np.quantile(model.H, 0.9))))
    with pytest.raises(NotImplementedError):                        # ... nor does the backend take the weights
        weighted._backend.event_patches(None, weighted._W, [0], [0], [[3, 3]], [1.])
    none = dataclasses.replace(det, **{f.name: getattr(det, f.name)[:0] for f in dataclasses.fields(Detections)})
    assert nmf.detection_patches(none).shape == (0, 1, 5, 5)
    S, g, s2, count = nmf.atom_patch_moments(none)
    assert S.shape == (1, 25, 25) and not S.any() and not g.any() and not s2.any() and not count.any()
