"""
The activation correlogram on the GPU: tnmf_hip_activation_correlogram through the C ABI on activations made on the host, and
the front end on ``backend='hip'``.

Exactness: H with integer values 0..7 and about 70 % zeros -- every product and every sum is an integer below 2^53, so every
entry must equal the int64 reference bit for bit, whatever the order of the additions.  Bounded error: random non-negative H;
every entry within the bar of tests/correlogram_reference.py, 4 n 2^-53 C with n the (sample, pixel) terms of the entry and no
absolute term, of the float64 reference.  Every such test prints the largest ratio of an error to its bar.

The shapes are those of tests/correlogram_dispatch.py: the smallest that reach every branch of the kernel.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import correlogram_dispatch as cd
import correlogram_reference as cref
from tnmf_amd import _lib
from tnmf_amd.backends.HIP import HIP_Backend
from tnmf_amd.correlogram_host import activation_correlogram_numpy, cooccurrence
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

pytestmark = pytest.mark.gpu

NP = {'f32': np.float32, 'f64': np.float64}
DTYPES = ['f32', 'f64']
PATTERN = -12345.5


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def context():
    be = HIP_Backend()
    return be._lib, be._ctx, be


@functools.lru_cache(maxsize=None)
def activations(name, kind):
    """-> H [N, P, *S] float64, read-only, holding values every element type holds exactly ('int': 0..7, about 70 % zeros)
    or values of float32 ('real': random, 40 % zeros, one dead plane where there are three or more)."""
    N, P, S, _ = cd.MATRIX[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if kind == 'int':
        H = rng.integers(1, 8, (N, P) + S) * (rng.random((N, P) + S) < 0.3)
    else:
        H = rng.random((N, P) + S) * (rng.random((N, P) + S) > 0.4)
        if P >= 3:
            H[:, P - 2] = 0.
    H = H.astype(np.float32).astype(np.float64)
    H.setflags(write=False)
    return H


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """The per-sample correlogram of activations(name, kind): int64 for 'int', float64 for 'real'; read-only."""
    H, L = activations(name, kind), cd.MATRIX[name][3]
    C = cref.exact_int64(H, L, True) if kind == 'int' else activation_correlogram_numpy(H, L, True)
    C.setflags(write=False)
    return C


def on_device(H, dt, stride=None):
    """(tensor, row stride for the geometry): C-contiguous, or rows `stride` elements apart with NaN in the pad columns."""
    if stride is None:
        return torch.from_numpy(np.array(H, dtype=NP[dt])).cuda(), 0
    buf = np.full(H.shape[:-1] + (stride,), np.nan, dtype=NP[dt])
    buf[..., :H.shape[-1]] = H
    return torch.from_numpy(buf).cuda(), stride


def call(H, dt, L, per_sample, stride=None, ndim=None, dtype_code=None, null=None, geom_stride=None):
    """-> (code, C on the host) of one call on an output filled with PATTERN."""
    lib, ctx, _ = context()
    N, P, S = H.shape[0], H.shape[1], H.shape[2:]
    Hd, ld = on_device(H, dt, stride)
    out = torch.full(((N,) if per_sample else ()) + (P, P) + tuple(2 * max(x, 0) + 1 for x in L), PATTERN,
                     dtype=torch.float64, device='cuda')
    g = _lib.make_geom(N, P, 1, S, (1,) * len(S), DTYPES.index(dt), ld if geom_stride is None else geom_stride)
    if ndim is not None:
        g.ndim = ndim
    if dtype_code is not None:
        g.dtype = dtype_code
    lags = (ctypes.c_int * 3)(*L)
    code = lib.tnmf_hip_activation_correlogram(ctx, ctypes.byref(g), None if null == 'H' else p(Hd),
                                               None if null == 'max_lag' else lags, int(per_sample),
                                               None if null == 'C' else p(out), None)
    torch.cuda.synchronize()
    return code, out.cpu().numpy()


def mirror_of(C, n_lag_axes):
    axes = list(range(C.ndim))
    a = C.ndim - n_lag_axes - 2
    axes[a], axes[a + 1] = axes[a + 1], axes[a]
    flip = (slice(None),) * (a + 2) + (slice(None, None, -1),) * n_lag_axes
    return np.ascontiguousarray(C.transpose(axes)[flip])


def judge(what, C, ref, S, L, n_samples):
    assert np.all(np.isfinite(C)) and not np.any(C == PATTERN)
    ratio = cref.within_bar(C, ref, S, L, n_samples)
    print(f'correlogram {what}: largest error / bar {ratio:.3f}')
    assert ratio <= 1., (what, ratio)
    assert C.tobytes() == mirror_of(C, len(S)).tobytes()   # C[p, q, D] and C[q, p, -D]: the same bits


# -- 1. the kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('per_sample', [False, True], ids=['summed', 'per-sample'])
@pytest.mark.parametrize('name', list(cd.MATRIX))
def test_integer_activations_give_the_int64_sums_bit_for_bit(name, per_sample, dt):
    H, L = activations(name, 'int'), cd.MATRIX[name][3]
    ref = reference(name, 'int')
    ref = ref if per_sample else ref.sum(axis=0)
    code, C = call(H, dt, L, per_sample)
    assert code == 0
    assert C.tobytes() == ref.astype(np.float64).tobytes()
    for k, (s, x) in enumerate(zip(H.shape[2:], L)):   # lags at or beyond the extent: exact zeros
        lag = np.abs(np.arange(-x, x + 1))
        assert np.all(np.compress(lag >= s, C, axis=C.ndim - len(L) + k) == 0)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('per_sample', [False, True], ids=['summed', 'per-sample'])
@pytest.mark.parametrize('name', list(cd.MATRIX))
def test_random_activations_are_within_the_bar(name, per_sample, dt):
    H, L = activations(name, 'real'), cd.MATRIX[name][3]
    ref = reference(name, 'real')
    ref = ref if per_sample else ref.sum(axis=0)
    code, C = call(H, dt, L, per_sample)
    assert code == 0
    judge(f'{name} {dt} {"per sample" if per_sample else "summed"}', C, ref, H.shape[2:], L, 1 if per_sample else H.shape[0])
    again = call(H, dt, L, per_sample)[1]
    assert C.tobytes() == again.tobytes()   # the same bits run after run


STRIDED = [('1d-70-lag-0', 96), ('1d-70-lag-5', 96), ('1d-70-lag-69', 96), ('1d-70-lag-200', 96),
           ('2d-19x37-lag-0-0', 64), ('2d-19x37-lag-3-0', 64), ('2d-19x37-lag-0-4', 64), ('2d-19x37-lag-11-11', 64),
           ('2d-19x37-lag-18-36', 64), ('2d-19x37-lag-31-31', 64), ('2d-5x65', 66), ('1d-257', 258)]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name,stride', STRIDED)
def test_pad_columns_filled_with_NaN_are_never_read(name, stride, dt):
    H, L = activations(name, 'real'), cd.MATRIX[name][3]
    code, plain = call(H, dt, L, True)
    assert code == 0
    code, C = call(H, dt, L, True, stride=stride)
    assert code == 0 and np.all(np.isfinite(C))
    assert C.tobytes() == plain.tobytes()
    judge(f'{name} {dt} stride {stride}', C, reference(name, 'real'), H.shape[2:], L, 1)


def test_a_placement_is_told_from_its_transpose():
    """One spike per plane: C[p, q, D] is 1 exactly where D is the offset from p's spike to q's -- an asymmetric pattern that a
    swap of rows and columns, of the operands or of the sign of a lag would move."""
    P, S, L = 20, (9, 21), (5, 9)
    rng = np.random.default_rng(0)
    at = np.stack([rng.integers(2, 7, P), rng.integers(6, 15, P)], axis=1)
    H = np.zeros((1, P) + S)
    H[0, np.arange(P), at[:, 0], at[:, 1]] = 1.
    for dt in DTYPES:
        code, C = call(H, dt, L, False)
        assert code == 0
        want = np.zeros_like(C)
        for a in range(P):
            for b in range(P):
                d = at[b] - at[a]
                if abs(d[0]) <= L[0] and abs(d[1]) <= L[1]:
                    want[a, b, d[0] + L[0], d[1] + L[1]] = 1.
        np.testing.assert_array_equal(C, want)


def test_no_sample_gives_zeros_and_one_plane_works():
    code, C = call(np.zeros((0, 3, 5, 6)), 'f32', (1, 2), False, null='H')
    assert code == 0 and C.shape == (3, 3, 3, 5) and np.all(C == 0)
    H = np.arange(1., 7.).reshape(1, 1, 6)
    code, C = call(H, 'f64', (2,), False)
    assert code == 0 and np.array_equal(C[0, 0], [50., 70., 91., 70., 50.])


# -- 2. refusals: the code, and nothing written --------------------------------------------------------------------------------------
REFUSALS = {
    'ndim-3': (dict(ndim=3), _lib.E_UNSUPPORTED),
    'negative-lag': (dict(L=(1, -1)), _lib.E_GEOM),
    'lag-beyond-the-limit-2d': (dict(L=(cd.MAX_LAG[2] + 1, 0)), _lib.E_UNSUPPORTED),
    'lag-beyond-the-limit-2d-x': (dict(L=(0, cd.MAX_LAG[2] + 1)), _lib.E_UNSUPPORTED),
    'null-H': (dict(null='H'), -1),
    'null-max-lag': (dict(null='max_lag'), -1),
    'null-C': (dict(null='C'), -1),
    'dtype-code': (dict(dtype_code=2), -3),
    'stride-below-the-width': (dict(geom_stride=5), _lib.E_GEOM),
    'ndim-0': (dict(ndim=0), _lib.E_GEOM),
}


@pytest.mark.parametrize('name', list(REFUSALS))
def test_refusals_answer_their_code_and_write_nothing(name):
    kw, want = REFUSALS[name]
    kw = dict(kw)
    L = kw.pop('L', (1, 2))
    H = activations('2d-planes-16', 'int')[:, :3, :4, :6]
    code, C = call(H, 'f32', L, False, **kw)
    assert code == want
    assert np.all(C == PATTERN)


def test_refusals_on_one_shift_axis():
    H = activations('1d-70-lag-5', 'int')
    for L, want in (((cd.MAX_LAG[1] + 1,), _lib.E_UNSUPPORTED), ((-1,), _lib.E_GEOM)):
        code, C = call(H, 'f64', L, True)
        assert code == want and np.all(C == PATTERN)
    code, C = call(H, 'f64', (cd.MAX_LAG[1],), False)   # the limit itself is served
    assert code == 0 and C.tobytes() == reference_at_limit().tobytes()


@functools.lru_cache(maxsize=None)
def reference_at_limit():
    return cref.exact_int64(activations('1d-70-lag-5', 'int'), (cd.MAX_LAG[1],)).astype(np.float64)


def test_the_backend_refuses_volumes_and_names_the_limit():
    np.random.seed(0)
    be = HIP_Backend()
    W, H = be.initialize(np.ones((1, 1, 5, 5, 5)), (2, 2, 2), 2, None, (-3, -2, -1))
    with pytest.raises(NotImplementedError, match='activation correlogram: 1 or 2 shift axes only'):
        be.activation_correlogram(H, (1, 1, 1))
    be = HIP_Backend()
    W, H = be.initialize(np.ones((1, 1, 9, 9)), (2, 2), 2, None, (-2, -1))
    with pytest.raises(NotImplementedError, match=f'beyond the limit of {cd.MAX_LAG[2]} per axis'):
        be.activation_correlogram(H, (cd.MAX_LAG[2] + 1, 0))


# -- 3. the front end ----------------------------------------------------------------------------------------------------------------
def fitted_hip(shape_V, M, A, mode='valid', transforms=None, seed=0, dtype=np.float32, n_iterations=3):
    V = (np.random.default_rng(seed).random(shape_V) + 0.05).astype(dtype)
    np.random.seed(42)
    hip = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip', reconstruction_mode=mode, transforms=transforms)
    hip.fit(V, n_iterations=n_iterations, sparsity_H=0.1)
    return hip


FRONT_END = {f'{k}d-{mode}': dict(shape_V=(3, 1, 14, 18) if k == 2 else (3, 2, 40), M=3, A=(3, 4) if k == 2 else (5,), mode=mode)
             for k in (1, 2) for mode in ('valid', 'full', 'circular', 'reflect')}
FRONT_END['rot90'] = dict(shape_V=(2, 1, 12, 12), M=2, A=(3, 3), transforms='rot90')
FRONT_END['2d-float64'] = dict(shape_V=(3, 1, 14, 18), M=3, A=(3, 4), dtype=np.float64)


@pytest.mark.parametrize('name', list(FRONT_END))
def test_front_end_on_hip_is_the_host_correlogram_of_H(name):
    nmf = fitted_hip(**FRONT_END[name])
    assert getattr(nmf._backend, 'activation_correlogram', None) is not None
    H = nmf.H
    N, k = H.shape[0], len(nmf.atom_shape)
    H = H.reshape((N, -1) + H.shape[-k:])
    P, S = H.shape[1], H.shape[2:]
    L = tuple(a - 1 for a in nmf.atom_shape)
    C = nmf.activation_correlogram()
    assert C.dtype == np.float64 and C.shape == (P, P) + tuple(2 * x + 1 for x in L)
    judge(f'front end {name}', C, activation_correlogram_numpy(H, L), S, L, N)
    wide = tuple(min(2 * a, cd.MAX_LAG[k]) for a in S)   # lags beyond the extent: zeros
    ref = activation_correlogram_numpy(H, wide, True)
    per = nmf.activation_correlogram(wide, per_sample=True)
    judge(f'front end {name} per sample', per, ref, S, wide, 1)
    nmf._shuffle_idx = np.arange(N)[::-1].copy()
    try:   # per sample in the order of nmf.H, which the shuffle permutes too
        Hs = nmf.H.reshape((N, P) + S)
        shuffled = nmf.activation_correlogram(wide, per_sample=True)
        np.testing.assert_array_equal(shuffled, per[np.argsort(nmf._shuffle_idx)])
        judge(f'front end {name} shuffled', shuffled, activation_correlogram_numpy(Hs, wide, True), S, wide, 1)
    finally:
        nmf._shuffle_idx = None
    score, lag = nmf.atom_cooccurrence()
    want = cooccurrence(C)
    np.testing.assert_array_equal(score, want[0])
    np.testing.assert_array_equal(lag, want[1])
    assert np.all((score >= 0) & (score <= 1))


def test_a_lag_beyond_the_limit_goes_through_the_host():
    nmf = fitted_hip(**FRONT_END['2d-valid'])
    L = (cd.MAX_LAG[2] + 1, 2)
    C = nmf.activation_correlogram(L)
    np.testing.assert_array_equal(C, activation_correlogram_numpy(nmf.H, L))


def test_planted_partner_and_rhythm_on_hip():
    """Plane 1 is plane 0 moved by (2, -3); plane 2 fires every 7th column; plane 3 is dead."""
    rng = np.random.default_rng(5)
    H = np.zeros((2, 4, 40, 50), dtype=np.float32)
    for n, y, x in zip(rng.integers(0, 2, 30), rng.integers(6, 32, 30), rng.integers(8, 40, 30)):
        h = np.float32(0.5 + rng.random())
        H[n, 0, y, x] += h
        H[n, 1, y + 2, x - 3] += h
    H[:, 2, 10:30:3, 1::7] = (1. + rng.random((2, 7, 7))).astype(np.float32)
    V = (rng.random((2, 1, 38, 48)) + 0.05).astype(np.float32)
    np.random.seed(0)
    nmf = TransformInvariantNMF(n_atoms=4, atom_shape=(3, 3), backend='hip')
    nmf.fit(V, n_iterations=0)
    nmf._H[...] = torch.from_numpy(H).cuda()
    score, lag = nmf.atom_cooccurrence(max_lag=(4, 15))
    assert score[0, 1] > 0.99 and tuple(lag[0, 1]) == (2, -3) and tuple(lag[1, 0]) == (-2, 3)
    assert lag[2, 2, 0] == 0 and lag[2, 2, 1] != 0 and lag[2, 2, 1] % 7 == 0
    assert np.all(score[3] == 0) and np.all(score[:, 3] == 0)
