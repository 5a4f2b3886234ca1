"""
The triggered sums on the GPU: tnmf_hip_triggered_sums through the C ABI on operands made on the host, and the front end on
``backend='hip'``.

Exactness: H with integer values 0..7 and about 70 % zeros, Y with integers in -7..7 -- every product and every sum is an
integer below 2^53, so every entry must equal the int64 reference bit for bit, whatever the order of the additions.  Bounded
error: random non-negative H and signed Y; every entry within the bar of tests/triggered_reference.py, 4 (n + 2) 2^-53 T
with n the (sample, pixel) terms of the entry, T the sum with |Y| in the place of Y and no absolute term, of the float64
reference.  Every such test prints the largest ratio of an error to its bar.

The shapes are those of tests/triggered_dispatch.py: the issue's cases and the smallest that reach every other branch.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import triggered_dispatch as td
import triggered_reference as tref
from oracle import tnmf_oracle as orc
from tnmf_amd import _lib
from tnmf_amd.atoms_host import pad_activations_numpy
from tnmf_amd.backends.HIP import HIP_Backend
from tnmf_amd.triggered_host import extend_atoms, tap_gains_from_sums, triggered_sums_numpy, window_gains
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

pytestmark = pytest.mark.gpu

NP = {'f32': np.float32, 'f64': np.float64}
DTYPES = ['f32', 'f64']
PATTERN = -12345.5
E_NULL, E_DTYPE, E_WORKSPACE = -1, -3, -4


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def context():
    be = HIP_Backend()
    return be._lib, be._ctx, be


@functools.lru_cache(maxsize=None)
def operands(name, kind):
    """-> (Hp [N, P, *(D + A - 1)], Y [N, F, *D]) float64, read-only, holding values every element type holds exactly:
    'int' H in 0..7 with about 70 % zeros and Y in -7..7; 'real' random values of float32, H with 40 % zeros and one dead
    plane where there are three or more, Y signed."""
    N, P, F, D, A, _ = td.MATRIX[name]
    S = tuple(d + a - 1 for d, a in zip(D, A))
    rng = np.random.default_rng(sum(map(ord, name)))
    if kind == 'int':
        H = rng.integers(1, 8, (N, P) + S) * (rng.random((N, P) + S) < 0.3)
        Y = rng.integers(-7, 8, (N, F) + D)
    else:
        H = rng.random((N, P) + S) * (rng.random((N, P) + S) > 0.4)
        if P >= 3:
            H[:, P - 2] = 0.
        Y = rng.standard_normal((N, F) + D)
    H, Y = (a.astype(np.float32).astype(np.float64) for a in (H, Y))
    H.setflags(write=False)
    Y.setflags(write=False)
    return H, Y


@functools.lru_cache(maxsize=None)
def reference(name, kind, power):
    """(per-sample sums, per-sample sums with |Y|) of operands(name, kind): int64 for 'int', float64 for 'real'."""
    (H, Y), (A, m) = operands(name, kind), td.MATRIX[name][4:]
    if kind == 'int':
        X, T = tref.exact_int64(H, Y, A, m, power, True), None
    else:
        X, T = triggered_sums_numpy(H, Y, A, m, power, True), triggered_sums_numpy(H, np.abs(Y), A, m, power, True)
        T.setflags(write=False)
    X.setflags(write=False)
    return X, T


def on_device(H, dt, stride=None):
    """(tensor, row stride for the geometry): C-contiguous, or rows `stride` elements apart with NaN in the pad columns."""
    if stride is None:
        return torch.from_numpy(np.array(H, dtype=NP[dt])).cuda(), 0
    buf = np.full(H.shape[:-1] + (stride,), np.nan, dtype=NP[dt])
    buf[..., :H.shape[-1]] = H
    return torch.from_numpy(buf).cuda(), stride


def field_in_the_middle(Y, dt):
    """Y as a view in the middle of a larger NaN-filled allocation."""
    n = int(np.prod(Y.shape))
    buf = torch.full((n + 2 * 777,), float('nan'), dtype=torch.float32 if dt == 'f32' else torch.float64, device='cuda')
    view = buf[777:777 + n].view(Y.shape)
    view.copy_(torch.from_numpy(np.array(Y, dtype=NP[dt])))
    return buf, view


def call(H, Y, dt, A, m, power=1, per_sample=False, stride=None, ndim=None, dtype_code=None, null=None, geom_stride=None,
         n_fields=None, short=0, middle=False, plan_only=False, edit=None):
    """-> (code, X on the host, the work buffer on the host) of one call on an output and a work buffer filled with
    PATTERN; the work buffer has the plan's bytes less `short` (64 where the plan itself refuses).  `edit(geom)` changes the
    geometry after it is made for the operands; `null` names the argument passed as NULL."""
    lib, ctx, _ = context()
    N, P, F, D = H.shape[0], H.shape[1], Y.shape[1], Y.shape[2:]
    Hd, ld = on_device(H, dt, stride)
    keep, Yd = field_in_the_middle(Y, dt) if middle else (None, torch.from_numpy(np.array(Y, dtype=NP[dt])).cuda())
    shape = ((N,) if per_sample else ()) + (P, F) + tuple(max(a + 2 * x, 1) for a, x in zip(A, m))
    size = int(np.prod(shape))
    out = torch.full((max(size, 1),), PATTERN, dtype=torch.float64, device='cuda')   # (never a null pointer by accident)
    g = _lib.make_geom(N, P, 1, D, A, DTYPES.index(dt), ld if geom_stride is None else geom_stride)
    if ndim is not None:
        g.ndim = ndim
    if dtype_code is not None:
        g.dtype = dtype_code
    if edit is not None:
        edit(g)
    F = F if n_fields is None else n_fields
    margin = (ctypes.c_int * 3)(*m)
    need = ctypes.c_size_t(64)
    ctx, gref = None if null == 'ctx' else ctx, None if null == 'geom' else ctypes.byref(g)
    plan_code = lib.tnmf_hip_triggered_sums_plan(ctx, gref, F, None if null == 'margin' else margin,
                                                 int(per_sample), ctypes.byref(need))
    if plan_only:
        return plan_code, need.value
    nbytes = max(need.value - short, 0)
    work = torch.full((max(nbytes // 8, 1),), PATTERN, dtype=torch.float64, device='cuda')
    code = lib.tnmf_hip_triggered_sums(ctx, gref, None if null == 'H' else p(Hd), None if null == 'Y' else p(Yd),
                                       F, None if null == 'margin' else margin, power, int(per_sample),
                                       None if null == 'work' else p(work), nbytes, None if null == 'X' else p(out), None)
    torch.cuda.synchronize()
    if null in ('ctx', 'geom', 'margin'):                    # the plan refuses exactly what the call refuses
        assert plan_code == code == E_NULL
    elif null != 'work' and power in (1, 2):                 # (the plan has no power, H, Y, X or work to refuse)
        assert plan_code == (code if code not in (E_NULL, E_WORKSPACE) else 0), (plan_code, code)
    return code, out.cpu().numpy()[:size].reshape(shape), work.cpu().numpy()


def judge(what, X, ref, T, D, A, m, n_samples):
    assert np.all(np.isfinite(X)) and not np.any(X == PATTERN)
    ratio = tref.within_bar(X, ref, T, D, A, m, n_samples)
    print(f'triggered sums {what}: largest error / bar {ratio:.3f}')
    assert ratio <= 1., (what, ratio)


# -- 1. the kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('power', [1, 2])
@pytest.mark.parametrize('per_sample', [False, True], ids=['summed', 'per-sample'])
@pytest.mark.parametrize('name', list(td.MATRIX))
def test_integer_operands_give_the_int64_sums_bit_for_bit(name, per_sample, power, dt):
    (H, Y), (D, A, m) = operands(name, 'int'), td.MATRIX[name][3:]
    ref = reference(name, 'int', power)[0]
    ref = ref if per_sample else ref.sum(axis=0)
    code, X, _ = call(H, Y, dt, A, m, power, per_sample)
    assert code == 0
    assert X.tobytes() == ref.astype(np.float64).tobytes()
    print(f'triggered sums {name} {dt} power {power}: {X.size} entries bit-equal to int64')
    assert np.all(X[np.broadcast_to(tref.terms(D, A, m, 1) == 0, X.shape)] == 0)   # no term: an exact 0


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('power', [1, 2])
@pytest.mark.parametrize('per_sample', [False, True], ids=['summed', 'per-sample'])
@pytest.mark.parametrize('name', list(td.MATRIX))
def test_random_operands_are_within_the_bar(name, per_sample, power, dt):
    (H, Y), (D, A, m) = operands(name, 'real'), td.MATRIX[name][3:]
    ref, T = reference(name, 'real', power)
    N = H.shape[0]
    code, X, _ = call(H, Y, dt, A, m, power, per_sample)
    assert code == 0
    what = f'{name} {dt} power {power} {"per sample" if per_sample else "summed"}'
    if per_sample:
        judge(what, X, ref, T, D, A, m, 1)
        summed = call(H, Y, dt, A, m, power, False)[1]            # the per-sample sums added on the host
        judge(what + ' added on the host', X.sum(axis=0), summed, T.sum(axis=0), D, A, m, max(N, 1))
    else:
        judge(what, X, ref.sum(axis=0), T.sum(axis=0), D, A, m, max(N, 1))
    again = call(H, Y, dt, A, m, power, per_sample)[1]
    assert X.tobytes() == again.tobytes()   # the same bits run after run


STRIDED = [('1d-window-is-atom', 48), ('1d-window-34', 320), ('1d-window-wider-than-sample', 9), ('2d-window-is-atom', 16),
           ('2d-window-13x20', 80), ('2d-mostly-outside', 7), ('2d-5x65', 66), ('2d-chunks-y', 24)]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name,stride', STRIDED)
def test_NaN_in_pad_columns_and_around_the_field_is_never_read_and_every_element_is_written(name, stride, dt):
    (H, Y), (D, A, m) = operands(name, 'real'), td.MATRIX[name][3:]
    ref, T = reference(name, 'real', 2)
    code, plain, _ = call(H, Y, dt, A, m, 2, True)
    assert code == 0
    code, X, work = call(H, Y, dt, A, m, 2, True, stride=stride, middle=True)
    assert code == 0 and np.all(np.isfinite(X)) and not np.any(X == PATTERN)
    assert X.tobytes() == plain.tobytes()
    assert not np.any(work == PATTERN)      # every partial sum the plan counts is written
    judge(f'{name} {dt} stride {stride}', X, ref, T, D, A, m, 1)


def test_a_placement_is_told_from_its_mirror():
    """One spike per plane and one per field: X[p, f, j] is 1 exactly at the offset from p's spike to f's -- a pattern that a
    swap of the operands, of the axes or of the sign of the offset would move."""
    P, F, D, A, m = 20, 3, (9, 21), (3, 4), (4, 7)
    rng = np.random.default_rng(0)
    S = tuple(d + a - 1 for d, a in zip(D, A))
    at_h = np.stack([rng.integers(0, S[0], P), rng.integers(0, S[1], P)], axis=1)
    at_y = np.stack([rng.integers(2, 7, F), rng.integers(6, 15, F)], axis=1)
    H, Y = np.zeros((1, P) + S), np.zeros((1, F) + D)
    H[0, np.arange(P), at_h[:, 0], at_h[:, 1]] = 1.
    Y[0, np.arange(F), at_y[:, 0], at_y[:, 1]] = 1.
    want = np.zeros((P, F) + tref.window(A, m))
    for a in range(P):
        for f in range(F):
            j = at_y[f] - at_h[a] + np.asarray(A) - 1 + np.asarray(m)      # y = q - (A - 1) - m + j
            if np.all(j >= 0) and np.all(j < want.shape[2:]):
                want[a, f, j[0], j[1]] = 1.
    assert want.sum() >= 10
    for dt in DTYPES:
        code, X, _ = call(H, Y, dt, A, m)
        assert code == 0
        np.testing.assert_array_equal(X, want)


def test_no_sample_gives_zeros_and_needs_no_work_buffer():
    H, Y = np.zeros((0, 3, 11, 14)), np.zeros((0, 1, 9, 11))
    assert call(H, Y, 'f32', (3, 4), (1, 1), plan_only=True) == (0, 0)
    code, X, _ = call(H, Y, 'f32', (3, 4), (1, 1), null='H')
    assert code == 0 and X.shape == (3, 1, 5, 6) and np.all(X == 0)
    code, X, _ = call(H, Y, 'f64', (3, 4), (1, 1), per_sample=True, null='Y')
    assert code == 0 and X.size == 0


def test_the_plan_reports_the_bytes_of_the_mirror():
    for name, case in td.MATRIX.items():
        for dt in DTYPES:
            for per_sample in (False, True):
                H, Y = operands(name, 'int')
                code, need = call(H, Y, dt, case[4], case[5], per_sample=per_sample, plan_only=True)
                assert code == 0 and need == td.plan(*case, per_sample, dt)['work_bytes'], (name, dt, per_sample)


# -- 2. refusals: the code, and nothing written --------------------------------------------------------------------------------------
REFUSALS = {
    'ndim-3': (dict(ndim=3), _lib.E_UNSUPPORTED),
    'ndim-0': (dict(ndim=0), _lib.E_GEOM),
    'ndim-4': (dict(ndim=4), _lib.E_GEOM),
    'negative-margin': (dict(m=(1, -1)), _lib.E_GEOM),
    'no-field': (dict(n_fields=0), _lib.E_GEOM),
    'power-0': (dict(power=0), _lib.E_GEOM),
    'power-3': (dict(power=3), _lib.E_GEOM),
    'stride-below-the-width': (dict(geom_stride=5), _lib.E_GEOM),
    'window-beyond-the-limit-y': (dict(m=((td.MAX_WINDOW[2] - 3) // 2 + 1, 0)), _lib.E_UNSUPPORTED),
    'window-beyond-the-limit-x': (dict(m=(0, (td.MAX_WINDOW[2] - 4) // 2 + 1)), _lib.E_UNSUPPORTED),
    'null-ctx': (dict(null='ctx'), E_NULL),
    'null-geom': (dict(null='geom'), E_NULL),
    'null-H': (dict(null='H'), E_NULL),
    'null-Y': (dict(null='Y'), E_NULL),
    'null-margin': (dict(null='margin'), E_NULL),
    'null-X': (dict(null='X'), E_NULL),
    'null-work': (dict(null='work'), E_NULL),
    'dtype-code': (dict(dtype_code=2), E_DTYPE),
    'work-one-byte-short': (dict(short=1), E_WORKSPACE),
    # sizes <= 0
    'negative-N': (dict(edit=lambda g: setattr(g, 'N', -1)), _lib.E_GEOM),
    'no-plane': (dict(edit=lambda g: setattr(g, 'M', 0)), _lib.E_GEOM),
    'negative-planes': (dict(edit=lambda g: setattr(g, 'M', -3)), _lib.E_GEOM),
    'D-0': (dict(edit=lambda g: g.D.__setitem__(0, 0)), _lib.E_GEOM),
    'D-negative': (dict(edit=lambda g: g.D.__setitem__(1, -11)), _lib.E_GEOM),
    'A-0': (dict(edit=lambda g: g.A.__setitem__(1, 0)), _lib.E_GEOM),
    'A-negative': (dict(edit=lambda g: g.A.__setitem__(0, -3)), _lib.E_GEOM),
    # more than 2^31 - 1 outputs, (sample, tile) items of a sample or workgroups: the geometry alone says so, and the call
    # answers before it looks at an operand (window 5 x 8: 40 outputs a plane)
    'outputs-2^31': (dict(edit=lambda g: setattr(g, 'M', 2 ** 31 // 40 + 1)), _lib.E_UNSUPPORTED),
    'outputs-2^31-per-sample': (dict(per_sample=True, edit=lambda g: setattr(g, 'N', 2 ** 31 // 200 + 1)), _lib.E_UNSUPPORTED),
    'tiles-2^31': (dict(edit=lambda g: (g.D.__setitem__(0, 2 ** 20), g.D.__setitem__(1, 2 ** 20))), _lib.E_UNSUPPORTED),
    'extent-2^31': (dict(edit=lambda g: g.D.__setitem__(1, 2 ** 31 - 2)), _lib.E_UNSUPPORTED),
}


@pytest.mark.parametrize('name', list(REFUSALS))
def test_refusals_answer_their_code_and_write_nothing(name):
    kw, want = REFUSALS[name]
    kw = dict(kw)
    m = kw.pop('m', (1, 2))
    H, Y = operands('2d-window-is-atom', 'int')
    code, X, work = call(H, Y, 'f32', (3, 4), m, **kw)
    assert code == want
    assert np.all(X == PATTERN) and np.all(work == PATTERN)


def test_the_largest_sizes_below_the_limits_are_planned():
    """One output below 2^31 is a plan, not a refusal (the plan alone: nothing is allocated, nothing launched)."""
    H, Y = operands('2d-window-is-atom', 'int')
    P = (2 ** 31 - 1) // 40                                    # window 5 x 8: 40 outputs a plane
    code, need = call(H, Y, 'f32', (3, 4), (1, 2), plan_only=True, edit=lambda g: setattr(g, 'M', P))
    assert code == 0 and need == td.plan(2, P, 1, (9, 11), (3, 4), (1, 2), False, 'f32')['work_bytes']
    code, _ = call(H, Y, 'f32', (3, 4), (1, 2), plan_only=True, edit=lambda g: setattr(g, 'M', P + 14))
    assert code == _lib.E_UNSUPPORTED


def test_refusals_on_one_shift_axis_and_the_limits_themselves():
    H, Y = operands('1d-window-is-atom', 'int')
    for m, want in ((((td.MAX_WINDOW[1] - 5) // 2 + 1,), _lib.E_UNSUPPORTED), ((-1,), _lib.E_GEOM)):
        code, X, work = call(H, Y, 'f64', (5,), m, per_sample=True)
        assert code == want and np.all(X == PATTERN) and np.all(work == PATTERN)
    m = ((2048 - 5) // 2 + 1,)                               # a window of 2048 and more on one axis is served
    code, X, _ = call(H, Y, 'f64', (5,), m)
    assert code == 0 and X.tobytes() == tref.exact_int64(H, Y, (5,), m).astype(np.float64).tobytes()
    H, Y = operands('2d-mostly-outside', 'int')
    code, X, _ = call(H, Y, 'f32', (2, 2), (31, 31))          # and of 64 per axis on two
    assert code == 0 and X.shape[-2:] == (64, 64)
    assert X.tobytes() == tref.exact_int64(H, Y, (2, 2), (31, 31)).astype(np.float64).tobytes()


def test_the_backend_refuses_volumes_and_a_window_beyond_the_limit():
    np.random.seed(0)
    be = HIP_Backend()
    W, H = be.initialize(np.ones((1, 1, 5, 5, 5)), (2, 2, 2), 2, None, (-3, -2, -1))
    with pytest.raises(NotImplementedError, match='triggered sums: 1 or 2 shift axes only'):
        be.triggered_sums(H, be._V_dev, (1, 1, 1))
    be = HIP_Backend()
    W, H = be.initialize(np.ones((1, 1, 9, 9), dtype=np.float32), (2, 2), 2, None, (-2, -1))
    assert be.supports_triggered
    with pytest.raises(NotImplementedError, match='beyond the library\'s limit'):
        be.triggered_sums(H, be._V_dev, (td.MAX_WINDOW[2], 0))
    # the plan is asked before anything is allocated: a window no memory holds is refused like any other, not an allocation
    # that fails
    for margin in ((10 ** 6, 10 ** 6), (2 ** 40, 0)):
        with pytest.raises(NotImplementedError, match='beyond the library\'s limit'):
            be.triggered_sums(H, be._V_dev, margin, per_sample=True)


# -- 3. the front end ----------------------------------------------------------------------------------------------------------------
def fitted_hip(shape_V, M, A, mode='valid', transforms=None, seed=0, dtype=np.float32, n_iterations=3, weights=False,
               beta_loss=2.):
    rng = np.random.default_rng(seed)
    V = (rng.random(shape_V) + 0.05).astype(dtype)
    kw = dict(weights=(rng.random(shape_V) * (rng.random(shape_V) > 0.3)).astype(dtype)) if weights else {}
    np.random.seed(42)
    hip = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip', reconstruction_mode=mode, transforms=transforms,
                                beta_loss=beta_loss)
    hip.fit(V, n_iterations=n_iterations, sparsity_H=0.1, **kw)
    return hip


FRONT_END = {f'{k}d-{mode}-{np.dtype(dt).name}': dict(shape_V=(3, 1, 18, 22) if k == 2 else (3, 2, 40), M=3,
                                                      A=(4, 5) if k == 2 else (5,), mode=mode, dtype=dt)
             for k in (1, 2) for mode in ('valid', 'full', 'circular', 'reflect') for dt in (np.float32, np.float64)}
FRONT_END['rot90'] = dict(shape_V=(2, 1, 12, 12), M=2, A=(3, 3), transforms='rot90')
FRONT_END['weights'] = dict(shape_V=(3, 2, 18, 22), M=3, A=(4, 5), weights=True, mode='full')
FRONT_END['kullback-leibler'] = dict(shape_V=(3, 1, 18, 22), M=3, A=(4, 5), beta_loss='kullback-leibler')


def host_route(nmf):
    """A context in which the backend's kernel refuses, so that the front end takes its host fallback on the same W, H, V
    and the same field."""
    class Refusing:
        def __enter__(self):
            self.kept = nmf._backend.triggered_sums
            nmf._backend.triggered_sums = self.refuse

        def refuse(self, *a, **kw):
            raise NotImplementedError('the host route')

        def __exit__(self, *exc):
            del nmf._backend.triggered_sums
            assert nmf._backend.triggered_sums.__func__ is self.kept.__func__
    return Refusing()


@pytest.mark.parametrize('name', list(FRONT_END))
def test_front_end_on_hip_is_the_host_fallback_within_the_bar(name):
    nmf = fitted_hip(**FRONT_END[name])
    be = nmf._backend
    assert getattr(be, 'supports_triggered', False)
    A, D, N = tuple(nmf.atom_shape), tuple(nmf._V.shape[2:]), nmf._V.shape[0]
    frobenius = nmf._beta == 2.
    before = [np.array(nmf.W, copy=True), np.array(nmf.H, copy=True)]
    Hp = pad_activations_numpy(np.asarray(be.to_ndarray(nmf._H), dtype=np.float64), A, nmf._mode)
    fields = {s: np.asarray(be.to_ndarray(be.triggered_field(nmf._V, nmf._W_dict, nmf._H, s)), dtype=np.float64)
              for s in ('data', 'reconstruction', 'residual', 'weights')}
    margins = (None, (0,) * len(A), tuple(d + 1 for d in D))
    for margin in margins:
        m = nmf._margin(margin)
        for source in ('data', 'reconstruction', 'residual'):
            for per_sample in (False, True):
                X = nmf.activation_triggered_sums(margin, source, per_sample)
                with host_route(nmf):
                    want = nmf.activation_triggered_sums(margin, source, per_sample)
                assert X.dtype == np.float64 and X.shape == want.shape
                T = triggered_sums_numpy(Hp, np.abs(fields[source]), A, m, 1, per_sample)
                judge(f'front end {name} {source} margin {m}', X, want, T, D, A, m, 1 if per_sample else N)
        # the average, the tap gains and the window gains are the host algebra on this run's sums
        mass = be.triggered_sums(nmf._H, be.triggered_field(nmf._V, nmf._W_dict, nmf._H, 'weights'), m)
        judge(f'front end {name} mass margin {m}', mass, triggered_sums_numpy(Hp, fields['weights'], A, m),
              triggered_sums_numpy(Hp, fields['weights'], A, m), D, A, m, N)
        avg = nmf.activation_triggered_average(margin)
        with np.errstate(invalid='ignore', divide='ignore'):
            want = np.where(mass == 0, np.nan, nmf.activation_triggered_sums(margin, 'data') / mass)
        np.testing.assert_array_equal(avg, want)
        assert np.array_equal(np.isnan(avg), mass == 0)
        # ... and within the bar of the host route, carried through the quotient: X and mass are within their bars bX, bm of
        # the host's X', m', so |X / m - X' / m'| <= (bX + |X' / m'| bm) / m; m >= m' (1 - bm / m') and bm / m' < 1e-9 is the
        # factor 1 + 1e-6; the quotient itself rounds once on either side
        with host_route(nmf):
            host_avg = nmf.activation_triggered_average(margin)
        host_mass = triggered_sums_numpy(Hp, fields['weights'], A, m)
        bX = tref.bar(triggered_sums_numpy(Hp, np.abs(fields['data']), A, m), D, A, m, N)
        bm = tref.bar(host_mass, D, A, m, N)
        live = host_mass > 0
        assert np.array_equal(np.isnan(host_avg), ~live) and np.array_equal(np.isnan(avg), ~live)
        bound = (bX[live] + np.abs(host_avg[live]) * bm[live]) / host_mass[live] * (1 + 1e-6) + 4 * tref.U * np.abs(host_avg[live])
        err = np.abs(avg[live] - host_avg[live])
        assert np.all(err[bound == 0] == 0)
        ratio = float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0), initial=0.))
        print(f'triggered average front end {name} margin {m}: largest error / bar {ratio:.3f}')
        assert ratio <= 1.
        if not frobenius:
            with pytest.raises(NotImplementedError, match='Frobenius objective'):
                nmf.atom_tap_gains(margin)
            continue
        E = nmf.activation_triggered_sums(margin)
        b = be.triggered_sums(nmf._H, be.triggered_field(nmf._V, nmf._W_dict, nmf._H, 'weights'), m, power=2)
        judge(f'front end {name} b margin {m}', b, triggered_sums_numpy(Hp, fields['weights'], A, m, 2),
              triggered_sums_numpy(Hp, fields['weights'], A, m, 2), D, A, m, N)
        gain, step = nmf.atom_tap_gains(margin)
        want = tap_gains_from_sums(E, b, extend_atoms(be.to_ndarray(nmf._W_dict), m))
        np.testing.assert_array_equal(gain, want[0])
        np.testing.assert_array_equal(step, want[1])
        assert np.all(gain >= 0)
        # ... and within the bar of the host route, carried through the algebra: gain(E, b) = max over t >= -W_ext of
        # t E - t^2 b / 2, a maximum of functions linear in (E, b), so two gains differ by at most |t| bE + t^2 bb / 2 at the
        # t either side chose (bE, bb the bars of E and b); the algebra rounds a few times on terms of size |t E| and t^2 b / 2
        with host_route(nmf):
            host_gain, host_step = nmf.atom_tap_gains(margin)
        host_E = triggered_sums_numpy(Hp, fields['residual'], A, m)
        host_b = triggered_sums_numpy(Hp, fields['weights'], A, m, 2)
        bE = tref.bar(triggered_sums_numpy(Hp, np.abs(fields['residual']), A, m), D, A, m, N)
        bb = tref.bar(host_b, D, A, m, N)
        bound = np.zeros_like(gain)
        for t in (np.abs(step), np.abs(host_step)):
            bound = np.maximum(bound, t * bE + 0.5 * t * t * bb + 4 * tref.U * (t * np.abs(host_E) + 0.5 * t * t * host_b))
        err = np.abs(gain - host_gain)
        assert np.all(err[bound == 0] == 0)
        ratio = float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0), initial=0.))
        print(f'tap gains front end {name} margin {m}: largest error / bar {ratio:.3f}')
        assert ratio <= 1.
        ins, outs = nmf.atom_window_gains(margin)
        np.testing.assert_array_equal(np.stack([ins, outs]), np.stack(window_gains(gain, m, nmf.n_atoms)))
    for a, b in zip(before, [nmf.W, nmf.H]):                           # W and H are not touched
        np.testing.assert_array_equal(a, b)
    # margin 0 against the reference's W gradient
    if nmf._V.dtype == np.float64 and nmf._transforms is None and not FRONT_END[name].get('weights'):
        V, W, H = nmf._V, np.asarray(nmf.W, dtype=np.float64), np.asarray(nmf.H, dtype=np.float64)
        neg, pos = orc.gradient_W(V, W, H, mode=nmf._mode)
        R = orc.reconstruct(W, H, mode=nmf._mode)
        m0 = (0,) * len(A)
        Hp = pad_activations_numpy(H, A, nmf._mode)
        judge(f'front end {name} neg', nmf.activation_triggered_sums(0, 'data'), neg,
              triggered_sums_numpy(Hp, np.abs(V), A, m0), D, A, m0, N)
        judge(f'front end {name} pos', nmf.activation_triggered_sums(0, 'reconstruction'), pos,
              triggered_sums_numpy(Hp, np.abs(R), A, m0), D, A, m0, N)


def test_per_sample_comes_in_the_order_of_V_under_a_shuffle():
    nmf = fitted_hip(**FRONT_END['2d-valid-float32'])
    per = nmf.activation_triggered_sums(per_sample=True)
    nmf._shuffle_idx = np.arange(3)[::-1].copy()
    try:
        np.testing.assert_array_equal(nmf.activation_triggered_sums(per_sample=True), per[np.argsort(nmf._shuffle_idx)])
    finally:
        nmf._shuffle_idx = None


def test_a_window_beyond_the_limit_goes_through_the_host():
    nmf = fitted_hip(**FRONT_END['2d-valid-float32'])
    margin = (td.MAX_WINDOW[2] // 2, 1)
    X = nmf.activation_triggered_sums(margin, 'data')
    Hp = np.asarray(nmf.H, dtype=np.float64)
    np.testing.assert_array_equal(X, triggered_sums_numpy(Hp, nmf._V, (4, 5), margin))
