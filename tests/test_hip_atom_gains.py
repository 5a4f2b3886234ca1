"""
Atom terms on the GPU: tnmf_hip_atom_terms through the C ABI on operands made on the host, ``HIP_Backend.atom_terms`` in the
four reconstruction modes, and ``atom_gains`` on ``backend='hip'``.

The kernel cases give R: the reconstruction in float64, rounded to the element type, so the kernel's own arithmetic is what
is judged.  The reference (tests/atoms_reference.py) is evaluated in float64 on the same rounded operands.  With
n = group * prod(A) taps and u = 2^-24 (f32) or 2^-53 (f64) the bound is derived, not measured:

    |a - a_ref| <= (2 n + 8) u sum r_ref |G d|          |b - b_ref| <= (4 n + 8) u b_ref

r is a chain of n non-negative products, d and G d round once each, the sums are in double.  Where the library computes R
itself (float64, generic kernels: another order of the same M * prod(A) products) n is replaced by M * prod(A) + n.  Every
test prints the largest ratio of an error to its bound.

The shapes are those of tests/atoms_dispatch.py: the smallest that reach every branch of the kernel.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import atoms_dispatch as ad
import atoms_reference as aref
import events_reference as eref
from test_atom_gains_cpu import _AtomStub, weights_of
from tnmf_amd import _lib
from tnmf_amd.backends.HIP import HIP_Backend
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

pytestmark = pytest.mark.gpu

NP = {'f32': np.float32, 'f64': np.float64}
U = {'f32': 2. ** -24, 'f64': 2. ** -53}
DTYPES = ['f32', 'f64']
KINDS = [None, 'mask', 'real']
PATTERN = -12345.5


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def context(path='auto'):
    """A context of its own: the entry takes its geometry per call."""
    be = HIP_Backend(path=path)
    return be._lib, be._ctx, be


def rounded(x, dt):
    return np.asarray(x).astype(NP[dt]).astype(np.float64)


@functools.lru_cache(maxsize=None)
def operands(name, dt, kind):
    """-> dict of float64 arrays holding values of the element type, read-only: padded activations Hp with zeros among
    them, W, V, G (or None), R = the float64 reconstruction rounded to the element type, and the reference (a, b, scale)."""
    N, C, M, D, A, group = ad.MATRIX[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    Hp = rng.random((N, M) + tuple(d + a - 1 for d, a in zip(D, A))) * (rng.random((N, M) + (1,) * len(D)) > 0.15)
    Hp = rounded(Hp * (rng.random(Hp.shape) > 0.3), dt)
    W = rounded(rng.random((M, C) + A) + 0.1, dt)
    parts = aref.parts_valid(W, Hp, group)
    R = rounded(parts.sum(axis=1), dt)
    V = rounded(R * (0.5 + rng.random(R.shape)) + 0.1 * rng.random(R.shape), dt)
    G = weights_of((N, C) + D, kind)
    if G is not None:
        G = rounded(G, dt)
    a, b, scale = aref.terms(parts, V, G, R)
    out = dict(Hp=Hp, W=W, V=V, G=G, R=R, a=a, b=b, scale=scale, n=group * int(np.prod(A)))
    for x in out.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out


def dev(x, dt):
    return None if x is None else torch.from_numpy(np.array(x, dtype=NP[dt])).cuda()


def padded_rows(Hp, dt):
    """(tensor [N, M, (Hy,) stride] whose pad is NaN, stride): the row stride is the shift width rounded up to 32."""
    stride = ad.cdiv(Hp.shape[-1], 32) * 32
    buf = np.full(Hp.shape[:-1] + (stride,), np.nan, dtype=NP[dt])
    buf[..., :Hp.shape[-1]] = Hp
    return torch.from_numpy(buf).cuda(), stride


def call(name, dt, ops, R='given', path='auto', stride=False, V=None):
    """-> (code, ab [N, M / group, 2] on the host) of one call on an output filled with PATTERN."""
    N, C, M, D, A, group = ad.MATRIX[name]
    lib, ctx, _ = context(path)
    H, ld = padded_rows(ops['Hp'], dt) if stride else (dev(ops['Hp'], dt), 0)
    ab = torch.full((N, M // group, 2), PATTERN, dtype=torch.float64, device='cuda')
    g = _lib.make_geom(N, M, C, D, A, DTYPES.index(dt), ld)
    Vd, Gd, Wd = dev(ops['V'] if V is None else V, dt), dev(ops['G'], dt), dev(ops['W'], dt)
    Rd = dev(ops['R'], dt) if R == 'given' else None
    code = lib.tnmf_hip_atom_terms(ctx, ctypes.byref(g), group, p(Vd), p(Gd), p(Rd), p(Wd), p(H), p(ab), None)
    torch.cuda.synchronize()
    return code, ab.cpu().numpy()


def ratios(ab, ops, u, n=None):
    """The largest |a - a_ref| and |b - b_ref| over their bounds; a bound of 0 asks for an exact 0."""
    n = ops['n'] if n is None else n
    assert np.all(np.isfinite(ab)) and not np.any(ab == PATTERN)
    ea, eb = np.abs(ab[..., 0] - ops['a']), np.abs(ab[..., 1] - ops['b'])
    ba, bb = (2 * n + 8) * u * ops['scale'], (4 * n + 8) * u * ops['b']
    assert np.all(ea[ba == 0] == 0) and np.all(eb[bb == 0] == 0)
    return (float(np.max(ea[ba > 0] / ba[ba > 0], initial=0.)), float(np.max(eb[bb > 0] / bb[bb > 0], initial=0.)))


def judge(what, ab, ops, u, n=None):
    ra, rb = ratios(ab, ops, u, n)
    print(f'atom terms {what}: largest error / bound: a {ra:.3f}, b {rb:.3f}')
    assert ra <= 1. and rb <= 1., (what, ra, rb)


# -- 1. the kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', list(ad.MATRIX))
def test_every_branch_of_the_kernel(name, dt):
    kind = KINDS[list(ad.MATRIX).index(name) % 3]
    ops = operands(name, dt, kind)
    code, ab = call(name, dt, ops)
    assert code == 0
    judge(f'{name} {dt} G={kind}', ab, ops, U[dt])


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('kind', KINDS, ids=str)
@pytest.mark.parametrize('name', ['tile-plus-one', '1d-50'])
def test_without_weights_under_a_mask_and_with_real_weights(name, kind, dt):
    ops = operands(name, dt, kind)
    V = None
    if kind == 'mask':   # what a mask hides is not data: NaN there must not reach the sums
        V = np.where(ops['G'] > 0, ops['V'], np.nan)
    code, ab = call(name, dt, ops, V=V)
    assert code == 0
    judge(f'{name} {dt} G={kind}', ab, ops, U[dt])
    if kind == 'mask':
        hidden = np.array(ops['G'])
        hidden[1] = 0.
        blind = dict(ops, G=hidden)
        code, ab = call(name, dt, blind, V=np.where(hidden > 0, ops['V'], np.nan))
        assert code == 0 and np.all(ab[1] == 0.) and np.all(ab[0] == call(name, dt, ops, V=V)[1][0])


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', ['tile-plus-one', 'atom-12x12', '1d-50'])
def test_row_padded_activations_whose_pad_is_nan(name, dt):
    ops = operands(name, dt, 'real')
    code, ab = call(name, dt, ops, stride=True)
    assert code == 0
    judge(f'{name} {dt} row-padded', ab, ops, U[dt])
    np.testing.assert_array_equal(ab, call(name, dt, ops)[1])   # the same sums in the same order


@pytest.mark.parametrize('name', ['tile-plus-one', 'atom-12x12', '1d-50', 'channels-5'])
def test_the_librarys_own_reconstruction_against_a_given_one(name):
    N, C, M, D, A, group = ad.MATRIX[name]
    ops = operands(name, 'f64', 'real')
    code, given = call(name, 'f64', ops, path='generic')
    assert code == 0
    judge(f'{name} f64 R given', given, ops, U['f64'])
    code, own = call(name, 'f64', ops, R=None, path='generic')
    assert code == 0 and context('generic')[2].last_path == 'generic'
    judge(f'{name} f64 R = NULL', own, ops, U['f64'], n=M * int(np.prod(A)) + ops['n'])


def test_two_calls_give_the_same_bits():
    for name, dt in (('tile-plus-one', 'f32'), ('atom-12x12', 'f32'), ('1d-many-atoms', 'f64')):
        ops = operands(name, dt, 'real')
        first, second = call(name, dt, ops)[1], call(name, dt, ops)[1]
        assert first.tobytes() == second.tobytes()


def test_refusals_return_their_code_and_write_nothing():
    lib, ctx, _ = context()
    N, C, M, D, A, _ = ad.MATRIX['tile-plus-one']
    ops = operands('tile-plus-one', 'f32', None)
    Vd, Rd, Wd, Hd = (dev(ops[k], 'f32') for k in ('V', 'R', 'W', 'Hp'))
    ab = torch.full((N, M, 2), PATTERN, dtype=torch.float64, device='cuda')
    flat = _lib.make_geom(N, M, C, D, A, 0)
    vol = _lib.make_geom(N, M, C, (4, 4, 4), (2, 2, 2), 0)
    huge = _lib.make_geom(1, 1, 1, (16, 16), (200, 200), 1)   # 215 rows of 268 doubles of H per tile: beyond the LDS
    for g, group, want in ((flat, 0, _lib.E_GEOM), (flat, -1, _lib.E_GEOM), (flat, 2, _lib.E_GEOM), (flat, M + 1, _lib.E_GEOM),
                           (vol, 1, _lib.E_UNSUPPORTED), (huge, 1, _lib.E_UNSUPPORTED)):
        code = lib.tnmf_hip_atom_terms(ctx, ctypes.byref(g), group, p(Vd), None, p(Rd), p(Wd), p(Hd), p(ab), None)
        torch.cuda.synchronize()
        assert code == want, (group, code, want)
        assert bool(torch.all(ab == PATTERN))
    assert lib.tnmf_hip_atom_terms(ctx, ctypes.byref(flat), 1, p(Vd), None, p(Rd), p(Wd), p(Hd), None, None) == -1
    assert lib.tnmf_hip_atom_terms(ctx, ctypes.byref(flat), 1, p(Vd), None, p(Rd), p(Wd), p(Hd), p(ab), None) == 0
    torch.cuda.synchronize()
    assert not bool(torch.any(ab == PATTERN))


# -- 2. the four modes through the backend, which pads -------------------------------------------------------------------------
# the smallest geometries at the limits of include/tnmf_hip.h: 'circular' wraps once around (A - 1 == S), 'reflect' mirrors
# all but the edge (A - 1 == S - 1), 'full' clips an atom as large as the sample (S == 1)
MODE_CASES = {
    'valid': ((4, 5), (3, 4)), 'full': ((8, 9), (8, 9)), 'circular': ((4, 5), (5, 6)), 'reflect': ((4, 5), (4, 5)),
    'valid-1d': ((9,), (4,)), 'full-1d': ((7,), (7,)), 'circular-1d': ((6,), (7,)), 'reflect-1d': ((6,), (6,)),
}


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('name', list(MODE_CASES))
def test_the_modes_are_a_valid_pass_over_padded_activations(name, weighted):
    mode = name.split('-')[0]
    D, A = MODE_CASES[name]
    N, C, P, group = 2, 2, 4, 2
    rng = np.random.default_rng(5)
    V = rng.random((N, C) + D) + 0.05
    G = weights_of(V.shape, 'real') if weighted else None
    np.random.seed(0)
    be = HIP_Backend(reconstruction_mode=mode, path='generic')
    be.initialize(V, A, P, None, tuple(range(-len(A), 0)), **({'weights': G} if weighted else {}))
    H = rng.random((N, P) + eref.shift_shape(D, A, mode))
    W = rng.random((P, C) + A) + 0.1
    a, b = be.atom_terms(V, torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda(), group)
    assert a.shape == b.shape == (N, P // group) and a.dtype == np.float64
    ra, rb, scale = aref.terms(aref.parts_loop(W, H, D, mode, group), V, G)
    ops = dict(a=ra, b=rb, scale=scale)
    judge(f'{name} {"weighted" if weighted else "plain"} f64', np.stack([a, b], axis=-1), ops, U['f64'],
          n=(P + group) * int(np.prod(A)))
    with pytest.raises(_lib.TnmfHipError):
        be.atom_terms(V, torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda(), 3)


def test_the_backend_refuses_volumes():
    np.random.seed(0)
    be = HIP_Backend()
    W, H = be.initialize(np.ones((1, 1, 5, 5, 5)), (2, 2, 2), 2, None, (-3, -2, -1))
    with pytest.raises(NotImplementedError, match='atom gains: 1 or 2 shift axes only'):
        be.atom_terms(None, W, H, 1)


# -- 3. the front end ----------------------------------------------------------------------------------------------------------
def fitted_pair(shape_V, M, A, mode='valid', transforms=None, weighted=False, seed=0):
    """A model fitted on backend='hip' in float64 and the same model on the oracle backend, which has no hook."""
    V = np.random.default_rng(seed).random(shape_V) + 0.05
    G = weights_of(shape_V, 'real') if weighted else None
    np.random.seed(42)
    hip = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip', reconstruction_mode=mode, transforms=transforms)
    hip.fit(V, n_iterations=3, sparsity_H=0.1, weights=G)
    np.random.seed(42)
    cpu = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend=_AtomStub(mode), transforms=transforms)
    cpu.fit(V, n_iterations=0, weights=G)
    cpu._W[...] = hip.W
    cpu._H[...] = hip._backend.to_ndarray(hip._H)
    cpu._expand_W()
    return hip, cpu


FRONT_END = {
    'valid': dict(shape_V=(3, 2, 20, 70), M=3, A=(5, 5)),
    'reflect': dict(shape_V=(3, 1, 18, 30), M=3, A=(4, 6), mode='reflect'),
    'rot90': dict(shape_V=(2, 1, 20, 20), M=2, A=(5, 5), transforms='rot90'),
    'weighted': dict(shape_V=(3, 2, 17, 65), M=3, A=(3, 4), weighted=True),
    '1d': dict(shape_V=(3, 2, 90), M=3, A=(7,), mode='circular'),
}
# The largest relative difference, max |hip - fallback| / max |fallback|, measured on these cases on an MI355X, and the bar at
# ten times that: the margin covers the different order in which the library's reconstruct sums.
FRONT_END_MEASURED = 2.1e-16   # ('valid', per sample: 2.02e-16; the others 0 to 1.9e-16)
FRONT_END_BAR = 10 * FRONT_END_MEASURED


@pytest.mark.parametrize('name', list(FRONT_END))
def test_atom_gains_on_hip_equal_the_host_fallback_in_float64(name):
    hip, cpu = fitted_pair(**FRONT_END[name])
    assert getattr(hip._backend, 'atom_terms', None) is not None and getattr(cpu._backend, 'atom_terms', None) is None
    before = [np.array(x) for x in (hip.W, hip.H)]
    for per_sample in (True, False):
        got, want = hip.atom_gains(per_sample=per_sample), cpu.atom_gains(per_sample=per_sample)
        assert got.shape == want.shape and got.dtype == np.float64
        diff = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print(f'atom gains {name} per_sample={per_sample}: relative difference to the float64 fallback {diff:.3e}')
        assert diff <= FRONT_END_BAR, (name, diff)
    np.testing.assert_array_equal(hip.atom_gains(), hip.atom_gains(per_sample=True).sum(axis=0))
    for was, now in zip(before, (hip.W, hip.H)):
        np.testing.assert_array_equal(was, now)


# float32, the default path at a small size (direct kernels) and at one where 'auto' reconstructs in the frequency domain:
# the two sum identities against the library's own R.  With N' = M * T * prod(A) + n products behind each pixel of R:
#   |sum_m a[n, m] - <R, d>| <= (2 N' + 8) u sum R |d|
#   one atom: |gain - (1/2 ||V||^2 - objective)| <= (2 N' + 8) u sum R |d| + (4 N' + 8) u b / 2 + 4 u (1/2 ||V||^2 + objective)
# (the last term: the library's objective squares d = V - R as rounded to float32)
F32_CASES = {'direct': (3, 2, 20, 70), 'frequency-domain': (4, 1, 128, 128)}


@pytest.mark.parametrize('name', list(F32_CASES))
def test_float32_sum_identities_against_the_librarys_own_reconstruction(name):
    shape_V, A, u = F32_CASES[name], (5, 5), U['f32']
    V = (np.random.default_rng(1).random(shape_V) + 0.05).astype(np.float32)
    for M in (8, 1):
        np.random.seed(42)
        nmf = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip')
        nmf.fit(V, n_iterations=3, sparsity_H=0.1)
        R = nmf.R.astype(np.float64)
        if M == 8:
            assert (nmf._backend.last_path == 'fft') == (name == 'frequency-domain'), nmf._backend.last_path
        a, b = nmf.atom_terms()
        d = V.astype(np.float64) - R
        n_prime = M * int(np.prod(A)) + int(np.prod(A))
        scale = np.sum(R * np.abs(d), axis=(1, 2, 3))
        bound = (2 * n_prime + 8) * u * scale
        err = np.abs(a.sum(axis=1) - np.sum(R * d, axis=(1, 2, 3)))
        print(f'atom terms f32 {name} M={M}: sum of a against <R, d>: largest error / bound {np.max(err / bound):.3f}')
        assert np.all(err <= bound)
        if M == 1:
            energy, objective = 0.5 * float(np.sum(V.astype(np.float64) ** 2)), nmf.objective()
            bound1 = float(bound.sum() + (4 * n_prime + 8) * u * 0.5 * b.sum() + 4 * u * (energy + objective))
            err1 = abs(float(nmf.atom_gains()[0]) - (energy - objective))
            print(f'atom terms f32 {name}: one atom against the objective: error / bound {err1 / bound1:.3f}')
            assert err1 <= bound1
