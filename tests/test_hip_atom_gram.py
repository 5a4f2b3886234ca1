"""
The atom Gram matrix on the GPU: tnmf_hip_atom_gram through the C ABI on operands made on the host, ``HIP_Backend.atom_gram``
in the four reconstruction modes, and the front end on ``backend='hip'``.

The kernel cases give R: the reconstruction in float64, rounded to the element type, so the kernel's own arithmetic is what is
judged.  The reference is evaluated in float64 on the same rounded operands (tests/atoms_reference.py).  With n = group *
prod(A) taps and u = 2^-24 (f32) or 2^-53 (f64) the bounds are derived, not measured:

    |B - B_ref| <= (2 n + 8) u B_ref                            |a - a_ref| <= (2 n + 8) u sum r_ref |G d|

r_m and r_m' are chains of n non-negative products each in the element type (relative error <= n u each: 2 n u in their
product), G r_m is one more rounding, in double, and the products are added in double; the constant 8, that of the atom terms,
covers the rounding of G r, the double additions and the reference's own.  All terms are non-negative, so the bound is
relative and a bound of 0 -- a dead atom's row and column -- demands an exact 0.  The double additions run along a chain of
at most L terms -- 256 per wave, tile and channel over the strip of tiles, the four waves, the strips
(atom_gram_dispatch.chain) -- whose worst case is L 2^-53: under 2^-13 u in float32, nothing next to the 8; in float64,
where the additions have the precision of the operands, the worst case L u of roundings that all point the same way is NOT
inside the constant, and the bound is asserted as it stands all the same: roundings to nearest of a growing sum do not line
up (largest ratio on an MI355X: 0.67, '1d-strip-boundary' with real weights, L = 4102; the others at most 0.62).  The float64 cases print the
ratio to (2 n + 8 + L) u as well: in float64 the bound is met on observation, not proved, and a kernel that added the same
terms in another order could exceed it without being wrong -- the second ratio is then the one to judge by.  ``a`` is folded
as tnmf_hip_atom_terms folds it and has its bound.  Where the library computes R itself (float64, generic kernels) n in the
bound of ``a`` is replaced by M * prod(A) + n; B does not depend on R.
Every test prints the largest ratio of an error to its bound.

The shapes are those of tests/atom_gram_dispatch.py: the smallest that reach every branch of the kernel.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import atom_gram_dispatch as gd
import atoms_reference as aref
import events_reference as eref
from test_atom_gains_cpu import _AtomStub, weights_of
from tnmf_amd import _lib
from tnmf_amd.atoms_host import atom_gram_numpy
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


def gram_of(parts, G):
    """B_ref[n, m, m'] = sum G R_m R_m' in float64; weights <= 0 count as 0."""
    N, Mo = parts.shape[:2]
    flat = parts.reshape(N, Mo, -1)
    g = np.ones((N, flat.shape[2])) if G is None else np.where(G > 0, G, 0.).reshape(N, -1)
    return np.einsum('nmx,nkx->nmk', flat * g[:, None], flat)


@functools.lru_cache(maxsize=None)
def operands(name, dt, kind):
    """-> dict of float64 arrays holding values of the element type, read-only: padded activations Hp with zeros among
    them (whole planes too: dead atoms), W, V, G (or None), R = the float64 reconstruction rounded to the element type, and
    the reference (a, B, scale)."""
    N, C, M, D, A, group = gd.ALL[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    Hp = rng.random((N, M) + tuple(d + a - 1 for d, a in zip(D, A)))
    Hp = Hp * np.repeat(rng.random((N, M // group) + (1,) * len(D)) > 0.15, group, axis=1)   # dead atoms, per sample
    Hp = rounded(Hp * (rng.random(Hp.shape) > 0.3), dt)
    W = rounded(rng.random((M, C) + A) + 0.1, dt)
    parts = aref.parts_valid(W, Hp, group)
    R = rounded(parts.sum(axis=1), dt)
    V = rounded(R * (0.5 + rng.random(R.shape)) + 0.1 * rng.random(R.shape), dt)
    G = weights_of((N, C) + D, kind)
    if G is not None:
        G = rounded(G, dt)
    a, _, scale = aref.terms(parts, V, G, R)
    out = dict(Hp=Hp, W=W, V=V, G=G, R=R, a=a, B=gram_of(parts, G), scale=scale, n=group * int(np.prod(A)),
               L=gd.chain(C, M, D, A, group, dt))
    for x in out.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out


def dev(x, dt):
    return None if x is None else torch.from_numpy(np.array(x, dtype=NP[dt])).cuda()


def padded_rows(Hp, dt):
    """(tensor [N, M, (Hy,) stride] whose pad is NaN, stride): the row stride is the shift width rounded up to 32."""
    stride = gd.cdiv(Hp.shape[-1], 32) * 32
    buf = np.full(Hp.shape[:-1] + (stride,), np.nan, dtype=NP[dt])
    buf[..., :Hp.shape[-1]] = Hp
    return torch.from_numpy(buf).cuda(), stride


def call(name, dt, ops, R='given', path='auto', stride=False, V=None):
    """-> (code, a [N, Mo], B [N, Mo, Mo] on the host) of one call on outputs filled with PATTERN."""
    N, C, M, D, A, group = gd.ALL[name]
    lib, ctx, _ = context(path)
    H, ld = padded_rows(ops['Hp'], dt) if stride else (dev(ops['Hp'], dt), 0)
    Mo = M // group
    a = torch.full((N, Mo), PATTERN, dtype=torch.float64, device='cuda')
    B = torch.full((N, Mo, Mo), PATTERN, dtype=torch.float64, device='cuda')
    g = _lib.make_geom(N, M, C, D, A, DTYPES.index(dt), ld)
    Vd, Gd, Wd = dev(ops['V'] if V is None else V, dt), dev(ops['G'], dt), dev(ops['W'], dt)
    Rd = dev(ops['R'], dt) if R == 'given' else None
    code = lib.tnmf_hip_atom_gram(ctx, ctypes.byref(g), group, p(Vd), p(Gd), p(Rd), p(Wd), p(H), p(a), p(B), None)
    torch.cuda.synchronize()
    return code, a.cpu().numpy(), B.cpu().numpy()


def ratios(a, B, ops, dt, n_a=None):
    """The largest |a - a_ref| and |B - B_ref| over their bounds; a bound of 0 asks for an exact 0."""
    u, n = U[dt], ops['n']
    for x in (a, B):
        assert np.all(np.isfinite(x)) and not np.any(x == PATTERN)
    ea, eb = np.abs(a - ops['a']), np.abs(B - ops['B'])
    ba = (2 * (n if n_a is None else n_a) + 8) * u * ops['scale']
    bb = (2 * n + 8) * u * ops['B']
    assert np.all(ea[ba == 0] == 0) and np.all(eb[bb == 0] == 0)
    return (float(np.max(ea[ba > 0] / ba[ba > 0], initial=0.)), float(np.max(eb[bb > 0] / bb[bb > 0], initial=0.)))


def judge(what, a, B, ops, dt, n_a=None):
    ra, rb = ratios(a, B, ops, dt, n_a)
    worst = f" (with the chain's worst case, L = {ops['L']}: {rb * (2 * ops['n'] + 8) / (2 * ops['n'] + 8 + ops['L']):.3f})"
    print(f'atom gram {what}: largest error / bound: a {ra:.3f}, B {rb:.3f}' + (worst if dt == 'f64' else ''))
    assert ra <= 1. and rb <= 1., (what, ra, rb)
    assert B.tobytes() == np.ascontiguousarray(B.transpose(0, 2, 1)).tobytes()   # symmetric to the bit


# -- 1. the kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('kind', KINDS, ids=str)
@pytest.mark.parametrize('name', list(gd.MATRIX))
def test_every_branch_of_the_kernel(name, kind, dt):
    ops = operands(name, dt, kind)
    code, a, B = call(name, dt, ops)
    assert code == 0
    judge(f'{name} {dt} G={kind}', a, B, ops, dt)
    dead = np.diagonal(ops['B'], axis1=1, axis2=2) == 0
    assert np.all(B[dead] == 0.) and np.all(B.transpose(0, 2, 1)[dead] == 0.)


@pytest.mark.parametrize('kind', KINDS, ids=str)
@pytest.mark.parametrize('name', list(gd.F32_ONLY))
def test_the_float32_only_branches_of_the_kernel(name, kind):
    ops = operands(name, 'f32', kind)
    code, a, B = call(name, 'f32', ops)
    assert code == 0
    judge(f'{name} f32 G={kind}', a, B, ops, 'f32')


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('kind', KINDS, ids=str)
@pytest.mark.parametrize('name', ['tile-plus-one', 'atoms-33', '1d-50'])
def test_without_weights_under_a_mask_and_with_real_weights(name, kind, dt):
    ops = operands(name, dt, kind)
    V = None
    if kind == 'mask':   # what a mask hides is not data: NaN there must not reach the sums
        V = np.where(ops['G'] > 0, ops['V'], np.nan)
    code, a, B = call(name, dt, ops, V=V)
    assert code == 0
    judge(f'{name} {dt} G={kind}', a, B, ops, dt)
    if kind == 'mask':
        hidden = np.array(ops['G'])
        hidden[1] = 0.
        blind = dict(ops, G=hidden)
        code, a1, B1 = call(name, dt, blind, V=np.where(hidden > 0, ops['V'], np.nan))
        assert code == 0 and np.all(a1[1] == 0.) and np.all(B1[1] == 0.)
        assert np.all(a1[0] == a[0]) and np.all(B1[0] == B[0])


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', ['tile-plus-one', 'atom-12x12', 'atoms-17', '1d-50'])
def test_row_padded_activations_whose_pad_is_nan(name, dt):
    ops = operands(name, dt, 'real')
    code, a, B = call(name, dt, ops, stride=True)
    assert code == 0
    judge(f'{name} {dt} row-padded', a, B, ops, dt)
    _, a0, B0 = call(name, dt, ops)
    assert a.tobytes() == a0.tobytes() and B.tobytes() == B0.tobytes()   # the same sums in the same order


@pytest.mark.parametrize('name', ['tile-plus-one', 'atom-12x12', '1d-50', 'channels-5'])
def test_the_librarys_own_reconstruction_against_a_given_one(name):
    N, C, M, D, A, group = gd.ALL[name]
    ops = operands(name, 'f64', 'real')
    code, a, B = call(name, 'f64', ops, path='generic')
    assert code == 0
    judge(f'{name} f64 R given', a, B, ops, 'f64')
    code, a1, B1 = call(name, 'f64', ops, R=None, path='generic')
    assert code == 0 and context('generic')[2].last_path == 'generic'
    judge(f'{name} f64 R = NULL', a1, B1, ops, 'f64', n_a=M * int(np.prod(A)) + ops['n'])
    assert B1.tobytes() == B.tobytes()   # (B does not look at R)


def test_two_calls_give_the_same_bits():
    for name, dt in (('tile-plus-one', 'f32'), ('atoms-33', 'f32'), ('atoms-33', 'f64'), ('strip-boundary', 'f32'),
                     ('1d-strip-boundary', 'f64')):
        ops = operands(name, dt, 'real')
        first, second = call(name, dt, ops), call(name, dt, ops)
        assert first[1].tobytes() == second[1].tobytes() and first[2].tobytes() == second[2].tobytes()


def test_the_diagonal_and_a_are_those_of_the_atom_terms():
    """diag(B) and a against tnmf_hip_atom_terms on the same operands: the same r, folded in double in another order --
    the sum of the two bounds against the float64 reference, (2 n + 8) + (4 n + 8) for the diagonal."""
    for name, dt in (('tile-plus-one', 'f32'), ('atom-12x12', 'f32'), ('atoms-17', 'f64')):
        N, C, M, D, A, group = gd.ALL[name]
        ops = operands(name, dt, 'real')
        _, a, B = call(name, dt, ops)
        lib, ctx, _ = context()
        ab = torch.empty((N, M // group, 2), dtype=torch.float64, device='cuda')
        g = _lib.make_geom(N, M, C, D, A, DTYPES.index(dt), 0)
        ts = [dev(ops[k], dt) for k in ('V', 'G', 'R', 'W', 'Hp')]
        assert lib.tnmf_hip_atom_terms(ctx, ctypes.byref(g), group, *(p(t) for t in ts), p(ab), None) == 0
        torch.cuda.synchronize()
        ab = ab.cpu().numpy()
        u, n = U[dt], ops['n']
        diag = np.diagonal(B, axis1=1, axis2=2)
        rb = np.max(np.abs(diag - ab[..., 1]) / np.maximum((6 * n + 16) * u * diag, 1e-300))
        ra = np.max(np.abs(a - ab[..., 0]) / np.maximum(2 * (2 * n + 8) * u * ops['scale'], 1e-300))
        print(f'atom gram {name} {dt} against the atom terms: largest difference / bound: a {ra:.3f}, diag(B) {rb:.3f}')
        assert ra <= 1. and rb <= 1.


def test_refusals_return_their_code_and_write_nothing():
    lib, ctx, _ = context()
    N, C, M, D, A, _ = gd.MATRIX['tile-plus-one']
    ops = operands('tile-plus-one', 'f32', None)
    Vd, Rd, Wd, Hd = (dev(ops[k], 'f32') for k in ('V', 'R', 'W', 'Hp'))
    a = torch.full((N, M), PATTERN, dtype=torch.float64, device='cuda')
    B = torch.full((N, M, M), PATTERN, dtype=torch.float64, device='cuda')
    flat = _lib.make_geom(N, M, C, D, A, 0)
    vol = _lib.make_geom(N, M, C, (4, 4, 4), (2, 2, 2), 0)
    huge = _lib.make_geom(1, 1, 1, (16, 16), (200, 200), 1)   # 215 rows of 268 doubles of H per tile: beyond the LDS
    for g, group, want in ((flat, 0, _lib.E_GEOM), (flat, -1, _lib.E_GEOM), (flat, 2, _lib.E_GEOM), (flat, M + 1, _lib.E_GEOM),
                           (vol, 1, _lib.E_UNSUPPORTED), (huge, 1, _lib.E_UNSUPPORTED)):
        assert gd.plan(1, 1, (16, 16), (200, 200), 1, 'f64')['cap'] == 0
        code = lib.tnmf_hip_atom_gram(ctx, ctypes.byref(g), group, p(Vd), None, p(Rd), p(Wd), p(Hd), p(a), p(B), None)
        torch.cuda.synchronize()
        assert code == want, (group, code, want)
        assert bool(torch.all(a == PATTERN)) and bool(torch.all(B == PATTERN))
    assert lib.tnmf_hip_atom_gram(ctx, ctypes.byref(flat), 1, p(Vd), None, p(Rd), p(Wd), p(Hd), None, p(B), None) == -1
    assert lib.tnmf_hip_atom_gram(ctx, ctypes.byref(flat), 1, p(Vd), None, p(Rd), p(Wd), p(Hd), p(a), None, None) == -1
    torch.cuda.synchronize()
    assert bool(torch.all(a == PATTERN)) and bool(torch.all(B == PATTERN))
    assert lib.tnmf_hip_atom_gram(ctx, ctypes.byref(flat), 1, p(Vd), None, p(Rd), p(Wd), p(Hd), p(a), p(B), None) == 0
    torch.cuda.synchronize()
    assert not bool(torch.any(a == PATTERN)) and not bool(torch.any(B == PATTERN))


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
    """HIP_Backend.atom_gram, float64, against atom_gram_numpy: the bounds of the kernel tests, with M * prod(A) more
    products behind ``a`` (the library's own R)."""
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
    a, B = be.atom_gram(V, torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda(), group)
    assert a.shape == (N, P // group) and B.shape == (N, P // group, P // group) and a.dtype == B.dtype == np.float64
    wa, wB = atom_gram_numpy(W, H, mode, V, G, group)
    parts = aref.parts_loop(W, H, D, mode, group)
    _, _, scale = aref.terms(parts, V, G)
    ops = dict(a=wa, B=wB, scale=scale, n=group * int(np.prod(A)), L=gd.chain(C, P, D, A, group, 'f64'))
    judge(f'{name} {"weighted" if weighted else "plain"} f64', a, B, ops, 'f64', n_a=(P + group) * int(np.prod(A)))
    with pytest.raises(_lib.TnmfHipError):
        be.atom_gram(V, torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda(), 3)


def test_the_backend_refuses_volumes():
    np.random.seed(0)
    be = HIP_Backend()
    W, H = be.initialize(np.ones((1, 1, 5, 5, 5)), (2, 2, 2), 2, None, (-3, -2, -1))
    with pytest.raises(NotImplementedError, match='atom gains: 1 or 2 shift axes only'):
        be.atom_gram(None, W, H, 1)


# -- 3. the front end ----------------------------------------------------------------------------------------------------------
def fitted_hip(shape_V, M, A, mode='valid', transforms=None, weighted=False, seed=0, dtype=np.float64, n_iterations=3):
    V = (np.random.default_rng(seed).random(shape_V) + 0.05).astype(dtype)
    G = weights_of(shape_V, 'real').astype(dtype) if weighted else None
    np.random.seed(42)
    hip = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip', reconstruction_mode=mode, transforms=transforms)
    hip.fit(V, n_iterations=n_iterations, sparsity_H=0.1, weights=G)
    return hip, V, G


FRONT_END = {
    'valid': dict(shape_V=(3, 2, 20, 70), M=3, A=(5, 5)),
    'rot90': dict(shape_V=(2, 1, 20, 20), M=2, A=(5, 5), transforms='rot90'),
    'weighted': dict(shape_V=(3, 2, 17, 65), M=3, A=(3, 4), weighted=True),
    '1d': dict(shape_V=(3, 2, 90), M=3, A=(7,), mode='circular'),
}


@pytest.mark.parametrize('name', list(FRONT_END))
def test_rescale_atoms_on_hip_changes_the_objective_by_the_returned_drop(name):
    """float64, u = 2^-53.  The drop is a^T e - 1/2 e^T B e with e = s - 1; the objective is 1/2 sum G (V - R)^2, before and
    after.  A pixel of R is a sum of n' = M T prod(A) non-negative products (relative error n' u), d = V - R rounds once,
    and an objective adds K = N C prod(D) squares: each objective is good to (2 n' + K + 4) u E_abs with
    E_abs = 1/2 sum G (|V| + R)^2, which bounds both the objective and sum G |d| R; R taken as the larger of before and
    after.  ``a`` (on the library's own R) is good to (2 (n' + n) + 8) u sum R_m |G d| and B to (2 n + 8) u B, the
    bounds of the kernel tests with n = T prod(A), so the drop to |e| times those.  The bar is the sum of the three; the
    host algebra on M <= 3 atoms adds a few u of the same terms and is covered by the constants.  The test prints the
    ratio."""
    cfg = FRONT_END[name]
    hip, V, G = fitted_hip(**cfg)
    assert getattr(hip._backend, 'atom_gram', None) is not None
    u, M, T = U['f64'], cfg['M'], hip.n_transforms
    g = np.ones(V.shape) if G is None else G
    before, R0 = hip.objective(), hip.R
    B = hip.atom_gram()
    scale_a = np.array([float(np.sum(np.abs(hip.R_partial(m)) * np.abs(g * (V - R0)))) for m in range(M)])
    version, W = hip._H._version, hip.W
    drop = hip.rescale_atoms()
    assert hip._H._version > version                      # an in-place torch operation: the spectrum cache sees it
    after, R1, s = hip.objective(), hip.R, hip.atom_scales_
    np.testing.assert_array_equal(hip.W, W)
    e = np.abs(s - 1.)
    n, n_prime, K = T * int(np.prod(cfg['A'])), M * T * int(np.prod(cfg['A'])), int(np.prod(V.shape))
    E_abs = 0.5 * float(np.sum(g * (np.abs(V) + np.maximum(R0, R1)) ** 2))
    bar = u * (2 * (2 * n_prime + K + 4) * E_abs + (2 * (n_prime + n) + 8) * float(e @ scale_a)
               + (2 * n + 8) * 0.5 * float(e @ B @ e))
    err = abs((before - after) - drop)
    print(f'rescale_atoms {name}: drop {drop:.6e} of {before:.6e}, scales {s}, error / bar {err / bar:.3f}')
    assert drop >= 0. and err <= bar
    # nothing is left to gain
    np.testing.assert_allclose(hip.atom_scales(), 1., atol=1e-9)


def test_the_front_end_on_hip_equals_the_host_fallback_in_float64():
    """atom_gram / atom_set_gain / atom_elimination on hip against the same model on a backend without the hook: B to the
    bound of the kernel tests, (2 n + 8) u sqrt(B_mm B_m'm')."""
    cfg = FRONT_END['weighted']
    hip, V, G = fitted_hip(**cfg)
    np.random.seed(42)
    cpu = TransformInvariantNMF(n_atoms=cfg['M'], atom_shape=cfg['A'], backend=_AtomStub('valid'))
    cpu.fit(V, n_iterations=0, weights=G)
    cpu._W[...] = hip.W
    cpu._H[...] = hip._backend.to_ndarray(hip._H)
    assert getattr(cpu._backend, 'atom_gram', None) is None
    before = [np.array(x) for x in (hip.W, hip.H)]
    got, want = hip.atom_gram(per_sample=True), cpu.atom_gram(per_sample=True)
    n = int(np.prod(cfg['A']))
    d = np.sqrt(np.diagonal(want, axis1=1, axis2=2))
    ratio = float(np.max(np.abs(got - want) / ((2 * n + 8) * U['f64'] * d[:, :, None] * d[:, None, :])))
    print(f'atom gram on hip against the fallback: largest error / bound {ratio:.3f}')
    assert ratio <= 1.
    np.testing.assert_array_equal(hip.atom_gram(), got.sum(axis=0))
    np.testing.assert_allclose(hip.atom_set_gain([0, 2]), cpu.atom_set_gain([0, 2]), rtol=1e-10)
    np.testing.assert_array_equal(hip.atom_elimination()[0], cpu.atom_elimination()[0])
    np.testing.assert_allclose(hip.atom_scales(), cpu.atom_scales(), rtol=1e-8)
    for was, now in zip(before, (hip.W, hip.H)):
        np.testing.assert_array_equal(was, now)


def test_planted_shifted_copies_overlap_at_least_as_planted():
    """Atom 1 is atom 0 moved by (1, 2) inside its window, and its activations are those of atom 0 moved back -- H absorbs
    the shift, R_1 = R_0 exactly -- plus extra events of its own, R_1 = R_0 + R_E with R_E >= 0 and |R_E| = t |R_0|.  Then
    cos(R_0, R_1) >= |R_0| / (|R_0| + |R_E|) = 1 / (1 + t): the planted value.  The overlap must reach it, and equal the
    cosine of the float64 parts to 2 (2 n + 8) u relative, n = 25, u = 2^-24: the three sums B_01, B_00, B_11 each have the
    kernel tests' bound (2 n + 8) u, the two under the square root count half each."""
    rng = np.random.default_rng(9)
    A, D, N = (5, 5), (20, 70), 2
    pattern = np.zeros(A)
    pattern[:3, :3] = rng.random((3, 3)) + 0.2
    W = np.stack([pattern, np.roll(pattern, (1, 2), axis=(0, 1))])[:, None].astype(np.float32)
    S = tuple(d + a - 1 for d, a in zip(D, A))
    H0 = (rng.random((N,) + S) * (rng.random((N,) + S) > 0.9)).astype(np.float32)
    H0[:, :2], H0[:, -2:], H0[:, :, :3], H0[:, :, -3:] = 0., 0., 0., 0.
    moved = np.roll(H0, (-1, -2), axis=(1, 2))   # r_1[x] = sum_a H_1[x + a] W_0[A - 1 - a - (1, 2)]: H_1[y] = H_0[y + (1, 2)]
    extra = (0.5 * rng.random((N,) + S) * (rng.random((N,) + S) > 0.97)).astype(np.float32)
    W64 = W.astype(np.float64)
    base = aref.parts_valid(W64, np.stack([H0, moved], axis=1).astype(np.float64))
    np.testing.assert_array_equal(base[:, 0], base[:, 1])
    H = np.stack([H0, moved + extra], axis=1)
    parts = aref.parts_valid(W64, H.astype(np.float64))
    norm = lambda x: float(np.sqrt(np.sum(x * x)))   # noqa: E731
    planted = 1. / (1. + norm(parts[:, 1] - parts[:, 0]) / norm(parts[:, 0]))
    cosine = float(np.sum(parts[:, 0] * parts[:, 1])) / (norm(parts[:, 0]) * norm(parts[:, 1]))
    assert 0.5 < planted <= cosine < 1.
    V = parts.sum(axis=1).astype(np.float32)
    np.random.seed(0)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=A, backend='hip')
    nmf.fit(V, n_iterations=0)
    nmf._W[...] = torch.from_numpy(W).cuda()
    nmf._H[...] = torch.from_numpy(H).cuda()
    ov = nmf.atom_overlaps()
    bound = 2 * (2 * 25 + 8) * U['f32']
    print(f'atom overlaps of planted shifted copies: {ov[0, 1]:.9f}, float64 cosine {cosine:.9f}, planted {planted:.9f}, '
          f'|difference| / bound {abs(ov[0, 1] - cosine) / (bound * cosine):.3f}')
    assert ov[0, 1] >= planted and abs(ov[0, 1] - cosine) <= bound * cosine
    assert ov[0, 1] == ov[1, 0] and ov[0, 0] == ov[1, 1] == 1.
