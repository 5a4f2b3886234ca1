"""
The atom terms, gains and Gram under a beta-divergence on the GPU: tnmf_hip_atom_terms_beta and tnmf_hip_atom_gram_beta
through the C ABI on operands made on the host, ``HIP_Backend.atom_divergence_terms`` / ``atom_divergence_gram`` in the four
reconstruction modes, and the three front-end methods on ``backend='hip'``.

The kernel cases give R = rounded(sum of the parts + floor), floor = 0.25 mean(sum of the parts) + 0.05: R - r_m stays away
from the kink of max(., 0) and the kernel's own arithmetic is what is judged.  V = R (0.25 + 2.5 rand), so that the curvature
c is negative on a good part of the pixels at beta 0 and 3 (asserted).  The reference (tests/atom_divergence_reference.py)
is evaluated on the same rounded operands.  With n = group * prod(A) taps and u = 2^-24 (f32) or 2^-53 (f64) the bounds are
derived, not fitted:

    |a - a_ref|       <= (2 n + 8) u sum r_ref |gd_ref|
    |b - b_ref|       <= (4 n + 8) u sum |gw_ref| r_ref^2              |B - B_ref| <= (2 n + 8) u sum |gw_ref| r_m r_m'
    |gain - gain_ref| <= (n + 8) u sum G r_ref max(|f(x_lo)|, |f(x_hi)|)
        f(x) = x^(beta-1) - V x^(beta-2),   x_lo/hi = max(R - r_ref -/+ (n + 2) u r_ref, 0) + eps

r is a chain of n non-negative products in the element type; gd and gw round once to the element type; everything else is
in double.  A bound of 0 asks for an exact 0.  So that the gain's bound says something, every (sample, atom) of every kernel
case must have it below 1e-3 of the sum of its absolute pixel terms (asserted).  Where the library computes R itself
(float64, generic kernels: another order of the same M * prod(A) products, relative error e = M prod(A) u) the factors move
with x: 4 e sum r (G (V + x) x^(beta-2)) is added to the bound of a, 4 e sum (G (|beta-1| x + |2-beta| V) x^(beta-3)) r r'
to those of b and B (|beta-2| + 1 and |beta-3| + 1 are at most 4 for 0 <= beta <= 3), and n in the gain's bound becomes
M prod(A) + n.  There, and on fitted models, R is the plain sum of the parts: pixels that one atom explains alone have
x_m = eps, their terms are of the size V log(R / eps) and as sensitive to the last bit of R - r, so the condition on the
gain's bound cannot hold and is printed, not asserted.  Every test prints the largest ratio of an error to its bound.
Largest ratios on an MI355X: float32 a 0.021, b 0.022, gain 0.025, B 0.021; float64 a 0.18, b 0.13, gain 0.23, B 0.91 ('1d-strip-boundary', beta 0: as
tests/test_hip_atom_gram.py says of its own bound, in float64 the chain of double additions of B is not inside the constant
and the bound is met on observation); the gain's bound is at most 6.6e-5 of the sum of the absolute pixel terms.

The shapes are those of tests/atoms_dispatch.py and tests/atom_gram_dispatch.py: the smallest that reach every branch of the
two kernels.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import atom_divergence_reference as dref
import atom_gram_dispatch as gd
import atoms_dispatch as ad
import atoms_reference as aref
import events_reference as eref
from test_atom_gains_cpu import weights_of
from tnmf_amd import _lib
from tnmf_amd.atoms_host import atom_divergence_terms_numpy
from tnmf_amd.backends.HIP import HIP_Backend
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

pytestmark = pytest.mark.gpu

NP = {'f32': np.float32, 'f64': np.float64}
U = {'f32': 2. ** -24, 'f64': 2. ** -53}
DTYPES = ['f32', 'f64']
KINDS = [None, 'mask', 'real']
BETAS = [0., 1., 1.5, 3.]
EPS = 1e-9
PATTERN = -12345.5
# the largest tile of H that tnmf_hip_atom_terms admits: 65 rows of 116 doubles = 60 320 bytes of the 60 KiB (61 440) it
# allows, beside which the waves' three sums per atom must fit the remaining 4 KiB of the 64
LDS_LIMIT_CASE = {'lds-limit': (1, 1, 2, (16, 16), (50, 50), 1)}
TABLES = {'terms': ad.MATRIX, 'gram': gd.ALL, 'limit': LDS_LIMIT_CASE}


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def context(path='auto'):
    """A context of its own: the entries take their geometry per call."""
    be = HIP_Backend(path=path)
    return be._lib, be._ctx, be


def rounded(x, dt):
    return np.asarray(x).astype(NP[dt]).astype(np.float64)


def frozen(out):
    for x in out.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def operands(table, name, dt, kind):
    """-> dict of read-only float64 arrays holding values of the element type: padded activations Hp with zeros and dead
    atoms among them, W, V, G (or None), the parts and R = rounded(their sum + floor)."""
    N, C, M, D, A, group = TABLES[table][name]
    rng = np.random.default_rng(sum(map(ord, table + name)))
    Hp = rng.random((N, M) + tuple(d + a - 1 for d, a in zip(D, A)))
    Hp = Hp * np.repeat(rng.random((N, M // group) + (1,) * len(D)) > 0.15, group, axis=1)   # dead atoms, per sample
    Hp = rounded(Hp * (rng.random(Hp.shape) > 0.3), dt)
    W = rounded(rng.random((M, C) + A) + 0.1, dt)
    parts = aref.parts_valid(W, Hp, group)
    total = parts.sum(axis=1)
    R = rounded(total + 0.25 * total.mean() + 0.05, dt)
    V = rounded(R * (0.25 + 2.5 * rng.random(R.shape)), dt)
    G = weights_of((N, C) + D, kind)
    if G is not None:
        G = rounded(G, dt)
    return frozen(dict(Hp=Hp, W=W, V=V, G=G, R=R, parts=parts, n=group * int(np.prod(A)), geometry=(N, C, M, D, A, group)))


@functools.lru_cache(maxsize=None)
def reference(table, name, dt, kind, beta, R='given'):
    """The reference sums and the bounds' scales of one case; R = None: the library reconstructs (R = the sum of the parts)."""
    ops = operands(table, name, dt, kind)
    Rr = ops['R'] if R == 'given' else ops['parts'].sum(axis=1)
    out = dref.terms(ops['parts'], ops['V'], ops['G'], Rr, beta, EPS)
    out['B'], out['scale_B'] = dref.gram(ops['parts'], ops['V'], ops['G'], Rr, beta, EPS)
    gd_abs, gw_abs = dref.factors_abs(ops['V'], Rr, ops['G'], beta, EPS)
    axes = tuple(range(2, ops['parts'].ndim))
    flat = ops['parts'].reshape(ops['parts'].shape[:2] + (-1,))
    out['abs_a'] = np.sum(ops['parts'] * gd_abs[:, None], axis=axes)
    out['abs_B'] = np.einsum('nmx,nkx->nmk', flat * gw_abs.reshape(flat.shape[0], 1, -1), flat)
    out['Rr'] = Rr
    return frozen(out)


def dev(x, dt):
    return None if x is None else torch.from_numpy(np.array(x, dtype=NP[dt])).cuda()


def padded_rows(Hp, dt):
    """(tensor [N, M, (Hy,) stride] whose pad is NaN, stride): the row stride is the shift width rounded up to 32."""
    stride = ad.cdiv(Hp.shape[-1], 32) * 32
    buf = np.full(Hp.shape[:-1] + (stride,), np.nan, dtype=NP[dt])
    buf[..., :Hp.shape[-1]] = Hp
    return torch.from_numpy(buf).cuda(), stride


def call(entry, ops, dt, beta, R='given', path='auto', stride=False, V=None, G='own', eps=EPS):
    """-> (code, outputs on the host) of one call on outputs filled with PATTERN: (abg [N, Mo, 3],) of 'terms',
    (a [N, Mo], B [N, Mo, Mo]) of 'gram'."""
    N, C, M, D, A, group = ops['geometry']
    lib, ctx, _ = context(path)
    H, ld = padded_rows(ops['Hp'], dt) if stride else (dev(ops['Hp'], dt), 0)
    Mo = M // group
    shapes = [(N, Mo, 3)] if entry == 'terms' else [(N, Mo), (N, Mo, Mo)]
    outs = [torch.full(s, PATTERN, dtype=torch.float64, device='cuda') for s in shapes]
    g = _lib.make_geom(N, M, C, D, A, DTYPES.index(dt), ld)
    Vd, Wd = dev(ops['V'] if V is None else V, dt), dev(ops['W'], dt)
    Gd = dev(ops['G'] if isinstance(G, str) else G, dt)
    Rd = dev(ops['R'], dt) if R == 'given' else None
    fn = lib.tnmf_hip_atom_terms_beta if entry == 'terms' else lib.tnmf_hip_atom_gram_beta
    code = fn(ctx, ctypes.byref(g), group, float(beta), float(eps), p(Vd), p(Gd), p(Rd), p(Wd), p(H), *(p(o) for o in outs),
              None)
    torch.cuda.synchronize()
    return (code,) + tuple(o.cpu().numpy() for o in outs)


def worst(err, bound):
    """The largest error over its bound; a bound of 0 asks for an exact 0."""
    assert np.all(np.isfinite(err)) and np.all(err[bound == 0] == 0), float(np.max(err[bound == 0], initial=0.))
    return float(np.max(err[bound > 0] / bound[bound > 0], initial=0.))


def bounds(ops, ref, u, beta, own_R=False):
    """The bounds of the module's docstring -> dict(a, b, gain, B)."""
    n = ops['n']
    N, C, M, D, A, group = ops['geometry']
    e = M * int(np.prod(A)) * u if own_R else 0.
    diag = np.diagonal(ref['abs_B'], axis1=1, axis2=2)
    n_gain = n + (M * int(np.prod(A)) if own_R else 0)
    return dict(a=(2 * n + 8) * u * ref['scale_a'] + 4 * e * ref['abs_a'],
                b=(4 * n + 8) * u * ref['scale_b'] + 4 * e * diag,
                B=(2 * n + 8) * u * ref['scale_B'] + 4 * e * ref['abs_B'],
                gain=dref.gain_bound(ops['parts'], ops['V'], ops['G'], ref['Rr'], beta, EPS, n_gain, u))


def judge_terms(what, abg, ops, ref, u, beta, own_R=False, vacuous='assert'):
    assert np.all(np.isfinite(abg)) and not np.any(abg == PATTERN)
    bd = bounds(ops, ref, u, beta, own_R)
    r = {k: worst(np.abs(abg[..., i] - ref[k]), bd[k]) for i, k in enumerate(('a', 'b', 'gain'))}
    live = ref['scale_gain'] > 0
    assert np.all(bd['gain'][~live] == 0)
    says = float(np.max(bd['gain'][live] / ref['scale_gain'][live], initial=0.))
    print(f'atom divergence terms {what}: largest error / bound: a {r["a"]:.3f}, b {r["b"]:.3f}, gain {r["gain"]:.3f}; '
          f'largest gain bound / sum of |pixel terms| {says:.2e}')
    assert r['a'] <= 1. and r['b'] <= 1. and r['gain'] <= 1., (what, r)
    if vacuous == 'assert':
        assert says <= 1e-3, (what, says)


def judge_gram(what, a, B, ops, ref, u, beta, own_R=False):
    for x in (a, B):
        assert np.all(np.isfinite(x)) and not np.any(x == PATTERN)
    bd = bounds(ops, ref, u, beta, own_R)
    ra, rb = worst(np.abs(a - ref['a']), bd['a']), worst(np.abs(B - ref['B']), bd['B'])
    print(f'atom divergence gram {what}: largest error / bound: a {ra:.3f}, B {rb:.3f}')
    assert ra <= 1. and rb <= 1., (what, ra, rb)
    assert B.tobytes() == np.ascontiguousarray(B.transpose(0, 2, 1)).tobytes()   # symmetric to the bit


def assert_negative_curvature(ops, ref, beta):
    if beta in (0., 3.):
        neg, live = dref.curvature_is_negative(ops['V'], ref['Rr'], ops['G'], beta, EPS)
        assert neg >= 0.05 * live, (beta, neg, live)


# -- 1. the two kernels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', list(ad.MATRIX))
def test_every_branch_of_the_terms_kernel(name, dt, beta):
    kind = KINDS[(list(ad.MATRIX).index(name) + BETAS.index(beta)) % 3]
    ops, ref = operands('terms', name, dt, kind), reference('terms', name, dt, kind, beta)
    assert_negative_curvature(ops, ref, beta)
    code, abg = call('terms', ops, dt, beta)
    assert code == 0
    judge_terms(f'{name} {dt} beta={beta} G={kind}', abg, ops, ref, U[dt], beta)


@pytest.mark.parametrize('beta', [1., 1.5])
def test_the_largest_tile_of_H_that_the_atom_terms_admit(beta):
    N, C, M, D, A, group = LDS_LIMIT_CASE['lds-limit']
    plan = ad.plan(C, D, A)
    assert 58 * 1024 < plan['SH'] * plan['SW'] * 8 <= ad.LDS_LIMIT
    ops, ref = operands('limit', 'lds-limit', 'f64', 'real'), reference('limit', 'lds-limit', 'f64', 'real', beta)
    code, abg = call('terms', ops, 'f64', beta)
    assert code == 0
    judge_terms(f'lds-limit f64 beta={beta}', abg, ops, ref, U['f64'], beta)


# (the float32-only shapes of the Gram kernel are refused in float64: test_refusals_return_their_code_and_write_nothing)
GRAM_CASES = [(name, dt) for name in gd.ALL for dt in DTYPES if not (dt == 'f64' and name in gd.F32_ONLY)]


@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('name,dt', GRAM_CASES)
def test_every_branch_of_the_gram_kernel(name, dt, beta):
    kind = KINDS[(list(gd.ALL).index(name) + BETAS.index(beta)) % 3]
    ops, ref = operands('gram', name, dt, kind), reference('gram', name, dt, kind, beta)
    assert_negative_curvature(ops, ref, beta)
    code, a, B = call('gram', ops, dt, beta)
    assert code == 0
    judge_gram(f'{name} {dt} beta={beta} G={kind}', a, B, ops, ref, U[dt], beta)
    dead = np.all(ops['parts'].reshape(ops['parts'].shape[:2] + (-1,)) == 0, axis=2)
    assert np.all(B[dead] == 0.) and np.all(B.transpose(0, 2, 1)[dead] == 0.)


@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('dt', DTYPES)
def test_the_gain_is_exact_at_the_kink(dt, beta):
    """One atom (M = group) with dyadic H and W: r is exact in float32, R is given equal to r, so x_m == eps exactly and the
    gain has no error but the epilogue's own: 64 * 2^-53 relative, in both element types."""
    N, C, M, D, A, group = 2, 1, 2, (17, 65), (3, 4), 2
    rng = np.random.default_rng(11)
    Hp = rng.integers(0, 9, (N, M, D[0] + A[0] - 1, D[1] + A[1] - 1)) / 4. * (rng.random((N, M, 19, 68)) > 0.3)
    W = rng.integers(1, 5, (M, C) + A) / 2.
    parts = aref.parts_valid(W, Hp, group)
    R = parts[:, 0]
    assert np.array_equal(rounded(R, 'f32'), R) and np.all(R > 0)
    V = rounded(rng.random(R.shape) + 0.05, dt)
    ops = dict(Hp=Hp, W=W, V=V, G=None, R=R, parts=parts, n=group * 12, geometry=(N, C, M, D, A, group))
    ref = dref.terms(parts, V, None, R, beta, EPS)
    code, abg = call('terms', ops, dt, beta)
    assert code == 0
    ratio = float(np.max(np.abs(abg[..., 2] - ref['gain']) / (64 * 2. ** -53 * ref['scale_gain'])))
    print(f'atom divergence gain at the kink {dt} beta={beta}: largest error / (64 * 2^-53 * gain) {ratio:.3f}')
    assert ratio <= 1.


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('entry,name', [('terms', 'tile-plus-one'), ('terms', '1d-50'), ('gram', 'atoms-33'), ('gram', '1d-50')])
def test_a_mask_hides_whatever_V_holds(entry, name, dt):
    beta = 1.
    ops, ref = operands(entry, name, dt, 'mask'), reference(entry, name, dt, 'mask', beta)
    V = np.where(ops['G'] > 0, ops['V'], np.nan)
    seen = call(entry, ops, dt, beta, V=V)
    assert seen[0] == 0
    if entry == 'terms':
        judge_terms(f'{name} {dt} NaN under the mask', seen[1], ops, ref, U[dt], beta)
    else:
        judge_gram(f'{name} {dt} NaN under the mask', seen[1], seen[2], ops, ref, U[dt], beta)
    hidden = np.array(ops['G'])
    hidden[1] = 0.
    blind = call(entry, ops, dt, beta, V=np.where(hidden > 0, ops['V'], np.nan), G=hidden)
    assert blind[0] == 0
    for got, full in zip(blind[1:], seen[1:]):
        assert np.all(got[1] == 0.) and got[0].tobytes() == full[0].tobytes()


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('entry,name', [('terms', 'tile-plus-one'), ('terms', 'atom-12x12'), ('terms', '1d-50'),
                                        ('gram', 'atom-12x12'), ('gram', 'atoms-17')])
def test_row_padded_activations_whose_pad_is_nan(entry, name, dt):
    beta = 1.5
    ops = operands(entry, name, dt, 'real')
    padded, plain = call(entry, ops, dt, beta, stride=True), call(entry, ops, dt, beta)
    assert padded[0] == 0 and plain[0] == 0
    for x, y in zip(padded[1:], plain[1:]):
        assert np.all(np.isfinite(x)) and x.tobytes() == y.tobytes()   # the same sums in the same order


@pytest.mark.parametrize('beta', [0., 1., 1.5])
@pytest.mark.parametrize('name', ['tile-plus-one', 'atom-12x12', '1d-50', 'channels-5'])
def test_the_librarys_own_reconstruction(name, beta):
    ops, ref = operands('terms', name, 'f64', 'real'), reference('terms', name, 'f64', 'real', beta, R=None)
    code, abg = call('terms', ops, 'f64', beta, R=None, path='generic')
    assert code == 0 and context('generic')[2].last_path == 'generic'
    judge_terms(f'{name} f64 beta={beta} R = NULL', abg, ops, ref, U['f64'], beta, own_R=True, vacuous='report')
    ops, ref = operands('gram', name, 'f64', 'real'), reference('gram', name, 'f64', 'real', beta, R=None)
    code, a, B = call('gram', ops, 'f64', beta, R=None, path='generic')
    assert code == 0
    judge_gram(f'{name} f64 beta={beta} R = NULL', a, B, ops, ref, U['f64'], beta, own_R=True)


@pytest.mark.parametrize('dt', DTYPES)
def test_beta_2_is_the_frobenius_entries_bit_for_bit(dt):
    lib, ctx, _ = context()
    for name in ('tile-plus-one', 'atom-12x12', '1d-50'):
        ops = operands('gram', name, dt, 'real')
        N, C, M, D, A, group = ops['geometry']
        g = _lib.make_geom(N, M, C, D, A, DTYPES.index(dt), 0)
        ts = [dev(ops[k], dt) for k in ('V', 'G', 'R', 'W', 'Hp')]
        ab = torch.empty((N, M // group, 2), dtype=torch.float64, device='cuda')
        a0 = torch.empty((N, M // group), dtype=torch.float64, device='cuda')
        B0 = torch.empty((N, M // group, M // group), dtype=torch.float64, device='cuda')
        assert lib.tnmf_hip_atom_terms(ctx, ctypes.byref(g), group, *(p(t) for t in ts), p(ab), None) == 0
        assert lib.tnmf_hip_atom_gram(ctx, ctypes.byref(g), group, *(p(t) for t in ts), p(a0), p(B0), None) == 0
        torch.cuda.synchronize()
        ab = ab.cpu().numpy()
        code, abg = call('terms', ops, dt, 2.)
        assert code == 0 and abg[..., :2].tobytes() == ab.tobytes()
        assert abg[..., 2].tobytes() == (ab[..., 0] + ab[..., 1] / 2).tobytes()
        code, a, B = call('gram', ops, dt, 2.)
        assert code == 0 and a.tobytes() == a0.cpu().numpy().tobytes() and B.tobytes() == B0.cpu().numpy().tobytes()


def test_two_calls_give_the_same_bits():
    for entry, name, dt, beta in (('terms', 'tile-plus-one', 'f32', 1.), ('terms', 'atom-12x12', 'f32', 0.),
                                  ('terms', '1d-many-atoms', 'f64', 1.5), ('gram', 'atoms-33', 'f32', 3.),
                                  ('gram', 'atoms-33', 'f64', 1.), ('gram', 'strip-boundary', 'f32', 0.)):
        ops = operands(entry, name, dt, 'real')
        first, second = call(entry, ops, dt, beta), call(entry, ops, dt, beta)
        for x, y in zip(first, second):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_refusals_return_their_code_and_write_nothing():
    lib, ctx, _ = context()
    N, C, M, D, A, _ = ad.MATRIX['tile-plus-one']
    ops = operands('terms', 'tile-plus-one', 'f32', None)
    Vd, Rd, Wd, Hd = (dev(ops[k], 'f32') for k in ('V', 'R', 'W', 'Hp'))
    abg = torch.full((N, M, 3), PATTERN, dtype=torch.float64, device='cuda')
    a = torch.full((N, M), PATTERN, dtype=torch.float64, device='cuda')
    B = torch.full((N, M, M), PATTERN, dtype=torch.float64, device='cuda')
    flat = _lib.make_geom(N, M, C, D, A, 0)
    vol = _lib.make_geom(N, M, C, (4, 4, 4), (2, 2, 2), 0)
    huge = _lib.make_geom(1, 1, 1, (16, 16), (200, 200), 1)   # 215 rows of 268 doubles of H per tile: beyond the LDS

    def terms(g, group, beta, eps=EPS, out=abg):
        return lib.tnmf_hip_atom_terms_beta(ctx, ctypes.byref(g), group, beta, eps, p(Vd), None, p(Rd), p(Wd), p(Hd), p(out),
                                            None)

    def gram(g, group, beta, eps=EPS, out_a=a, out_B=B):
        return lib.tnmf_hip_atom_gram_beta(ctx, ctypes.byref(g), group, beta, eps, p(Vd), None, p(Rd), p(Wd), p(Hd), p(out_a),
                                           p(out_B), None)

    for g, group, beta, eps, want in ((flat, 0, 1., EPS, _lib.E_GEOM), (flat, -1, 1., EPS, _lib.E_GEOM),
                                      (flat, 2, 1., EPS, _lib.E_GEOM), (flat, M + 1, 2., EPS, _lib.E_GEOM),
                                      (flat, 1, float('nan'), EPS, _lib.E_GEOM), (flat, 1, float('inf'), EPS, _lib.E_GEOM),
                                      (flat, 1, -float('inf'), EPS, _lib.E_GEOM), (flat, 1, 1., -1e-9, _lib.E_GEOM),
                                      (flat, 1, 0., float('nan'), _lib.E_GEOM),
                                      (vol, 1, 1., EPS, _lib.E_UNSUPPORTED), (huge, 1, 1., EPS, _lib.E_UNSUPPORTED),
                                      (vol, 1, 2., EPS, _lib.E_UNSUPPORTED), (huge, 1, 2., EPS, _lib.E_UNSUPPORTED)):
        for code in (terms(g, group, beta, eps), gram(g, group, beta, eps)):
            torch.cuda.synchronize()
            assert code == want, (group, beta, eps, code, want)
        assert all(bool(torch.all(x == PATTERN)) for x in (abg, a, B))
    for name, (n, c, m, d, a_shape, group) in gd.F32_ONLY.items():   # fits beside 32 parked float rows, not beside 16 of doubles
        assert gd.plan(c, m, d, a_shape, group, 'f64')['cap'] == 0
        assert gram(_lib.make_geom(n, m, c, d, a_shape, 1), group, 1.) == _lib.E_UNSUPPORTED, name
        torch.cuda.synchronize()
        assert all(bool(torch.all(x == PATTERN)) for x in (a, B))
    assert terms(flat, 1, 1., out=None) == -1 and gram(flat, 1, 1., out_a=None) == -1 and gram(flat, 1, 1., out_B=None) == -1
    torch.cuda.synchronize()
    assert all(bool(torch.all(x == PATTERN)) for x in (abg, a, B))
    assert terms(flat, 1, 1.) == 0 and gram(flat, 1, 1.) == 0
    torch.cuda.synchronize()
    assert not any(bool(torch.any(x == PATTERN)) for x in (abg, a, B))


# -- 2. the four modes through the backend, which pads -------------------------------------------------------------------------
MODE_CASES = {
    'valid': ((4, 5), (3, 4)), 'full': ((8, 9), (8, 9)), 'circular': ((4, 5), (5, 6)), 'reflect': ((4, 5), (4, 5)),
    'valid-1d': ((9,), (4,)), 'full-1d': ((7,), (7,)), 'circular-1d': ((6,), (7,)), 'reflect-1d': ((6,), (6,)),
}


@pytest.mark.parametrize('beta', [0., 1., 1.5])
@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('name', list(MODE_CASES))
def test_the_modes_are_a_valid_pass_over_padded_activations(name, weighted, beta):
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
    Wd, Hd = torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda()
    a, b, gain = be.atom_divergence_terms(V, Wd, Hd, group, beta, EPS)
    a2, B = be.atom_divergence_gram(V, Wd, Hd, group, beta, EPS)
    Mo = P // group
    assert a.shape == b.shape == gain.shape == a2.shape == (N, Mo) and B.shape == (N, Mo, Mo)
    assert all(x.dtype == np.float64 for x in (a, b, gain, a2, B))
    parts = aref.parts_loop(W, H, D, mode, group)
    ops = dict(parts=parts, V=V, G=G, n=group * int(np.prod(A)), geometry=(N, C, P, D, A, group))
    ref = dref.terms(parts, V, G, None, beta, EPS)
    ref['B'], ref['scale_B'] = dref.gram(parts, V, G, None, beta, EPS)
    Rr = parts.sum(axis=1)
    gd_abs, gw_abs = dref.factors_abs(V, Rr, G, beta, EPS)
    flat = parts.reshape(N, Mo, -1)
    ref.update(abs_a=np.sum(parts * gd_abs[:, None], axis=tuple(range(2, parts.ndim))), Rr=Rr,
               abs_B=np.einsum('nmx,nkx->nmk', flat * gw_abs.reshape(N, 1, -1), flat))
    what = f'{name} {"weighted" if weighted else "plain"} f64 beta={beta}'
    judge_terms(what, np.stack([a, b, gain], axis=-1), ops, ref, U['f64'], beta, own_R=True, vacuous='report')
    judge_gram(what, a2, B, ops, ref, U['f64'], beta, own_R=True)
    with pytest.raises(_lib.TnmfHipError):
        be.atom_divergence_terms(V, Wd, Hd, 3, beta, EPS)
    with pytest.raises(_lib.TnmfHipError):
        be.atom_divergence_gram(V, Wd, Hd, 3, beta, EPS)


def test_the_backend_refuses_volumes():
    np.random.seed(0)
    be = HIP_Backend()
    W, H = be.initialize(np.ones((1, 1, 5, 5, 5)), (2, 2, 2), 2, None, (-3, -2, -1))
    for hook in (be.atom_divergence_terms, be.atom_divergence_gram):
        with pytest.raises(NotImplementedError, match='atom gains: 1 or 2 shift axes only'):
            hook(None, W, H, 1, 1., EPS)


# -- 3. the front end ----------------------------------------------------------------------------------------------------------
def fitted_hip(shape_V, M, A, beta, mode='valid', transforms=None, weighted=False, seed=0, dtype=np.float64, backend='hip'):
    V = (np.random.default_rng(seed).random(shape_V) + 0.05).astype(dtype)
    G = weights_of(shape_V, 'real').astype(dtype) if weighted else None
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend=backend, reconstruction_mode=mode, transforms=transforms,
                                beta_loss=beta)
    nmf.fit(V, n_iterations=3, sparsity_H=0.1, weights=G)
    return nmf, V, G


FRONT_END = {
    'valid': dict(shape_V=(3, 2, 20, 70), M=3, A=(5, 5)),
    'reflect': dict(shape_V=(3, 1, 18, 30), M=3, A=(4, 6), mode='reflect'),
    'rot90': dict(shape_V=(2, 1, 20, 20), M=2, A=(5, 5), transforms='rot90'),
    'weighted': dict(shape_V=(3, 2, 17, 65), M=3, A=(3, 4), weighted=True),
    '1d': dict(shape_V=(3, 2, 90), M=3, A=(7,), mode='circular'),
}


def objective_differences(nmf):
    """[N, n_atoms]: sample_objective() with the planes of atom m at 0, minus sample_objective(); H is restored."""
    T = nmf.n_transforms
    base = nmf.sample_objective()
    out = []
    for m in range(nmf.n_atoms):
        keep = nmf._H[:, m * T:(m + 1) * T].clone()
        nmf._H[:, m * T:(m + 1) * T] = 0.
        try:
            out.append(nmf.sample_objective() - base)
        finally:
            nmf._H[:, m * T:(m + 1) * T] = keep
    return np.stack(out, axis=1)


@pytest.mark.parametrize('beta', [1., 0.], ids=['KL', 'IS'])
@pytest.mark.parametrize('name', list(FRONT_END))
def test_the_gain_is_the_difference_of_two_objectives_after_a_fit(name, beta):
    """float64.  The difference of two objectives limits the agreement: the bar is ten times what the float64 host
    fallback, on the same (W, H), misses the same differences by."""
    nmf, V, G = fitted_hip(beta=beta, **FRONT_END[name])
    before = [np.array(x) for x in (nmf.W, nmf.H)]
    got = nmf.atom_divergence_gains(per_sample=True)
    assert got.shape == (V.shape[0], nmf.n_atoms) and got.dtype == np.float64
    want = objective_differences(nmf)
    host = atom_divergence_terms_numpy(nmf._backend.to_ndarray(nmf._W_dict), nmf._backend.to_ndarray(nmf._H), nmf._mode, V,
                                       G, nmf.n_transforms, beta, nmf.eps)[2]
    size = float(np.max(np.abs(want)))
    miss_host, miss_hip = float(np.max(np.abs(host - want))) / size, float(np.max(np.abs(got - want))) / size
    print(f'atom divergence gains {name} beta={beta}: relative distance to the difference of two objectives: '
          f'hip {miss_hip:.3e}, float64 host fallback {miss_host:.3e}')
    assert miss_hip <= 10 * miss_host, (name, beta, miss_hip, miss_host)
    np.testing.assert_array_equal(nmf.atom_divergence_gains(), got.sum(axis=0))
    a, b = nmf.atom_divergence_terms()
    B = nmf.atom_divergence_gram(per_sample=True)
    assert a.shape == b.shape == got.shape and B.shape == got.shape + (nmf.n_atoms,)
    np.testing.assert_array_equal(nmf.atom_divergence_gram(), B.sum(axis=0))
    for was, now in zip(before, (nmf.W, nmf.H)):
        np.testing.assert_array_equal(was, now)


@pytest.mark.parametrize('beta', [1., 0.], ids=['KL', 'IS'])
@pytest.mark.parametrize('name', ['valid', 'weighted', '1d'])
def test_a_float32_fit_against_the_reference_on_the_librarys_reconstruction(name, beta):
    """The reference evaluated on ``nmf.R`` (float32, the library's own) under the derived bounds.  A real fit can hold
    pixels that one atom explains alone, where the gain's bound is as large as the term: reported, not asserted."""
    kw = FRONT_END[name]
    nmf, V, G = fitted_hip(beta=beta, dtype=np.float32, **kw)
    W, H = nmf._backend.to_ndarray(nmf._W_dict).astype(np.float64), nmf._backend.to_ndarray(nmf._H).astype(np.float64)
    D, A = V.shape[2:], tuple(kw['A'])
    parts = aref.parts_loop(W, H, D, nmf._mode, nmf.n_transforms)
    R = nmf.R.astype(np.float64)
    Vd, Gd = V.astype(np.float64), None if G is None else G.astype(np.float64)
    ref = dref.terms(parts, Vd, Gd, R, beta, nmf.eps)
    ref['B'], ref['scale_B'] = dref.gram(parts, Vd, Gd, R, beta, nmf.eps)
    ref.update(abs_a=np.zeros_like(ref['a']), abs_B=np.zeros_like(ref['B']), Rr=R)
    ops = dict(parts=parts, V=Vd, G=Gd, n=nmf.n_transforms * int(np.prod(A)),
               geometry=(V.shape[0], V.shape[1], W.shape[0], D, A, nmf.n_transforms))
    a, b = nmf.atom_divergence_terms()
    gain = nmf.atom_divergence_gains(per_sample=True)
    judge_terms(f'fit {name} f32 beta={beta}', np.stack([a, b, gain], axis=-1), ops, ref, U['f32'], beta, vacuous='report')
    judge_gram(f'fit {name} f32 beta={beta}', a, nmf.atom_divergence_gram(per_sample=True), ops, ref, U['f32'], beta)


def test_at_beta_2_the_front_end_is_the_frobenius_family_bit_for_bit():
    nmf, _, _ = fitted_hip(beta=2., dtype=np.float32, **FRONT_END['weighted'])
    for got, want in zip(nmf.atom_divergence_terms(), nmf.atom_terms()):
        assert got.tobytes() == want.tobytes()
    for per_sample in (False, True):
        assert nmf.atom_divergence_gains(per_sample).tobytes() == nmf.atom_gains(per_sample).tobytes()
        assert nmf.atom_divergence_gram(per_sample).tobytes() == nmf.atom_gram(per_sample).tobytes()
    # and so are the backend's hooks asked for beta 2
    be = nmf._backend
    a, b, gain = be.atom_divergence_terms(nmf._V, nmf._W_dict, nmf._H, 1, 2., nmf.eps)
    a0, b0 = be.atom_terms(nmf._V, nmf._W_dict, nmf._H, 1)
    assert a.tobytes() == a0.tobytes() and b.tobytes() == b0.tobytes() and gain.tobytes() == (a0 + b0 / 2).tobytes()


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_a_used_context_gives_the_bits_of_a_fresh_one(dtype):
    """Both entries after a fit, after atom_terms() and after atom_gram() on the same backend (all four share the work
    buffer of the context) against a backend that has run nothing else."""
    def results(nmf):
        return (nmf.atom_divergence_gains(per_sample=True),) + nmf.atom_divergence_terms() + (
            nmf.atom_divergence_gram(per_sample=True),)

    kw = dict(FRONT_END['valid'], dtype=dtype)
    used, _, _ = fitted_hip(beta=2., **dict(kw, M=8))   # a larger Frobenius model first, on the backend that stays
    used.atom_terms(), used.atom_gram()
    backend = used._backend
    used, _, _ = fitted_hip(beta=1., backend=backend, **kw)
    be = used._backend
    assert be is backend
    be.atom_terms(used._V, used._W_dict, used._H, 1), be.atom_gram(used._V, used._W_dict, used._H, 1)
    after = results(used)
    fresh, _, _ = fitted_hip(beta=1., **kw)
    assert fresh._backend is not backend
    np.testing.assert_array_equal(used.H, fresh.H)
    for x, y in zip(after, results(fresh)):
        assert np.all(np.isfinite(x)) and x.tobytes() == y.tobytes()
