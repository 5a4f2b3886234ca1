"""
Sources on the GPU: tnmf_hip_atom_sources through the C ABI on operands made on the host, ``HIP_Backend.source_parts`` /
``dominant_parts`` in the four reconstruction modes, and ``separate`` / ``dominant_source`` on ``backend='hip'``.

The reference (tests/sources_reference.py) is evaluated in float64 on the operands as rounded to the element type.  The
bounds are derived from the kernel's order of operations (tnmf_amd/csrc/sources.hip, atom_walk.h), not measured.  With
u = 2^-24 (f32) or 2^-53 (f64), n_g = (planes of source g) * prod(A) and n_max the largest such count over the groups,
the hidden group of the unlisted planes included:

  r_g    per pixel two chains of fused multiply-adds, over the even and the odd elements of the thread's window, and one
         add of the two.  All terms are >= 0, so every rounding is relative to a partial sum <= the final one; a product
         with a zero (a zero of H, the zero padding of a tap row) leaves the sum as it is, exactly.  The two chains hold
         n_g non-zero products together: relative error <= (n_g + 1) u, within the (n_g + 8) u the tests hold.
  total  0 + r_0 is exact, then S adds of sums with relative error <= (n_max + 1) u: <= (n_max + S + 1) u.
  mask   total + eps (one rounding), one correctly rounded division: <= (n_g + n_max + S + 4) u; masked: one product more,
         <= (n_g + n_max + S + 5) u, within the (n_g + n_max + S + 8) u the tests hold.
  share  the same on the channel sums of W, whose C - 1 adds put (C - 1) u on numerator and denominator each:
         <= (max n_g + n_max + S + 8 + 2 (C - 1)) u.  With integer operands only total + eps and the division round: 2 u.

(First order in u; the second-order terms are below 1e-3 of the bounds at these sizes.)  Every test prints the largest
ratio of an error to its bound.

The shapes are those of tests/atoms_dispatch.py: the smallest that reach every branch of the walk.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import atoms_dispatch as ad
import events_reference as eref
import sources_reference as sref
from test_atom_gains_cpu import _AtomStub, weights_of
from test_hip_atom_gains import DTYPES, NP, PATTERN, U, context, dev, p, padded_rows, rounded
from tnmf_amd import _lib
from tnmf_amd.atoms_host import pad_activations_numpy
from tnmf_amd.backends.HIP import HIP_Backend
from tnmf_amd.sources_host import source_tables
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

pytestmark = pytest.mark.gpu

SHAPES = ['one-tile', 'tile-plus-one', 'below-halo', 'atom-12x12', 'tall-atom', 'channels-5', '1d-50', '1d-tile-plus-one',
          '1d-many-atoms']
LAYOUTS = ['each', 'interleaved', 'all']
EMIT = _lib.SOURCE_OUTPUTS
EPS = 1e-9


def plane_sets(M, layout):
    """The three source layouts over M planes: every plane on its own; the even and the odd planes with the last plane
    unlisted (M >= 3); one source of all planes, listed from the last to the first."""
    if layout == 'each':
        return [[m] for m in range(M)]
    if layout == 'interleaved':
        return [list(range(0, M - 1, 2)), list(range(1, M - 1, 2))]
    return [list(range(M - 1, -1, -1))]


@functools.lru_cache(maxsize=None)
def operands(name, dt):
    """-> dict of read-only float64 arrays holding values of the element type: padded activations Hp (values >= 0.1 or
    exactly 0, whole planes of zeros among them), W >= 0.1, V."""
    N, C, M, D, A, _ = ad.MATRIX[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    Hp = (rng.random((N, M) + tuple(d + a - 1 for d, a in zip(D, A))) + 0.1) * (rng.random((N, M) + (1,) * len(D)) > 0.15)
    Hp = rounded(Hp * (rng.random(Hp.shape) > 0.3), dt)
    W = rounded(rng.random((M, C) + A) + 0.1, dt)
    V = rounded(rng.random((N, C) + D) + 0.1, dt)
    out = dict(Hp=Hp, W=W, V=V)
    for x in out.values():
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name, dt, layout):
    ops = operands(name, dt)
    want = sref.outputs(ops['W'], ops['Hp'], ops['V'], plane_sets(ad.MATRIX[name][2], layout), float(NP[dt](EPS)))
    for x in want.values():
        x.setflags(write=False)
    return want


def call(name, dt, ops, sets, emit, stride=False, eps=EPS, tables='device', frame=0):
    """-> (code, out | (label, share)) of one call on outputs filled with PATTERN (labels: -7).  ``frame``: that many
    elements of PATTERN in front of and behind ``out``, returned with it."""
    N, C, M, D, A, _ = ad.MATRIX[name]
    lib, ctx, _ = context()
    H, ld = padded_rows(ops['Hp'], dt) if stride else (dev(ops['Hp'], dt), 0)
    g = _lib.make_geom(N, M, C, D, A, DTYPES.index(dt), ld)
    order, start = source_tables(sets)
    if tables == 'device':
        order_t, start_t = torch.from_numpy(order).cuda(), torch.from_numpy(start).cuda()
        po, ps = p(order_t), p(start_t)
    else:
        po, ps = order.ctypes.data_as(ctypes.c_void_p), start.ctypes.data_as(ctypes.c_void_p)
    Vd, Wd = dev(ops['V'], dt), dev(ops['W'], dt)
    S = len(sets)
    tdt = torch.float32 if dt == 'f32' else torch.float64
    if emit == 'dominant':
        label = torch.full((N,) + D, -7, dtype=torch.int32, device='cuda')
        share = torch.full((N,) + D, PATTERN, dtype=tdt, device='cuda')
        code = lib.tnmf_hip_atom_sources(ctx, ctypes.byref(g), S, po, len(order), ps, EMIT[emit], eps, p(Vd), p(Wd), p(H),
                                         None, p(label), p(share), None)
        torch.cuda.synchronize()
        return code, (label.cpu().numpy(), share.cpu().numpy())
    n_out = N * S * C * int(np.prod(D))
    buf = torch.full((n_out + 2 * frame,), PATTERN, dtype=tdt, device='cuda')
    out = buf[frame:frame + n_out]
    code = lib.tnmf_hip_atom_sources(ctx, ctypes.byref(g), S, po, len(order), ps, EMIT[emit], eps, p(Vd), p(Wd), p(H),
                                     p(out), None, None, None)
    torch.cuda.synchronize()
    if frame:
        return code, buf.cpu().numpy()
    return code, out.cpu().numpy().reshape((N, S, C) + D)


def counts(name, sets):
    """(n_g [S], n_max): multiply-adds behind a pixel of each source, and the most of any group, the hidden one included."""
    N, C, M, D, A, _ = ad.MATRIX[name]
    nA = int(np.prod(A))
    n_g = np.array([len(s) * nA for s in sets])
    return n_g, max(int(n_g.max()), (M - sum(len(s) for s in sets)) * nA)


def ratio(got, want, bound):
    """The largest |got - want| / bound; a bound of 0 asks for an exact 0."""
    assert np.all(np.isfinite(got)) and not np.any(got == PATTERN)
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err[bound == 0] == 0)
    return float(np.max(err[bound > 0] / bound[bound > 0], initial=0.))


# -- 1. the derived rounding bound, every branch of the walk -----------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('name', SHAPES)
def test_every_branch_of_the_walk_within_the_derived_bound(name, layout, dt):
    N, C, M, D, A, _ = ad.MATRIX[name]
    ops, sets, want, u = operands(name, dt), plane_sets(M, layout), expected(name, dt, layout), U[dt]
    n_g, n_max = counts(name, sets)
    S = len(sets)
    per_source = n_g.reshape((1, S, 1) + (1,) * len(D))
    worst = {}
    for emit in ('contribution', 'mask', 'masked'):
        code, got = call(name, dt, ops, sets, emit, stride=True)   # (a NaN-filled row pad throughout)
        assert code == 0
        ref = want[emit]
        bound = ((per_source + 8) if emit == 'contribution' else (per_source + n_max + S + 8)) * u * np.abs(ref)
        worst[emit] = ratio(got, ref, bound)
        if emit == 'mask':
            assert np.all(got >= 0) and np.all(got <= 1)   # no tolerance: r_g <= total in the pass's own sums
        if emit == 'masked':
            assert np.all(got >= 0) and np.all(got <= ops['V'][:, None].astype(NP[dt]))
    code, (label, share) = call(name, dt, ops, sets, 'dominant', stride=True)
    assert code == 0 and not np.any(label == -7)
    worst['share'] = ratio(share, want['share'], (n_max + int(n_g.max()) + S + 8 + 2 * (C - 1)) * u * want['share'])
    # a label may differ from the reference only where two sources are within rounding of each other
    rc = want['contribution'].sum(axis=2)
    differ = label != want['label']
    if differ.any():
        chosen = np.take_along_axis(rc, np.maximum(label, 0)[:, None].astype(np.int64), axis=1)[:, 0]
        assert np.all(label[differ] >= 0)
        assert np.all((rc.max(axis=1) - chosen)[differ] <= 2 * (n_max + C + 8) * u * rc.max(axis=1)[differ])
    print(f'sources {name} {layout} {dt}: largest error / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1., worst


# -- 2. exact cases: small integers, every sum exact in float32 ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def integer_operands(name):
    N, C, M, D, A, _ = ad.MATRIX[name]
    rng = np.random.default_rng(11)
    Hp = rng.integers(0, 4, (N, M) + tuple(d + a - 1 for d, a in zip(D, A))).astype(np.float64)
    Hp *= rng.random(Hp.shape) > 0.5
    W = rng.integers(0, 4, (M, C) + A).astype(np.float64)
    # planted: planes 0 and 1 alike (ties between the sources that hold them), and a block of pixels nobody explains
    W[1], Hp[:, 1] = W[0], Hp[:, 0]
    Hp[0, ..., : A[-1] + 3] = 0.
    V = rng.integers(0, 9, (N, C) + D).astype(np.float64)
    return dict(Hp=Hp, W=W, V=V)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', ['tile-plus-one', 'channels-5', '1d-50'])
def test_integer_operands_give_exact_contributions_labels_and_ties(name, dt):
    N, C, M, D, A, _ = ad.MATRIX[name]
    ops = integer_operands(name)
    sets = plane_sets(M, 'each')
    want = sref.outputs(ops['W'], ops['Hp'], ops['V'], sets, float(NP[dt](EPS)))
    assert want['total'].max() < 2 ** 24 and np.any(want['label'] == -1)
    rc = want['contribution'].sum(axis=2)
    assert np.any((rc[:, 0] == rc[:, 1]) & (want['label'] == 0))   # a planted tie that the lowest index wins
    code, got = call(name, dt, ops, sets, 'contribution')
    assert code == 0
    np.testing.assert_array_equal(got, want['contribution'])
    np.testing.assert_array_equal(got.astype(np.float64).sum(axis=1), want['total'])   # a partition: the parts add to R
    code, (label, share) = call(name, dt, ops, sets, 'dominant')
    assert code == 0
    np.testing.assert_array_equal(label, want['label'])
    worst = ratio(share, want['share'], 2 * U[dt] * want['share'])
    print(f'sources {name} {dt} integer operands: share, largest error / (2 u share): {worst:.3f}')
    assert worst <= 1.
    # the masks of a pixel nobody explains are 0, with eps = 0 as well
    code, mask = call(name, dt, ops, sets, 'mask', eps=0.)
    assert code == 0 and np.all(mask[(want['total'] == 0)[:, None].repeat(len(sets), axis=1)] == 0) and np.all(mask <= 1)


# -- 3. properties -------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bits_and_the_tables_may_live_on_the_host():
    for name, dt, layout in (('tile-plus-one', 'f32', 'interleaved'), ('atom-12x12', 'f32', 'each'),
                             ('1d-many-atoms', 'f64', 'interleaved')):
        ops, sets = operands(name, dt), plane_sets(ad.MATRIX[name][2], layout)
        first, second = call(name, dt, ops, sets, 'masked')[1], call(name, dt, ops, sets, 'masked')[1]
        assert first.tobytes() == second.tobytes()
        assert first.tobytes() == call(name, dt, ops, sets, 'masked', tables='host')[1].tobytes()
        np.testing.assert_array_equal(first, call(name, dt, ops, sets, 'masked', stride=True)[1])
        a, b = call(name, dt, ops, sets, 'dominant')[1], call(name, dt, ops, sets, 'dominant')[1]
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize('frame', [4096, 4097])
@pytest.mark.parametrize('name', ['tile-plus-one', 'one-tile', '1d-50'])
def test_nothing_outside_the_output_is_written(name, frame):
    # (one-tile, D_x a multiple of four: one aligned store per thread, unless the output itself is not aligned -- frame
    # 4097; the other shapes store pixel by pixel)
    N, C, M, D, A, _ = ad.MATRIX[name]
    ops, sets = operands(name, 'f32'), plane_sets(M, 'interleaved')
    for emit in ('contribution', 'masked'):
        code, buf = call(name, 'f32', ops, sets, emit, frame=frame)
        assert code == 0
        assert np.all(buf[:frame] == PATTERN) and np.all(buf[-frame:] == PATTERN)
        assert not np.any(buf[frame:-frame] == PATTERN)


def test_refusals_return_their_code_and_write_nothing():
    lib, ctx, _ = context()
    name = 'tile-plus-one'
    N, C, M, D, A, _ = ad.MATRIX[name]
    ops = operands(name, 'f32')
    Vd, Wd, Hd = (dev(ops[k], 'f32') for k in ('V', 'W', 'Hp'))
    out = torch.full((N, M, C) + D, PATTERN, dtype=torch.float32, device='cuda')
    label = torch.full((N,) + D, -7, dtype=torch.int32, device='cuda')
    share = torch.full((N,) + D, PATTERN, dtype=torch.float32, device='cuda')
    flat = _lib.make_geom(N, M, C, D, A, 0)
    vol = _lib.make_geom(N, M, C, (4, 4, 4), (2, 2, 2), 0)
    huge = _lib.make_geom(1, 1, 1, (16, 16), (200, 200), 1)   # beyond the LDS limit of tnmf_hip_atom_terms
    ints = lambda *x: torch.tensor(x, dtype=torch.int32, device='cuda')   # noqa: E731
    good = (M, ints(0, 1, 2), 3, ints(0, 1, 2, 3))
    cases = [
        (flat, (2, ints(0, 1, 1), 3, ints(0, 1, 3)), 0, _lib.E_GEOM),      # a plane listed twice
        (flat, (2, ints(0, 3), 2, ints(0, 1, 2)), 0, _lib.E_GEOM),         # a plane out of range
        (flat, (2, ints(0, -1), 2, ints(0, 1, 2)), 0, _lib.E_GEOM),
        (flat, (2, ints(0, 1), 2, ints(0, 2, 2)), 0, _lib.E_GEOM),         # source_start not ascending: an empty source
        (flat, (2, ints(0, 1), 2, ints(0, 2, 1)), 0, _lib.E_GEOM),
        (flat, (2, ints(0, 1), 2, ints(1, 1, 2)), 0, _lib.E_GEOM),         # does not start at 0
        (flat, (2, ints(0, 1, 2), 3, ints(0, 1, 2)), 0, _lib.E_GEOM),      # does not end at n_listed
        (flat, (0, ints(0), 0, ints(0)), 0, _lib.E_GEOM),                  # no source
        (flat, (1, ints(0, 1, 2, 0), 4, ints(0, 4)), 0, _lib.E_GEOM),      # more planes listed than there are
        (flat, good, 4, _lib.E_GEOM), (flat, good, -1, _lib.E_GEOM),       # an unknown emit
        (vol, good, 0, _lib.E_UNSUPPORTED), (huge, (1, ints(0), 1, ints(0, 1)), 0, _lib.E_UNSUPPORTED),
        (huge, (1, ints(0), 1, ints(0, 1)), 3, _lib.E_UNSUPPORTED),
    ]
    for g, (S, order, n_listed, start), emit, want in cases:
        code = lib.tnmf_hip_atom_sources(ctx, ctypes.byref(g), S, p(order), n_listed, p(start), emit, EPS, p(Vd), p(Wd),
                                         p(Hd), p(out), p(label), p(share), None)
        torch.cuda.synchronize()
        assert code == want, (S, n_listed, emit, code, want)
        assert bool(torch.all(out == PATTERN)) and bool(torch.all(label == -7)) and bool(torch.all(share == PATTERN))
    S, order, n_listed, start = good
    args = lambda **k: [k.get(x, y) for x, y in (('V', p(Vd)), ('W', p(Wd)), ('H', p(Hd)), ('out', p(out)),   # noqa: E731
                                                  ('label', p(label)), ('share', p(share)))] + [None]
    for emit, missing in ((0, 'out'), (2, 'V'), (0, 'W'), (0, 'H'), (3, 'label'), (3, 'share')):
        code = lib.tnmf_hip_atom_sources(ctx, ctypes.byref(flat), S, p(order), n_listed, p(start), emit, EPS,
                                         *args(**{missing: None}))
        assert code == -1, (emit, missing, code)
    for po, ps in ((None, p(start)), (p(order), None)):
        assert lib.tnmf_hip_atom_sources(ctx, ctypes.byref(flat), S, po, n_listed, ps, 0, EPS, *args()) == -1
    assert lib.tnmf_hip_atom_sources(ctx, ctypes.byref(flat), S, p(order), n_listed, p(start), 0, -1., *args()) == _lib.E_GEOM
    torch.cuda.synchronize()
    assert bool(torch.all(out == PATTERN)) and bool(torch.all(label == -7)) and bool(torch.all(share == PATTERN))
    assert lib.tnmf_hip_atom_sources(ctx, ctypes.byref(flat), S, p(order), n_listed, p(start), 0, EPS, *args()) == 0
    torch.cuda.synchronize()
    assert not bool(torch.any(out == PATTERN)) and bool(torch.all(label == -7))


# -- 4. through the layers -------------------------------------------------------------------------------------------------------
MODE_CASES = {
    'valid': ((4, 5), (3, 4)), 'full': ((8, 9), (8, 9)), 'circular': ((4, 5), (5, 6)), 'reflect': ((4, 5), (4, 5)),
    'valid-1d': ((9,), (4,)), 'full-1d': ((7,), (7,)), 'circular-1d': ((6,), (7,)), 'reflect-1d': ((6,), (6,)),
}


@pytest.mark.parametrize('name', list(MODE_CASES))
def test_the_modes_are_a_valid_pass_over_padded_activations(name):
    mode = name.split('-')[0]
    D, A = MODE_CASES[name]
    N, C, P = 2, 2, 4
    rng = np.random.default_rng(5)
    V = rng.random((N, C) + D) + 0.05
    np.random.seed(0)
    be = HIP_Backend(reconstruction_mode=mode, path='generic')
    be.initialize(V, A, P, None, tuple(range(-len(A), 0)))
    H = rng.random((N, P) + eref.shift_shape(D, A, mode))
    W = rng.random((P, C) + A) + 0.1
    sets = [[2, 0], [3]]
    order, start = source_tables(sets)
    want = sref.outputs(W, pad_activations_numpy(H, A, mode), V, sets, EPS)
    Wd, Hd = torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda()
    nA, u = int(np.prod(A)), U['f64']
    worst = {}
    for output in ('contribution', 'mask', 'masked'):
        got = be.source_parts(V, Wd, Hd, order, start, output, eps=EPS)
        assert got.is_cuda and tuple(got.shape) == (N, 2, C) + D
        n_g = np.array([2 * nA, nA]).reshape((1, 2, 1) + (1,) * len(D))
        bound = ((n_g + 8) if output == 'contribution' else (n_g + 2 * nA + 2 + 8)) * u * np.abs(want[output])
        worst[output] = ratio(got.cpu().numpy(), want[output], bound)
    label, share = be.dominant_parts(V, Wd, Hd, order, start, eps=EPS)
    assert label.dtype == torch.int32
    np.testing.assert_array_equal(label.cpu().numpy(), want['label'])
    worst['share'] = ratio(share.cpu().numpy(), want['share'], (4 * nA + 2 + 8 + 2) * u * want['share'])
    print(f'sources backend {name} f64: largest error / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1., worst


def test_the_backend_refuses_volumes_and_turns_unsupported_into_not_implemented():
    np.random.seed(0)
    be = HIP_Backend()
    W, H = be.initialize(np.ones((1, 1, 5, 5, 5)), (2, 2, 2), 2, None, (-3, -2, -1))
    with pytest.raises(NotImplementedError, match='separate: 1 or 2 shift axes only'):
        be.source_parts(None, W, H, [0, 1], [0, 1, 2], 'mask')
    with pytest.raises(NotImplementedError, match='separate: 1 or 2 shift axes only'):
        be.dominant_parts(None, W, H, [0, 1], [0, 1, 2])
    np.random.seed(0)
    be = HIP_Backend()   # 215 rows of 268 doubles of H per tile: beyond the LDS
    W, H = be.initialize(np.ones((1, 1, 16, 16)), (200, 200), 1, None, (-2, -1))
    with pytest.raises(NotImplementedError):
        be.source_parts(None, W, H, [0], [0, 1], 'mask')


FRONT_END = {
    'kullback-leibler': dict(shape_V=(3, 2, 20, 70), M=3, A=(5, 5), beta_loss='kullback-leibler'),
    'weighted': dict(shape_V=(3, 2, 17, 65), M=3, A=(3, 4), weighted=True),
    'rot90': dict(shape_V=(2, 1, 20, 20), M=2, A=(5, 5), transforms='rot90'),
    'plain': dict(shape_V=(3, 1, 18, 32), M=3, A=(4, 6), mode='reflect'),
    '1d': dict(shape_V=(3, 2, 90), M=3, A=(7,), mode='circular'),
}


def fitted_pair(shape_V, M, A, mode='valid', transforms=None, weighted=False, beta_loss='frobenius'):
    """A model fitted on backend='hip' in float64 and a model on the oracle backend, which has no hook, with its (W, H)."""
    V = np.random.default_rng(0).random(shape_V) + 0.05
    G = weights_of(shape_V, 'mask') if weighted else None
    np.random.seed(42)
    hip = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip', reconstruction_mode=mode, transforms=transforms,
                                beta_loss=beta_loss)
    hip.fit(V, n_iterations=3, sparsity_H=0.1, weights=G)
    np.random.seed(42)
    cpu = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend=_AtomStub(mode), transforms=transforms)
    cpu.fit(V, n_iterations=0, weights=G)
    cpu._W[...] = hip.W
    cpu._H[...] = hip._backend.to_ndarray(hip._H)
    cpu._expand_W()
    return hip, cpu, G


@pytest.mark.parametrize('name', list(FRONT_END))
def test_separate_on_hip_equals_the_host_fallback_within_the_bound(name):
    hip, cpu, G = fitted_pair(**FRONT_END[name])
    assert hip._backend.supports_sources and not getattr(cpu._backend, 'supports_sources', False)
    before = [np.array(x) for x in (hip.W, hip.H)]
    M, T, nA, u = hip.n_atoms, hip.n_transforms, int(np.prod(hip.atom_shape)), U['f64']
    worst = {}
    for sources in (None, [[M - 1], [0]]):
        sets = [[m] for m in range(M)] if sources is None else sources
        S, n_max = len(sets), T * nA * max(1, M - len(sets))
        for output in ('contribution', 'mask', 'masked'):
            got, want = hip.separate(sources, output=output), cpu.separate(sources, output=output)
            assert got.shape == want.shape == (hip.V.shape[0], S) + hip.V.shape[1:] and got.dtype == hip.V.dtype
            n = (T * nA + 8) if output == 'contribution' else (T * nA + n_max + S + 8)
            key = f'{output}{"" if sources is None else " (two sources)"}'
            worst[key] = ratio(got, want.astype(np.float64), n * u * np.abs(want))
        label, share = hip.dominant_source(sources)
        want_label, want_share = cpu.dominant_source(sources)
        np.testing.assert_array_equal(label, want_label)
        C = hip.V.shape[1]
        worst[f'share{"" if sources is None else " (two sources)"}'] = ratio(
            share, want_share.astype(np.float64), (T * nA + n_max + S + 8 + 2 * (C - 1)) * u * want_share)
    if G is not None:
        hidden = np.broadcast_to((G == 0)[:, None], hip.separate().shape)
        assert hidden.any() and np.all(hip.separate()[hidden] == 0.)
        assert np.all(hip.separate(output='contribution')[hidden] > 0.)
    print(f'separate {name}: largest difference to the float64 fallback / bound: '
          + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1., worst
    for was, now in zip(before, (hip.W, hip.H)):
        np.testing.assert_array_equal(was, now)


def test_float32_through_the_front_end_keeps_the_masks_in_range():
    V = (np.random.default_rng(1).random((4, 1, 128, 128)) ** 4).astype(np.float32)   # (dark nearly everywhere)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=8, atom_shape=(5, 5), backend='hip')
    nmf.fit(V, n_iterations=3, sparsity_H=0.1)
    assert nmf._backend.last_path == 'fft'   # the route on which R_partial's error is absolute
    mask, masked = nmf.separate(output='mask'), nmf.separate([[0, 1, 2, 3], [4, 5, 6, 7]])
    assert mask.dtype == np.float32 and np.all(mask >= 0) and np.all(mask <= 1)
    assert np.all(masked >= 0) and np.all(masked <= V[:, None])
    # over a partition the estimates add up to V R / (R + eps) with R the pass's own total: against the exact sum of the
    # stored contributions the kernel's total rounds once (two sources), total + eps, the division and the product once
    # each -- 4 u on every estimate, first order; the bar is 5 u V
    parts = nmf.separate([[0, 1, 2, 3], [4, 5, 6, 7]], output='contribution').astype(np.float64)
    total = parts.sum(axis=1)
    err = np.abs(masked.astype(np.float64).sum(axis=1) - V * total / (total + np.float64(np.float32(nmf.eps))))
    print(f'separate f32: sum of the estimates against V R / (R + eps): largest error / (5 u V) '
          f'{float(np.max(err[V > 0] / (5 * U["f32"] * V[V > 0]))):.3f}')
    assert np.all(err <= 5 * U['f32'] * V)
