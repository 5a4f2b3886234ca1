"""Atom operators (TransformInvariantNMF(..., transforms=AtomOperators)) without a GPU: the built-in maps against their
definitions and the permutation groups, the fold as the adjoint of the expansion, the refusals, the front end's schedules on
a float64 stub backend against the dense reference of tests/operator_reference.py, the planted motifs whose margins are
fixed there, and the ABI of the operator entry points."""
import os

import numpy as np
import pytest

import operator_reference as oref
import transform_reference as tref
import weighted_reference as wref
from oracle import tnmf_oracle as orc
from oracle_backend import OracleBackend
from tnmf_amd import _lib, sharding, transforms as tr
from tnmf_amd.backends._Backend import Backend, sliceNone
from tnmf_amd.TransformInvariantNMF import MiniBatchAlgorithm, TransformInvariantNMF

GROUPS = ['flip', 'mirrors', 'rot90', 'dihedral']


def dense(ops):
    return oref.dense(ops)


# -- the built-in maps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('A', [(5, 5), (6, 6), (1, 1), (12, 12)])
def test_quarter_turns_are_the_rot90_group_exactly(A):
    G = tr.from_group('rot90', A)
    R4 = tr.rotations(A, 4)
    R8 = tr.rotations(A, 8)
    assert np.array_equal(dense(R4), dense(G)) and R4 == G
    assert np.array_equal(dense(R8)[::2], dense(G))
    assert all(np.array_equal(x, y) for x, y in zip(R4.entries, G.entries))
    a = np.random.default_rng(0).random(A)
    for k in range(4):
        assert np.array_equal(R4.expand(a[None, None])[k, 0], np.rot90(a, k))


@pytest.mark.parametrize('A', [(5, 5), (4, 7), (9,), (1,)])
def test_the_identities(A):
    eye = np.eye(int(np.prod(A)))
    assert np.array_equal(dense(tr.scales(A, [1.]))[0], eye)
    if len(A) == 2:
        assert np.array_equal(dense(tr.rotations(A, 1))[0], eye)
        assert np.array_equal(dense(tr.rotations(A, 8))[0], eye)
    assert tr.scales(A, [1.]).T == 1 and tr.scales(A, [1., 2.]).T == 2


BUILTINS = {
    'rot8_9x9': lambda: tr.rotations((9, 9), 8),
    'rot12_4x7': lambda: tr.rotations((4, 7), 12),
    'rot5_6x6': lambda: tr.rotations((6, 6), 5),
    'scales_2d': lambda: tr.scales((8, 8), [1., .8, .64, .3, 1.25, 2.]),
    'scales_1d': lambda: tr.scales((15,), [1., .75, .5, 1.5, 1 / 3]),
    'compose': lambda: tr.compose(tr.rotations((12, 12), 8), tr.scales((12, 12), [1., .8, .64])),
}


@pytest.mark.parametrize('name', list(BUILTINS))
def test_builtin_weights_are_non_negative_and_rows_sum_to_at_most_one(name):
    ops = BUILTINS[name]()
    t, o, i, w = ops.entries
    assert np.all(w >= 1e-12) and np.all(np.isfinite(w))
    L = dense(ops)
    assert L.sum(axis=-1).max() <= 1. + 1e-12
    # the interior of the atom keeps its mass under a rotation (all four bilinear taps inside)
    if name.startswith('rot'):
        A = ops.atom_shape
        c = (A[0] // 2) * A[1] + A[1] // 2
        assert np.all(np.abs(L[:, c].sum(axis=-1) - 1.) <= 1e-12)


def test_the_sampling_definition():
    """out[p] samples the source at c + R(-theta)(p - c)/s, bilinear; s < 1 averages ceil(1/s)^2 sub-points."""
    A = (7, 7)
    a = np.random.default_rng(1).random(A)
    theta = 2 * np.pi / 12
    got = tr.rotations(A, 12).expand(a[None, None])[1, 0]
    c = 3.
    for py, px in [(3, 3), (2, 4), (3, 5), (5, 1)]:
        dy, dx = py - c, px - c
        sy = c + np.cos(theta) * dy + np.sin(theta) * dx
        sx = c - np.sin(theta) * dy + np.cos(theta) * dx
        y0, x0 = int(np.floor(sy)), int(np.floor(sx))
        fy, fx = sy - y0, sx - x0
        want = ((1 - fy) * (1 - fx) * a[y0, x0] + (1 - fy) * fx * a[y0, x0 + 1] + fy * (1 - fx) * a[y0 + 1, x0]
                + fy * fx * a[y0 + 1, x0 + 1])
        assert abs(got[py, px] - want) <= 1e-14
    # 1-D, s = 1/2: output pixel p averages the linear samples at c + (p - 1/4 - c) * 2 and c + (p + 1/4 - c) * 2
    b = np.arange(9.) ** 2
    half = tr.scales((9,), [.5]).expand(b[None, None])[0, 0]
    assert half[4] == pytest.approx(np.mean([np.interp(4 - .5, np.arange(9), b), np.interp(4 + .5, np.arange(9), b)]))
    assert half[0] == pytest.approx(0.)          # (both samples fall left of the atom)
    # magnification: the centre pixel stays, its neighbour samples halfway
    dbl = tr.scales((9,), [2.]).expand(b[None, None])[0, 0]
    assert dbl[4] == b[4] and dbl[5] == pytest.approx((b[4] + b[5]) / 2)


def test_compose_applies_the_inner_map_first():
    A = (6, 6)
    outer, inner = tr.rotations(A, 3), tr.scales(A, [1., .7])
    C = tr.compose(outer, inner)
    assert C.T == 6
    Lo, Li, Lc = dense(outer), dense(inner), dense(C)
    for i in range(3):
        for j in range(2):
            assert np.abs(Lc[i * 2 + j] - Lo[i] @ Li[j]).max() <= 1e-15
    assert tr.compose(tr.from_group('flip', A), tr.from_group('flip', A)) == tr.AtomOperators.from_dense(
        np.stack([dense(tr.from_group('flip', A))[k] @ dense(tr.from_group('flip', A))[j]
                  for k in range(2) for j in range(2)]).reshape((4,) + A * 2))


@pytest.mark.parametrize('name', GROUPS)
def test_from_group_equals_the_group_bit_for_bit(name):
    rng = np.random.default_rng(2)
    for A in ((5, 5), (3, 4), (7,)):
        try:
            tr.check(name, A)
        except ValueError:
            with pytest.raises(ValueError):
                tr.from_group(name, A)
            continue
        ops = tr.from_group(name, A)
        assert ops.T == tr.size(name) == tr.size(ops) and np.all(ops.entries[3] == 1.)
        W = rng.random((2, 3) + A)
        X = rng.random((2 * ops.T, 3) + A)
        assert np.array_equal(tr.expand(W, ops), tr.expand(W, name))
        assert np.array_equal(tr.fold(X, ops), tr.fold(X, name))
        assert np.array_equal(tr.expand(W.astype(np.float32), ops), tr.expand(W.astype(np.float32), name))


def random_ops(A, T, density, seed):
    rng = np.random.default_rng(seed)
    L = rng.random((T,) + tuple(A) * 2) * (rng.random((T,) + tuple(A) * 2) < density)
    return tr.AtomOperators.from_dense(L)


ADJOINT = {
    'compose': BUILTINS['compose'],
    'scales_1d': BUILTINS['scales_1d'],
    'rot12_4x7': BUILTINS['rot12_4x7'],
    'dense_random': lambda: random_ops((4, 5), 3, 0.2, 3),
    'dense_random_1d': lambda: random_ops((11,), 2, 0.3, 4),
}


@pytest.mark.parametrize('name', list(ADJOINT))
def test_fold_is_the_adjoint_of_the_expansion(name):
    ops = ADJOINT[name]()
    rng = np.random.default_rng(5)
    W = rng.random((3, 2) + ops.atom_shape)
    X = rng.random((3 * ops.T, 2) + ops.atom_shape)
    lhs = float(np.sum(tr.expand(W, ops) * X))
    rhs = float(np.sum(W * tr.fold(X, ops)))
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    L = dense(ops)
    assert np.abs(tr.expand(W, ops) - oref.expand(W, L)).max() <= 1e-14
    assert np.abs(tr.fold(X, ops) - oref.fold(X, L)).max() <= 1e-13 * np.abs(oref.fold(X, L)).max()
    assert tr.expand(W.astype(np.float32), ops).dtype == np.float32


def test_operators_are_immutable_values():
    ops = tr.rotations((5, 5), 8)
    with pytest.raises(AttributeError):
        ops._T = 3
    for a in ops.entries:
        assert not a.flags.writeable
        with pytest.raises(ValueError):
            a[0] = 0
    assert ops == tr.rotations((5, 5), 8) and hash(ops) == hash(tr.rotations((5, 5), 8))
    assert ops != tr.rotations((5, 5), 7) and ops != 'rot90'
    t, o, i, w = ops.entries
    perm = np.random.default_rng(0).permutation(len(w))
    assert tr.AtomOperators((5, 5), 8, t[perm], o[perm], i[perm], w[perm]) == ops   # (kept in canonical order)


# -- refusals -----------------------------------------------------------------------------------------------------------
BAD_DENSE = {
    'negative': -np.ones((1, 2, 2, 2, 2)),
    'nan': np.full((1, 2, 2, 2, 2), np.nan),
    'inf': np.full((1, 2, 2, 2, 2), np.inf),
    'shape': np.ones((1, 2, 3, 3, 2)),
    'odd_axes': np.ones((1, 2, 2, 2)),
    'no_T': np.ones((0, 2, 2, 2, 2)),
    'complex': np.ones((1, 2, 2, 2, 2), dtype=complex),
    'strings': np.array([['a']]),
}


@pytest.mark.parametrize('name', list(BAD_DENSE))
def test_from_dense_refuses(name):
    with pytest.raises(ValueError):
        tr.AtomOperators.from_dense(BAD_DENSE[name])


def test_constructors_refuse():
    bad = [lambda: tr.rotations((5,), 4), lambda: tr.rotations((3, 3, 3), 4), lambda: tr.rotations((5, 5), 0),
           lambda: tr.rotations((5, 5), 1.5), lambda: tr.scales((5, 5), []), lambda: tr.scales((5, 5), [0.]),
           lambda: tr.scales((5, 5), [-1.]), lambda: tr.scales((5, 5), [np.nan]), lambda: tr.scales((5, 5), [np.inf]),
           lambda: tr.scales((3, 3, 3), [1.]), lambda: tr.compose(tr.rotations((5, 5), 2), tr.rotations((4, 4), 2)),
           lambda: tr.compose(tr.rotations((5, 5), 2), 'rot90'), lambda: tr.from_group('rotate', (5, 5)),
           lambda: tr.from_group('rot90', (3, 4)), lambda: tr.from_group('mirrors', (5,)),
           lambda: tr.AtomOperators((2, 2), 1, [0, 0], [0, 0], [1, 1], [1., 2.]),      # a duplicate entry
           lambda: tr.AtomOperators((2, 2), 1, [1], [0], [0], [1.]),                   # t out of range
           lambda: tr.AtomOperators((2, 2), 1, [0], [4], [0], [1.]),                   # pixel out of range
           lambda: tr.AtomOperators((2, 2), 1, [0], [0], [-1], [1.]),
           lambda: tr.AtomOperators((2, 2), 1, [0], [0], [0], [-1.]),
           lambda: tr.AtomOperators((2, 2), 0, [], [], [], [])]
    for make in bad:
        with pytest.raises(ValueError):
            make()


class _Initialised(Exception):
    pass


class _OperatorStub(OracleBackend):
    """A float64 backend on the oracle's pieces with every hook a fit with atom operators uses (beta, weights, transforms
    and operators included) -- enough to drive the front end's schedules on CPU."""

    supports_beta_loss = True
    supports_weights = True
    supports_transforms = True
    supports_atom_operators = True

    def __init__(self, stop_at_init=False):
        super().__init__(impl='contract')
        self.stop_at_init = stop_at_init
        self.inits = []

    def _initialize_matrices(self, V, atom_shape, n_atoms, W=None, axes_W_normalization=None, weights=None,
                             transforms=None):
        self.inits.append(transforms)
        if self.stop_at_init:
            raise _Initialised
        self._V_local = V
        self._G = np.broadcast_to(np.asarray(1. if weights is None else weights, dtype=np.float64), V.shape)
        T = 1 if transforms is None else tr.size(transforms)
        H = np.empty((V.shape[0], n_atoms * T) + self._transform_shape, dtype=V.dtype)
        for i, h in sharding.reference_init_stream(V.shape[0], H.shape[1:], (0, V.shape[0]), V.dtype):
            H[i] = h
        if W is None:
            W = sharding.reference_init_W(n_atoms, self.n_channels, self.atom_shape, V.dtype)
        return W, H

    def reconstruction_energy(self, V, W, H, beta=2., eps=1e-9):
        return wref.energy(self._V_local, self._G, W, H, beta, eps)

    def fused_update_H(self, V, W, H, s=sliceNone, sparsity=0., eps=1e-9, inhibition=0., cross_inhibition=0.,
                       inhibition_kernels=None, beta=2.):
        wref.update_H(self._V_local, self._G, W, H, s, beta, eps, sparsity, inhibition, cross_inhibition,
                      inhibition_kernels)

    def local_gradient_W(self, V, W, H, s=sliceNone, beta=2., eps=1e-9):
        return np.stack(wref.gradient_W(self._V_local, self._G, W, H, s, beta, eps))

    def all_reduce_gradient_W(self, negpos):
        return negpos

    def apply_W(self, W, negpos, eps=1e-9):
        orc.multiplicative_update(W, negpos[0], negpos[1], eps, normalization_axes=tuple(range(-len(self.atom_shape), 0)))

    def expand_W(self, W, transforms, W_eff=None):
        e = tr.expand(W, transforms)
        if W_eff is None:
            return e
        W_eff[...] = e
        return W_eff

    def fold_gradient_W(self, negpos_eff, transforms):
        return np.stack([tr.fold(negpos_eff[0], transforms), tr.fold(negpos_eff[1], transforms)])

    def fused_update_W_transformed(self, V, W, W_eff, H, s=sliceNone, transforms=None, eps=1e-9, beta=2.):
        negpos = self.fold_gradient_W(self.local_gradient_W(V, W_eff, H, s, beta, eps), transforms)
        self.apply_W(W, negpos, eps)
        self.expand_W(W, transforms, W_eff)


class _GroupsOnly(_OperatorStub):
    supports_atom_operators = False


@pytest.mark.parametrize('bad', [np.ones((1, 3, 3, 3, 3)), [np.eye(9)], (np.eye(9),), 'rotations', 8], ids=str)
def test_raw_arrays_and_unknown_values_are_refused(bad):
    with pytest.raises(ValueError):
        TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=_OperatorStub(), transforms=bad)


def test_operators_of_another_atom_shape_are_refused():
    for A, ops in [((3, 3), tr.rotations((4, 4), 8)), ((4, 5), tr.rotations((5, 4), 8)), ((9,), tr.scales((8,), [1.])),
                   ((3, 3), tr.scales((9,), [1.]))]:
        be = _OperatorStub(stop_at_init=True)
        with pytest.raises(ValueError):
            TransformInvariantNMF(n_atoms=2, atom_shape=A, backend=be, transforms=ops)
        assert be.inits == []


def test_volumes_are_refused_before_initialising():
    ops = tr.AtomOperators.from_dense(np.ones((2,) + (2, 2, 2) * 2))
    be = _OperatorStub(stop_at_init=True)
    with pytest.raises(NotImplementedError):
        nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(2, 2, 2), backend=be, transforms=ops)
        nmf.fit_batch(np.ones((2, 1, 4, 4, 4)), n_iterations=1)
    assert be.inits == []


def test_a_backend_without_atom_operators_is_refused():
    assert Backend.supports_atom_operators is False and OracleBackend.supports_atom_operators is False
    ops = tr.rotations((3, 3), 8)
    for be in (_GroupsOnly(stop_at_init=True), OracleBackend(hooks=True)):
        with pytest.raises(NotImplementedError):
            TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=be, transforms=ops)
        with pytest.raises(NotImplementedError):
            be.initialize(np.ones((2, 1, 6, 6)), (3, 3), 2, None, (-2, -1), transforms=ops)
    TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=_GroupsOnly(), transforms='rot90')   # (groups: as before)


def test_an_operator_model_reads_out_like_a_transformed_one():
    be = _OperatorStub()
    ops = tr.compose(tr.rotations((3, 3), 4), tr.scales((3, 3), [1., .5]))
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=be, transforms=ops)
    nmf._initialize_matrices(np.random.default_rng(0).random((2, 1, 8, 8)), False)
    assert be.inits == [ops] and nmf.n_transforms == 8 and nmf.transforms is ops
    assert not nmf._plain_frobenius and nmf._scheduler(dict(sparsity=0., inhibition=0., cross_inhibition=0.)) is None
    assert nmf.W.shape == (2, 1, 3, 3) and nmf.H.shape == (2, 2, 8, 10, 10)
    assert nmf.transformed_atoms.shape == (2, 8, 1, 3, 3)
    assert np.array_equal(nmf.transformed_atoms.reshape(16, 1, 3, 3), tr.expand(nmf.W, ops))


# -- the front end on the stub against the dense reference ------------------------------------------------------------------
def positive_V(shape, seed):
    return np.random.default_rng(seed).random(shape) + 0.05


OPS = {
    'rot8_2d': ((4, 4), lambda: tr.rotations((4, 4), 8)),
    'scales_1d': ((5,), lambda: tr.scales((5,), [1., .7, 1.5])),
    'compose_2d': ((3, 4), lambda: tr.compose(tr.rotations((3, 4), 3), tr.scales((3, 4), [1., .6]))),
    'dense_2d': ((3, 3), lambda: random_ops((3, 3), 3, 0.3, 6)),
}


def close(got, want, tol=1e-12):
    return np.abs(np.asarray(got) - want).max() <= tol * np.abs(want).max()


@pytest.mark.parametrize('beta', [2., 1., 0.])
@pytest.mark.parametrize('name', list(OPS))
def test_front_end_batch_fit_equals_the_reference(name, beta):
    A, make = OPS[name]
    ops = make()
    shape = (3, 2, 17) if len(A) == 1 else (3, 2, 11, 12)
    V = positive_V(shape, 1)
    kw = dict(n_iterations=3, sparsity_H=0.05, inhibition_strength=0.1, cross_atom_inhibition_strength=0.05)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=A, backend=_OperatorStub(), transforms=ops, beta_loss=beta)
    nmf.fit(V, progress_callback=lambda *_: True, **kw)
    np.random.seed(42)
    ref = oref.OperatorOracleNMF(n_atoms=2, atom_shape=A, ops=ops, beta=beta).fit(V, **kw)
    assert close(nmf.W, ref.W) and close(nmf.H, ref.H4)
    assert close(nmf.transformed_atoms.reshape(ref.W_eff.shape), ref.W_eff)
    assert abs(nmf._energy_function() - ref.energy()) <= 1e-12 * ref.energy()
    assert close(nmf.R, ref.R) and close(nmf.R_partial(1), ref.R_partial(1))


@pytest.mark.parametrize('beta', [2., 1.])
def test_front_end_weighted_fit_equals_the_reference(beta):
    V = positive_V((4, 1, 12, 12), 2)
    rng = np.random.default_rng(2)
    G = rng.random(V.shape) + 0.5
    G[rng.random(G.shape) < 0.2] = 0.
    V = np.where(G == 0, 0., V)
    ops = tr.rotations((4, 4), 6)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(4, 4), backend=_OperatorStub(), transforms=ops, beta_loss=beta)
    nmf.fit_batch(V, n_iterations=3, progress_callback=lambda *_: True, weights=G)
    np.random.seed(42)
    ref = oref.OperatorOracleNMF(n_atoms=2, atom_shape=(4, 4), ops=ops, beta=beta, weights=G).fit(V, n_iterations=3)
    assert close(nmf.W, ref.W) and close(nmf.H, ref.H4)
    assert abs(nmf._energy_function() - ref.energy()) <= 1e-12 * ref.energy()


@pytest.mark.parametrize('lateral', [False, True], ids=['plain', 'inhibition'])
@pytest.mark.parametrize('algorithm', list(MiniBatchAlgorithm), ids=[a.name for a in MiniBatchAlgorithm])
def test_front_end_epochs_equal_the_reference(algorithm, lateral):
    V = positive_V((5, 1, 10, 10), 3)
    ops = tr.compose(tr.rotations((3, 3), 4), tr.scales((3, 3), [1., .5]))
    kw = dict(algorithm=algorithm, batch_size=2, n_epochs=2, sparsity_H=0.05)
    if lateral:
        kw.update(inhibition_strength=0.1, cross_atom_inhibition_strength=0.05)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=_OperatorStub(), transforms=ops)
    nmf.fit(V, progress_callback=lambda *_: True, **kw)
    np.random.seed(42)
    kw['algorithm'] = orc.MiniBatchAlgorithm(algorithm.value)
    ref = oref.OperatorOracleNMF(n_atoms=2, atom_shape=(3, 3), ops=ops).fit(V, **kw)
    assert close(nmf.W, ref.W) and close(nmf.H, ref.H4)


def test_front_end_stream_keeps_W():
    V = positive_V((6, 1, 9, 9), 4)
    ops = tr.rotations((3, 3), 8)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=_OperatorStub(), transforms=ops)
    nmf.fit(iter(V), subsample_size=3, n_iterations=2, progress_callback=lambda *_: True)
    np.random.seed(42)
    ref = oref.OperatorOracleNMF(n_atoms=2, atom_shape=(3, 3), ops=ops).fit(iter(V), subsample_size=3, n_iterations=2)
    assert close(nmf.W, ref.W) and close(nmf.H, ref.H4)


def test_group_operators_fit_like_the_group():
    """from_group('dihedral') through the operator reference = 'dihedral' through the group reference."""
    V = positive_V((3, 1, 10, 10), 5)
    np.random.seed(42)
    a = oref.OperatorOracleNMF(n_atoms=2, atom_shape=(3, 3), ops=tr.from_group('dihedral', (3, 3))).fit(V, n_iterations=3)
    np.random.seed(42)
    b = tref.TransformOracleNMF(n_atoms=2, atom_shape=(3, 3), transforms='dihedral').fit(V, n_iterations=3)
    assert close(a.W, b.W, 1e-14) and close(a.H, b.H, 1e-14)


# -- the planted motifs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1])
def test_planted_motif_at_eight_angles_on_the_reference(seed):
    """One motif at 8 angles 45 degrees apart: a 1-atom rotations(A, 8) fit ends PLANTED_ANGLES_MARGIN times lower in
    energy than a 1-atom 'rot90' fit (which can only follow every second angle)."""
    P = oref.PLANTED_ANGLES
    V = oref.planted_angles(seed)
    np.random.seed(42)
    rot = oref.OperatorOracleNMF(n_atoms=1, atom_shape=P['atom_shape'],
                                 ops=tr.rotations(P['atom_shape'], P['n_angles'])).fit(V, n_iterations=P['iterations'])
    np.random.seed(42)
    quarter = tref.TransformOracleNMF(n_atoms=1, atom_shape=P['atom_shape'], transforms='rot90').fit(
        V, n_iterations=P['iterations'])
    assert quarter.energy() >= oref.PLANTED_ANGLES_MARGIN * rot.energy(), (rot.energy(), quarter.energy())


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_planted_motif_at_three_stretches_on_the_reference(seed):
    """One 1-D motif at 3 stretches: a 1-atom scales fit ends PLANTED_STRETCH_MARGIN times lower in energy than a 1-atom
    plain fit."""
    P = oref.PLANTED_STRETCH
    V = oref.planted_stretch(seed)
    np.random.seed(42)
    st = oref.OperatorOracleNMF(n_atoms=1, atom_shape=P['atom_shape'],
                                ops=tr.scales(P['atom_shape'], P['factors'])).fit(V, n_iterations=P['iterations'])
    np.random.seed(42)
    plain = orc.OracleNMF(n_atoms=1, atom_shape=P['atom_shape']).fit(V, n_iterations=P['iterations'])
    assert plain.energy() >= oref.PLANTED_STRETCH_MARGIN * st.energy(), (st.energy(), plain.energy())


# -- the ABI --------------------------------------------------------------------------------------------------------------
NAMES = ('tnmf_hip_atom_ops_create', 'tnmf_hip_atom_ops_destroy', 'tnmf_hip_ops_expand_W', 'tnmf_hip_ops_fold_grad_W',
         'tnmf_hip_ops_apply_W')


def test_abi_8_exports_the_operator_entry_points():
    assert _lib.ABI_VERSION == 8
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                               'tnmf_hip.h')).read()
    assert 'typedef struct tnmf_hip_atom_ops tnmf_hip_atom_ops;' in header
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert f'int {name}(' in header
    lib = _lib.load()
    assert lib.tnmf_hip_abi_version() == 8
    for name in NAMES:
        assert hasattr(lib, name)
