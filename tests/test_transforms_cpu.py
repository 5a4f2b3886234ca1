"""Rotation and mirror invariance (TransformInvariantNMF(..., transforms=...)) without a GPU: the group tables against
their numpy definitions, the fold as the adjoint of the expansion, the checks and refusals of the constructor, the front
end's transformed schedules on a float64 stub backend against the reference of tests/transform_reference.py, the planted
rotated motif whose margin tests/test_hip_transforms.py asserts on the GPU, and the ABI of the group entry points."""
import itertools
import os

import numpy as np
import pytest

import beta_reference as bref
import transform_reference as tref
from oracle import tnmf_oracle as orc
from oracle_backend import OracleBackend
from tnmf_amd import _lib, sharding, transforms as tr
from tnmf_amd.backends._Backend import sliceNone
from tnmf_amd.TransformInvariantNMF import MiniBatchAlgorithm, TransformInvariantNMF

GROUPS = ['flip', 'mirrors', 'rot90', 'dihedral']


# -- the group tables ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', GROUPS)
def test_group_table_matches_the_numpy_definitions(name):
    a = np.random.default_rng(0).random((5, 5))
    fwd, inv = tref.ops(name, 2)
    assert len(tr.GROUPS[name]) == len(fwd) == tr.size(name)
    for code, f, g in zip(tr.GROUPS[name], fwd, inv):
        assert np.array_equal(tr.apply(code, a), f(a))
        assert np.array_equal(tr.apply_inverse(code, a), g(a))
        assert np.array_equal(g(f(a)), a)
    if name == 'flip':
        b = np.random.default_rng(1).random(7)
        assert [tr.apply(c, b).tolist() for c in tr.GROUPS[name]] == [f(b).tolist() for f in tref.ops(name, 1)[0]]
    # non-square atoms: the groups without a transpose
    if name in ('flip', 'mirrors'):
        r = np.random.default_rng(2).random((3, 6))
        for code, f in zip(tr.GROUPS[name], fwd):
            assert np.array_equal(tr.apply(code, r), f(r))
    assert _lib.GROUPS[name] == GROUPS.index(name)


@pytest.mark.parametrize('name', GROUPS)
def test_groups_are_closed_under_composition_and_inverse(name):
    a = np.arange(36.).reshape(6, 6)          # distinct pixels: an image of a transform identifies it
    images = [tr.apply(c, a).tobytes() for c in tr.GROUPS[name]]
    assert len(set(images)) == len(images)    # T distinct permutations
    assert images[0] == a.tobytes()           # the identity first
    for c1, c2 in itertools.product(tr.GROUPS[name], repeat=2):
        assert tr.apply(c1, tr.apply(c2, a)).tobytes() in images
    for c in tr.GROUPS[name]:
        assert tr.apply_inverse(c, a).tobytes() in images


@pytest.mark.parametrize('name', GROUPS)
def test_permutations_preserve_the_normalisation_sums(name):
    W = np.random.default_rng(3).random((3, 2, 5, 5))
    W_eff = tr.expand(W, name)
    T = tr.size(name)
    assert W_eff.shape == (3 * T, 2, 5, 5)
    assert np.array_equal(W_eff.reshape(3, T, 2, 5, 5)[:, 0], W)
    sums = W_eff.sum(axis=(-2, -1)).reshape(3, T, 2)
    assert np.allclose(sums, W.sum(axis=(-2, -1))[:, None, :], rtol=1e-15, atol=0)
    assert np.array_equal(W_eff, tref.expand(W, name))


ADJOINT = [(n, s) for n in GROUPS for s in ((2, 3, 5, 5), (2, 1, 4, 4))] + [('flip', (3, 2, 9))]


@pytest.mark.parametrize('name,shape', ADJOINT, ids=[f'{n}_{"x".join(map(str, s[2:]))}' for n, s in ADJOINT])
def test_fold_is_the_adjoint_of_the_expansion(name, shape):
    rng = np.random.default_rng(4)
    W = rng.random(shape)
    T = tr.size(name)
    X = rng.random((shape[0] * T,) + shape[1:])
    lhs = float(np.sum(tref.expand(W, name) * X))
    rhs = float(np.sum(W * tref.fold(X, name)))
    assert abs(lhs - rhs) <= 1e-13 * abs(lhs)
    assert np.array_equal(tr.fold(X, name), tref.fold(X, name))
    assert np.array_equal(tr.expand(W, name), tref.expand(W, name))


# -- the constructor: checks and refusals ---------------------------------------------------------------------------------
class _Initialised(Exception):
    pass


class _TransformStub(OracleBackend):
    """A float64 backend on the oracle's pieces that offers every hook a transformed fit uses (beta and the transform
    group included) -- enough to drive the front end's schedules on CPU."""

    supports_beta_loss = True
    supports_transforms = True

    def __init__(self, stop_at_init=False):
        super().__init__(impl='contract')
        self.stop_at_init = stop_at_init
        self.inits = []

    def _initialize_matrices(self, V, atom_shape, n_atoms, W=None, axes_W_normalization=None, transforms=None):
        self.inits.append(transforms)
        if self.stop_at_init:
            raise _Initialised
        self._V_local = V
        T = 1 if transforms is None else tr.size(transforms)
        H = np.empty((V.shape[0], n_atoms * T) + self._transform_shape, dtype=V.dtype)
        for i, h in sharding.reference_init_stream(V.shape[0], H.shape[1:], (0, V.shape[0]), V.dtype):
            H[i] = h
        if W is None:
            W = sharding.reference_init_W(n_atoms, self.n_channels, self.atom_shape, V.dtype)
        return W, H

    def reconstruction_energy(self, V, W, H, beta=2., eps=1e-9):
        return bref.energy(self._V_local, W, H, beta, eps)

    def fused_update_H(self, V, W, H, s=sliceNone, sparsity=0., eps=1e-9, inhibition=0., cross_inhibition=0.,
                       inhibition_kernels=None, beta=2.):
        bref.update_H(self._V_local, W, H, s, beta, eps, sparsity, inhibition, cross_inhibition, inhibition_kernels)

    def local_gradient_W(self, V, W, H, s=sliceNone, beta=2., eps=1e-9):
        return np.stack(bref.gradient_W(self._V_local, W, H, s, beta, eps))

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


@pytest.mark.parametrize('bad', ['rotate', 'Flip', 3, ('flip',), ['rot90'], True], ids=str)
def test_unknown_transforms_are_refused(bad):
    with pytest.raises(ValueError):
        TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=_TransformStub(), transforms=bad)


@pytest.mark.parametrize('name', ['rot90', 'dihedral'])
def test_rotations_of_non_square_atoms_are_refused(name):
    with pytest.raises(ValueError):
        TransformInvariantNMF(n_atoms=2, atom_shape=(3, 4), backend=_TransformStub(), transforms=name)
    for ok in ('flip', 'mirrors'):
        TransformInvariantNMF(n_atoms=2, atom_shape=(3, 4), backend=_TransformStub(), transforms=ok)


@pytest.mark.parametrize('name', ['mirrors', 'rot90', 'dihedral'])
def test_two_axis_groups_on_one_shift_axis_are_refused(name):
    with pytest.raises(ValueError):
        TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend=_TransformStub(), transforms=name)
    TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend=_TransformStub(), transforms='flip')


@pytest.mark.parametrize('name', GROUPS)
def test_volumes_are_refused_before_initialising(name):
    be = _TransformStub(stop_at_init=True)
    with pytest.raises(NotImplementedError):
        nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(2, 2, 2), backend=be, transforms=name)
        nmf.fit_batch(np.ones((2, 1, 4, 4, 4)), n_iterations=1)
    assert be.inits == []


def test_a_backend_without_transforms_is_refused():
    be = OracleBackend(hooks=True)
    be._initialize_matrices = lambda *a, **k: (_ for _ in ()).throw(_Initialised())
    with pytest.raises(NotImplementedError):
        TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=be, transforms='flip')
    with pytest.raises(NotImplementedError):
        be.initialize(np.ones((2, 1, 6, 6)), (3, 3), 2, None, (-2, -1), transforms='flip')
    TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=be)   # (no transforms: accepted as before)


def test_a_transformed_fit_is_not_the_plain_frobenius_objective():
    be = _TransformStub()
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=be, transforms='rot90')
    nmf._initialize_matrices(np.random.default_rng(0).random((2, 1, 8, 8)), False)
    assert be.inits == ['rot90'] and nmf.n_transforms == 4
    assert not nmf._plain_frobenius and nmf._objective() == dict(beta=2., eps=nmf.eps)
    assert nmf._scheduler(dict(sparsity=0., inhibition=0., cross_inhibition=0.)) is None
    assert nmf.W.shape == (2, 1, 3, 3) and nmf.H.shape == (2, 2, 4, 10, 10)
    assert nmf.transformed_atoms.shape == (2, 4, 1, 3, 3)
    assert np.array_equal(nmf.transformed_atoms[:, 1, 0], np.rot90(nmf.W[:, 0], 1, axes=(-2, -1)))
    plain = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=_TransformStub())
    assert plain.transforms is None and plain.n_transforms == 1 and plain._plain_frobenius


# -- the front end on the stub against the reference ---------------------------------------------------------------------
def positive_V(shape, seed):
    return np.random.default_rng(seed).random(shape) + 0.05


CASES = [('flip', (4,)), ('flip', (3, 4)), ('mirrors', (3, 4)), ('rot90', (4, 4)), ('dihedral', (3, 3))]


@pytest.mark.parametrize('beta', [2., 1.])
@pytest.mark.parametrize('name,A', CASES, ids=[f'{n}_{len(a)}d' for n, a in CASES])
def test_front_end_batch_fit_equals_the_reference(name, A, beta):
    shape = (3, 2, 17) if len(A) == 1 else (3, 2, 11, 12)
    V = positive_V(shape, 1)
    kw = dict(n_iterations=3, sparsity_H=0.05, inhibition_strength=0.1, cross_atom_inhibition_strength=0.05)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=A, backend=_TransformStub(), transforms=name, beta_loss=beta)
    nmf.fit(V, progress_callback=lambda *_: True, **kw)
    np.random.seed(42)
    ref = tref.TransformOracleNMF(n_atoms=2, atom_shape=A, transforms=name, beta=beta).fit(V, **kw)
    assert np.abs(nmf.W - ref.W).max() <= 1e-12 * np.abs(ref.W).max()
    assert np.abs(nmf.H - ref.H4).max() <= 1e-12 * np.abs(ref.H).max()
    assert np.array_equal(nmf.transformed_atoms.reshape(ref.W_eff.shape), ref.W_eff)
    assert abs(nmf._energy_function() - ref.energy()) <= 1e-12 * ref.energy()
    assert np.abs(nmf.R - ref.R).max() <= 1e-12 * np.abs(ref.R).max()
    assert np.abs(nmf.R_partial(1) - ref.R_partial(1)).max() <= 1e-12 * np.abs(ref.R_partial(1)).max()


@pytest.mark.parametrize('lateral', [False, True], ids=['plain', 'inhibition'])
@pytest.mark.parametrize('algorithm', list(MiniBatchAlgorithm), ids=[a.name for a in MiniBatchAlgorithm])
def test_front_end_epochs_equal_the_reference(algorithm, lateral):
    V = positive_V((5, 1, 10, 10), 2)
    kw = dict(algorithm=algorithm, batch_size=2, n_epochs=2, sparsity_H=0.05)
    if lateral:
        kw.update(inhibition_strength=0.1, cross_atom_inhibition_strength=0.05)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=_TransformStub(), transforms='rot90')
    nmf.fit(V, progress_callback=lambda *_: True, **kw)
    np.random.seed(42)
    kw['algorithm'] = orc.MiniBatchAlgorithm(algorithm.value)
    ref = tref.TransformOracleNMF(n_atoms=2, atom_shape=(3, 3), transforms='rot90').fit(V, **kw)
    assert np.abs(nmf.W - ref.W).max() <= 1e-12 * np.abs(ref.W).max()
    assert np.abs(nmf.H - ref.H4).max() <= 1e-12 * np.abs(ref.H).max()


def test_front_end_stream_keeps_W():
    V = positive_V((6, 1, 9, 9), 3)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend=_TransformStub(), transforms='mirrors')
    nmf.fit(iter(V), subsample_size=3, n_iterations=2, progress_callback=lambda *_: True)
    np.random.seed(42)
    ref = tref.TransformOracleNMF(n_atoms=2, atom_shape=(3, 3), transforms='mirrors').fit(
        iter(V), subsample_size=3, n_iterations=2)
    assert np.abs(nmf.W - ref.W).max() <= 1e-12 * np.abs(ref.W).max()
    assert np.abs(nmf.H - ref.H4).max() <= 1e-12 * np.abs(ref.H).max()


# -- the planted rotated motif -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1])
def test_planted_rotated_motif_on_the_reference(seed):
    """Data made of one motif in its four rotations: a 'rot90' fit with ONE atom ends PLANTED_MARGIN times lower in
    energy than a plain fit with one atom (measured 4.5x and 3.9x for these seeds)."""
    P = tref.PLANTED
    V = tref.planted(seed)
    np.random.seed(42)
    rot = tref.TransformOracleNMF(n_atoms=1, atom_shape=P['atom_shape'], transforms='rot90').fit(
        V, n_iterations=P['iterations'])
    np.random.seed(42)
    plain = orc.OracleNMF(n_atoms=1, atom_shape=P['atom_shape']).fit(V, n_iterations=P['iterations'])
    assert plain.energy() >= tref.PLANTED_MARGIN * rot.energy(), (rot.energy(), plain.energy())


# -- the ABI --------------------------------------------------------------------------------------------------------------
def test_abi_8_exports_the_group_entry_points():
    assert _lib.ABI_VERSION == 8
    names = ('tnmf_hip_group_expand_W', 'tnmf_hip_group_fold_grad_W', 'tnmf_hip_group_apply_W')
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                               'tnmf_hip.h')).read()
    for name in names:
        assert name in _lib.EXPORTS
        assert f'int {name}(' in header
    for group, i in _lib.GROUPS.items():
        assert f'TNMF_GROUP_{group.upper()} = {i}' in header
    lib = _lib.load()
    assert lib.tnmf_hip_abi_version() == 8
    for name in names:
        assert hasattr(lib, name)
