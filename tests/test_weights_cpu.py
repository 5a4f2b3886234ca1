"""Elementwise weights (missing-data masks) of TransformInvariantNMF without a GPU: the float64 reference of the weighted
steps (tests/weighted_reference.py), the checks and refusals of fit, the ABI of the weighted entry points, and the planted
inpainting property whose margin tests/test_hip_weights.py asserts on the GPU."""
import numpy as np
import pytest

import beta_reference as bref
import weighted_reference as wref
from oracle import tnmf_oracle as orc
from oracle_backend import OracleBackend
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import MiniBatchAlgorithm, TransformInvariantNMF


def problem(seed=5, shape=(4, 2, 12, 13), A=(3, 4), M=3):
    rng = np.random.default_rng(seed)
    V = rng.random(shape) + 0.05
    np.random.seed(1)
    W, H = orc.init_matrices(V, A, M)
    return V, W, H


# -- the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [2., 1., 0.])
def test_unit_weights_are_the_beta_reference(beta):
    V, W, H = problem()
    G = np.ones_like(V)
    H1, H2, W1, W2 = H.copy(), H.copy(), W.copy(), W.copy()
    bref.update_H(V, W1, H1, beta=beta, sparsity=0.1)
    wref.update_H(V, G, W2, H2, beta=beta, sparsity=0.1)
    assert np.abs(H2 - H1).max() <= 1e-12 * np.abs(H1).max()
    for a, b in zip(bref.gradient_W(V, W1, H1, beta=beta), wref.gradient_W(V, G, W2, H2, beta=beta)):
        assert np.abs(b - a).max() <= 1e-12 * np.abs(a).max()
    e1, e2 = bref.energy(V, W1, H1, beta), wref.energy(V, G, W2, H2, beta)
    assert abs(e2 - e1) <= 1e-12 * abs(e1)


@pytest.mark.parametrize('beta', [2., 1., 0.])
def test_constant_weight_leaves_the_H_step_unchanged(beta):
    """G = c scales both correlations by c: the step changes only through the eps in its denominator."""
    V, W, H = problem()
    H1, H2 = H.copy(), H.copy()
    wref.update_H(V, np.ones_like(V), W, H1, beta=beta)
    wref.update_H(V, np.full_like(V, 3.7), W, H2, beta=beta)
    assert np.abs(H2 - H1).max() <= 1e-8 * np.abs(H1).max()


@pytest.mark.parametrize('beta', [2., 1.])
def test_zero_weight_on_whole_samples_drops_them_from_the_W_gradient(beta):
    V, W, H = problem()
    G = np.ones_like(V)
    G[[1, 3]] = 0.
    V_nan = V.copy()
    V_nan[[1, 3]] = np.nan          # (never read)
    got = wref.gradient_W(V_nan, G, W, H, beta=beta)
    keep = [0, 2]
    want = bref.gradient_W(V[keep], W, H[keep], beta=beta)
    for a, b in zip(want, got):
        assert np.abs(b - a).max() <= 1e-12 * np.abs(a).max()


@pytest.mark.parametrize('beta', [2., 1.5, 1., 0.])
def test_binary_weights_restrict_the_energy(beta):
    V, W, H = problem()
    G = (np.random.default_rng(9).random(V.shape) < 0.7).astype(np.float64)
    R = orc.reconstruct(W, H)
    keep = G == 1
    want = bref.divergence(V[keep], R[keep], beta)
    V_inf = np.where(keep, V, np.inf)
    assert abs(wref.divergence(V_inf, G, R, beta) - want) <= 1e-12 * abs(want)


def test_zero_weight_fields_are_exactly_zero():
    V = np.array([np.nan, np.inf, 1., 0., 2.])
    R = np.array([1., 1., -1., 0., 3.])
    G = np.array([0., 0., 0., 0., 2.])
    for beta in (2., 1., 0., -3.):
        Q, P = wref.fields(V, G, R, beta, dtype=np.float32)
        assert np.all(Q[:4] == 0) and np.all(P[:4] == 0) and np.all(np.isfinite(Q)) and np.all(np.isfinite(P))


# -- the front end: checks and refusals -----------------------------------------------------------------------------------
class _WeightedStub(OracleBackend):
    """An oracle backend that claims weighted objectives and records what initialize() was given."""

    supports_weights = True
    supports_beta_loss = True

    def _initialize_matrices(self, V, atom_shape, n_atoms, W=None, axes_W_normalization=None, weights=None):
        self.got_weights = weights
        return super()._initialize_matrices(V, atom_shape, n_atoms, W, axes_W_normalization)


class _Initialised(Exception):
    pass


class _StopAtInit(_WeightedStub):
    def _initialize_matrices(self, V, atom_shape, n_atoms, W=None, axes_W_normalization=None, weights=None):
        self.got_weights = weights
        raise _Initialised


FITS = [('fit_batch', dict(n_iterations=1)), ('fit_minibatches', dict(n_epochs=1))]


def V3(seed=0, shape=(3, 2, 8)):
    return np.random.default_rng(seed).random(shape) + 0.1


@pytest.mark.parametrize('how,kw', FITS, ids=[f[0] for f in FITS])
@pytest.mark.parametrize('weights', [np.ones((3, 2, 7)), np.ones((2, 2, 8)), np.ones((4,))],
                         ids=['bad_last', 'bad_samples', 'bad_1d'])
def test_weights_that_do_not_broadcast_are_refused(how, kw, weights):
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend=_StopAtInit())
    with pytest.raises(ValueError):
        getattr(nmf, how)(V3(), weights=weights, **kw)


@pytest.mark.parametrize('how,kw', FITS, ids=[f[0] for f in FITS])
@pytest.mark.parametrize('bad', [-1., np.nan, np.inf, 1e300], ids=['negative', 'nan', 'inf', 'inf_in_f32'])
def test_negative_or_non_finite_weights_are_refused(how, kw, bad):
    V = V3().astype(np.float32)
    G = np.ones(V.shape)
    G[1, 0, 3] = bad
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend=_StopAtInit())
    with pytest.raises(ValueError):
        getattr(nmf, how)(V, weights=G, **kw)


def test_fit_stream_refuses_weights():
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend=_StopAtInit())
    with pytest.raises(ValueError):
        nmf.fit(iter(V3(shape=(6, 2, 8))), subsample_size=3, weights=np.ones((3, 2, 8)), n_iterations=1)
    with pytest.raises(ValueError):
        nmf.fit_stream(iter(V3(shape=(6, 2, 8))), weights=1.)


@pytest.mark.parametrize('how,kw', FITS, ids=[f[0] for f in FITS])
def test_backend_without_weights_is_refused_before_initialising(how, kw):
    be = OracleBackend(hooks=True)
    be._initialize_matrices = lambda *a, **k: (_ for _ in ()).throw(_Initialised())
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend=be)
    with pytest.raises(NotImplementedError):
        getattr(nmf, how)(V3(), weights=np.ones((3, 1, 8)), **kw)
    with pytest.raises(NotImplementedError):
        be.initialize(V3(), (3,), 2, None, (-1,), weights=np.ones((3, 2, 8)))


@pytest.mark.parametrize('how,kw', FITS, ids=[f[0] for f in FITS])
def test_volumes_are_refused_before_initialising(how, kw):
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(2, 2, 2), backend=_StopAtInit())
    with pytest.raises(NotImplementedError):
        getattr(nmf, how)(V3(shape=(2, 1, 4, 4, 4)), weights=np.ones((2, 1, 1, 1, 1)), **kw)


@pytest.mark.parametrize('how,kw', FITS, ids=[f[0] for f in FITS])
def test_weights_are_broadcast_and_materialised_in_V_dtype(how, kw):
    be = _StopAtInit()
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend=be)
    V = V3().astype(np.float32)
    mask = np.array([[[1.]], [[0.]], [[True]]])          # [N, 1, 1]: per-sample weights
    with pytest.raises(_Initialised):
        getattr(nmf, how)(V, weights=mask, **kw)
    G = be.got_weights
    assert G.shape == V.shape and G.dtype == np.float32 and G.flags.writeable
    assert np.array_equal(G, np.broadcast_to(mask, V.shape))


@pytest.mark.parametrize('how,kw', FITS, ids=[f[0] for f in FITS])
def test_nan_in_V_is_accepted_only_under_zero_weight(how, kw):
    V = V3()
    V[1, 0, 2] = np.nan
    G = np.ones(V.shape)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend=_StopAtInit())
    with pytest.raises(AssertionError):
        getattr(nmf, how)(V, weights=G, **kw)
    G[1, 0, 2] = 0.
    with pytest.raises(_Initialised):
        getattr(nmf, how)(V, weights=G, **kw)
    V[1, 1, 5] = -3.
    with pytest.raises(AssertionError):
        getattr(nmf, how)(V, weights=G, **kw)


@pytest.mark.parametrize('how,kw', FITS, ids=[f[0] for f in FITS])
def test_zeros_in_V_for_beta_at_most_zero_count_only_under_positive_weight(how, kw):
    V = V3()
    V[1, 0, 4] = 0.
    G = np.ones(V.shape)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend=_StopAtInit(), beta_loss='itakura-saito')
    with pytest.raises(ValueError):
        getattr(nmf, how)(V, weights=G, **kw)
    G[1, 0, 4] = 0.
    with pytest.raises(_Initialised):
        getattr(nmf, how)(V, weights=G, **kw)


def test_a_weighted_fit_is_not_the_plain_frobenius_objective_and_a_later_fit_is_unweighted():
    be = _WeightedStub()
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend=be)
    V = V3()
    nmf._initialize_matrices(V, False, weights=np.ones(V.shape))
    assert not nmf._plain_frobenius and nmf._objective() == dict(beta=2., eps=nmf.eps)
    assert nmf._scheduler(dict(sparsity=0., inhibition=0., cross_inhibition=0.)) is None
    nmf._initialize_matrices(V, True)
    assert nmf._plain_frobenius and nmf._objective() == {} and be.got_weights is None


# -- the ABI ------------------------------------------------------------------------------------------------------------
def test_abi_8_exports_the_weighted_entry_points():
    assert _lib.ABI_VERSION == 8
    names = ('tnmf_hip_weighted_fields', 'tnmf_hip_update_H_weighted', 'tnmf_hip_grad_W_weighted',
             'tnmf_hip_energy_weighted')
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                               'tnmf_hip.h')).read()
    for name in names:
        assert name in _lib.EXPORTS
        assert f'int {name}(' in header
    lib = _lib.load()
    assert lib.tnmf_hip_abi_version() == 8
    for name in names:
        assert hasattr(lib, name)


# -- planted inpainting ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1])
def test_planted_inpainting_on_the_reference(seed):
    """A weighted fit that leaves the hidden block out reconstructs it at least INPAINT_MARGIN times better than an
    unweighted fit on the zero-filled samples (measured 3.5x and 3.9x)."""
    P = wref.INPAINT
    V, V0, mask = wref.planted(seed)
    np.random.seed(42)
    weighted = wref.WeightedOracleNMF(n_atoms=P['n_atoms'], atom_shape=P['atom_shape'], beta=2., weights=mask,
                                      impl='c').fit(V0, n_iterations=P['iterations'])
    np.random.seed(42)
    zero_filled = orc.OracleNMF(n_atoms=P['n_atoms'], atom_shape=P['atom_shape'], impl='c').fit(
        V0, n_iterations=P['iterations'])
    e_w, e_0 = wref.hole_error(weighted.R, V, mask), wref.hole_error(zero_filled.R, V, mask)
    assert e_0 >= wref.INPAINT_MARGIN * e_w, (e_w, e_0)


def test_weighted_reference_epochs_run():
    """The reference's mini-batch loops take the weighted steps (a smoke test of WeightedOracleNMF's plumbing)."""
    V, _, _ = problem()
    G = np.ones(V.shape)
    G[:, :, 3:6, 4:8] = 0.
    np.random.seed(3)
    a = wref.WeightedOracleNMF(n_atoms=3, atom_shape=(3, 4), beta=1., weights=G).fit(
        V, algorithm=orc.MiniBatchAlgorithm(MiniBatchAlgorithm.ASAG_MU.value), batch_size=2, n_epochs=2)
    V2 = V.copy()
    V2[:, :, 3:6, 4:8] = 7.
    np.random.seed(3)
    b = wref.WeightedOracleNMF(n_atoms=3, atom_shape=(3, 4), beta=1., weights=G).fit(
        V2, algorithm=orc.MiniBatchAlgorithm(MiniBatchAlgorithm.ASAG_MU.value), batch_size=2, n_epochs=2)
    assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H)
