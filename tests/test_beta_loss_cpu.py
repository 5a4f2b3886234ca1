"""beta_loss of TransformInvariantNMF without a GPU: parsing, the checks fit makes, the backend contract, the ABI of the
beta entry points, and the test suite's own float64 reference of the D_beta updates (tests/beta_reference.py)."""
import numpy as np
import pytest

import beta_reference as bref
from oracle import tnmf_oracle as orc
from oracle_backend import OracleBackend
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF, beta_loss_value


@pytest.mark.parametrize('value, beta', [('frobenius', 2.), ('kullback-leibler', 1.), ('itakura-saito', 0.),
                                         (2, 2.), (1.5, 1.5), (0., 0.), (-0.5, -0.5), (np.float32(3), 3.)])
def test_beta_loss_parsing(value, beta):
    assert beta_loss_value(value) == beta
    if beta == 2.:
        nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend=OracleBackend(), beta_loss=value)
        assert nmf.beta_loss == 2.


@pytest.mark.parametrize('value', ['kl', 'Frobenius', 'euclidean', None, float('nan'), float('inf'), True, [1.], '1'])
def test_beta_loss_rejected(value):
    with pytest.raises(ValueError):
        beta_loss_value(value)
    with pytest.raises(ValueError):
        TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend=OracleBackend(), beta_loss=value)


@pytest.mark.parametrize('value', ['kullback-leibler', 'itakura-saito', 1.5])
def test_backend_without_beta_hooks_is_refused(value):
    with pytest.raises(NotImplementedError):
        TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend=OracleBackend(hooks=True), beta_loss=value)


class _BetaHooks(OracleBackend):
    """An oracle backend that claims the beta hooks (never called here: fit refuses the samples first)."""

    supports_beta_loss = True


@pytest.mark.parametrize('beta', ['itakura-saito', -1.])
@pytest.mark.parametrize('how', ['fit_batch', 'fit_minibatches'])
def test_zeros_in_V_are_refused_for_beta_at_most_zero_by_a_beta_backend(beta, how):
    V = np.random.default_rng(0).random((3, 1, 8)) + 0.1
    V[1, 0, 4] = 0.
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3,), backend=_BetaHooks(), beta_loss=beta)
    with pytest.raises(ValueError):
        getattr(nmf, how)(V, **({'n_iterations': 1} if how == 'fit_batch' else {'n_epochs': 1}))


def test_abi_8_exports_the_beta_entry_points():
    assert _lib.ABI_VERSION == 8
    for name in ('tnmf_hip_beta_fields', 'tnmf_hip_update_H_beta', 'tnmf_hip_grad_W_beta', 'tnmf_hip_energy_beta'):
        assert name in _lib.EXPORTS
    lib = _lib.load()
    assert lib.tnmf_hip_abi_version() == 8
    for name in _lib.EXPORTS:
        assert hasattr(lib, name)


@pytest.mark.parametrize('mode', ['valid', 'full'])
def test_reference_at_beta_2_is_the_oracle_step(mode):
    rng = np.random.default_rng(5)
    V = rng.random((3, 2, 10, 11))
    A = (3, 4)
    np.random.seed(1)
    W, H = orc.init_matrices(V, A, 4, mode=mode)
    W2, H2 = W.copy(), H.copy()
    for _ in range(3):
        neg, pos = orc.gradient_H(V, W, H, mode=mode)
        orc.multiplicative_update(H, neg, pos, sparsity=0.1)
        neg, pos = orc.gradient_W(V, W, H, mode=mode)
        orc.multiplicative_update(W, neg, pos, normalization_axes=(-2, -1))
        bref.update_H(V, W2, H2, beta=2., sparsity=0.1, mode=mode)
        bref.update_W(V, W2, H2, beta=2., mode=mode)
    assert np.abs(W2 - W).max() <= 1e-12 * np.abs(W).max()
    assert np.abs(H2 - H).max() <= 1e-12 * np.abs(H).max()
    assert abs(bref.energy(V, W2, H2, 2., mode=mode) - orc.energy(V, W, H, mode=mode)) <= 1e-12 * orc.energy(V, W, H, mode=mode)


def test_reference_kl_decreases_the_divergence():
    """Sanity of the reference itself: plain MU on KL does not increase D_1 with W fixed."""
    rng = np.random.default_rng(2)
    V = rng.random((2, 1, 12, 12)) + 0.05
    np.random.seed(3)
    W, H = orc.init_matrices(V, (3, 3), 3)
    e = [bref.energy(V, W, H, 1.)]
    for _ in range(10):
        bref.update_H(V, W, H, beta=1.)
        e.append(bref.energy(V, W, H, 1.))
    assert all(b <= a * (1 + 1e-12) for a, b in zip(e, e[1:]))
