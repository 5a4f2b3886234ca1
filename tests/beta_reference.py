"""Float64 reference of the beta-divergence multiplicative updates, built from the oracle's own pieces
(reconstruct, _correlate_with_W, _correlate_H_with, normalize, multiplicative_update) plus numpy for the fields and
D_beta.  Shared by tests/test_beta_loss_cpu.py and tests/test_hip_beta.py.

    R~ = max(R, 0) + eps,  Q = V * R~^(beta-2),  P = R~^(beta-1)   (beta == 2: Q = V, P = R -- the Frobenius step itself)
    H <- H * corr_W(W, Q) / (corr_W(W, P) + eps + sparsity [+ lateral terms])
    W <- W * corr_H(H, Q) / (corr_H(H, P) + eps), normalised
"""
import numpy as np

from oracle import tnmf_oracle as orc

EPS = orc.EPS
IMPL = 'contract'   # the oracle's contraction flavour ('c': its C flavour, for the larger GPU-test problems)


def fields(V, R, beta, eps=EPS, dtype=np.float64):
    """(Q, P) in the working precision `dtype` (R~ formed in that precision, as the kernel does)."""
    V = np.asarray(V, dtype=dtype)
    R = np.asarray(R, dtype=dtype)
    Rt = np.maximum(R, dtype(0)) + dtype(eps)
    Rt64, V64 = Rt.astype(np.float64), V.astype(np.float64)
    return V64 * Rt64 ** (beta - 2.), Rt64 ** (beta - 1.)


def divergence(V, R, beta, eps=EPS):
    """sum D_beta(V | max(R, 0) + eps) in float64 (beta == 2: 1/2 sum (V - R)^2)."""
    V = np.asarray(V, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    if beta == 2:
        return float(0.5 * np.sum(np.square(V - R)))
    Rt = np.maximum(R, 0.) + eps
    if beta == 1:
        with np.errstate(divide='ignore', invalid='ignore'):
            vlog = np.where(V > 0, V * np.log(np.where(V > 0, V, 1.) / Rt), 0.)
        return float(np.sum(vlog - V + Rt))
    if beta == 0:
        x = V / Rt
        return float(np.sum(x - np.log(x) - 1.))
    return float(np.sum((V ** beta + (beta - 1.) * Rt ** beta - beta * V * Rt ** (beta - 1.)) / (beta * (beta - 1.))))


def _qp(V, R, beta, eps):
    if beta == 2:
        return V, R
    return fields(V, R, beta, eps)


def update_H(V, W, H, s=slice(None), beta=1., eps=EPS, sparsity=0., inhibition=0., cross_inhibition=0.,
             kernels=None, mode='valid'):
    """One H half step on H[s], in place."""
    A = W.shape[2:]
    Hs = H[s]
    Hp = orc.pad_activations(Hs, A, mode)
    Q, P = _qp(V[s], orc.reconstruct(W, Hp, IMPL), beta, eps)
    neg = orc.fold_gradient(orc._correlate_with_W(W, Q, IMPL), Hs.shape[2:], A, mode)
    pos = orc.fold_gradient(orc._correlate_with_W(W, P, IMPL), Hs.shape[2:], A, mode)
    if inhibition > 0 or cross_inhibition > 0:
        k = len(A)
        g = orc.convolve_multi_1d(Hs, kernels, range(-k, 0))
        if inhibition > 0:
            pos = pos + inhibition * (g - Hs)
        if cross_inhibition > 0:
            pos = pos + (cross_inhibition / (W.shape[0] - 1)) * (g.sum(axis=1, keepdims=True) - g)
    orc.multiplicative_update(Hs, neg, np.array(pos), eps, sparsity)


def gradient_W(V, W, H, s=slice(None), beta=1., eps=EPS, mode='valid'):
    A = W.shape[2:]
    Hp = orc.pad_activations(H[s], A, mode)
    Q, P = _qp(V[s], orc.reconstruct(W, Hp, IMPL), beta, eps)
    return orc._correlate_H_with(Q, Hp, A, IMPL), orc._correlate_H_with(P, Hp, A, IMPL)


def update_W(V, W, H, s=slice(None), beta=1., eps=EPS, mode='valid'):
    neg, pos = gradient_W(V, W, H, s, beta, eps, mode)
    orc.multiplicative_update(W, neg, pos, eps, normalization_axes=tuple(range(-(W.ndim - 2), 0)))


def energy(V, W, H, beta, eps=EPS, mode='valid'):
    return divergence(V, orc.reconstruct(W, H, IMPL, mode), beta, eps)


class BetaOracleNMF(orc.OracleNMF):
    """The oracle's fit loops (batch and the five mini-batch schedules, same RNG use) on the D_beta steps above."""

    def __init__(self, *args, beta=1., **kw):
        super().__init__(*args, **kw)
        self.beta = beta

    def energy(self) -> float:
        return energy(self.V, self.W, self.H, self.beta, self.eps, self.mode)

    def update_H(self, s=slice(None), sparsity=0., inhibition=0., cross_inhibition=0.):
        update_H(self.V, self.W, self.H, s, self.beta, self.eps, sparsity, inhibition, cross_inhibition, self._kernels,
                 self.mode)

    def update_W(self, s=slice(None)):
        update_W(self.V, self.W, self.H, s, self.beta, self.eps, self.mode)

    def _accumulate(self, acc_neg, acc_pos, lam, s):
        neg, pos = gradient_W(self.V, self.W, self.H, s, self.beta, self.eps, self.mode)
        if lam == 1:
            acc_neg = acc_neg + neg if np.isscalar(acc_neg) else acc_neg.__iadd__(neg)
            acc_pos = acc_pos + pos if np.isscalar(acc_pos) else acc_pos.__iadd__(pos)
        else:
            if np.isscalar(acc_neg):
                acc_neg, acc_pos = acc_neg * (1 - lam) + lam * neg, acc_pos * (1 - lam) + lam * pos
            else:
                acc_neg *= (1 - lam)
                acc_pos *= (1 - lam)
                acc_neg += lam * neg
                acc_pos += lam * pos
        return acc_neg, acc_pos
