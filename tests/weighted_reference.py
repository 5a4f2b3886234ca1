"""Float64 reference of the weighted multiplicative updates, built from the oracle's own pieces the way
tests/beta_reference.py is (and on top of its fields and divergence).  Shared by tests/test_weights_cpu.py and
tests/test_hip_weights.py.

    beta != 2:  Q = G V R~^(beta-2),  P = G R~^(beta-1)        (R~ = max(R, 0) + eps)
    beta == 2:  Q = G V,              P = G R
    entries with G == 0: Q = P = 0, and they add 0 to the energy sum G * D_beta(V | R)
"""
import numpy as np

import beta_reference as bref
from oracle import tnmf_oracle as orc

EPS = orc.EPS


def fields(V, G, R, beta, eps=EPS, dtype=np.float64):
    """(Q, P) in float64 from operands in the working precision `dtype` (as the kernel forms them)."""
    V = np.asarray(V, dtype=dtype)
    G64 = np.asarray(G, dtype=dtype).astype(np.float64)
    keep = G64 > 0
    Vk = np.where(keep, V, 0).astype(dtype)            # (what V holds under G == 0 is never data)
    if beta == 2:
        Q, P = Vk.astype(np.float64), np.asarray(R, dtype=dtype).astype(np.float64)
    else:
        with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
            Q, P = bref.fields(Vk, R, beta, eps, dtype=dtype)
    with np.errstate(over='ignore', invalid='ignore'):
        return np.where(keep, G64 * Q, 0.), np.where(keep, G64 * P, 0.)


def divergence(V, G, R, beta, eps=EPS):
    """sum G * D_beta(V | max(R, 0) + eps) in float64 (beta == 2: sum 1/2 G (V - R)^2); G == 0 entries add 0."""
    G = np.asarray(G, dtype=np.float64)
    keep = G > 0
    V = np.where(keep, np.asarray(V, dtype=np.float64), 1.)   # (any value where the weight is 0: never reaches the sum)
    R = np.asarray(R, dtype=np.float64)
    if beta == 2:
        d = 0.5 * np.square(V - R)
    else:
        Rt = np.maximum(R, 0.) + eps
        with np.errstate(divide='ignore', invalid='ignore'):
            if beta == 1:
                d = np.where(V > 0, V * np.log(np.where(V > 0, V, 1.) / Rt), 0.) - V + Rt
            elif beta == 0:
                x = V / Rt
                d = x - np.log(x) - 1.
            else:
                d = (V ** beta + (beta - 1.) * Rt ** beta - beta * V * Rt ** (beta - 1.)) / (beta * (beta - 1.))
    return float(np.sum(np.where(keep, G * d, 0.)))


def update_H(V, G, W, H, s=slice(None), beta=2., eps=EPS, sparsity=0., inhibition=0., cross_inhibition=0.,
             kernels=None, mode='valid'):
    """One weighted H half step on H[s], in place."""
    A = W.shape[2:]
    Hs = H[s]
    Hp = orc.pad_activations(Hs, A, mode)
    Q, P = fields(V[s], G[s], orc.reconstruct(W, Hp, bref.IMPL), beta, eps)
    neg = orc.fold_gradient(orc._correlate_with_W(W, Q, bref.IMPL), Hs.shape[2:], A, mode)
    pos = orc.fold_gradient(orc._correlate_with_W(W, P, bref.IMPL), Hs.shape[2:], A, mode)
    if inhibition > 0 or cross_inhibition > 0:
        k = len(A)
        g = orc.convolve_multi_1d(Hs, kernels, range(-k, 0))
        if inhibition > 0:
            pos = pos + inhibition * (g - Hs)
        if cross_inhibition > 0:
            pos = pos + (cross_inhibition / (W.shape[0] - 1)) * (g.sum(axis=1, keepdims=True) - g)
    orc.multiplicative_update(Hs, neg, np.array(pos), eps, sparsity)


def gradient_W(V, G, W, H, s=slice(None), beta=2., eps=EPS, mode='valid'):
    A = W.shape[2:]
    Hp = orc.pad_activations(H[s], A, mode)
    Q, P = fields(V[s], G[s], orc.reconstruct(W, Hp, bref.IMPL), beta, eps)
    return orc._correlate_H_with(Q, Hp, A, bref.IMPL), orc._correlate_H_with(P, Hp, A, bref.IMPL)


def update_W(V, G, W, H, s=slice(None), beta=2., eps=EPS, mode='valid'):
    neg, pos = gradient_W(V, G, W, H, s, beta, eps, mode)
    orc.multiplicative_update(W, neg, pos, eps, normalization_axes=tuple(range(-(W.ndim - 2), 0)))


def energy(V, G, W, H, beta, eps=EPS, mode='valid'):
    return divergence(V, G, orc.reconstruct(W, H, bref.IMPL, mode), beta, eps)


class WeightedOracleNMF(bref.BetaOracleNMF):
    """The oracle's fit loops (batch and the five mini-batch schedules, same RNG use) on the weighted steps above.
    `weights` broadcasts to the V given to fit; V must be non-negative everywhere (the oracle's own check)."""

    def __init__(self, *args, weights=None, **kw):
        super().__init__(*args, **kw)
        self.weights = weights
        self.G = None

    def _init(self, V, keep_W):
        super()._init(V, keep_W)
        self.G = np.broadcast_to(np.asarray(self.weights, dtype=np.float64), V.shape)

    def energy(self) -> float:
        return energy(self.V, self.G, self.W, self.H, self.beta, self.eps, self.mode)

    def update_H(self, s=slice(None), sparsity=0., inhibition=0., cross_inhibition=0.):
        update_H(self.V, self.G, self.W, self.H, s, self.beta, self.eps, sparsity, inhibition, cross_inhibition,
                 self._kernels, self.mode)

    def update_W(self, s=slice(None)):
        update_W(self.V, self.G, self.W, self.H, s, self.beta, self.eps, self.mode)

    def _accumulate(self, acc_neg, acc_pos, lam, s):
        neg, pos = gradient_W(self.V, self.G, self.W, self.H, s, self.beta, self.eps, self.mode)
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


# -- planted inpainting (tests/test_weights_cpu.py fixes the margin, tests/test_hip_weights.py asserts it on the GPU) --
INPAINT_MARGIN = 2.0   # the weighted fit's error in the hole is at least this many times lower than the zero-filled fit's
# (a hole smaller than an atom: every activation that reaches into it also sees visible samples)
INPAINT = dict(shape=(6, 1, 24, 24), n_atoms=4, atom_shape=(7, 7), hole=(slice(9, 13), slice(9, 13)), density=0.1,
               iterations=40)


def planted(seed=0, shape=INPAINT['shape'], n_atoms=INPAINT['n_atoms'], atom_shape=INPAINT['atom_shape'],
            hole=INPAINT['hole'], density=INPAINT['density']):
    """bench.py's synthetic samples in small: V = reconstruct(W*, H*) + 0.01 U, W* ~ U normalised, H* = U * Bernoulli,
    with a block of every sample hidden.  -> (V, V with the hole filled with 0, the 0/1 mask of the visible entries)."""
    rng = np.random.default_rng(seed)
    N, C = shape[:2]
    W = rng.random((n_atoms, C) + tuple(atom_shape))
    W /= W.sum(axis=(-2, -1), keepdims=True)
    hshape = (N, n_atoms) + orc.transform_shape(shape[2:], atom_shape)
    H = rng.random(hshape) * (rng.random(hshape) < density)
    V = orc.reconstruct(W, H, 'contract') + 0.01 * rng.random(shape)
    mask = np.ones(shape)
    mask[(slice(None), slice(None)) + tuple(hole)] = 0.
    return V, V * mask, mask


def hole_error(R, V, mask):
    """Root-mean-square error of the reconstruction R inside the hole (mask == 0)."""
    hole = np.broadcast_to(mask, V.shape) == 0
    return float(np.sqrt(np.mean(np.square(np.asarray(R, dtype=np.float64)[hole] - V[hole]))))
