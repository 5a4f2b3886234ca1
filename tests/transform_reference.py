"""Float64 reference of the transform-invariant model (TransformInvariantNMF(..., transforms=...)), built the way
tests/beta_reference.py and tests/weighted_reference.py are: W is expanded EXPLICITLY into the effective atoms with the
numpy operations that define the groups, the oracle's steps run on the effective problem, and the W gradient is folded back
with the inverse operations.  Shared by tests/test_transforms_cpu.py and tests/test_hip_transforms.py.

    W_eff[m*T + t, c] = T_t(W[m, c])                      (a = W[m, c]; the table below)
    H step:  the (weighted, beta) H step of the effective problem, M*T atoms
    W step:  neg[m] = sum_t T_t^-1(neg_eff[m*T + t]), pos likewise;  W <- W * neg / (pos + eps), normalised;  re-expand
"""
import numpy as np

import beta_reference as bref
import weighted_reference as wref
from oracle import tnmf_oracle as orc

EPS = orc.EPS


def _rot(k):
    return lambda a: np.rot90(a, k)


def _rot_inv(k):
    return lambda a: np.rot90(a, -k)


def _mirror_rot(k):
    return lambda a: np.rot90(a[:, ::-1], k)


def _mirror_rot_inv(k):
    return lambda a: np.rot90(a, -k)[:, ::-1]


# name -> ([T_t], [T_t^-1]) on one atom channel a (2-D); 'flip' on 1-D atoms is a[::-1]
GROUPS_2D = {
    'flip': ([lambda a: a, lambda a: a[:, ::-1]], [lambda a: a, lambda a: a[:, ::-1]]),
    'mirrors': ([lambda a: a, lambda a: a[:, ::-1], lambda a: a[::-1, :], lambda a: a[::-1, ::-1]],
                [lambda a: a, lambda a: a[:, ::-1], lambda a: a[::-1, :], lambda a: a[::-1, ::-1]]),
    'rot90': ([_rot(k) for k in range(4)], [_rot_inv(k) for k in range(4)]),
    'dihedral': ([_rot(k) for k in range(4)] + [_mirror_rot(k) for k in range(4)],
                 [_rot_inv(k) for k in range(4)] + [_mirror_rot_inv(k) for k in range(4)]),
}
GROUPS_1D = {'flip': ([lambda a: a, lambda a: a[::-1]], [lambda a: a, lambda a: a[::-1]])}


def ops(name, ndim):
    return (GROUPS_2D if ndim == 2 else GROUPS_1D)[name]


def n_transforms(name):
    return len(GROUPS_2D[name][0])


def expand(W, name):
    """W[M, C, *A] -> W_eff[M*T, C, *A]."""
    fwd, _ = ops(name, W.ndim - 2)
    M, C = W.shape[:2]
    return np.array([[fwd[t](W[m, c]) for c in range(C)] for m in range(M) for t in range(len(fwd))])


def fold(X, name):
    """X[M*T, C, *A] -> [M, C, *A]: sum over t of T_t^-1(X[m*T + t]), ascending t, in float64."""
    _, inv = ops(name, X.ndim - 2)
    T = len(inv)
    M, C = X.shape[0] // T, X.shape[1]
    out = np.zeros((M, C) + X.shape[2:])
    for m in range(M):
        for c in range(C):
            for t in range(T):
                out[m, c] += inv[t](np.asarray(X[m * T + t, c], dtype=np.float64))
    return out


class TransformOracleNMF(wref.WeightedOracleNMF):
    """The oracle's fit loops (batch, the five mini-batch schedules, the stream; same RNG use) on the transformed model,
    with any beta and optional weights (None: the unweighted objective)."""

    def __init__(self, *args, transforms='flip', weights=None, beta=2., **kw):
        super().__init__(*args, weights=weights, beta=beta, **kw)
        self.transforms = transforms
        self.T = n_transforms(transforms)
        self.W_eff = None

    def _init(self, V, keep_W):
        # the reference's convention with the effective atom count: H = 1 - rand(N, M*T, *shift) first, then
        # W = 1 - rand(M, C, *A), normalised
        self.V = V
        shifts = orc.transform_shape(V.shape[2:], self.atom_shape, self.mode)
        self.H = np.asarray(1 - np.random.rand(V.shape[0], self.n_atoms * self.T, *shifts), dtype=V.dtype)
        if not keep_W or self.W is None:
            self.W = np.asarray(1 - np.random.rand(self.n_atoms, V.shape[1], *self.atom_shape), dtype=V.dtype)
            orc.normalize(self.W, self._norm_axes)
        self.G = np.broadcast_to(np.asarray(1. if self.weights is None else self.weights, dtype=np.float64), V.shape)
        self.W_eff = expand(self.W, self.transforms)

    @property
    def R(self):
        return orc.reconstruct(self.W_eff, self.H, bref.IMPL, self.mode)

    def R_partial(self, i_atom):
        eff = slice(i_atom * self.T, (i_atom + 1) * self.T)
        return orc.reconstruct(self.W_eff[eff], self.H[:, eff], bref.IMPL, self.mode)

    def energy(self) -> float:
        return wref.energy(self.V, self.G, self.W_eff, self.H, self.beta, self.eps, self.mode)

    def update_H(self, s=slice(None), sparsity=0., inhibition=0., cross_inhibition=0.):
        wref.update_H(self.V, self.G, self.W_eff, self.H, s, self.beta, self.eps, sparsity, inhibition, cross_inhibition,
                      self._kernels, self.mode)

    def gradient_W(self, s=slice(None)):
        neg, pos = wref.gradient_W(self.V, self.G, self.W_eff, self.H, s, self.beta, self.eps, self.mode)
        return fold(neg, self.transforms), fold(pos, self.transforms)

    def _mu_W(self, neg, pos):
        super()._mu_W(neg, pos)
        self.W_eff = expand(self.W, self.transforms)

    def update_W(self, s=slice(None)):
        self._mu_W(*self.gradient_W(s))

    def _accumulate(self, acc_neg, acc_pos, lam, s):
        neg, pos = self.gradient_W(s)
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

    @property
    def H4(self):
        """H as [N, M, T, *shift] (the front end's read-out)."""
        return self.H.reshape((self.H.shape[0], self.n_atoms, self.T) + self.H.shape[2:])


# -- a planted rotated motif (tests/test_transforms_cpu.py fixes the margin, tests/test_hip_transforms.py asserts it) --
PLANTED = dict(shape=(6, 1, 28, 28), atom_shape=(6, 6), density=0.01, noise=0.01, iterations=40)
# a 'rot90' fit with one atom ends at least this many times lower in energy than a plain one (measured 3.9x to 5.8x)
PLANTED_MARGIN = 3.0


def planted(seed=0, shape=PLANTED['shape'], atom_shape=PLANTED['atom_shape'], density=PLANTED['density'],
            noise=PLANTED['noise']):
    """V = sum over the four rotations of ONE asymmetric motif, each placed at sparse random shifts, + noise U."""
    rng = np.random.default_rng(seed)
    a = np.zeros(atom_shape)
    a[0, :] = 1.                   # an 'L' with a dot: no rotation of it equals another
    a[:, 0] = 1.
    a[atom_shape[0] // 2, atom_shape[1] - 2] = 1.
    a /= a.sum()
    W = np.array([[np.rot90(a, k)] for k in range(4)])
    hshape = (shape[0], 4) + orc.transform_shape(shape[2:], atom_shape)
    H = rng.random(hshape) * (rng.random(hshape) < density)
    return orc.reconstruct(W, H, 'contract') + noise * rng.random(shape)
