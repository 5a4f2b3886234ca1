"""
What each atom explains and how atoms overlap, on the host: the NumPy fallbacks of ``atom_terms`` and ``atom_gram`` for a
backend without the hooks (tnmf_amd/backends/_Backend.py) -- the semantics of tnmf_hip_atom_terms and tnmf_hip_atom_gram
(include/tnmf_hip.h, "atom terms", "atom Gram") in float64; not on the hip path -- and the algebra on ``(a, B)`` that every
backend's front end runs on the host: joint scale factors, set gains, backward elimination.
"""
import itertools
from typing import Optional, Tuple

import numpy as np

from .backends._Backend import shift_shape as _shift_shape


def pad_activations_numpy(H: np.ndarray, atom_shape: Tuple[int, ...], mode: str) -> np.ndarray:
    """Activations ``H[N, P, *S]`` of a reconstruction mode -> the padded ones ``[N, P, *(D + A - 1)]`` every mode
    reconstructs from in 'valid' form (include/tnmf_hip.h, "reconstruction modes other than 'valid'"): 'full' pads A - 1
    zeros on both sides, 'circular' / 'reflect' pad A - 1 wrapped / mirrored elements on the left."""
    if mode == 'valid':
        return H
    lead = [(0, 0), (0, 0)]
    if mode == 'full':
        return np.pad(H, lead + [(a - 1, a - 1) for a in atom_shape])
    if mode in ('circular', 'reflect'):
        return np.pad(H, lead + [(a - 1, 0) for a in atom_shape], mode='wrap' if mode == 'circular' else 'reflect')
    raise ValueError(f'unknown reconstruction mode {mode!r}')


def atom_terms_numpy(W: np.ndarray, H: np.ndarray, mode: str, V: np.ndarray, G: Optional[np.ndarray] = None,
                     group: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """(a, b), float64 ``[N, P / group]``: with ``R_m`` what the planes ``m * group + t`` of ``W[P, C, *A]`` and of the
    activations ``H[N, P, *S]`` (in the shift shape of ``mode``) add to the reconstruction R of the samples ``V[N, C, *D]``
    and ``d = V - R``: ``a = sum G R_m d`` and ``b = sum G R_m^2`` (``G``: weights of V's shape, None for 1; entries of
    weight 0 add exactly 0 whatever V holds there).  ``a + b / 2`` is what the objective rises by without the atom."""
    parts, gd, g = _parts_and_residual(W, H, mode, V, G, group)
    axes = tuple(range(2, parts.ndim))
    return np.sum(parts * gd[:, None], axis=axes), np.sum(g[:, None] * parts * parts, axis=axes)


def _parts_and_residual(W, H, mode, V, G, group):
    """(R_m ``[N, P / group, C, *D]``, G d with exact zeros where the weight is <= 0, G clipped at 0), float64."""
    W, H = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    A, D = tuple(W.shape[2:]), tuple(V.shape[2:])
    P = W.shape[0]
    if group < 1 or P % group != 0:
        raise ValueError(f'group = {group} does not divide the {P} planes')
    if tuple(H.shape[2:]) != _shift_shape(mode, D, A) or H.shape[:2] != (V.shape[0], P):
        raise ValueError(f'activations of shape {H.shape} do not fit {P} planes, mode {mode!r} and samples {V.shape}')
    Hp = pad_activations_numpy(H, A, mode)
    parts = np.zeros((V.shape[0], P // group, W.shape[1]) + D)
    for p in range(P):
        for tap in itertools.product(*[range(a) for a in A]):
            window = tuple(slice(t, t + d) for t, d in zip(tap, D))
            w = W[(p, slice(None)) + tuple(a - 1 - t for a, t in zip(A, tap))]
            parts[:, p // group] += Hp[(slice(None), p, None) + window] * w.reshape((1, -1) + (1,) * len(D))
    g = np.ones(V.shape) if G is None else np.asarray(G, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        gd = np.where(g > 0, g * (np.asarray(V, dtype=np.float64) - parts.sum(axis=1)), 0.)
    g = np.where(g > 0, g, 0.)
    return parts, gd, g


def atom_gram_numpy(W: np.ndarray, H: np.ndarray, mode: str, V: np.ndarray, G: Optional[np.ndarray] = None,
                    group: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """(a, B), float64 ``[N, Mo]`` and ``[N, Mo, Mo]`` with ``Mo = P / group``: ``a`` of ``atom_terms_numpy`` and
    ``B[n, m, m'] = sum G R_m R_m'``, symmetric, whose diagonal is ``b`` (same operands, same treatment of weights)."""
    parts, gd, g = _parts_and_residual(W, H, mode, V, G, group)
    N, Mo = parts.shape[:2]
    flat = parts.reshape(N, Mo, -1)
    B = np.einsum('nmx,nkx->nmk', flat * g.reshape(N, 1, -1), flat)
    B = 0.5 * (B + B.transpose(0, 2, 1))
    b = np.sum(g[:, None] * parts * parts, axis=tuple(range(2, parts.ndim)))
    B[:, np.arange(Mo), np.arange(Mo)] = b
    return np.sum(parts * gd[:, None], axis=tuple(range(2, parts.ndim))), B


def _divergence_factors(parts, V, g, beta, eps):
    """(R, x, V, G (V x^(beta-2) - x^(beta-1)), G c) of include/tnmf_hip.h, "atom terms, beta": V and the two factors
    with exact zeros where the weight is <= 0 (``g``: the weights clipped at 0), whatever V holds there."""
    R = parts.sum(axis=1)
    x = np.maximum(R, 0.) + eps
    with np.errstate(invalid='ignore', over='ignore'):
        v = np.where(g > 0, np.asarray(V, dtype=np.float64), 0.)
        gd = g * ((v - x) * x ** (beta - 2.))
        gc = g * (((beta - 1.) * x + (2. - beta) * v) * x ** (beta - 3.))
    return R, x, v, np.where(g > 0, gd, 0.), np.where(g > 0, gc, 0.)


def atom_divergence_terms_numpy(W: np.ndarray, H: np.ndarray, mode: str, V: np.ndarray, G: Optional[np.ndarray] = None,
                                group: int = 1, beta: float = 1., eps: float = 1e-9
                                ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(a, b, gain), float64 ``[N, P / group]``, under the beta-divergence (include/tnmf_hip.h, "atom terms, beta"): with
    ``r = R_m`` of ``atom_terms_numpy``, ``x = max(R, 0) + eps`` and ``x_m = max(R - r, 0) + eps``,
    ``a = sum G r (V x^(beta-2) - x^(beta-1))``, ``b = sum G r^2 c`` with ``c = (beta-1) x^(beta-2) + (2-beta) V x^(beta-3)``
    and ``gain = sum G (D_beta(V | x_m) - D_beta(V | x))``, the last in the forms of the header in which nothing cancels.
    ``beta == 2``: ``atom_terms_numpy`` and ``a + b / 2``."""
    if beta == 2:
        a, b = atom_terms_numpy(W, H, mode, V, G, group)
        return a, b, a + b / 2
    parts, _, g = _parts_and_residual(W, H, mode, V, G, group)
    R, x, v, gd, gc = _divergence_factors(parts, V, g, float(beta), float(eps))
    axes = tuple(range(2, parts.ndim))
    a = np.sum(parts * gd[:, None], axis=axes)
    b = np.sum(gc[:, None] * parts * parts, axis=axes)
    c0, rm = np.maximum(R, 0.)[:, None], R[:, None] - parts
    # x - x_m, from R_m itself where neither clamp acts (the rounding of R - R_m is of the size of R, not of R_m)
    dx = np.where(rm > 0, np.where(R[:, None] > 0, parts, -rm), c0)
    xm, x, v = np.maximum(rm, 0.) + eps, x[:, None], v[:, None]
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        l1p = np.log1p(dx / xm)   # log(x / x_m)
        if beta == 1:
            term = np.where(v > 0, v * l1p, 0.) - dx
        elif beta == 0:
            term = v * (dx / (x * xm)) - l1p
        else:
            p1 = x ** (beta - 1.)
            term = ((beta - 1.) * (p1 * x) * np.expm1(-beta * l1p) - beta * v * p1 * np.expm1((1. - beta) * l1p)) \
                / (beta * (beta - 1.))
        term = np.where((g[:, None] > 0) & (parts != 0), g[:, None] * term, 0.)
    return a, b, np.sum(term, axis=axes)


def atom_divergence_gram_numpy(W: np.ndarray, H: np.ndarray, mode: str, V: np.ndarray, G: Optional[np.ndarray] = None,
                               group: int = 1, beta: float = 1., eps: float = 1e-9) -> Tuple[np.ndarray, np.ndarray]:
    """(a, B), float64 ``[N, Mo]`` and ``[N, Mo, Mo]``: ``a`` of ``atom_divergence_terms_numpy`` and
    ``B[n, m, m'] = sum G c R_m R_m'``, symmetric, whose diagonal is its ``b``; the weights ``G c`` are signed.
    ``beta == 2``: ``atom_gram_numpy``."""
    if beta == 2:
        return atom_gram_numpy(W, H, mode, V, G, group)
    parts, _, g = _parts_and_residual(W, H, mode, V, G, group)
    _, _, _, gd, gc = _divergence_factors(parts, V, g, float(beta), float(eps))
    N, Mo = parts.shape[:2]
    flat = parts.reshape(N, Mo, -1)
    B = np.einsum('nmx,nkx->nmk', flat * gc.reshape(N, 1, -1), flat)
    B = 0.5 * (B + B.transpose(0, 2, 1))
    axes = tuple(range(2, parts.ndim))
    B[:, np.arange(Mo), np.arange(Mo)] = np.sum(gc[:, None] * parts * parts, axis=axes)
    return np.sum(parts * gd[:, None], axis=axes), B


# -- the algebra on (a, B): E(s) = E(1) - a^T (s - 1) + 1/2 (s - 1)^T B (s - 1) for per-atom scale factors s ------------------
def gram_drop(a: np.ndarray, B: np.ndarray, s: np.ndarray) -> float:
    """E(1) - E(s): what the objective falls by under the scale factors s."""
    e = np.asarray(s, dtype=np.float64) - 1.
    return float(a @ e - 0.5 * e @ B @ e)


def _min_norm(B, c, idx):
    z = np.zeros(len(c))
    if len(idx):
        z[idx] = np.linalg.lstsq(B[np.ix_(idx, idx)], c[idx], rcond=None)[0]   # (minimum norm where the block is singular)
    return z


def gram_scales(a: np.ndarray, B: np.ndarray, nonnegative: bool = True, fixed_zero=()) -> np.ndarray:
    """The scale factors s that minimise E(s): ``B s = a + B 1``, over ``s >= 0`` when ``nonnegative`` (an active-set
    solve: Lawson and Hanson's NNLS on the normal equations), with ``s[fixed_zero] = 0`` held.  Atoms with ``B[m, m] == 0``
    are dead: they change nothing and keep scale 1.  A singular block gets its minimum-norm solution."""
    a, B = np.asarray(a, dtype=np.float64), np.asarray(B, dtype=np.float64)
    M = len(a)
    s = np.ones(M)
    out = np.zeros(M, dtype=bool)
    out[list(fixed_zero)] = True
    s[out] = 0.
    live = np.flatnonzero((np.diag(B) > 0) & ~out)
    if len(live) == 0:
        return s
    # minimise 1/2 z^T Bl z - c^T z over the live ones; the held ones, at 0, drop out of B s and stay in c = a + B 1
    Bl, c = B[np.ix_(live, live)], (a + B @ np.ones(M))[live]
    every = np.arange(len(live))
    z = _min_norm(Bl, c, every)
    tol = 64 * np.finfo(np.float64).eps * len(live) * max(float(np.max(np.abs(c))), float(np.max(np.abs(Bl @ np.abs(z)))))
    if nonnegative and np.any(z < 0):
        z = np.zeros(len(live))
        passive = np.zeros(len(live), dtype=bool)
        for _ in range(3 * len(live) + 3):
            w = c - Bl @ z
            cand = ~passive & (w > tol)
            if not np.any(cand):
                break
            passive[np.argmax(np.where(cand, w, -np.inf))] = True
            while True:
                t = _min_norm(Bl, c, np.flatnonzero(passive))
                bad = passive & (t <= 0)
                if not np.any(bad):
                    z = t
                    break
                alpha = np.min(z[bad] / (z[bad] - t[bad]))
                z = z + alpha * (t - z)
                passive &= z > tol / max(float(np.max(np.diag(Bl))), 1e-300)
                z[~passive] = 0.
        # atoms at 0 whose gradient vanishes too (duplicates of a passive one) share its load: the minimum-norm solution
        w = c - Bl @ z
        tied = np.flatnonzero(passive | (np.abs(w) <= tol))
        t = _min_norm(Bl, c, tied)
        if np.all(t >= 0) and 0.5 * t @ Bl @ t - c @ t <= 0.5 * z @ Bl @ z - c @ z + tol:
            z = t
    s[live] = z
    return s


def gram_set_gain(a: np.ndarray, B: np.ndarray, atoms) -> float:
    """E(s) - E(1) with ``s[atoms] = 0``: what the objective rises by without the atoms."""
    idx = np.asarray(list(atoms), dtype=np.int64)
    return float(a[idx].sum() + 0.5 * B[np.ix_(idx, idx)].sum())


def gram_elimination(a: np.ndarray, B: np.ndarray, rescale: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """Backward elimination on (a, B) alone -> (order [M] int64, rise [M] float64): each time the atom whose removal
    raises the objective least given those already removed; ``rise[k]`` is the cumulative rise over the model as it stands
    (all scales 1) after ``order[:k + 1]`` are gone.  ``rescale``: the remaining atoms are rescaled optimally (s >= 0) at
    every step, and the rise is measured against the model as it stands all the same (it may start negative)."""
    a, B = np.asarray(a, dtype=np.float64), np.asarray(B, dtype=np.float64)
    M = len(a)
    gone, order, rise = [], [], []
    for _ in range(M):
        best = None
        for m in range(M):
            if m in gone:
                continue
            trial = gone + [m]
            if rescale:
                val = -gram_drop(a, B, gram_scales(a, B, True, trial))
            else:
                val = gram_set_gain(a, B, trial)
            if best is None or val < best[0]:
                best = (val, m)
        gone.append(best[1])
        order.append(best[1])
        rise.append(best[0])
    return np.asarray(order, dtype=np.int64), np.asarray(rise, dtype=np.float64)
