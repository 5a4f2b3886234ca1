"""
What each atom explains, on the host: the NumPy fallback of ``atom_terms`` for a backend without the hook
(tnmf_amd/backends/_Backend.py) -- the semantics of tnmf_hip_atom_terms (include/tnmf_hip.h, "atom terms") in float64.
Not on the hip path.
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
    axes = tuple(range(2, parts.ndim))
    return np.sum(parts * gd[:, None], axis=axes), np.sum(g[:, None] * parts * parts, axis=axes)
