"""
Which planes of H co-occur, and at what offset, on the host: the NumPy fallback of ``activation_correlogram`` for a backend
without the hook (tnmf_amd/backends/_Backend.py) -- the semantics of tnmf_hip_activation_correlogram (include/tnmf_hip.h,
"activation correlogram") -- and the host algebra on the result.  Not on the hip path.
"""
import itertools
from typing import Sequence, Tuple

import numpy as np


def activation_correlogram_numpy(H: np.ndarray, max_lag: Sequence[int], per_sample: bool = False) -> np.ndarray:
    """``C[n, p, q, D] = sum_u H[n, p, u] H[n, q, u + D]`` over the u with u and u + D inside the plane, for the lags
    ``|D_k| <= max_lag[k]``, stored at index ``D_k + max_lag[k]``: float64 ``[P, P, *(2 L + 1)]`` summed over the samples,
    or ``[N, P, P, *(2 L + 1)]`` with ``per_sample``.  ``H`` is ``[N, P, *S]``; nothing wraps, and lags at or beyond the
    extent of an axis are 0.  One product of the two shifted views per lag of the half that is >= 0 in C order, in float64;
    the other half is its mirror ``C[q, p, -D]``, the same numbers."""
    H = np.asarray(H, dtype=np.float64)
    S, L = H.shape[2:], tuple(int(x) for x in max_lag)
    assert len(L) == len(S) and all(x >= 0 for x in L)
    N, P = H.shape[:2]
    C = np.zeros((N, P, P) + tuple(2 * x + 1 for x in L))
    for lag in itertools.product(*(range(-min(x, s - 1), min(x, s - 1) + 1) for x, s in zip(L, S))):
        if lag < (0,) * len(L):
            continue
        a = H[(slice(None), slice(None)) + tuple(slice(max(0, -d), s - max(0, d)) for d, s in zip(lag, S))]
        b = H[(slice(None), slice(None)) + tuple(slice(max(0, d), s - max(0, -d)) for d, s in zip(lag, S))]
        c = np.einsum('npu,nqu->npq', a.reshape(N, P, -1), b.reshape(N, P, -1))
        C[(Ellipsis,) + tuple(d + x for d, x in zip(lag, L))] = c
        C[(Ellipsis,) + tuple(x - d for d, x in zip(lag, L))] = c.transpose(0, 2, 1)
    return C if per_sample else C.sum(axis=0)


def cooccurrence(C: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(score [P, P], lag [P, P, k]) of a correlogram ``C[P, P, *(2 L + 1)]``: ``score[p, q]`` is the largest
    ``C[p, q, D] / sqrt(C[p, p, 0] C[q, q, 0])`` over the lags -- for p == q without D = 0 -- and ``lag`` the D that
    reaches it, the first in C order on a tie.  A plane with ``C[p, p, 0] == 0`` scores 0 (and with no lag but 0 the
    diagonal does, at lag 0)."""
    C = np.asarray(C, dtype=np.float64)
    P, win = C.shape[0], C.shape[2:]
    L = tuple(w // 2 for w in win)
    centre = int(np.ravel_multi_index(L, win))
    flat = C.reshape(P, P, -1).copy()
    energy = flat[np.arange(P), np.arange(P), centre].copy()
    flat[np.arange(P), np.arange(P), centre] = -np.inf   # (p == q: D = 0 does not compete)
    best = flat.argmax(axis=2)                            # (the first of equal maxima)
    top = np.take_along_axis(flat, best[..., None], axis=2)[..., 0]
    norm = np.sqrt(np.outer(energy, energy))
    live = (norm > 0) & np.isfinite(top)
    score = np.zeros((P, P))
    score[live] = np.minimum(top[live] / norm[live], 1.)   # (Cauchy-Schwarz; the rounding of the quotient aside)
    best = np.where(np.isfinite(top), best, centre)
    lag = np.stack(np.unravel_index(best, win), axis=-1).astype(np.int64) - np.asarray(L, dtype=np.int64)
    return score, lag
