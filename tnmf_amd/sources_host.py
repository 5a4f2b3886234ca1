"""
The per-source signals of a fitted model on the host: the NumPy fallbacks of ``separate`` and ``dominant_source`` for a
backend without the hooks (tnmf_amd/backends/_Backend.py) -- the semantics of tnmf_hip_atom_sources (include/tnmf_hip.h,
"sources") in float64, from the per-plane contributions like ``atoms_host.atom_terms_numpy``; not on the hip path.
"""
import itertools
from typing import Sequence, Tuple

import numpy as np

from .atoms_host import pad_activations_numpy
from .backends._Backend import shift_shape as _shift_shape

OUTPUTS = ('contribution', 'mask', 'masked')


def source_tables(sources: Sequence[Sequence[int]], group: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """(plane_order, source_start), int32: the planes ``m * group + t`` of the atoms of each source, source after source,
    and where each source starts in that list (``S + 1`` entries) -- the two tables of tnmf_hip_atom_sources."""
    order = [m * group + t for atoms in sources for m in atoms for t in range(group)]
    start = np.cumsum([0] + [len(atoms) * group for atoms in sources])
    return np.asarray(order, dtype=np.int32), np.asarray(start, dtype=np.int32)


def _source_sums(W, H, mode, D, plane_order, source_start):
    """(r [N, S, C, *D], total [N, C, *D]), float64: per source the sum of its planes' contributions, and the sum over every
    plane (the unlisted ones included)."""
    W, H = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    A, D = tuple(W.shape[2:]), tuple(D)
    P, S = W.shape[0], len(source_start) - 1
    if tuple(H.shape[2:]) != _shift_shape(mode, D, A) or H.shape[1] != P:
        raise ValueError(f'activations of shape {H.shape} do not fit {P} planes, mode {mode!r} and samples of shape {D}')
    owner = np.full(P, S)   # (S: the hidden group)
    for g in range(S):
        owner[np.asarray(plane_order[source_start[g]:source_start[g + 1]], dtype=np.int64)] = g
    Hp = pad_activations_numpy(H, A, mode)
    r = np.zeros((H.shape[0], S + 1, W.shape[1]) + D)
    for p in range(P):
        for tap in itertools.product(*[range(a) for a in A]):
            window = tuple(slice(t, t + d) for t, d in zip(tap, D))
            w = W[(p, slice(None)) + tuple(a - 1 - t for a, t in zip(A, tap))]
            r[:, owner[p]] += Hp[(slice(None), p, None) + window] * w.reshape((1, -1) + (1,) * len(D))
    return r[:, :S], r.sum(axis=1)


def _over(num, den):
    """num / den, and 0 where den is 0"""
    return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape), where=den != 0)


def separate_numpy(W: np.ndarray, H: np.ndarray, mode: str, V: np.ndarray, plane_order, source_start,
                   output: str = 'masked', eps: float = 1e-9) -> np.ndarray:
    """float64 ``[N, S, C, *D]``: per source g -- the planes ``plane_order[source_start[g]:source_start[g + 1]]`` of
    ``W[P, C, *A]`` and of the activations ``H[N, P, *S]`` (in the shift shape of ``mode``) -- its part ``r_g`` of the
    reconstruction of ``V[N, C, *D]`` ('contribution'), ``r_g / (total + eps)`` ('mask') or ``V * (r_g / (total + eps))``
    ('masked'), with ``total`` the sum over every plane, listed or not; 0 where ``total + eps`` is 0."""
    if output not in OUTPUTS:
        raise ValueError(f'output must be one of {OUTPUTS}, not {output!r}')
    r, total = _source_sums(W, H, mode, V.shape[2:], plane_order, source_start)
    if output == 'contribution':
        return r
    mask = _over(r, (total + eps)[:, None])
    return mask if output == 'mask' else np.asarray(V, dtype=np.float64)[:, None] * mask


def dominant_numpy(W: np.ndarray, H: np.ndarray, mode: str, D: Tuple[int, ...], plane_order, source_start,
                   eps: float = 1e-9) -> Tuple[np.ndarray, np.ndarray]:
    """(label int32 ``[N, *D]``, share float64 ``[N, *D]``): per pixel the source with the largest ``sum_c r_g`` -- the
    lowest index of a tie, -1 where ``sum_c total`` is 0 -- and that sum over ``sum_c total + eps``."""
    r, total = _source_sums(W, H, mode, D, plane_order, source_start)
    r, total = r.sum(axis=2), total.sum(axis=1)
    label = np.argmax(r, axis=1)   # (the first of equal maxima)
    best = np.take_along_axis(r, label[:, None], axis=1)[:, 0]
    return np.where(total > 0, label, -1).astype(np.int32), _over(best, total + eps)
