"""
Activation-triggered sums on the host: the NumPy fallback of ``triggered_sums`` for a backend without the hook
(tnmf_amd/backends/_Backend.py) and for windows beyond the kernel's limit -- the semantics of tnmf_hip_triggered_sums
(include/tnmf_hip.h, "triggered sums") in float64 -- and the host algebra on the sums.  Not on the hip path.
"""
import itertools
from typing import Sequence, Tuple

import numpy as np


def triggered_sums_numpy(Hp: np.ndarray, Y: np.ndarray, atom_shape: Sequence[int], margin: Sequence[int], power: int = 1,
                         per_sample: bool = False) -> np.ndarray:
    """``X[p, f, j] = sum_n sum_q Hp[n, p, q]^power Y[n, f, q - (A - 1) - m + j]`` for ``0 <= j_k < A_k + 2 m_k``, over
    the terms whose index of Y lies inside the sample: float64 ``[P, F, *(A + 2 m)]`` summed over the samples, or
    ``[N, P, F, *(A + 2 m)]`` with ``per_sample``.  ``Hp`` is the padded activations ``[N, P, *(D + A - 1)]``
    (``pad_activations_numpy``), ``Y`` a field ``[N, F, *D]``.  One einsum of the two shifted views per window position,
    in float64; a position with no term is 0."""
    Hp, Y = np.asarray(Hp, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    A, m = tuple(int(a) for a in atom_shape), tuple(int(x) for x in margin)
    D, S = Y.shape[2:], Hp.shape[2:]
    assert power in (1, 2) and len(A) == len(m) == len(D) == len(S) and all(x >= 0 for x in m)
    assert Hp.shape[0] == Y.shape[0] and all(s == d + a - 1 for s, d, a in zip(S, D, A))
    if power == 2:
        Hp = Hp * Hp
    N, P, F = Hp.shape[0], Hp.shape[1], Y.shape[1]
    win = tuple(a + 2 * x for a, x in zip(A, m))
    X = np.zeros((N, P, F) + win)
    if N == 0:   # (no sample: nothing to reshape)
        return X if per_sample else X.sum(axis=0)
    for j in itertools.product(*(range(w) for w in win)):
        off = tuple(jk - (a - 1) - x for jk, a, x in zip(j, A, m))         # the index of Y is q + off
        lo = tuple(max(0, -o) for o in off)                                # the q whose index of Y is inside the sample
        hi = tuple(min(s, d - o) for s, d, o in zip(S, D, off))
        if any(h <= l for l, h in zip(lo, hi)):
            continue
        h = Hp[(slice(None), slice(None)) + tuple(slice(l, u) for l, u in zip(lo, hi))]
        y = Y[(slice(None), slice(None)) + tuple(slice(l + o, u + o) for l, u, o in zip(lo, hi, off))]
        X[(Ellipsis,) + j] = np.einsum('npu,nfu->npf', h.reshape(N, P, -1), y.reshape(N, F, -1))
    return X if per_sample else X.sum(axis=0)


def extend_atoms(W: np.ndarray, margin: Sequence[int]) -> np.ndarray:
    """The atoms ``W[P, C, *A]`` zero-extended to the window ``[P, C, *(A + 2 m)]``."""
    return np.pad(np.asarray(W, dtype=np.float64), [(0, 0), (0, 0)] + [(int(x), int(x)) for x in margin])


def tap_gains_from_sums(E: np.ndarray, b: np.ndarray, W_ext: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(gain, step) of every tap of the window: with ``E`` the triggered sums of the weighted residual and ``b`` the
    power-2 sums of the weights, the objective as a function of a change t of ONE tap is ``-t E + t^2 b / 2``; the tap
    must stay >= 0, so ``step = max(E / b, -W_ext)`` where ``b > 0`` (else 0) and ``gain = step E - step^2 b / 2 >= 0``."""
    E, b, W_ext = (np.asarray(x, dtype=np.float64) for x in (E, b, W_ext))
    live = b > 0
    step = np.zeros_like(E)
    step[live] = np.maximum(E[live] / b[live], -W_ext[live])
    return step * E - 0.5 * step * step * b, step


def window_gains(gain: np.ndarray, margin: Sequence[int], n_atoms: int) -> Tuple[np.ndarray, np.ndarray]:
    """(inside, outside) ``[n_atoms]``: the tap gains ``[P, C, *(A + 2 m)]`` summed over an atom's planes, its channels and
    the taps inside / outside ``[m, m + A)``."""
    gain = np.asarray(gain, dtype=np.float64)
    k = len(margin)
    per_atom = gain.reshape((n_atoms, -1) + gain.shape[1:])
    axes = tuple(range(1, per_atom.ndim))
    core = np.zeros(gain.shape[-k:], dtype=bool)
    core[tuple(slice(int(x), w - int(x)) for x, w in zip(margin, gain.shape[-k:]))] = True
    return (per_atom * core).sum(axis=axes), (per_atom * ~core).sum(axis=axes)
