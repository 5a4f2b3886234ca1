"""
The patches of a list of events on the host (include/tnmf_hip.h, "patches"): the table of the fold into the atom frame that
every backend uses, the NumPy fallbacks of ``event_patches`` and ``event_patch_moments`` for a backend without the hooks
(tnmf_amd/backends/_Backend.py) -- the semantics of tnmf_hip_events_patches and tnmf_hip_patch_moments in float64; not on
the hip path -- and ``modes_from_moments``, the algebra on the four additive moments that every backend's front end (and a
caller who has all-reduced them over a process group) runs on the host.
"""
from typing import Optional, Tuple

import numpy as np

from . import transforms as _transforms
from .events_host import _clip, _occurrence, _shapes, event_images, events_numpy

SOURCES = ('data', 'residual', 'cleaned')
FRAMES = ('atom', 'image')


def fold_table(transforms, atom_shape: Tuple[int, ...]):
    """(fold_ptr [T * nA + 1] int32, fold_src [nnz] int32, fold_w [nnz] float64, T): the table of tnmf_hip_events_patches for
    ``transforms`` (a group name or an ``AtomOperators``; None: (None, None, None, 1), the image frame is the atom frame).
    Row (t, i) holds the entries (t, out pixel, in pixel = i, weight) of the operators in ascending out pixel, fold_src the
    out pixel: ``y[i] = sum fold_w * x[fold_src]`` is ``L_t^T x``.  Built from ``AtomOperators._adjoint()``, a group through
    ``transforms.from_group``."""
    if transforms is None:
        return None, None, None, 1
    ops = transforms if isinstance(transforms, _transforms.AtomOperators) else _transforms.from_group(transforms, atom_shape)
    nA, T = ops.n_pixels, ops.T
    mask, (t, out_px, w) = ops._adjoint()                        # [nA, width]: per in pixel, ascending (t, out pixel)
    in_px = np.broadcast_to(np.arange(nA)[:, None], mask.shape)[mask]
    key = t[mask] * nA + in_px
    order = np.argsort(key, kind='stable')                       # (stable: the out pixels of a row stay ascending)
    ptr = _transforms._csr(key[order], T * nA)
    return (ptr.astype(np.int32), np.ascontiguousarray(out_px[mask][order], dtype=np.int32),
            np.ascontiguousarray(w[mask][order], dtype=np.float64), T)


def fold_patches_numpy(X: np.ndarray, plane, table) -> np.ndarray:
    """``X[K, C, *A]`` in the image frame of the planes ``plane[K]`` -> the atom frame, by the table of ``fold_table``: the
    products of an element summed in table order in float64."""
    ptr, src, w, T = table
    if ptr is None:
        return X
    K, C = X.shape[:2]
    nA = int(np.prod(X.shape[2:]))
    Xf, out = X.reshape(K, C, nA), np.zeros((K, C, nA))
    t_of = np.asarray(plane, dtype=np.int64) % T
    for t in range(T):
        rows = np.flatnonzero(t_of == t)
        if not len(rows):
            continue
        mask, (s, ws) = _transforms._padded(ptr[t * nA:(t + 1) * nA + 1].astype(np.int64), src, w)
        acc = np.zeros((len(rows), C, nA))
        for k in range(mask.shape[1]):
            acc += np.where(mask[:, k], ws[:, k] * Xf[rows][:, :, s[:, k]], 0.)
        out[rows] = acc
    return out.reshape(X.shape)


def event_patches_numpy(W: np.ndarray, sample_shape: Tuple[int, ...], n_samples: int, mode: str, sample, plane, shift,
                        strength, V: np.ndarray, source: str = 'cleaned', transforms=None, frame: str = 'atom') -> np.ndarray:
    """[K, C, *A] float64: the patch of every event, on the host, for backends without ``event_patches`` -- the semantics of
    tnmf_hip_events_patches: the signal (``'data'``: V, ``'residual'``: V - R with R the render of the whole list,
    ``'cleaned'``: V - R + h phi, the list without the row) gathered under every image of the event, pixels outside the
    sample contributing 0; ``frame='atom'`` folds it by the transposed operator of the row's transform.  Not on the hip
    path."""
    assert source in SOURCES and frame in FRAMES
    A, D, shift_shape = _shapes(W, sample_shape, mode)
    W, V = np.asarray(W, dtype=np.float64), np.asarray(V, dtype=np.float64)
    h = np.array(strength, dtype=np.float64).reshape(-1)
    signal = V if source == 'data' else V - events_numpy(W, D, n_samples, mode, sample, plane, shift, h)
    event, q = event_images(shift, A, shift_shape, mode)
    out = np.zeros((len(h), W.shape[1]) + A)
    for e in range(len(h)):
        s = signal[int(sample[e])]
        if source == 'cleaned':
            s = s + h[e] * _occurrence(W, D, shift_shape, mode, int(plane[e]), shift[e])
        for at in q[event == e]:
            clipped = _clip(at, A, D)
            if clipped:
                out[(e, slice(None)) + clipped[1]] += s[(slice(None),) + clipped[0]]
    if frame == 'atom':
        out = fold_patches_numpy(out, plane, fold_table(transforms, A))
    return out


def patch_moments_numpy(Y: np.ndarray, strength, atom, n_atoms: int):
    """(S [M, D, D], g [M, D], s2 [M], count [M]) float64 of the patches ``Y[K, ...]`` (flattened to ``[K, D]``) with the
    strengths ``strength[K]`` and the atoms ``atom[K]`` -- the semantics of tnmf_hip_patch_moments: ``S[m] = sum y y^T``,
    ``g[m] = sum h y``, ``s2[m] = sum h^2``, ``count[m]`` the rows of atom m.  S is symmetric to the bit."""
    Y = np.asarray(Y, dtype=np.float64)
    Y = Y.reshape(len(Y), int(np.prod(Y.shape[1:])))
    h, atom = np.asarray(strength, dtype=np.float64).reshape(-1), np.asarray(atom, dtype=np.int64).reshape(-1)
    D = Y.shape[1]
    S, g, s2, count = np.zeros((n_atoms, D, D)), np.zeros((n_atoms, D)), np.zeros(n_atoms), np.zeros(n_atoms)
    for m in range(n_atoms):
        rows = np.flatnonzero(atom == m)
        upper = np.triu(Y[rows].T @ Y[rows])
        S[m] = upper + np.triu(upper, 1).T
        g[m], s2[m], count[m] = h[rows] @ Y[rows], np.sum(h[rows] * h[rows]), len(rows)
    return S, g, s2, count


def event_patch_moments_numpy(W: np.ndarray, sample_shape: Tuple[int, ...], n_samples: int, mode: str, sample, plane, shift,
                              strength, V: np.ndarray, source: str = 'cleaned', transforms=None,
                              max_rows: Optional[int] = None):
    """(S, g, s2, count) of the list on the host, for backends without ``event_patch_moments``: the atom-frame patches of
    ``event_patches_numpy`` into ``patch_moments_numpy``, the atom of a row being ``plane // T``.  ``max_rows`` is the hip
    backend's chunk length and not used here.  Not on the hip path."""
    T = 1 if transforms is None else _transforms.size(transforms)
    Y = event_patches_numpy(W, sample_shape, n_samples, mode, sample, plane, shift, strength, V, source, transforms, 'atom')
    return patch_moments_numpy(Y, strength, np.asarray(plane, dtype=np.int64) // T, W.shape[0] // T)


def modes_from_moments(S, g, s2, count, n_modes: int):
    """(mean [M, D], modes [M, n_modes, D], variance [M, n_modes], total [M]) float64 from the four additive moments of
    ``atom_patch_moments`` (summed over the ranks of a process group first, where there is one).  Per atom with ``s2 > 0``:
    ``mean = g / s2`` is the least-squares template of the occurrences ``y_e ~ h_e mean``; ``Cm = (S - g g^T / s2) / s2`` is
    the scatter of ``y_e - h_e mean``, weighted as the model weights it; its eigenvectors with the largest eigenvalues are
    the modes, eigenvalues descending and clipped at 0 (``variance``), each mode's sign fixed so that its entry of largest
    magnitude is positive; ``total`` is the trace of Cm clipped at 0.  An atom with fewer than 2 rows or with ``s2 = 0`` gets
    NaN modes and 0 variance and total (and a NaN mean when ``s2 = 0``)."""
    S, g = np.asarray(S, dtype=np.float64), np.asarray(g, dtype=np.float64)
    s2, count = np.asarray(s2, dtype=np.float64).reshape(-1), np.asarray(count, dtype=np.float64).reshape(-1)
    M, D = g.shape
    if S.shape != (M, D, D) or len(s2) != M or len(count) != M:
        raise ValueError(f'modes_from_moments: S {S.shape}, g {g.shape}, s2 {s2.shape} and count {count.shape} do not match')
    if isinstance(n_modes, bool) or int(n_modes) != n_modes or not 1 <= n_modes <= D:
        raise ValueError(f'n_modes must be an integer in [1, {D}], not {n_modes!r}')
    n_modes = int(n_modes)
    mean, modes = np.full((M, D), np.nan), np.full((M, n_modes, D), np.nan)
    variance, total = np.zeros((M, n_modes)), np.zeros(M)
    for m in range(M):
        if not s2[m] > 0:
            continue
        mean[m] = g[m] / s2[m]
        if count[m] < 2:
            continue
        Cm = (S[m] - np.outer(g[m], g[m]) / s2[m]) / s2[m]
        lam, vec = np.linalg.eigh(0.5 * (Cm + Cm.T))
        lam, vec = lam[::-1][:n_modes], vec[:, ::-1][:, :n_modes].T
        sign = np.sign(vec[np.arange(n_modes), np.argmax(np.abs(vec), axis=1)])
        modes[m] = vec * np.where(sign == 0, 1., sign)[:, None]
        variance[m] = np.maximum(lam, 0.)
        total[m] = max(float(np.trace(Cm)), 0.)
    return mean, modes, variance, total
