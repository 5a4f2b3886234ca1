"""
TEST-ONLY reference of the atom terms (include/tnmf_hip.h, "atom terms"): float64, independent of the front end's host
fallback (tnmf_amd.atoms_host.atom_terms_numpy, which pads the activations and adds shifted slices).

``parts_loop`` is on purpose naive: every positive activation is an event and every event is placed image by image, pixel by
pixel, per reconstruction mode (events_reference.pixels).  ``parts_valid`` serves the kernel tests, whose operands are padded
activations already: one correlation per plane, written tap by tap over whole samples.
"""
import itertools

import numpy as np

import events_reference as eref


def parts_loop(W, H, D, mode, group=1):
    """R_m[N, P / group, C, *D]: what the planes m * group + t of W[P, C, *A] and H[N, P, *S] add to R, pixel by pixel."""
    W, H = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    parts = np.zeros((H.shape[0], W.shape[0] // group, W.shape[1]) + tuple(D))
    for at in zip(*np.nonzero(H)):
        n, p, u = at[0], at[1], at[2:]
        for (nn, c, *x), w in eref.pixels(W, D, mode, n, p, u):
            parts[(nn, p // group, c) + tuple(x)] += H[at] * w
    return parts


def parts_valid(W, Hp, group=1):
    """The same from PADDED activations Hp[N, P, *(D + A - 1)]: r[x] = sum_a Hp[x + a] W[A - 1 - a]."""
    W, Hp = np.asarray(W, dtype=np.float64), np.asarray(Hp, dtype=np.float64)
    A = W.shape[2:]
    D = tuple(h - a + 1 for h, a in zip(Hp.shape[2:], A))
    parts = np.zeros((Hp.shape[0], W.shape[0] // group, W.shape[1]) + D)
    for p in range(W.shape[0]):
        for tap in itertools.product(*[range(a) for a in A]):
            win = Hp[(slice(None), p) + tuple(slice(t, t + d) for t, d in zip(tap, D))]
            w = W[(p, slice(None)) + tuple(a - 1 - t for a, t in zip(A, tap))]
            parts[:, p // group] += win[:, None] * w.reshape((1, -1) + (1,) * len(D))
    return parts


def terms(parts, V, G=None, R=None):
    """(a, b, scale): a = sum G R_m d, b = sum G R_m^2 with d = V - R (R: the sum of the parts unless given) and
    scale = sum R_m |G d|, the size the rounding of ``a`` is measured against.  Entries of weight 0 count as exact zeros."""
    V = np.asarray(V, dtype=np.float64)
    g = np.ones(V.shape) if G is None else np.asarray(G, dtype=np.float64)
    R = parts.sum(axis=1) if R is None else np.asarray(R, dtype=np.float64)
    gd = np.zeros(V.shape)
    gd[g > 0] = (g * (V - R))[g > 0]
    axes = tuple(range(2, parts.ndim))
    a = np.sum(parts * gd[:, None], axis=axes)
    b = np.sum(g[:, None] * parts ** 2, axis=axes)
    return a, b, np.sum(np.abs(parts) * np.abs(gd[:, None]), axis=axes)
