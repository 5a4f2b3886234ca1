"""
TEST-ONLY reference of the events (include/tnmf_hip.h, "events"): float64, written straight from the image table and on
purpose naive -- one Python loop per event, per image and per pixel.  Independent of the front end's host fallback
(tnmf_amd.TransformInvariantNMF.events_numpy), which clips slices per image.
"""
import itertools

import numpy as np


def shift_shape(D, A, mode):
    return tuple({'valid': d + a - 1, 'full': d - a + 1}.get(mode, d) for d, a in zip(D, A))


def axis_images(u, a, S, mode):
    """The padded positions of the shift u on one axis (atom extent a, shift extent S)."""
    if mode == 'valid':
        return [u]
    if mode == 'full':
        return [u + a - 1]
    if mode == 'circular':
        return [u + a - 1] + ([u - (S - (a - 1))] if u >= S - (a - 1) else [])
    if mode == 'reflect':
        return [u + a - 1] + ([(a - 1) - u] if 1 <= u <= a - 1 else [])
    raise ValueError(mode)


def images(u, A, S, mode):
    return list(itertools.product(*[axis_images(int(x), a, s, mode) for x, a, s in zip(u, A, S)]))


def pixels(W, D, mode, n, p, u):
    """Every (index into [N, C, *D], entry of W) an event at (n, p, u) touches, images and channels included."""
    A = W.shape[2:]
    S = shift_shape(D, A, mode)
    for q in images(u, A, S, mode):
        for c in range(W.shape[1]):
            for j in itertools.product(*[range(a) for a in A]):
                x = tuple(qq - (a - 1) + jj for qq, a, jj in zip(q, A, j))
                if all(0 <= xx < d for xx, d in zip(x, D)):
                    yield (int(n), c) + x, float(W[(int(p), c) + j])


def render(W, D, N, mode, sample, plane, shift, strength):
    """R[N, C, *D] in float64: the sum over all images of all events."""
    R = np.zeros((N, W.shape[1]) + tuple(D))
    for n, p, u, h in zip(sample, plane, np.asarray(shift).reshape(len(sample), -1), strength):
        for at, w in pixels(W, D, mode, n, p, u):
            R[at] += float(h) * w
    return R


def refit(V, W, mode, sample, plane, shift, strength, n_iterations, sparsity=0., eps=1e-9):
    """The strengths after n_iterations of h <- h * neg / (pos + eps + sparsity) in float64."""
    D, N = V.shape[2:], V.shape[0]
    V = np.asarray(V, dtype=np.float64)
    h = np.array(strength, dtype=np.float64)
    shift = np.asarray(shift).reshape(len(sample), -1)
    reg = eps + (sparsity if sparsity > 0 else 0.)
    for _ in range(n_iterations):
        R = render(W, D, N, mode, sample, plane, shift, h)
        new = np.empty_like(h)
        for e, (n, p, u) in enumerate(zip(sample, plane, shift)):
            neg = pos = 0.
            for at, w in pixels(W, D, mode, n, p, u):
                neg += w * V[at]
                pos += w * R[at]
            new[e] = h[e] * neg / (pos + reg)
        h = new
    return h


def scatter(N, P, S, sample, plane, shift, strength, dtype=np.float64):
    """The dense activations [N, P, *S] that hold the strengths at the events (added up) and zero elsewhere."""
    H = np.zeros((N, P) + tuple(S), dtype=dtype)
    for n, p, u, h in zip(sample, plane, np.asarray(shift).reshape(len(sample), -1), strength):
        H[(int(n), int(p)) + tuple(int(x) for x in u)] += h
    return H
