"""
TEST-ONLY reference of the exact strengths of a list (include/tnmf_hip.h, "events: exact strengths"): float64, the occurrence
of every row written pixel by pixel from the image table of tests/events_reference.py into a dense sample, G_ref = Phi Phi',
c_ref = Phi v, and the KKT conditions of  min 1/2 h'Gh - c'h, h >= 0.  Independent of tnmf_amd/events_host.py, and without a
solver: optimality of a convex quadratic programme is checked by its KKT conditions.
"""
import functools

import numpy as np

import events_reference as eref


def occurrences(W, D, N, mode, sample, plane, shift):
    """Phi [K, N * C * prod(D)]: per row its occurrence phi -- all images, clipped to the sample, images that overlap added --
    laid into the frame of all samples (rows of different samples are orthogonal there)."""
    sample = np.asarray(sample).reshape(-1)
    shift = np.asarray(shift).reshape(len(sample), -1)
    frame = (N, W.shape[1]) + tuple(D)
    Phi = np.zeros((len(sample),) + frame)
    for e, (n, p, u) in enumerate(zip(sample, plane, shift)):
        for at, w in eref.pixels(W, D, mode, n, p, u):
            Phi[(e,) + at] += w
    return Phi.reshape(len(sample), -1)


def gram(V, W, mode, sample, plane, shift):
    """(G_ref [K, K], c_ref [K]) in float64."""
    V = np.asarray(V, dtype=np.float64)
    Phi = occurrences(np.asarray(W, dtype=np.float64), V.shape[2:], V.shape[0], mode, sample, plane, shift)
    return Phi @ Phi.T, Phi @ V.reshape(-1)


def taps_of(W):
    return int(np.prod(W.shape[1:]))


def kkt(G, c, h):
    """max |pg| / max |c| with g = G h - c, pg = g where h > 0, min(g, 0) where h = 0, over the rows with G_ii > 0."""
    G, c, h = np.asarray(G, dtype=np.float64), np.asarray(c, dtype=np.float64), np.asarray(h, dtype=np.float64)
    cmax = np.max(np.abs(c)) if len(c) else 0.
    if cmax == 0:
        return 0.
    g = G @ h - c
    pg = np.where(h > 0, np.abs(g), np.maximum(-g, 0.))
    return float(np.max(pg[np.diag(G) > 0], initial=0.) / cmax)


def objective(V, G, c, h):
    """E(h) = 1/2 ||V||^2 - c'h + 1/2 h'Gh."""
    h = np.asarray(h, dtype=np.float64)
    return float(0.5 * np.sum(np.asarray(V, dtype=np.float64) ** 2) - c @ h + 0.5 * h @ G @ h)


def densify(K, row_start, col, val):
    """The dense matrix of a CSR triple; asserts columns ascending within a row and the diagonal present."""
    row_start, col, val = (np.asarray(a) for a in (row_start, col, val))
    G = np.zeros((K, K))
    present = np.zeros((K, K), dtype=bool)
    assert row_start[0] == 0 and row_start[-1] == len(col) == len(val)
    for i in range(K):
        cols = col[row_start[i]:row_start[i + 1]]
        assert np.all(np.diff(cols) > 0) and i in cols
        G[i, cols] = val[row_start[i]:row_start[i + 1]]
        present[i, cols] = True
    return G, present


@functools.lru_cache(maxsize=None)
def decoys(seed, mode='valid', noise=1e-3, N=2, C=2, M=3, D=(24, 28), A=(5, 5), n_true=12, n_random=20):
    """A scene with decoys: V = the render of n_true planted events per scene (strengths 1 .. 2, spread over the samples) plus
    noise; the list = the planted rows, their four one-pixel neighbours, the same place under the next atom, and n_random
    random rows, distinct, inside the shift shape, shuffled: K around 90, the Gram matrix far from diagonal.  Every value is
    float32-representable.  -> dict(V, W, mode, sample, plane, shift, strength, true), read-only."""
    rng = np.random.default_rng(1000 + seed)
    S = eref.shift_shape(D, A, mode)
    W = rng.random((M, C) + A) ** 2 + 0.05
    W = (W / W.sum(axis=(2, 3), keepdims=True)).astype(np.float32).astype(np.float64)
    true = []
    while len(true) < n_true:
        r = (int(rng.integers(N)), int(rng.integers(M))) + tuple(int(rng.integers(1, s - 1)) for s in S)
        if r not in true:
            true.append(r)
    rows = list(true)

    def add(r):
        if r not in rows and all(0 <= x < s for x, s in zip(r[2:], S)):
            rows.append(r)
    for n, p, y, x in true:
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            add((n, p, y + dy, x + dx))
        add((n, (p + 1) % M, y, x))
    want = len(rows) + n_random
    while len(rows) < want:
        add((int(rng.integers(N)), int(rng.integers(M))) + tuple(int(rng.integers(s)) for s in S))
    is_true = np.array([True] * n_true + [False] * (len(rows) - n_true))
    order = rng.permutation(len(rows))
    rows, is_true = np.array(rows, dtype=np.int64)[order], is_true[order]
    strength = np.where(is_true, 1. + rng.integers(0, 9, len(rows)) / 8., 0.25).astype(np.float64)
    V = eref.render(W, D, N, mode, rows[is_true, 0], rows[is_true, 1], rows[is_true, 2:], strength[is_true])
    V = (V + noise * rng.random(V.shape)).astype(np.float32).astype(np.float64)
    out = dict(V=V, W=W, mode=mode, sample=rows[:, 0], plane=rows[:, 1], shift=rows[:, 2:], strength=strength, true=is_true)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
