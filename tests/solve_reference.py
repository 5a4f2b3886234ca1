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


# -- the sparse Gram matrix and the solver's iterates (tests/solve_dispatch.py, tests/test_hip_solve_matrix.py) ------------------
def _entries(W, D, N, mode, sample, plane, shift):
    """(row [E], pixel [E], phi [E]): the non-blank pixels of every occurrence -- pixel an index into [N, C, *D] --, the images
    of a row that meet on a pixel added, sorted by (row, pixel).  The images per row are those of events_reference.images;
    the taps are walked one numpy pass per tap over all images."""
    A, C = W.shape[2:], W.shape[1]
    S = eref.shift_shape(D, A, mode)
    sample = np.asarray(sample, dtype=np.int64).reshape(-1)
    plane = np.asarray(plane, dtype=np.int64).reshape(-1)
    shift = np.asarray(shift, dtype=np.int64).reshape(len(sample), len(A))
    table = {}
    for u in set(map(tuple, shift.tolist())):
        table[u] = eref.images(u, A, S, mode)
    e, q = [], []
    for row, u in enumerate(map(tuple, shift.tolist())):
        for at in table[u]:
            e.append(row)
            q.append(at)
    e, q = np.array(e, dtype=np.int64), np.array(q, dtype=np.int64).reshape(len(e), len(A))
    rows, pixels, values = [], [], []
    for c in range(C):
        for j in np.ndindex(*A):
            at = q - (np.array(A) - 1) + np.array(j)
            inside = np.all((at >= 0) & (at < np.array(D)), axis=1)
            flat = sample[e] * C + c
            for axis, d in enumerate(D):
                flat = flat * d + at[:, axis]
            rows.append(e[inside])
            pixels.append(flat[inside])
            values.append(W[(plane[e[inside]], c) + j])
    rows, pixels, values = np.concatenate(rows), np.concatenate(pixels), np.concatenate(values).astype(np.float64)
    size = N * C * int(np.prod(D))
    key = rows * size + pixels
    order = np.argsort(key, kind='stable')
    key, values = key[order], values[order]
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if len(key) else np.zeros(0, dtype=np.int64)
    values = np.add.reduceat(values, first) if len(key) else values
    key = key[first]
    live = values != 0
    return key[live] // size, key[live] % size, values[live]


def gram_sparse(V, W, mode, sample, plane, shift):
    """((row_start [K + 1], col [nnz], val [nnz]), c [K]) in float64: the non-zeros of G_ref plus the whole diagonal, columns
    ascending, and c_ref, without a dense matrix: the occurrences bucketed by pixel, every two rows of a bucket a product."""
    V = np.asarray(V, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    K = len(np.asarray(sample).reshape(-1))
    row, pixel, phi = _entries(W, V.shape[2:], V.shape[0], mode, sample, plane, shift)
    c = np.bincount(row, weights=phi * V.reshape(-1)[pixel], minlength=K)
    order = np.argsort(pixel, kind='stable')
    row, pixel, phi = row[order], pixel[order], phi[order]
    first = np.flatnonzero(np.concatenate([[True], pixel[1:] != pixel[:-1]])) if len(pixel) else np.zeros(0, dtype=np.int64)
    size = np.diff(np.concatenate([first, [len(pixel)]]))
    mine = np.repeat(size, size)                              # per entry: the entries of its bucket ...
    start = np.repeat(first, size)                            # ... and where they begin
    a = np.repeat(np.arange(len(pixel)), mine)
    b = np.repeat(start, mine) + (np.arange(int(mine.sum())) - np.repeat(np.cumsum(mine) - mine, mine))
    key = np.concatenate([row[a] * K + row[b], np.arange(K) * (K + 1)])
    product = np.concatenate([phi[a] * phi[b], np.zeros(K)])
    key, inverse = np.unique(key, return_inverse=True)
    val = np.bincount(inverse.reshape(-1), weights=product, minlength=len(key))
    keep = (val != 0) | (key // K == key % K)
    key, val = key[keep], val[keep]
    row_start = np.searchsorted(key // K, np.arange(K + 1))
    return (row_start.astype(np.int64), (key % K).astype(np.int64), val), c


def csr_entries(K, row_start, col, val):
    """(row, col, val) of the entries tnmf_hip_events_nnls reads: row_start clamped as the header promises (to [0, nnz], a
    run never ending before it begins), columns outside [0, K) skipped."""
    row_start, col, val = np.asarray(row_start, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(val, dtype=np.float64)
    nnz = len(val)
    rows, at = [], []
    for i in range(K):
        a = min(max(int(row_start[i]), 0), nnz)
        b = min(max(int(row_start[i + 1]), a), nnz)
        k = np.arange(a, b)
        k = k[(col[k] >= 0) & (col[k] < K)]
        rows.append(np.full(len(k), i, dtype=np.int64))
        at.append(k)
    rows, at = np.concatenate(rows), np.concatenate(at)
    return rows, col[at], val[at]


def nnls_iterates(G, c, start, n):
    """The iteration of tnmf_hip_events_nnls as include/tnmf_hip.h states it, in float64, step by step: a list of n + 1 tuples
    (x, kkt, restarted, restart sum, sum of the magnitudes of its terms) -- the iterate it, its kkt, and the restart test of
    the step that leaves it.  G: a dense matrix (sums in the order of numpy's product) or a CSR triple (row sums entry by
    entry in storage order; clamped and filtered by csr_entries)."""
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    K = len(c)
    if isinstance(G, tuple):
        row, col, val = csr_entries(K, *G)
        matvec = lambda x: np.bincount(row, weights=val * x[col], minlength=K)
        diag = np.bincount(row[row == col], weights=val[row == col], minlength=K)
        rowabs = np.bincount(row, weights=np.abs(val), minlength=K)
    else:
        G = np.asarray(G, dtype=np.float64)
        matvec = lambda x: G @ x
        diag, rowabs = np.diag(G).copy(), np.abs(G).sum(axis=1)
    L = float(np.max(rowabs))
    cmax = float(np.max(np.abs(c)))
    act = (diag > 0) & (cmax > 0)
    start = np.asarray(start, dtype=np.float64).reshape(-1)
    with np.errstate(invalid='ignore'):
        x = np.where(act & (start > 0), start, 0.)            # (NaN > 0 is false)
    previous, beta, t = x.copy(), 0., 1.
    out = []
    for _ in range(n + 1):
        g = matvec(x) - c
        pg = np.where(x > 0, np.abs(g), np.maximum(-g, 0.))
        kkt = float(np.max(pg[act], initial=0.)) / cmax if cmax > 0 else 0.
        y = x + beta * (x - previous)
        step = (matvec(y) - c) / L if L > 0 else np.zeros(K)
        following = np.where(act, np.maximum(y - step, 0.), 0.)
        terms = np.where(act, (y - following) * (following - x), 0.)
        total = float(np.sum(terms))
        restarted = total > 0
        out.append((x, kkt, restarted, total, float(np.sum(np.abs(terms)))))
        if restarted:
            t, beta = 1., 0.
        else:
            t_next = 0.5 * (1. + np.sqrt(1. + 4. * t * t))
            t, beta = t_next, (t - 1.) / t_next
        previous, x = x, following
    return out
