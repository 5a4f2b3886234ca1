"""
TEST-ONLY reference of the standard errors of a list (include/tnmf_hip.h, "events: standard errors"): the dense Gram matrix of
tests/solve_reference.py, numpy.linalg.inv of its active block in float64 and the components of that block by a plain
breadth-first search.  Independent of tnmf_amd/events_host.py (union-find, a factorisation per component) and of the device
(min-label hooking, Cholesky per component).

The bar of d = diag (G_AA)^-1, per component of n rows with kappa = cond_2 of the reference block and taps the products of a
Gram entry:  |d - d_ref| <= kappa * (8 * taps + 4 * n^2) * 2^-52 * d_ref.  The first term is the Gram entries' own bar
(tests/test_hip_events_solve.py) carried through the inverse -- a relative perturbation e of the matrix moves the inverse by
kappa * e to first order --, the second a generous form of the backward errors of the Cholesky factorisation and the two
triangular solves, (n + 1) and n units each per entry.
"""
import functools

import numpy as np

import events_reference as eref
import solve_reference as sr

N_LDS = 200                                                   # include/tnmf_hip.h, TNMF_EVENTS_INVERSE_LDS
CHAIN_SIZES = (1, 2, 3, 63, 64, 65, N_LDS - 1, N_LDS, N_LDS + 1, 300)


def components(G, active):
    """The connected components of the graph of G restricted to the active rows, by breadth-first search: a list of ascending
    row arrays, in ascending size, equal sizes by their smallest row."""
    active = np.asarray(active, dtype=bool)
    K = len(active)
    seen = ~active
    out = []
    for start in range(K):
        if seen[start]:
            continue
        seen[start] = True
        queue, found = [start], []
        while queue:
            i = queue.pop()
            found.append(i)
            for j in np.flatnonzero((G[i] != 0) & ~seen):
                seen[j] = True
                queue.append(int(j))
        out.append(np.array(sorted(found), dtype=np.int64))
    out.sort(key=lambda g: (len(g), g[0]))
    return out


def inverse_diag(G, active, taps):
    """-> dict(d [K] (NaN off the active rows), bar [K] (the bar of the module docstring, relative: |d - d_ref| <= bar * d_ref),
    kappa [K], size [K] (0 off the active rows), groups).  The inverse is that of the WHOLE active block: it is block diagonal
    because the matrix is, not because this function says so."""
    active = np.asarray(active, dtype=bool)
    K = len(active)
    rows = np.flatnonzero(active)
    d, bar, kappa, size = np.full(K, np.nan), np.full(K, np.nan), np.full(K, np.nan), np.zeros(K, dtype=np.int64)
    if len(rows):
        d[rows] = np.diag(np.linalg.inv(G[np.ix_(rows, rows)]))
    groups = components(G, active)
    for g in groups:
        n = len(g)
        kappa[g] = np.linalg.cond(G[np.ix_(g, g)])
        size[g] = n
        bar[g] = kappa[g] * (8 * taps + 4 * n * n) * 2. ** -52
    return dict(d=d, bar=bar, kappa=kappa, size=size, groups=groups)


@functools.lru_cache(maxsize=None)
def chain():
    """The sizes at which the kernel takes another path, from a 1-D chain: one sample, atoms of 7 taps, 'valid'.  Events 3
    cells apart overlap their two neighbours on either side (lags 3 and 6) and form a banded component of any chosen length;
    the next component starts 10 cells after the last row, beyond the reach of 7.  In every gap sits a row of strength 0 that
    touches BOTH its neighbours (5 cells from either): a row that is not active must not join them.  Components of
    CHAIN_SIZES rows; rows in a random order; two planes at random.  -> dict(V, W, mode, sample, plane, shift, strength,
    G, c, ref), read-only; ref = inverse_diag of the active rows."""
    rng = np.random.default_rng(4711)
    A, P = (7,), 2
    W = rng.random((P, 1) + A) ** 2 + 0.05
    W = (W / W.sum(axis=2, keepdims=True)).astype(np.float32).astype(np.float64)
    shifts, active, at = [], [], 0
    for n in CHAIN_SIZES:
        if shifts:
            shifts.append(at - 5)            # the bridge: 5 from the last row of the component before, 5 from the next
            active.append(False)
        shifts += [at + 3 * i for i in range(n)]
        active += [True] * n
        at += 3 * (n - 1) + 10
    S = at
    D = (S + A[0] - 1,)
    K = len(shifts)
    order = rng.permutation(K)
    shift = np.array(shifts, dtype=np.int64)[order].reshape(K, 1)
    active = np.array(active)[order]
    plane = rng.integers(0, P, K)
    sample = np.zeros(K, dtype=np.int64)
    strength = np.where(active, 1. + rng.integers(0, 9, K) / 8., 0.)
    V = eref.render(W, D, 1, 'valid', sample, plane, shift, strength)
    V = (V + 1e-3 * rng.random(V.shape)).astype(np.float32).astype(np.float64)
    G, c = sr.gram(V, W, 'valid', sample, plane, shift)
    out = dict(V=V, W=W, mode='valid', sample=sample, plane=plane, shift=shift, strength=strength, G=G, c=c,
               ref=inverse_diag(G, active, sr.taps_of(W)))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def symmetric_atoms(M=2, C=1, a=4, seed=3):
    """W [M, C, a, a]: atom 0 invariant under rotations by 90 degrees (its four orientations are the same array), the others
    not."""
    rng = np.random.default_rng(seed)
    W = rng.integers(1, 9, (M, C, a, a)) / 8.                 # (eighths: the sum of four rotations is exact)
    W[0] = sum(np.rot90(W[0], k, axes=(1, 2)) for k in range(4)) / 4.
    assert all(np.array_equal(W[0], np.rot90(W[0], k, axes=(1, 2))) for k in range(4))
    return W


def chi_square_interval(dof, tail):
    """(lo, hi) with P(chi2_dof < lo) = P(chi2_dof > hi) = tail / 2, by bisection on the regularised incomplete gamma
    function (the series of the lower one; dof / 2 an integer or half-integer of moderate size)."""
    import math

    def cdf(x):
        s, k = dof / 2., x / 2.
        term = total = 1. / s
        for i in range(1, 2000):
            term *= k / (s + i)
            total += term
            if term < 1e-17 * total:
                break
        return total * math.exp(-k + s * math.log(k) - math.lgamma(s))

    def quantile(q):
        lo, hi = 1e-9, 10. * dof + 100.
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if cdf(mid) < q else (lo, mid)
        return 0.5 * (lo + hi)
    return quantile(tail / 2.), quantile(1. - tail / 2.)
