"""
References of the triggered sums (include/tnmf_hip.h, "triggered sums") and the one error bar their tests use.

    X[p, f, j] = sum_n sum_q Hp[n, p, q]^power Y[n, f, q - (A - 1) - m + j]        0 <= j_k < A_k + 2 m_k

over the terms whose index of Y lies inside the sample.  The bar is derived, not measured.  With T the same sum with |Y|
in the place of Y and n the (sample, pixel) terms of the entry, any order of double additions of n terms is within
n 2^-53 T of the exact sum; a product adds at most three more roundings (the square, times Y, an unfused add).  So two
evaluations in double -- the kernel's and the float64 reference's -- differ by at most

    4 (n + 2) 2^-53 T        per entry,

with no absolute term: an entry with T == 0 must be an exact 0.
"""
import itertools

import numpy as np

U = 2. ** -53


def window(A, m):
    return tuple(int(a) + 2 * int(x) for a, x in zip(A, m))


def terms(D, A, m, n_samples):
    """The number of (sample, pixel) terms behind each window position: ``[*(A + 2 m)]``.  Along an axis, position j reads
    Y at q - (a - 1) - m + j for 0 <= q < d + a - 1: the overlap of [j - (a - 1) - m, j - m + d) with [0, d)."""
    out = np.asarray(n_samples, dtype=np.float64)
    for k, (d, a, x) in enumerate(zip(D, A, m)):
        lo = np.arange(a + 2 * x) - (a - 1) - x
        n = np.maximum(np.minimum(lo + d + a - 1, d) - np.maximum(lo, 0), 0)
        out = out[..., None] * n.reshape((1,) * k + (-1,))
    return out


def bar(T, D, A, m, n_samples):
    """The largest |X - X_ref| allowed per entry; T the sums with |Y| in the place of Y."""
    return 4. * (terms(D, A, m, n_samples) + 2.) * U * np.asarray(T, dtype=np.float64)


def within_bar(X, X_ref, T, D, A, m, n_samples):
    """-> the largest ratio of an error to its bar (0 where both are 0); asserts nothing."""
    err, b = np.abs(np.asarray(X) - X_ref), bar(T, D, A, m, n_samples)
    b = np.broadcast_to(b, err.shape)
    if np.any(err[b == 0] != 0):
        return np.inf
    return float(np.max(np.divide(err, b, out=np.zeros_like(err), where=b > 0), initial=0.))


def brute(Hp, Y, A, m, power=1, per_sample=False):
    """The definition, one term at a time: loops over the window position and the padded pixel q (vectorised over n, p, f
    only)."""
    Hp, Y = np.asarray(Hp, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    N, P, F = Hp.shape[0], Hp.shape[1], Y.shape[1]
    D, S = Y.shape[2:], Hp.shape[2:]
    assert all(s == d + a - 1 for s, d, a in zip(S, D, A))
    X = np.zeros((N, P, F) + window(A, m))
    for j in itertools.product(*(range(w) for w in window(A, m))):
        for q in np.ndindex(*S):
            y = tuple(qk - (a - 1) - x + jk for qk, a, x, jk in zip(q, A, m, j))
            if all(0 <= yk < d for yk, d in zip(y, D)):
                h = Hp[(slice(None), slice(None)) + q] ** power
                X[(Ellipsis,) + j] += h[:, :, None] * Y[(slice(None), slice(None)) + y][:, None, :]
    return X if per_sample else X.sum(axis=0)


def exact_int64(Hp, Y, A, m, power=1, per_sample=False):
    """The sums of integer-valued operands in int64: every sum exact, whatever the order."""
    Hi, Yi = np.asarray(Hp).astype(np.int64), np.asarray(Y).astype(np.int64)
    assert np.array_equal(Hi, np.asarray(Hp)) and np.array_equal(Yi, np.asarray(Y))
    Hi = Hi ** power
    N, P, F = Hi.shape[0], Hi.shape[1], Yi.shape[1]
    D, S = Yi.shape[2:], Hi.shape[2:]
    X = np.zeros((N, P, F) + window(A, m), dtype=np.int64)
    if N == 0:
        return X if per_sample else X.sum(axis=0)
    for j in itertools.product(*(range(w) for w in window(A, m))):
        off = tuple(jk - (a - 1) - x for jk, a, x in zip(j, A, m))
        lo = tuple(max(0, -o) for o in off)
        hi = tuple(min(s, d - o) for s, d, o in zip(S, D, off))
        if any(h <= l for l, h in zip(lo, hi)):
            continue
        h = Hi[(slice(None), slice(None)) + tuple(slice(l, u) for l, u in zip(lo, hi))].reshape(N, P, -1)
        y = Yi[(slice(None), slice(None)) + tuple(slice(l + o, u + o) for l, u, o in zip(lo, hi, off))].reshape(N, F, -1)
        X[(Ellipsis,) + j] = np.matmul(h, y.transpose(0, 2, 1))
    return X if per_sample else X.sum(axis=0)
