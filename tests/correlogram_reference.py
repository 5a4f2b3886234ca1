"""
References of the activation correlogram (include/tnmf_hip.h, "activation correlogram") and the one error bar its tests use.

    C[n, p, q, D] = sum_u H[n, p, u] H[n, q, u + D]        over the u with u and u + D inside the plane

The bar is derived, not measured.  All terms are non-negative; any order of double additions of n terms is within
n 2^-53 of the exact sum, relatively; each product adds at most one more rounding (float64 H; for float32 H none).  So two
evaluations in double -- the kernel's and the float64 reference's -- differ by at most

    4 n 2^-53 C        per entry, n = the (sample, pixel) terms of that entry,

with no absolute term: an entry whose reference is 0 must be an exact 0.
"""
import itertools

import numpy as np

U = 2. ** -53


def terms(S, L, n_samples):
    """The number of (sample, pixel) terms behind the entry of each lag: ``[*(2 L + 1)]``."""
    per_axis = [np.maximum(s - np.abs(np.arange(-x, x + 1)), 0) for s, x in zip(S, L)]
    out = np.asarray(n_samples, dtype=np.float64)
    for k, a in enumerate(per_axis):
        out = out[..., None] * a.reshape((1,) * k + (-1,))
    return out


def bar(C_ref, S, L, n_samples):
    """The largest |C - C_ref| allowed per entry of a correlogram over ``n_samples`` samples of shift shape S."""
    return 4. * terms(S, L, n_samples) * U * np.asarray(C_ref, dtype=np.float64)


def within_bar(C, C_ref, S, L, n_samples):
    """-> the largest ratio of an error to its bar (0 where both are 0); asserts nothing."""
    err, b = np.abs(np.asarray(C) - C_ref), bar(C_ref, S, L, n_samples)
    if np.any(err[b == 0] != 0):
        return np.inf
    return float(np.max(np.divide(err, b, out=np.zeros_like(err), where=b > 0), initial=0.))


def brute(H, L, per_sample=False):
    """The definition, one term at a time: loops over the lag and over the pixel u (vectorised over n, p, q only)."""
    H = np.asarray(H, dtype=np.float64)
    N, P = H.shape[:2]
    S = H.shape[2:]
    C = np.zeros((N, P, P) + tuple(2 * x + 1 for x in L))
    for lag in itertools.product(*(range(-x, x + 1) for x in L)):
        at = (Ellipsis,) + tuple(d + x for d, x in zip(lag, L))
        for u in np.ndindex(*S):
            v = tuple(a + d for a, d in zip(u, lag))
            if all(0 <= b < s for b, s in zip(v, S)):
                hp = H[(slice(None), slice(None)) + u]
                hq = H[(slice(None), slice(None)) + v]
                C[at] += hp[:, :, None] * hq[:, None, :]
    return C if per_sample else C.sum(axis=0)


def exact_int64(H, L, per_sample=False):
    """The correlogram of integer-valued H in int64: every sum exact, whatever the order."""
    Hi = np.asarray(H).astype(np.int64)
    assert np.array_equal(Hi, np.asarray(H))
    N, P = Hi.shape[:2]
    S = Hi.shape[2:]
    C = np.zeros((N, P, P) + tuple(2 * x + 1 for x in L), dtype=np.int64)
    flat = lambda a: a.reshape(N, P, -1)   # noqa: E731
    for lag in itertools.product(*(range(-min(x, s - 1), min(x, s - 1) + 1) for x, s in zip(L, S))):
        a = Hi[(slice(None), slice(None)) + tuple(slice(max(0, -d), s - max(0, d)) for d, s in zip(lag, S))]
        b = Hi[(slice(None), slice(None)) + tuple(slice(max(0, d), s - max(0, -d)) for d, s in zip(lag, S))]
        C[(Ellipsis,) + tuple(d + x for d, x in zip(lag, L))] = np.matmul(flat(a), flat(b).transpose(0, 2, 1))
    return C if per_sample else C.sum(axis=0)
