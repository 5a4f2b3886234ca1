"""
TEST-ONLY reference of the landscape of events (include/tnmf_hip.h, tnmf_hip_events_landscape): on purpose naive, built on
tests/events_reference.py and independent of the front end's host fallback (events_host.events_landscape_numpy) -- a dense phi
per neighbour, summed pixel by pixel into a dense sample.

landscape() is the definition against a render that is GIVEN, so a device's own R can be scored; it works in extended precision
(np.longdouble) and rounds once at the end, so its own error stays far below that of any double sum it is compared with.
brute_force() reads g = a^2 / (2 b) literally: the energy of the list without the row minus that of the list with the row
replaced, both from actual renders.  refine() is the parabola of ``refine_detections``.  places() and staged() name the kinds
of rows the tests need and mirror the rule that picks the kernel's path.
"""
import itertools

import numpy as np

import events_reference as eref
from events_gain_reference import energy, render

LD = np.longdouble
PATCH_MAX = 2048          # landscape.hip, kPatchMax: the doubles of LDS a wave of the staged path may use


def deltas(k):
    """The neighbour offsets in the order of the outputs: C order over {-1, 0, 1}^k."""
    return list(itertools.product((-1, 0, 1), repeat=k))


def dense_phi(W, D, mode, p, u, dtype=np.float64):
    """phi [C, *D]: plane p at shift u, every image clipped to the sample, images that overlap added."""
    phi = np.zeros((W.shape[1],) + tuple(D), dtype=dtype)
    for at, w in eref.pixels(W, D, mode, 0, p, u):
        phi[at[1:]] += w
    return phi


def in_range(N, P, S, n, p, u):
    return 0 <= n < N and 0 <= p < P and all(0 <= x < s for x, s in zip(u, S))


def landscape(V, R, W, mode, sample, plane, shift, strength):
    """(a, b, mag), each [K, 3^k] float64: a = <phi', d_e>, b = <phi', phi'>, mag = the sum over the taps of every image of
    phi' of |w d_e|, with d_e = V - R + h_e phi_e.  Zeros for a row out of range and for a neighbour outside the shift shape."""
    D, N, k = V.shape[2:], V.shape[0], V.ndim - 2
    S = eref.shift_shape(D, W.shape[2:], mode)
    K = len(sample)
    shift = np.asarray(shift).reshape(K, k)
    d = np.asarray(V, dtype=LD) - np.asarray(R, dtype=LD)
    out = np.zeros((3, K, 3 ** k))
    for e in range(K):
        n, p, u = int(sample[e]), int(plane[e]), tuple(int(x) for x in shift[e])
        if not in_range(N, W.shape[0], S, n, p, u):
            continue
        de = d[n] + LD(strength[e]) * dense_phi(W, D, mode, p, u, LD)
        for j, delta in enumerate(deltas(k)):
            v = tuple(x + dd for x, dd in zip(u, delta))
            if not in_range(N, W.shape[0], S, n, p, v):
                continue
            phi = dense_phi(W, D, mode, p, v, LD)
            m = LD(0)
            for at, w in eref.pixels(W, D, mode, 0, p, v):
                m += abs(LD(w) * de[at[1:]])
            out[:, e, j] = float(np.sum(phi * de)), float(np.sum(phi * phi)), float(m)
    return out[0], out[1], out[2]


def gains(a, b):
    live = (a > 0) & (b > 0)
    return np.where(live, a * a / (2. * np.where(live, b, 1.)), 0.)


def brute_force(V, W, mode, sample, plane, shift, strength, a, b):
    """[K, 3^k]: E(list without e) - E(list with e replaced by a row at the neighbour of strength max(a, 0) / b), from renders
    in float64; 0 where there is no such neighbour."""
    D, N, k = V.shape[2:], V.shape[0], V.ndim - 2
    S = eref.shift_shape(D, W.shape[2:], mode)
    K = len(sample)
    sample, plane = np.asarray(sample), np.asarray(plane)
    shift, h = np.asarray(shift).reshape(K, k), np.asarray(strength, dtype=np.float64)
    out = np.zeros((K, 3 ** k))
    for e in range(K):
        rest = np.arange(K) != e
        without = render(W, D, N, mode, sample[rest], plane[rest], shift[rest], h[rest])
        E0 = energy(V, without)
        for j, delta in enumerate(deltas(k)):
            v = tuple(int(x) + dd for x, dd in zip(shift[e], delta))
            if not in_range(N, W.shape[0], S, int(sample[e]), int(plane[e]), v) or not b[e, j] > 0:
                continue
            there = max(a[e, j], 0.) / b[e, j] * dense_phi(W, D, mode, int(plane[e]), v)
            replaced = without.copy()
            replaced[int(sample[e])] += there
            out[e, j] = E0 - energy(V, replaced)
    return out


def refine(a, b, k):
    """(offset [K, k], gain [K], is_peak [K]) by the formula of ``refine_detections``, row by row."""
    g = gains(np.asarray(a), np.asarray(b)).reshape((-1,) + (3,) * k)
    K = len(g)
    offset, peak = np.zeros((K, k)), np.ones(K, dtype=bool)
    centre = (1,) * k
    for e in range(K):
        g0 = g[e][centre]
        for i in range(k):
            lo, hi = (g[e][centre[:i] + (j,) + centre[i + 1:]] for j in (0, 2))
            c = lo - 2. * g0 + hi
            if g0 >= max(lo, hi) and c < 0:
                offset[e, i] = min(max(0.5 * (lo - hi) / c, -0.5), 0.5)
            else:
                peak[e] = False
    return offset, g[(slice(None),) + centre].copy(), peak


# -- the kinds of rows -----------------------------------------------------------------------------------------------------------
def axis_whole(u, a, S, D, mode):
    """The shift u on one axis is in range and stands for one image wholly inside the sample."""
    if not 0 <= u < S:
        return False
    q = eref.axis_images(u, a, S, mode)
    return len(q) == 1 and q[0] - (a - 1) >= 0 and q[0] + 1 <= D


def staged(geo, shift):
    """[K] bool: the host mirror of the kernel's path rule (landscape.hip, landscape_staged) -- the row and every neighbour
    are single images wholly inside the sample, and the patch of C * prod(A + 2) doubles fits PATCH_MAX."""
    N, C, P, D, A, mode = geo
    S = eref.shift_shape(D, A, mode)
    fits = C * int(np.prod([a + 2 for a in A])) <= PATCH_MAX
    return np.array([fits and all(axis_whole(int(u) + dd, a, s, d, mode) for u, a, s, d in zip(row, A, S, D)
                                  for dd in (-1, 0, 1)) for row in np.asarray(shift).reshape(-1, len(A))], dtype=bool)


def places(D, A, mode):
    """name -> shift: the places a landscape has to be right at.  'interior' and 'near' (the occurrence one pixel from the
    border of the sample on every axis) have all their neighbours whole; 'edge' is the same atom ON the border; the corners
    and rims of the shift shape have neighbours out of range; the zones are the overlapping images of 'reflect' and the
    wrapped ones of 'circular'."""
    S = eref.shift_shape(D, A, mode)
    k = len(D)
    first = [a - 1 if mode == 'valid' else 0 for a in A]        # the shift whose occurrence starts at pixel 0
    out = {'interior': tuple(f + (d - a) // 2 for f, d, a in zip(first, D, A)),
           'near': tuple(f + 1 for f in first), 'edge': tuple(first),
           'far': tuple(f + d - a - 1 for f, d, a in zip(first, D, A))}
    for i, corner in enumerate(itertools.product(*[(0, s - 1) for s in S])):
        out[f'corner{i}'] = corner
    for i in range(k):
        for name, x in (('rim-lo', 0), ('rim-hi', S[i] - 1)):
            out[f'{name}{i}'] = tuple(x if j == i else S[j] // 2 for j in range(k))
    if mode == 'reflect':
        for u in range(1, max(A)):
            out[f'mirror{u}'] = tuple(min(u, a - 1) if a > 1 else S[j] // 2 for j, a in enumerate(A))
        out['mirror-one-axis'] = tuple(1 if j == k - 1 and A[j] > 1 else S[j] // 2 for j in range(k))
        out['beside-mirror'] = tuple(A)                         # u - 1 = a - 1 is mirrored, u is not
    if mode == 'circular':
        for u in range(1, max(A)):
            out[f'wrap{u}'] = tuple(s - min(u, a - 1) if a > 1 else s // 2 for s, a in zip(S, A))
        out['wrap-one-axis'] = tuple(S[j] - 1 if j == k - 1 and A[j] > 1 else S[j] // 2 for j in range(k))
        out['beside-wrap'] = tuple(s - a for s, a in zip(S, A))  # u + 1 = S - (a - 1) wraps, u does not
    for name, u in out.items():
        assert all(0 <= x < s for x, s in zip(u, S)), (name, u, S)
    return out
