"""
TEST-ONLY reference of the alternatives of events (include/tnmf_hip.h, tnmf_hip_events_alternatives): on purpose naive, built on
tests/events_reference.py and independent of the front end's host route (events_host.events_alternatives_numpy) -- a dense phi
per candidate plane, summed pixel by pixel into a dense sample.

alternatives() is the definition against a render that is GIVEN, so a device's own R can be scored; it works in extended
precision (np.longdouble) and rounds once at the end, so its own error stays far below that of any double sum it is compared
with.  brute_force() reads g = a^2 / (2 b) literally: the energy of the list without the row minus that of the list with the
row replaced by the candidate plane, both from actual renders.  candidates() spells the index rule out row by row, and
staged() mirrors the rule that picks the kernel's path.
"""
import numpy as np

import events_reference as eref
from events_gain_reference import energy, render
from landscape_reference import LD, axis_whole, dense_phi, in_range

PATCH_MAX = 2048          # alternatives.hip, kPatchMax: the doubles of LDS a wave of the staged path may use
BATCH = 4                 # alternatives.hip, kBatch: the candidate planes of one pass over the taps


def candidates(p, n_alt, stride):
    """(the planes p'_0 .. p'_{n_alt - 1} of a row of plane p, j_own): the progression through p inside its block."""
    block = n_alt * stride
    first = (p // block) * block + p % stride
    planes = [first + j * stride for j in range(n_alt)]
    assert planes.count(p) == 1
    return planes, planes.index(p)


def alternatives(V, R, W, mode, sample, plane, shift, strength, n_alt, stride):
    """(a, b, mag), each [K, n_alt] float64: a = <phi', d_e>, b = <phi', phi'>, mag = the sum over the taps of every image of
    phi' of |w' d_e|, with d_e = V - R + h_e phi_e and phi' the candidate plane at the row's shift.  Zeros for a row out of
    range."""
    D, N, k = V.shape[2:], V.shape[0], V.ndim - 2
    S = eref.shift_shape(D, W.shape[2:], mode)
    K = len(sample)
    shift = np.asarray(shift).reshape(K, k)
    assert W.shape[0] % (n_alt * stride) == 0
    d = np.asarray(V, dtype=LD) - np.asarray(R, dtype=LD)
    out = np.zeros((3, K, n_alt))
    for e in range(K):
        n, p, u = int(sample[e]), int(plane[e]), tuple(int(x) for x in shift[e])
        if not in_range(N, W.shape[0], S, n, p, u):
            continue
        de = d[n] + LD(strength[e]) * dense_phi(W, D, mode, p, u, LD)
        for j, q in enumerate(candidates(p, n_alt, stride)[0]):
            phi = dense_phi(W, D, mode, q, u, LD)
            m = LD(0)
            for at, w in eref.pixels(W, D, mode, 0, q, u):
                m += abs(LD(w) * de[at[1:]])
            out[:, e, j] = float(np.sum(phi * de)), float(np.sum(phi * phi)), float(m)
    return out[0], out[1], out[2]


def gains(a, b):
    live = (a > 0) & (b > 0)
    return np.where(live, a * a / (2. * np.where(live, b, 1.)), 0.)


def brute_force(V, W, mode, sample, plane, shift, strength, a, b, n_alt, stride):
    """[K, n_alt]: E(list without e) - E(list with e replaced by plane p'_j at the same shift, strength max(a, 0) / b), from
    renders in float64; 0 where b is 0."""
    D, N, k = V.shape[2:], V.shape[0], V.ndim - 2
    K = len(sample)
    sample, plane = np.asarray(sample), np.asarray(plane)
    shift, h = np.asarray(shift).reshape(K, k), np.asarray(strength, dtype=np.float64)
    out = np.zeros((K, n_alt))
    for e in range(K):
        rest = np.arange(K) != e
        without = render(W, D, N, mode, sample[rest], plane[rest], shift[rest], h[rest])
        E0 = energy(V, without)
        for j, q in enumerate(candidates(int(plane[e]), n_alt, stride)[0]):
            if not b[e, j] > 0:
                continue
            replaced = without.copy()
            replaced[int(sample[e])] += max(a[e, j], 0.) / b[e, j] * dense_phi(W, D, mode, q, tuple(int(x) for x in shift[e]))
            out[e, j] = E0 - energy(V, replaced)
    return out


def staged(geo, shift):
    """[K] bool: the host mirror of the kernel's path rule (alternatives.hip, alternatives_staged) -- the row's occurrence is
    a single image wholly inside the sample, and the patch of C * prod(A) doubles fits PATCH_MAX."""
    N, C, P, D, A, mode = geo
    S = eref.shift_shape(D, A, mode)
    fits = C * int(np.prod(A)) <= PATCH_MAX
    return np.array([fits and all(axis_whole(int(u), a, s, d, mode) for u, a, s, d in zip(row, A, S, D))
                     for row in np.asarray(shift).reshape(-1, len(A))], dtype=bool)
