"""
TEST-ONLY reference of the gains of events (include/tnmf_hip.h, tnmf_hip_events_gain): float64, on purpose naive, built on
tests/events_reference.py and independent of the front end's host fallback (events_gain_numpy, which sums the images into a
dense sample).

leave_one_out() is the definition read literally: render the list with and without the row, subtract the energies.
closed_form() is the formula, tap by tap, against a render that is GIVEN -- so a device's own R can be scored bit for bit --
with the sum of the magnitudes of its terms.
"""
import numpy as np

import events_reference as eref


def energy(V, R):
    return 0.5 * float(np.sum((np.asarray(V, dtype=np.float64) - R) ** 2))


def render(W, D, N, mode, sample, plane, shift, strength):
    """events_reference.render, which does not take an empty list."""
    if len(sample) == 0:
        return np.zeros((N, W.shape[1]) + tuple(D))
    return eref.render(W, D, N, mode, sample, plane, shift, strength)


def leave_one_out(V, W, mode, sample, plane, shift, strength):
    """(gain [K], E): E(list without e) - E(list) per row, and E(list)."""
    D, N = V.shape[2:], V.shape[0]
    K = len(sample)
    shift = np.asarray(shift).reshape(K, -1)
    h = np.asarray(strength, dtype=np.float64)
    E = energy(V, render(W, D, N, mode, sample, plane, shift, h))
    gain = np.empty(K)
    for e in range(K):
        rest = np.arange(K) != e
        gain[e] = energy(V, render(W, D, N, mode, sample[rest], plane[rest], shift[rest], h[rest])) - E
    return gain, E


def closed_form(V, R, W, mode, sample, plane, shift, strength):
    """(gain [K], mag [K]): h a + h^2 b / 2 with a = sum w * (V - R)(px), b = sum w * phi(px) over every tap of every image
    that lies in the sample, phi(px) the sum of the taps of all images of the row on that pixel; mag the sum of the
    magnitudes of the terms.  A row whose sample, plane or shift is out of range gets 0 in both."""
    V, R = np.asarray(V, dtype=np.float64), np.asarray(R, dtype=np.float64)
    D, N = V.shape[2:], V.shape[0]
    S = eref.shift_shape(D, W.shape[2:], mode)
    K = len(sample)
    d = V - R
    gain, mag = np.zeros(K), np.zeros(K)
    for e, (n, p, u, h) in enumerate(zip(sample, plane, np.asarray(shift).reshape(K, -1), strength)):
        if not (0 <= n < N and 0 <= p < W.shape[0] and all(0 <= x < s for x, s in zip(u, S))):
            continue
        h = float(h)
        taps = list(eref.pixels(W, D, mode, n, p, u))
        phi = {}
        for at, w in taps:
            phi[at] = phi.get(at, 0.) + w
        a = b = m = 0.
        for at, w in taps:
            a += w * d[at]
            b += w * phi[at]
            m += h * abs(w * d[at]) + 0.5 * h * h * abs(w * phi[at])
        gain[e], mag[e] = h * a + 0.5 * h * h * b, m
    return gain, mag


def planted(seed, mode='valid', N=2, M=2, D=(24, 26), A=(4, 4), n_true=6, n_spurious=6):
    """A pruning problem whose answer is known: V = the render of a TRUE list (strengths 1 .. 2) of a dictionary W plus a
    little noise, and the list to prune = the true rows and SPURIOUS ones of strength 0.05 elsewhere -- for each sample a
    few alone and one pair on neighbouring shifts, whose footprints overlap -- shuffled.  Every value is
    float32-representable, so both element types work on the same numbers.
    -> dict(V, W, mode, sample, plane, shift, strength, true [K] bool), read-only."""
    rng = np.random.default_rng(seed)
    S = eref.shift_shape(D, A, mode)
    W = rng.random((M, 1) + A) + 0.1
    W = (W / W.sum(axis=(2, 3), keepdims=True)).astype(np.float32).astype(np.float64)
    rows, true = [], []
    for n in range(N):
        drawn = []   # distinct; the first n_true are the true ones
        while len(drawn) < n_true + n_spurious:
            r = (int(rng.integers(M)),) + tuple(int(rng.integers(1, s - 1)) for s in S)
            if r not in drawn and r[:-1] + (r[-1] + 1,) not in drawn:
                drawn.append(r)
        drawn.append(drawn[-1][:-1] + (drawn[-1][-1] + 1,))   # the neighbour of the last spurious row
        rows += [(n,) + r for r in drawn]
        true += [True] * n_true + [False] * (n_spurious + 1)
    order = rng.permutation(len(rows))
    rows, true = np.array(rows, dtype=np.int64)[order], np.array(true)[order]
    strength = np.where(true, 1. + rng.integers(0, 9, len(rows)) / 8., 0.05).astype(np.float32).astype(np.float64)
    V = eref.render(W, D, N, mode, rows[true, 0], rows[true, 1], rows[true, 2:], strength[true])
    V = (V + 0.01 * rng.random(V.shape)).astype(np.float32).astype(np.float64)
    out = dict(V=V, W=W, mode=mode, sample=rows[:, 0], plane=rows[:, 1], shift=rows[:, 2:], strength=strength, true=true)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
