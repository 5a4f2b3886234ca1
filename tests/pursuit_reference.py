"""
TEST-ONLY reference of the forward selection of events (include/tnmf_hip.h, "pursuit"; TransformInvariantNMF.pursue_detections):
float64, on purpose naive, built on tests/events_reference.py (the pixels of an occurrence), tests/peaks_reference.py (the
peaks of the gain map) and the front end's ``event_boxes`` -- independent of the front end's driver and of its host fallback
(pursuit_numpy, which correlates in the padded frame and folds).

Every possible row (p, u) is tabulated once as the pixels it touches and phi on them (images that overlap added); a and b
are then sums over that table, row by row.
"""
import numpy as np

import events_reference as eref
import peaks_reference as pref
from tnmf_amd.TransformInvariantNMF import event_boxes


class Table:
    """Per plane and shift of (W, D, mode): the flat pixels in [C, *D] the occurrence touches and phi there."""

    def __init__(self, W, D, mode):
        self.W, self.D, self.mode = np.asarray(W, dtype=np.float64), tuple(D), mode
        self.S = eref.shift_shape(D, W.shape[2:], mode)
        self.P = W.shape[0]
        self.rows = {}
        frame = (W.shape[1],) + self.D
        for p in range(self.P):
            for u in np.ndindex(*self.S):
                phi = {}
                for at, w in eref.pixels(self.W, self.D, mode, 0, p, u):
                    phi[at[1:]] = phi.get(at[1:], 0.) + w
                px = np.array([np.ravel_multi_index(at, frame) for at in phi], dtype=np.int64)
                self.rows[(p,) + u] = (px, np.array(list(phi.values()), dtype=np.float64))

    def norms(self):
        """b [P, *S]: ||phi||^2."""
        b = np.zeros((self.P,) + self.S)
        for key, (_, phi) in self.rows.items():
            b[key] = np.sum(phi * phi)
        return b

    def correlate(self, d):
        """a [N, P, *S]: <phi, d[n]>."""
        a = np.zeros((len(d), self.P) + self.S)
        flat = d.reshape(len(d), -1)
        for key, (px, phi) in self.rows.items():
            a[(slice(None),) + key] = flat[:, px] @ phi
        return a


def exact(V, R, W, mode, rows):
    """(a [K], b [K], mag [K]) of the rows (sample, plane, shift) against a GIVEN render R: a = sum w * (V - R)(px) and
    b = sum w * phi(px) over every tap of every image inside the sample, mag = sum |w * (V - R)(px)|."""
    d = np.asarray(V, dtype=np.float64) - np.asarray(R, dtype=np.float64)
    out = np.zeros((3, len(rows)))
    for e, r in enumerate(np.asarray(rows)):
        taps = list(eref.pixels(W, V.shape[2:], mode, r[0], r[1], r[2:]))
        phi = {}
        for at, w in taps:
            phi[at] = phi.get(at, 0.) + w
        for at, w in taps:
            out[0, e] += w * d[at]
            out[1, e] += w * phi[at]
            out[2, e] += abs(w * d[at])
    return out


def gain_map(a, b):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where((a > 0) & (b > 0), a * a / (2. * b), 0.)


def energy(V, W, mode, rows, strength):
    rows = np.asarray(rows, dtype=np.int64).reshape(len(strength), -1)
    R = np.zeros(V.shape) if not len(rows) else eref.render(W, V.shape[2:], len(V), mode, rows[:, 0], rows[:, 1], rows[:, 2:],
                                                            strength)
    return 0.5 * float(np.sum((np.asarray(V, dtype=np.float64) - R) ** 2))


def meet(lo, hi, i, j):
    return bool(np.all(np.maximum(lo[i], lo[j]) < np.minimum(hi[i], hi[j])))


def pursue(V, W, mode, min_gain, max_events=None, max_rounds=100, refit_iterations=0, start=None, table=None, eps=1e-9):
    """-> dict(rows [K, 2 + k] (sample, plane, shift), strength [K], history [rounds, 3], added: per round the rows it added,
    energies: the energy of the list after every round (refit included)).  ``start``: (rows, strength)."""
    V = np.asarray(V, dtype=np.float64)
    A, D, N = W.shape[2:], V.shape[2:], len(V)
    k = len(D)
    table = table or Table(W, D, mode)
    b = table.norms()
    rows = np.zeros((0, 2 + k), dtype=np.int64) if start is None else np.array(start[0], dtype=np.int64).reshape(-1, 2 + k)
    h = np.zeros(0) if start is None else np.array(start[1], dtype=np.float64)
    history, added, energies = [], [], []
    for _ in range(max_rounds):
        if max_events is not None and len(rows) >= max_events:
            break
        R = np.zeros(V.shape) if not len(rows) else eref.render(W, D, N, mode, rows[:, 0], rows[:, 1], rows[:, 2:], h)
        a = table.correlate(V - R)
        g = gain_map(a, b)
        g[tuple(rows.T)] = 0.
        idx, val = pref.find_peaks(g, min_gain, tuple(x - 1 for x in A), table.P)
        at = np.stack(np.unravel_index(idx, g.shape), axis=1).reshape(len(idx), 2 + k)
        lo, hi = event_boxes(at[:, 2:], A, D, table.S, mode)
        kept = []
        for e in sorted(range(len(idx)), key=lambda i: (-val[i], idx[i])):
            if not any(at[e, 0] == at[j, 0] and meet(lo, hi, e, j) for j in kept):
                kept.append(e)
        kept = sorted(kept)
        kept = [e for e in kept if float(g[tuple(at[e])]) > min_gain]     # (float64: the map IS the exact score)
        if max_events is not None and len(kept) > max_events - len(rows):
            kept = sorted(sorted(kept, key=lambda e: (-g[tuple(at[e])], idx[e]))[:max_events - len(rows)])
        history.append((len(idx), len(kept), float(sum(g[tuple(at[e])] for e in kept))))
        if not kept:
            break
        new = at[kept]
        rows = np.concatenate([rows, new])
        h = np.concatenate([h, [a[tuple(r)] / b[tuple(r[1:])] for r in new]])
        added.append(new)
        if refit_iterations:
            h = eref.refit(V, W, mode, rows[:, 0], rows[:, 1], rows[:, 2:], h, refit_iterations, eps=eps)
        energies.append(energy(V, W, mode, rows, h))
    return dict(rows=rows, strength=h, history=np.array(history, dtype=np.float64).reshape(len(history), 3), added=added,
                energies=energies)


def separated(seed, mode, N=2, M=2, C=2, D=(24, 26), A=(4, 4), n_events=5):
    """A scene whose answer is known: per sample ``n_events`` events of strengths 1 + k / 8 whose boxes (event_boxes) leave,
    pair by pair, a gap >= A - 1 on some axis -- no candidate footprint meets two true ones -- and V their render, rounded to
    float32, without noise.  The shifts are drawn by rejection; in 'circular' and 'reflect' two per sample from the zones
    where an event stands for several images.  -> dict(V, W, mode, rows [K, 4], strength [K]), read-only."""
    rng = np.random.default_rng(seed)
    S = eref.shift_shape(D, A, mode)
    W = rng.random((M, C) + A) * (rng.random((M, C) + A) < 0.5) + 0.05
    W = (W / W.sum(axis=(2, 3), keepdims=True)).astype(np.float32).astype(np.float64)
    rows = []
    for n in range(N):
        mine = []
        while len(mine) < n_events:
            u = tuple(int(rng.integers(s)) for s in S)
            if mode in ('circular', 'reflect') and len(mine) < (2 if mode == 'reflect' else 1):
                # 'reflect': each sample's first event lies in the mirror zone of both axes (4 images), its second in that of
                # the last axis (2); 'circular': the first in the wrap zone of the last axis (2 images: a band as wide as the
                # sample) -- one that wraps on both axes has the whole sample for its box, which no other event can keep
                # a gap to
                zone = tuple(int(rng.integers(s - (a - 1), s)) if mode == 'circular' else int(rng.integers(1, a))
                             for s, a in zip(S, A))
                u = zone if mode == 'reflect' and not mine else u[:-1] + zone[-1:]
            if mode == 'circular' and all(x >= s - (a - 1) for x, s, a in zip(u, S, A)):
                continue
            lo, hi = event_boxes(np.array([u] + [m[1:] for m in mine]), A, D, S, mode)
            if np.any(hi[0] <= lo[0]):
                continue
            # (a gap of g pixels between two boxes on an axis: lo_b - hi_a >= g)
            if all(np.any(np.maximum(lo[0] - hi[j], lo[j] - hi[0]) >= np.asarray(A) - 1) for j in range(1, len(lo))):
                mine.append((int(rng.integers(M)),) + u)
        rows += [(n,) + m for m in mine]
    rows = np.array(rows, dtype=np.int64)
    strength = 1. + (np.arange(len(rows)) % n_events) / 8.
    V = eref.render(W, D, N, mode, rows[:, 0], rows[:, 1], rows[:, 2:], strength).astype(np.float32).astype(np.float64)
    out = dict(V=V, W=W, mode=mode, rows=rows, strength=strength)
    for x in out.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out
