"""
An independent restatement of include/tnmf_hip.h, "patches", written from the definitions and from nothing else in the
package: the images of an event, the three signals, the patch of an event with the scale of its rounding error, the fold of a
patch by a table, the moments of a list and the modes of the moments.  Everything is evaluated per pixel in extended
precision (``np.longdouble``: 64 bits of mantissa where the platform has them), so next to the float64 of the code under
test the reference's own rounding is 2^-11 of a unit roundoff and the bounds below are bounds on the code alone.
"""
import itertools

import numpy as np

LD = np.longdouble
U = 2. ** -53                       # the unit roundoff of the doubles under test
SOURCES = ('data', 'residual', 'cleaned')
# roundings of the definition per element of x, each at most U * (the sum of the magnitudes of the terms): the additions of
# the images (at most 4 images: 3; the first is added to an exact zero), the subtraction V - R, the fma of h * phi, and the
# additions inside phi (at most 4)
ROUNDINGS = {'data': 3, 'residual': 3 + 1, 'cleaned': 3 + 1 + 1 + 4}


def shift_shape(D, A, mode):
    return tuple({'valid': d + a - 1, 'full': d - a + 1}.get(mode, d) for d, a in zip(D, A))


def axis_images(u, a, s, mode):
    """The padded positions of shift u on one axis: the table of the header."""
    if mode == 'valid':
        return [u]
    q = [u + a - 1]
    if mode == 'circular' and u >= s - (a - 1):
        q.append(u - (s - (a - 1)))
    if mode == 'reflect' and 1 <= u <= a - 1:
        q.append((a - 1) - u)
    return q


def images(u, A, S, mode):
    """The images of the shift ``u``: the Cartesian product of the axes' positions, the first axis slowest."""
    return list(itertools.product(*[axis_images(int(x), a, s, mode) for x, a, s in zip(u, A, S)]))


def in_range(rows, N, P, S):
    rows = np.asarray(rows)
    return ((rows[:, 0] >= 0) & (rows[:, 0] < N) & (rows[:, 1] >= 0) & (rows[:, 1] < P)
            & np.all((rows[:, 2:] >= 0) & (rows[:, 2:] < np.array(S)), axis=1))


def render(W, D, N, mode, rows, h):
    """R[N, C, *D] of the rows in range, in extended precision."""
    A = W.shape[2:]
    S = shift_shape(D, A, mode)
    R = np.zeros((N, W.shape[1]) + tuple(D), dtype=LD)
    for row, hv in zip(np.asarray(rows)[in_range(rows, N, W.shape[0], S)], np.asarray(h)[in_range(rows, N, W.shape[0], S)]):
        for q in images(row[2:], A, S, mode):
            for j in np.ndindex(*A):
                px = tuple(qi - (a - 1) + ji for qi, a, ji in zip(q, A, j))
                if all(0 <= x < d for x, d in zip(px, D)):
                    R[(int(row[0]), slice(None)) + px] += LD(hv) * W[(int(row[1]), slice(None)) + j].astype(LD)
    return R


def patches(V, R, W, mode, rows, h, source):
    """(x [K, C, *A], mag [K, C, *A], n_images [K]) in extended precision: the patch of every row by the definition, and the
    sum of the magnitudes of the terms of each element -- |V| (+ |R| (+ h * sum |w| of phi)) over the images.  Zeros for a row
    out of range."""
    assert source in SOURCES
    N, C, D = V.shape[0], V.shape[1], V.shape[2:]
    A = W.shape[2:]
    S = shift_shape(D, A, mode)
    rows = np.asarray(rows)
    ok = in_range(rows, N, W.shape[0], S)
    x, mag = np.zeros((len(rows), C) + tuple(A), dtype=LD), np.zeros((len(rows), C) + tuple(A), dtype=LD)
    count = np.zeros(len(rows), dtype=np.int64)
    for e, row in enumerate(rows):
        if not ok[e]:
            continue
        n, p = int(row[0]), int(row[1])
        qs = images(row[2:], A, S, mode)
        count[e] = len(qs)
        phi, aphi = np.zeros((C,) + tuple(D), dtype=LD), np.zeros((C,) + tuple(D), dtype=LD)
        if source == 'cleaned':
            for q in qs:
                for j in np.ndindex(*A):
                    px = tuple(qi - (a - 1) + ji for qi, a, ji in zip(q, A, j))
                    if all(0 <= t < d for t, d in zip(px, D)):
                        phi[(slice(None),) + px] += W[(p, slice(None)) + j].astype(LD)
                        aphi[(slice(None),) + px] += np.abs(W[(p, slice(None)) + j]).astype(LD)
        s, a = V[n].astype(LD), np.abs(V[n]).astype(LD)
        if source != 'data':
            s, a = s - R[n].astype(LD), a + np.abs(R[n]).astype(LD)
        if source == 'cleaned':
            s, a = s + LD(h[e]) * phi, a + LD(abs(h[e])) * aphi
        for q in qs:
            for j in np.ndindex(*A):
                px = tuple(qi - (a_ - 1) + ji for qi, a_, ji in zip(q, A, j))
                if all(0 <= t < d for t, d in zip(px, D)):
                    x[(e, slice(None)) + j] += s[(slice(None),) + px]
                    mag[(e, slice(None)) + j] += a[(slice(None),) + px]
    return x, mag, count


def fold(x, bound, planes, table):
    """(y, bound of y): ``y[e, c, i] = sum_k w_k x[e, c, src_k]`` over row ``(planes[e] % T, i)`` of the table, in extended
    precision, and what the rounding of the device may add to ``bound`` (that of x): ``sum |w_k| bound[src_k]`` plus, for a
    row with more than one entry or a weight other than 1, ``(entries + 1) U sum |w_k x_k|``."""
    ptr, src, w, T = table
    if ptr is None:
        return x, bound
    K, C = x.shape[:2]
    nA = int(np.prod(x.shape[2:]))
    xf, bf = x.reshape(K, C, nA), bound.reshape(K, C, nA)
    y, by = np.zeros_like(xf), np.zeros_like(bf)
    t_of = np.where(np.asarray(planes) >= 0, np.asarray(planes) % T, 0)   # (a row out of range is all zeros: any t)
    for t in range(T):
        rows = np.flatnonzero(t_of == t)
        for i in range(nA):
            ks = range(int(ptr[t * nA + i]), int(ptr[t * nA + i + 1]))
            mags = np.zeros((len(rows), C), dtype=LD)
            for k in ks:
                y[rows, :, i] += LD(w[k]) * xf[rows, :, src[k]]
                mags += LD(w[k]) * np.abs(xf[rows, :, src[k]])
                by[rows, :, i] += LD(w[k]) * bf[rows, :, src[k]]
            if not (len(ks) == 1 and w[ks[0]] == 1.):
                by[rows, :, i] += (len(ks) + 1) * U * mags
    return y.reshape(x.shape), by.reshape(x.shape)


def table_from_dense(L):
    """The fold table of dense operators ``L[T, nA(out), nA(in)]``: row (t, i) lists the out pixels o with L[t, o, i] != 0 in
    ascending order."""
    T, nA, _ = L.shape
    ptr, src, w = [0], [], []
    for t in range(T):
        for i in range(nA):
            for o in np.flatnonzero(L[t, :, i]):
                src.append(int(o))
                w.append(float(L[t, o, i]))
            ptr.append(len(src))
    return np.array(ptr, dtype=np.int32), np.array(src, dtype=np.int32), np.array(w, dtype=np.float64), T


def moments(Y, h, atom, n_atoms):
    """(S, g, s2, count) and the magnitudes (sum |y_i y_j|, sum |h y_i|) per atom, in extended precision."""
    Y, h = np.asarray(Y, dtype=LD).reshape(len(Y), -1), np.asarray(h, dtype=LD)
    D = Y.shape[1]
    S, Sm = np.zeros((n_atoms, D, D), dtype=LD), np.zeros((n_atoms, D, D), dtype=LD)
    g, gm = np.zeros((n_atoms, D), dtype=LD), np.zeros((n_atoms, D), dtype=LD)
    s2, count = np.zeros(n_atoms, dtype=LD), np.zeros(n_atoms)
    for e in range(len(Y)):
        m = int(atom[e])
        if not 0 <= m < n_atoms:
            continue
        S[m] += np.outer(Y[e], Y[e])
        Sm[m] += np.abs(np.outer(Y[e], Y[e]))
        g[m] += h[e] * Y[e]
        gm[m] += np.abs(h[e] * Y[e])
        s2[m] += h[e] * h[e]
        count[m] += 1
    return S, g, s2, count, Sm, gm


def modes(S, g, s2, count, n_modes):
    """(mean, modes, variance, total) by the definition of the issue, in float64 (eigh has no extended precision)."""
    S, g, s2 = (np.asarray(a, dtype=np.float64) for a in (S, g, s2))
    M, D = g.shape
    mean, vec = np.full((M, D), np.nan), np.full((M, n_modes, D), np.nan)
    var, total = np.zeros((M, n_modes)), np.zeros(M)
    for m in range(M):
        if not s2[m] > 0:
            continue
        mean[m] = g[m] / s2[m]
        if count[m] < 2:
            continue
        Cm = (S[m] - np.outer(g[m], g[m]) / s2[m]) / s2[m]
        lam, v = np.linalg.eigh((Cm + Cm.T) / 2)
        for k in range(n_modes):
            col = v[:, D - 1 - k]
            vec[m, k] = col if col[np.argmax(np.abs(col))] > 0 else -col
            var[m, k] = max(lam[D - 1 - k], 0.)
        total[m] = max(np.trace(Cm), 0.)
    return mean, vec, var, total
