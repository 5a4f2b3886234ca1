"""
High-precision references, operands and error bounds of the kernels that tests/pointwise_dispatch.py mirrors.  Shared by
tests/test_pointwise_dispatch_cpu.py (which checks that a plain emulation of each operation in the element type stays inside
the bound: a wrong bound is found without a GPU) and tests/test_hip_pointwise_matrix.py.

Every operand holds values of the element type T (float32 or float64); u = 2^-24 or 2^-53 is its unit roundoff and
gamma(k) = k u / (1 - k u).  The references are evaluated in numpy's long double (a 64-bit mantissa where this suite runs:
2^-11 u of float64, so the reference of a float64 kernel is not itself a float64 rounding chain) and summed with math.fsum.

Elementwise and row kernels
    mu_update    pos_out == fl_T(pos + reg) bit for bit; arr_out within gamma(3) of (arr neg) / (pos + reg): the sum, the
                 product and the quotient round once each.
    axpby        (0, 1) a copy of g; (1, 1) fl_T(acc + g); (0, b) fl_T(T(b) g): bit for bit.  Otherwise
                 |got - want| <= gamma(2) (|a acc| + |b g|) with a, b rounded to T: two roundings on either term, fused
                 (generic.hip is compiled with -ffp-contract=fast) or not.
    sum_parts    the sum in rank order in the element type: bit for bit.
    normalize_W  gamma(2) + nA 2^-53 relative to w / fsum(w) (w > 0): the row sum is added in double (at most nA additions,
                 all terms positive), rounded to T, and the quotient rounds.
    apply_W      gamma(8) + nA 2^-53 relative to the update followed by the normalisation: three roundings in every
                 w' = (w neg) / (pos + eps), so three in their sum, its rounding to T and the quotient; pos_out bit for bit.
    beta_fields  the bars of test_beta_fields and test_weighted_fields.  In float32 with beta in {0, 1, 2}, r roundings
                 follow R~ (formed in T by the reference as by the kernel) and 1 ulp of the result is more than u relative:
                 r = 2 without weights (2 ulp), one more product with them (3 ulp); pow: 1e-6 relative.  float64: 1e-14.

Energies and objectives (all arithmetic in double, whatever T)
    Frobenius    the reference is 0.5 fsum(float64(fl_T(V - R))^2); every term is >= 0, so the bound is relative:
                 chain 2^-53, chain = pointwise_dispatch.chain() the longest run of double additions.
    divergences  bound = (chain + c_elem + w + 1) 2^-53 fsum(|every addend of every term|), w = 1 with weights (the product
                 G d), 1 for the reference's term rounded to double before fsum.  c_elem counts the roundings of
                 divergence<K> in units of u, a log or pow call allowed 2 ulp = 4 units:
                   K = 0   R~ and x = V / R~ (2), log x (4), the two subtractions (2)                              8
                   K = 1   R~, V / R~ (2: they move log by 2 u absolute, times V, an addend), log (4), V log (1),
                           - V, + R~ (2)                                                                           9
                   K = 3   pow(V, b) (4); R~ (1), pow(R~, b) (4 + |b| for R~'s rounding), (b - 1) * (1); pow(R~, b - 1)
                           (4 + |b - 1|), b V (1), its product (1); two additions (2); b (b - 1) and the division (2):
                           22 for |b| <= 1
                   K = 2 with weights   V - R, its square and the half (2 + 1 for a fused form)                    3
                 C_ELEM below holds the counts; a count that a GPU run showed too small would be raised there, with the
                 observed ratio next to it (none was).
"""
import math

import numpy as np

import pointwise_dispatch as pd

NP = {'f32': np.float32, 'f64': np.float64}
U = {'f32': 2. ** -24, 'f64': 2. ** -53}
U53 = 2. ** -53
HP = np.longdouble
assert np.finfo(HP).eps <= 2. ** -63, 'the references want a long double of 64 mantissa bits'

FIELD_EPS = 1e-9         # the library's eps (oracle: EPS)
ENERGY_EPS = 2. ** -10   # the energies' eps: a clamped R < 0 gives V / R~ of 1e3, not 1e9 -- one such term does not bury the rest
C_ELEM = {0: 8, 1: 9, 2: 3, 3: 22}


def gamma(k, u):
    return k * u / (1. - k * u)


def T_(x, dt):
    return np.asarray(x).astype(NP[dt])


def hp(x):
    return np.asarray(x).astype(HP)


def fsum(x):
    return math.fsum(np.asarray(x, dtype=np.float64).ravel().tolist())


def readonly(d):
    for x in d.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return d


# -- streaming kernels ------------------------------------------------------------------------------------------------------------
def stream_operands(kind, dt, n, seed=0, parts=1):
    rng = np.random.default_rng(1000 * seed + n % 9973 + len(kind))
    if kind == 'mu_update':
        return readonly(dict(arr=T_(rng.random(n) + 0.05, dt), neg=T_(rng.random(n) + 0.05, dt),
                             pos=T_(rng.random(n) + 0.05, dt), reg=0.1))
    if kind == 'axpby':
        return readonly(dict(acc=T_(2 * rng.random(n) - 1, dt), g=T_(2 * rng.random(n) - 1, dt)))
    if kind == 'sum_parts':
        return readonly(dict(parts=T_(2 * rng.random((parts, n)) - 1, dt)))
    raise ValueError(kind)


def mu_update_ref(arr, neg, pos, reg, dt):
    """-> (pos_out in T, exact; arr_out in long double; its relative bound)."""
    t = NP[dt]
    pos_out = (pos + t(reg)).astype(t)
    want = (hp(arr) * hp(neg)) / (hp(pos) + hp(t(reg)))
    return pos_out, want, gamma(3, U[dt])


def axpby_ref(acc, g, a, b, dt):
    """-> ('exact', array in T) or ('bound', want in long double, absolute bound per element)."""
    t = NP[dt]
    a, b = t(a), t(b)
    if a == 0:
        return 'exact', (g.copy() if b == 1 else (b * g).astype(t))
    if a == 1 and b == 1:
        return 'exact', (acc + g).astype(t)
    want = hp(a) * hp(acc) + hp(b) * hp(g)
    return 'bound', want, gamma(2, U[dt]) * (np.abs(hp(a) * hp(acc)) + np.abs(hp(b) * hp(g)))


def sum_parts_ref(parts):
    acc = parts[0].copy()
    for r in range(1, len(parts)):
        acc = (acc + parts[r]).astype(parts.dtype)
    return acc


def field_operands(dt, n, weighted, seed=0):
    """V in [0.05, 1.05) with zeros, R = V / x, x in [1.5, 4], with entries below zero (clamped) and at zero, G with a
    fifth of zeros, some of them over V = NaN or inf."""
    rng = np.random.default_rng(77 + 1000 * seed + n % 9973)
    V = rng.random(n) + 0.05
    R = V / (1.5 + 2.5 * rng.random(n))
    G = rng.random(n) + 0.5
    G[rng.random(n) < 0.2] = 0.
    if n > 16:
        R[[2, 9]] = -0.25, 0.
        V[5] = 0.
        G[[11, 12, 13]] = 0.
        if weighted:
            V[11], V[12] = np.nan, np.inf
    elif n == 3:
        G[1] = 0.
        if weighted:
            V[1] = np.nan
    return readonly(dict(V=T_(V, dt), R=T_(R, dt), G=T_(G, dt) if weighted else None))


def fields_ref(V, G, R, beta, eps, dt):
    """-> (Q, P in float64, mask of the entries that weights <= 0 select to an exact +0)."""
    t = NP[dt]
    if G is not None and beta == 2.:
        rt = R.astype(np.float64)                       # the weighted Frobenius step: no clamp, no eps
    else:
        rt = (np.maximum(R, t(0)) + t(eps)).astype(t).astype(np.float64)
    v = V.astype(np.float64)
    with np.errstate(all='ignore'):
        Q, P = v * rt ** (beta - 2.), rt ** (beta - 1.)
        if beta == 2.:
            Q, P = v, rt
        zero = np.zeros(V.shape, dtype=bool)
        if G is not None:
            g = G.astype(np.float64)
            zero = ~(g > 0)
            Q, P = np.where(zero, 0., g * Q), np.where(zero, 0., g * P)
    return Q, P, zero


def fields_bar(want, beta, weighted, dt):
    """The absolute bar per element (module docstring)."""
    if dt == 'f64':
        return 1e-14 * np.abs(want)
    if beta in (0., 1., 2.):
        return (3 if weighted else 2) * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return 1e-6 * np.abs(want)


# -- row kernels ------------------------------------------------------------------------------------------------------------------
def row_operands(dt, rows, nA, seed=0):
    rng = np.random.default_rng(31 + 1000 * seed + rows * 7919 + nA)
    return readonly(dict(W=T_(rng.random((rows, nA)) + 0.1, dt), neg=T_(rng.random((rows, nA)) + 0.05, dt),
                         pos=T_(rng.random((rows, nA)) + 0.05, dt), eps=FIELD_EPS))


def _row_sums(w):
    if w.dtype == HP:
        return np.sum(w, axis=1, keepdims=True)
    return np.array([fsum(row) for row in w])[:, None].astype(HP)   # (values of T: exact in float64, fsum is exact)


def normalize_ref(W, dt):
    """-> (W / fsum(W) per row in long double, relative bound)."""
    nA = W.shape[1]
    return hp(W) / _row_sums(W), gamma(2, U[dt]) + nA * U53


def apply_ref(W, neg, pos, eps, dt):
    """-> (pos_out in T, exact; the updated and normalised W in long double; relative bound)."""
    t = NP[dt]
    pos_out = (pos + t(eps)).astype(t)
    w = (hp(W) * hp(neg)) / (hp(pos) + hp(t(eps)))
    return pos_out, w / _row_sums(w), gamma(8, U[dt]) + W.shape[1] * U53


# -- ordered sums of the operator tables --------------------------------------------------------------------------------------------
def _ordered_dot(row, col, w, X, n_rows):
    """out[..., r] = the sum of w * X[..., col] over the entries of row r in ascending col, in float64 with every product and
    every addition rounded on its own, starting from 0."""
    order = np.lexsort((col, row))
    row, col, w = row[order], col[order], w[order]
    start = np.searchsorted(row, np.arange(n_rows))
    rank = np.arange(len(row)) - start[row] if len(row) else np.zeros(0, dtype=int)
    out = np.zeros(X.shape[:-1] + (n_rows,))
    for k in range(int(rank.max()) + 1 if len(rank) else 0):
        sel = rank == k
        prod = w[sel] * X[..., col[sel]]
        out[..., row[sel]] = out[..., row[sel]] + prod
    return out


def table_arrays(entries):
    t, o, i, w = (np.array([e[k] for e in entries]) for k in range(4))
    return t.astype(np.int64), o.astype(np.int64), i.astype(np.int64), w.astype(np.float64)


def ops_expand_ref(W, T, entries, dt):
    """W[M, C, *A] -> W_eff[M*T, C, *A]: the forward table's ordered float64 sums, rounded once."""
    M, C = W.shape[:2]
    nA = int(np.prod(W.shape[2:]))
    t, o, i, w = table_arrays(entries)
    out = _ordered_dot(t * nA + o, i, w, W.reshape(M, C, nA).astype(np.float64), T * nA)
    return out.reshape(M, C, T, nA).transpose(0, 2, 1, 3).reshape((M * T, C) + W.shape[2:]).astype(NP[dt])


def ops_fold_ref(X, T, entries, dt):
    """X[M*T, C, *A] -> [M, C, *A]: the adjoint table's ordered float64 sums (ascending (t, out pixel)), rounded once."""
    C = X.shape[1]
    M = X.shape[0] // T
    nA = int(np.prod(X.shape[2:]))
    t, o, i, w = table_arrays(entries)
    flat = X.reshape(M, T, C, nA).transpose(0, 2, 1, 3).reshape(M, C, T * nA).astype(np.float64)
    return _ordered_dot(i, t * nA + o, w, flat, nA).reshape((M, C) + X.shape[2:]).astype(NP[dt])


def dense_of(T, entries, nA):
    L = np.zeros((T, nA, nA))
    for t, o, i, w in entries:
        L[t, o, i] = w
    return L


# -- energies and objectives ------------------------------------------------------------------------------------------------------
RECON_W = (0.25, 0.5)    # W[0, 0, :] of the M = 1, A = (2,) problems: R[d] = 0.5 H[d] + 0.25 H[d + 1]


def activations(dt, N, L, seed=0):
    """H[N, 1, L + 1] in [0.045, 0.35) -- R in [0.034, 0.263), so V = R x with x in [1.5, 4] lies in [0.05, 1.05) -- with a
    handful of negative pairs from 257 elements on: R < 0 there, which the divergences clamp."""
    rng = np.random.default_rng(5 + 1000 * seed + 31 * N + L % 9973)
    H = 0.045 + 0.305 * rng.random((N, 1, L + 1))
    if L >= 257:
        for d in (7, 130, L - 2):
            H[:, 0, d:d + 2] = -0.2
    return T_(H, dt)


def reconstruct_T(H, dt):
    """The reconstruction of (RECON_W, H) in the element type, for the emulation without a GPU."""
    t = NP[dt]
    return (t(RECON_W[1]) * H[:, :, :-1] + t(RECON_W[0]) * H[:, :, 1:]).astype(t)


def samples_of(R, dt, beta, weighted, seed=0):
    """-> (V, G or None) of R's shape and type for a reconstruction R: V / R in [1.5, 4] where R > 0.01 and V in [0.05, 1.05)
    elsewhere; V == 0 entries at beta == 1; a fifth of G == 0, some of them over V = NaN or inf."""
    rng = np.random.default_rng(9 + 1000 * seed + R.size % 9973)
    r = R.astype(np.float64)
    V = np.where(r > 0.01, r * (1.5 + 2.5 * rng.random(R.shape)), 0.05 + rng.random(R.shape))
    flatV = V.reshape(-1)
    G = None
    if R.size >= 257 and beta == 1.:
        flatV[[3, 100]] = 0.
    if weighted:
        G = rng.random(R.shape) + 0.5
        G[rng.random(R.shape) < 0.2] = 0.
        flatG = G.reshape(-1)
        flatG[0], flatG[1] = 1.25, 0.
        flatV[1] = np.nan
        if R.size >= 257:
            flatG[[50, 51]] = 0.
            flatV[50], flatV[51] = np.inf, -1.
        G = T_(G, dt)
    return T_(V, dt), G


def terms(V, G, R, beta, eps, dt):
    """-> (term, the sum of |addends| of each term) per element in long double: the data term of k_beta_energy and of
    k_sample_objective.  Unweighted beta == 2 squares the difference taken in T."""
    v, r = hp(V), hp(R)
    K = pd.K_of(beta)
    with np.errstate(all='ignore'):
        if K == 2 and G is None:
            d = hp((V - R).astype(NP[dt]).astype(np.float64))
            term = hp((d.astype(np.float64) ** 2) * 0.5)
            mag = term
        elif K == 2:
            term = HP(0.5) * (v - r) ** 2
            mag = term
        else:
            rt = np.maximum(r, HP(0)) + HP(eps)
            if K == 0:
                x = v / rt
                lx = np.log(x)
                term, mag = x - lx - 1, np.abs(x) + np.abs(lx) + 1
            elif K == 1:
                vl = np.where(v > 0, v * np.log(np.where(v > 0, v, 1) / rt), HP(0))
                term, mag = vl - v + rt, np.abs(vl) + np.abs(v) + rt
            else:
                b = HP(beta)
                den = b * (b - 1)
                t1, t2, t3 = v ** b / den, (b - 1) * rt ** b / den, b * v * rt ** (b - 1) / den
                term, mag = t1 + t2 - t3, np.abs(t1) + np.abs(t2) + np.abs(t3)
        if G is not None:
            g = hp(G)
            live = g > 0
            term, mag = np.where(live, g * term, HP(0)), np.where(live, g * mag, HP(0))
    return term, mag


def reduced_ref(V, G, R, beta, eps, dt, chain):
    """-> (value, absolute bound) of the sum of the terms over all of V (module docstring)."""
    term, mag = terms(V, G, R, beta, eps, dt)
    value = fsum(term.astype(np.float64))
    if beta == 2. and G is None:
        return value, chain * U53 * value
    return value, (chain + C_ELEM[pd.K_of(beta)] + (G is not None) + 1) * U53 * fsum(mag.astype(np.float64))
