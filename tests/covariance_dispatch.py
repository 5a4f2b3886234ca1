"""
Host mirror of the launches and the control flow of the inverse-diagonal kernels -- k_inverse_diag_rows, k_inverse_diag_lds and
k_inverse_diag_tile of tnmf_amd/csrc/covariance.hip, driven by events_inverse_diag, behind tnmf_hip_events_inverse_diag
(api.hip) -- restated in plain Python in the manner of tests/scoring_dispatch.py, so that tests/test_hip_covariance_matrix.py
can run lists that execute every branch of them and tests/test_covariance_dispatch_cpu.py can check without a GPU that the
lists cover them all.

The cases of MATRIX are SYNTHETIC Gram matrices, handed to the device as a CSR triple: they do not go through the Gram kernel
(inverse_diag_event_list and the C entry take any CSR on the device).  A case is a list of named components (COMPONENTS) and a
number of rows that are not active, laid out by `case`: the global rows of a component are a seeded random interleaving with
the other components and with the inactive rows, ascending inside the component.  Every inactive row couples to rows of at
least two components; its entries, and an active row's entries into inactive columns, hold POISON (1e30): any use of one
destroys the bits of the answer.

Every component is G = L L' with L = D L0 lower triangular, D a diagonal of powers of two, L0 of unit diagonal (the bar
components: a power of two) with small dyadic entries, and X0 = L0^-1 known in closed form with small dyadic entries too:
  'ones'        the all-ones lower triangle T_n (dense L), whose inverse is the bidiagonal (1, -1) (sparse X);
  'bidiagonal'  the two exchanged (sparse L, dense X);
  'kron'        Kronecker products of these (mixed: L = T (x) B has X = B (x) T);
  'blocks'      a block diagonal of T_8 times the elementary I + 2^-6 1_{i >= n/2} 1_{j < n/2}' (either order): a dense
                lower-left block in L, G of 76 % fill -- every run of a row longer than 64 entries from 128 rows on, and exact
                zeros inside the lower triangle, which a missing zero fill would leave as garbage;
  signs S L0 S and scalings D by 2^0 .. 2^1 on top.
The families are chosen for cond_2(G) <= 1e4, the condition of the scenes of tests/test_events_errors_cpu.py, under which the
host fallback (LAPACK) is held to the bar of tests/errors_reference.py: T_n has cond ~ (4 n + 2)^2 / pi^2, 6.95e3 at 65 rows and
1.5e5 at 300, and a Kronecker product multiplies the conditions of its parts (T_7 (x) B_10 has 1.6e4), so the all-ones family
stops at 65 rows and the larger components are 'blocks', of cond 420 .. 1 620.  The three components of the bar are the
exception on purpose: a last pivot of 2^-46 IS a condition of 2^46 n.
Every pivot is then the square of a power of two and every partial sum of the factorisation, of the inversion and of
d_i = sum_k X_ki^2 is an integer (times a common power of two) below 2^53 -- `exactness` computes the three bounds per
component in int64 -- exact in double in any order, with or without FMA: the device must equal the reference BIT FOR BIT.  The
reference d comes from X0 in integers and is checked by L0 X0 = I in integers; no floating-point factorisation is involved.

The singular components have row j of L0 made equal to row j - 1: the pivot is exactly 0 at j.  The bar components have the last
row (1, 0, ..., 0, 2^-e) under T_{n-1}: the last pivot is 2^-2e against the bar n 2^-52 (1 + 2^-2e).

`device_model` is a numpy transcription of the kernels' steps in float64 on these lists (the scatter through `local`, the
left-looking Cholesky, the inverse in place from the last column, the column sums of squares; the tiles of a batch side by side
in one scratch), vectorised over the rows of a column.  With ``defect`` it takes one wrong turn; tests/
test_covariance_dispatch_cpu.py asserts that each defect differs from the reference on the component named for it (DEFECTS) --
the proof that the case could catch it.  No kernel is broken for that.

OUT OF SCOPE, on record in NOT_REACHED: lists that break the device contract are not run -- comp_start not ascending, members
out of range, row_start outside [0, nnz], columns outside [0, K).  The clamps for them are defensive, and exercising them on a
shared GPU would mean feeding garbage indices to a kernel.  An entry between two active rows of different components cannot
exist (such an entry is an edge), so that term of the scatter's skip is not reached either; nor are the kernels' own refusals
of a component that is not of their launch, which the host plan never sends.  A CSR without its diagonal entries is outside the
contract of gram_event_list; the one-row component without a diagonal entry is the one exception the kernel documents (g = 0).
"""
import functools
import zlib

import numpy as np

import errors_reference as er

THREADS = 256                       # events.h, kEventThreads
N_LDS = er.N_LDS                    # include/tnmf_hip.h, TNMF_EVENTS_INVERSE_LDS
CLASSES = (16, 32, 64, 128, N_LDS)  # events_inverse_diag: for (const int cap : {16, 32, 64, 128, kInverseDiagLds})
LDS_DEFAULT = 64 * 1024             # beyond it the launch raises hipFuncAttributeMaxDynamicSharedMemorySize
LDS_RAISED = 160 * 1024
EPS = 2. ** -52                     # covariance.hip, kEps
POISON = 1e30
E_NULL, E_GEOM, E_UNSUPPORTED = -1, -2, -5

BRANCHES = (
    'singles:none', 'singles:some',                     # n_single == 0: every thread of k_inverse_diag_rows returns early
    'class-16:empty', 'class-16:non-empty',             # if (c1 == c0) continue;
    'class-32:empty', 'class-32:non-empty',
    'class-64:empty', 'class-64:non-empty',
    'class-128:empty', 'class-128:non-empty',
    'class-200:empty', 'class-200:non-empty',
    'tiles:none', 'tiles:some',                         # while (c0 < n_comp)
    'lds:64-threads', 'lds:256-threads',                # dim3(cap <= 64 ? 64 : kEventThreads)
    'lds:default-limit', 'lds:raised-limit',            # if (lds > 64 * 1024) hipFuncSetAttribute
    'workgroup>1-behind-c0>0',                          # c = c0 + blockIdx.x with blockIdx.x >= 2 and c0 > 0
    'rows-per-thread>1',                                # i += nt takes a second trip: n > 256, the tile path
    'run<=64', 'run>64',                                # for (k = a + lane; k < b; k += 64): a second trip
    'skip:inactive-column',                             # lj < 0
    'skip:above-diagonal',                              # lj > r
    'single:healthy', 'singular:rows:no-diagonal', 'singular:rows:zero-diagonal',   # g > 0.
    'singular:lds-64-threads', 'singular:lds-256-threads', 'singular:tile',
    'singular:first-pivot', 'singular:middle-pivot', 'singular:last-pivot',          # j = 1, n / 2, n - 1
    'singular:beside-healthy-of-its-class',
    'bar:pivot==n*eps', 'bar:pivot==4*n*eps',           # the strict > at 2^-46 against 64 and 16 times 2^-52 (1 + 2^-46)
    'batch:one', 'batch:three-tiles', 'batch:exact-fit', 'batch:several',
    'not-reached: comp_start outside the list', 'not-reached: member out of range', 'not-reached: row_start outside [0, nnz]',
    'not-reached: column out of range', 'not-reached: entry into another component',
    'not-reached: component not of the launch', 'not-reached: tile beyond the scratch',
)
NOT_REACHED = tuple(b for b in BRANCHES if b.startswith('not-reached'))


# -- the launch rules ----------------------------------------------------------------------------------------------------------
def lds_bytes(cap):
    """(size_t)cap * (cap + 3) / 2 * sizeof(double): the packed triangle and the original diagonal."""
    return cap * (cap + 3) // 2 * 8


def lds_threads(cap):
    return 64 if cap <= 64 else THREADS


def lds_raised(cap):
    return lds_bytes(cap) > LDS_DEFAULT


def packed_index(n, i, j):
    """Packed::at: column j starts at j n - j (j - 1) / 2 and holds rows j .. n - 1."""
    return j * n - j * (j - 1) // 2 + (i - j)


def tile_doubles(n):
    """covariance.h, events_inverse_diag_tile."""
    return n * n + n


def class_of(n):
    """'single', the cap of the LDS class, or 'tile'."""
    if n == 1:
        return 'single'
    return next((cap for cap in CLASSES if n <= cap), 'tile')


def default_scratch(sizes):
    """HIP.py, inverse_diag_event_list: what all tiles take, at most 2^24 doubles or one tile of the largest."""
    tiles = [tile_doubles(int(n)) for n in sizes if n > N_LDS]
    return min(sum(tiles), max(2 ** 24, tiles[-1])) if tiles else 0


def plan_batches(sizes, scratch_doubles):
    """The batch loop of events_inverse_diag over the ascending sizes -> [[component, ...], ...] of the tile launches, None
    where a tile does not fit (TNMF_E_GEOM)."""
    sizes = [int(n) for n in sizes]
    c0 = sum(n <= N_LDS for n in sizes)
    out = []
    while c0 < len(sizes):
        c1, used = c0, 0
        while c1 < len(sizes) and used + tile_doubles(sizes[c1]) <= scratch_doubles:
            used += tile_doubles(sizes[c1])
            c1 += 1
        if c1 == c0:
            return None
        out.append(list(range(c0, c1)))
        c0 = c1
    return out


def singular_bar(n, g):
    """A pivot <= n * 2^-52 * (the original G_jj) marks the component singular."""
    return float(n) * EPS * g


def refusal(n_rows, nnz, n_comp, n_active, scratch_doubles, sizes, ctx=True, row_start=True, col=True, val=True, local=True,
            d=True, comp_start=True, comp_sizes=True, member=True, status=True, scratch=True):
    """The refusals of tnmf_hip_events_inverse_diag (api.hip), in its order -> the code, 0 where the call goes through."""
    if not ctx:
        return E_NULL
    if n_rows < 0 or nnz < 0 or n_comp < 0 or n_active < 0 or scratch_doubles < 0:
        return E_NULL
    if n_rows > 0 and (not row_start or not local or not d or (nnz > 0 and (not col or not val))):
        return E_NULL
    if n_comp > 0 and (not comp_start or not comp_sizes or not member or not status):
        return E_NULL
    if n_rows > 0x7fffffff or nnz > 0x7fffffff:
        return E_UNSUPPORTED
    if n_active > n_rows or n_comp > n_active:
        return E_GEOM
    total, previous = 0, 1
    for n in list(sizes)[:n_comp]:
        if n < previous:
            return E_GEOM
        previous, total = n, total + n
        if total > n_active:
            return E_GEOM
    if total != n_active:
        return E_GEOM
    if n_comp > 0 and previous > N_LDS:
        if tile_doubles(previous) > scratch_doubles:
            return E_GEOM
        if not scratch:
            return E_NULL
    return 0


# -- the exact factors ---------------------------------------------------------------------------------------------------------
def _ones(n):
    """(T_n, its inverse): the all-ones lower triangle and the bidiagonal (1, -1)."""
    return np.tril(np.ones((n, n))), np.eye(n) - np.eye(n, k=-1)


def _factor(family, *args):
    """(L0, X0) of a family, float64 with dyadic entries; L0 X0 = I is checked in integers by `exactness`."""
    if family == 'ones':
        return _ones(args[0])
    if family == 'bidiagonal':
        return _ones(args[0])[::-1]
    if family == 'kron':                                # ('kron', ('ones', a), ('bidiagonal', b), ...)
        L, X = np.ones((1, 1)), np.ones((1, 1))
        for part in args:
            l, x = _factor(*part)
            L, X = np.kron(L, l), np.kron(X, x)
        return L, X
    if family == 'blocks':                              # (n, a, s, order): blocks of T_a, the split at n / 2, the value 2^-s
        n, a, s, order = args
        A, Ai = np.zeros((n, n)), np.zeros((n, n))
        for at in range(0, n, a):
            end = min(n, at + a)
            A[at:end, at:end], Ai[at:end, at:end] = _ones(end - at)
        E, Ei = np.eye(n), np.eye(n)
        E[n // 2:, :n // 2], Ei[n // 2:, :n // 2] = 2. ** -s, -2. ** -s
        return (A @ E, Ei @ Ai) if order == 'AE' else (E @ A, Ai @ Ei)
    if family == 'bar':                                 # (n, e): T_{n-1} and the last row (1, 0, ..., 0, 2^-e)
        n, e = args
        L, X = np.zeros((n, n)), np.zeros((n, n))
        L[:n - 1, :n - 1], X[:n - 1, :n - 1] = _ones(n - 1)
        L[n - 1, 0], L[n - 1, n - 1] = 1., 2. ** -e
        X[n - 1, 0], X[n - 1, n - 1] = -2. ** e, 2. ** e
        return L, X
    raise KeyError(family)


# name -> (kind, factor, options).  kind 'exact': finite and exact; 'singular': (factor, j) with row j of L0 := row j - 1;
# 'single': a component of one row with the diagonal value g (None: no diagonal entry in its run).
# options: sign (S L0 S, seeded), scale (the exponents of D drawn from 0 .. scale).
COMPONENTS = {
    'ones-2': ('exact', ('ones', 2), dict(scale=1)),
    'ones-16': ('exact', ('ones', 16), dict(scale=1)),
    'bidiagonal-17': ('exact', ('bidiagonal', 17), dict(scale=1)),
    'kron-20': ('exact', ('kron', ('ones', 4), ('bidiagonal', 5)), dict(scale=1)),
    'bidiagonal-29': ('exact', ('bidiagonal', 29), dict(sign=True)),
    'ones-32': ('exact', ('ones', 32), dict(sign=True)),
    'kron-33': ('exact', ('kron', ('ones', 3), ('bidiagonal', 11)), dict(sign=True)),
    'bidiagonal-64': ('exact', ('bidiagonal', 64), dict()),
    'ones-65': ('exact', ('ones', 65), dict()),
    'kron-96': ('exact', ('kron', ('ones', 3), ('blocks', 32, 8, 6, 'EA')), dict(sign=True)),
    'blocks-128': ('exact', ('blocks', 128, 8, 6, 'AE'), dict(sign=True, scale=1)),
    'blocks-129': ('exact', ('blocks', 129, 8, 6, 'EA'), dict(scale=1)),
    'blocks-199': ('exact', ('blocks', 199, 8, 6, 'AE'), dict(sign=True)),
    'blocks-200': ('exact', ('blocks', 200, 8, 6, 'EA'), dict(sign=True, scale=1)),
    'blocks-201': ('exact', ('blocks', 201, 8, 6, 'AE'), dict(scale=1)),
    'blocks-257': ('exact', ('blocks', 257, 8, 6, 'EA'), dict(sign=True)),
    'blocks-300': ('exact', ('blocks', 300, 8, 6, 'AE'), dict(sign=True, scale=1)),
    # the bar: the last pivot 2^-46 (2^-44) against n 2^-52 (1 + 2^-46)
    'bar-16-finite': ('exact', ('bar', 16, 23), dict()),
    'bar-64-singular': ('singular', (('bar', 64, 23), 63), dict(pivot=2. ** -46)),
    'bar-64-finite': ('exact', ('bar', 64, 22), dict()),
    'single-1': ('single', 1., {}), 'single-2^-4': ('single', 2. ** -4, {}), 'single-2^6': ('single', 64., {}),
    'single-2^-40': ('single', 2. ** -40, {}), 'single-2^20': ('single', 2. ** 20, {}),
    'single-no-diagonal': ('single', None, {}), 'single-zero-diagonal': ('single', 0., {}),
}
SINGULAR_SIZES = {24: 'lds-64-threads', 150: 'lds-256-threads', 210: 'tile'}
for _n in SINGULAR_SIZES:
    for _where, _j in (('first', 1), ('middle', _n // 2), ('last', _n - 1)):
        COMPONENTS[f'singular-{_n}-{_where}'] = ('singular', (('blocks', _n, 8, 6, 'AE'), _j), dict(pivot=0.))


def _seed(*what):
    return zlib.crc32(' '.join(str(w) for w in ('covariance',) + what).encode())


@functools.lru_cache(maxsize=None)
def component(name):
    """-> dict(kind, n, G [n, n] exact float64, d [n] (the exact answer; +inf on a singular one), status, and for the
    factored kinds L0, X0 (None on a singular one), exps [n] (L = diag(2^exps) L0)), read-only."""
    kind, what, opt = COMPONENTS[name]
    if kind == 'single':
        ok = what is not None and what > 0
        out = dict(kind=kind, n=1, G=np.array([[0. if what is None else what]]), has_diagonal=what is not None,
                   d=np.array([1. / what if ok else np.inf]), status=0 if ok else 1)
    else:
        rng = np.random.default_rng(_seed(name))
        L0, X0 = _factor(*(what[0] if kind == 'singular' else what))
        n = len(L0)
        if opt.get('sign'):
            s = np.where(rng.integers(0, 2, n) == 1, 1., -1.)
            L0, X0 = s[:, None] * L0 * s[None, :], s[:, None] * X0 * s[None, :]
        exps = rng.integers(0, opt['scale'] + 1, n) if opt.get('scale') else np.zeros(n, dtype=np.int64)
        if kind == 'singular':
            j = what[1]
            if opt['pivot'] == 0.:
                L0 = L0.copy()
                L0[j] = L0[j - 1]
            X0 = None
        p = _shift_of(L0)
        Li = np.round(L0 * 2. ** p).astype(np.int64)
        Gi = Li @ Li.T                                   # (entries far below 2^53: `exactness`)
        G = np.ldexp(Gi.astype(np.float64), -2 * p + exps[:, None] + exps[None, :])
        if X0 is None:
            d = np.full(n, np.inf)
        else:
            q = _shift_of(X0)
            Xi = np.round(X0 * 2. ** q).astype(np.int64)
            d = np.ldexp(np.sum(Xi * Xi, axis=0).astype(np.float64), -2 * q - 2 * exps)
        out = dict(kind=kind, n=n, G=G, d=d, status=int(kind == 'singular'), L0=L0, X0=X0, exps=exps)
        if kind == 'singular':
            out['pivot_at'] = what[1]
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _shift_of(M):
    """The smallest p with M * 2^p integer-valued."""
    for p in range(64):
        S = M * 2. ** p
        if np.array_equal(S, np.round(S)):
            return p
    raise AssertionError('not dyadic')


def exactness(name):
    """The bounds of the module docstring for a factored component, in int64 with the powers of two scaled out ->
    dict(identity: L0 X0 = I in integers (None on a singular one), cholesky = max_ij sum_k |L_ik L_jk|,
    inverse = max_ij sum_k |X_ik L_kj|, squares = max_i sum_k X_ki^2, pivots: every diagonal entry of L0 a power of two (a
    singular one: up to its zero pivot))."""
    c = component(name)
    L0, X0, n = c['L0'], c['X0'], c['n']
    p = _shift_of(L0)
    Li = np.abs(np.round(L0 * 2. ** p).astype(np.int64))
    assert int(Li.max()) ** 2 * n < 2 ** 62
    diag = np.diag(L0)[:c.get('pivot_at', n)]
    out = dict(cholesky=int((Li @ Li.T).max()), identity=None, inverse=0, squares=0,
               pivots=bool(np.all(diag > 0) and np.all(np.frexp(diag)[0] == 0.5)))
    if X0 is not None:
        q = _shift_of(X0)
        Xs = np.round(X0 * 2. ** q).astype(np.int64)
        assert int(np.abs(Xs).max()) * int(Li.max()) * n < 2 ** 62 and int(np.abs(Xs).max()) ** 2 * n < 2 ** 62
        Ls = np.round(L0 * 2. ** p).astype(np.int64)
        out['identity'] = bool(np.array_equal(Ls @ Xs, np.eye(n, dtype=np.int64) << (p + q))
                               and np.array_equal(np.triu(Ls, 1), np.zeros_like(Ls)))
        out['inverse'] = int((np.abs(Xs) @ Li).max())
        out['squares'] = int(np.sum(Xs * Xs, axis=0).max())
    return out


# -- the matrix ----------------------------------------------------------------------------------------------------------------
_SINGLES = tuple(n for n in COMPONENTS if n.startswith('single-'))
_SINGULAR = {n: tuple(f'singular-{n}-{w}' for w in ('first', 'middle', 'last')) for n in SINGULAR_SIZES}
TILES = ('blocks-201', 'blocks-257', 'blocks-300')
# the scratch sizes the tile cases are repeated under (None: the backend's default, everything in one batch)
PLANS = {'one-batch': None, 'three-batches': tile_doubles(300), 'exact-fit': tile_doubles(201) + tile_doubles(257)}

# name -> (components, rows that are not active, the branches the case is there for)
MATRIX = {
    'singles': (_SINGLES, 6, ('single:healthy', 'singular:rows:no-diagonal', 'singular:rows:zero-diagonal', 'class-16:empty',
                              'class-32:empty', 'class-64:empty', 'class-128:empty', 'class-200:empty', 'tiles:none')),
    'class-16': (('ones-2', 'ones-16', 'bar-16-finite'), 4, ('singles:none', 'bar:pivot==4*n*eps')),
    'class-32': (('bidiagonal-17', 'kron-20', 'bidiagonal-29', 'ones-32') + _SINGULAR[24] + _SINGLES[:2], 8,
                 ('workgroup>1-behind-c0>0', 'singular:lds-64-threads')),
    'class-64': (('kron-33', 'bidiagonal-64', 'bar-64-singular', 'bar-64-finite'), 4, ('bar:pivot==n*eps',)),
    'class-128': (('ones-65', 'kron-96', 'blocks-128'), 4, ()),
    'class-200': (('blocks-129', 'blocks-199', 'blocks-200') + _SINGULAR[150], 8, ('singular:lds-256-threads',)),
    'tiles': (TILES, 6, ('batch:three-tiles', 'batch:exact-fit', 'batch:several')),
    'tiles-singular': (('blocks-201',) + _SINGULAR[210], 6, ('singular:tile',)),
    'all': (tuple(COMPONENTS), 48, ()),
}
# the case and the component a defect of `device_model` is named for
DEFECTS = {
    'cholesky-one-term-short': ('class-128', 'ones-65'),
    'inverse-k<i': ('class-64', 'bidiagonal-64'),
    'inverse-read-after-write': ('class-64', 'kron-33'),
    'scatter-first-trip-only': ('class-128', 'ones-65'),
    'scatter-inactive-column': ('class-16', 'ones-16'),
    'tile-not-zeroed': ('tiles', 'blocks-201'),
    'packed-index-j(j+1)/2': ('class-16', 'ones-16'),
    'bar-without-n': ('class-64', 'bar-64-singular'),
    'bar-of-the-factored-pivot': ('class-64', 'bar-64-singular'),
    'third-tile-from-one-predecessor': ('tiles', 'blocks-257'),
}


def _csr(K, rows, cols, vals):
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    assert not np.any((rows[1:] == rows[:-1]) & (cols[1:] == cols[:-1])), 'an entry twice'
    row_start = np.searchsorted(rows, np.arange(K + 1)).astype(np.int32)
    return row_start, cols.astype(np.int32), vals.astype(np.float64)


def _lists(K, active, entries):
    """The CSR and the component lists by the breadth-first search of errors_reference on the pattern of the non-zero values."""
    rows, cols, vals = entries
    pattern = np.zeros((K, K), dtype=bool)
    pattern[rows, cols] = vals != 0
    groups = er.components(pattern, active)
    sizes = np.array([len(g) for g in groups], dtype=np.int32)
    member = np.concatenate(groups).astype(np.int32) if groups else np.zeros(0, dtype=np.int32)
    comp_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    local = np.full(K, -1, dtype=np.int32)
    for g in groups:
        local[g] = np.arange(len(g))
    return dict(K=K, active=active, csr=_csr(K, rows, cols, vals), groups=groups, sizes=sizes, member=member,
                comp_start=comp_start, local=local)


def _freeze(out):
    for a in list(out.values()) + list(out.get('csr', ())) + list(out.get('groups', ())):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _poison(rng, K, inactive, rows_of):
    """The entries of the rows that are not active: each couples to one row of two to four components, the first two taken in
    turn so that every component is touched; both triangles and the row's own diagonal hold POISON."""
    names = list(rows_of)
    r, c = [], []
    for t, u in enumerate(inactive):
        picked = {names[(2 * t) % len(names)], names[(2 * t + 1) % len(names)]}
        picked |= set(rng.choice(names, size=int(rng.integers(0, 3)), replace=False).tolist())
        assert len(picked) >= 2
        r.append(u), c.append(u)
        for name in sorted(picked):
            i = int(rng.choice(rows_of[name]))
            r += [u, i]
            c += [i, u]
    return np.array(r, dtype=np.int64), np.array(c, dtype=np.int64), np.full(len(r), POISON)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(K, active [K], csr (row_start, col, val), rows_of {component: its global rows, ascending}, groups, sizes,
    comp_start, member, local (the lists by breadth-first search), names [n_comp] (the component of every group), d [K] (the
    exact answer, NaN off the active rows), status [n_comp]), read-only."""
    names, n_inactive, _ = MATRIX[name]
    rng = np.random.default_rng(_seed('case', name))
    K = sum(component(c)['n'] for c in names) + n_inactive
    order = rng.permutation(K)
    rows_of, at = {}, 0
    for c in names:
        rows_of[c] = np.sort(order[at:at + component(c)['n']])
        at += component(c)['n']
    inactive = np.sort(order[at:])
    active = np.ones(K, dtype=bool)
    active[inactive] = False
    entries = [_poison(rng, K, inactive, rows_of)]
    d = np.full(K, np.nan)
    for c, rows in rows_of.items():
        comp = component(c)
        if comp['kind'] == 'single':                       # its diagonal entry (a stored 0.0 too), or no entry at all
            i = j = np.zeros(1 if comp['has_diagonal'] else 0, dtype=np.int64)
        else:
            i, j = np.nonzero(comp['G'] != 0)
        entries.append((rows[i], rows[j], comp['G'][i, j]))
        d[rows] = comp['d']
    out = _lists(K, active, tuple(np.concatenate(x) for x in zip(*entries)))
    owner = {int(rows[0]): c for c, rows in rows_of.items()}
    out['names'] = tuple(owner[int(g[0])] for g in out['groups'])
    assert all(np.array_equal(g, rows_of[c]) for g, c in zip(out['groups'], out['names'])) and len(out['names']) == len(names)
    out.update(rows_of=rows_of, d=d, status=np.array([component(c)['status'] for c in out['names']], dtype=np.int32))
    return _freeze(out)


def reached(name, plan='one-batch'):
    """The names of BRANCHES the case executes, its tiles under the scratch of PLANS[plan]."""
    c = case(name)
    sizes, names = c['sizes'].tolist(), c['names']
    row_start, col, _ = c['csr']
    out = {'singles:some' if 1 in sizes else 'singles:none'}
    c0 = sizes.count(1)
    for cap in CLASSES:
        mine = [i for i, n in enumerate(sizes) if class_of(n) == cap]
        out.add(f'class-{cap}:non-empty' if mine else f'class-{cap}:empty')
        if mine:
            out |= {f'lds:{lds_threads(cap)}-threads', 'lds:raised-limit' if lds_raised(cap) else 'lds:default-limit'}
            if len(mine) > 2 and mine[0] > 0:
                out.add('workgroup>1-behind-c0>0')
    tiles = [n for n in sizes if n > N_LDS]
    out.add('tiles:some' if tiles else 'tiles:none')
    if tiles:
        scratch = default_scratch(sizes) if PLANS[plan] is None else PLANS[plan]
        batches = plan_batches(sizes, scratch)
        out.add('batch:several' if len(batches) > 1 else 'batch:one')
        if any(len(b) >= 3 for b in batches):
            out.add('batch:three-tiles')
        if any(len(b) >= 2 and sum(tile_doubles(sizes[i]) for i in b) == scratch for b in batches):
            out.add('batch:exact-fit')
        if max(tiles) > THREADS:
            out.add('rows-per-thread>1')
    touched = np.zeros(c['K'], dtype=bool)              # the rows with an entry into a column that is not active
    touched[np.repeat(np.arange(c['K']), np.diff(row_start))[~c['active'][col]]] = True
    for g, n, comp in zip(c['groups'], sizes, names):
        if n > 1:
            runs = np.diff(row_start)[g]
            out |= {'run>64'} if np.any(runs > 64) else set()
            out |= {'run<=64'} if np.any(runs <= 64) else set()
            out.add('skip:above-diagonal')
        if touched[g].any():
            out.add('skip:inactive-column')
        kind = COMPONENTS[comp][0]
        if kind == 'single':
            g0 = COMPONENTS[comp][1]
            out.add('singular:rows:no-diagonal' if g0 is None else 'singular:rows:zero-diagonal' if g0 == 0 else 'single:healthy')
        if kind == 'singular':
            cls = class_of(n)
            out.add('singular:tile' if cls == 'tile' else f'singular:lds-{lds_threads(cls)}-threads')
            if any(class_of(m) == cls and COMPONENTS[o][0] == 'exact' for m, o in zip(sizes, names)):
                out.add('singular:beside-healthy-of-its-class')
            j = component(comp)['pivot_at']
            if COMPONENTS[comp][2]['pivot'] == 0.:
                out.add('singular:first-pivot' if j == 1 else 'singular:last-pivot' if j == n - 1 else 'singular:middle-pivot')
            else:
                out.add('bar:pivot==n*eps')
        if comp == 'bar-16-finite':
            out.add('bar:pivot==4*n*eps')
    assert out <= set(BRANCHES), out - set(BRANCHES)
    return out


def also():
    """{branch: every case that reaches it} for the branches more than one case reaches, the tiles under every plan."""
    out = {}
    for b in BRANCHES:
        reach = tuple(n for n in MATRIX if any(b in reached(n, plan) for plan in (PLANS if 'tiles' == n else ('one-batch',))))
        if len(reach) > 1:
            out[b] = reach
    return out


# the branches more than one case reaches: every case that does (the CPU test holds this list to `also`); 'all' holds every
# component, so it reaches whatever a class reaches but a class that is empty
ALSO = {
    'singles:none': ('class-16', 'class-64', 'class-128', 'class-200', 'tiles', 'tiles-singular'),
    'singles:some': ('singles', 'class-32', 'all'),
    'class-16:empty': ('singles', 'class-32', 'class-64', 'class-128', 'class-200', 'tiles', 'tiles-singular'),
    'class-16:non-empty': ('class-16', 'all'),
    'class-32:empty': ('singles', 'class-16', 'class-64', 'class-128', 'class-200', 'tiles', 'tiles-singular'),
    'class-32:non-empty': ('class-32', 'all'),
    'class-64:empty': ('singles', 'class-16', 'class-32', 'class-128', 'class-200', 'tiles', 'tiles-singular'),
    'class-64:non-empty': ('class-64', 'all'),
    'class-128:empty': ('singles', 'class-16', 'class-32', 'class-64', 'class-200', 'tiles', 'tiles-singular'),
    'class-128:non-empty': ('class-128', 'all'),
    'class-200:empty': ('singles', 'class-16', 'class-32', 'class-64', 'class-128', 'tiles', 'tiles-singular'),
    'class-200:non-empty': ('class-200', 'all'),
    'tiles:none': ('singles', 'class-16', 'class-32', 'class-64', 'class-128', 'class-200'),
    'tiles:some': ('tiles', 'tiles-singular', 'all'),
    'lds:64-threads': ('class-16', 'class-32', 'class-64', 'all'),
    'lds:256-threads': ('class-128', 'class-200', 'all'),
    'lds:default-limit': ('class-16', 'class-32', 'class-64', 'all'),
    'lds:raised-limit': ('class-128', 'class-200', 'all'),
    'workgroup>1-behind-c0>0': ('class-32', 'all'),
    'rows-per-thread>1': ('tiles', 'all'),
    'run<=64': ('class-16', 'class-32', 'class-64', 'all'),
    'run>64': ('class-64', 'class-128', 'class-200', 'tiles', 'tiles-singular', 'all'),
    'skip:inactive-column': ('singles', 'class-16', 'class-32', 'class-64', 'class-128', 'class-200', 'tiles',
        'tiles-singular', 'all'),
    'skip:above-diagonal': ('class-16', 'class-32', 'class-64', 'class-128', 'class-200', 'tiles', 'tiles-singular', 'all'),
    'single:healthy': ('singles', 'class-32', 'all'),
    'singular:rows:no-diagonal': ('singles', 'all'),
    'singular:rows:zero-diagonal': ('singles', 'all'),
    'singular:lds-64-threads': ('class-32', 'class-64', 'all'),
    'singular:lds-256-threads': ('class-200', 'all'),
    'singular:tile': ('tiles-singular', 'all'),
    'singular:first-pivot': ('class-32', 'class-200', 'tiles-singular', 'all'),
    'singular:middle-pivot': ('class-32', 'class-200', 'tiles-singular', 'all'),
    'singular:last-pivot': ('class-32', 'class-200', 'tiles-singular', 'all'),
    'singular:beside-healthy-of-its-class': ('class-32', 'class-64', 'class-200', 'tiles-singular', 'all'),
    'bar:pivot==n*eps': ('class-64', 'all'),
    'bar:pivot==4*n*eps': ('class-16', 'all'),
    'batch:one': ('tiles', 'tiles-singular', 'all'),
    'batch:three-tiles': ('tiles', 'tiles-singular', 'all'),
    'batch:exact-fit': ('tiles', 'tiles-singular', 'all'),
}


# -- the kernels' steps in numpy -----------------------------------------------------------------------------------------------
def _bases(n, packed, defect=None):
    """base[j] with at(i, j) = base[j] + i: the rows of a column are consecutive doubles in both layouts."""
    j = np.arange(n, dtype=np.int64)
    if packed:
        return j * n - j * ((j + 1) if defect == 'packed-index-j(j+1)/2' else (j - 1)) // 2 - j
    return j * n


def _scatter(a, base, n, mem, lists, defect):
    row_start, col, val = lists['csr']
    local, K = lists['local'], lists['K']
    for r in range(n):
        i = int(mem[r])
        k0, k1 = int(row_start[i]), int(row_start[i + 1])
        if defect == 'scatter-first-trip-only':
            k1 = min(k1, k0 + 64)
        j = col[k0:k1].astype(np.int64)
        v = val[k0:k1]
        lj = local[j].astype(np.int64)
        keep = (lj >= 0) & (lj <= r)
        keep[keep] = mem[lj[keep]] == j[keep]
        a[base[lj[keep]] + r] = v[keep]
        if defect == 'scatter-inactive-column':          # the test lj < 0 dropped: the entry lands in the row's first slot
            if np.any(lj < 0):
                a[base[0] + r] = v[lj < 0][-1]


def _factor_in_place(a, base, n, diag0, defect):
    """The left-looking Cholesky -> True where a pivot fails the bar."""
    for j in range(n):
        s = a[base[j] + j:base[j] + n].copy()
        for k in range(j - 1 if defect == 'cholesky-one-term-short' else j):
            s -= a[base[k] + j:base[k] + n] * a[base[k] + j]
        a[base[j] + j:base[j] + n] = s
        pivot = a[base[j] + j]
        bar = (EPS * diag0[j] if defect == 'bar-without-n' else float(n) * EPS * pivot if defect == 'bar-of-the-factored-pivot'
               else float(n) * EPS * diag0[j])
        if not pivot > bar:
            return True
        l = np.sqrt(pivot)
        a[base[j] + j + 1:base[j] + n] = a[base[j] + j + 1:base[j] + n] / l
        a[base[j] + j] = l
    return False


def _invert_in_place(a, base, n, tmp, defect):
    """X = L^-1 in place, column by column from the last."""
    for j in range(n - 1, -1, -1):
        x = 1. / a[base[j] + j]
        if defect == 'inverse-read-after-write':         # a row stores its X_ij at once: the rows after it read it as L_ij
            for i in range(j + 1, n):
                s = 0.
                for k in range(j + 1, i + 1):
                    s += a[base[k] + i] * a[base[j] + k]
                a[base[j] + i] = -s * x
        else:
            s = np.zeros(n - j - 1)
            for k in range(j + 1, n):                    # the term k of the rows i >= k (i > k with the defect)
                lo = k + 1 if defect == 'inverse-k<i' else k
                s[lo - j - 1:] += a[base[k] + lo:base[k] + n] * a[base[j] + k]
            keep = -s * x
            if tmp is not None:
                tmp[j + 1:n] = keep
            a[base[j] + j + 1:base[j] + n] = keep
        a[base[j] + j] = x


def _sum_of_squares(a, base, n):
    return np.array([np.sum(a[base[i] + i:base[i] + n] ** 2) for i in range(n)])


def device_model(lists, scratch_doubles=None, defect=None, only=None, prefill=np.nan):
    """The three kernels on the lists of a case (`case`, or any dict with K, csr, sizes, comp_start, member, local) -> (d [K],
    status [n_comp]); -7 where nothing is written.  ``only``: the components (indices) to run.  ``prefill``: what the LDS and
    the scratch hold before.  ``defect``: a key of DEFECTS."""
    K, sizes, member, local = lists['K'], lists['sizes'].tolist(), lists['member'], lists['local']
    row_start, col, val = lists['csr']
    start = lists['comp_start']
    d, status = np.full(K, -7.), np.full(len(sizes), -7, dtype=np.int32)
    d[local < 0] = np.nan
    todo = range(len(sizes)) if only is None else only

    def finish(c, a, base, n, mem, diag0, tmp):
        if _factor_in_place(a, base, n, diag0, defect):
            d[mem], status[c] = np.inf, 1
            return
        _invert_in_place(a, base, n, tmp, defect)
        d[mem], status[c] = _sum_of_squares(a, base, n), 0

    for c in todo:
        n, mem = sizes[c], member[start[c]:start[c + 1]]
        if n == 1:
            i = int(mem[0])
            run = slice(int(row_start[i]), int(row_start[i + 1]))
            g = val[run][col[run] == i]
            g = float(g[-1]) if len(g) else 0.
            d[i], status[c] = (1. / g, 0) if g > 0. else (np.inf, 1)
        elif n <= N_LDS:
            size = n * (n + 1) // 2
            a = np.full(size + n, prefill)
            base = _bases(n, True, defect)
            a[:size] = 0.
            _scatter(a, base, n, mem, lists, defect)
            a[size:] = a[base + np.arange(n)]
            finish(c, a, base, n, mem, a[size:], None)
    tiles = [c for c in range(len(sizes)) if sizes[c] > N_LDS]
    if tiles:
        if scratch_doubles is None:
            scratch_doubles = default_scratch(sizes)
        scratch = np.full(scratch_doubles, prefill)
        for batch in plan_batches(sizes, scratch_doubles):
            at, views = 0, []
            for c in batch:     # at: the tiles of the batch before this one
                before = [c - 1] if defect == 'third-tile-from-one-predecessor' and c > batch[0] else range(batch[0], c)
                at = sum(tile_doubles(sizes[b]) for b in before)
                views.append((c, scratch[at:at + tile_doubles(sizes[c])]))
            live = [(c, a) for c, a in views if only is None or c in only or defect == 'third-tile-from-one-predecessor']
            # the workgroups of a launch run side by side: step by step over the batch
            for c, a in live:
                if defect != 'tile-not-zeroed':
                    a[:sizes[c] ** 2] = 0.
            for c, a in live:
                _scatter(a, _bases(sizes[c], False), sizes[c], member[start[c]:start[c + 1]], lists, defect)
            for c, a in live:
                n = sizes[c]
                a[n * n:] = a[_bases(n, False) + np.arange(n)]
            for c, a in live:
                n = sizes[c]
                finish(c, a, _bases(n, False), n, member[start[c]:start[c + 1]], a[n * n:], a[n * n:])
    return d, status


def hooking(lists):
    """event_components of the HIP backend in numpy -> (label [K], rounds): min-label hooking with ceil(log2 K) pointer jumps
    a round, until a round changes nothing; no rounds for a list with the diagonal alone."""
    K, active = lists['K'], lists['active']
    row_start, col, _ = lists['csr']
    label, rounds = np.arange(K, dtype=np.int64), 0
    if len(col) > K:
        u = np.repeat(np.arange(K, dtype=np.int64), np.diff(row_start))
        c = col.astype(np.int64)
        v = np.where(active[u] & active[c], c, u)
        jumps = max(1, (K - 1).bit_length())
        while True:
            rounds += 1
            new = label.copy()
            np.minimum.at(new, label[u], label[v])
            for _ in range(jumps):
                new = new[new]
            changed = bool(np.any(new != label))
            label = new
            if not changed:
                break
    return label, rounds


# -- the component-graph cases and the dense random cases ----------------------------------------------------------------------
def _bit_reversed(n):
    bits = (n - 1).bit_length()
    assert 1 << bits == n
    return np.array([int(format(i, f'0{bits}b')[::-1], 2) for i in range(n)], dtype=np.int64)


def _graph_edges(name):
    """(K, [(i, j, value)]): the couplings above the diagonal; the diagonal is 1."""
    if name.startswith('path'):
        K = 256
        at = {'path-ascending': np.arange(K), 'path-descending': np.arange(K)[::-1], 'path-bit-reversed': _bit_reversed(K)}[name]
        return K, [(int(at[s]), int(at[s + 1]), 0.25 if s % 3 else 0.125) for s in range(K - 1)]    # (position s sits at row at[s])
    if name == 'star-hub-last':
        K = 300
        return K, [(i, K - 1, 2. ** -6 * (1 + i % 3)) for i in range(K - 1)]
    if name == 'complete-40':
        return 40, [(i, j, 2. ** -7) for i in range(40) for j in range(i + 1, 40)]
    if name == 'three-equal':       # rows 3 s + r of component r, joined along a bit-reversed order; the smallest rows 0, 1, 2
        order = _bit_reversed(16)
        return 48, [(3 * int(order[s]) + r, 3 * int(order[s + 1]) + r, 0.25) for r in range(3) for s in range(15)]
    if name == 'diagonal-only':
        return 50, []
    raise KeyError(name)


GRAPHS = ('path-ascending', 'path-descending', 'path-bit-reversed', 'star-hub-last', 'complete-40', 'three-equal',
          'diagonal-only')
DENSE_SIZES = (31, 129, 257)


@functools.lru_cache(maxsize=None)
def graph_case(name):
    """A component-graph case (every row active) or 'random-dense' (G = B B' + n I of DENSE_SIZES rows, B seeded in [-1, 1),
    interleaved, with six poisoned rows that are not active) -> the lists of `case` and dense [K, K], ref =
    errors_reference.inverse_diag(dense, active, taps = 0)."""
    if name == 'random-dense':
        rng = np.random.default_rng(_seed('dense'))
        K = sum(DENSE_SIZES) + 6
        order = rng.permutation(K)
        dense, active, at, rows_of = np.zeros((K, K)), np.ones(K, dtype=bool), 0, {}
        for n in DENSE_SIZES:
            rows = np.sort(order[at:at + n])
            B = rng.random((n, n)) * 2. - 1.
            G = np.tril(B @ B.T + n * np.eye(n))
            dense[np.ix_(rows, rows)] = G + np.tril(G, -1).T          # (bit-symmetric)
            rows_of[n], at = rows, at + n
        active[order[at:]] = False
        r, c, v = _poison(rng, K, np.sort(order[at:]), rows_of)
        dense[r, c] = v
    else:
        K, edges = _graph_edges(name)
        dense, active = np.eye(K) * (1. + np.arange(K) % 4 if name == 'diagonal-only' else 1.), np.ones(K, dtype=bool)
        for i, j, v in edges:
            assert i != j and dense[i, j] == 0
            dense[i, j] = dense[j, i] = v
    rows, cols = np.nonzero(dense)
    out = _lists(K, active, (rows, cols, dense[rows, cols]))
    out.update(dense=dense, ref=er.inverse_diag(dense, active, 0))
    assert all(np.array_equal(a, b) for a, b in zip(out['groups'], out['ref']['groups']))
    return _freeze(out)
