"""
Host mirror of the launches of the small kernels between the heavy families, restated in plain Python in the manner of
tests/atom_gram_dispatch.py:

    generic.hip   k_mu_update, k_axpby, k_sum_parts, k_apply_normalize_W<APPLY>, k_sqdiff_partial, k_sum_partials
    beta.hip      k_beta_fields<K,T,kVec,kW>, k_beta_energy<K,T,kW>, k_beta_sum, k_sample_objective<K,T,kVec,kW>,
                  k_objective_finish
    group.hip     k_group_expand, k_group_fold, k_group_apply
    atom_ops.hip  k_ops_expand, k_ops_fold, k_ops_apply<T,STAGE>

so that tests/test_hip_pointwise_matrix.py can choose the smallest problems that execute every branch of these kernels and
tests/test_pointwise_dispatch_cpu.py can check without a GPU that the choice covers them.  The number of compute units is
a parameter: the grid caps of the streaming kernels follow it, and a size of the matrix may be a function of it.

A case is a dict: ``kind``, ``dt`` ('f32' | 'f64') and the sizes of its kind; a size is a number or a function of num_cu.
"""
import random

BLOCK = 256              # kBlock of the four files
WAVES = BLOCK // 64
SHUFFLES = 6             # the steps of the wave's shuffle tree (32, 16, ..., 1)
CAP_PER_CU = 8           # grid_for (generic.hip) and grid_of (beta.hip): at most num_cu * 8 blocks
MAP_CAP = 1024           # grid_of of group.hip and atom_ops.hip
ENERGY_PARTIALS = 2048   # kEnergyPartials (generic.h)
BETA_PARTIALS = 2048     # kBetaPartials (beta.h)
OBJ_CHUNK = 4096         # kObjChunk (beta.h): elements of one sample per block
MAX_LDS = 64 * 1024      # kMaxLdsBytes (atom_ops.hip)
ESIZE = {'f32': 4, 'f64': 8}
VEC = {'f32': 4, 'f64': 2}   # elements of a 16-byte vector
DTYPES = ('f32', 'f64')
TAPS = (0, 1, 3, 4, 5, 9)    # the row lengths around the unroll by 4 of dot2_ordered


def cdiv(a, b):
    return -(-a // b)


def size(x, num_cu):
    return x(num_cu) if callable(x) else x


# -- the launch rules -----------------------------------------------------------------------------------------------------------
def grid_stream(work, num_cu):
    """grid_for / grid_of(work, ctx): one thread per unit of work, capped."""
    want, cap = cdiv(work, BLOCK), num_cu * CAP_PER_CU
    return (want if want else 1) if want < cap else cap


def grid_map(n):
    """grid_of(n) of group.hip and atom_ops.hip."""
    return 1 if n <= 0 else min(cdiv(n, BLOCK), MAP_CAP)


def grid_energy(n, num_cu, partials=ENERGY_PARTIALS):
    """launch_half_sqdiff / launch_beta_energy: the streaming grid cut to the words of the partials."""
    return min(grid_stream(n, num_cu), partials)


def full_grid(num_cu):
    """F: the threads of a full streaming grid."""
    return num_cu * CAP_PER_CU * BLOCK


def energy_full_grid(num_cu):
    return min(num_cu * CAP_PER_CU, ENERGY_PARTIALS) * BLOCK


def K_of(beta):
    """The kernel instance of a beta: 0 Itakura-Saito, 1 Kullback-Leibler, 2 Frobenius, 3 pow."""
    return {0.: 0, 1.: 1, 2.: 2}.get(float(beta), 3)


def is_vec(offsets, dt, L=None):
    """fields_as: every operand 16-byte aligned; launch_sample_objective: and samples of a whole number of vectors.
    offsets: the operands' distances from a 16-byte aligned address, in elements."""
    aligned = all((o * ESIZE[dt]) % 16 == 0 for o in offsets)
    return aligned and (L is None or (L * ESIZE[dt]) % 16 == 0)


def fields_work(n, dt, vec):
    """What fields_as sizes the grid by: n / L + 1 vectors, or n elements."""
    return n // VEC[dt] + 1 if vec else n


def objective_blocks(L):
    return cdiv(L, OBJ_CHUNK) if L else 1


def k_iter(dt):
    """kIter: the passes of a block's threads over its chunk."""
    return OBJ_CHUNK // (BLOCK * VEC[dt])


def staged_bytes(nA, T, dt):
    """launch_apply: the row and its slice of [neg | pos] of W_eff."""
    return nA * ESIZE[dt] * (1 + 2 * T)


def is_staged(nA, T, dt):
    return staged_bytes(nA, T, dt) <= MAX_LDS


def row_refused(nA, dt):
    """tnmf_hip_ops_apply_W: a row larger than the LDS staging answers TNMF_E_GEOM."""
    return nA * ESIZE[dt] > MAX_LDS


def largest_staged_nA(T, dt):
    return MAX_LDS // (ESIZE[dt] * (1 + 2 * T))


# -- operator tables in plain Python ----------------------------------------------------------------------------------------------
def hand_table(nA=20):
    """-> (T, entries [(t, out, in, w)]) with rows of 0, 1, 3, 4, 5 and 9 taps in the forward table (t = 0, out < 10) and in
    the adjoint table (in >= 10, all from t = 1): a 10 x 10 pattern whose row i holds its first r[i] columns, and its
    transpose moved to the other half of the pixels under the second map."""
    r = list(TAPS) + [2, 2, 2, 2]
    h = nA // 2
    assert h >= 10
    rnd = random.Random(5)
    out = []
    for i in range(10):
        for j in range(r[i]):
            out.append((0, i, j, 0.25 + rnd.random()))
            out.append((1, h + j, h + i, 0.25 + rnd.random()))
    return 2, out


def sparse_table(nA, T, seed):
    """Random rows of 0 to 9 taps, the lengths in a fixed cycle, weights in [0.25, 1.25)."""
    rnd = random.Random(seed)
    cycle = (2, 3, 0, 1, 4, 5, 9, 2, 1, 3)
    out = []
    for row in range(T * nA):
        k = min(cycle[row % len(cycle)], nA)
        for i in sorted(rnd.sample(range(nA), k)):
            out.append((row // nA, row % nA, i, 0.25 + rnd.random()))
    return T, out


def table_of(case):
    nA = n_pixels(case['A'])
    return hand_table(nA) if case['table'] == 'hand' else sparse_table(nA, case['T'], case.get('seed', 1))


def row_lengths(T, entries, nA):
    """-> (lengths of the forward rows (t, out), lengths of the adjoint rows (in))."""
    fwd, adj = [0] * (T * nA), [0] * nA
    for t, o, i, _ in entries:
        fwd[t * nA + o] += 1
        adj[i] += 1
    return fwd, adj


def n_pixels(A):
    n = 1
    for a in A:
        n *= a
    return n


GROUP_T = {'flip': 2, 'mirrors': 4, 'rot90': 4, 'dihedral': 8}

# -- branches ---------------------------------------------------------------------------------------------------------------------
STREAMING = ('mu_update', 'axpby', 'sum_parts', 'fields')
ROWS = ('normalize_W', 'apply_W', 'group_apply', 'ops_apply')

BRANCHES = tuple(
    [f'{k}:{b}' for k in STREAMING for b in ('one-block', 'several-blocks', 'stride-second-trip', 'ragged-last-trip')]
    + [f'axpby:a-{a}-b-{b}' for a in ('0', '1', 'other') for b in ('1', 'other')]
    + [f'sum_parts:parts-{p}' for p in ('1', '2', 'several')]
    + [f'fields:K{K}-{v}-{w}' for K in (0, 1, 3) for v in ('vec', 'scalar') for w in ('plain', 'weighted')]
    + [f'fields:K2-{v}-weighted' for v in ('vec', 'scalar')]
    + ['fields:tail-empty', 'fields:tail-some', 'fields:tail-only', 'fields:alias-vec', 'fields:alias-scalar']
    + [f'{k}:{b}' for k in ROWS for b in ('nA<64', 'nA=256', 'nA-257..511', 'nA>512')]
    + ['rows:APPLY-true', 'rows:APPLY-false', 'ops_apply:STAGE-true', 'ops_apply:STAGE-false',
       'ops_apply:staged-largest', 'ops_apply:staged-first-beyond']
    + [f'{k}:{b}' for k in ('sqdiff', 'beta_energy') for b in ('grid-below-cut', 'grid-at-cut', 'stride-second-trip')]
    + ['sum_partials:n<=256', 'sum_partials:n>256', 'beta_sum:n<=256', 'beta_sum:n>256']
    + [f'beta_energy:K{K}-plain' for K in (0, 1, 3)] + [f'beta_energy:K{K}-weighted' for K in (0, 1, 2, 3)]
    + ['beta_energy:v==0-at-K1', 'beta_energy:g<=0']
    + ['objective:B==1', 'objective:B>1', 'objective:last-block-full', 'objective:last-block-ragged',
       'objective:len-whole-passes', 'objective:len-ragged-pass', 'objective:kVec-true', 'objective:scalar-by-length',
       'objective:scalar-by-base', 'objective:finish-N<=256', 'objective:finish-N>256']
    + [f'objective:K{K}-{w}' for K in (0, 1, 2, 3) for w in ('plain', 'weighted')]
    + [f'{k}:{b}' for k in ('group_expand', 'group_fold', 'ops_expand', 'ops_fold') for b in ('below-cap', 'above-cap')]
    + ['group:flip-1d'] + [f'group:square-{g}' for g in GROUP_T]
    + [f'ops:{tab}-taps-{k}' for tab in ('forward', 'adjoint') for k in TAPS]
)


def _stream_branches(kind, work, grid, num_cu):
    out = {f'{kind}:one-block' if grid == 1 else f'{kind}:several-blocks'}
    if work > grid * BLOCK:
        out.add(f'{kind}:stride-second-trip')
    if work % BLOCK:
        out.add(f'{kind}:ragged-last-trip')
    return out


def _row_branches(kind, nA):
    if nA < 64:
        return {f'{kind}:nA<64'}
    if nA == 256:
        return {f'{kind}:nA=256'}
    if 257 <= nA <= 511:
        return {f'{kind}:nA-257..511'}
    return {f'{kind}:nA>512'} if nA > 512 else set()


def _coef(x):
    return '0' if x == 0 else '1' if x == 1 else 'other'


def reached(case, num_cu):
    """The branches a case executes on a device of num_cu compute units."""
    kind, dt = case['kind'], case['dt']
    out = set()
    if kind in ('mu_update', 'axpby', 'sum_parts'):
        n = size(case['n'], num_cu)
        out |= _stream_branches(kind, n, grid_stream(n, num_cu), num_cu)
        if kind == 'axpby':
            out.add(f'axpby:a-{_coef(case["a"])}-b-{"1" if case["b"] == 1 else "other"}')
        if kind == 'sum_parts':
            p = case['parts']
            out.add(f'sum_parts:parts-{p if p <= 2 else "several"}')
    elif kind == 'fields':
        n = size(case['n'], num_cu)
        vec = is_vec(case['offsets'], dt)
        work = fields_work(n, dt, vec)
        grid = grid_stream(work, num_cu)
        nv = n // VEC[dt] if vec else n
        out |= _stream_branches('fields', nv if nv else 1, grid, num_cu)
        w = 'weighted' if case['weighted'] else 'plain'
        out.add(f'fields:K{K_of(case["beta"])}-{"vec" if vec else "scalar"}-{w}')
        if vec:
            tail = n % VEC[dt]
            out.add('fields:tail-only' if n < VEC[dt] else 'fields:tail-some' if tail else 'fields:tail-empty')
        if case.get('alias'):
            out.add('fields:alias-vec' if vec else 'fields:alias-scalar')
    elif kind in ROWS:
        nA = n_pixels(case['A'])
        out |= _row_branches(kind, nA)
        out.add('rows:APPLY-false' if kind == 'normalize_W' else 'rows:APPLY-true')
        if kind == 'ops_apply':
            T = case['T'] if case['table'] != 'hand' else 2
            staged = is_staged(nA, T, dt)
            out.add('ops_apply:STAGE-true' if staged else 'ops_apply:STAGE-false')
            if nA == largest_staged_nA(T, dt):
                out.add('ops_apply:staged-largest')
            if nA == largest_staged_nA(T, dt) + 1:
                out.add('ops_apply:staged-first-beyond')
    elif kind == 'energy':
        n = size(case['n'], num_cu)
        plain = case['beta'] == 2. and not case['weighted']
        name, second = ('sqdiff', 'sum_partials') if plain else ('beta_energy', 'beta_sum')
        grid = grid_energy(n, num_cu, ENERGY_PARTIALS if plain else BETA_PARTIALS)
        cut = min(num_cu * CAP_PER_CU, ENERGY_PARTIALS)
        out.add(f'{name}:grid-at-cut' if grid == cut else f'{name}:grid-below-cut')
        if n > grid * BLOCK:
            out.add(f'{name}:stride-second-trip')
        out.add(f'{second}:n<=256' if grid <= BLOCK else f'{second}:n>256')
        if not plain:
            out.add(f'beta_energy:K{K_of(case["beta"])}-{"weighted" if case["weighted"] else "plain"}')
            if K_of(case['beta']) == 1 and n >= 257:
                out.add('beta_energy:v==0-at-K1')     # (the operands plant V == 0 from 257 elements on)
            if case['weighted']:
                out.add('beta_energy:g<=0')
    elif kind == 'objective':
        N, L = case['N'], case['L']
        B = objective_blocks(L)
        out.add('objective:B==1' if B == 1 else 'objective:B>1')
        last = L - (B - 1) * OBJ_CHUNK
        out.add('objective:last-block-full' if last == OBJ_CHUNK else 'objective:last-block-ragged')
        out.add('objective:len-whole-passes' if last % (BLOCK * VEC[dt]) == 0 else 'objective:len-ragged-pass')
        if is_vec(case['offsets'], dt, L):
            out.add('objective:kVec-true')
        elif not is_vec(case['offsets'], dt):
            out.add('objective:scalar-by-base')
        else:
            out.add('objective:scalar-by-length')
        if B > 1:
            out.add('objective:finish-N<=256' if N <= BLOCK else 'objective:finish-N>256')
        out.add(f'objective:K{K_of(case["beta"])}-{"weighted" if case["weighted"] else "plain"}')
    elif kind == 'group_map':
        M, C, A, name = case['M'], case['C'], case['A'], case['group']
        n = M * C * n_pixels(A)
        out.add('group_expand:above-cap' if n * GROUP_T[name] > MAP_CAP * BLOCK else 'group_expand:below-cap')
        out.add('group_fold:above-cap' if 2 * n > MAP_CAP * BLOCK else 'group_fold:below-cap')
        if len(A) == 1:
            out.add('group:flip-1d')
        elif A[0] == A[1]:
            out.add(f'group:square-{name}')
    elif kind == 'ops_map':
        M, C, nA = case['M'], case['C'], n_pixels(case['A'])
        T, entries = table_of(case)
        out.add('ops_expand:above-cap' if M * T * C * nA > MAP_CAP * BLOCK else 'ops_expand:below-cap')
        out.add('ops_fold:above-cap' if 2 * M * C * nA > MAP_CAP * BLOCK else 'ops_fold:below-cap')
        fwd, adj = row_lengths(T, entries, nA)
        out |= {f'ops:forward-taps-{k}' for k in set(fwd) & set(TAPS)}
        out |= {f'ops:adjoint-taps-{k}' for k in set(adj) & set(TAPS)}
    else:
        raise ValueError(kind)
    assert out <= set(BRANCHES), out - set(BRANCHES)
    return out


def elements(case, num_cu):
    """The elements the largest operand of a case moves ([neg | pos] counts as the two operands it holds)."""
    kind = case['kind']
    if kind in STREAMING:
        return size(case['n'], num_cu) * (case.get('parts', 1) if kind == 'sum_parts' else 1)
    if kind == 'energy':
        return size(case['n'], num_cu)
    if kind == 'objective':
        return case['N'] * case['L']
    nA = n_pixels(case['A'])
    rows = case['M'] * case['C']
    if kind in ('normalize_W', 'apply_W'):
        return rows * nA
    T = GROUP_T[case['group']] if 'group' in case else 2 if case.get('table') == 'hand' else case['T']
    return rows * T * nA


def n_rows(case):
    return case['M'] * case['C'] if case['kind'] in ROWS else 0


def chain(case, num_cu):
    """The longest chain of double additions behind a reduced value: the elements of a thread, the 6 shuffle steps, the
    waves, and for a second stage its partials per thread, its shuffle steps and its waves (k_objective_finish: the blocks
    of a sample, one after the other).  0 for a case that reduces nothing."""
    kind = case['kind']
    tree = SHUFFLES + WAVES
    if kind == 'energy':
        n = size(case['n'], num_cu)
        grid = grid_energy(n, num_cu)
        return cdiv(n, grid * BLOCK) + tree + cdiv(grid, BLOCK) + tree
    if kind == 'objective':
        return k_iter(case['dt']) * VEC[case['dt']] + tree + objective_blocks(case['L'])
    if kind in ROWS:
        return cdiv(n_pixels(case['A']), BLOCK) + tree
    return 0


# -- the matrix -------------------------------------------------------------------------------------------------------------------
def F_plus(k):
    return lambda num_cu: full_grid(num_cu) + k


STREAM_N = (1, 3, 255, 256, 257, 4097, F_plus(257))
STREAM_N_IDS = ('1', '3', '255', '256', '257', '4097', 'F+257')
OPERANDS = {'mu_update': ('arr', 'neg', 'pos'), 'axpby': ('acc', 'g'), 'sum_parts': ('parts', 'out'),
            'fields': ('V', 'G', 'R', 'Q', 'P')}
AXPBY_COEFS = ((0., 1.), (0., 0.375), (1., 1.), (1., 0.375), (0.625, 1.), (0.625, 0.375))
SUM_PARTS = (1, 2, 5)
FIELD_BETAS = (0., 0.5, 1., 2., 3.)


def offsets_of(kind):
    """The placements of a streaming kernel's operands: all aligned, each operand in turn one element off, all off."""
    names = OPERANDS[kind]
    return [('aligned', (0,) * len(names))] + [(f'{n}-off', tuple(int(m == n) for m in names)) for n in names] \
        + [('all-off', (1,) * len(names))]


def fields_n(n, dt):
    """A fields case sizes the vector kernel in vectors: F + 257 of them (and no tail)."""
    return (lambda num_cu: (full_grid(num_cu) + 257) * VEC[dt]) if callable(n) else n


def fields_offsets(weighted):
    """(id, offsets of V, G, R, Q, P); without weights G is not an operand (its slot stays aligned)."""
    return [(i, o) for i, o in offsets_of('fields') if weighted or (i != 'G-off')]


ROW_A = ((5,), (8, 8), (16, 16), (17, 17), (300,), (23, 29))
ROW_MC = ((1, 1), (2, 3))                 # (M, C): M * C in {1, 6}, C in {1, 3}
GROUPS_FOR = {1: ('flip',), 'square': ('flip', 'mirrors', 'rot90', 'dihedral'), 'oblong': ('flip', 'mirrors')}
STAGING = {'f32': ((35, 52), (1821,)), 'f64': ((26, 35), (911,))}   # T = 4: staged = 65520 B, and the first size beyond
ENERGY_N = (2, 257, 65537, lambda num_cu: energy_full_grid(num_cu) + 257)
ENERGY_N_IDS = ('2', '257', '65537', 'cut+257')
OBJECTIVE_BETAS = (2., 1., 0., 0.5)
OBJECTIVE_L = (2, 3, 1023, 1024, 1025, 4095, 4096, 4097, 8193)
BIG_GROUP = dict(M=228, C=1, A=(24, 24), group='dihedral')   # expand 1 050 624 elements, fold 262 656: above both caps
BIG_OPS = dict(M=228, C=1, A=(24, 24), table='sparse', T=2, seed=3)   # expand and fold 262 656 elements each


def groups_for(A):
    return GROUPS_FOR[1] if len(A) == 1 else GROUPS_FOR['square' if A[0] == A[1] else 'oblong']


def _matrix():
    m = {}
    for dt in DTYPES:
        for n, nid in zip(STREAM_N, STREAM_N_IDS):
            for oid, off in offsets_of('mu_update'):
                m[f'mu_update-{dt}-{nid}-{oid}'] = dict(kind='mu_update', dt=dt, n=n, offsets=off)
            for oid, off in offsets_of('axpby'):
                for a, b in AXPBY_COEFS:
                    m[f'axpby-{dt}-{nid}-{oid}-a{a}-b{b}'] = dict(kind='axpby', dt=dt, n=n, offsets=off, a=a, b=b)
            for oid, off in offsets_of('sum_parts'):
                for parts in SUM_PARTS[:2] if callable(n) else SUM_PARTS:   # (parts is one operand: 2^21 elements at most)
                    m[f'sum_parts-{dt}-{nid}-{oid}-{parts}'] = dict(kind='sum_parts', dt=dt, n=n, offsets=off, parts=parts)
        # (258: the float32 tail of two elements, which the sizes of the other streaming kernels leave out)
        for n, nid in list(zip(STREAM_N, STREAM_N_IDS)) + [(258, '258')]:
            for beta in FIELD_BETAS:
                for weighted in (False, True):
                    if beta == 2. and not weighted:
                        continue                      # (unweighted beta = 2 is the Frobenius step: no fields)
                    for oid, off in fields_offsets(weighted):
                        if (callable(n) or n == 258) and oid not in ('aligned', 'all-off'):
                            continue                  # (the full grid once per path)
                        for alias in (False, True):
                            if alias and off[2] != off[4]:
                                continue              # (P is R: one placement)
                            m[f'fields-{dt}-{nid}-{oid}-beta{beta}-{"w" if weighted else "p"}{"-alias" if alias else ""}'] = \
                                dict(kind='fields', dt=dt, n=fields_n(n, dt) if off == (0,) * 5 else n, offsets=off,
                                     beta=beta, weighted=weighted, alias=alias)
        for A in ROW_A:
            for M, C in ROW_MC:
                m[f'normalize_W-{dt}-{A}-{M}x{C}'] = dict(kind='normalize_W', dt=dt, A=A, M=M, C=C)
                m[f'apply_W-{dt}-{A}-{M}x{C}'] = dict(kind='apply_W', dt=dt, A=A, M=M, C=C)
            for M, C in ((1, 1), (3, 2)):             # M * C in {1, 6}
                for g in groups_for(A):
                    m[f'group_apply-{dt}-{A}-{M}x{C}-{g}'] = dict(kind='group_apply', dt=dt, A=A, M=M, C=C, group=g)
                m[f'ops_apply-{dt}-{A}-{M}x{C}'] = dict(kind='ops_apply', dt=dt, A=A, M=M, C=C, table='sparse', T=3,
                                                       seed=len(A) + A[-1])
        for A in STAGING[dt]:
            m[f'ops_apply-{dt}-{A}-staging'] = dict(kind='ops_apply', dt=dt, A=A, M=2, C=1, table='sparse', T=4, seed=7)
        m[f'ops_apply-{dt}-hand'] = dict(kind='ops_apply', dt=dt, A=(20,), M=2, C=2, table='hand')
        for g in GROUP_T:
            m[f'group_map-{dt}-17x17-{g}'] = dict(kind='group_map', dt=dt, M=3, C=2, A=(17, 17), group=g)
        m[f'group_map-{dt}-300-flip'] = dict(kind='group_map', dt=dt, M=3, C=2, A=(300,), group='flip')
        m[f'group_map-{dt}-above-the-cap'] = dict(kind='group_map', dt=dt, **BIG_GROUP)
        m[f'ops_map-{dt}-hand'] = dict(kind='ops_map', dt=dt, M=2, C=2, A=(20,), table='hand')
        m[f'ops_map-{dt}-sparse-1d'] = dict(kind='ops_map', dt=dt, M=3, C=2, A=(37,), table='sparse', T=3, seed=1)
        m[f'ops_map-{dt}-sparse-2d'] = dict(kind='ops_map', dt=dt, M=3, C=1, A=(7, 9), table='sparse', T=5, seed=2)
        m[f'ops_map-{dt}-above-the-cap'] = dict(kind='ops_map', dt=dt, **BIG_OPS)
        for n, nid in zip(ENERGY_N, ENERGY_N_IDS):
            for beta in OBJECTIVE_BETAS:
                for weighted in (False, True):
                    m[f'energy-{dt}-{nid}-beta{beta}-{"w" if weighted else "p"}'] = \
                        dict(kind='energy', dt=dt, n=n, beta=beta, weighted=weighted)
        for beta in OBJECTIVE_BETAS:
            for weighted in (False, True):
                w = 'w' if weighted else 'p'
                for N, L in [(3, L) for L in OBJECTIVE_L] + [(257, 4097)]:
                    m[f'objective-{dt}-{N}x{L}-beta{beta}-{w}'] = \
                        dict(kind='objective', dt=dt, N=N, L=L, beta=beta, weighted=weighted, offsets=(0, 0))
                for L in (4096, 8192):                # whole vectors behind a base one element off: the scalar path
                    m[f'objective-{dt}-3x{L}-beta{beta}-{w}-off'] = \
                        dict(kind='objective', dt=dt, N=3, L=L, beta=beta, weighted=weighted, offsets=(1, 1))
    return m


MATRIX = _matrix()
