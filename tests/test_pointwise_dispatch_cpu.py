"""CPU guard of tests/pointwise_dispatch.py and tests/pointwise_reference.py: the mirror's constants and rules are those of
the sources (read as text), its matrix -- the cases tests/test_hip_pointwise_matrix.py runs -- reaches every branch in both
precisions on devices of 64, 256 and 304 compute units and stays small, and a plain emulation of every operation in the
element type sits inside the bound that the GPU test will ask of the kernel.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

import operator_reference as oref
import pointwise_dispatch as pd
import pointwise_reference as pr
import transform_reference as tref
from conftest import ROOT
from tnmf_amd import transforms as tr

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')
NUM_CU = (256, 64, 304)


def _flat(name):
    return re.sub(r'\s+', ' ', open(os.path.join(CSRC, name)).read())


# -- 1. the mirror is the source ----------------------------------------------------------------------------------------------------
def test_the_constants_and_rules_are_the_kernels():
    generic, gh, beta, bh = _flat('generic.hip'), _flat('generic.h'), _flat('beta.hip'), _flat('beta.h')
    group, ops, make = _flat('group.hip'), _flat('atom_ops.hip'), _flat('Makefile')
    body = ('const size_t want = ({} + kBlock - 1) / kBlock; const size_t cap = (size_t)ctx->num_cu * %d; '
            'return (int)(want < cap ? (want ? want : 1) : cap); }}' % pd.CAP_PER_CU)
    assert 'inline int grid_for(size_t n, const tnmf_hip_ctx *ctx) { ' + body.format('n') in generic
    assert 'inline int grid_of(size_t work, const tnmf_hip_ctx *ctx) { ' + body.format('work') in beta
    for src in (generic, beta, group, ops):
        assert f'constexpr int kBlock = {pd.BLOCK};' in src
    assert f'constexpr int kEnergyPartials = {pd.ENERGY_PARTIALS};' in gh
    assert f'constexpr int kBetaPartials = {pd.BETA_PARTIALS};' in bh and f'constexpr int kObjChunk = {pd.OBJ_CHUNK};' in bh
    assert 'inline size_t objective_blocks(size_t L) { return L ? (L + kObjChunk - 1) / kObjChunk : 1; }' in bh
    assert 'int grid = grid_for(n, ctx); if (grid > kEnergyPartials) grid = kEnergyPartials;' in generic
    assert 'int grid = grid_of(n, ctx); if (grid > kBetaPartials) grid = kBetaPartials;' in beta
    for line in (
            'template <> struct Vec<float> { using type = float4; static constexpr int n = 4; };',
            'template <> struct Vec<double> { using type = double2; static constexpr int n = 2; };',
            'const bool vec = ((reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(R) '
            '| reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(P)) & 15) == 0;',
            'const int grid = grid_of(vec ? n / Vec<T>::n + 1 : n, ctx);',
            'const bool vec = ((reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(G) | '
            'reinterpret_cast<uintptr_t>(R)) & 15) == 0 && (L * esize(dtype)) % 16 == 0;',
            'constexpr int kIter = kObjChunk / (kBlock * kL);',
            'if (beta == 0.0) return fields_as<0, T, kW>(ctx, beta, eps, V, G, R, Q, P, n, s); '
            'if (beta == 1.0) return fields_as<1, T, kW>(ctx, beta, eps, V, G, R, Q, P, n, s); '
            'if (beta == 2.0) return fields_as<2, T, kW>(ctx, beta, eps, V, G, R, Q, P, n, s); '
            'return fields_as<3, T, kW>(ctx, beta, eps, V, G, R, Q, P, n, s);',
            'if (beta == 0.0) objective_as<0, T, kW>(vec, beta, eps, V, G, R, L, B, grid, dst, s); '
            'else if (beta == 1.0) objective_as<1, T, kW>(vec, beta, eps, V, G, R, L, B, grid, dst, s); '
            'else if (beta == 2.0) objective_as<2, T, kW>(vec, beta, eps, V, G, R, L, B, grid, dst, s); '
            'else objective_as<3, T, kW>(vec, beta, eps, V, G, R, L, B, grid, dst, s);',
            'double *dst = B == 1 ? out : partials;',
            'for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);'):
        assert line in beta, line
    assert 'for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);' in _flat('rowsum.h')
    grid_of = f'int grid_of(int n) {{ return n <= 0 ? 1 : std::min(cdiv(n, kBlock), {pd.MAP_CAP}); }}'
    assert grid_of in group and grid_of in ops
    assert f'constexpr size_t kMaxLdsBytes = {pd.MAX_LDS // 1024} * 1024;' in ops
    for line in ('const size_t row = (size_t)tb.nA * sizeof(T), staged = row * (1 + 2 * (size_t)tb.T);',
                 'if (staged <= kMaxLdsBytes)', 'const size_t lds = (size_t)ops->nA * esize(geom->dtype); '
                 'if (lds > kMaxLdsBytes) return TNMF_E_GEOM;', '#pragma unroll 4',
                 'for (int i = threadIdx.x; i < nA; i += kBlock) {'):
        assert line in ops, line
    assert 'for (int i = threadIdx.x; i < nA; i += kBlock) {' in generic and 'for (int i = threadIdx.x; i < nA; i += kBlock) {' in group
    # the contraction flags the bounds lean on: fused forms allowed everywhere but in atom_ops.hip
    assert '-munsafe-fp-atomics -ffp-contract=fast $(DIAGFLAG)' in make
    assert '$(OBJDIR)/atom_ops.o: CXXFLAGS += -ffp-contract=off' in make


def test_the_rules():
    assert pd.grid_stream(0, 256) == 1 and pd.grid_stream(256, 256) == 1 and pd.grid_stream(257, 256) == 2
    assert pd.grid_stream(2047 * 256, 256) == 2047 and pd.grid_stream(10 ** 9, 256) == 2048 == pd.grid_stream(2048 * 256, 256)
    assert pd.grid_energy(10 ** 9, 304) == 2048 and pd.grid_energy(10 ** 9, 64) == 512 and pd.grid_stream(10 ** 9, 304) == 2432
    assert pd.grid_map(0) == 1 and pd.grid_map(262144) == 1024 == pd.grid_map(1050624) and pd.grid_map(262143) == 1024
    assert pd.grid_map(261889) == 1024 and pd.grid_map(261888) == 1023
    assert pd.k_iter('f32') == 4 and pd.k_iter('f64') == 8
    assert pd.objective_blocks(0) == 1 and pd.objective_blocks(4096) == 1 and pd.objective_blocks(4097) == 2
    assert pd.is_vec((0, 0, 0), 'f32', 4096) and not pd.is_vec((0, 1, 0), 'f32', 4096) and not pd.is_vec((0, 0), 'f32', 1023)
    assert pd.is_vec((0, 0), 'f64', 2) and not pd.is_vec((0, 0), 'f32', 2) and not pd.is_vec((0, 0), 'f64', 3)
    assert pd.is_vec((0, 2, 4), 'f64') and pd.is_vec((4,), 'f32') and not pd.is_vec((2,), 'f32')
    assert [pd.K_of(b) for b in (0., 1., 2., 0.5, 3., -1.)] == [0, 1, 2, 3, 3, 3]
    # the staging rule at its edge (T = 4): 1820 floats and 910 doubles are the largest staged rows
    assert pd.staged_bytes(1820, 4, 'f32') == 65520 == pd.staged_bytes(910, 4, 'f64')
    assert pd.is_staged(1820, 4, 'f32') and not pd.is_staged(1821, 4, 'f32')
    assert pd.is_staged(910, 4, 'f64') and not pd.is_staged(911, 4, 'f64')
    assert pd.largest_staged_nA(4, 'f32') == 1820 and pd.largest_staged_nA(4, 'f64') == 910
    assert not pd.row_refused(16384, 'f32') and pd.row_refused(16385, 'f32') and pd.row_refused(8193, 'f64')
    T, entries = pd.hand_table()
    fwd, adj = pd.row_lengths(T, entries, 20)
    assert set(fwd) >= set(pd.TAPS) and set(adj) >= set(pd.TAPS) and len(set(e[:3] for e in entries)) == len(entries)


# -- 2. the matrix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('num_cu', NUM_CU)
def test_the_matrix_reaches_every_branch_in_both_precisions(num_cu):
    for dt in pd.DTYPES:
        got = set()
        for name, case in pd.MATRIX.items():
            if case['dt'] == dt:
                got |= pd.reached(case, num_cu)
        assert got == set(pd.BRANCHES), (num_cu, dt, set(pd.BRANCHES) ^ got)
    r = lambda name: pd.reached(pd.MATRIX[name], num_cu)   # noqa: E731
    assert {'mu_update:stride-second-trip', 'mu_update:ragged-last-trip'} <= r('mu_update-f32-F+257-aligned')
    assert {'fields:K3-vec-plain', 'fields:stride-second-trip', 'fields:tail-empty'} <= r('fields-f32-F+257-aligned-beta0.5-p')
    assert {'fields:K2-scalar-weighted', 'fields:stride-second-trip', 'fields:alias-scalar'} <= \
        r('fields-f64-F+257-all-off-beta2.0-w-alias')
    assert 'fields:tail-only' in r('fields-f32-3-aligned-beta1.0-p') and 'fields:tail-some' in r('fields-f64-4097-aligned-beta0.0-w')
    assert 'fields:K0-scalar-weighted' in r('fields-f32-257-G-off-beta0.0-w')
    assert {'ops_apply:STAGE-true', 'ops_apply:staged-largest'} <= r('ops_apply-f32-(35, 52)-staging')
    assert {'ops_apply:STAGE-false', 'ops_apply:staged-first-beyond'} <= r('ops_apply-f32-(1821,)-staging')
    assert {'ops_apply:STAGE-true', 'ops_apply:staged-largest'} <= r('ops_apply-f64-(26, 35)-staging')
    assert {'ops_apply:STAGE-false', 'ops_apply:staged-first-beyond'} <= r('ops_apply-f64-(911,)-staging')
    assert {'group_expand:above-cap', 'group_fold:above-cap'} <= r('group_map-f32-above-the-cap')
    assert {'ops_expand:above-cap', 'ops_fold:above-cap'} <= r('ops_map-f64-above-the-cap')
    assert {'sqdiff:grid-at-cut', 'sqdiff:stride-second-trip', 'sum_partials:n>256'} <= r('energy-f32-cut+257-beta2.0-p')
    assert {'beta_energy:grid-at-cut', 'beta_energy:K2-weighted', 'beta_sum:n>256'} <= r('energy-f64-cut+257-beta2.0-w')
    assert {'objective:B>1', 'objective:finish-N>256', 'objective:scalar-by-length'} <= r('objective-f32-257x4097-beta1.0-p')
    assert {'objective:scalar-by-base', 'objective:last-block-full'} <= r('objective-f64-3x8192-beta0.0-w-off')
    assert 'objective:kVec-true' in r('objective-f64-3x2-beta2.0-p') and 'objective:scalar-by-length' in r('objective-f32-3x2-beta2.0-p')


@pytest.mark.parametrize('num_cu', NUM_CU)
def test_the_matrix_stays_small(num_cu):
    for name, case in pd.MATRIX.items():
        n = pd.elements(case, num_cu)
        if case['kind'] == 'fields' and callable(case['n']) and case['dt'] == 'f32' and pd.is_vec(case['offsets'], 'f32'):
            # the one case that cannot stay under 2^21: the second trip of the float32 vector kernel wants more than
            # num_cu * 8 * 256 vectors, which are 2^21 floats on 256 compute units already -- F + 257 vectors it is
            assert n == 4 * (pd.full_grid(num_cu) + 257), name
        else:
            assert n <= 2 ** 21, (name, n)
        assert pd.n_rows(case) <= 512, name
        assert pd.chain(case, num_cu) * 2. ** -53 <= 1e-9, name


# -- 3. the references alone stay inside their own bounds ---------------------------------------------------------------------------
def block_sums(x, rng):
    """x[blocks, k, 256]: every thread adds its k values in order, the wave's shuffle tree, the waves in order: block_sum."""
    acc = np.zeros(x.shape[::2])
    for k in range(x.shape[1]):
        acc = acc + x[:, k]
    lanes = acc.reshape(len(x), pd.WAVES, 64).copy()
    o = 32
    while o:
        lanes[:, :, :64 - o] = lanes[:, :, :64 - o] + lanes[:, :, o:]
        o >>= 1
    tot = np.zeros(len(x))
    for w in range(pd.WAVES):
        tot = tot + lanes[:, w, 0]
    return tot


def reduce_like_the_kernels(values, grid, rng):
    """The sum of float64 values in a shuffled order through the two stages of the energies."""
    v = rng.permutation(values.ravel())
    per = pd.cdiv(len(v), grid * pd.BLOCK)
    pad = np.zeros(per * grid * pd.BLOCK)
    pad[:len(v)] = v
    partials = block_sums(pad.reshape(per, grid, pd.BLOCK).transpose(1, 0, 2), rng)
    per2 = pd.cdiv(grid, pd.BLOCK)
    pad2 = np.zeros(per2 * pd.BLOCK)
    pad2[:grid] = partials
    return float(block_sums(pad2.reshape(1, per2, pd.BLOCK), rng)[0])


def row_sum_T(w, rng, dt):
    """Row sums in double in a shuffled order through block_sum, rounded to T."""
    rows, nA = w.shape
    per = pd.cdiv(nA, pd.BLOCK)
    pad = np.zeros((rows, per * pd.BLOCK))
    pad[:, :nA] = rng.permuted(w.astype(np.float64), axis=1)
    return block_sums(pad.reshape(rows, per, pd.BLOCK), rng).astype(pr.NP[dt])[:, None]


def terms_in_double(V, G, R, beta, eps, dt):
    """term<K, T, kW> of beta.hip in numpy float64."""
    v, r = V.astype(np.float64), R.astype(np.float64)
    K = pd.K_of(beta)
    with np.errstate(all='ignore'):
        if K == 2 and G is None:
            d = (V - R).astype(pr.NP[dt]).astype(np.float64)
            return 0.5 * (d * d)
        if K == 2:
            d = 0.5 * (v - r) * (v - r)
        else:
            rt = np.where(r > 0, r, 0.) + eps
            if K == 0:
                x = v / rt
                d = x - np.log(x) - 1.
            elif K == 1:
                d = np.where(v > 0, v * np.log(np.where(v > 0, v, 1.) / rt), 0.) - v + rt
            else:
                d = (v ** beta + (beta - 1.) * rt ** beta - beta * v * rt ** (beta - 1.)) / (beta * (beta - 1.))
        if G is None:
            return d
        g = G.astype(np.float64)
        return np.where(g > 0, g * d, 0.)


def _keys(kind, *fields):
    """The distinct cases of a kind, without the placements (an emulation does not see an address)."""
    seen = {}
    for case in pd.MATRIX.values():
        if case['kind'] == kind:
            seen.setdefault(tuple(str(case.get(f)) for f in ('dt',) + fields), case)
    return list(seen.values())


def n_of(case):
    """The full-grid sizes at 256 compute units; the float32 vector case at the scalar one's size (elementwise bounds do
    not know the grid)."""
    return min(pd.size(case['n'], 256), pd.full_grid(256) + 257)


def test_the_streaming_references_stay_inside_their_bounds():
    for case in _keys('mu_update', 'n'):
        dt, t = case['dt'], pr.NP[case['dt']]
        o = pr.stream_operands('mu_update', dt, n_of(case))
        pos_out, want, bound = pr.mu_update_ref(o['arr'], o['neg'], o['pos'], o['reg'], dt)
        p = o['pos'] + t(o['reg'])
        got = (o['arr'] * o['neg']) / p
        assert got.dtype == t and np.array_equal(p, pos_out)
        assert np.all(np.abs(pr.hp(got) - want) <= bound * np.abs(want)), dt
    for case in _keys('axpby', 'n', 'a', 'b'):
        dt, t = case['dt'], pr.NP[case['dt']]
        o = pr.stream_operands('axpby', dt, n_of(case))
        a, b = t(case['a']), t(case['b'])
        got = a * o['acc'] + b * o['g']
        assert got.dtype == t
        ref = pr.axpby_ref(o['acc'], o['g'], case['a'], case['b'], dt)
        if ref[0] == 'exact':
            assert np.array_equal(got, ref[1]), case
        else:
            assert np.all(np.abs(pr.hp(got) - ref[1]) <= ref[2]), case
    for case in _keys('sum_parts', 'n', 'parts'):
        parts = pr.stream_operands('sum_parts', case['dt'], n_of(case), parts=case['parts'])['parts']
        assert np.array_equal(np.cumsum(parts, axis=0, dtype=parts.dtype)[-1], pr.sum_parts_ref(parts))


def fields_in_T(V, G, R, beta, eps, dt):
    """field / wfield of beta.hip in numpy arithmetic of the element type."""
    t = NP = pr.NP[dt]   # noqa: N806
    one = t(1)
    with np.errstate(all='ignore'):
        rt = (np.where(R > 0, R, t(0)) + t(eps)).astype(t)
        K = pd.K_of(beta)
        if K == 0:
            q, p = V / (rt * rt), one / rt
        elif K == 1:
            q, p = V / rt, np.ones_like(V)
        elif K == 2:
            q, p = (V, rt) if G is None else (V, R)
        else:
            q, p = V * np.power(rt, t(beta - 2.)), np.power(rt, t(beta - 1.))
        if G is not None:
            q, p = np.where(G > 0, G * q, t(0)), np.where(G > 0, G if K == 1 else G * p, t(0))
    assert q.dtype == NP and p.dtype == NP
    return q, p


def test_the_field_references_stay_inside_their_bars():
    for case in _keys('fields', 'n', 'beta', 'weighted'):
        dt, beta, weighted = case['dt'], case['beta'], case['weighted']
        o = pr.field_operands(dt, n_of(case), weighted)
        Qw, Pw, zero = pr.fields_ref(o['V'], o['G'], o['R'], beta, pr.FIELD_EPS, dt)
        q, p = fields_in_T(o['V'], o['G'], o['R'], beta, pr.FIELD_EPS, dt)
        for got, want in ((q, Qw), (p, Pw)):
            assert np.all(np.isfinite(got)) and np.all(got[zero] == 0.) and not np.any(np.signbit(got[zero]))
            assert np.all(np.abs(got.astype(np.float64) - want) <= pr.fields_bar(want, beta, weighted, dt)), case


def test_the_row_references_stay_inside_their_bounds():
    rng = np.random.default_rng(0)
    for case in _keys('normalize_W', 'A', 'M', 'C'):
        dt, t, nA = case['dt'], pr.NP[case['dt']], pd.n_pixels(case['A'])
        o = pr.row_operands(dt, case['M'] * case['C'], nA)
        want, bound = pr.normalize_ref(o['W'], dt)
        got = o['W'] / row_sum_T(o['W'], rng, dt)
        assert got.dtype == t and np.all(np.abs(pr.hp(got) - want) <= bound * want)
        pos_out, want, bound = pr.apply_ref(o['W'], o['neg'], o['pos'], o['eps'], dt)
        p = o['pos'] + t(o['eps'])
        w = (o['W'] * o['neg']) / p
        got = w / row_sum_T(w, rng, dt)
        assert got.dtype == t and np.array_equal(p, pos_out) and np.all(np.abs(pr.hp(got) - want) <= bound * want)
        assert abs(float(np.sum(want[0])) - 1.) < 1e-15


def test_the_ordered_sums_are_the_tables_sums():
    """The ordered float64 sums of the reference against the package's numpy tables (bit for bit) and against the dense
    einsum of tests/operator_reference.py (k + 1 roundings behind a row of k taps)."""
    for case in _keys('ops_map', 'A', 'table', 'T', 'seed', 'M', 'C'):
        if case['M'] > 10:
            continue                                     # (the case above the grid cap: the same table code)
        dt, A, M, C = case['dt'], case['A'], case['M'], case['C']
        T, entries = pd.table_of(case)
        nA = pd.n_pixels(A)
        ops = tr.AtomOperators(A, T, *pr.table_arrays(entries))
        rng = np.random.default_rng(3)
        W = pr.T_(rng.random((M, C) + A) + 0.1, dt)
        X = pr.T_(rng.random((M * T, C) + A) + 0.05, dt)
        We, F = pr.ops_expand_ref(W, T, entries, dt), pr.ops_fold_ref(X, T, entries, dt)
        assert We.dtype == W.dtype and np.array_equal(We, tr.expand(W, ops)) and np.array_equal(F, tr.fold(X, ops))
        L = pr.dense_of(T, entries, nA)
        np.testing.assert_array_equal(L, oref.dense(ops))
        fwd, adj = pd.row_lengths(T, entries, nA)
        u = pr.U[dt] + (max(fwd + adj) + 1) * pr.U53
        dWe, dF = oref.expand(W, L), oref.fold(X, L)
        assert np.all(np.abs(We - dWe) <= u * dWe) and np.all(np.abs(F - dF) <= u * dF)
    for name in pd.GROUP_T:                              # a group as a table: the permutation and the float64 fold
        A = (4, 4)
        ops = tr.from_group(name, A)
        entries = list(zip(*(x.tolist() for x in ops.entries)))
        W = np.random.default_rng(1).random((2, 2) + A)
        X = np.random.default_rng(2).random((2 * ops.T, 2) + A).astype(np.float32)
        assert np.array_equal(pr.ops_expand_ref(W, ops.T, entries, 'f64'), tref.expand(W, name))
        assert np.array_equal(pr.ops_fold_ref(X, ops.T, entries, 'f32'), tref.fold(X.astype(np.float64), name).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _reconstruction(dt, N, L):
    H = pr.activations(dt, N, L)
    return pr.reconstruct_T(H, dt)


def test_the_energy_references_stay_inside_their_bounds():
    rng = np.random.default_rng(1)
    worst = {}
    for case in _keys('energy', 'n', 'beta', 'weighted'):
        dt, n, beta, weighted = case['dt'], pd.size(case['n'], 256), case['beta'], case['weighted']
        R = _reconstruction(dt, 1, n)
        V, G = pr.samples_of(R, dt, beta, weighted)
        chain = pd.chain(case, 256)
        want, bound = pr.reduced_ref(V, G, R, beta, pr.ENERGY_EPS, dt, chain)
        got = reduce_like_the_kernels(terms_in_double(V, G, R, beta, pr.ENERGY_EPS, dt), pd.grid_energy(n, 256), rng)
        assert np.isfinite(want) and want > 0 and abs(got - want) <= bound, (case, got, want, bound)
        key = (pd.K_of(beta), dt)
        worst[key] = max(worst.get(key, 0.), abs(got - want) / bound)
    print('energy emulation, largest error / bound per (K, type):', {k: round(v, 3) for k, v in sorted(worst.items())})


def test_the_objective_references_stay_inside_their_bounds():
    rng = np.random.default_rng(2)
    for case in _keys('objective', 'N', 'L', 'beta', 'weighted'):
        dt, N, L, beta, weighted = case['dt'], case['N'], case['L'], case['beta'], case['weighted']
        if N > 3 and (beta, weighted) not in ((2., False), (0.5, True)):
            continue                                     # (257 samples: the same sums 257 times)
        R = _reconstruction(dt, N, L)
        V, G = pr.samples_of(R, dt, beta, weighted)
        chain = pd.chain(case, 256)
        t = terms_in_double(V, G, R, beta, pr.ENERGY_EPS, dt)
        B = pd.objective_blocks(L)
        for n in range(min(N, 3)):
            want, bound = pr.reduced_ref(V[n], None if G is None else G[n], R[n], beta, pr.ENERGY_EPS, dt, chain)
            pad = np.zeros(B * pd.OBJ_CHUNK)
            pad[:L] = t[n].ravel()
            blocks = pad.reshape(B, pd.OBJ_CHUNK)
            for b in range(B):
                blocks[b] = rng.permutation(blocks[b])
            partials = block_sums(blocks.reshape(B, pd.OBJ_CHUNK // pd.BLOCK, pd.BLOCK), rng)
            got = 0.
            for x in partials:
                got = got + x
            assert abs(got - want) <= bound, (case, n, got, want, bound)
