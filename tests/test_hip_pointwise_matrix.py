"""
Every branch of the pointwise, row-sum and atom-map kernels on the GPU, through the C ABI, against the references and
bounds of tests/pointwise_reference.py (derived there, and checked without a GPU by tests/test_pointwise_dispatch_cpu.py):

    generic.hip   k_mu_update, k_axpby, k_sum_parts, k_apply_normalize_W<APPLY>, k_sqdiff_partial, k_sum_partials
    beta.hip      k_beta_fields<K,T,kVec,kW>, k_beta_energy<K,T,kW>, k_beta_sum, k_sample_objective<K,T,kVec,kW>,
                  k_objective_finish
    group.hip     k_group_expand, k_group_fold, k_group_apply
    atom_ops.hip  k_ops_expand, k_ops_fold, k_ops_apply<T,STAGE>

The cases are those of tests/pointwise_dispatch.py: the smallest that reach every branch on the device's number of compute
units.  Every buffer a kernel writes is followed by 64 sentinel elements (and preceded by 64 where the operand sits one
element off a 16-byte boundary); the sentinels must come back untouched and every read-only operand bit-identical.  The
energies and objectives reconstruct internally: their reference is built from the library's own reconstruction of the same
(W, H) on the same context (two calls, the same bits), so the bound is the reduction's own.  The context runs the generic
kernels (M = 1, A = (2,) on one shift axis, so that L = C * D takes any value).  Every case prints the largest ratio of an
error to its bound, every test the largest of its cases.

Largest ratios on an MI355X (256 compute units), float32 / float64: mu_update 0.85 / 0.97, axpby 0.96 / 0.99, normalize_W
0.85 / 0.25, apply_W 0.34 / 0.19, group_apply 0.36 / 0.18, ops_apply 0.36 / 0.17, beta_fields 0.76 / 0.12 of their bars,
the energies 0.06 / 0.06 (K = 0: 0.03 / 0.05, K = 1: 0.015 / 0.008, K = 3: 0.009 / 0.002: no count of
pointwise_reference.C_ELEM had to be raised), the per-sample objectives 0.11 / 0.11, their sum against the energy 0.04.
sum_parts, the maps and the fused updates against their unfused chains: the same bits.  k_ops_apply<T, true> with 65520
bytes of dynamic LDS next to its 32 static bytes: the launch is accepted, in both precisions.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import operator_reference as oref
import pointwise_dispatch as pd
import pointwise_reference as pr
import transform_reference as tref
from tnmf_amd import _lib

pytestmark = pytest.mark.gpu

NP = pr.NP
TORCH = {'f32': torch.float32, 'f64': torch.float64}
CODE = {'f32': 0, 'f64': 1}
PATTERN = -12345.5
MARGIN = 64


@functools.lru_cache(maxsize=None)
def context():
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    _lib.check(lib.tnmf_hip_ctx_create(torch.cuda.current_device(), ctypes.byref(ctx)), 'ctx_create')
    _lib.check(lib.tnmf_hip_ctx_set_path(ctx, _lib.PATHS['generic']), 'set_path')
    return lib, ctx


@functools.lru_cache(maxsize=None)
def num_cu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def cases(kind, dt, **fixed):
    return [(name, c) for name, c in pd.MATRIX.items()
            if c['kind'] == kind and c['dt'] == dt and all(c[k] == v for k, v in fixed.items())]


class Buf:
    """A device operand between sentinels: 64 behind it, and 64 + 1 before it when it is one element off alignment."""

    def __init__(self, host, dt=None, off=0):
        dtype = TORCH[dt] if dt else torch.float64
        self.host = np.array(host, dtype=NP[dt] if dt else np.float64, order='C')   # (a copy: the operands are read-only)
        self.n = self.host.size
        self.front = MARGIN + 1 if off else 0
        self.t = torch.full((self.front + self.n + MARGIN,), PATTERN, dtype=dtype, device='cuda')
        self.view = self.t[self.front:self.front + self.n]
        self.view.copy_(torch.from_numpy(self.host.reshape(-1)))
        assert self.view.data_ptr() % 16 == (off * self.t.element_size()) % 16
        self.ptr = ctypes.c_void_p(self.view.data_ptr())

    @classmethod
    def out(cls, shape, dt=None, off=0):
        return cls(np.full(shape, PATTERN, dtype=NP[dt] if dt else np.float64), dt, off)

    def get(self):
        return self.view.cpu().numpy().reshape(self.host.shape)

    def margins_ok(self):
        return bool(torch.all(self.t[:self.front] == PATTERN)) and bool(torch.all(self.t[self.front + self.n:] == PATTERN))

    def unchanged(self):
        return self.margins_ok() and self.get().tobytes() == self.host.tobytes()

    def written(self):
        return self.margins_ok() and not np.any(self.get() == PATTERN)


def sync():
    torch.cuda.synchronize()


def ratio(err, bound):
    """The largest err / bound; a bound of 0 asks for an exact 0."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.all(np.isfinite(err)) and np.all(err[bound == 0] == 0)
    return float(np.max(err[bound > 0] / bound[bound > 0], initial=0.))


def report(name, *ratios):
    """One line per case: its largest error over its bound."""
    print(f'pointwise {name}: error / bound ' + ', '.join(f'{r:.3f}' for r in ratios))
    return max(ratios)


def test_the_matrix_reaches_every_branch_on_this_device():
    for dt in pd.DTYPES:
        got = set()
        for _, c in pd.MATRIX.items():
            if c['dt'] == dt:
                got |= pd.reached(c, num_cu())
        assert got == set(pd.BRANCHES), (num_cu(), set(pd.BRANCHES) ^ got)
    F = pd.full_grid(num_cu())
    assert pd.grid_stream(F + 257, num_cu()) == num_cu() * 8 and pd.grid_stream(F - 256, num_cu()) == num_cu() * 8 - 1


# -- 1. streaming kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', pd.DTYPES)
def test_mu_update(dt):
    lib, ctx = context()
    worst = 0.
    for name, c in cases('mu_update', dt):
        n = pd.size(c['n'], num_cu())
        o = pr.stream_operands('mu_update', dt, n)
        pos_out, want, bound = pr.mu_update_ref(o['arr'], o['neg'], o['pos'], o['reg'], dt)
        arr, neg, pos = (Buf(o[k], dt, off) for k, off in zip(('arr', 'neg', 'pos'), c['offsets']))
        assert lib.tnmf_hip_mu_update(ctx, CODE[dt], arr.ptr, neg.ptr, pos.ptr, o['reg'], n, None) == 0, name
        sync()
        assert neg.unchanged() and arr.margins_ok() and pos.margins_ok(), name
        assert pos.get().tobytes() == pos_out.tobytes(), name
        worst = max(worst, report(name, ratio(np.abs(pr.hp(arr.get()) - want), bound * np.abs(want))))
        assert worst <= 1., name
    print(f'pointwise mu_update {dt}: largest error / bound {worst:.3f}')


@pytest.mark.parametrize('dt', pd.DTYPES)
def test_axpby(dt):
    lib, ctx = context()
    worst = 0.
    for name, c in cases('axpby', dt):
        n = pd.size(c['n'], num_cu())
        o = pr.stream_operands('axpby', dt, n)
        ref = pr.axpby_ref(o['acc'], o['g'], c['a'], c['b'], dt)
        acc, g = Buf(o['acc'], dt, c['offsets'][0]), Buf(o['g'], dt, c['offsets'][1])
        assert lib.tnmf_hip_axpby(ctx, CODE[dt], acc.ptr, g.ptr, c['a'], c['b'], n, None) == 0, name
        sync()
        assert g.unchanged() and acc.margins_ok(), name
        if ref[0] == 'exact':
            assert acc.get().tobytes() == ref[1].tobytes(), name
        else:
            worst = max(worst, report(name, ratio(np.abs(pr.hp(acc.get()) - ref[1]), ref[2])))
            assert worst <= 1., name
    print(f'pointwise axpby {dt}: largest error / bound {worst:.3f} (the exact cases: the same bits)')


@pytest.mark.parametrize('dt', pd.DTYPES)
def test_sum_parts(dt):
    lib, ctx = context()
    for name, c in cases('sum_parts', dt):
        n = pd.size(c['n'], num_cu())
        parts = pr.stream_operands('sum_parts', dt, n, parts=c['parts'])['parts']
        src, out = Buf(parts, dt, c['offsets'][0]), Buf.out(n, dt, c['offsets'][1])
        assert lib.tnmf_hip_sum_parts(ctx, CODE[dt], src.ptr, c['parts'], n, out.ptr, None) == 0, name
        sync()
        assert src.unchanged() and out.margins_ok(), name
        assert out.get().tobytes() == pr.sum_parts_ref(parts).tobytes(), name
    print(f'pointwise sum_parts {dt}: the same bits as the sum in rank order')


@pytest.mark.parametrize('dt', pd.DTYPES)
def test_no_elements_is_no_launch(dt):
    lib, ctx = context()
    bufs = [Buf(np.arange(8.), dt) for _ in range(5)]
    a, b, c, d, e = (x.ptr for x in bufs)
    assert lib.tnmf_hip_mu_update(ctx, CODE[dt], a, b, c, 0.1, 0, None) == 0
    assert lib.tnmf_hip_axpby(ctx, CODE[dt], a, b, 0.5, 0.5, 0, None) == 0
    assert lib.tnmf_hip_sum_parts(ctx, CODE[dt], a, 2, 0, b, None) == 0
    assert lib.tnmf_hip_beta_fields(ctx, CODE[dt], 1., 1e-9, a, b, c, d, 0, None) == 0
    assert lib.tnmf_hip_weighted_fields(ctx, CODE[dt], 1., 1e-9, a, b, c, d, e, 0, None) == 0
    sync()
    assert all(x.unchanged() for x in bufs)


FIELD_CASES = [(b, w) for b in pd.FIELD_BETAS for w in (False, True) if w or b != 2.]


@pytest.mark.parametrize('dt', pd.DTYPES)
@pytest.mark.parametrize('beta,weighted', FIELD_CASES, ids=[f'beta{b}-{"weighted" if w else "plain"}' for b, w in FIELD_CASES])
def test_beta_fields(beta, weighted, dt):
    lib, ctx = context()
    worst = 0.
    for name, c in cases('fields', dt, beta=beta, weighted=weighted):
        n = pd.size(c['n'], num_cu())
        o = pr.field_operands(dt, n, weighted)
        Qw, Pw, zero = pr.fields_ref(o['V'], o['G'], o['R'], beta, pr.FIELD_EPS, dt)
        oV, oG, oR, oQ, oP = c['offsets']
        V, R, Q = Buf(o['V'], dt, oV), Buf(o['R'], dt, oR), Buf.out(n, dt, oQ)
        G = Buf(o['G'], dt, oG) if weighted else None
        P = R if c['alias'] else Buf.out(n, dt, oP)
        if weighted:
            rc = lib.tnmf_hip_weighted_fields(ctx, CODE[dt], beta, pr.FIELD_EPS, V.ptr, G.ptr, R.ptr, Q.ptr, P.ptr, n, None)
        else:
            rc = lib.tnmf_hip_beta_fields(ctx, CODE[dt], beta, pr.FIELD_EPS, V.ptr, R.ptr, Q.ptr, P.ptr, n, None)
        sync()
        assert rc == 0 and V.unchanged() and (G is None or G.unchanged()) and (c['alias'] or R.unchanged()), name
        assert Q.margins_ok() and P.margins_ok(), name
        for got, want in ((Q.get().astype(np.float64), Qw), (P.get().astype(np.float64), Pw)):
            assert np.all(np.isfinite(got)) and np.all(got[zero] == 0.) and not np.any(np.signbit(got[zero])), name
            worst = max(worst, report(name, ratio(np.abs(got - want), pr.fields_bar(want, beta, weighted, dt))))
            assert worst <= 1., name
    print(f'pointwise beta_fields {dt} beta={beta} {"weighted" if weighted else "plain"}: largest error / bar {worst:.3f}')


# -- 2. row kernels -----------------------------------------------------------------------------------------------------------------
def dict_geom(M, C, A, dt):
    return _lib.make_geom(0, M, C, tuple(2 * a for a in A), A, CODE[dt])   # (N and D are not read)


@pytest.mark.parametrize('dt', pd.DTYPES)
def test_normalize_W_and_apply_W(dt):
    lib, ctx = context()
    worst_n = worst_a = 0.
    for name, c in cases('normalize_W', dt):
        M, C, A = c['M'], c['C'], c['A']
        nA = pd.n_pixels(A)
        o = pr.row_operands(dt, M * C, nA)
        g = dict_geom(M, C, A, dt)
        W = Buf(o['W'], dt)
        assert lib.tnmf_hip_normalize_W(ctx, ctypes.byref(g), W.ptr, None) == 0, name
        sync()
        want, bound = pr.normalize_ref(o['W'], dt)
        assert W.margins_ok(), name
        worst_n = max(worst_n, ratio(np.abs(pr.hp(W.get()) - want), bound * want))
        W, negpos = Buf(o['W'], dt), Buf(np.stack([o['neg'], o['pos']]), dt)
        assert lib.tnmf_hip_apply_W(ctx, ctypes.byref(g), W.ptr, negpos.ptr, o['eps'], None) == 0, name
        sync()
        pos_out, want, bound = pr.apply_ref(o['W'], o['neg'], o['pos'], o['eps'], dt)
        assert W.margins_ok() and negpos.margins_ok(), name
        assert negpos.get()[0].tobytes() == o['neg'].tobytes() and negpos.get()[1].tobytes() == pos_out.tobytes(), name
        worst_a = max(worst_a, ratio(np.abs(pr.hp(W.get()) - want), bound * want))
        report(name + ' / apply_W', worst_n, worst_a)
        assert worst_n <= 1. and worst_a <= 1., name
    print(f'pointwise normalize_W {dt}: largest error / bound {worst_n:.3f}; apply_W: {worst_a:.3f}')


def gradient_of(rng, M, T, C, A, dt):
    return pr.T_(rng.random((2, M * T, C) + tuple(A)) + 0.05, dt)


@pytest.mark.parametrize('dt', pd.DTYPES)
def test_group_apply_is_fold_apply_expand_to_the_bit(dt):
    lib, ctx = context()
    worst = 0.
    for name, c in cases('group_apply', dt):
        M, C, A, gname = c['M'], c['C'], c['A'], c['group']
        T, gid, nA = pd.GROUP_T[gname], _lib.GROUPS[gname], pd.n_pixels(A)
        rng = np.random.default_rng(nA + M)
        W0 = pr.T_(rng.random((M, C) + A) + 0.1, dt)
        X0 = gradient_of(rng, M, T, C, A, dt)
        g = ctypes.byref(dict_geom(M, C, A, dt))
        W1, We1, X = Buf(W0, dt), Buf.out((M * T, C) + A, dt), Buf(X0, dt)
        assert lib.tnmf_hip_group_apply_W(ctx, g, gid, W1.ptr, We1.ptr, X.ptr, pr.FIELD_EPS, None) == 0, name
        W2, F2, We2 = Buf(W0, dt), Buf.out((2, M, C) + A, dt), Buf.out((M * T, C) + A, dt)
        assert lib.tnmf_hip_group_fold_grad_W(ctx, g, gid, X.ptr, F2.ptr, None) == 0
        assert lib.tnmf_hip_apply_W(ctx, g, W2.ptr, F2.ptr, pr.FIELD_EPS, None) == 0
        assert lib.tnmf_hip_group_expand_W(ctx, g, gid, W2.ptr, We2.ptr, None) == 0
        sync()
        assert X.unchanged() and W1.written() and We1.written() and W2.written() and We2.written() and F2.written(), name
        assert W1.get().tobytes() == W2.get().tobytes() and We1.get().tobytes() == We2.get().tobytes(), name
        # and the chain is right: the float64 fold, rounded once, through the bound of apply_W
        fold = np.stack([tref.fold(X0[h].astype(np.float64), gname) for h in (0, 1)]).astype(NP[dt])
        _, want, bound = pr.apply_ref(W0.reshape(M * C, nA), fold[0].reshape(M * C, nA), fold[1].reshape(M * C, nA),
                                      pr.FIELD_EPS, dt)
        worst = max(worst, report(name, ratio(np.abs(pr.hp(W1.get().reshape(M * C, nA)) - want), bound * want)))
        assert worst <= 1. and np.array_equal(We1.get(), tref.expand(W1.get(), gname)), name
    print(f'pointwise group_apply {dt}: the bits of the unfused chain; W against the reference: largest error / bound '
          f'{worst:.3f}')


class Handles:
    """Operator handles on the shared context, destroyed on exit."""

    def __enter__(self):
        self.made = []
        return self

    def create(self, A, T, entries):
        lib, ctx = context()
        ci = ctypes.c_int
        t, o, i, w = pr.table_arrays(entries)
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (t, o, i)]
        h = ctypes.c_void_p()
        _lib.check(lib.tnmf_hip_atom_ops_create(ctx, len(A), (ci * 3)(*A), T, len(w),
                                                *[a.ctypes.data_as(ctypes.POINTER(ci)) for a in arrs],
                                                w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(h)),
                   'tnmf_hip_atom_ops_create')
        self.made.append(h)
        return h

    def __exit__(self, *exc):
        for h in self.made:
            context()[0].tnmf_hip_atom_ops_destroy(h)
        return False


@pytest.mark.parametrize('dt', pd.DTYPES)
def test_ops_apply_is_fold_apply_expand_to_the_bit_on_both_sides_of_the_staging_rule(dt):
    lib, ctx = context()
    worst, staged_seen = 0., set()
    with Handles() as hs:
        for name, c in cases('ops_apply', dt):
            M, C, A = c['M'], c['C'], c['A']
            T, entries = pd.table_of(c)
            nA = pd.n_pixels(A)
            staged = pd.is_staged(nA, T, dt)
            staged_seen.add((staged, pd.staged_bytes(nA, T, dt)))
            h = hs.create(A, T, entries)
            rng = np.random.default_rng(nA + M)
            W0 = pr.T_(rng.random((M, C) + A) + 0.1, dt)
            X0 = gradient_of(rng, M, T, C, A, dt)
            g = ctypes.byref(dict_geom(M, C, A, dt))
            W1, We1, X = Buf(W0, dt), Buf.out((M * T, C) + A, dt), Buf(X0, dt)
            rc = lib.tnmf_hip_ops_apply_W(ctx, g, h, W1.ptr, We1.ptr, X.ptr, pr.FIELD_EPS, None)
            assert rc == 0, (name, 'staged' if staged else 'not staged', pd.staged_bytes(nA, T, dt), rc)
            W2, F2, We2 = Buf(W0, dt), Buf.out((2, M, C) + A, dt), Buf.out((M * T, C) + A, dt)
            assert lib.tnmf_hip_ops_fold_grad_W(ctx, g, h, X.ptr, F2.ptr, None) == 0
            assert lib.tnmf_hip_apply_W(ctx, g, W2.ptr, F2.ptr, pr.FIELD_EPS, None) == 0
            assert lib.tnmf_hip_ops_expand_W(ctx, g, h, W2.ptr, We2.ptr, None) == 0
            sync()
            assert X.unchanged() and W1.written() and We1.margins_ok() and W2.written() and We2.margins_ok(), name
            assert F2.written(), name
            assert W1.get().tobytes() == W2.get().tobytes() and We1.get().tobytes() == We2.get().tobytes(), name
            fold = np.stack([pr.ops_fold_ref(X0[h_], T, entries, dt) for h_ in (0, 1)])
            fold_eps = np.stack([fold[0], (fold[1] + NP[dt](pr.FIELD_EPS)).astype(NP[dt])])   # (apply_W: pos += eps in place)
            assert F2.get().tobytes() == fold_eps.tobytes(), name
            live = fold[0].reshape(M * C, nA) > 0          # (a pixel no tap reads folds to 0 / eps: W = 0 there, exactly)
            _, want, bound = pr.apply_ref(W0.reshape(M * C, nA), fold[0].reshape(M * C, nA), fold[1].reshape(M * C, nA),
                                          pr.FIELD_EPS, dt)
            got = pr.hp(W1.get().reshape(M * C, nA))
            assert np.all(got[~live] == 0)
            worst = max(worst, report(name, ratio(np.abs(got - want), bound * want)))
            assert worst <= 1., name
            assert We1.get().tobytes() == pr.ops_expand_ref(W1.get(), T, entries, dt).tobytes(), name
    assert (True, 65520) in staged_seen and any(not s for s, _ in staged_seen)
    print(f'pointwise ops_apply {dt}: the bits of the unfused chain, staged (65520 bytes of dynamic LDS accepted) and not; '
          f'W against the reference: largest error / bound {worst:.3f}')


def test_ops_apply_refuses_a_row_beyond_the_staging_and_writes_nothing():
    lib, ctx = context()
    for dt, nA in (('f32', 16385), ('f64', 8193)):
        assert pd.row_refused(nA, dt) and not pd.row_refused(nA - 1, dt)
        with Handles() as hs:
            h = hs.create((nA,), 1, [(0, 0, 0, 1.)])
            W, We, X = Buf(np.ones((1, 1, nA)), dt), Buf.out((1, 1, nA), dt), Buf(np.ones((2, 1, 1, nA)), dt)
            g = ctypes.byref(dict_geom(1, 1, (nA,), dt))
            assert lib.tnmf_hip_ops_apply_W(ctx, g, h, W.ptr, We.ptr, X.ptr, 1e-9, None) == _lib.E_GEOM
            sync()
            assert W.unchanged() and We.unchanged() and X.unchanged()


# -- 3. maps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', pd.DTYPES)
def test_group_expand_and_fold_below_and_above_the_grid_cap(dt):
    lib, ctx = context()
    for name, c in cases('group_map', dt):
        M, C, A, gname = c['M'], c['C'], c['A'], c['group']
        T, gid = pd.GROUP_T[gname], _lib.GROUPS[gname]
        rng = np.random.default_rng(M + A[0])
        W0 = pr.T_(rng.random((M, C) + A) + 0.1, dt)
        X0 = gradient_of(rng, M, T, C, A, dt)
        g = ctypes.byref(dict_geom(M, C, A, dt))
        W, We, X, F = Buf(W0, dt), Buf.out((M * T, C) + A, dt), Buf(X0, dt), Buf.out((2, M, C) + A, dt)
        assert lib.tnmf_hip_group_expand_W(ctx, g, gid, W.ptr, We.ptr, None) == 0, name
        assert lib.tnmf_hip_group_fold_grad_W(ctx, g, gid, X.ptr, F.ptr, None) == 0, name
        sync()
        assert W.unchanged() and X.unchanged() and We.written() and F.written(), name
        assert We.get().tobytes() == np.ascontiguousarray(tref.expand(W0, gname)).tobytes(), name   # a permutation
        want = np.stack([tref.fold(X0[h].astype(np.float64), gname) for h in (0, 1)]).astype(NP[dt])
        assert F.get().tobytes() == want.tobytes(), name                                            # rounded once
    print(f'pointwise group expand / fold {dt}: the same bits, below and above the cap of {pd.MAP_CAP} blocks')


@pytest.mark.parametrize('dt', pd.DTYPES)
def test_ops_expand_and_fold_with_rows_of_every_length(dt):
    lib, ctx = context()
    with Handles() as hs:
        for name, c in cases('ops_map', dt):
            M, C, A = c['M'], c['C'], c['A']
            T, entries = pd.table_of(c)
            nA = pd.n_pixels(A)
            if c['table'] == 'hand':
                fwd, adj = pd.row_lengths(T, entries, nA)
                assert set(fwd) >= set(pd.TAPS) and set(adj) >= set(pd.TAPS)
            h = hs.create(A, T, entries)
            rng = np.random.default_rng(M + A[0])
            W0 = pr.T_(rng.random((M, C) + A) + 0.1, dt)
            X0 = gradient_of(rng, M, T, C, A, dt)
            g = ctypes.byref(dict_geom(M, C, A, dt))
            W, We, X, F = Buf(W0, dt), Buf.out((M * T, C) + A, dt), Buf(X0, dt), Buf.out((2, M, C) + A, dt)
            assert lib.tnmf_hip_ops_expand_W(ctx, g, h, W.ptr, We.ptr, None) == 0, name
            assert lib.tnmf_hip_ops_fold_grad_W(ctx, g, h, X.ptr, F.ptr, None) == 0, name
            sync()
            assert W.unchanged() and X.unchanged() and We.margins_ok() and F.margins_ok(), name
            assert We.get().tobytes() == pr.ops_expand_ref(W0, T, entries, dt).tobytes(), name
            want = np.stack([pr.ops_fold_ref(X0[h_], T, entries, dt) for h_ in (0, 1)])
            assert F.get().tobytes() == want.tobytes(), name
            if M <= 10:    # and the dense matrices of tests/operator_reference.py: k + 1 roundings behind a row of k taps
                L = pr.dense_of(T, entries, nA)
                fwd, adj = pd.row_lengths(T, entries, nA)
                u = pr.U[dt] + (max(fwd + adj) + 1) * pr.U53
                dWe, dF = oref.expand(W0, L), np.stack([oref.fold(X0[h_], L) for h_ in (0, 1)])
                assert np.all(np.abs(We.get() - dWe) <= u * dWe) and np.all(np.abs(F.get() - dF) <= u * dF), name
    print(f'pointwise ops expand / fold {dt}: the float64 ordered sums rounded once, rows of {pd.TAPS} taps in both tables')


# -- 4. energies ------------------------------------------------------------------------------------------------------------------
def problem(dt, N, L):
    """-> (geom, W, H on the device, R = the library's reconstruction on the host; two calls, the same bits)."""
    lib, ctx = context()
    g = _lib.make_geom(N, 1, 1, (L,), (2,), CODE[dt])
    W = Buf(np.array(pr.RECON_W).reshape(1, 1, 2), dt)
    H = Buf(pr.activations(dt, N, L), dt)
    R1, R2 = Buf.out((N, 1, L), dt), Buf.out((N, 1, L), dt)
    assert lib.tnmf_hip_reconstruct(ctx, ctypes.byref(g), W.ptr, H.ptr, R1.ptr, None) == 0
    assert lib.tnmf_hip_reconstruct(ctx, ctypes.byref(g), W.ptr, H.ptr, R2.ptr, None) == 0
    sync()
    assert R1.written() and R2.written() and R1.get().tobytes() == R2.get().tobytes() and W.unchanged() and H.unchanged()
    R = R1.get()
    assert np.all(np.abs(R - pr.reconstruct_T(H.host, dt)) <= 4 * pr.U[dt] * np.abs(R).max())
    return g, W, H, R


def energy_call(g, W, H, V, G, beta, weighted):
    lib, ctx = context()
    out = ctypes.c_double(PATTERN)
    gp = ctypes.byref(g)
    if weighted:
        rc = lib.tnmf_hip_energy_weighted(ctx, gp, beta, pr.ENERGY_EPS, V.ptr, G.ptr, W.ptr, H.ptr, ctypes.byref(out), None)
    elif beta == 2.:
        rc = lib.tnmf_hip_energy(ctx, gp, V.ptr, W.ptr, H.ptr, ctypes.byref(out), None)
    else:
        rc = lib.tnmf_hip_energy_beta(ctx, gp, beta, pr.ENERGY_EPS, V.ptr, W.ptr, H.ptr, ctypes.byref(out), None)
    assert rc == 0
    return out.value


@pytest.mark.parametrize('dt', pd.DTYPES)
@pytest.mark.parametrize('n', pd.ENERGY_N, ids=pd.ENERGY_N_IDS)
def test_energies(n, dt):
    n = pd.size(n, num_cu())
    g, W, H, R = problem(dt, 1, n)
    worst = {}
    for name, c in cases('energy', dt):
        if pd.size(c['n'], num_cu()) != n:
            continue
        beta, weighted = c['beta'], c['weighted']
        Vh, Gh = pr.samples_of(R, dt, beta, weighted)
        V, G = Buf(Vh, dt), (Buf(Gh, dt) if weighted else None)
        want, bound = pr.reduced_ref(Vh, Gh, R, beta, pr.ENERGY_EPS, dt, pd.chain(c, num_cu()))
        got = energy_call(g, W, H, V, G, beta, weighted)
        assert V.unchanged() and (G is None or G.unchanged()) and W.unchanged() and H.unchanged(), name
        assert np.isfinite(got) and want > 0, name
        key = f'K{pd.K_of(beta)}{"w" if weighted else ""}'
        worst[key] = max(worst.get(key, 0.), abs(got - want) / bound)
        print(f'pointwise energy {name}: {got:.17g} against {want:.17g}, error / bound {abs(got - want) / bound:.3f}')
    assert len(worst) == 8 and max(worst.values()) <= 1., worst
    print(f'pointwise energies {dt} n={n}: largest error / bound per kernel instance {worst}')


# -- 5. the objective of every sample -----------------------------------------------------------------------------------------------
def objective_call(g, W, H, V, G, beta, N):
    lib, ctx = context()
    out = Buf.out(N)
    rc = lib.tnmf_hip_sample_objective(ctx, ctypes.byref(g), beta, pr.ENERGY_EPS, V.ptr, G.ptr if G else None, W.ptr, H.ptr,
                                       out.ptr, None)
    sync()
    assert rc == 0 and out.written()
    return out.get()


OBJECTIVE_CASES = [(b, w) for b in pd.OBJECTIVE_BETAS for w in (False, True)]
OBJECTIVE_IDS = [f'beta{b}-{"weighted" if w else "plain"}' for b, w in OBJECTIVE_CASES]


@pytest.mark.parametrize('dt', pd.DTYPES)
@pytest.mark.parametrize('beta,weighted', OBJECTIVE_CASES, ids=OBJECTIVE_IDS)
def test_sample_objective(beta, weighted, dt):
    worst = worst_sum = 0.
    for name, c in cases('objective', dt, beta=beta, weighted=weighted):
        N, L, off = c['N'], c['L'], c['offsets']
        g, W, H, R = problem(dt, N, L)
        Vh, Gh = pr.samples_of(R, dt, beta, weighted)
        V, G = Buf(Vh, dt, off[0]), (Buf(Gh, dt, off[1]) if weighted else None)
        got = objective_call(g, W, H, V, G, beta, N)
        assert V.unchanged() and (G is None or G.unchanged()) and W.unchanged() and H.unchanged(), name
        chain = pd.chain(c, num_cu())
        refs = [pr.reduced_ref(Vh[n], None if Gh is None else Gh[n], R[n], beta, pr.ENERGY_EPS, dt, chain) for n in range(N)]
        want, bound = np.array([r[0] for r in refs]), np.array([r[1] for r in refs])
        worst = max(worst, report(name, ratio(np.abs(got - want), bound)))
        # the samples add up to the energy, within the two bounds
        e_case = dict(kind='energy', dt=dt, n=N * L, beta=beta, weighted=weighted)
        e_want, e_bound = pr.reduced_ref(Vh, Gh, R, beta, pr.ENERGY_EPS, dt, pd.chain(e_case, num_cu()))
        if off == (0, 0):
            E = energy_call(g, W, H, V, G, beta, weighted)
            total = pr.fsum(got)
            worst_sum = max(worst_sum, abs(total - E) / (e_bound + pr.fsum(bound)))
        assert worst <= 1. and worst_sum <= 1., (name, worst, worst_sum)
        if off != (0, 0):     # whole vectors behind a base one element off: the scalar path gives the same bits
            V0, G0 = Buf(Vh, dt), (Buf(Gh, dt) if weighted else None)
            assert pd.is_vec((0, 0), dt, L) and not pd.is_vec(off, dt, L)
            assert objective_call(g, W, H, V0, G0, beta, N).tobytes() == got.tobytes(), name
    print(f'pointwise sample objective {dt} beta={beta} {"weighted" if weighted else "plain"}: largest error / bound '
          f'{worst:.3f}, the samples\' sum against the energy {worst_sum:.3f}')


@pytest.mark.parametrize('dt', pd.DTYPES)
@pytest.mark.parametrize('L', [4096, 4097, 8193])
def test_a_sample_does_not_depend_on_its_company(L, dt):
    for beta, weighted in ((2., False), (1., True), (0.5, False)):
        g3, W, H3, R = problem(dt, 3, L)
        Vh, Gh = pr.samples_of(R, dt, beta, weighted)
        three = objective_call(g3, W, H3, Buf(Vh, dt), Buf(Gh, dt) if weighted else None, beta, 3)
        g1 = _lib.make_geom(1, 1, 1, (L,), (2,), CODE[dt])
        alone = objective_call(g1, W, Buf(H3.host[1:2], dt), Buf(Vh[1:2], dt), Buf(Gh[1:2], dt) if weighted else None, beta, 1)
        assert alone.tobytes() == three[1:2].tobytes(), (L, beta, weighted)


@pytest.mark.parametrize('dt', pd.DTYPES)
@pytest.mark.parametrize('beta,weighted', [(2., False), (1., True)], ids=['frobenius', 'weighted-kl'])
def test_the_tap_takes_the_same_route(beta, weighted, dt):
    lib, ctx = context()
    N, L = 3, 4097
    g, W, H, R = problem(dt, N, L)
    Vh, Gh = pr.samples_of(R, dt, beta, weighted)
    V, G = Buf(Vh, dt), (Buf(Gh, dt) if weighted else None)
    direct = objective_call(g, W, H, V, G, beta, N)
    tap = Buf.out(N)
    gp = ctypes.byref(g)
    assert lib.tnmf_hip_ctx_set_objective_tap(ctx, tap.ptr) == 0
    try:
        if weighted:
            no = ctypes.POINTER(ctypes.c_double)()
            rc = lib.tnmf_hip_update_H_weighted(ctx, gp, _lib.MODES['valid'], V.ptr, G.ptr, W.ptr, H.ptr, None, pr.ENERGY_EPS,
                                                0., 0., 0., no, 0, no, 0, no, 0, beta, None)
        else:
            rc = lib.tnmf_hip_update_H(ctx, gp, V.ptr, W.ptr, H.ptr, None, 0, pr.ENERGY_EPS, 0., None)
        sync()
    finally:
        lib.tnmf_hip_ctx_set_objective_tap(ctx, None)
    assert rc == 0 and tap.written() and H.margins_ok() and H.get().tobytes() != H.host.tobytes()
    assert V.unchanged() and (G is None or G.unchanged()) and W.unchanged()
    assert tap.get().tobytes() == direct.tobytes()
