"""Atom operators on the GPU (tnmf_hip_atom_ops_* and tnmf_hip_ops_expand_W / _fold_grad_W / _apply_W, and
TransformInvariantNMF(..., transforms=AtomOperators)) against the float64 dense reference of tests/operator_reference.py
and, for operator tables of the permutation groups, against the group entry points bit for bit."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import beta_reference as bref
import operator_reference as oref
from local_collective import run_ranks
from oracle import tnmf_oracle as orc
from tnmf_amd import _lib, transforms as tr
from tnmf_amd.TransformInvariantNMF import MiniBatchAlgorithm, TransformInvariantNMF

pytestmark = pytest.mark.gpu

bref.IMPL = 'c'
CB = lambda *_: True  # noqa: E731  (a progress callback: no per-iteration energy through the logger)
GROUPS = ['flip', 'mirrors', 'rot90', 'dihedral']


def relmax(got, want):
    want = np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max()
    return np.abs(np.asarray(got, dtype=np.float64) - want).max() / (scale if scale > 0 else 1.0)


def positive_V(shape, seed, dtype=np.float64):
    return (np.random.default_rng(seed).random(shape) + 0.05).astype(dtype)


def p(t):
    return ctypes.c_void_p(t.data_ptr())


class Ctx:
    """A library context and the operator handles made on it (destroyed before the context)."""

    def __enter__(self):
        self.lib = _lib.load()
        self.ctx = ctypes.c_void_p()
        self.handles = []
        _lib.check(self.lib.tnmf_hip_ctx_create(torch.cuda.current_device(), ctypes.byref(self.ctx)), 'ctx_create')
        return self

    def create(self, ndim, A, T, t, o, i, w):
        """-> (return code, handle or None)."""
        ci = ctypes.c_int
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (t, o, i)]
        wd = np.ascontiguousarray(w, dtype=np.float64)
        h = ctypes.c_void_p()
        rc = self.lib.tnmf_hip_atom_ops_create(self.ctx, ndim, (ci * 3)(*A), T, len(wd),
                                               *[a.ctypes.data_as(ctypes.POINTER(ci)) for a in arrs],
                                               wd.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(h))
        if rc == 0:
            self.handles.append(h)
        return rc, (h if h.value else None)

    def handle(self, ops):
        rc, h = self.create(len(ops.atom_shape), ops.atom_shape, ops.T, *ops.entries)
        _lib.check(rc, 'tnmf_hip_atom_ops_create')
        return h

    def __exit__(self, *exc):
        for h in self.handles:
            self.lib.tnmf_hip_atom_ops_destroy(h)
        self.lib.tnmf_hip_ctx_destroy(self.ctx)
        return False


def dict_geom(M, C, A, dtype):
    D = tuple(2 * a for a in A)    # (not read by the operator entry points)
    return _lib.make_geom(0, M, C, D, A, 0 if dtype == np.float32 else 1)


def random_ops(A, T, density, seed):
    rng = np.random.default_rng(seed)
    L = rng.random((T,) + tuple(A) * 2) * (rng.random((T,) + tuple(A) * 2) < density)
    return tr.AtomOperators.from_dense(L)


# -- 1. the kernels -------------------------------------------------------------------------------------------------
KERNEL_OPS = {
    'rot8_5x5': lambda: tr.rotations((5, 5), 8),
    'rot6_4x7': lambda: tr.rotations((4, 7), 6),
    'compose_6x6': lambda: tr.compose(tr.rotations((6, 6), 4), tr.scales((6, 6), [1., .7, 1.4])),
    'scales_1d': lambda: tr.scales((9,), [1., .6, .3, 1.5]),
    'dense_1d': lambda: random_ops((8,), 3, 0.3, 1),
    'dense_2d': lambda: random_ops((3, 5), 2, 0.2, 2),
    # (float64: the [neg | pos] slice of a row does not fit the fused update's LDS -- it folds from global memory)
    'rot32_12x12': lambda: tr.rotations((12, 12), 32),
}


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('name', list(KERNEL_OPS))
def test_kernels_expand_fold_and_fused_apply(name, dtype, C):
    ops = KERNEL_OPS[name]()
    A, T, M = ops.atom_shape, ops.T, 3
    rng = np.random.default_rng(len(A) * 100 + A[-1] + C)
    W = (rng.random((M, C) + A) + 0.1).astype(dtype)
    W /= W.sum(axis=tuple(range(-len(A), 0)), keepdims=True)
    X = (rng.random((2, M * T, C) + A) + 0.05).astype(dtype)
    g = dict_geom(M, C, A, dtype)
    with Ctx() as c:
        h = c.handle(ops)
        tW = torch.from_numpy(W).cuda()
        tWe = torch.full((M * T, C) + A, -1., dtype=tW.dtype, device='cuda')
        _lib.check(c.lib.tnmf_hip_ops_expand_W(c.ctx, ctypes.byref(g), h, p(tW), p(tWe), None), 'expand')
        assert np.array_equal(tWe.cpu().numpy(), tr.expand(W, ops))          # the float64 sums, rounded once
        assert relmax(tWe.cpu().numpy(), oref.expand(W, oref.dense(ops))) < (1e-15 if dtype == np.float64 else 1e-7)

        tX = torch.from_numpy(X).cuda()
        tF = torch.full((2, M, C) + A, -1., dtype=tW.dtype, device='cuda')
        _lib.check(c.lib.tnmf_hip_ops_fold_grad_W(c.ctx, ctypes.byref(g), h, p(tX), p(tF), None), 'fold')
        want = np.stack([tr.fold(X[0], ops), tr.fold(X[1], ops)])
        assert np.array_equal(tF.cpu().numpy(), want)

        eps = 1e-9
        W1, We1 = tW.clone(), torch.empty_like(tWe)
        _lib.check(c.lib.tnmf_hip_ops_apply_W(c.ctx, ctypes.byref(g), h, p(W1), p(We1), p(tX), eps, None), 'ops_apply')
        W2, F2, We2 = tW.clone(), torch.empty_like(tF), torch.empty_like(tWe)
        _lib.check(c.lib.tnmf_hip_ops_fold_grad_W(c.ctx, ctypes.byref(g), h, p(tX), p(F2), None), 'fold')
        _lib.check(c.lib.tnmf_hip_apply_W(c.ctx, ctypes.byref(g), p(W2), p(F2), eps, None), 'apply_W')
        _lib.check(c.lib.tnmf_hip_ops_expand_W(c.ctx, ctypes.byref(g), h, p(W2), p(We2), None), 'expand')
        assert torch.equal(W1, W2) and torch.equal(We1, We2)
        assert torch.equal(tX, torch.from_numpy(X).cuda())                  # negpos_eff is only read
        Wref = W.astype(np.float64)
        L = oref.dense(ops)
        orc.multiplicative_update(Wref, oref.fold(X[0], L), oref.fold(X[1], L), eps,
                                  normalization_axes=tuple(range(-len(A), 0)))
        assert relmax(W1.cpu().numpy(), Wref) < (1e-14 if dtype == np.float64 else 1e-6)


GROUP_CASES = [(n, A) for n in GROUPS for A in ((5, 5), (4, 4))] + [('flip', (9,)), ('mirrors', (3, 6))]


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('name,A', GROUP_CASES, ids=[f'{n}_{"x".join(map(str, A))}' for n, A in GROUP_CASES])
def test_group_tables_give_the_group_bits(name, A, dtype):
    ops = tr.from_group(name, A)
    M, C, T = 3, 2, ops.T
    rng = np.random.default_rng(7)
    W = (rng.random((M, C) + A) + 0.1).astype(dtype)
    X = (rng.random((2, M * T, C) + A) + 0.05).astype(dtype)
    g = dict_geom(M, C, A, dtype)
    gid = _lib.GROUPS[name]
    with Ctx() as c:
        h = c.handle(ops)
        tW, tX = torch.from_numpy(W).cuda(), torch.from_numpy(X).cuda()
        out = []
        for kind, arg in (('group', gid), ('ops', h)):
            We = torch.empty((M * T, C) + A, dtype=tW.dtype, device='cuda')
            F = torch.empty((2, M, C) + A, dtype=tW.dtype, device='cuda')
            W1, We1 = tW.clone(), torch.empty_like(We)
            gp = ctypes.byref(g)
            _lib.check(getattr(c.lib, f'tnmf_hip_{kind}_expand_W')(c.ctx, gp, arg, p(tW), p(We), None), kind)
            _lib.check(getattr(c.lib, f'tnmf_hip_{kind}_fold_grad_W')(c.ctx, gp, arg, p(tX), p(F), None), kind)
            _lib.check(getattr(c.lib, f'tnmf_hip_{kind}_apply_W')(c.ctx, gp, arg, p(W1), p(We1), p(tX), 1e-9, None),
                       kind)
            out.append((We, F, W1, We1))
        for a, b in zip(*out):
            assert torch.equal(a, b)


def test_refusals_leave_the_outputs_untouched():
    with Ctx() as c:
        ops = tr.rotations((4, 4), 4)
        h = c.handle(ops)
        # the handle: refused entries, and *out stays NULL
        one = ([0], [0], [0], [1.])
        cases = [((3, (4, 4, 4), 1) + one, _lib.E_UNSUPPORTED),                      # a volume
                 ((0, (4, 4, 0), 1) + one, -2), ((2, (4, 0, 0), 1) + one, -2),         # ndim, sizes
                 ((2, (4, 4, 0), 0) + one, -2),                                        # T
                 ((2, (4, 4, 0), 1, [1], [0], [0], [1.]), -2),                         # t out of range
                 ((2, (4, 4, 0), 1, [0], [16], [0], [1.]), -2),                        # out pixel out of range
                 ((2, (4, 4, 0), 1, [0], [0], [-1], [1.]), -2),                        # in pixel out of range
                 ((2, (4, 4, 0), 1, [0, 0], [3, 3], [2, 2], [1., 1.]), -2),            # a duplicate
                 ((2, (4, 4, 0), 1, [0], [0], [0], [-1.]), _lib.E_UNSUPPORTED),        # a negative weight
                 ((2, (4, 4, 0), 1, [0], [0], [0], [np.nan]), _lib.E_UNSUPPORTED),
                 ((2, (4, 4, 0), 1, [0], [0], [0], [np.inf]), _lib.E_UNSUPPORTED)]
        for args, code in cases:
            rc, made = c.create(*args)
            assert rc == code and made is None, (args, rc)
        assert c.lib.tnmf_hip_atom_ops_create(c.ctx, 2, (ctypes.c_int * 3)(4, 4, 0), 1, 0, None, None, None, None,
                                              None) == -1
        assert c.lib.tnmf_hip_atom_ops_destroy(None) == 0

        W = torch.rand((2, 1, 4, 4), dtype=torch.float64, device='cuda')
        We = torch.full((8, 1, 4, 4), 7., dtype=torch.float64, device='cuda')
        F = torch.full((2, 2, 1, 4, 4), 7., dtype=torch.float64, device='cuda')
        X = torch.rand((2, 8, 1, 4, 4), dtype=torch.float64, device='cuda')
        W0 = W.clone()
        with Ctx() as other:
            foreign = other.handle(ops)
            calls = [(dict_geom(2, 1, (4, 5), np.float64), h, -2),                    # atom shape of another handle
                     (dict_geom(2, 1, (16,), np.float64), h, -2),                      # ndim likewise
                     (_lib.make_geom(0, 2, 1, (6, 6, 6), (4, 4, 4), 1), h, _lib.E_UNSUPPORTED),   # a volume
                     (dict_geom(2, 1, (4, 4), np.float64), None, -1),                   # no handle
                     (dict_geom(2, 1, (4, 4), np.float64), foreign, _lib.E_UNSUPPORTED)]  # another context's handle
            for g, handle, code in calls:
                gp = ctypes.byref(g)
                assert c.lib.tnmf_hip_ops_expand_W(c.ctx, gp, handle, p(W), p(We), None) == code
                assert c.lib.tnmf_hip_ops_fold_grad_W(c.ctx, gp, handle, p(X), p(F), None) == code
                assert c.lib.tnmf_hip_ops_apply_W(c.ctx, gp, handle, p(W), p(We), p(X), 1e-9, None) == code
        g = dict_geom(2, 1, (4, 4), np.float64)
        assert c.lib.tnmf_hip_ops_expand_W(c.ctx, ctypes.byref(g), h, None, p(We), None) == -1
        assert c.lib.tnmf_hip_ops_apply_W(c.ctx, ctypes.byref(g), h, p(W), p(We), None, 1e-9, None) == -1
        torch.cuda.synchronize()
        assert bool(torch.all(We == 7.)) and bool(torch.all(F == 7.)) and torch.equal(W, W0)


# -- 2. the half steps against the reference --------------------------------------------------------------------------
def half_steps(V, M, A, ops, path, mode='valid', sparsity=0., inhibition=0., cross=0.):
    """One H half step, then one W half step (from the GPU's H) -> (dH, dW) against the reference."""
    nmf = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip', transforms=ops, path=path,
                                reconstruction_mode=mode)
    np.random.seed(7)
    nmf._initialize_matrices(V, False)
    ref = oref.OperatorOracleNMF(n_atoms=M, atom_shape=A, ops=ops, impl='c', reconstruction_mode=mode,
                                 inhibition_range=None)
    ref._kernels = nmf._inhibition_kernels_1D
    ref.V, ref.G = V.astype(np.float64), np.ones(V.shape)
    ref.W = nmf.W.astype(np.float64)
    ref.W_eff = oref.expand(ref.W, ref.L)
    N = V.shape[0]
    ref.H = nmf.H.astype(np.float64).reshape((N, M * ops.T) + nmf.H.shape[3:])
    nmf._update_H(sparsity=sparsity, inhibition=inhibition, cross_inhibition=cross)
    ref.update_H(sparsity=sparsity, inhibition=inhibition, cross_inhibition=cross)
    dH = relmax(nmf.H.reshape(ref.H.shape), ref.H)
    ref.H = nmf.H.astype(np.float64).reshape(ref.H.shape)
    nmf._update_W()
    ref.update_W()
    assert np.array_equal(nmf.transformed_atoms.reshape(ref.W_eff.shape), tr.expand(nmf.W, ops))
    return dH, relmax(nmf.W, ref.W), nmf


PATH_CASES = ([(np.float64, p_) for p_ in ('generic', 'fft', 'hybrid', 'auto')]
              + [(np.float32, p_) for p_ in ('generic', 'mfma', 'split', 'hybrid', 'auto', 'fft')])


@pytest.mark.parametrize('dtype,path', PATH_CASES, ids=[f'{np.dtype(d).name}_{p_}' for d, p_ in PATH_CASES])
def test_operator_half_steps_on_every_path(dtype, path):
    """rotations(9x9, 8) with 8 atoms: 64 effective atoms."""
    V = positive_V((3, 1, 48, 48), seed=1, dtype=dtype)
    dH, dW, nmf = half_steps(V, 8, (9, 9), tr.rotations((9, 9), 8), path, sparsity=0.05)
    assert nmf._H.shape[1] == 64
    tol = 1e-10 if dtype == np.float64 else 2e-5
    assert dW < tol, dW
    if not (dtype == np.float32 and path == 'fft'):   # (float32 FFT is a W-only path, include/tnmf_hip.h)
        assert dH < tol, dH


@pytest.mark.parametrize('lateral', [False, True], ids=['plain', 'inhibition'])
@pytest.mark.parametrize('mode', ['valid', 'full', 'circular', 'reflect'])
@pytest.mark.parametrize('dtype,path', [(np.float64, 'generic'), (np.float64, 'auto'), (np.float32, 'auto')],
                         ids=['f64_generic', 'f64_auto', 'f32_auto'])
def test_operator_half_steps_modes_and_lateral_terms(dtype, path, mode, lateral):
    V = positive_V((3, 2, 20, 24), seed=2, dtype=dtype)
    ops = tr.compose(tr.rotations((4, 5), 3), tr.scales((4, 5), [1., .7]))
    kw = dict(sparsity=0.05, inhibition=0.1, cross=0.05) if lateral else {}
    dH, dW, _ = half_steps(V, 3, (4, 5), ops, path, mode=mode, **kw)
    tol = 1e-10 if dtype == np.float64 else 2e-5
    assert dH < tol and dW < tol, (dH, dW)


# -- 3. fits against the reference ------------------------------------------------------------------------------------
FIT_CASES = {
    'scales_1d': ((6,), (4, 2, 40), lambda: tr.scales((6,), [1., .7, 1.4])),
    'rot8_2d': ((6, 6), (4, 1, 30, 32), lambda: tr.rotations((6, 6), 8)),
    'compose_2d': ((5, 4), (4, 2, 30, 32), lambda: tr.compose(tr.rotations((5, 4), 4), tr.scales((5, 4), [1., .6]))),
}


def reference_fit(V, M, A, ops, seed=42, beta=2., weights=None, **kw):
    np.random.seed(seed)
    return oref.OperatorOracleNMF(n_atoms=M, atom_shape=A, ops=ops, impl='c', beta=beta,
                                  weights=weights).fit(V.astype(np.float64), **kw)


def check_fit(nmf, ref, tol=1e-10):
    assert relmax(nmf.W, ref.W) < tol and relmax(nmf.H, ref.H4) < tol, (relmax(nmf.W, ref.W), relmax(nmf.H, ref.H4))
    assert abs(nmf._energy_function() - ref.energy()) < tol * ref.energy()
    assert relmax(nmf.R, ref.R) < tol and relmax(nmf.R_partial(1), ref.R_partial(1)) < tol


@pytest.mark.parametrize('name', list(FIT_CASES))
def test_operator_fit_batch_f64_equals_the_reference(name):
    A, shape, make = FIT_CASES[name]
    ops = make()
    V = positive_V(shape, seed=3)
    kw = dict(n_iterations=4, sparsity_H=0.05, inhibition_strength=0.1, cross_atom_inhibition_strength=0.05)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=A, backend='hip', transforms=ops)
    nmf.fit_batch(V, progress_callback=CB, **kw)
    check_fit(nmf, reference_fit(V, 3, A, ops, **kw))


@pytest.mark.parametrize('beta', [1., 0.])
def test_operator_beta_fits_equal_the_reference(beta):
    V = positive_V((4, 1, 30, 32), seed=5)
    ops = tr.rotations((6, 6), 6)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(6, 6), backend='hip', transforms=ops, beta_loss=beta)
    nmf.fit_batch(V, n_iterations=4, sparsity_H=0.05, progress_callback=CB)
    check_fit(nmf, reference_fit(V, 3, (6, 6), ops, beta=beta, n_iterations=4, sparsity_H=0.05))


@pytest.mark.parametrize('beta', [2., 1.])
def test_operator_weighted_fits_equal_the_reference(beta):
    V = positive_V((4, 1, 30, 32), seed=6)
    rng = np.random.default_rng(6)
    G = rng.random((4, 1, 30, 32)) + 0.5
    G[rng.random(G.shape) < 0.2] = 0.
    V0 = np.where(G == 0, 0., V)
    ops = tr.scales((5, 4), [1., .8, .6])
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(5, 4), backend='hip', transforms=ops, beta_loss=beta)
    nmf.fit_batch(np.where(G == 0, np.nan, V), n_iterations=4, progress_callback=CB, weights=G)
    ref = reference_fit(V0, 3, (5, 4), ops, beta=beta, weights=G, n_iterations=4)
    assert relmax(nmf.W, ref.W) < 1e-10 and relmax(nmf.H, ref.H4) < 1e-10
    assert abs(nmf._energy_function() - ref.energy()) < 1e-10 * ref.energy()


@pytest.mark.parametrize('lateral', [False, True], ids=['plain', 'inhibition'])
@pytest.mark.parametrize('algorithm', list(MiniBatchAlgorithm), ids=[a.name for a in MiniBatchAlgorithm])
def test_operator_epochs_equal_the_reference(algorithm, lateral):
    V = positive_V((7, 2, 20, 24), seed=7)
    ops = tr.rotations((5, 5), 8)
    kw = dict(batch_size=2, n_epochs=3, sparsity_H=0.05)
    if lateral:
        kw.update(inhibition_strength=0.1, cross_atom_inhibition_strength=0.05)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(5, 5), backend='hip', transforms=ops)
    nmf.fit(V, algorithm=algorithm, progress_callback=CB, **kw)
    ref = reference_fit(V, 3, (5, 5), ops, algorithm=orc.MiniBatchAlgorithm(algorithm.value), **kw)
    assert relmax(nmf.W, ref.W) < 1e-10 and relmax(nmf.H, ref.H4) < 1e-10


def test_operator_stream_keeps_W():
    V = positive_V((6, 1, 24, 24), seed=8)
    ops = tr.compose(tr.rotations((5, 5), 4), tr.scales((5, 5), [1., .6]))
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(5, 5), backend='hip', transforms=ops)
    nmf.fit(iter(V), subsample_size=3, n_iterations=3, progress_callback=CB)
    np.random.seed(42)
    ref = oref.OperatorOracleNMF(n_atoms=2, atom_shape=(5, 5), ops=ops, impl='c').fit(
        iter(V), subsample_size=3, n_iterations=3)
    assert relmax(nmf.W, ref.W) < 1e-10 and relmax(nmf.H, ref.H4) < 1e-10


def test_one_handle_per_model_and_context_reused_across_fits():
    V = positive_V((3, 1, 20, 20), seed=9)
    ops = tr.rotations((5, 5), 8)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(5, 5), backend='hip', transforms=ops)
    nmf.fit_batch(V, n_iterations=2, progress_callback=CB)
    handles = dict(nmf._backend._ops_handles)
    assert list(handles) == [ops.key]
    nmf.fit_batch(V, n_iterations=2, progress_callback=CB)
    assert nmf._backend._ops_handles[ops.key][1] is handles[ops.key][1]
    assert len(nmf._backend._ops_handles) == 1


# -- 4. two ranks in one process ------------------------------------------------------------------------------------
_init_lock = threading.Lock()
RANK_OPS = tr.rotations((5, 5), 6)


def _fit(V, mode, pg=None, reduce='all_reduce'):
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(5, 5), backend='hip', process_group=pg, transforms=RANK_OPS,
                                reduce=reduce)
    plain_init = nmf._initialize_matrices

    def seeded_init(V_, keep_W, **kw):
        with _init_lock:
            np.random.seed(42)
            plain_init(V_, keep_W, **kw)

    nmf._initialize_matrices = seeded_init
    if mode == 'batch':
        nmf.fit(V, n_iterations=3, sparsity_H=0.05, progress_callback=CB)
    else:
        nmf.fit(V, algorithm=MiniBatchAlgorithm.Cyclic_MU, batch_size=2, n_epochs=3, sparsity_H=0.05,
                progress_callback=CB)
    return nmf


@pytest.mark.parametrize('reduce', ['all_reduce', 'ordered'])
@pytest.mark.parametrize('mode', ['batch', 'cyclic'])
def test_operator_two_ranks_equal_the_unsharded_run(mode, reduce):
    V = positive_V((7, 2, 20, 24), seed=12)

    def rank_body(rank, coll):
        torch.cuda.set_device(0)
        nmf = _fit(V, mode, coll, reduce=reduce)
        return dict(W=nmf.W, H=nmf.H, E=nmf._energy_function(), Weff=nmf.transformed_atoms)

    (r0, r1), group = run_ranks(2, rank_body)
    assert np.array_equal(r0['W'], r1['W']) and np.array_equal(r0['Weff'], r1['Weff']) and r0['E'] == r1['E']
    single = _fit(V, mode)
    assert relmax(r0['W'], single.W) < 1e-10
    assert relmax(np.concatenate([r0['H'], r1['H']]), single.H) < 1e-10
    assert abs(r0['E'] - single._energy_function()) < 1e-10 * abs(r0['E'])


# -- 5. the spectrum cache: W_eff changes at a fixed address --------------------------------------------------------------
@pytest.mark.parametrize('algorithm', [None, MiniBatchAlgorithm.ASG_MU], ids=['batch', 'ASG_MU'])
def test_operator_iterations_with_the_spectrum_cache_equal_fresh_contexts(algorithm):
    V = positive_V((4, 1, 40, 40), seed=13)
    A = (6, 6)
    ops = tr.rotations(A, 8)
    fit_kw = dict(n_iterations=4) if algorithm is None else dict(algorithm=algorithm, batch_size=2, n_epochs=2)
    out = []
    for fresh in (False, True):
        np.random.seed(42)
        nmf = TransformInvariantNMF(n_atoms=3, atom_shape=A, backend='hip', path='fft', transforms=ops)
        if fresh:
            be = nmf._backend
            for hook in ('fused_update_H', 'fused_update_W_transformed'):
                plain = getattr(be, hook)

                def wrapped(*a, _plain=plain, **k):
                    be._foreign_H()     # (drops the spectra of H, V and the dictionary)
                    return _plain(*a, **k)
                setattr(be, hook, wrapped)
        nmf.fit(V, progress_callback=CB, **fit_kw)
        out.append((nmf.W, nmf.H, nmf._backend.cache_counters))
    (W0, H0, counters), (W1, H1, _) = out
    assert counters['h_hits'] > 0, counters
    assert relmax(W0, W1) < 1e-13 and relmax(H0, H1) < 1e-13, (relmax(W0, W1), relmax(H0, H1))
    ref_kw = dict(fit_kw)
    if algorithm is not None:
        ref_kw['algorithm'] = orc.MiniBatchAlgorithm(algorithm.value)
    ref = reference_fit(V, 3, A, ops, **ref_kw)
    assert relmax(W0, ref.W) < 1e-10 and relmax(H0, ref.H4) < 1e-10


# -- 6. group operators fit exactly like the group ---------------------------------------------------------------------
def test_rot90_operators_and_the_rot90_group_give_identical_fits():
    V = positive_V((12, 1, 96, 96), seed=9, dtype=np.float32)
    out = []
    for transforms in ('rot90', tr.from_group('rot90', (12, 12))):
        np.random.seed(42)
        nmf = TransformInvariantNMF(n_atoms=8, atom_shape=(12, 12), backend='hip', path='auto', transforms=transforms)
        nmf.fit_batch(V, n_iterations=5, progress_callback=CB)
        out.append((nmf.W, nmf.H))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# -- 7. the planted motif at eight angles --------------------------------------------------------------------------------
def test_planted_motif_at_eight_angles_f32():
    """The property tests/test_atom_operators_cpu.py fixes on the reference, on the GPU in float32."""
    P = oref.PLANTED_ANGLES
    V = oref.planted_angles(0).astype(np.float32)
    energies = []
    for transforms in (tr.rotations(P['atom_shape'], P['n_angles']), 'rot90'):
        np.random.seed(42)
        nmf = TransformInvariantNMF(n_atoms=1, atom_shape=P['atom_shape'], backend='hip', transforms=transforms)
        nmf.fit_batch(V, n_iterations=P['iterations'], progress_callback=CB)
        energies.append(nmf._energy_function())
    print(f'planted motif at 8 angles, float32: energy {energies[0]:.3e} rotations(A, 8), {energies[1]:.3e} rot90')
    assert energies[1] >= oref.PLANTED_ANGLES_MARGIN * energies[0], energies
