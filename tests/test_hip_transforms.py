"""Rotation and mirror invariance on the GPU (tnmf_hip_group_expand_W / _fold_grad_W / _apply_W and
TransformInvariantNMF(..., transforms=...)) against the float64 reference of tests/transform_reference.py."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import beta_reference as bref
import transform_reference as tref
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
    def __enter__(self):
        self.lib = _lib.load()
        self.ctx = ctypes.c_void_p()
        _lib.check(self.lib.tnmf_hip_ctx_create(torch.cuda.current_device(), ctypes.byref(self.ctx)), 'ctx_create')
        return self

    def __exit__(self, *exc):
        self.lib.tnmf_hip_ctx_destroy(self.ctx)
        return False


def dict_geom(M, C, A, dtype):
    D = tuple(2 * a for a in A)    # (not read by the group entry points)
    return _lib.make_geom(0, M, C, D, A, 0 if dtype == np.float32 else 1)


# -- 1. the kernels -------------------------------------------------------------------------------------------------
KERNEL_CASES = ([(n, A) for n in GROUPS for A in ((5, 5), (4, 4))] + [(n, (3, 6)) for n in ('flip', 'mirrors')]
                + [('flip', (7,)), ('flip', (8,))])


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('name,A', KERNEL_CASES, ids=[f'{n}_{"x".join(map(str, A))}' for n, A in KERNEL_CASES])
def test_kernels_expand_fold_and_fused_apply(name, A, dtype, C):
    M, T = 3, tr.size(name)
    rng = np.random.default_rng(len(A) * 100 + A[-1] + C)
    W = (rng.random((M, C) + A) + 0.1).astype(dtype)
    W /= W.sum(axis=tuple(range(-len(A), 0)), keepdims=True)
    X = (rng.random((2, M * T, C) + A) + 0.05).astype(dtype)
    g = dict_geom(M, C, A, dtype)
    group = _lib.GROUPS[name]
    with Ctx() as c:
        tW = torch.from_numpy(W).cuda()
        tWe = torch.full((M * T, C) + A, -1., dtype=tW.dtype, device='cuda')
        _lib.check(c.lib.tnmf_hip_group_expand_W(c.ctx, ctypes.byref(g), group, p(tW), p(tWe), None), 'expand')
        assert np.array_equal(tWe.cpu().numpy(), tref.expand(W, name))       # a permutation: bit-exact

        tX = torch.from_numpy(X).cuda()
        tF = torch.full((2, M, C) + A, -1., dtype=tW.dtype, device='cuda')
        _lib.check(c.lib.tnmf_hip_group_fold_grad_W(c.ctx, ctypes.byref(g), group, p(tX), p(tF), None), 'fold')
        want = np.stack([tref.fold(X[0].astype(np.float64), name), tref.fold(X[1].astype(np.float64), name)])
        assert np.array_equal(tF.cpu().numpy(), want.astype(dtype))         # the float64 fold, rounded once

        # fused: fold -> apply_W -> expand in one launch, same bits
        eps = 1e-9
        W1, We1 = tW.clone(), torch.empty_like(tWe)
        _lib.check(c.lib.tnmf_hip_group_apply_W(c.ctx, ctypes.byref(g), group, p(W1), p(We1), p(tX), eps, None),
                   'group_apply')
        W2, F2, We2 = tW.clone(), torch.empty_like(tF), torch.empty_like(tWe)
        _lib.check(c.lib.tnmf_hip_group_fold_grad_W(c.ctx, ctypes.byref(g), group, p(tX), p(F2), None), 'fold')
        _lib.check(c.lib.tnmf_hip_apply_W(c.ctx, ctypes.byref(g), p(W2), p(F2), eps, None), 'apply_W')
        _lib.check(c.lib.tnmf_hip_group_expand_W(c.ctx, ctypes.byref(g), group, p(W2), p(We2), None), 'expand')
        assert torch.equal(W1, W2) and torch.equal(We1, We2)
        assert torch.equal(tX, torch.from_numpy(X).cuda())                  # negpos_eff is only read
        Wref = W.astype(np.float64)
        orc.multiplicative_update(Wref, want[0], want[1].copy(), eps, normalization_axes=tuple(range(-len(A), 0)))
        assert relmax(W1.cpu().numpy(), Wref) < (1e-14 if dtype == np.float64 else 1e-6)


def test_kernels_refuse_what_they_do_not_cover_untouched():
    with Ctx() as c:
        W = torch.rand((2, 1, 4, 4), dtype=torch.float64, device='cuda')
        We = torch.full((16, 1, 4, 4), 7., dtype=torch.float64, device='cuda')
        F = torch.full((2, 2, 1, 4, 4), 7., dtype=torch.float64, device='cuda')
        X = torch.rand((2, 16, 1, 4, 4), dtype=torch.float64, device='cuda')
        cases = [(_lib.make_geom(0, 2, 1, (6, 6, 6), (4, 4, 4), 1), 0),       # volume
                 (dict_geom(2, 1, (4, 4), np.float64), -1),                    # unknown group ids
                 (dict_geom(2, 1, (4, 4), np.float64), 4),
                 (dict_geom(2, 1, (16,), np.float64), _lib.GROUPS['mirrors']),  # a 2-axis group on one axis
                 (dict_geom(2, 1, (16,), np.float64), _lib.GROUPS['rot90']),
                 (dict_geom(2, 1, (2, 8), np.float64), _lib.GROUPS['rot90']),   # rotations of non-square atoms
                 (dict_geom(2, 1, (2, 8), np.float64), _lib.GROUPS['dihedral'])]
        for g, group in cases:
            gp = ctypes.byref(g)
            assert c.lib.tnmf_hip_group_expand_W(c.ctx, gp, group, p(W), p(We), None) == _lib.E_UNSUPPORTED
            assert c.lib.tnmf_hip_group_fold_grad_W(c.ctx, gp, group, p(X), p(F), None) == _lib.E_UNSUPPORTED
            assert c.lib.tnmf_hip_group_apply_W(c.ctx, gp, group, p(W), p(We), p(X), 1e-9, None) == _lib.E_UNSUPPORTED
        g = dict_geom(2, 1, (4, 4), np.float64)
        assert c.lib.tnmf_hip_group_expand_W(c.ctx, ctypes.byref(g), 2, None, p(We), None) == -1
        torch.cuda.synchronize()
        assert bool(torch.all(We == 7.)) and bool(torch.all(F == 7.))


# -- 2. the half steps against the reference --------------------------------------------------------------------------
def model(V, M, A, name, seed=7, beta=2., **kw):
    nmf = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip', transforms=name, beta_loss=beta, **kw)
    np.random.seed(seed)
    nmf._initialize_matrices(V, False)
    return nmf


def half_steps(V, M, A, name, path, mode='valid', sparsity=0., inhibition=0., cross=0.):
    """One H half step, then one W half step (from the GPU's H) -> (dH, dW) against the reference."""
    nmf = model(V, M, A, name, path=path, reconstruction_mode=mode)
    ref = tref.TransformOracleNMF(n_atoms=M, atom_shape=A, transforms=name, impl='c', reconstruction_mode=mode,
                                  inhibition_range=None)
    ref._kernels = nmf._inhibition_kernels_1D
    ref.V, ref.G = V.astype(np.float64), np.ones(V.shape)
    ref.W = nmf.W.astype(np.float64)
    ref.W_eff = tref.expand(ref.W, name)
    assert np.array_equal(nmf.transformed_atoms.reshape(ref.W_eff.shape), tref.expand(nmf.W, name))
    N = V.shape[0]
    ref.H = nmf.H.astype(np.float64).reshape((N, M * ref.T) + nmf.H.shape[3:])
    nmf._update_H(sparsity=sparsity, inhibition=inhibition, cross_inhibition=cross)
    ref.update_H(sparsity=sparsity, inhibition=inhibition, cross_inhibition=cross)
    dH = relmax(nmf.H.reshape(ref.H.shape), ref.H)
    ref.H = nmf.H.astype(np.float64).reshape(ref.H.shape)
    nmf._update_W()
    ref.update_W()
    assert np.array_equal(nmf.transformed_atoms.reshape(ref.W_eff.shape), tref.expand(nmf.W, name))
    return dH, relmax(nmf.W, ref.W), nmf


# (mfma and split are float32 kernel families: they run in float32 at the float32 bar)
PATH_CASES = ([(np.float64, p_) for p_ in ('generic', 'fft', 'hybrid', 'auto')]
              + [(np.float32, p_) for p_ in ('generic', 'mfma', 'split', 'hybrid', 'auto', 'fft')])


@pytest.mark.parametrize('dtype,path', PATH_CASES, ids=[f'{np.dtype(d).name}_{p_}' for d, p_ in PATH_CASES])
def test_transformed_half_steps_on_every_path(dtype, path):
    """'dihedral' with 8 atoms: 64 effective atoms."""
    V = positive_V((3, 1, 48, 48), seed=1, dtype=dtype)
    dH, dW, nmf = half_steps(V, 8, (9, 9), 'dihedral', path, sparsity=0.05)
    assert nmf._H.shape[1] == 64
    tol = 1e-10 if dtype == np.float64 else 2e-5
    assert dW < tol, dW
    if not (dtype == np.float32 and path == 'fft'):   # (float32 FFT is a W-only path, include/tnmf_hip.h)
        assert dH < tol, dH


@pytest.mark.parametrize('lateral', [False, True], ids=['plain', 'inhibition'])
@pytest.mark.parametrize('mode', ['valid', 'full', 'circular', 'reflect'])
@pytest.mark.parametrize('dtype,path', [(np.float64, 'generic'), (np.float64, 'auto'), (np.float32, 'auto')],
                         ids=['f64_generic', 'f64_auto', 'f32_auto'])
def test_transformed_half_steps_modes_and_lateral_terms(dtype, path, mode, lateral):
    V = positive_V((3, 2, 20, 24), seed=2, dtype=dtype)
    kw = dict(sparsity=0.05, inhibition=0.1, cross=0.05) if lateral else {}
    dH, dW, _ = half_steps(V, 3, (4, 5), 'mirrors', path, mode=mode, **kw)
    tol = 1e-10 if dtype == np.float64 else 2e-5
    assert dH < tol and dW < tol, (dH, dW)


# -- 3. fits against the reference ------------------------------------------------------------------------------------
FIT_CASES = [('flip', (6,), (4, 2, 40)), ('flip', (4, 5), (4, 1, 30, 32)), ('mirrors', (5, 4), (4, 2, 30, 32)),
             ('rot90', (6, 6), (4, 1, 30, 32)), ('dihedral', (5, 5), (4, 1, 30, 32))]


def reference_fit(V, M, A, name, seed=42, beta=2., weights=None, **kw):
    np.random.seed(seed)
    return tref.TransformOracleNMF(n_atoms=M, atom_shape=A, transforms=name, impl='c', beta=beta,
                                   weights=weights).fit(V.astype(np.float64), **kw)


def check_fit(nmf, ref, tol=1e-10):
    assert relmax(nmf.W, ref.W) < tol and relmax(nmf.H, ref.H4) < tol, (relmax(nmf.W, ref.W), relmax(nmf.H, ref.H4))
    assert abs(nmf._energy_function() - ref.energy()) < tol * ref.energy()
    assert relmax(nmf.R, ref.R) < tol and relmax(nmf.R_partial(1), ref.R_partial(1)) < tol


@pytest.mark.parametrize('name,A,shape', FIT_CASES, ids=[f'{n}_{len(A)}d' for n, A, _ in FIT_CASES])
def test_transformed_fit_batch_f64_equals_the_reference(name, A, shape):
    V = positive_V(shape, seed=3)
    kw = dict(n_iterations=4, sparsity_H=0.05, inhibition_strength=0.1, cross_atom_inhibition_strength=0.05)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=A, backend='hip', transforms=name)
    nmf.fit_batch(V, progress_callback=CB, **kw)
    check_fit(nmf, reference_fit(V, 3, A, name, **kw))


def test_transformed_f32_fit_batch_W_at_the_hybrid_size():
    V = positive_V((12, 1, 96, 96), seed=9, dtype=np.float32)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=8, atom_shape=(12, 12), backend='hip', transforms='rot90')
    nmf.fit_batch(V, n_iterations=5, progress_callback=CB)
    ref = reference_fit(V, 8, (12, 12), 'rot90', n_iterations=5)
    dW = relmax(nmf.W, ref.W)
    print(f'rot90: float32 W after 5 iterations within {dW:.2e} of the float64 reference')
    assert dW < 1e-5, dW


def test_transformed_init_device_draws_the_model_shapes():
    V = positive_V((3, 1, 20, 20), seed=4)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(5, 5), backend='hip', transforms='dihedral', init='device')
    nmf.fit_batch(V, n_iterations=2, progress_callback=CB)
    assert nmf.W.shape == (2, 1, 5, 5) and nmf.H.shape == (3, 2, 8, 24, 24)
    assert np.allclose(nmf.W.sum(axis=(-2, -1)), 1.) and np.all(np.isfinite(nmf.H))
    assert np.array_equal(nmf.transformed_atoms.reshape(16, 1, 5, 5), tref.expand(nmf.W, 'dihedral'))


# -- 4. composition -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [1., 0.])
def test_transformed_beta_fits_equal_the_reference(beta):
    V = positive_V((4, 1, 30, 32), seed=5)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(6, 6), backend='hip', transforms='rot90', beta_loss=beta)
    nmf.fit_batch(V, n_iterations=4, sparsity_H=0.05, progress_callback=CB)
    check_fit(nmf, reference_fit(V, 3, (6, 6), 'rot90', beta=beta, n_iterations=4, sparsity_H=0.05))


@pytest.mark.parametrize('beta', [2., 1.])
def test_transformed_weighted_fits_equal_the_reference(beta):
    V = positive_V((4, 1, 30, 32), seed=6)
    rng = np.random.default_rng(6)
    G = rng.random((4, 1, 30, 32)) + 0.5
    G[rng.random(G.shape) < 0.2] = 0.
    V0 = np.where(G == 0, 0., V)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(5, 4), backend='hip', transforms='mirrors', beta_loss=beta)
    nmf.fit_batch(np.where(G == 0, np.nan, V), n_iterations=4, progress_callback=CB, weights=G)
    ref = reference_fit(V0, 3, (5, 4), 'mirrors', beta=beta, weights=G, n_iterations=4)
    assert relmax(nmf.W, ref.W) < 1e-10 and relmax(nmf.H, ref.H4) < 1e-10
    assert abs(nmf._energy_function() - ref.energy()) < 1e-10 * ref.energy()


@pytest.mark.parametrize('lateral', [False, True], ids=['plain', 'inhibition'])
@pytest.mark.parametrize('algorithm', list(MiniBatchAlgorithm), ids=[a.name for a in MiniBatchAlgorithm])
def test_transformed_epochs_equal_the_reference(algorithm, lateral):
    V = positive_V((7, 2, 20, 24), seed=7)
    kw = dict(batch_size=2, n_epochs=3, sparsity_H=0.05)
    if lateral:
        kw.update(inhibition_strength=0.1, cross_atom_inhibition_strength=0.05)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(5, 5), backend='hip', transforms='rot90')
    nmf.fit(V, algorithm=algorithm, progress_callback=CB, **kw)
    ref = reference_fit(V, 3, (5, 5), 'rot90', algorithm=orc.MiniBatchAlgorithm(algorithm.value), **kw)
    assert relmax(nmf.W, ref.W) < 1e-10 and relmax(nmf.H, ref.H4) < 1e-10


def test_transformed_stream_keeps_W():
    V = positive_V((6, 1, 24, 24), seed=8)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(5, 5), backend='hip', transforms='dihedral')
    nmf.fit(iter(V), subsample_size=3, n_iterations=3, progress_callback=CB)
    np.random.seed(42)
    ref = tref.TransformOracleNMF(n_atoms=2, atom_shape=(5, 5), transforms='dihedral', impl='c').fit(
        iter(V), subsample_size=3, n_iterations=3)
    assert relmax(nmf.W, ref.W) < 1e-10 and relmax(nmf.H, ref.H4) < 1e-10


def test_transformed_small_problem_runs_step_by_step():
    """A problem small enough for the persistent schedule kernel: transformed, it runs step by step and matches."""
    V = positive_V((2, 1, 24, 24), seed=12)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(5, 5), backend='hip', transforms='rot90')
    nmf._initialize_matrices(V, False)
    assert nmf._backend.prefers_schedule(nmf._H)
    calls = []
    plain = nmf._backend.run_schedule
    nmf._backend.run_schedule = lambda *a, **k: calls.append(1) or plain(*a, **k)
    np.random.seed(42)
    nmf.fit_batch(V, n_iterations=4, progress_callback=CB)
    assert not calls and not nmf._backend.last_schedule_persistent
    check_fit(nmf, reference_fit(V, 2, (5, 5), 'rot90', n_iterations=4))


# -- 5. two ranks in one process ------------------------------------------------------------------------------------
_init_lock = threading.Lock()


def _fit(V, mode, pg=None, sharded=False, reduce='all_reduce'):
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(5, 5), backend='hip', process_group=pg, transforms='rot90',
                                reduce=reduce, **({'sharded_input': True} if sharded else {}))
    plain_init = nmf._initialize_matrices

    def seeded_init(V_, keep_W, **kw):
        if sharded:
            nmf._backend.exchange_sample_counts(V_.shape[0])   # (a collective: before the lock)
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
@pytest.mark.parametrize('sharded', [False, True], ids=['global_V', 'sharded_input'])
@pytest.mark.parametrize('mode', ['batch', 'cyclic'])
def test_transformed_two_ranks_equal_the_unsharded_run(mode, sharded, reduce):
    V = positive_V((7, 2, 20, 24), seed=12)
    cuts = [(0, 4), (4, 7)]

    def rank_body(rank, coll):
        torch.cuda.set_device(0)
        lo, hi = cuts[rank]
        nmf = _fit(V[lo:hi], mode, coll, sharded=True, reduce=reduce) if sharded else _fit(V, mode, coll, reduce=reduce)
        return dict(W=nmf.W, H=nmf.H, E=nmf._energy_function(), Weff=nmf.transformed_atoms)

    (r0, r1), group = run_ranks(2, rank_body)
    assert np.array_equal(r0['W'], r1['W']) and np.array_equal(r0['Weff'], r1['Weff']) and r0['E'] == r1['E']
    single = _fit(V, mode)
    assert relmax(r0['W'], single.W) < 1e-10
    assert relmax(np.concatenate([r0['H'], r1['H']]), single.H) < 1e-10
    assert abs(r0['E'] - single._energy_function()) < 1e-10 * abs(r0['E'])


# -- 6. the spectrum cache: W_eff changes at a fixed address --------------------------------------------------------------
@pytest.mark.parametrize('algorithm', [None, MiniBatchAlgorithm.ASG_MU], ids=['batch', 'ASG_MU'])
def test_transformed_iterations_with_the_spectrum_cache_equal_fresh_contexts(algorithm):
    """The FFT family keeps the spectra of the dictionary between the W updates; W_eff keeps its address while every W
    step rewrites it.  Iterations with the cache on must equal iterations that drop every cached spectrum before each
    half step (the state of a fresh context), bit for bit, and the float64 reference."""
    V = positive_V((4, 1, 40, 40), seed=13)
    A = (6, 6)
    fit_kw = dict(n_iterations=4) if algorithm is None else dict(algorithm=algorithm, batch_size=2, n_epochs=2)
    out = []
    for fresh in (False, True):
        np.random.seed(42)
        nmf = TransformInvariantNMF(n_atoms=3, atom_shape=A, backend='hip', path='fft', transforms='rot90')
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
    assert counters['h_hits'] > 0, counters      # (the cache did serve the cached run)
    # (a stale spectrum of the dictionary would be that of the W before the step: a difference of order 1)
    assert relmax(W0, W1) < 1e-13 and relmax(H0, H1) < 1e-13, (relmax(W0, W1), relmax(H0, H1))
    ref_kw = dict(fit_kw)
    if algorithm is not None:
        ref_kw['algorithm'] = orc.MiniBatchAlgorithm(algorithm.value)
    ref = reference_fit(V, 3, A, 'rot90', **ref_kw)
    assert relmax(W0, ref.W) < 1e-10 and relmax(H0, ref.H4) < 1e-10


# -- 7. the planted rotated motif ----------------------------------------------------------------------------------------
def test_planted_rotated_motif_f32():
    """The property tests/test_transforms_cpu.py fixes on the reference, on the GPU in float32."""
    P = tref.PLANTED
    V = tref.planted(0).astype(np.float32)
    energies = []
    for transforms in ('rot90', None):
        np.random.seed(42)
        nmf = TransformInvariantNMF(n_atoms=1, atom_shape=P['atom_shape'], backend='hip', transforms=transforms)
        nmf.fit_batch(V, n_iterations=P['iterations'], progress_callback=CB)
        energies.append(nmf._energy_function())
    print(f'planted rotated motif, float32: energy {energies[0]:.3e} rot90, {energies[1]:.3e} plain')
    assert energies[1] >= tref.PLANTED_MARGIN * energies[0], energies
