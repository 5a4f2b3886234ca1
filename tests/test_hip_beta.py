"""beta-divergence objectives on the GPU (tnmf_hip_beta_fields / _update_H_beta / _grad_W_beta / _energy_beta and
TransformInvariantNMF(beta_loss=...)) against the float64 reference of tests/beta_reference.py."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import beta_reference as bref
from local_collective import run_ranks
from oracle import tnmf_oracle as orc
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import MiniBatchAlgorithm, TransformInvariantNMF

pytestmark = pytest.mark.gpu

bref.IMPL = 'c'
CB = lambda *_: True  # noqa: E731  (a progress callback: no per-iteration energy through the logger)


def relmax(got, want):
    want = np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max()
    return np.abs(np.asarray(got, dtype=np.float64) - want).max() / (scale if scale > 0 else 1.0)


def positive_V(shape, seed, dtype=np.float64):
    return (np.random.default_rng(seed).random(shape) + 0.05).astype(dtype)


def model(V, M, A, beta, seed=7, **kw):
    nmf = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip', beta_loss=beta, **kw)
    np.random.seed(seed)
    nmf._initialize_matrices(V, False)
    return nmf


# -- 1. the fields primitive ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('alias', [False, True], ids=['PnotR', 'PisR'])
@pytest.mark.parametrize('n', [1, 3, 4097])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('beta', [0., 0.5, 1., 1.5, 2., 3.])
def test_beta_fields(beta, dtype, n, alias):
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    _lib.check(lib.tnmf_hip_ctx_create(torch.cuda.current_device(), ctypes.byref(ctx)), 'ctx_create')
    try:
        rng = np.random.default_rng(n)
        V = rng.random(n).astype(dtype)
        R = (rng.random(n) * 1.2 - 0.1).astype(dtype)     # some entries below zero: clamped before + eps
        if n > 3:
            V[5] = 0.
            R[7] = 0.
        Qw, Pw = bref.fields(V, R, beta, bref.EPS, dtype=dtype)
        tV, tR = torch.from_numpy(V).cuda(), torch.from_numpy(R).cuda()
        tQ = torch.empty_like(tV)
        tP = tR if alias else torch.empty_like(tR)
        code = 0 if dtype == np.float32 else 1
        _lib.check(lib.tnmf_hip_beta_fields(ctx, code, beta, bref.EPS, ctypes.c_void_p(tV.data_ptr()),
                                            ctypes.c_void_p(tR.data_ptr()), ctypes.c_void_p(tQ.data_ptr()),
                                            ctypes.c_void_p(tP.data_ptr()), n, None), 'beta_fields')
        torch.cuda.synchronize()
        Q, P = tQ.cpu().numpy().astype(np.float64), tP.cpu().numpy().astype(np.float64)
        for got, want in ((Q, Qw), (P, Pw)):
            if dtype == np.float64:
                assert np.all(np.abs(got - want) <= 1e-14 * np.abs(want)), (beta, n)
            elif beta in (0., 1., 2.):
                ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
                assert np.all(np.abs(got - want) <= 2 * ulp), (beta, n)
            else:
                assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want)), (beta, n)
    finally:
        lib.tnmf_hip_ctx_destroy(ctx)


# -- 2. the half steps against the reference ------------------------------------------------------------------------
F64_PATHS = ['generic', 'fft', 'hybrid', 'auto']
F32_PATHS = ['generic', 'mfma', 'split', 'hybrid', 'auto', 'fft']
CASES = ([(np.float64, p) for p in F64_PATHS] + [(np.float32, p) for p in F32_PATHS])


def half_steps(V, M, A, beta, path, mode='valid', sparsity=0., inhibition=0., cross=0.):
    """One H half step, then one W half step (from the GPU's H) -> (dH, dW) against the reference."""
    nmf = model(V, M, A, beta, path=path, reconstruction_mode=mode)
    W0, H0 = nmf.W.astype(np.float64), nmf.H.astype(np.float64)
    V64 = V.astype(np.float64)
    nmf._update_H(sparsity=sparsity, inhibition=inhibition, cross_inhibition=cross)
    Href = H0.copy()
    bref.update_H(V64, W0, Href, beta=beta, sparsity=sparsity, inhibition=inhibition, cross_inhibition=cross,
                  kernels=nmf._inhibition_kernels_1D, mode=mode)
    Hgpu = nmf.H.astype(np.float64)
    dH = relmax(Hgpu, Href)
    nmf._update_W()
    Wref = W0.copy()
    bref.update_W(V64, Wref, Hgpu, beta=beta, mode=mode)
    return dH, relmax(nmf.W, Wref), nmf


@pytest.mark.parametrize('sparsity', [0., 0.1], ids=['plain', 'sparse'])
@pytest.mark.parametrize('beta', [0., 1., 1.5])
@pytest.mark.parametrize('dtype,path', CASES, ids=[f'{np.dtype(d).name}_{p}' for d, p in CASES])
def test_half_steps_on_every_path(dtype, path, beta, sparsity):
    V = positive_V((4, 1, 64, 64), seed=1, dtype=dtype)
    dH, dW, _ = half_steps(V, 8, (9, 9), beta, path, sparsity=sparsity)
    tol = 1e-10 if dtype == np.float64 else 2e-5
    assert dW < tol, dW
    if not (dtype == np.float32 and path == 'fft'):   # (float32 FFT is a W-only path, include/tnmf_hip.h)
        assert dH < tol, dH


@pytest.mark.parametrize('lateral', [False, True], ids=['plain', 'inhibition'])
@pytest.mark.parametrize('mode', ['valid', 'full', 'circular', 'reflect'])
@pytest.mark.parametrize('beta', [0., 1., 1.5])
@pytest.mark.parametrize('dtype,path', [(np.float64, 'generic'), (np.float64, 'auto'), (np.float32, 'auto')],
                         ids=['f64_generic', 'f64_auto', 'f32_auto'])
def test_half_steps_modes_and_lateral_terms(dtype, path, beta, mode, lateral):
    V = positive_V((3, 2, 20, 24), seed=2, dtype=dtype)
    kw = dict(sparsity=0.05, inhibition=0.1, cross=0.05) if lateral else {}
    dH, dW, _ = half_steps(V, 5, (4, 5), beta, path, mode=mode, **kw)
    tol = 1e-10 if dtype == np.float64 else 2e-5
    assert dH < tol and dW < tol, (dH, dW)


@pytest.mark.parametrize('lateral', [False, True], ids=['plain', 'inhibition'])
@pytest.mark.parametrize('beta', [0., 1., 1.5])
def test_row_padded_activations_on_the_split_path(beta, lateral):
    """float32 at a size where 'auto' is the hybrid dispatch: H lives in row-padded storage and the H update runs on the
    split kernel (the lateral terms in its epilogue)."""
    V = positive_V((12, 1, 96, 96), seed=3, dtype=np.float32)
    kw = dict(inhibition=0.1, cross=0.05) if lateral else {}
    nmf = model(V, 32, (12, 12), beta)
    assert not nmf._H.is_contiguous()     # rows padded to whole cache lines
    W0, H0 = nmf.W.astype(np.float64), nmf.H.astype(np.float64)
    nmf._update_H(inhibition=kw.get('inhibition', 0.), cross_inhibition=kw.get('cross', 0.))
    assert nmf._backend.last_path == 'split'
    Href = H0.copy()
    bref.update_H(V.astype(np.float64), W0, Href, beta=beta, inhibition=kw.get('inhibition', 0.),
                  cross_inhibition=kw.get('cross', 0.), kernels=nmf._inhibition_kernels_1D)
    assert relmax(nmf.H, Href) < 2e-5


# -- 3. beta == 2 through the new entries is the Frobenius step ------------------------------------------------------
def _entries(nmf):
    """(library, ctx, geometry, V, W, H, R scratch, stream) of a model's resident problem, for calling the C ABI."""
    be = nmf._backend
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = be._geom(nmf._H.shape[0], nmf._W.shape[0], be._row_stride(nmf._H))
    return be._lib, be._ctx, ctypes.byref(g), p(be._V_dev), p(nmf._W), p(nmf._H), p(be._R_scratch), be._stream()


@pytest.mark.parametrize('dtype,path', [(np.float64, 'auto'), (np.float32, 'auto'), (np.float32, 'fft')],
                         ids=['f64_auto', 'f32_auto', 'f32_fft'])
def test_beta_2_entry_points_are_the_frobenius_calls(dtype, path):
    """include/tnmf_hip.h: at beta == 2 each beta entry point is its Frobenius counterpart, and tnmf_hip_update_H is the
    'valid' step of tnmf_hip_update_H_ex without lateral terms -- same bits.  So are the backend hooks with beta=2."""
    V = positive_V((12, 1, 96, 96), seed=4, dtype=dtype)
    a, b = model(V, 32, (12, 12), 2., path=path), model(V, 32, (12, 12), 2., path=path)
    sp, eps = 0.05, a.eps
    none = (None, 0, None, 0, None, 0)
    for _ in range(2):
        lib, ca, ga, Va, Wa, Ha, Ra, sa = _entries(a)
        _, cb, gb, Vb, Wb, Hb, Rb, sb = _entries(b)
        _lib.check(lib.tnmf_hip_update_H(ca, ga, Va, Wa, Ha, Ra, 0, eps, sp, sa), 'update_H')
        _lib.check(lib.tnmf_hip_update_H_ex(cb, gb, 0, Vb, Wb, Hb, Rb, eps, sp, 0., 0., *none, sb), 'update_H_ex')
        assert np.array_equal(a.H, b.H)
        _lib.check(lib.tnmf_hip_update_H_ex(ca, ga, 0, Va, Wa, Ha, Ra, eps, sp, 0., 0., *none, sa), 'update_H_ex')
        _lib.check(lib.tnmf_hip_update_H_beta(cb, gb, 0, Vb, Wb, Hb, Rb, eps, sp, 0., 0., *none, 2., sb), 'update_H_beta')
        assert np.array_equal(a.H, b.H)
        npa, npb = torch.empty_like(a._backend._negpos), torch.empty_like(b._backend._negpos)
        _lib.check(lib.tnmf_hip_grad_W_fused(ca, ga, Va, Wa, Ha, Ra, 0, ctypes.c_void_p(npa.data_ptr()), sa), 'grad_W')
        _lib.check(lib.tnmf_hip_grad_W_beta(cb, gb, Vb, Wb, Hb, Rb, 0, ctypes.c_void_p(npb.data_ptr()), 2., eps, sb),
                   'grad_W_beta')
        assert np.array_equal(npa.cpu().numpy(), npb.cpu().numpy())
        a._backend.apply_W(a._W, npa, eps)
        b._backend.apply_W(b._W, npb, eps)
        assert np.array_equal(a.W, b.W)
        ea, eb = ctypes.c_double(0.), ctypes.c_double(1.)
        _lib.check(lib.tnmf_hip_energy(ca, ga, Va, Wa, Ha, ctypes.byref(ea), sa), 'energy')
        _lib.check(lib.tnmf_hip_energy_beta(cb, gb, 2., eps, Vb, Wb, Hb, ctypes.byref(eb), sb), 'energy_beta')
        assert ea.value == eb.value
    # the hooks: beta=2. is the default objective
    for _ in range(2):
        a._backend.fused_update_H(a._V, a._W, a._H, sparsity=sp, eps=eps)
        b._backend.fused_update_H(b._V, b._W, b._H, sparsity=sp, eps=eps, beta=2.)
        assert np.array_equal(a.H, b.H)
        ga = a._backend.local_gradient_W(a._V, a._W, a._H).cpu().numpy()
        gb = b._backend.local_gradient_W(b._V, b._W, b._H, beta=2., eps=eps).cpu().numpy()
        assert np.array_equal(ga, gb)
        a._backend.fused_update_W(a._V, a._W, a._H, eps=eps)
        b._backend.fused_update_W(b._V, b._W, b._H, eps=eps, beta=2.)
        assert np.array_equal(a.W, b.W)
    assert a._backend.reconstruction_energy(a._V, a._W, a._H) == \
        b._backend.reconstruction_energy(b._V, b._W, b._H, beta=2., eps=eps)


def test_frobenius_by_name_is_the_default_fit():
    V = positive_V((12, 1, 96, 96), seed=5, dtype=np.float32)
    out = []
    for kw in ({}, {'beta_loss': 'frobenius'}):
        np.random.seed(42)
        nmf = TransformInvariantNMF(n_atoms=32, atom_shape=(12, 12), backend='hip', **kw)
        nmf.fit_batch(V, n_iterations=3, sparsity_H=0.05, progress_callback=CB)
        out.append((nmf.W, nmf.H, nmf._energy_function()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


# -- 4. the energy --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('beta', [0., 1., 1.5, 2.])
def test_energy_beta(beta, dtype):
    V = positive_V((4, 2, 30, 33), seed=6, dtype=dtype)
    if beta == 1.:
        V[0, 0, :5] = 0.                  # 0 log 0 = 0
    nmf = model(V, 6, (5, 4), beta)
    want = bref.energy(V.astype(np.float64), nmf.W.astype(np.float64), nmf.H.astype(np.float64), beta)
    got = nmf._energy_function()
    assert abs(got - want) <= (1e-12 if dtype == np.float64 else 1e-5) * abs(want), (got, want)


# -- 5. end to end --------------------------------------------------------------------------------------------------
def reference_fit(V, M, A, beta, seed=42, **kw):
    np.random.seed(seed)
    return bref.BetaOracleNMF(n_atoms=M, atom_shape=A, impl='c', beta=beta).fit(V.astype(np.float64), **kw)


def test_kl_fit_batch_f64_equals_the_reference_loop():
    V = positive_V((4, 1, 40, 48), seed=8)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=16, atom_shape=(12, 12), backend='hip', beta_loss='kullback-leibler')
    nmf.fit_batch(V, n_iterations=10, progress_callback=CB)
    ref = reference_fit(V, 16, (12, 12), 1., n_iterations=10)
    assert relmax(nmf.W, ref.W) < 1e-10 and relmax(nmf.H, ref.H) < 1e-10
    assert abs(nmf._energy_function() - ref.energy()) < 1e-10 * ref.energy()


@pytest.mark.parametrize('beta,bar', [(1., 1e-5), (0., 1e-5)], ids=['kl', 'is'])   # (measured 4.9e-7 / 6.9e-7)
def test_f32_fit_batch_W_against_the_reference(beta, bar):
    V = positive_V((12, 1, 96, 96), seed=9, dtype=np.float32)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=32, atom_shape=(12, 12), backend='hip', beta_loss=beta)
    nmf.fit_batch(V, n_iterations=5, progress_callback=CB)
    ref = reference_fit(V, 32, (12, 12), beta, n_iterations=5)
    dW = relmax(nmf.W, ref.W)
    print(f'beta={beta}: float32 W after 5 iterations within {dW:.2e} of the float64 reference')
    assert dW < bar, dW


@pytest.mark.parametrize('beta', [1., 1.5])
def test_divergence_does_not_increase_over_H_steps(beta):
    V = positive_V((4, 1, 40, 48), seed=10)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=16, atom_shape=(12, 12), backend='hip', beta_loss=beta)
    nmf.fit_batch(V, n_iterations=1, progress_callback=CB)
    energies = []
    nmf.fit_batch(V, n_iterations=20, update_W=False, keep_W=True,
                  progress_callback=lambda m, _i: energies.append(m._energy_function()) or True)
    assert len(energies) == 20
    assert all(b <= a * (1 + 1e-12) for a, b in zip(energies, energies[1:])), energies


# -- 6. mini-batch schedules ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('algorithm', [MiniBatchAlgorithm.Cyclic_MU, MiniBatchAlgorithm.ASG_MU,
                                       MiniBatchAlgorithm.GSAG_MU], ids=['cyclic', 'asg', 'gsag'])
def test_kl_epochs_equal_the_reference_loop(algorithm):
    V = positive_V((7, 2, 20, 24), seed=11)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=5, atom_shape=(4, 5), backend='hip', beta_loss=1.)
    nmf.fit(V, algorithm=algorithm, batch_size=2, n_epochs=3, sparsity_H=0.05, progress_callback=CB)
    ref = reference_fit(V, 5, (4, 5), 1., algorithm=orc.MiniBatchAlgorithm(algorithm.value), batch_size=2, n_epochs=3,
                        sparsity_H=0.05)
    assert relmax(nmf.W, ref.W) < 1e-10 and relmax(nmf.H, ref.H) < 1e-10


# -- 7. two ranks in one process ------------------------------------------------------------------------------------
_init_lock = threading.Lock()


def _fit(V, mode, pg=None):
    nmf = TransformInvariantNMF(n_atoms=5, atom_shape=(4, 5), backend='hip', process_group=pg, beta_loss=1.)
    plain_init = nmf._initialize_matrices

    def seeded_init(V_, keep_W):
        with _init_lock:
            np.random.seed(42)
            plain_init(V_, keep_W)

    nmf._initialize_matrices = seeded_init
    if mode == 'batch':
        nmf.fit(V, n_iterations=3, sparsity_H=0.05, progress_callback=CB)
    else:
        nmf.fit(V, algorithm=MiniBatchAlgorithm.Cyclic_MU, batch_size=2, n_epochs=3, sparsity_H=0.05,
                progress_callback=CB)
    return nmf


@pytest.mark.parametrize('mode', ['batch', 'cyclic'])
def test_kl_two_ranks_equal_the_unsharded_run(mode):
    V = positive_V((7, 2, 20, 24), seed=12)

    def rank_body(rank, coll):
        torch.cuda.set_device(0)
        nmf = _fit(V, mode, coll)
        return dict(W=nmf.W, H=nmf.H, E=nmf._energy_function())

    (r0, r1), _group = run_ranks(2, rank_body)
    assert np.array_equal(r0['W'], r1['W']) and r0['E'] == r1['E']
    single = _fit(V, mode)
    assert relmax(r0['W'], single.W) < 1e-10
    assert relmax(np.concatenate([r0['H'], r1['H']]), single.H) < 1e-10
    assert abs(r0['E'] - single._energy_function()) < 1e-10 * abs(r0['E'])


# -- 8. the FFT spectrum cache --------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('path', ['hybrid', 'fft'])
def test_kl_iterations_with_the_cache_equal_fresh_contexts(path, dtype):
    V = positive_V((6, 1, 40, 48), seed=13, dtype=dtype)
    h_args = dict(sparsity=0., inhibition=0., cross_inhibition=0.)
    a = model(V, 16, (12, 12), 1., path=path)      # one context, cache on ('valid' mode)
    W1, H1 = a._W.clone(), a._H.clone()
    a._iteration(h_args)
    Wa1, Ha1 = a.W, a.H
    a._iteration(h_args)
    for W_in, H_in, want in ((W1, H1, (Wa1, Ha1)), (None, None, (a.W, a.H))):
        b = model(V, 16, (12, 12), 1., path=path)  # a fresh context for each iteration
        if W_in is None:
            b._W.copy_(torch.from_numpy(Wa1).to(b._W.device))
            b._H.copy_(torch.from_numpy(Ha1).to(b._H.device))
        else:
            b._W.copy_(W_in)
            b._H.copy_(H_in)
        b._iteration(h_args)
        assert np.array_equal(b.W, want[0]) and np.array_equal(b.H, want[1])
