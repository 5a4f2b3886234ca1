"""Elementwise weights on the GPU (tnmf_hip_weighted_fields / _update_H_weighted / _grad_W_weighted / _energy_weighted
and TransformInvariantNMF.fit(..., weights=G)) against the float64 reference of tests/weighted_reference.py."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import beta_reference as bref
import weighted_reference as wref
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


def mixed_weights(shape, seed, dtype=np.float64, zeros=0.2):
    """Random weights in [0.5, 1.5) with a 0/1 mask: about `zeros` of the entries 0, a few exactly 1."""
    rng = np.random.default_rng(seed + 1000)
    G = rng.random(shape) + 0.5
    G[rng.random(shape) < 0.1] = 1.
    G[rng.random(shape) < zeros] = 0.
    return G.astype(dtype)


def model(V, M, A, beta=2., seed=7, weights=None, **kw):
    nmf = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip', beta_loss=beta, **kw)
    np.random.seed(seed)
    G = nmf._weights_of(V, weights)
    if G is None:
        nmf._initialize_matrices(V, False)
    else:
        nmf._initialize_matrices(V, False, weights=G)
    return nmf


def p(t):
    return ctypes.c_void_p(t.data_ptr())


# -- 1. the fields primitive ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('g_offset', [False, True], ids=['Galigned', 'Goffset'])
@pytest.mark.parametrize('alias', [False, True], ids=['PnotR', 'PisR'])
@pytest.mark.parametrize('n', [1, 3, 4097])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('beta', [0., 0.5, 1., 1.5, 2., 3.])
def test_weighted_fields(beta, dtype, n, alias, g_offset):
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    _lib.check(lib.tnmf_hip_ctx_create(torch.cuda.current_device(), ctypes.byref(ctx)), 'ctx_create')
    try:
        rng = np.random.default_rng(n)
        V = rng.random(n).astype(dtype)
        R = (rng.random(n) * 1.2 - 0.1).astype(dtype)     # some entries below zero: clamped before + eps (beta != 2)
        G = (rng.random(n) * 2.).astype(dtype)
        zero = np.zeros(n, dtype=bool)
        if n == 3:
            G[1], V[1], zero[1] = 0., np.nan, True
        if n > 3:
            V[5] = 0.
            R[7] = 0.
            G[8] = 1.
            G[9], V[9] = 0., np.nan          # G == 0 over V = NaN
            G[11], R[11] = 0., -0.5          # ... over R < 0
            G[13], V[13] = 0., 0.            # ... over V = 0
            G[20:40] = 0.
            zero[[9, 11, 13]] = True
            zero[20:40] = True
        Qw, Pw = wref.fields(V, G, R, beta, bref.EPS, dtype=dtype)
        tV, tR = torch.from_numpy(V).cuda(), torch.from_numpy(R).cuda()
        if g_offset:      # G one element off 16-byte alignment: the scalar path
            tGbuf = torch.zeros(n + 1, dtype=tV.dtype, device=tV.device)
            tGbuf[1:] = torch.from_numpy(G).cuda()
            tG = tGbuf[1:]
        else:
            tG = torch.from_numpy(G).cuda()
        tQ = torch.empty_like(tV)
        tP = tR if alias else torch.empty_like(tR)
        code = 0 if dtype == np.float32 else 1
        _lib.check(lib.tnmf_hip_weighted_fields(ctx, code, beta, bref.EPS, p(tV), p(tG), p(tR), p(tQ), p(tP), n, None),
                   'weighted_fields')
        torch.cuda.synchronize()
        Q, P = tQ.cpu().numpy().astype(np.float64), tP.cpu().numpy().astype(np.float64)
        for got, want in ((Q, Qw), (P, Pw)):
            assert np.all(got[zero] == 0.) and np.all(np.signbit(got[zero]) == False), (beta, n)  # noqa: E712
            assert np.all(np.isfinite(got)), (beta, n)
            if dtype == np.float64:
                assert np.all(np.abs(got - want) <= 1e-14 * np.abs(want)), (beta, n)
            elif beta in (0., 1., 2.):
                ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
                assert np.all(np.abs(got - want) <= 3 * ulp), (beta, n)
            else:
                assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want)), (beta, n)
    finally:
        lib.tnmf_hip_ctx_destroy(ctx)


def test_zero_weight_selects_zero_where_the_field_overflows():
    """beta = -3 in float32: R~^(beta-2) = (1e-9)^-5 overflows, V * inf and 0 * inf are inf / NaN -- G == 0 selects 0."""
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    _lib.check(lib.tnmf_hip_ctx_create(torch.cuda.current_device(), ctypes.byref(ctx)), 'ctx_create')
    try:
        n = 64
        V = np.ones(n, dtype=np.float32)
        V[::2] = 0.
        R = np.full(n, -1., dtype=np.float32)
        G = np.zeros(n, dtype=np.float32)
        tV, tG, tR = (torch.from_numpy(x).cuda() for x in (V, G, R))
        tQ, tP = torch.empty_like(tV), torch.empty_like(tV)
        _lib.check(lib.tnmf_hip_weighted_fields(ctx, 0, -3., bref.EPS, p(tV), p(tG), p(tR), p(tQ), p(tP), n, None),
                   'weighted_fields')
        assert torch.all(tQ == 0).item() and torch.all(tP == 0).item()
        assert lib.tnmf_hip_weighted_fields(ctx, 0, 1., bref.EPS, p(tV), None, p(tR), p(tQ), p(tP), n, None) == -1
    finally:
        lib.tnmf_hip_ctx_destroy(ctx)


# -- 2. the half steps against the reference ------------------------------------------------------------------------
F64_PATHS = ['generic', 'fft', 'hybrid', 'auto']
F32_PATHS = ['generic', 'mfma', 'split', 'hybrid', 'auto', 'fft']
CASES = ([(np.float64, p_) for p_ in F64_PATHS] + [(np.float32, p_) for p_ in F32_PATHS])


def half_steps(V, G, M, A, beta, path, mode='valid', sparsity=0., inhibition=0., cross=0.):
    """One weighted H half step, then one W half step (from the GPU's H) -> (dH, dW) against the reference."""
    nmf = model(V, M, A, beta, weights=G, path=path, reconstruction_mode=mode)
    W0, H0 = nmf.W.astype(np.float64), nmf.H.astype(np.float64)
    V64, G64 = V.astype(np.float64), G.astype(np.float64)
    nmf._update_H(sparsity=sparsity, inhibition=inhibition, cross_inhibition=cross)
    Href = H0.copy()
    wref.update_H(V64, G64, W0, Href, beta=beta, sparsity=sparsity, inhibition=inhibition, cross_inhibition=cross,
                  kernels=nmf._inhibition_kernels_1D, mode=mode)
    Hgpu = nmf.H.astype(np.float64)
    dH = relmax(Hgpu, Href)
    nmf._update_W()
    Wref = W0.copy()
    wref.update_W(V64, G64, Wref, Hgpu, beta=beta, mode=mode)
    return dH, relmax(nmf.W, Wref), nmf


@pytest.mark.parametrize('beta', [2., 1., 0.])
@pytest.mark.parametrize('dtype,path', CASES, ids=[f'{np.dtype(d).name}_{p_}' for d, p_ in CASES])
def test_weighted_half_steps_on_every_path(dtype, path, beta):
    V = positive_V((4, 1, 64, 64), seed=1, dtype=dtype)
    G = mixed_weights(V.shape, seed=1, dtype=dtype)
    dH, dW, nmf = half_steps(V, G, 8, (9, 9), beta, path, sparsity=0.05)
    tol = 1e-10 if dtype == np.float64 else 2e-5
    assert dW < tol, dW
    if not (dtype == np.float32 and path == 'fft'):   # (float32 FFT is a W-only path, include/tnmf_hip.h)
        assert dH < tol, dH
    with pytest.raises(NotImplementedError):           # (the unweighted primitive refuses while weights are bound)
        nmf._backend.reconstruction_gradient_H(nmf._V, nmf._W, nmf._H)


@pytest.mark.parametrize('lateral', [False, True], ids=['plain', 'inhibition'])
@pytest.mark.parametrize('mode', ['valid', 'full', 'circular', 'reflect'])
@pytest.mark.parametrize('beta', [2., 1.])
@pytest.mark.parametrize('dtype,path', [(np.float64, 'generic'), (np.float32, 'auto')], ids=['f64_generic', 'f32_auto'])
def test_weighted_half_steps_modes_and_lateral_terms(dtype, path, beta, mode, lateral):
    V = positive_V((3, 2, 20, 24), seed=2, dtype=dtype)
    G = mixed_weights(V.shape, seed=2, dtype=dtype)
    kw = dict(sparsity=0.05, inhibition=0.1, cross=0.05) if lateral else {}
    dH, dW, _ = half_steps(V, G, 5, (4, 5), beta, path, mode=mode, **kw)
    tol = 1e-10 if dtype == np.float64 else 2e-5
    assert dH < tol and dW < tol, (dH, dW)


@pytest.mark.parametrize('lateral', [False, True], ids=['plain', 'inhibition'])
@pytest.mark.parametrize('beta', [2., 1.])
def test_weighted_row_padded_activations_on_the_split_path(beta, lateral):
    V = positive_V((12, 1, 96, 96), seed=3, dtype=np.float32)
    G = mixed_weights(V.shape, seed=3, dtype=np.float32)
    inh, cross = (0.1, 0.05) if lateral else (0., 0.)
    nmf = model(V, 32, (12, 12), beta, weights=G)
    assert not nmf._H.is_contiguous()     # rows padded to whole cache lines
    W0, H0 = nmf.W.astype(np.float64), nmf.H.astype(np.float64)
    nmf._update_H(inhibition=inh, cross_inhibition=cross)
    assert nmf._backend.last_path == 'split'
    Href = H0.copy()
    wref.update_H(V.astype(np.float64), G.astype(np.float64), W0, Href, beta=beta, inhibition=inh,
                  cross_inhibition=cross, kernels=nmf._inhibition_kernels_1D)
    assert relmax(nmf.H, Href) < 2e-5


# -- 3. unit weights --------------------------------------------------------------------------------------------------
UNIT_CASES = [(np.float64, 'auto', (4, 1, 40, 48)), (np.float32, 'auto', (12, 1, 96, 96)),
              (np.float32, 'fft', (4, 1, 40, 48))]


@pytest.mark.parametrize('beta', [2., 1., 0.])
@pytest.mark.parametrize('dtype,path,shape', UNIT_CASES, ids=['f64_auto', 'f32_auto_hybrid', 'f32_fft'])
def test_unit_weights_are_the_unweighted_fit(dtype, path, shape, beta):
    V = positive_V(shape, seed=4, dtype=dtype)
    out = []
    for weights in (None, np.ones(V.shape[:2] + (1, 1))):
        np.random.seed(42)
        nmf = TransformInvariantNMF(n_atoms=16, atom_shape=(12, 12), backend='hip', path=path, beta_loss=beta)
        nmf._use_schedules = False   # (the unweighted run steps too: the comparison is of the half steps themselves)
        nmf.fit_batch(V, n_iterations=3, sparsity_H=0.05, progress_callback=CB, weights=weights)
        out.append((nmf.W, nmf.H, nmf._energy_function()))
    (W0, H0, E0), (W1, H1, E1) = out
    if beta != 2.:
        # both run the fields (Q volatile, the same correlations) and x 1.0 is exact: the same bits
        assert np.array_equal(W0, W1) and np.array_equal(H0, H1) and E0 == E1
    else:
        tol = 1e-12 if dtype == np.float64 else 1e-6
        print(f'beta=2 G=1 {np.dtype(dtype).name} {path}: W identical={np.array_equal(W0, W1)} '
              f'H identical={np.array_equal(H0, H1)} dW={relmax(W1, W0):.1e} dH={relmax(H1, H0):.1e}')
        assert relmax(W1, W0) <= tol and abs(E1 - E0) <= tol * E0
        if path != 'fft':     # (float32 FFT is a W-only path, include/tnmf_hip.h)
            assert relmax(H1, H0) <= tol


# -- 4. masked-out values are never read ------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [2., 1.])
@pytest.mark.parametrize('dtype,path,shape', [(np.float64, 'auto', (4, 1, 40, 48)), (np.float32, 'auto', (12, 1, 96, 96))],
                         ids=['f64', 'f32_hybrid'])
def test_masked_out_values_are_never_read(dtype, path, shape, beta):
    V = positive_V(shape, seed=5, dtype=dtype)
    G = mixed_weights(V.shape, seed=5, dtype=dtype)
    out = []
    for fill in (0., np.nan, 1e30):
        Vf = np.where(G == 0, dtype(fill), V).astype(dtype)
        np.random.seed(42)
        nmf = TransformInvariantNMF(n_atoms=16, atom_shape=(12, 12), backend='hip', path=path, beta_loss=beta)
        nmf.fit_batch(Vf, n_iterations=2, progress_callback=CB, weights=G)
        out.append((nmf.W, nmf.H, nmf._energy_function()))
    for W, H, E in out[1:]:
        assert np.array_equal(W, out[0][0]) and np.array_equal(H, out[0][1]) and E == out[0][2]


# -- 5. the energy ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('beta', [0., 1., 1.5, 2.])
def test_weighted_energy(beta, dtype):
    V = positive_V((4, 2, 30, 33), seed=6, dtype=dtype)
    G = mixed_weights(V.shape, seed=6, dtype=dtype)
    V[G == 0] = 0.                                      # (beta 0: zeros are allowed where the weight is 0)
    nmf = model(V, 6, (5, 4), beta, weights=G)
    want = wref.energy(V.astype(np.float64), G.astype(np.float64), nmf.W.astype(np.float64),
                       nmf.H.astype(np.float64), beta)
    got = nmf._energy_function()
    again = nmf._energy_function()
    assert np.isfinite(got) and got == again
    assert abs(got - want) <= (1e-12 if dtype == np.float64 else 1e-5) * abs(want), (got, want)


# -- 6. fits ----------------------------------------------------------------------------------------------------------
def reference_fit(V, G, M, A, beta, seed=42, **kw):
    np.random.seed(seed)
    V0 = np.where(np.broadcast_to(G, V.shape) == 0, 0., V).astype(np.float64)
    return wref.WeightedOracleNMF(n_atoms=M, atom_shape=A, impl='c', beta=beta, weights=G).fit(V0, **kw)


def test_weighted_kl_fit_batch_f64_equals_the_reference_loop():
    V = positive_V((4, 1, 40, 48), seed=8)
    G = mixed_weights((4, 1, 40, 48), seed=8)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=16, atom_shape=(12, 12), backend='hip', beta_loss='kullback-leibler')
    nmf.fit_batch(V, n_iterations=10, progress_callback=CB, weights=G)
    ref = reference_fit(V, G, 16, (12, 12), 1., n_iterations=10)
    assert relmax(nmf.W, ref.W) < 1e-10 and relmax(nmf.H, ref.H) < 1e-10
    assert abs(nmf._energy_function() - ref.energy()) < 1e-10 * ref.energy()


@pytest.mark.parametrize('beta', [2., 1.])
def test_weighted_f32_fit_batch_W_at_the_hybrid_size(beta):
    V = positive_V((12, 1, 96, 96), seed=9, dtype=np.float32)
    G = mixed_weights((12, 1, 96, 96), seed=9, dtype=np.float32)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=32, atom_shape=(12, 12), backend='hip', beta_loss=beta)
    nmf.fit_batch(V, n_iterations=5, progress_callback=CB, weights=G)
    ref = reference_fit(V, G.astype(np.float64), 32, (12, 12), beta, n_iterations=5)
    dW = relmax(nmf.W, ref.W)
    print(f'weighted beta={beta}: float32 W after 5 iterations within {dW:.2e} of the float64 reference')
    assert dW < 1e-5, dW


@pytest.mark.parametrize('beta', [2., 1.])
@pytest.mark.parametrize('algorithm', list(MiniBatchAlgorithm), ids=[a.name for a in MiniBatchAlgorithm])
def test_weighted_epochs_equal_the_reference_loop(algorithm, beta):
    V = positive_V((7, 2, 20, 24), seed=11)
    G = mixed_weights((7, 1, 20, 24), seed=11)          # [N, 1, *D]: a mask shared by the channels
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=5, atom_shape=(4, 5), backend='hip', beta_loss=beta)
    nmf.fit(V, algorithm=algorithm, batch_size=2, n_epochs=3, sparsity_H=0.05, progress_callback=CB, weights=G)
    ref = reference_fit(V, G, 5, (4, 5), beta, algorithm=orc.MiniBatchAlgorithm(algorithm.value), batch_size=2,
                        n_epochs=3, sparsity_H=0.05)
    assert relmax(nmf.W, ref.W) < 1e-10 and relmax(nmf.H, ref.H) < 1e-10


def test_weighted_small_problem_runs_step_by_step():
    """A problem small enough for the persistent schedule kernel: weighted, it runs step by step and matches."""
    V = positive_V((2, 1, 24, 24), seed=12)
    G = mixed_weights((2, 1, 1, 1), seed=3, zeros=0.)        # per-sample weights
    G[1] = 0.25
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=4, atom_shape=(5, 5), backend='hip')
    nmf._initialize_matrices(V, False)
    assert nmf._backend.prefers_schedule(nmf._H)
    calls = []
    plain = nmf._backend.run_schedule
    nmf._backend.run_schedule = lambda *a, **k: calls.append(1) or plain(*a, **k)
    np.random.seed(42)
    nmf.fit_batch(V, n_iterations=4, progress_callback=CB, weights=G)
    assert not calls and not nmf._backend.last_schedule_persistent
    ref = reference_fit(V, G, 4, (5, 5), 2., n_iterations=4)
    assert relmax(nmf.W, ref.W) < 1e-10 and relmax(nmf.H, ref.H) < 1e-10


# -- 7. two ranks in one process ------------------------------------------------------------------------------------
_init_lock = threading.Lock()


def _fit(V, G, mode, pg=None, sharded=False):
    nmf = TransformInvariantNMF(n_atoms=5, atom_shape=(4, 5), backend='hip', process_group=pg, beta_loss=1.,
                                **({'sharded_input': True} if sharded else {}))
    plain_init = nmf._initialize_matrices

    def seeded_init(V_, keep_W, **kw):
        if sharded:
            nmf._backend.exchange_sample_counts(V_.shape[0])   # (a collective: before the lock)
        with _init_lock:
            np.random.seed(42)
            plain_init(V_, keep_W, **kw)

    nmf._initialize_matrices = seeded_init
    if mode == 'batch':
        nmf.fit(V, n_iterations=3, sparsity_H=0.05, progress_callback=CB, weights=G)
    else:
        nmf.fit(V, algorithm=MiniBatchAlgorithm.Cyclic_MU, batch_size=2, n_epochs=3, sparsity_H=0.05,
                progress_callback=CB, weights=G)
    return nmf


@pytest.mark.parametrize('sharded', [False, True], ids=['global_V', 'sharded_input'])
@pytest.mark.parametrize('mode', ['batch', 'cyclic'])
def test_weighted_two_ranks_equal_the_unsharded_run(mode, sharded):
    V = positive_V((7, 2, 20, 24), seed=12)
    G = mixed_weights(V.shape, seed=12)
    cuts = [(0, 4), (4, 7)]

    def rank_body(rank, coll):
        torch.cuda.set_device(0)
        lo, hi = cuts[rank]
        nmf = _fit(V[lo:hi], G[lo:hi], mode, coll, sharded=True) if sharded else _fit(V, G, mode, coll)
        return dict(W=nmf.W, H=nmf.H, E=nmf._energy_function())

    (r0, r1), _group = run_ranks(2, rank_body)
    assert np.array_equal(r0['W'], r1['W']) and r0['E'] == r1['E']
    single = _fit(V, G, mode)
    assert relmax(r0['W'], single.W) < 1e-10
    assert relmax(np.concatenate([r0['H'], r1['H']]), single.H) < 1e-10
    assert abs(r0['E'] - single._energy_function()) < 1e-10 * abs(r0['E'])


# -- 8. no weights leak into a later fit ------------------------------------------------------------------------------
def test_refit_without_weights_is_unweighted():
    V = positive_V((4, 1, 40, 48), seed=13)
    G = mixed_weights(V.shape, seed=13)
    np.random.seed(42)
    a = TransformInvariantNMF(n_atoms=16, atom_shape=(12, 12), backend='hip')
    a.fit_batch(V, n_iterations=2, progress_callback=CB, weights=G)
    W_weighted = a.W
    np.random.seed(43)
    a.fit_batch(V, n_iterations=3, keep_W=True, progress_callback=CB)
    assert a._backend._G_dev is None and a._plain_frobenius
    b = TransformInvariantNMF(n_atoms=16, atom_shape=(12, 12), backend='hip')
    np.random.seed(0)
    b._initialize_matrices(V, False)
    b._W.copy_(torch.from_numpy(W_weighted).to(b._W.device))
    np.random.seed(43)
    b.fit_batch(V, n_iterations=3, keep_W=True, progress_callback=CB)
    assert relmax(a.W, b.W) < 1e-12 and relmax(a.H, b.H) < 1e-12
    assert abs(a._energy_function() - b._energy_function()) <= 1e-12 * b._energy_function()


# -- 9. volumes and non-finite beta are refused before anything is written --------------------------------------------
def test_weighted_volumes_and_bad_beta_are_refused_untouched():
    with pytest.raises(NotImplementedError):
        TransformInvariantNMF(n_atoms=2, atom_shape=(2, 2, 2), backend='hip').fit_batch(
            positive_V((2, 1, 6, 6, 6), seed=14), n_iterations=1, weights=np.ones((2, 1, 6, 6, 6)))
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    _lib.check(lib.tnmf_hip_ctx_create(torch.cuda.current_device(), ctypes.byref(ctx)), 'ctx_create')
    try:
        for geom, shape_H, beta in (((2, 3, 1, (6, 6, 6), (2, 2, 2)), (2, 3, 7, 7, 7), 1.),
                                    ((2, 3, 1, (8, 8), (3, 3)), (2, 3, 10, 10), float('nan')),
                                    ((2, 3, 1, (8, 8), (3, 3)), (2, 3, 10, 10), float('inf'))):
            n, m, c, D, A = geom
            g = _lib.make_geom(n, m, c, D, A, 1)
            V = torch.rand((n, c) + D, dtype=torch.float64, device='cuda')
            G = torch.ones_like(V)
            W = torch.rand((m, c) + A, dtype=torch.float64, device='cuda')
            H = torch.rand(shape_H, dtype=torch.float64, device='cuda')
            R = torch.full_like(V, 5.)
            negpos = torch.full((2, m, c) + A, 7., dtype=torch.float64, device='cuda')
            H0, R0 = H.clone(), R.clone()
            none = (None, 0, None, 0, None, 0)
            gp = ctypes.byref(g)
            assert lib.tnmf_hip_update_H_weighted(ctx, gp, 0, p(V), p(G), p(W), p(H), p(R), 1e-9, 0., 0., 0., *none,
                                                  beta, None) == _lib.E_UNSUPPORTED
            assert lib.tnmf_hip_grad_W_weighted(ctx, gp, p(V), p(G), p(W), p(H), p(R), 0, p(negpos), beta, 1e-9,
                                                None) == _lib.E_UNSUPPORTED
            out = ctypes.c_double(-1.)
            assert lib.tnmf_hip_energy_weighted(ctx, gp, beta, 1e-9, p(V), p(G), p(W), p(H), ctypes.byref(out),
                                                None) == _lib.E_UNSUPPORTED
            torch.cuda.synchronize()
            assert torch.equal(H, H0) and torch.equal(R, R0) and bool(torch.all(negpos == 7.)) and out.value == -1.
    finally:
        lib.tnmf_hip_ctx_destroy(ctx)


# -- 10. planted inpainting -------------------------------------------------------------------------------------------
def test_planted_inpainting_f32():
    """The property tests/test_weights_cpu.py fixes on the reference, on the GPU in float32."""
    P = wref.INPAINT
    V, V0, mask = wref.planted(0)
    errs = []
    for weights in (mask, None):
        np.random.seed(42)
        nmf = TransformInvariantNMF(n_atoms=P['n_atoms'], atom_shape=P['atom_shape'], backend='hip')
        nmf.fit_batch(V0.astype(np.float32), n_iterations=P['iterations'], progress_callback=CB,
                      weights=None if weights is None else weights.astype(np.float32))
        errs.append(wref.hole_error(nmf.R, V, mask))
    print(f'planted inpainting, float32: error in the hole {errs[0]:.3e} weighted, {errs[1]:.3e} zero-filled')
    assert errs[1] >= wref.INPAINT_MARGIN * errs[0], errs
