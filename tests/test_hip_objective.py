"""The objective tap of the H half steps (tnmf_hip_ctx_set_objective_tap), tnmf_hip_sample_objective and
``fit(..., objective_every=, tol=)`` on the GPU: the per-sample values against numpy float64 on the oracle's reconstruction
of the state before the step (formulas of tests/beta_reference.py / tests/weighted_reference.py), the step's own result
against an untapped twin, and whole fits against the float64 trajectory of the oracle."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import beta_reference as bref
import weighted_reference as wref
from convergence_reference import pick_tol, predict, trajectory
from local_collective import run_ranks
from oracle import tnmf_oracle as orc
from oracle_backend import OracleBackend
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

pytestmark = pytest.mark.gpu

CB = lambda *_: True  # noqa: E731
BAR = {np.float64: 1e-10, np.float32: 1e-5}   # the project's energy bars, relative


def relmax(got, want):
    want = np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max()
    return np.abs(np.asarray(got, dtype=np.float64) - want).max() / (scale if scale > 0 else 1.0)


def positive_V(shape, seed, dtype=np.float64):
    return (np.random.default_rng(seed).random(shape) + 0.05).astype(dtype)


def mixed_weights(shape, seed, dtype=np.float64, zeros=0.2):
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


def per_sample_reference(V, G, W, H, beta, mode='valid'):
    """Each sample's objective in numpy float64 on the oracle's reconstruction of (W, H)."""
    V, W, H = (np.asarray(x, dtype=np.float64) for x in (V, W, H))
    R = orc.reconstruct(W, H, 'c' if W.ndim <= 4 else 'contract', mode)
    if G is None:
        return np.array([bref.divergence(V[n], R[n], beta) for n in range(len(V))])
    G = np.asarray(G, dtype=np.float64)
    return np.array([wref.divergence(V[n], G[n], R[n], beta) for n in range(len(V))])


def tapped_step(V, G, M, A, beta, path='auto', mode='valid', h_args=None, expect_path=None, padded=None):
    """One tapped H half step of a fresh model and the same step of an untapped twin; the checks every case shares."""
    h_args = h_args or {}
    dtype = V.dtype.type
    a = model(V, M, A, beta, weights=G, path=path, reconstruction_mode=mode)
    b = model(V, M, A, beta, weights=G, path=path, reconstruction_mode=mode)
    if padded is not None:
        assert a._H.is_contiguous() != padded
    W0, H0 = a.W, a.H
    assert np.array_equal(H0, b.H)
    E0, E0b = a._energy_function(), b._energy_function()
    assert E0 == E0b
    assert a._update_H(record=True, **h_args) is None, 'the step goes through the tap'
    tap = a._objective_buf.cpu().numpy()
    b._update_H(**h_args)
    if expect_path is not None:
        assert a._backend.last_path == expect_path
    assert np.array_equal(a.H, b.H), 'the tap changes nothing the step computes'
    assert not np.array_equal(a.H, H0)
    want = per_sample_reference(V, G, W0, H0, beta, mode)
    err = np.abs(tap - want) / np.abs(want)
    gap = abs(float(np.sum(tap)) - E0) / abs(E0)
    print(f'tap {np.dtype(dtype).name} beta={beta} path={path} mode={mode} weighted={G is not None}: '
          f'per-sample {err.max():.2e}, sum vs energy {gap:.2e}')
    assert np.all(np.isfinite(tap)) and tap.shape == (len(V),)
    assert err.max() <= BAR[dtype], err
    assert gap <= 1e-10, (float(np.sum(tap)), E0)
    return a, tap


# -- 1. one tapped H half step ---------------------------------------------------------------------------------------
F64_PATHS = ['generic', 'fft', 'hybrid', 'auto']
F32_PATHS = ['generic', 'mfma', 'split', 'hybrid', 'auto', 'fft']
CASES = [(np.float64, p_) for p_ in F64_PATHS] + [(np.float32, p_) for p_ in F32_PATHS]


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('beta', [2., 1., 0., 0.5])
@pytest.mark.parametrize('dtype,path', CASES, ids=[f'{np.dtype(d).name}_{p_}' for d, p_ in CASES])
def test_tap_2d_on_every_path(dtype, path, beta, weighted):
    V = positive_V((4, 1, 64, 64), seed=1, dtype=dtype)
    G = mixed_weights(V.shape, seed=1, dtype=dtype) if weighted else None
    tapped_step(V, G, 8, (9, 9), beta, path, h_args=dict(sparsity=0.05))


ONE_D = [(np.float64, 'generic'), (np.float64, 'hybrid'), (np.float64, 'auto'), (np.float32, 'generic'),
         (np.float32, 'split'), (np.float32, 'hybrid'), (np.float32, 'auto')]


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('beta', [2., 1., 0., 0.5])
@pytest.mark.parametrize('dtype,path', ONE_D, ids=[f'{np.dtype(d).name}_{p_}' for d, p_ in ONE_D])
def test_tap_1d_on_every_path(dtype, path, beta, weighted):
    V = positive_V((10, 3, 60), seed=2, dtype=dtype)
    G = mixed_weights(V.shape, seed=2, dtype=dtype) if weighted else None
    tapped_step(V, G, 8, (20,), beta, path)


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('beta', [2., 1.])
def test_tap_auto_at_a_hybrid_size_with_row_padded_H(beta, weighted):
    V = positive_V((12, 1, 96, 96), seed=3, dtype=np.float32)
    G = mixed_weights(V.shape, seed=3, dtype=np.float32) if weighted else None
    tapped_step(V, G, 32, (12, 12), beta, 'auto', expect_path='split', padded=True)
    tapped_step(V, G, 32, (12, 12), beta, 'auto', h_args=dict(inhibition=0.1, cross_inhibition=0.05),
                expect_path='split', padded=True)


@pytest.mark.parametrize('lateral', [False, True], ids=['plain', 'inhibition'])
@pytest.mark.parametrize('mode', ['valid', 'full', 'circular', 'reflect'])
@pytest.mark.parametrize('beta,weighted', [(2., False), (2., True), (1., False), (0.5, True)])
@pytest.mark.parametrize('dtype,path', [(np.float64, 'generic'), (np.float32, 'auto')], ids=['f64_generic', 'f32_auto'])
def test_tap_modes_and_lateral_terms(dtype, path, beta, weighted, mode, lateral):
    V = positive_V((3, 2, 20, 24), seed=4, dtype=dtype)
    G = mixed_weights(V.shape, seed=4, dtype=dtype) if weighted else None
    h_args = dict(sparsity=0.05, inhibition=0.1, cross_inhibition=0.05) if lateral else {}
    tapped_step(V, G, 5, (4, 5), beta, path, mode=mode, h_args=h_args)


@pytest.mark.parametrize('mode,lateral', [('valid', False), ('valid', True), ('circular', False)])
@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_tap_frobenius_volume(dtype, mode, lateral):
    V = positive_V((3, 2, 5, 6, 70), seed=5, dtype=dtype)
    h_args = dict(sparsity=0.05, inhibition=0.1, cross_inhibition=0.05) if lateral else {}
    a, _ = tapped_step(V, None, 3, (2, 3, 4), 2., mode=mode, h_args=h_args)
    assert a._backend.last_path == 'volume'


def test_tap_with_a_valid_reconstruction_handed_in():
    """tnmf_hip_update_H with r_is_valid: the tap reads the reconstruction the caller brought (the backend's timeline
    mode launches it separately)."""
    V = positive_V((4, 1, 40, 48), seed=6)
    a = model(V, 6, (5, 4))
    W0, H0 = a.W, a.H
    a._backend.start_timeline()
    assert a._update_H(record=True) is None
    a._backend.stop_timeline()
    tap = a._objective_buf.cpu().numpy()
    want = per_sample_reference(V, None, W0, H0, 2.)
    assert np.all(np.abs(tap - want) <= 1e-10 * want)


def test_a_minibatch_slice_writes_its_own_samples_and_no_others():
    V = positive_V((6, 2, 30, 33), seed=7)
    a = model(V, 5, (4, 5), path='generic')
    full, W0, H0 = model(V, 5, (4, 5), path='generic'), a.W, a.H
    assert full._update_H(record=True) is None
    all_samples = full._objective_buf.cpu().numpy()
    be = a._backend
    buf = torch.full((6,), -1., dtype=torch.float64, device='cuda')
    be.fused_update_H(a._V, a._W, a._H, slice(2, 5), objective_out=buf)
    got = buf.cpu().numpy()
    assert np.all(got[[0, 1, 5]] == -1.), 'samples outside the slice are not written'
    # how a sample is cut into blocks depends on C * D alone: the same bits whoever shares the call
    assert np.array_equal(got[2:5], all_samples[2:5])
    want = per_sample_reference(V, None, W0, H0, 2.)
    assert np.all(np.abs(got[2:5] - want[2:5]) <= 1e-10 * want[2:5])
    assert np.array_equal(a.H[[0, 1, 5]], H0[[0, 1, 5]]) and relmax(a.H[2:5], full.H[2:5]) < 1e-12
    # the tap is cleared after the call: a later untapped step writes nothing
    buf.fill_(-2.)
    be.fused_update_H(a._V, a._W, a._H, slice(0, 6))
    assert bool(torch.all(buf == -2.))


def test_the_tap_is_cleared_when_the_step_raises():
    """float64 under path='mfma' has no kernel: the library refuses the step; the tap set for it must not survive."""
    V = positive_V((3, 1, 20, 24), seed=8)
    a = model(V, 4, (4, 5), path='mfma')
    be = a._backend
    buf = be.new_objective_buffer().fill_(-1.)
    with pytest.raises(_lib.TnmfHipError):
        be.fused_update_H(a._V, a._W, a._H, slice(None), objective_out=buf)
    _lib.check(be._lib.tnmf_hip_ctx_set_path(be._ctx, _lib.PATHS['generic']), 'tnmf_hip_ctx_set_path')
    H0 = a.H
    be.fused_update_H(a._V, a._W, a._H, slice(None))
    assert not np.array_equal(a.H, H0)
    assert bool(torch.all(buf == -1.)), 'no tap survives a failed call'


# -- 2. the read-outs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['valid', 'reflect'])
@pytest.mark.parametrize('beta,weighted', [(2., False), (2., True), (1., False), (0., True)])
@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_sample_objective_sums_to_objective_and_follows_V(dtype, beta, weighted, mode):
    V = positive_V((5, 2, 30, 33), seed=9, dtype=dtype)
    G = mixed_weights(V.shape, seed=9, dtype=dtype) if weighted else None
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=6, atom_shape=(5, 4), backend='hip', beta_loss=beta, reconstruction_mode=mode)
    nmf.fit(V, n_iterations=3, progress_callback=CB, weights=G)
    per_sample, total = nmf.sample_objective(), nmf.objective()
    assert per_sample.shape == (5,) and per_sample.dtype == np.float64
    assert total == nmf._energy_function()
    assert abs(per_sample.sum() - total) <= 1e-10 * total
    want = per_sample_reference(V, G, nmf.W, nmf.H, beta, mode)
    assert np.all(np.abs(per_sample - want) <= BAR[dtype] * want), (per_sample, want)
    assert len(set(np.round(want / want.max(), 3))) > 1, 'the samples differ: the order is checked'


def test_sample_objective_of_a_volume():
    V = positive_V((3, 1, 5, 6, 20), seed=10)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=3, atom_shape=(2, 3, 4), backend='hip')
    nmf.fit(V, n_iterations=2, progress_callback=CB)
    per_sample = nmf.sample_objective()
    want = per_sample_reference(V, None, nmf.W, nmf.H, 2.)
    assert np.all(np.abs(per_sample - want) <= 1e-10 * want)
    assert abs(per_sample.sum() - nmf.objective()) <= 1e-10 * nmf.objective()


# -- 3. whole fits ------------------------------------------------------------------------------------------------------
def oracle_trajectory(V, M, A, n, **fit_kw):
    """The float64 trajectory of the objective, run on the CPU by the product front end on the oracle backend."""
    return trajectory(lambda: TransformInvariantNMF(n_atoms=M, atom_shape=A, backend=OracleBackend(hooks=True)),
                      V.astype(np.float64), n, **fit_kw)


# dtype, shape, M, A, iterations, the record that is to decide.  On uniform random samples the decrease per record first
# grows (a plateau behind the first iterations, which remove 99.8 % of the objective of the random initialisation), then
# falls: the tolerance sits between the decrease of the deciding record and the smallest one before it.
FITS = {'f64': (np.float64, (4, 1, 40, 48), 16, (12, 12), 80, 13),
        'f32_hybrid': (np.float32, (8, 1, 64, 64), 16, (9, 9), 60, 9)}


@pytest.mark.parametrize('case', list(FITS))
def test_fit_with_tol_end_to_end(case):
    dtype, shape, M, A, n, j_star = FITS[case]
    V = np.random.default_rng(11).random(shape).astype(dtype)
    every = 5
    E = oracle_trajectory(V, M, A, n, sparsity_H=0.05)
    tol = pick_tol(E, every, j_star)
    n_iter, converged, records = predict(E, every, tol, n)
    assert converged and n_iter == j_star * every + 1

    def fit(tap=True, **kw):
        np.random.seed(42)
        nmf = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip')
        assert nmf._backend.supports_objective_tap
        if not tap:
            nmf._backend.supports_objective_tap = False   # the generic route: an energy evaluation before the iteration
        nmf.fit(V, n_iterations=n, sparsity_H=0.05, **kw)
        return nmf

    seen = []
    twin = fit(progress_callback=lambda m, i: seen.append(m._energy_function()) or i + 1 < n_iter)
    nmf = fit(objective_every=every, tol=tol)
    print(f'{case}: tol={tol:.3e} n_iter_={nmf.n_iter_} (predicted {n_iter}) history={nmf.objective_history_[:, 1]}')
    assert (nmf.n_iter_, nmf.converged_) == (n_iter, True)
    hist = nmf.objective_history_
    np.testing.assert_array_equal(hist[:, 0], [r[0] for r in records])
    # E[i] of the twin: after iteration i - 1 (the initial state is compared with the oracle's)
    twin_at = {i + 1: e for i, e in enumerate(seen)}
    for i, e in hist[1:]:
        assert abs(e - twin_at[int(i)]) <= BAR[dtype] * twin_at[int(i)], (i, e, twin_at[int(i)])
    print(f'{case}: history against the float64 oracle trajectory: {relmax(hist[:, 1], [r[1] for r in records]):.2e}')
    assert abs(hist[0, 1] - E[0]) <= BAR[dtype] * E[0]
    if case == 'f32_hybrid':
        assert nmf._backend.last_path == 'fft', 'the hybrid dispatch'
    generic = fit(tap=False, objective_every=every, tol=tol)
    assert (generic.n_iter_, generic.converged_) == (n_iter, True)
    assert np.all(np.abs(generic.objective_history_[:, 1] - hist[:, 1]) <= BAR[dtype] * hist[:, 1])
    if dtype == np.float64:
        assert relmax(generic.W, nmf.W) <= 1e-12
    assert relmax(nmf.W, twin.W) <= (1e-12 if dtype == np.float64 else 1e-6)


def test_tiny_problem_keeps_its_persistent_kernel_and_stops():
    V = np.random.default_rng(12).random((2, 1, 24, 24))
    n, every = 60, 5
    E = oracle_trajectory(V, 4, (5, 5), n)
    tol = pick_tol(E, every, 5)
    n_iter, converged, records = predict(E, every, tol, n)
    assert converged
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=4, atom_shape=(5, 5), backend='hip')
    nmf.fit(V, n_iterations=n, objective_every=every, tol=tol)
    assert nmf._backend.prefers_schedule(nmf._H) and nmf._backend.last_schedule_persistent
    assert (nmf.n_iter_, nmf.converged_) == (n_iter, True)
    np.testing.assert_array_equal(nmf.objective_history_[:, 0], [r[0] for r in records])
    assert abs(nmf.objective_history_[0, 1] - E[0]) <= 1e-10 * E[0]


_init_lock = threading.Lock()


def test_two_ranks_stop_together():
    V = positive_V((7, 2, 20, 24), seed=13)
    n, every = 40, 4
    E = oracle_trajectory(V, 5, (4, 5), n, sparsity_H=0.05)
    tol = pick_tol(E, every, 4)
    n_iter, converged, _ = predict(E, every, tol, n)
    assert converged

    def fit(pg=None):
        nmf = TransformInvariantNMF(n_atoms=5, atom_shape=(4, 5), backend='hip', process_group=pg)
        plain_init = nmf._initialize_matrices

        def seeded_init(V_, keep_W, **kw):
            with _init_lock:
                np.random.seed(42)
                plain_init(V_, keep_W, **kw)
        nmf._initialize_matrices = seeded_init
        nmf.fit(V, n_iterations=n, sparsity_H=0.05, objective_every=every, tol=tol)
        return nmf

    def rank_body(rank, coll):
        torch.cuda.set_device(0)
        nmf = fit(coll)
        return dict(n_iter=nmf.n_iter_, converged=nmf.converged_, hist=nmf.objective_history_, W=nmf.W,
                    per_sample=nmf.sample_objective(), total=nmf.objective())

    (r0, r1), _group = run_ranks(2, rank_body)
    single = fit()
    assert r0['n_iter'] == r1['n_iter'] == single.n_iter_ == n_iter and r0['converged'] and r1['converged']
    assert np.array_equal(r0['hist'], r1['hist'])
    assert np.all(np.abs(r0['hist'][:, 1] - single.objective_history_[:, 1]) <= 1e-10 * single.objective_history_[:, 1])
    assert relmax(r0['W'], single.W) < 1e-10
    # sample_objective holds this rank's samples, like H
    both = np.concatenate([r0['per_sample'], r1['per_sample']])
    assert both.shape == (7,) and np.all(np.abs(both - single.sample_objective()) <= 1e-10 * both)
    assert abs(both.sum() - r0['total']) <= 1e-10 * r0['total']


# -- 4. refusals --------------------------------------------------------------------------------------------------------
def p(t):
    return ctypes.c_void_p(t.data_ptr())


def test_refusals_answer_before_anything_is_written():
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    _lib.check(lib.tnmf_hip_ctx_create(torch.cuda.current_device(), ctypes.byref(ctx)), 'ctx_create')
    try:
        assert lib.tnmf_hip_ctx_set_objective_tap(None, None) == -1
        cases = (((2, 3, 1, (6, 6, 6), (2, 2, 2)), (2, 3, 7, 7, 7), 2., True, _lib.E_UNSUPPORTED),    # weighted volume
                 ((2, 3, 1, (6, 6, 6), (2, 2, 2)), (2, 3, 7, 7, 7), 1., False, _lib.E_UNSUPPORTED),   # beta on a volume
                 ((2, 3, 1, (8, 8), (3, 3)), (2, 3, 10, 10), float('nan'), False, _lib.E_UNSUPPORTED),
                 ((2, 3, 1, (8, 8), (3, 3)), (2, 3, 10, 10), float('inf'), True, _lib.E_UNSUPPORTED))
        for geom, shape_H, beta, weighted, code in cases:
            n, m, c, D, A = geom
            g = _lib.make_geom(n, m, c, D, A, 1)
            V = torch.rand((n, c) + D, dtype=torch.float64, device='cuda')
            G = torch.ones_like(V)
            W = torch.rand((m, c) + A, dtype=torch.float64, device='cuda')
            H = torch.rand(shape_H, dtype=torch.float64, device='cuda')
            out = torch.full((n,), -1., dtype=torch.float64, device='cuda')
            assert lib.tnmf_hip_sample_objective(ctx, ctypes.byref(g), beta, 1e-9, p(V), p(G) if weighted else None,
                                                 p(W), p(H), p(out), None) == code
            torch.cuda.synchronize()
            assert bool(torch.all(out == -1.))
        # NULL output, NULL operands
        g = _lib.make_geom(2, 3, 1, (8, 8), (3, 3), 1)
        V = torch.rand((2, 1, 8, 8), dtype=torch.float64, device='cuda')
        W = torch.rand((3, 1, 3, 3), dtype=torch.float64, device='cuda')
        H = torch.rand((2, 3, 10, 10), dtype=torch.float64, device='cuda')
        out = torch.full((2,), -1., dtype=torch.float64, device='cuda')
        gp = ctypes.byref(g)
        assert lib.tnmf_hip_sample_objective(ctx, gp, 2., 1e-9, p(V), None, p(W), p(H), None, None) == -1
        assert lib.tnmf_hip_sample_objective(ctx, gp, 2., 1e-9, None, None, p(W), p(H), p(out), None) == -1
        assert lib.tnmf_hip_sample_objective(ctx, None, 2., 1e-9, p(V), None, p(W), p(H), p(out), None) == -1
        torch.cuda.synchronize()
        assert bool(torch.all(out == -1.))
        # ... and the call itself, with the tap set and cleared by hand around a plain step
        assert lib.tnmf_hip_sample_objective(ctx, gp, 2., 1e-9, p(V), None, p(W), p(H), p(out), None) == 0
        tap = torch.full((2,), -1., dtype=torch.float64, device='cuda')
        assert lib.tnmf_hip_ctx_set_objective_tap(ctx, p(tap)) == 0
        assert lib.tnmf_hip_update_H(ctx, gp, p(V), p(W), p(H), None, 0, 1e-9, 0., None) == 0
        assert lib.tnmf_hip_ctx_set_objective_tap(ctx, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(tap, out), 'the tap and the read-out run the same kernel on the same reconstruction'
    finally:
        lib.tnmf_hip_ctx_destroy(ctx)
