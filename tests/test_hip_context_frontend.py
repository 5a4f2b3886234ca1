"""The front end on a USED backend: one HIP_Backend (one tnmf_hip_ctx) carries a first fit, then a second, different one,
and is then asked for atom_gains(), atom_gram(), separate() and activation_correlogram().  A fresh backend given the second
fit alone must compute the same bits: W, H and all four results.  This drives HIP_Backend._initialize_matrices on a live
context -- _foreign_H, bind, reserve, the reset of the weights, _R_scratch and _negpos -- where the C ABI tier
(tests/test_hip_context_matrix.py) drives the library alone.

init='reference' draws from NumPy's global generator: it is seeded before every fit, so a fit's start does not depend on
what was fitted before it."""
import numpy as np
import pytest
import torch

import context_dispatch as cx
from test_atom_gains_cpu import weights_of
from tnmf_amd.backends.HIP import HIP_Backend
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

pytestmark = pytest.mark.gpu

ITERATIONS = 3
SMALL, LARGE = cx.GEOMETRY[('2d', cx.SMALL)], cx.GEOMETRY[('2d', cx.LARGE)]
ONE_D = cx.GEOMETRY[('1d', cx.SMALL)]


def samples(geometry, dtype, seed):
    N, C, D, M, A = geometry
    return (np.random.default_rng(seed).random((N, C) + D) + 0.05).astype(dtype)


def fit(backend, geometry, dtype, seed, model=None, weighted=False, keep_W=False, **model_kw):
    """One fit of ITERATIONS iterations on `backend` -> the model (a new one unless `model` is refitted)."""
    N, C, D, M, A = geometry
    V = samples(geometry, dtype, seed)
    G = weights_of(V.shape, 'real').astype(dtype) if weighted else None
    if model is None:
        model = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend=backend, **model_kw)
    np.random.seed(1000 + seed)
    model.fit(V, n_iterations=ITERATIONS, sparsity_H=0.1, weights=G, keep_W=keep_W)
    return model


def results(model):
    torch.cuda.synchronize()
    return dict(W=model.W, H=model.H, gains=model.atom_gains(per_sample=True), gram=model.atom_gram(per_sample=True),
                separate=model.separate(), correlogram=model.activation_correlogram(per_sample=True))


def same_bits(used, fresh):
    assert sorted(used) == sorted(fresh)
    for key in used:
        a, b = np.ascontiguousarray(used[key]), np.ascontiguousarray(fresh[key])
        assert a.dtype == b.dtype and a.shape == b.shape, key
        assert np.all(np.isfinite(a)), key
        print(f'    {key}: {a.dtype} {a.shape}, largest entry {float(np.abs(a).max()):.6g}')
        assert a.tobytes() == b.tobytes(), (key, 'a used backend differs from a fresh one', float(np.abs(a - b).max()))


def test_float32_2d_kl_weighted_then_float64_1d_frobenius():
    used = HIP_Backend()
    fit(used, SMALL, np.float32, 1, weighted=True, beta_loss=1.)
    second = fit(used, ONE_D, np.float64, 2)
    same_bits(results(second), results(fit(HIP_Backend(), ONE_D, np.float64, 2)))


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_small_then_large(dtype):
    used = HIP_Backend()
    fit(used, SMALL, dtype, 3)
    second = fit(used, LARGE, dtype, 4)
    same_bits(results(second), results(fit(HIP_Backend(), LARGE, dtype, 4)))


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_large_then_small_keeping_W(dtype):
    geometry = SMALL[:3] + LARGE[3:]                # (the small samples under the large problem's dictionary)
    used = HIP_Backend()
    model = fit(used, LARGE, dtype, 5)
    W1 = model.W
    fit(used, geometry, dtype, 6, model=model, keep_W=True)
    fresh_backend = HIP_Backend()
    fresh = TransformInvariantNMF(n_atoms=LARGE[3], atom_shape=LARGE[4], backend=fresh_backend)
    fresh._W = torch.from_numpy(W1).cuda()
    fit(fresh_backend, geometry, dtype, 6, model=fresh, keep_W=True)
    same_bits(results(model), results(fresh))


def test_rot90_then_no_transforms():
    geometry = (2, 1, (12, 20), 3, (3, 3))          # (a rotation by 90 degrees wants square atoms)
    used = HIP_Backend()
    fit(used, geometry, np.float32, 7, transforms='rot90')
    second = fit(used, geometry, np.float32, 8)
    same_bits(results(second), results(fit(HIP_Backend(), geometry, np.float32, 8)))
