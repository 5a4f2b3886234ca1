"""
Detections on the GPU: tnmf_hip_find_peaks through the C ABI, HIP_Backend.find_peaks and ``detections()`` on
``backend='hip'``, against the brute-force reference tests/peaks_reference.py.  Exact: equal index arrays, bit-equal values.
"""
import ctypes
import functools
import threading

import numpy as np
import pytest
import torch

import peaks_reference as pref
from local_collective import run_ranks
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

pytestmark = pytest.mark.gpu

SENTINEL_IDX, SENTINEL_VAL, PAD_VALUE = -7, -3., 9.
NP_DTYPES = {0: np.float32, 1: np.float64}
TORCH_DTYPES = {0: torch.float32, 1: torch.float64}


def p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope='module')
def ctx():
    lib = _lib.load()
    c = ctypes.c_void_p()
    _lib.check(lib.tnmf_hip_ctx_create(torch.cuda.current_device(), ctypes.byref(c)), 'ctx_create')
    yield c
    lib.tnmf_hip_ctx_destroy(c)


@functools.lru_cache(maxsize=None)
def tie_rich(shape, seed=0):
    """Integer-valued entries 0..5, about 70 % zeros (float64; exact in float32 too): ties and plateaus are common."""
    rng = np.random.default_rng(seed)
    H = np.where(rng.random(shape) < 0.7, 0, rng.integers(1, 6, shape)).astype(np.float64)
    H.setflags(write=False)
    return H


@functools.lru_cache(maxsize=None)
def reference(shape, seed, threshold, radius, group):
    """The reference's detections of tie_rich(shape, seed), computed once per case and shared (the two element types hold
    the same integers).  A case that detects nothing, or everything, would test nothing."""
    idx, val = pref.find_peaks(tie_rich(shape, seed), threshold, radius, group)
    assert 0 < len(idx) < int(np.prod(shape)), (shape, threshold, radius, group, len(idx))
    idx.setflags(write=False)
    return idx


def on_device(H, dtype, stride=None):
    """(storage, row stride for the geometry): H on the device, its rows `stride` apart with the pad columns holding a
    value larger than any entry of H."""
    t = torch.from_numpy(np.array(H)).to('cuda', TORCH_DTYPES[dtype])
    if stride is None:
        return t, 0
    store = torch.full(tuple(H.shape[:-1]) + (stride,), PAD_VALUE, dtype=TORCH_DTYPES[dtype], device='cuda')
    store[..., :H.shape[-1]] = t
    return store, stride


def find(ctx, store, shape, dtype, stride, threshold, radius, group, capacity, expect_rc=0):
    """One call of tnmf_hip_find_peaks with output buffers 64 elements longer than `capacity`, prefilled with sentinels.
    -> (count, idx[:capacity], val[:capacity]) on the host, after checking that the tail is untouched."""
    lib = _lib.load()
    k = len(shape) - 2
    g = _lib.make_geom(shape[0], shape[1], 1, shape[2:], (1,) * k, dtype, stride)
    idx = torch.full((capacity + 64,), SENTINEL_IDX, dtype=torch.int64, device='cuda')
    val = torch.full((capacity + 64,), SENTINEL_VAL, dtype=TORCH_DTYPES[dtype], device='cuda')
    count = torch.full((1,), -1, dtype=torch.int64, device='cuda')
    rad = (ctypes.c_int * 3)(*radius)
    rc = lib.tnmf_hip_find_peaks(ctx, ctypes.byref(g), p(store), float(threshold), rad, group, p(idx), p(val), capacity,
                                 p(count), None)
    torch.cuda.synchronize()
    assert rc == expect_rc, rc
    idx, val, count = idx.cpu().numpy(), val.cpu().numpy(), int(count.item())
    assert np.all(idx[capacity:] == SENTINEL_IDX) and np.all(val[capacity:] == SENTINEL_VAL), 'written beyond capacity'
    if rc != 0:
        assert count == -1 and np.all(idx == SENTINEL_IDX) and np.all(val == SENTINEL_VAL), 'a refused call wrote'
    return count, idx[:capacity], val[:capacity]


def check_case(ctx, shape, seed, dtype, stride, threshold, radius, group):
    H = tie_rich(shape, seed)
    want = reference(shape, seed, threshold, radius, group)
    store, ld = on_device(H, dtype, stride)
    count, idx, val = find(ctx, store, shape, dtype, ld, threshold, radius, group, capacity=len(want) + 5)
    assert count == len(want)
    order = np.argsort(idx[:count])
    np.testing.assert_array_equal(idx[:count][order], want)
    assert val[:count][order].tobytes() == H.reshape(-1)[want].astype(NP_DTYPES[dtype]).tobytes()
    assert np.all(idx[count:] == SENTINEL_IDX)


# -- the kernel through the C ABI -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [0, 1], ids=['f32', 'f64'])
@pytest.mark.parametrize('group', [1, 4, 8])
@pytest.mark.parametrize('radius', [(3, 5), (0, 0), (40, 40)], ids=str)
@pytest.mark.parametrize('threshold', [0., 2.])
def test_2d_row_padded(ctx, threshold, radius, group, dtype):
    """Rows of 37 entries 64 apart, the pad columns larger than any entry: never a neighbour, never reported."""
    check_case(ctx, (3, 8, 19, 37), 1, dtype, 64, threshold, radius, group)


@pytest.mark.parametrize('dtype', [0, 1], ids=['f32', 'f64'])
@pytest.mark.parametrize('threshold', [0., 2.])
def test_2d_contiguous_full_rows(ctx, threshold, dtype):
    check_case(ctx, (2, 3, 33, 32), 2, dtype, None, threshold, (2, 3), 1)
    check_case(ctx, (2, 3, 33, 32), 2, dtype, None, threshold, (1, 40), 3)


@pytest.mark.parametrize('dtype', [0, 1], ids=['f32', 'f64'])
@pytest.mark.parametrize('threshold', [0., 2.])
def test_2d_over_several_workgroups(ctx, threshold, dtype):
    check_case(ctx, (2, 3, 70, 130), 3, dtype, None, threshold, (11, 11), 1)


@pytest.mark.parametrize('dtype', [0, 1], ids=['f32', 'f64'])
@pytest.mark.parametrize('radius', [0, 63])
@pytest.mark.parametrize('threshold', [0., 2.])
def test_1d(ctx, threshold, radius, dtype):
    check_case(ctx, (2, 5, 300), 4, dtype, None, threshold, (radius,), 1)
    check_case(ctx, (2, 5, 300), 4, dtype, None, threshold, (radius,), 5)


@pytest.mark.parametrize('threshold', [0., 2.])
@pytest.mark.parametrize('group', [1, 2])
def test_3d(ctx, threshold, group):
    check_case(ctx, (2, 4, 6, 7, 9), 5, 0, None, threshold, (1, 2, 3), group)


def test_capacity(ctx):
    shape, args = (3, 8, 19, 37), (0., (3, 5), 1)
    H = tie_rich(shape, 1)
    want = reference(shape, 1, *args)
    for dtype in (0, 1):
        store, ld = on_device(H, dtype, 64)
        for capacity in (len(want) // 3, 1, 0):
            count, idx, val = find(ctx, store, shape, dtype, ld, *args, capacity=capacity)
            assert count == len(want), 'the counter keeps counting past the capacity'
            assert len(set(idx.tolist())) == capacity and set(idx.tolist()) <= set(want.tolist())
            assert val.tobytes() == H.reshape(-1)[idx].astype(NP_DTYPES[dtype]).tobytes()
        lib = _lib.load()   # capacity 0 takes NULL lists
        g = _lib.make_geom(shape[0], shape[1], 1, shape[2:], (1, 1), dtype, ld)
        count = torch.full((1,), -1, dtype=torch.int64, device='cuda')
        assert lib.tnmf_hip_find_peaks(ctx, ctypes.byref(g), p(store), 0., (ctypes.c_int * 3)(3, 5, 0), 1, None, None, 0,
                                       p(count), None) == 0
        assert int(count.item()) == len(want)
        zeros = torch.zeros(shape, dtype=TORCH_DTYPES[dtype], device='cuda')
        count, idx, _ = find(ctx, zeros, shape, dtype, 0, *args, capacity=16)
        assert count == 0 and np.all(idx == SENTINEL_IDX)


def test_bad_arguments_write_nothing(ctx):
    shape = (2, 6, 10, 12)
    store, _ = on_device(tie_rich(shape, 6), 0)
    E_NULL, E_DTYPE = -1, -3
    for radius, group, rc in (((-1, 0), 1, _lib.E_GEOM), ((0, -3), 1, _lib.E_GEOM), ((1, 1), 4, _lib.E_GEOM),
                              ((1, 1), 0, _lib.E_GEOM), ((1, 1), -2, _lib.E_GEOM), ((1, 1), 12, _lib.E_GEOM)):
        find(ctx, store, shape, 0, 0, 0., radius, group, capacity=32, expect_rc=rc)
    find(ctx, store, shape, 0, 5, 0., (1, 1), 1, capacity=32, expect_rc=_lib.E_GEOM)      # rows closer than their width
    find(ctx, store, shape, 0, 0, -1., (1, 1), 1, capacity=32, expect_rc=_lib.E_UNSUPPORTED)
    find(ctx, store, shape, 0, 0, float('nan'), (1, 1), 1, capacity=32, expect_rc=_lib.E_UNSUPPORTED)
    lib = _lib.load()
    g = _lib.make_geom(2, 6, 1, (10, 12), (1, 1), 0)
    rad = (ctypes.c_int * 3)(1, 1, 0)
    idx = torch.full((8,), SENTINEL_IDX, dtype=torch.int64, device='cuda')
    val = torch.full((8,), SENTINEL_VAL, dtype=torch.float32, device='cuda')
    count = torch.full((1,), -1, dtype=torch.int64, device='cuda')
    gp = ctypes.byref(g)
    assert lib.tnmf_hip_find_peaks(None, gp, p(store), 0., rad, 1, p(idx), p(val), 8, p(count), None) == E_NULL
    assert lib.tnmf_hip_find_peaks(ctx, None, p(store), 0., rad, 1, p(idx), p(val), 8, p(count), None) == E_NULL
    assert lib.tnmf_hip_find_peaks(ctx, gp, None, 0., rad, 1, p(idx), p(val), 8, p(count), None) == E_NULL
    assert lib.tnmf_hip_find_peaks(ctx, gp, p(store), 0., None, 1, p(idx), p(val), 8, p(count), None) == E_NULL
    assert lib.tnmf_hip_find_peaks(ctx, gp, p(store), 0., rad, 1, None, p(val), 8, p(count), None) == E_NULL
    assert lib.tnmf_hip_find_peaks(ctx, gp, p(store), 0., rad, 1, p(idx), None, 8, p(count), None) == E_NULL
    assert lib.tnmf_hip_find_peaks(ctx, gp, p(store), 0., rad, 1, p(idx), p(val), 8, None, None) == E_NULL
    g.dtype = 2
    assert lib.tnmf_hip_find_peaks(ctx, gp, p(store), 0., rad, 1, p(idx), p(val), 8, p(count), None) == E_DTYPE
    torch.cuda.synchronize()
    assert int(count.item()) == -1 and bool(torch.all(idx == SENTINEL_IDX)) and bool(torch.all(val == SENTINEL_VAL))


# -- the backend ------------------------------------------------------------------------------------------------------------
def hip_model(V, n_atoms, atom_shape, n_iterations=1, seed=42, **kw):
    fit_kw = {k: kw.pop(k) for k in ('sparsity_H', 'update_W') if k in kw}
    np.random.seed(seed)
    nmf = TransformInvariantNMF(n_atoms=n_atoms, atom_shape=atom_shape, backend='hip', **kw)
    nmf.fit(V, n_iterations=n_iterations, **fit_kw)
    return nmf


@pytest.mark.parametrize('padded', [False, True], ids=['contiguous', 'row-padded'])
def test_a_minibatch_slice_equals_the_slice_copied_out(padded):
    nmf = hip_model(np.random.default_rng(0).random((2, 1, 12, 12)).astype(np.float32), 2, (3, 3))
    be = nmf._backend
    shape = (5, 4, 19, 37)
    Hn = tie_rich(shape, 7)
    store, _ = on_device(Hn, 0, 64 if padded else None)
    H = store[..., :37] if padded else store
    assert H.is_contiguous() != padded
    view = H[1:3]
    want_idx, want_val = pref.find_peaks(Hn[1:3].astype(np.float32), 0., (2, 3), 2)
    assert 0 < len(want_idx) < Hn[1:3].size
    for arg in (view, view.clone()):
        idx, val = be.find_peaks(arg, 0., (2, 3), 2)
        np.testing.assert_array_equal(idx, want_idx)
        assert val.tobytes() == want_val.tobytes()
    # a capacity guess below the count: one more run with the exact size, the same answer
    idx, val = be.find_peaks(view, 0., (2, 3), 2, capacity=7)
    np.testing.assert_array_equal(idx, want_idx)
    assert val.tobytes() == want_val.tobytes()
    idx, val = be.find_peaks(H[0:0], 0., (2, 3), 2)
    assert idx.shape == (0,) and idx.dtype == np.int64 and val.shape == (0,) and val.dtype == np.float32


# -- end to end -------------------------------------------------------------------------------------------------------------
def check_model(nmf, threshold, min_distance, suppress='atom', max_per_sample=None):
    assert nmf._backend.supports_peaks
    H = nmf.H
    T = nmf.n_transforms
    k = len(nmf.atom_shape)
    radius = nmf._inhibition_range if min_distance is None else \
        (min_distance,) * k if isinstance(min_distance, int) else min_distance
    group = {'atom': 1, 'transforms': T, 'all': nmf._H.shape[1]}[suppress]
    want = pref.detections(H, threshold, radius, group, nmf.atom_shape, nmf._backend._reconstruction_mode, T,
                           max_per_sample)
    assert 0 < len(want['sample']) < H.size
    det = nmf.detections(threshold=threshold, min_distance=min_distance, suppress=suppress,
                         max_per_sample=max_per_sample)
    pref.assert_equal(det, want)
    assert det.strength.dtype == H.dtype
    return det


@pytest.mark.parametrize('mode', ['valid', 'circular'])
@pytest.mark.parametrize('case', ['2d-f32', '1d-f64'])
def test_fit_then_detections(case, mode):
    rng = np.random.default_rng(21)
    if case == '2d-f32':
        V, M, A = rng.random((3, 2, 24, 30)).astype(np.float32), 4, (5, 6)
    else:
        V, M, A = rng.random((4, 1, 120)), 3, (9,)
    nmf = hip_model(V, M, A, n_iterations=5, sparsity_H=0.1, reconstruction_mode=mode)
    t = float(np.quantile(nmf.H, 0.6))
    check_model(nmf, t, None)
    check_model(nmf, t, None, max_per_sample=5)
    check_model(nmf, 0., 1, suppress='all')
    check_model(nmf, 0., 1, suppress='all', max_per_sample=3)


def test_fit_with_rot90_then_the_winning_orientation():
    V = np.random.default_rng(22).random((3, 1, 20, 22)).astype(np.float32)
    nmf = hip_model(V, 2, (4, 4), n_iterations=5, sparsity_H=0.1, transforms='rot90')
    assert nmf.H.shape == (3, 2, 4, 23, 25)
    t = float(np.quantile(nmf.H, 0.5))
    det = check_model(nmf, t, None, suppress='transforms')
    assert set(det.transform.tolist()) <= {0, 1, 2, 3} and set(det.atom.tolist()) <= {0, 1}
    check_model(nmf, t, (2, 2), suppress='transforms', max_per_sample=4)
    check_model(nmf, t, (2, 2), suppress='atom')


_init_lock = threading.Lock()


def test_two_ranks_report_their_shards_of_the_single_process_detections():
    # (W fixed: every sample's activations then depend on that sample alone, so the shards hold the single process's bits)
    V = np.random.default_rng(23).random((8, 1, 64, 64)).astype(np.float32)

    def fit(pg=None):
        nmf = TransformInvariantNMF(n_atoms=8, atom_shape=(5, 5), backend='hip', process_group=pg)
        plain_init = nmf._initialize_matrices

        def seeded_init(V_, keep_W, **kw):
            with _init_lock:
                np.random.seed(42)
                plain_init(V_, keep_W, **kw)
        nmf._initialize_matrices = seeded_init
        nmf.fit(V, n_iterations=5, sparsity_H=0.1, update_W=False)
        return nmf

    single = fit()
    t = float(np.quantile(single.H, 0.95))
    want = check_model(single, t, None, max_per_sample=6)

    def rank_body(rank, coll):
        torch.cuda.set_device(0)
        nmf = fit(coll)
        return nmf._backend.shard, nmf.detections(threshold=t, max_per_sample=6)

    ((s0, d0), (s1, d1)), _group = run_ranks(2, rank_body)
    assert s0 == (0, 4) and s1 == (4, 8)
    assert set(d0.sample.tolist()) <= set(range(0, 4)) and set(d1.sample.tolist()) <= set(range(4, 8))
    for name in ('sample', 'atom', 'transform', 'shift', 'origin'):
        np.testing.assert_array_equal(np.concatenate([getattr(d0, name), getattr(d1, name)]), getattr(want, name))
    assert np.concatenate([d0.strength, d1.strength]).tobytes() == want.strength.tobytes()
