"""
k_find_peaks in the plain form the product runs, every branch of it: each call of peaks_dispatch.MATRIX is chosen with
the host mirror of the launch (tests/peaks_dispatch.py) so that together with the calls of tests/test_hip_peaks.py they
execute every named branch (tests/test_peaks_dispatch_cpu.py checks that without a GPU): both grid loops striding, each
thinning test alone, windows two and three entries wide, a 2-D window wider than a wave, a threshold that float32 rounds
up, and inputs with NaN and +inf.  The plane-stride calls are sized from the CU count of the device the test runs on, and
the mirror is asked whether they stride there.

Exact throughout, against the brute-force reference tests/peaks_reference.py: equal index arrays, bit-equal values.
"""
import functools

import numpy as np
import pytest
import torch

import peaks_dispatch as pd
import peaks_reference as pref
from test_hip_peaks import NP_DTYPES, SENTINEL_IDX, check_case, ctx, find, hip_model, on_device, reference, tie_rich  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize('dtype', [0, 1], ids=['f32', 'f64'])


@functools.lru_cache(maxsize=None)
def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# -- tie-rich inputs ------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize('name', list(pd.MATRIX))
def test_matrix_call(ctx, name, dtype):
    cu = device_cus()
    shape, seed, stride, threshold, radius, group = pd.call_of(name, cu)
    got = pd.reached(shape, radius, group, stride, threshold, dtype, cu)
    assert set(pd.MATRIX[name][6]) <= got, (name, cu, sorted(set(pd.MATRIX[name][6]) - got))
    check_case(ctx, shape, seed, dtype, stride, threshold, radius, group)


def test_some_plane_stride_call_changes_the_place_in_the_group():
    """On this device's grid: a workgroup's second plane has another place in its suppression group than its first."""
    cu = device_cus()
    calls = [pd.call_of(name, cu) for name in pd.MATRIX if name.startswith('plane-stride')]
    assert any(pd.launch(shape, radius, group, stride, cu).qc_changes for shape, _, stride, _, radius, group in calls), cu


def check_input(ctx, H, want, dtype, stride, threshold, radius, group):
    """check_case of tests/test_hip_peaks.py on an input of the caller's: H float64 of values the element type holds."""
    store, ld = on_device(H, dtype, stride)
    count, idx, val = find(ctx, store, H.shape, dtype, ld, threshold, radius, group, capacity=len(want) + 5)
    assert count == len(want)
    order = np.argsort(idx[:count])
    np.testing.assert_array_equal(idx[:count][order], want)
    assert val[:count][order].tobytes() == H.reshape(-1)[want].astype(NP_DTYPES[dtype]).tobytes()
    assert np.all(idx[count:] == SENTINEL_IDX)


# -- P6: a threshold that is no float32 ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ulp_input(dtype):
    """(H, the reference's detections): entries drawn from 0, 5, float32(0.1) -- above the threshold 0.1 --, its predecessor
    -- below it -- and its successor; for float64 also 0.1 itself, which is not above it.  Radius 0: the pure threshold,
    decided by the reference in float64, which holds every entry exactly."""
    t32 = np.float32(pd.ULP_THRESHOLD)
    values = [0., 5., float(t32), float(np.nextafter(t32, np.float32(0))), float(np.nextafter(t32, np.float32(1)))]
    assert values[3] < pd.ULP_THRESHOLD < values[2] < values[4]
    if dtype == 1:
        values.append(pd.ULP_THRESHOLD)
    rng = np.random.default_rng(17)
    H = np.array(values)[rng.integers(0, len(values), pd.ULP_SHAPE)]
    want, _ = pref.find_peaks(H, pd.ULP_THRESHOLD, (0, 0), 1)
    above = np.isin(H.reshape(-1), [values[1], values[2], values[4]])
    assert np.array_equal(want, np.flatnonzero(above)) and 0 < len(want) < H.size
    for v in values:
        assert np.count_nonzero(H == v) > 100
    H.setflags(write=False)
    want.setflags(write=False)
    return H, want


@DTYPES
def test_threshold_between_two_float32(ctx, dtype):
    H, want = ulp_input(dtype)
    assert ('P6:threshold-rounded-down' in pd.reached(H.shape, (0, 0), 1, None, pd.ULP_THRESHOLD, dtype)) == (dtype == 0)
    check_input(ctx, H, want, dtype, None, pd.ULP_THRESHOLD, (0, 0), 1)
    check_input(ctx, H, want, dtype, 128, pd.ULP_THRESHOLD, (0, 0), 1)


# -- P7: NaN is never a detection and never a suppressor; +inf is an ordinary largest value -----------------------------------
@functools.lru_cache(maxsize=None)
def nan_inf_input():
    """A tie-rich input with about 1 % NaN, NaN beside some of its maxima, and +inf beside others: to the right of one,
    to the left of one, below one, above one, and two +inf side by side (the lower index wins the tie)."""
    H = np.array(tie_rich(pd.NAN_INF_SHAPE, 18))
    rng = np.random.default_rng(19)
    H[rng.random(H.shape) < 0.01] = np.nan
    n, q, y, x = np.nonzero(H[:, :, 1:-1, 1:-2] == 5.)
    picks = rng.choice(len(n), 14, replace=False)
    for i, (dy, dx, v) in zip(picks, [(0, 1, np.inf), (0, -1, np.inf), (1, 0, np.inf), (-1, 0, np.inf), (0, 1, np.nan),
                                      (0, -1, np.nan), (1, 0, np.nan), (-1, 0, np.nan), (0, 1, np.inf), (0, -1, np.inf),
                                      (1, 0, np.inf), (-1, 0, np.inf), (0, 1, np.nan), (1, 0, np.nan)]):
        H[n[i], q[i], y[i] + 1 + dy, x[i] + 1 + dx] = v
    i = picks[0]
    H[n[i], q[i], y[i] + 1, x[i] + 2:x[i] + 4] = np.inf            # ... and a second +inf behind the first
    assert 0.005 < np.isnan(H).mean() < 0.02 and 8 <= np.isinf(H).sum() <= 12
    H.setflags(write=False)
    return H


@functools.lru_cache(maxsize=None)
def nan_inf_reference(radius, group, threshold):
    H = nan_inf_input()
    want, val = pref.find_peaks(H, threshold, radius, group)
    assert 0 < len(want) < H.size and not np.isnan(val).any() and np.isinf(val).any()
    want.setflags(write=False)
    return want


@DTYPES
@pytest.mark.parametrize('radius,group', pd.NAN_INF_CALLS, ids=str)
def test_nan_and_inf(ctx, radius, group, dtype):
    H = nan_inf_input()
    for threshold in (0., 2.):
        check_input(ctx, H, nan_inf_reference(radius, group, threshold), dtype, None, threshold, radius, group)


# -- P8: the backend's second run with the counted size -----------------------------------------------------------------------
@pytest.mark.parametrize('padded', [False, True], ids=['contiguous', 'row-padded'])
def test_a_capacity_too_small_returns_what_the_default_returns(padded):
    nmf = hip_model(np.random.default_rng(0).random((2, 1, 12, 12)).astype(np.float32), 2, (3, 3))
    be = nmf._backend
    shape, args = (3, 8, 19, 37), (0., (3, 5), 2)
    want = reference(shape, 1, *args)
    assert len(want) > 1
    store, _ = on_device(tie_rich(shape, 1), 0, 64 if padded else None)
    H = store[..., :37] if padded else store
    idx, val = be.find_peaks(H, *args)
    np.testing.assert_array_equal(idx, want)
    for capacity in (1, len(want) - 1, len(want)):
        idx1, val1 = be.find_peaks(H, *args, capacity=capacity)
        np.testing.assert_array_equal(idx1, idx)
        assert val1.dtype == val.dtype and val1.tobytes() == val.tobytes()
