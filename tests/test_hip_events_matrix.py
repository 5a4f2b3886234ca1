"""
The events kernels, every branch of them: each case of events_dispatch.MATRIX is chosen with the host mirror of
k_events_render, k_events_update, k_events_grad_W and k_events_grad_W_sum (tests/events_dispatch.py) so that together they
execute every named branch of the four (tests/test_events_dispatch_cpu.py checks that without a GPU) -- the second pass of
every loop, every clamp, every seam of the sub-lane scheme.  The two stride cases are sized from the CU count of the device
the test runs on, and the mirror is asked whether they stride there.

Everything is integer-valued (W and V in 0..3, strengths 1..4), so nothing needs a tolerance of its own: the render is
compared EXACTLY with tests/events_reference.py, the W gradient bit for bit with tests/events_w_reference.py rounded once to
the element type, both over poisoned outputs and a second time; one multiplicative update of the strengths is held to one
step of the reference at the per-strength bars of tests/test_hip_events.py.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import events_dispatch as ed
import events_reference as eref
import events_w_reference as wref
from test_hip_events import BAR, DTYPES, NP, dev
from tnmf_amd import _lib
from tnmf_amd.backends.HIP import HIP_Backend

pytestmark = pytest.mark.gpu

EPS = 1e-9


def p(t):
    return ctypes.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def backend(N, C, P, D, A, mode, dt):
    """An initialised backend of this geometry whose resident samples the tests overwrite (be._V_dev).  Initialised on the
    device: the host stream of tests/test_hip_events.py::backend makes one copy per sample, and 'many-tiles' has 16 421."""
    be = HIP_Backend(reconstruction_mode=mode, init='device')
    be.initialize(np.ones((N, C) + D, dtype=NP[dt]), A, P, None, tuple(range(-len(A), 0)))
    return be


@functools.lru_cache(maxsize=None)
def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def integer_problem(name, num_cu=ed.NUM_CU):
    """(V, R, the reference gradient [2, P, C, *A]) of the matrix case, float64, read-only: integers that both element types
    hold exactly (R below 2^20, the gradient below 2^52)."""
    (N, C, P, D, A, mode), sample, plane, shift, h, W = ed.matrix_case(name, num_cu)
    V = np.random.default_rng(32).integers(0, 4, (N, C) + D).astype(np.float64)
    R = eref.render(W, D, N, mode, sample, plane, shift, h)
    assert R.max() < 2 ** 20 and R.any()
    want = wref.grad_W(V, R, W, D, mode, sample, plane, shift, h)
    assert want.max() < 2 ** 52 and want[0].any() and want[1].any()
    for a in (V, R, want):
        a.setflags(write=False)
    return V, R, want


@functools.lru_cache(maxsize=None)
def reference_step(name, num_cu=ed.NUM_CU):
    """(the integer strengths with one of them 0, the strengths after one step of the reference from them)."""
    (N, C, P, D, A, mode), sample, plane, shift, h, W = ed.matrix_case(name, num_cu)
    V, _, _ = integer_problem(name, num_cu)
    start = np.array(h)
    start[1] = 0.   # stays 0
    out = eref.refit(V, W, mode, sample, plane, shift, start, 1, 0., EPS)
    for a in (start, out):
        a.setflags(write=False)
    return start, out


def lists_of(be, n_planes, sample, plane, shift, h):
    """-> (checked strengths, images, cell_start, events, (by_plane, plane_start, workspace)) on the device."""
    s, pl, sh, hh = be._check_events(n_planes, sample, plane, shift, h)
    images, cell_start, events = be.event_list(s, pl, sh)
    return hh, images, cell_start, events, be.event_plane_list(pl, n_planes)


@pytest.mark.parametrize('name', list(ed.MATRIX))
def test_the_case_reaches_its_branches_on_this_device(name):
    """What the case is there for, by the mirror, with the CU count of this device -- the stride cases stride here."""
    cu = device_cus()
    geo, sample, plane, shift, _, _ = ed.matrix_case(name, cu)
    got = ed.reached(geo, sample, plane, shift, cu)
    for kernel, names in ed.MATRIX[name][1].items():
        assert set(names) <= got[kernel], (name, kernel, cu, sorted(set(names) - got[kernel]))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', list(ed.MATRIX))
def test_render_of_integers_is_exact(name, dt):
    cu = device_cus()
    geo, sample, plane, shift, h, W = ed.matrix_case(name, cu)
    N, C, P, D, A, mode = geo
    be = backend(*geo, dt)
    _, want, _ = integer_problem(name, cu)
    Wd = dev(W, dt)
    hh, images, cell_start, _, _ = lists_of(be, P, sample, plane, shift, h)
    # the lists the kernel walks are the ones the mirror counted its runs on
    counts = ed.cell_counts(geo, sample, shift)
    assert images.shape[0] == counts.sum()
    assert np.array_equal(np.diff(cell_start.cpu().numpy()), counts.reshape(-1))
    R = be.render_event_list(Wd, images, cell_start, hh)
    assert R.dtype == be._torch_dtype and tuple(R.shape) == want.shape
    assert np.array_equal(R.cpu().numpy().astype(np.float64), want)
    # over a poisoned buffer: every pixel is written, zeros included; and the same bits again
    poisoned = torch.full_like(R, float('nan'))
    be.render_event_list(Wd, images, cell_start, hh, poisoned)
    assert torch.equal(poisoned, R)
    assert torch.equal(be.render_event_list(Wd, images, cell_start, hh), R)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', list(ed.MATRIX))
def test_gradient_of_integers_is_the_reference_rounded_once(name, dt):
    cu = device_cus()
    geo, sample, plane, shift, h, W = ed.matrix_case(name, cu)
    N, C, P, D, A, mode = geo
    be = backend(*geo, dt)
    V, R, want = integer_problem(name, cu)
    be._V_dev.copy_(dev(V, dt))
    Wd, Rd = dev(W, dt), dev(R, dt)
    hh, _, _, events, lists = lists_of(be, P, sample, plane, shift, h)
    by_plane, plane_start, workspace = lists
    assert np.array_equal(np.diff(plane_start.cpu().numpy()), ed.plane_counts(geo, plane))
    assert workspace.numel() == ed.events_grad_W_slabs(len(sample), P) * 2 * C * int(np.prod(A))
    got = be.gradient_W_event_list(Wd, events, lists, hh, Rd)
    assert got.dtype == be._torch_dtype and tuple(got.shape) == (2, P, C) + A
    assert got.cpu().numpy().tobytes() == want.astype(NP[dt]).tobytes()
    # over a poisoned output and workspace: every element is written, none is read; and the same bits again
    workspace.fill_(float('nan'))
    poisoned = torch.full_like(got, float('nan'))
    g = _lib.make_geom(N, P, C, D, A, 0 if dt == 'f32' else 1)
    assert be._lib.tnmf_hip_events_grad_W(be._ctx, ctypes.byref(g), _lib.MODES[mode], p(events), p(by_plane), p(plane_start),
                                          p(hh), len(sample), p(be._V_dev), p(Rd), p(workspace), p(poisoned), None) == 0
    assert torch.equal(poisoned, got)
    assert torch.equal(be.gradient_W_event_list(Wd, events, lists, hh, Rd), got)
    for pl in np.flatnonzero(ed.plane_counts(geo, plane) == 0):     # planes without events are exactly zero
        assert not bool(got[:, pl].any())


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', list(ed.MATRIX))
def test_one_update_step(name, dt):
    cu = device_cus()
    geo, sample, plane, shift, _, W = ed.matrix_case(name, cu)
    N, C, P, D, A, mode = geo
    be = backend(*geo, dt)
    V, _, _ = integer_problem(name, cu)
    start, want = reference_step(name, cu)
    be._V_dev.copy_(dev(V, dt))
    Wd = dev(W, dt)
    hh, images, cell_start, events, _ = lists_of(be, P, sample, plane, shift, start)
    R = be.render_event_list(Wd, images, cell_start, hh)
    be.update_event_list(Wd, events, hh, R, 0., EPS)
    got = hh.cpu().numpy().astype(np.float64)
    again, _, _, _, _ = lists_of(be, P, sample, plane, shift, start)
    be.update_event_list(Wd, events, again, R, 0., EPS)
    assert torch.equal(again, hh), 'an update is deterministic'
    assert got[1] == 0. and want[1] == 0.
    live = want > 0
    assert live.sum() > len(want) // 2 and not got[~live].any()
    err = np.abs(got[live] - want[live]) / want[live]
    print(f'{name} {dt}: one update step vs reference {err.max():.3g} (per strength, relative)')
    assert err.max() <= BAR[dt]
