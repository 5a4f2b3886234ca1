"""
The W side of the events on the GPU: tnmf_hip_events_grad_W through HIP_Backend and the C ABI, ``fit_events`` and
``fit_detections`` on ``backend='hip'``, against the naive float64 reference tests/events_w_reference.py and against the dense
kernels on the scattered H.

Gradients of integer-valued inputs (V and W in 0..3, strengths 1..4: R and every double partial sum are exact integers) are
compared EXACTLY with the float64 reference rounded once to the element type.  Float-valued gradients, dictionaries and
strengths are held to the project's bars per entry, relative (1e-10 float64, 1e-5 float32).
"""
import ctypes
import functools
import threading

import numpy as np
import pytest
import torch

import events_reference as eref
import events_w_reference as wref
from local_collective import run_ranks
from test_hip_events import BAR, DTYPES, NP, backend, case, dev, float_problem
from tnmf_amd import _lib
from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF

pytestmark = pytest.mark.gpu

SEG = _lib.EVENT_SEGMENT
EPS = 1e-9


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# -- the cases: those of tests/test_hip_events.py and three for the segments, the tap loop and the sub-lanes ----------------------
OWN = {'segments': (3, 2, 4, (37, 150), (5, 7), 'valid'),      # plane 1: two full segments and a partial one; plane 3: none
       'more-taps-than-threads': (1, 3, 2, (16, 16), (12, 12), 'valid'),      # C * Ay * Ax = 432 > 256
       'few-taps': (2, 1, 3, (40,), (7,), 'reflect')}          # C * A = 7 < 64: 36 sub-lanes per tap


@functools.lru_cache(maxsize=None)
def wcase(name):
    """-> (geometry, sample, plane, shift, integer strengths, integer W), read-only; distinct rows in shuffled order."""
    if name not in OWN:
        return case(name)
    N, C, P, D, A, mode = geo = OWN[name]
    S = eref.shift_shape(D, A, mode)
    rng = np.random.default_rng(31)
    per_plane = {'segments': [9, 2 * SEG + 17, SEG, 0], 'more-taps-than-threads': [21, 14], 'few-taps': [30, 1, 60]}[name]
    rows = set()
    if name == 'few-taps':                                           # the mirror zone and its edges
        rows |= {(0, 0, 1), (1, 0, A[0] - 1), (1, 2, A[0]), (0, 2, 0), (0, 2, S[0] - 1)}
    for pl, count in enumerate(per_plane):
        while sum(r[1] == pl for r in rows) < count:
            rows.add((int(rng.integers(N)), pl) + tuple(int(rng.integers(s)) for s in S))
    rows = np.array(sorted(rows), dtype=np.int64)
    rows = rows[rng.permutation(len(rows))]
    out = (geo, rows[:, 0], rows[:, 1], rows[:, 2:], rng.integers(1, 5, len(rows)).astype(np.float64),
           rng.integers(0, 4, (P, C) + A).astype(np.float64))
    for a in out[1:]:
        a.setflags(write=False)
    return out


ALL = ['2d-valid', '1d', 'full-atom-as-large-as-the-sample', 'valid', 'full', 'circular', 'reflect'] + list(OWN)


def test_the_own_cases_reach_what_they_are_for():
    _, _, plane, _, _, _ = wcase('segments')
    counts = np.bincount(plane, minlength=4)
    assert counts[1] >= 2 * SEG + 1 and counts[1] % SEG != 0 and counts[3] == 0 and counts[2] == SEG
    (_, C, _, _, A, _) = wcase('more-taps-than-threads')[0]
    assert C * int(np.prod(A)) > 256
    (_, C, _, _, A, _) = wcase('few-taps')[0]
    assert C * int(np.prod(A)) < 64
    # ... and the verdict of the host mirror of the kernels (tests/events_dispatch.py) on the same three
    import events_dispatch as ed
    reached = {name: ed.reached(*wcase(name)[:4]) for name in OWN}
    assert {'full-segment', 'partial-segment', 'plane-of-several-segments', 'slab-beyond-the-last-segment',
            'L-2..63'} <= reached['segments']['grad_W']
    assert {'plane-without-slabs', 'one-slab', 'several-slabs'} <= reached['segments']['grad_W_sum']
    assert {'tap-loop-strides', 'L==1', 'idle-threads'} <= reached['more-taps-than-threads']['grad_W']
    assert 'G1:three-tap-passes' not in reached['more-taps-than-threads']['grad_W']
    assert {'several-chunks', 'threads-beyond-the-taps'} <= reached['more-taps-than-threads']['grad_W_sum']
    assert {'L-2..63', 'idle-threads', 'two-images'} <= reached['few-taps']['grad_W']
    assert ed.sub_lanes(7) == 36 and 'U1:idle-lanes' in reached['few-taps']['update']


@functools.lru_cache(maxsize=None)
def integer_problem(name):
    """(V, R, the reference gradient [2, P, C, *A]) of the integer case, float64, read-only."""
    (N, C, P, D, A, mode), sample, plane, shift, h, W = wcase(name)
    V = np.random.default_rng(32).integers(0, 4, (N, C) + D).astype(np.float64)
    R = eref.render(W, D, N, mode, sample, plane, shift, h)
    want = wref.grad_W(V, R, W, D, mode, sample, plane, shift, h)
    assert want.max() < 2 ** 52 and want[0].any() and want[1].any()
    for a in (V, R, want):
        a.setflags(write=False)
    return V, R, want


def lists_of(be, n_planes, sample, plane, shift, h):
    """-> (checked strengths, events, (by_plane, plane_start, workspace)) on the device."""
    s, pl, sh, hh = be._check_events(n_planes, sample, plane, shift, h)
    _, _, events = be.event_list(s, pl, sh)
    return hh, events, be.event_plane_list(pl, n_planes)


def gradient(be, W, sample, plane, shift, h, R, dt):
    hh, events, lists = lists_of(be, W.shape[0], sample, plane, shift, h)
    return be.gradient_W_event_list(dev(W, dt), events, lists, hh, dev(R, dt)).cpu().numpy()


# -- the gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', ALL)
def test_gradient_of_integers_is_the_reference_rounded_once(name, dt):
    geo, sample, plane, shift, h, W = wcase(name)
    N, C, P, D, A, mode = geo
    be = backend(*geo, dt)
    V, R, want = integer_problem(name)
    be._V_dev.copy_(dev(V, dt))
    # R from the render of the same list: integers, exact
    Wd = dev(W, dt)
    Rd = be.render_events(Wd, sample, plane, shift, h)
    assert np.array_equal(Rd.cpu().numpy().astype(np.float64), R)
    hh, events, lists = lists_of(be, P, sample, plane, shift, h)
    got = be.gradient_W_event_list(Wd, events, lists, hh, Rd)
    assert got.dtype == be._torch_dtype and tuple(got.shape) == (2, P, C) + A
    assert got.cpu().numpy().tobytes() == want.astype(NP[dt]).tobytes()
    # over a poisoned output and workspace: every element is written, none is read; and the same bits again
    by_plane, plane_start, workspace = lists
    workspace.fill_(float('nan'))
    poisoned = torch.full_like(got, float('nan'))
    g = _lib.make_geom(N, P, C, D, A, 0 if dt == 'f32' else 1)
    assert be._lib.tnmf_hip_events_grad_W(be._ctx, ctypes.byref(g), _lib.MODES[mode], p(events), p(by_plane), p(plane_start),
                                          p(hh), len(sample), p(be._V_dev), p(Rd), p(workspace), p(poisoned), None) == 0
    assert torch.equal(poisoned, got)
    assert torch.equal(be.gradient_W_event_list(Wd, events, lists, hh, Rd), got)
    for pl in set(range(P)) - set(plane.tolist()):                  # planes without events are exactly zero
        assert not bool(got[:, pl].any())
    if name == 'segments':
        assert not bool(got[:, 3].any())


@pytest.mark.parametrize('dt', DTYPES)
def test_no_events_duplicates_and_zero_strengths(dt):
    geo, sample, plane, shift, h, W = wcase('circular')
    N, C, P, D, A, mode = geo
    be = backend(*geo, dt)
    V, R, want = integer_problem('circular')
    be._V_dev.copy_(dev(V, dt))
    none = gradient(be, W, sample[:0], plane[:0], shift[:0], h[:0], R, dt)
    assert none.shape == want.shape and not none.any()
    # duplicate rows add up (R is an operand of its own: the same for both lists)
    twice = [np.concatenate([x, x[:9]]) for x in (sample, plane, shift, h)]
    doubled = np.concatenate([2 * h[:9], h[9:]])
    assert np.array_equal(gradient(be, W, *twice, R, dt), gradient(be, W, sample, plane, shift, doubled, R, dt))
    more = wref.grad_W(V, R, W, D, mode, sample[:9], plane[:9], shift[:9], h[:9])
    assert gradient(be, W, *twice, R, dt).tobytes() == (want + more).astype(NP[dt]).tobytes()
    # a strength of 0 contributes nothing
    zeroed = np.array(h)
    zeroed[::3] = 0.
    live = zeroed > 0
    assert np.array_equal(gradient(be, W, sample, plane, shift, zeroed, R, dt),
                          gradient(be, W, sample[live], plane[live], shift[live], h[live], R, dt))
    # K = 0 through fit_events: W unchanged, nothing NaN
    Wd = dev(W + 1., dt)
    before = Wd.clone()
    out = be.fit_events(None, Wd, None, None, sample[:0], plane[:0], shift[:0], h[:0], 3)
    assert out.shape == (0,) and torch.equal(Wd, before)


# -- float-valued problems ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(name):
    """W (each atom of sum 1 per channel), the starting strengths and V = the render of 'true' strengths + 0.1, in float64 of
    float32-representable values, so that both element types work on the same numbers."""
    geo, sample, plane, shift, _, _ = wcase(name)
    if name not in OWN:
        W, start, V = float_problem(name)
        return W, start, V
    N, C, P, D, A, mode = geo
    rng = np.random.default_rng(33)
    W = (rng.random((P, C) + A) + 0.1).astype(np.float32).astype(np.float64)
    true = (rng.random(len(sample)) + 0.5).astype(np.float32).astype(np.float64)
    start = (rng.random(len(sample)) + 0.5).astype(np.float32).astype(np.float64)
    start[1] = 0.   # stays 0
    V = (eref.render(W, D, N, mode, sample, plane, shift, true) + 0.1).astype(np.float32).astype(np.float64)
    for a in (W, start, V):
        a.setflags(write=False)
    return W, start, V


@functools.lru_cache(maxsize=None)
def reference_fit(name):
    geo, sample, plane, shift, _, _ = wcase(name)
    W, start, V = problem(name)
    out = wref.fit(V, W, geo[5], sample, plane, shift, start, 3, 0.1, EPS)
    for a in out:
        a.setflags(write=False)
    return out


FLOAT_CASES = ['2d-valid', '1d', 'full', 'circular', 'reflect'] + list(OWN)


def rel(got, other, ref=None):
    """The worst |got - other| relative to the reference's entry (``ref``; ``other`` itself when not given).  An entry the
    reference has as exactly zero -- a tap no event reaches inside the sample -- must be exactly zero in ``got``."""
    ref = other if ref is None else ref
    nz = ref != 0
    assert nz.any() and not got[~nz].any()
    return float(np.max(np.abs(got[nz] - other[nz]) / np.abs(ref[nz])))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', FLOAT_CASES)
def test_gradient_agrees_with_the_reference_and_the_dense_gradient(name, dt):
    geo, sample, plane, shift, _, _ = wcase(name)
    N, C, P, D, A, mode = geo
    be = backend(*geo, dt)
    W, start, V = problem(name)
    be._V_dev.copy_(dev(V, dt))
    Wd = dev(W, dt)
    Rd = be.render_events(Wd, sample, plane, shift, start)
    hh, events, lists = lists_of(be, P, sample, plane, shift, start)
    got = be.gradient_W_event_list(Wd, events, lists, hh, Rd).cpu().numpy().astype(np.float64)
    R = eref.render(W, D, N, mode, sample, plane, shift, start)
    want = wref.grad_W(V, R, W, D, mode, sample, plane, shift, start)
    H = dev(eref.scatter(N, P, eref.shift_shape(D, A, mode), sample, plane, shift, start), dt)
    dense = be.local_gradient_W(None, Wd, H).cpu().numpy().astype(np.float64)
    seen = want[0].reshape(P, -1).any(axis=1)                       # planes with events (the others: exactly zero)
    assert not got[:, ~seen].any() and seen.sum() >= P - 1
    err, err_dense = rel(got[:, seen], want[:, seen]), rel(got[:, seen], dense[:, seen], want[:, seen])
    print(f'{name} {dt}: gradient vs reference {err:.3g}, vs dense local_gradient_W {err_dense:.3g} (per entry, relative)')
    assert err <= BAR[dt] and err_dense <= BAR[dt]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', FLOAT_CASES)
def test_three_fit_events_iterations(name, dt):
    geo, sample, plane, shift, _, _ = wcase(name)
    N, C, P, D, A, mode = geo
    be = backend(*geo, dt)
    W, start, V = problem(name)
    be._V_dev.copy_(dev(V, dt))
    Wd = dev(W, dt)
    got_h = be.fit_events(None, Wd, None, None, sample, plane, shift, start, 3, sparsity=0.1, eps=EPS)
    again_W = dev(W, dt)
    again_h = be.fit_events(None, again_W, None, None, sample, plane, shift, start, 3, sparsity=0.1, eps=EPS)
    assert torch.equal(got_h, again_h) and torch.equal(Wd, again_W), 'a fit on the list is deterministic'
    got_W, got_h = Wd.cpu().numpy().astype(np.float64), got_h.cpu().numpy().astype(np.float64)
    want_W, want_h = reference_fit(name)
    assert np.all(np.isfinite(got_W)) and np.all(np.isfinite(got_h)) and got_h[1] == 0. and want_h[1] == 0.
    live = want_h > 0
    err_W, err_h = rel(got_W, want_W), rel(got_h[live], want_h[live])
    print(f'{name} {dt}: 3 fit_events iterations vs reference: W {err_W:.3g}, strengths {err_h:.3g} (per entry, relative)')
    assert err_W <= BAR[dt] and err_h <= BAR[dt]
    seen = np.bincount(plane, minlength=P) > 0
    for pl in np.flatnonzero(~seen):                                # no evidence: the atom keeps its bits
        assert Wd[pl].cpu().numpy().tobytes() == W[pl].astype(NP[dt]).tobytes()
    np.testing.assert_allclose(got_W[seen].sum(axis=tuple(range(2, got_W.ndim))), 1., rtol=10 * BAR[dt])
    if not seen.all():
        return   # (the dense step makes an atom without activations 0 / 0, and with it every R)
    # three dense iterations on the scattered H: the H half step without inhibition, the W half step
    H = dev(eref.scatter(N, P, eref.shift_shape(D, A, mode), sample, plane, shift, start), dt)
    Wdense = dev(W, dt)
    for _ in range(3):
        be.fused_update_H(None, Wdense, H, sparsity=0.1, eps=EPS)
        be.fused_update_W(None, Wdense, H, eps=EPS)
    dense_h = H.cpu().numpy().astype(np.float64)[(sample, plane) + tuple(shift.T)]
    err_W = rel(got_W, Wdense.cpu().numpy().astype(np.float64), want_W)
    err_h = rel(got_h[live], dense_h[live], want_h[live])
    print(f'{name} {dt}: 3 fit_events iterations vs 3 dense iterations: W {err_W:.3g}, strengths {err_h:.3g}')
    assert err_W <= BAR[dt] and err_h <= BAR[dt]


@pytest.mark.parametrize('dt', DTYPES)
def test_an_atom_without_evidence_keeps_its_bits_on_the_device(dt):
    geo, sample, plane, shift, _, _ = wcase('segments')
    N, C, P, D, A, mode = geo
    be = backend(*geo, dt)
    W, start, V = problem('segments')
    be._V_dev.copy_(dev(V, dt))
    start = np.where(plane == 0, 0., start)                         # plane 0: zero strengths only; plane 3: no events
    Wd = dev(W, dt)
    before = Wd.clone()
    h = be.fit_events(None, Wd, None, None, sample, plane, shift, start, 3, eps=EPS)
    assert bool(torch.isfinite(Wd).all()) and bool(torch.isfinite(h).all())
    assert torch.equal(Wd[0], before[0]) and torch.equal(Wd[3], before[3])
    assert not torch.equal(Wd[1], before[1]) and not torch.equal(Wd[2], before[2])
    # update_H off: the strengths keep their bits
    Wd = dev(W, dt)
    h = be.fit_events(None, Wd, None, None, sample, plane, shift, start, 2, update_H=False, eps=EPS)
    assert h.cpu().numpy().tobytes() == start.astype(NP[dt]).tobytes() and not torch.equal(Wd[1], before[1])


# -- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing_and_rows_outside_the_contract_are_skipped():
    geo, sample, plane, shift, h, W = wcase('circular')
    N, C, P, D, A, mode = geo
    be = backend(*geo, 'f32')
    lib, ctx = be._lib, be._ctx
    V, R, want = integer_problem('circular')
    be._V_dev.copy_(dev(V, 'f32'))
    Vd, Rd = be._V_dev, dev(R, 'f32')
    hh, events, (by_plane, plane_start, workspace) = lists_of(be, P, sample, plane, shift, h)
    K = len(sample)
    negpos = torch.full((2, P, C) + A, -7., dtype=torch.float32, device='cuda')
    workspace.fill_(-7.)
    E_NULL, E_DTYPE = -1, -3

    def geom(**kw):
        g = _lib.make_geom(N, P, C, D, A, 0)
        for key, val in kw.items():
            setattr(g, key, val)
        return ctypes.byref(g)

    def call(g, m=_lib.MODES[mode], ev=events, bp=by_plane, ps=plane_start, st=hh, k_=K, V_=Vd, R_=Rd, ws=workspace,
             out=negpos, c=ctx):
        return lib.tnmf_hip_events_grad_W(c, g, m, p(ev), p(bp), p(ps), p(st), k_, p(V_), p(R_), p(ws), p(out), None)

    assert call(geom(), c=None) == E_NULL and call(None) == E_NULL
    for kw in (dict(ev=None), dict(bp=None), dict(ps=None), dict(st=None), dict(V_=None), dict(R_=None), dict(ws=None),
               dict(out=None)):
        assert call(geom(), **kw) == E_NULL, kw
    assert call(geom(dtype=2)) == E_DTYPE and call(geom(dtype=-1)) == E_DTYPE
    assert call(geom(ndim=3)) == _lib.E_UNSUPPORTED and call(geom(), k_=2 ** 31) == _lib.E_UNSUPPORTED
    for kw in (dict(ndim=0), dict(ndim=4), dict(N=-1), dict(M=0), dict(C=0)):
        assert call(geom(**kw)) == _lib.E_GEOM, kw
    assert call(geom(), m=4) == _lib.E_GEOM and call(geom(), m=-1) == _lib.E_GEOM and call(geom(), k_=-1) == _lib.E_GEOM
    g = _lib.make_geom(N, P, C, (4, 23), (6, 6), 0)                 # circular: more than one wrap
    assert call(ctypes.byref(g)) == _lib.E_GEOM
    g = _lib.make_geom(N, P, C, (3, 23), (4, 6), 0)                 # reflect: a mirror without the edge; full: no shift
    assert call(ctypes.byref(g), m=_lib.MODES['reflect']) == _lib.E_GEOM
    assert call(ctypes.byref(g), m=_lib.MODES['full']) == _lib.E_GEOM
    torch.cuda.synchronize()
    assert bool(torch.all(negpos == -7.)) and bool(torch.all(workspace == -7.))
    # rows outside the contract are skipped, not followed: a wild sample, plane and shift, wild entries of by_plane, a
    # plane_start beyond the list
    ev = events.clone()
    ev[0, 0], ev[1, 1], ev[2, 2], ev[3, 3], ev[4, 1] = N, -1, D[0], -5, (int(ev[4, 1]) + 1) % P
    bp = by_plane.clone()
    order = by_plane.cpu().numpy()
    at5, at6 = int(np.flatnonzero(order == 5)[0]), int(np.flatnonzero(order == 6)[0])
    bp[at5], bp[at6] = -1, K
    ps = plane_start.clone()
    ps[-1] = K + 1000
    assert call(geom(), ev=ev, bp=bp, ps=ps) == 0
    keep = np.ones(K, dtype=bool)
    keep[:7] = False
    rest = wref.grad_W(V, R, W, D, mode, sample[keep], plane[keep], shift[keep], h[keep])
    assert negpos.cpu().numpy().tobytes() == rest.astype(np.float32).tobytes()


# -- end to end -----------------------------------------------------------------------------------------------------------------
def hip_model(V, n_atoms, atom_shape, **kw):
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=n_atoms, atom_shape=atom_shape, backend='hip', **kw)
    nmf.fit(V, n_iterations=5, sparsity_H=0.1)
    return nmf


def check_model(nmf, dt):
    be = nmf._backend
    mode = be._reconstruction_mode
    V = np.asarray(nmf.V, dtype=np.float64)
    T = nmf.n_transforms
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.95)), min_distance=1)
    assert 10 < len(det) < 1000
    plane = det.atom * T + det.transform

    def loss(d):
        return 0.5 * np.sum((V - nmf.reconstruct_detections(d).astype(np.float64)) ** 2)
    H_before, W_before = nmf.H.copy(), nmf.W.copy()
    # three iterations against the reference, from the same state
    want_W, want_h = wref.fit(V, W_before.astype(np.float64), mode, det.sample, plane, det.shift,
                              det.strength.astype(np.float64), 3, 0.05, nmf.eps, transforms=nmf.transforms)
    refit_loss = loss(nmf.refit_detections(det, 10))                # (W fixed: the model is left as it was)
    assert nmf.W.tobytes() == W_before.tobytes()
    fit = nmf.fit_detections(det, 3, sparsity_H=0.05)
    assert isinstance(fit, Detections) and fit.strength.dtype == det.strength.dtype
    for name in ('sample', 'atom', 'transform', 'shift', 'origin'):
        np.testing.assert_array_equal(getattr(fit, name), getattr(det, name))
    seen = np.bincount(det.atom, minlength=nmf.n_atoms) > 0
    err_W, err_h = rel(nmf.W[seen].astype(np.float64), want_W[seen]), rel(fit.strength.astype(np.float64), want_h)
    print(f'{mode} {dt} T={T}: fit_detections 3 iterations vs reference: W {err_W:.3g}, strengths {err_h:.3g}')
    assert err_W <= BAR[dt] and err_h <= BAR[dt]
    assert nmf.W[~seen].tobytes() == W_before[~seen].tobytes() and np.all(np.isfinite(nmf.W))
    assert nmf.H.tobytes() == H_before.tobytes()                    # the dense H is left as it is
    if nmf.transforms is not None:
        import tnmf_amd.transforms as tr
        np.testing.assert_allclose(nmf.transformed_atoms.reshape((-1,) + nmf.W.shape[1:]), tr.expand(nmf.W, nmf.transforms),
                                   rtol=BAR[dt])
    # alternating strengths and atoms explain V at least as well as the strengths alone, from the same state
    nmf._W.copy_(torch.from_numpy(W_before).to(nmf._W.device))
    nmf._expand_W()
    fit_loss = loss(nmf.fit_detections(det, 10))
    print(f'{mode} {dt} T={T}: 1/2 |V - R_det|^2 after 10 iterations: strengths alone {refit_loss:.6g}, with W {fit_loss:.6g}')
    assert fit_loss <= refit_loss * (1 + 1e-6)


@pytest.mark.parametrize('mode', ['valid', 'circular'])
@pytest.mark.parametrize('which', ['2d-f32', '1d-f64'])
def test_fit_detect_fit_detections_reconstruct(which, mode):
    rng = np.random.default_rng(21)
    if which == '2d-f32':
        V, M, A = rng.random((3, 2, 24, 30)).astype(np.float32), 4, (5, 6)
    else:
        V, M, A = rng.random((4, 1, 120)), 3, (9,)
    check_model(hip_model(V, M, A, reconstruction_mode=mode), which[-3:])


def test_fit_with_rot90_detect_fit_detections_reconstruct():
    V = np.random.default_rng(22).random((3, 1, 20, 22)).astype(np.float32)
    check_model(hip_model(V, 2, (4, 4), transforms='rot90'), 'f32')


def test_refusals_through_the_front_end():
    V = np.random.default_rng(23).random((2, 1, 12, 14)).astype(np.float32) + 0.1
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend='hip', beta_loss=1.)
    nmf.fit(V, n_iterations=2)
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)))
    with pytest.raises(NotImplementedError):
        nmf.fit_detections(det, 1)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend='hip')
    nmf.fit(V, n_iterations=2, weights=np.ones((2, 1, 1, 1), dtype=np.float32))
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)))
    with pytest.raises(NotImplementedError):
        nmf.fit_detections(det, 1)
    with pytest.raises(NotImplementedError):                        # ... nor does the backend take it
        nmf._backend.fit_events(None, nmf._W, None, None, det.sample, det.atom, det.shift, det.strength, 1)
    np.random.seed(42)
    nmf = TransformInvariantNMF(n_atoms=2, atom_shape=(3, 3), backend='hip')
    nmf.fit(V, n_iterations=2)
    det = nmf.detections(threshold=float(np.quantile(nmf.H, 0.9)))
    W = nmf.W.copy()
    with pytest.raises(ValueError):
        nmf.fit_detections(det, 1, update_H=False, update_W=False)
    want = nmf.refit_detections(det, 2)
    assert nmf.fit_detections(det, 2, update_W=False).strength.tobytes() == want.strength.tobytes()
    assert nmf.W.tobytes() == W.tobytes()


_init_lock = threading.Lock()


def test_two_ranks_learn_the_single_process_dictionary():
    V = np.random.default_rng(24).random((8, 1, 48, 48)).astype(np.float32)
    V[5:] *= 0.02                                                   # rank 1: one sample with events, three almost without

    def fit(pg=None):
        nmf = TransformInvariantNMF(n_atoms=4, atom_shape=(5, 5), backend='hip', process_group=pg)
        plain_init = nmf._initialize_matrices

        def seeded_init(V_, keep_W, **kw):
            with _init_lock:
                np.random.seed(42)
                plain_init(V_, keep_W, **kw)
        nmf._initialize_matrices = seeded_init
        nmf.fit(V, n_iterations=5, sparsity_H=0.1, update_W=False)  # (W fixed: the shards hold the single process's H)
        return nmf

    single = fit()
    t = float(np.quantile(single.H, 0.97))
    det = single.detections(threshold=t)
    want_h = single.fit_detections(det, 3, sparsity_H=0.05).strength
    want_W = single.W

    def rank_body(rank, coll):
        torch.cuda.set_device(0)
        nmf = fit(coll)
        d = nmf.detections(threshold=t)
        out = nmf.fit_detections(d, 3, sparsity_H=0.05)
        return d, out.strength, nmf.W

    ((d0, h0, W0), (d1, h1, W1)), _group = run_ranks(2, rank_body)
    assert len(d0) + len(d1) == len(det) and 0 < len(d1) < len(d0) // 2
    assert set(d1.sample.tolist()) <= set(range(4, 8))
    assert W0.tobytes() == W1.tobytes()                             # the same rule and the same sum on every rank
    err_W, err_h = rel(W0.astype(np.float64), want_W), rel(np.concatenate([h0, h1]).astype(np.float64), want_h)
    print(f'two ranks vs one process, 3 iterations: W {err_W:.3g}, strengths {err_h:.3g} (per entry, relative)')
    assert err_W <= BAR['f32'] and err_h <= BAR['f32']
