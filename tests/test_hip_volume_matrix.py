"""
Every branch of the three-shift-axis family (tnmf_amd/csrc/volume.hip, the vol_api_* entries of api.hip) against the float64
oracle: the cases of tests/volume_dispatch.py, each in float32 and float64 on a fresh backend.  Operands are float64 images
of float32 values, so both dtypes see the same numbers and the oracle's answer is computed once per case.  Forms HIP.py
never makes (a finished reconstruction handed in, no caller's scratch) go through ctypes.  Bars: those of
tests/test_hip_volumes.py -- 2e-5 / 1e-10 of the output's maximum for a primitive, five times that for the fused half
steps, twice for tnmf_hip_update_H_ex -- and of tests/test_hip_objective.py for the tap (1e-5 / 1e-10 per sample).
Every test prints what it measured (`pytest -s`): DESIGN section 4g quotes the worst of each.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import volume_dispatch as vd
from oracle import tnmf_oracle as orc
from tnmf_amd import _lib
from tnmf_amd.backends.HIP import HIP_Backend, _ptr

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(np.float32, id='f32'), pytest.param(np.float64, id='f64')]
BAR = {np.float32: 2e-5, np.float64: 1e-10}
TAP_BAR = {np.float32: 1e-5, np.float64: 1e-10}
CODE = {np.float32: 0, np.float64: 1}
AXES = (-3, -2, -1)
EPS, SPARSITY = 1e-9, 0.1
E = {'E_GEOM': _lib.E_GEOM, 'E_UNSUPPORTED': _lib.E_UNSUPPORTED, 'E_STRIDE': _lib.E_STRIDE, 'E_DTYPE': -3, 'E_NULL': -1}
CASES = {kind: [cid for cid, c in vd.MATRIX.items() if c.kind == kind] for kind in ('prim', 'pad', 'ex')}


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def relmax(got, want):
    want = np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max()
    return np.abs(np.asarray(got, dtype=np.float64) - want).max() / (scale if scale > 0 else 1.0)


def note(cid, dtype, **figures):
    print(f'volume-matrix {cid} {np.dtype(dtype).name} ' + ' '.join(f'{k}={v:.2e}' for k, v in figures.items()))


def backend(geometry, V, dtype, mode='valid'):
    _, _, _, M, A = geometry
    be = HIP_Backend(reconstruction_mode=mode)
    np.random.seed(1)
    be.initialize(V.astype(dtype), A, M, None, AXES)
    return be


def geom(geometry, dtype, n=None, stride=0, code=None):
    N, C, D, M, A = geometry
    return _lib.make_geom(N if n is None else n, M, C, D, A, CODE[dtype] if code is None else code, stride)


def poisoned(shape, dtype):
    return torch.full(shape, float('nan'), dtype=torch.float32 if dtype is np.float32 else torch.float64, device='cuda')


def compute_units(be):
    return torch.cuda.get_device_properties(be.device).multi_processor_count


@functools.lru_cache(maxsize=None)
def operands(cid):
    """V, W (normalised), H of a case as float64 images of float32 values, and the oracle's answers -- computed once."""
    case = vd.MATRIX[cid]
    N, C, D, M, A = case.geometry
    rng = np.random.default_rng(sum(map(ord, cid)))
    V = f32(rng.random((N, C) + D))
    W = rng.random((M, C) + A)
    W = f32(W / W.sum(axis=AXES, keepdims=True))
    H = f32(rng.random((N, M) + orc.transform_shape(D, A, case.mode)))
    out = dict(V=V, W=W, H=H)
    if case.kind == 'prim':
        out['R'] = orc.reconstruct(W, H)
        out['gH'] = orc.gradient_H(V, W, H)
        out['gW'] = orc.gradient_W(V, W, H)
        out['energy'] = orc.energy(V, W, H)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# ctypes forms
# ----------------------------------------------------------------------------------------------------------------------
def call_grad_W_fused(be, g, V, W, H, R_scratch, r_is_valid, shape, dtype):
    negpos = poisoned((2,) + shape, dtype)
    rc = be._lib.tnmf_hip_grad_W_fused(be._ctx, ctypes.byref(g), _ptr(V), _ptr(W), _ptr(H), _ptr(R_scratch), r_is_valid,
                                       _ptr(negpos), be._stream())
    assert rc == 0, rc
    assert be.last_path == 'volume'
    return negpos


def call_grad_W(be, g, V, R, W, H, shape, dtype):
    neg, pos = poisoned(shape, dtype), poisoned(shape, dtype)
    rc = be._lib.tnmf_hip_grad_W(be._ctx, ctypes.byref(g), _ptr(V), _ptr(R), _ptr(W), _ptr(H), _ptr(neg), _ptr(pos), be._stream())
    assert rc == 0, rc
    return torch.stack((neg, pos))


def call_grad_H(be, g, V, R, W, H, dtype):
    neg, pos = poisoned(tuple(H.shape), dtype), poisoned(tuple(H.shape), dtype)
    rc = be._lib.tnmf_hip_grad_H(be._ctx, ctypes.byref(g), _ptr(V), _ptr(R), _ptr(W), _ptr(H), _ptr(neg), _ptr(pos), be._stream())
    assert rc == 0, rc
    assert be.last_path == 'volume'
    return neg, pos


def call_update_H(be, g, V, W, H, R_scratch, r_is_valid):
    rc = be._lib.tnmf_hip_update_H(be._ctx, ctypes.byref(g), _ptr(V), _ptr(W), _ptr(H), _ptr(R_scratch), r_is_valid, EPS, SPARSITY,
                                   be._stream())
    assert rc == 0, rc
    assert be.last_path == 'volume'
    return H


def call_update_H_ex(be, g, mode, V, W, H, R_scratch, sparsity, inhibition, cross, kernels):
    ks = [np.ascontiguousarray(k, dtype=np.float64) for k in (kernels or ())]
    kp = [k.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for k in ks] + [None, None, None]
    kl = [len(k) for k in ks] + [0, 0, 0]
    mode = _lib.MODES[mode] if isinstance(mode, str) else mode
    return be._lib.tnmf_hip_update_H_ex(be._ctx, ctypes.byref(g), mode, _ptr(V), _ptr(W), _ptr(H), _ptr(R_scratch), EPS, sparsity,
                                        inhibition, cross, kp[0], kl[0], kp[1], kl[1], kp[2], kl[2], be._stream())


# ----------------------------------------------------------------------------------------------------------------------
# 1. the primitives
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cid', CASES['prim'])
def test_primitives_against_oracle(cid, dtype):
    case, o, tol = vd.MATRIX[cid], operands(cid), BAR[dtype]
    N, C, D, M, A = G = case.geometry
    be = backend(G, o['V'], dtype)
    # the chunk count the case was chosen for, at this device's number of compute units
    cu = compute_units(be)
    P = vd.vol_corr_H_chunks(vd.vol(G), cu)
    if isinstance(case.P, dict):
        assert P in case.P.values() and case.P.get(cu, P) == P, (cu, P)
    else:
        assert P == case.P, (cu, P)
    V, W, H = be._V_dev, dev(o['W'], dtype), dev(o['H'], dtype)
    g = geom(G, dtype)
    R = be.reconstruct(W, H)
    assert be.last_path == 'volume'
    eR = relmax(host(R), o['R'])
    # H gradient: the reconstruction computed by the library, or handed in
    neg, pos = be.reconstruction_gradient_H(o['V'], W, H)
    eH = max(relmax(host(neg), o['gH'][0]), relmax(host(pos), o['gH'][1]))
    neg2, pos2 = call_grad_H(be, g, V, R, W, H, dtype)
    assert torch.equal(neg, neg2) and torch.equal(pos, pos2), 'grad_H: R handed in against R computed'
    # W gradient: the library's own scratch, a caller's scratch filled on the way, a valid reconstruction handed in
    wshape = (M, C) + A
    own = call_grad_W_fused(be, g, V, W, H, None, 0, wshape, dtype)
    scratch = poisoned(tuple(R.shape), dtype)
    filled = call_grad_W_fused(be, g, V, W, H, scratch, 0, wshape, dtype)
    assert torch.equal(scratch, R), 'the caller\'s scratch holds the reconstruction afterwards'
    valid = call_grad_W_fused(be, g, V, W, H, R, 1, wshape, dtype)
    assert torch.equal(own, filled) and torch.equal(own, valid), 'grad_W: the three R arms'
    assert torch.equal(own, call_grad_W(be, g, V, None, W, H, wshape, dtype)), 'tnmf_hip_grad_W without R'
    assert torch.equal(own, call_grad_W(be, g, V, R, W, H, wshape, dtype)), 'tnmf_hip_grad_W with R'
    assert torch.equal(own, call_grad_W_fused(be, g, V, W, H, None, 0, wshape, dtype)), 'the same bits from launch to launch'
    assert torch.equal(own, be.local_gradient_W(o['V'], W, H))
    eW = max(relmax(host(own[0]), o['gW'][0]), relmax(host(own[1]), o['gW'][1]))
    eE = abs(be.reconstruction_energy(o['V'], W, H) - o['energy']) / o['energy']
    note(cid, dtype, reconstruct=eR, grad_H=eH, grad_W=eW, energy=eE)
    assert eR < tol and eH < tol and eW < tol and eE < tol, (eR, eH, eW, eE)
    if not case.slices:
        return
    # an empty slice: exact zeros of the right shape, whatever scratch the caller brings; nothing else is written
    g0 = geom(G, dtype, n=0)
    assert torch.count_nonzero(call_grad_W_fused(be, g0, None, W, None, None, 0, wshape, dtype)) == 0
    scratch = poisoned((4,), dtype)
    assert torch.count_nonzero(call_grad_W_fused(be, g0, None, W, None, scratch, 0, wshape, dtype)) == 0
    assert bool(torch.isnan(scratch).all())
    zn, zp = be.reconstruction_gradient_W(o['V'], W, H, slice(0, 0))
    assert tuple(zn.shape) == wshape and torch.count_nonzero(zn) == 0 and torch.count_nonzero(zp) == 0
    zn, zp = be.reconstruction_gradient_H(o['V'], W, H, slice(0, 0))
    assert tuple(zn.shape) == (0, M) + tuple(H.shape[2:]) == tuple(zp.shape)
    # the last sample alone
    s = slice(N - 1, N)
    on, op = orc.gradient_H(o['V'], o['W'], o['H'], s)
    neg, pos = be.reconstruction_gradient_H(o['V'], W, H, s)
    eH = max(relmax(host(neg), on), relmax(host(pos), op))
    on, op = orc.gradient_W(o['V'], o['W'], o['H'], s)
    neg, pos = be.reconstruction_gradient_W(o['V'], W, H, s)
    eW = max(relmax(host(neg), on), relmax(host(pos), op))
    note(cid + '[last]', dtype, grad_H=eH, grad_W=eW)
    assert eH < tol and eW < tol, (eH, eW)


# ----------------------------------------------------------------------------------------------------------------------
# 2. the fused half steps
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cid', CASES['prim'])
def test_fused_half_steps_against_oracle(cid, dtype):
    case, o, tol = vd.MATRIX[cid], operands(cid), BAR[dtype]
    G = case.geometry
    be = backend(G, o['V'], dtype)
    V, W = be._V_dev, dev(o['W'], dtype)
    g = geom(G, dtype)
    want = o['H'] * o['gH'][0] / (o['gH'][1] + EPS + SPARSITY)
    own = call_update_H(be, g, V, W, dev(o['H'], dtype), None, 0)
    scratch = poisoned(tuple(V.shape), dtype)
    filled = call_update_H(be, g, V, W, dev(o['H'], dtype), scratch, 0)
    R = be.reconstruct(W, dev(o['H'], dtype))
    assert torch.equal(scratch, R)
    valid = call_update_H(be, g, V, W, dev(o['H'], dtype), R.clone(), 1)
    assert torch.equal(own, filled) and torch.equal(own, valid), 'update_H: the R_scratch / r_is_valid arms'
    Hf = dev(o['H'], dtype)
    be.fused_update_H(o['V'], W, Hf, slice(None), sparsity=SPARSITY, eps=EPS)
    assert torch.equal(own, Hf) and be.last_path == 'volume'
    eH = relmax(host(own), want)
    Wf = dev(o['W'], dtype)
    be.fused_update_W(o['V'], Wf, dev(o['H'], dtype), slice(None), eps=EPS)
    assert be.last_path == 'volume'
    wantW = o['W'] * o['gW'][0] / (o['gW'][1] + EPS)
    wantW /= wantW.sum(axis=AXES, keepdims=True)
    eW = relmax(host(Wf), wantW)
    note(cid, dtype, update_H=eH, update_W=eW)
    assert eH < 5 * tol and eW < 5 * tol, (eH, eW)


# ----------------------------------------------------------------------------------------------------------------------
# 3. pad and fold
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pad_reference(cid):
    case = vd.MATRIX[cid]
    N, _, D, M, A = case.geometry
    S = orc.transform_shape(D, A, case.mode)
    rng = np.random.default_rng(sum(map(ord, cid)))
    H = f32(rng.random((N, M) + S))
    Hp = orc.pad_activations(H, A, case.mode)
    Gp = f32(rng.random(Hp.shape))
    out = dict(H=H, Hp=Hp, Gp=Gp, G=orc.fold_gradient(Gp, S, A, case.mode), S=S)
    return out


PAD_RUN = [c for c in CASES['pad'] if not vd.pad_fold_guard(vd.MATRIX[c].geometry[2], vd.MATRIX[c].geometry[4], vd.MATRIX[c].mode)]
PAD_REFUSED = [c for c in CASES['pad'] if c not in PAD_RUN]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cid', PAD_RUN)
def test_pad_and_fold_against_oracle(cid, dtype):
    case, o = vd.MATRIX[cid], pad_reference(cid)
    N, C, D, M, A = G = case.geometry
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    if cid == 'pad_large':
        assert vd.strided_grid(o['Hp'].size, cu)[1] >= 2 and vd.strided_grid(o['H'].size, cu)[1] >= 2, 'the grid-stride loop'
    be = backend(G, np.zeros((N, C) + D), dtype, case.mode)
    Hp = be._pad(dev(o['H'], dtype))
    assert be.last_path == 'volume'
    assert tuple(Hp.shape) == o['Hp'].shape and np.array_equal(host(Hp), o['Hp']), 'the pad copies: exact'
    Gf = be._fold(dev(o['Gp'], dtype))
    assert tuple(Gf.shape) == o['G'].shape
    # the fold adds at most eight values: seven roundings of the element type, each relative to the sum so far
    err = np.abs(host(Gf) - o['G'])
    assert np.all(err <= 7 * np.finfo(dtype).eps * np.abs(o['G'])), err.max()
    note(cid, dtype, fold=err.max() / np.abs(o['G']).max())
    if dtype is np.float64:
        # the fold is the pad's adjoint: <pad(H), G> == <H, fold(G)>, to the rounding of two sums of n products in
        # float64 (pairwise: log2(n) roundings each) and the seven of the fold
        lhs, rhs = float(np.sum(host(Hp) * o['Gp'])), float(np.sum(o['H'] * host(Gf)))
        n = o['Hp'].size
        assert abs(lhs - rhs) <= (2 * np.log2(n) + 9) * np.finfo(np.float64).eps * float(np.sum(np.abs(o['Hp'] * o['Gp'])))


def _buffers(G, mode, dtype, seed=0):
    """Device operands of a geometry the library may refuse: nothing of them depends on a backend's own shapes."""
    N, C, D, M, A = G
    rng = np.random.default_rng(seed)
    S = tuple(max(1, s) for s in orc.transform_shape(D, A, mode))
    Hp = tuple(d + a - 1 for d, a in zip(D, A))
    mk = lambda shape: dev(0.5 + rng.random(shape), dtype)  # noqa: E731
    return dict(V=mk((N, C) + D), W=mk((M, C) + A), H=mk((N, M) + S), R=mk((N, C) + D), Hp=mk((N, M) + Hp), neg=mk((N, M) + Hp),
                pos=mk((N, M) + Hp), negpos=mk((2, M, C) + A))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cid', PAD_REFUSED)
def test_pad_and_fold_refuse_one_step_past_each_limit(cid, dtype):
    case = vd.MATRIX[cid]
    G, mode = case.geometry, case.mode
    ok = vd.REFUSAL_GEOMETRY
    be = backend(ok, np.zeros((ok[0], ok[1]) + ok[2]), dtype)
    b = _buffers(G, mode, dtype)
    g = geom(G, dtype)
    for fn, src, dst in ((be._lib.tnmf_hip_pad_H, b['H'], b['Hp']), (be._lib.tnmf_hip_fold_H, b['Hp'], b['H'])):
        before = dst.clone()
        assert fn(be._ctx, ctypes.byref(g), _lib.MODES[mode], _ptr(src), _ptr(dst), be._stream()) == _lib.E_GEOM
        assert torch.equal(dst, before)
    # the half step meets the same guard: without lateral terms before any launch, with them after the lateral-term
    # kernels have run on the library's work arrays -- H and the caller's scratch as they were either way
    v = vd.vol(G)
    for inh, kernels in ((0., None), (0.1, [np.ones(3)] * 3)):
        assert vd.update_H_ex_arm(v, mode, inh, 0., (3, 3, 3))[0] == 'E_GEOM'
        H0, R0 = b['H'].clone(), b['R'].clone()
        assert call_update_H_ex(be, g, mode, b['V'], b['W'], b['H'], b['R'], 0.05, inh, 0., kernels) == _lib.E_GEOM
        assert torch.equal(b['H'], H0) and torch.equal(b['R'], R0)
    _context_still_works(be, dtype)


def _context_still_works(be, dtype):
    G = vd.REFUSAL_GEOMETRY
    N, C, D, M, A = G
    rng = np.random.default_rng(9)
    W, H = f32(rng.random((M, C) + A)), f32(rng.random((N, M) + tuple(d + a - 1 for d, a in zip(D, A))))
    assert relmax(host(be.reconstruct(dev(W, dtype), dev(H, dtype))), orc.reconstruct(W, H)) < BAR[dtype]
    assert be.last_path == 'volume'


# ----------------------------------------------------------------------------------------------------------------------
# 4. tnmf_hip_update_H_ex: the modes crossed with the lateral terms
# ----------------------------------------------------------------------------------------------------------------------
def lateral_kernels(case):
    A = case.geometry[4]
    if case.kernels == 'parabolic':
        return orc.inhibition_kernels(tuple(a - 1 for a in A))
    rng = np.random.default_rng(17)
    out = []
    for t in (3, 5, 3):
        k = 0.25 + rng.random(t)        # asymmetric, odd
        k[(t - 1) // 2] = 1.5 + rng.random()
        out.append(k)
    return tuple(out)


def oracle_step(case, o, kernels, inhibition, cross):
    _, _, _, M, A = case.geometry
    ref = orc.OracleNMF(n_atoms=M, atom_shape=A, reconstruction_mode=case.mode)
    ref._kernels = kernels
    ref.V, ref.W, ref.H = o['V'], o['W'], o['H'].copy()
    ref.update_H(slice(None), sparsity=0.05, inhibition=inhibition, cross_inhibition=cross)
    return ref.H


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cid', CASES['ex'])
def test_update_H_ex_against_oracle(cid, dtype):
    case, o, tol = vd.MATRIX[cid], operands(cid), BAR[dtype]
    N, C, D, M, A = G = case.geometry
    be = backend(G, o['V'], dtype, case.mode)
    V, W = be._V_dev, dev(o['W'], dtype)
    g = geom(G, dtype)
    kernels = lateral_kernels(case)
    worst = 0.
    for term in case.terms:
        inh, cross = vd.STRENGTHS['both' if term == 'M_1_cross_dropped' else term]
        ks = kernels if inh > 0 or cross > 0 else None
        # through the backend (its own R_scratch, the objective tap set) and through ctypes without a scratch
        Hb, tap = dev(o['H'], dtype), be.new_objective_buffer()
        be.fused_update_H(o['V'], W, Hb, slice(None), sparsity=0.05, eps=EPS, inhibition=inh, cross_inhibition=cross,
                          inhibition_kernels=ks, objective_out=tap)
        assert be.last_path == 'volume'
        Hc = dev(o['H'], dtype)
        assert call_update_H_ex(be, g, case.mode, V, W, Hc, None, 0.05, inh, cross, ks) == 0
        assert torch.equal(Hb, Hc), 'with and without R_scratch, with and without the tap'
        if term == 'M_1_cross_dropped':
            # one atom has no other atom to be inhibited by: the term is dropped, bit for bit
            Hd = dev(o['H'], dtype)
            assert call_update_H_ex(be, g, case.mode, V, W, Hd, None, 0.05, inh, 0., ks) == 0
            assert torch.equal(Hc, Hd)
            cross = 0.
        err = relmax(host(Hb), oracle_step(case, o, kernels, inh, cross))
        worst = max(worst, err)
        assert err < 2 * tol, (term, err)
        # the tap: each sample's 1/2 sum (V - R)^2 at the state the step started from
        R = orc.reconstruct(o['W'], o['H'], mode=case.mode)
        want = 0.5 * np.sum(np.square(o['V'] - R), axis=(1, 2, 3, 4))
        terr = np.abs(tap.cpu().numpy() - want) / want
        assert terr.max() <= TAP_BAR[dtype], (term, terr)
        worst_tap = terr.max()
    note(cid, dtype, update_H_ex=worst, tap=worst_tap)


# ----------------------------------------------------------------------------------------------------------------------
# 5. the refusals of to_vol, through every entry
# ----------------------------------------------------------------------------------------------------------------------
def _entry_call(be, entry, g, b):
    """(return code, the buffers the entry may write) of one entry on the geometry g."""
    lib, ctx, s, ref = be._lib, be._ctx, be._stream(), ctypes.byref(g)
    if entry == 'reconstruct':
        return lib.tnmf_hip_reconstruct(ctx, ref, _ptr(b['W']), _ptr(b['Hp']), _ptr(b['R']), s), ('R',)
    if entry == 'grad_H':
        return lib.tnmf_hip_grad_H(ctx, ref, _ptr(b['V']), None, _ptr(b['W']), _ptr(b['Hp']), _ptr(b['neg']), _ptr(b['pos']), s), (
            'neg', 'pos')
    if entry == 'grad_W':
        rc = lib.tnmf_hip_grad_W_fused(ctx, ref, _ptr(b['V']), _ptr(b['W']), _ptr(b['Hp']), _ptr(b['R']), 0, _ptr(b['negpos']), s)
        rc2 = lib.tnmf_hip_grad_W(ctx, ref, _ptr(b['V']), None, _ptr(b['W']), _ptr(b['Hp']), _ptr(b['negpos'][0]), _ptr(b['negpos'][1]), s)
        assert rc == rc2
        return rc, ('R', 'negpos')
    if entry == 'update_H':
        return lib.tnmf_hip_update_H(ctx, ref, _ptr(b['V']), _ptr(b['W']), _ptr(b['Hp']), _ptr(b['R']), 0, EPS, SPARSITY, s), ('Hp', 'R')
    if entry == 'update_H_ex':
        return call_update_H_ex(be, g, 'valid', b['V'], b['W'], b['Hp'], b['R'], 0.05, 0.1, 0.05, [np.ones(3)] * 3), ('Hp', 'R')
    if entry == 'pad_H':
        return lib.tnmf_hip_pad_H(ctx, ref, _lib.MODES['circular'], _ptr(b['H']), _ptr(b['Hp']), s), ('Hp',)
    raise KeyError(entry)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('entry', vd.ENTRIES)
def test_entries_refuse_what_to_vol_refuses(entry, dtype):
    G = vd.REFUSAL_GEOMETRY
    be = backend(G, np.zeros((G[0], G[1]) + G[2]), dtype)
    b = _buffers(G, 'circular', dtype)            # (H in the shape of the sample: what tnmf_hip_pad_H reads; Hp: the 'valid' H)
    for name, err in vd.TO_VOL_REFUSALS.items():
        bad, code, stride, mirror = vd.refused_geometry(name)
        assert mirror == err
        before = {k: t.clone() for k, t in b.items()}
        rc, outs = _entry_call(be, entry, geom(bad, dtype, stride=stride, code=code if name == 'dtype_2' else None), b)
        assert rc == E[err], (name, rc)
        assert set(outs) <= set(b)
        for k in b:           # (the entry's outputs, and everything else)
            assert torch.equal(b[k], before[k]), (name, k)
    _context_still_works(be, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_row_stride_bad_modes_and_even_kernels(dtype):
    G = vd.REFUSAL_GEOMETRY
    N, C, D, M, A = G
    be = backend(G, np.zeros((N, C) + D), dtype)
    b = _buffers(G, 'valid', dtype)
    Hx = D[2] + A[2] - 1
    # a row stride equal to the row length is C-contiguous: accepted, the same bits as 0
    outs = []
    for stride in (0, Hx):
        R = poisoned(tuple(b['R'].shape), dtype)
        assert be._lib.tnmf_hip_reconstruct(be._ctx, ctypes.byref(geom(G, dtype, stride=stride)), _ptr(b['W']), _ptr(b['H']), _ptr(R),
                                            be._stream()) == 0
        outs.append(R)
    assert torch.equal(*outs) and not bool(torch.isnan(outs[0]).any())
    g = geom(G, dtype)
    ones = [np.ones(3)] * 3
    H0, R0, Hp0 = b['H'].clone(), b['R'].clone(), b['Hp'].clone()
    for mode in (-1, 4):
        assert call_update_H_ex(be, g, mode, b['V'], b['W'], b['H'], b['R'], 0.05, 0.1, 0.05, ones) == _lib.E_UNSUPPORTED
        assert be._lib.tnmf_hip_pad_H(be._ctx, ctypes.byref(g), mode, _ptr(b['H']), _ptr(b['Hp']), be._stream()) == _lib.E_UNSUPPORTED
    for lens in ((3, 4, 3), (2, 3, 3), (3, 3, 128)):
        assert vd.update_H_ex_arm(vd.vol(G), 'valid', 0.1, 0., lens)[0] == 'E_UNSUPPORTED'
        ks = [np.ones(n) for n in lens]
        assert call_update_H_ex(be, g, 'valid', b['V'], b['W'], b['H'], b['R'], 0.05, 0.1, 0., ks) == _lib.E_UNSUPPORTED
    assert call_update_H_ex(be, g, 'valid', b['V'], b['W'], b['H'], b['R'], 0.05, -0.1, 0., ones) == _lib.E_GEOM
    assert torch.equal(b['H'], H0) and torch.equal(b['R'], R0) and torch.equal(b['Hp'], Hp0)
    _context_still_works(be, dtype)
