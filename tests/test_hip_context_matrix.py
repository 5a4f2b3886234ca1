"""Every entry point on a USED context, at the C ABI, against the host model of tests/context_dispatch.py.

Baseline: every op of context_dispatch.OPS on a context created for it alone, its outputs written over a pattern, held to
the float64 reference and the bar of its family's own test; the same op on a second fresh context gives the same bits (the
project's no-atomics claim, which fails HERE under its own name if it ever does).

History: every sequence of context_dispatch.SEQUENCES on one context (two for `two_contexts`).  Consecutive calls alternate
between two operand sets -- the op's own and another seed scaled by 2^12 -- so that what a predecessor leaves in a buffer is
large, non-zero and never what the successor would have written there itself.  After every call the return code is the
model's, tnmf_hip_ctx_last_path is the baseline's, and every output, host scalars included, equals bit for bit what a fresh
context with the same switches computes from the same operands.  No tolerance: a scratch buffer is not an input.  A refused
call leaves its outputs as they were.

The device operands of an (op, operand set) are allocated once and reused by baseline and history, so branches that look
at an address's alignment take the same side in both.
"""
import contextlib
import ctypes
import functools
import time
from collections import namedtuple

import numpy as np
import pytest
import torch

import atoms_reference as aref
import beta_reference as bref
import context_dispatch as cx
import correlogram_reference as cref
import schedule_dispatch as sd
import schedule_reference as sr
import sources_dispatch as srd
import sources_reference as sref
import weighted_reference as wref
from oracle import tnmf_oracle as orc
from test_hip_atom_gains import ratios as atom_terms_ratios
from test_hip_atom_gram import ratios as atom_gram_ratios
from test_hip_cache_matrix import ORACLE_TOL as FFT_TOL
from test_hip_objective import BAR as ENERGY_BAR
from test_hip_parity import relmax
from test_hip_schedule_matrix import TOL
from test_hip_sources import ratio as sources_ratio
from tnmf_amd import _lib
from tnmf_amd.correlogram_host import activation_correlogram_numpy
from tnmf_amd.sources_host import source_tables

pytestmark = pytest.mark.gpu

NP = {'f': np.float32, 'd': np.float64}
TORCH = {'f': torch.float32, 'd': torch.float64}
U = {'f': 2. ** -24, 'd': 2. ** -53}
PATTERN = -12345.5
EPS, SPARSITY = 1e-9, 0.05
HALF_STEPS = cx.HALF_STEPS
Config = namedtuple('Config', 'path split persistent tap')
SLOWEST = {}


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def p(t, first=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + first * t.element_size())


def kernels_of(k):
    return tuple(f32(x) for x in orc.inhibition_kernels((cx.TAPS // 2,) * k))


def source_sets(M):
    return [[0], list(range(1, M - 1))] if M > 2 else [[0], [1]]


# ---- operands and references, once per (op without its dtype) ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_operands(kind, family, size, which):
    """(V, W, H, acc) -- and the weights G for the weighted kinds -- as float64 images of float32 values, read-only.
    which: 'own', or 'other': another seed, V and H 2^12 times as large."""
    N, C, D, M, A = geometry = cx.GEOMETRY[(family, size)]
    k = len(A)
    orc.set_threads(orc.default_threads(cap=16))
    rng = np.random.default_rng(sum(map(ord, kind + family + size)) + (0 if which == 'own' else 7919))
    Hs = D if kind == 'modes' else cx.shift_shape(geometry)
    W = 0.1 + rng.random((M, C) + A)
    W /= W.sum(axis=tuple(range(-k, 0)), keepdims=True)
    H = 0.05 + rng.random((N, M) + Hs)
    V = 0.1 + rng.random((N, C) + D) * (1. + 0.5 * M)
    acc = 0.5 + rng.random((2, M, C) + A)
    G = (0.5 + rng.random(V.shape)) * (rng.random(V.shape) > 0.2)           # weights, a fifth of them 0 (hidden entries)
    if which == 'other':
        V, H = V * cx.PREDECESSOR_SCALE, H * cx.PREDECESSOR_SCALE
    assert max(np.abs(x).max() for x in (V / (1 + 0.5 * M), W, H)) < cx.OPERAND_MAX * (cx.PREDECESSOR_SCALE if which == 'other' else 1)
    out = tuple(f32(x) for x in (V, W, H, acc, G))
    for x in out:
        x.setflags(write=False)
    return out if kind.endswith('_weighted') else out[:4]


def impl_of(geometry):
    return 'c' if len(geometry[4]) < 3 else 'contract'


@contextlib.contextmanager
def beta_impl(impl):
    """beta_reference on the oracle's C flavour for the larger problems, and back."""
    was, bref.IMPL = bref.IMPL, impl
    try:
        yield
    finally:
        bref.IMPL = was


def step_reference(op, V, W, H, mode='valid', lateral=False, beta=None):
    geometry = cx.geometry_of(op)
    if beta is not None:
        want = H.copy()
        with beta_impl(impl_of(geometry)):
            bref.update_H(V, W, want, slice(None), beta=beta, eps=EPS, sparsity=SPARSITY)
        return want
    ref = orc.OracleNMF(n_atoms=geometry[3], atom_shape=geometry[4], impl=impl_of(geometry), reconstruction_mode=mode)
    ref._kernels = kernels_of(len(geometry[4]))
    ref.V, ref.W, ref.H = V, W, H.copy()
    inh, cross = cx.STRENGTHS if lateral else (0., 0.)
    ref.update_H(slice(None), sparsity=SPARSITY, inhibition=inh, cross_inhibition=cross if geometry[3] > 1 else 0.)
    return ref.H


def per_sample_objective(op, V, W, H, mode='valid', beta=2.):
    R = orc.reconstruct(W, H, impl_of(cx.geometry_of(op)), mode)
    return np.array([bref.divergence(V[n], R[n], beta, EPS) for n in range(V.shape[0])])


# ---- the device side of one (op, operand set) -------------------------------------------------------------------------------
class Slot:
    """Device operands, work copies and outputs of one (op, operand set): made once."""

    def __init__(self, op, which):
        self.op, self.which = op, which
        N, C, D, M, A = self.geometry = cx.geometry_of(op)
        dt, T = TORCH[op.T], op.T
        V, W, H, acc, *G = host_operands(op.kind, op.family, op.size, which)
        d = lambda a: torch.from_numpy(np.array(a, dtype=NP[T])).cuda()  # noqa: E731
        self.V, self.W0, self.H0, self.acc0 = d(V), d(W), d(H), d(acc)
        self.W, self.H, self.acc = self.W0.clone(), self.H0.clone(), self.acc0.clone()
        self.NP = torch.empty((2, M, C) + A, dtype=dt, device='cuda')
        self.tap = torch.empty(N, dtype=torch.float64, device='cuda')
        self.G = d(G[0]) if G else None
        if op.kind == 'reconstruct':
            self.R = torch.empty_like(self.V)
        if op.kind == 'grad_H':
            self.neg, self.pos = torch.empty_like(self.H0), torch.empty_like(self.H0)
        self.obj = torch.empty(N, dtype=torch.float64, device='cuda')
        k = op.kind
        if k == 'atom_terms':
            self.ab = torch.empty((N, M, 2), dtype=torch.float64, device='cuda')
        if k == 'atom_gram':
            self.a = torch.empty((N, M), dtype=torch.float64, device='cuda')
            self.B = torch.empty((N, M, M), dtype=torch.float64, device='cuda')
        if k == 'atom_sources':
            self.sets = source_sets(M)
            self.order, self.start = (torch.from_numpy(x).cuda() for x in source_tables(self.sets))
            self.out = torch.empty((N, len(self.sets), C) + D, dtype=dt, device='cuda')
        if k == 'correlogram':
            self.C = torch.empty((M, M) + (2 * cx.CORR_LAG + 1,) * len(A), dtype=torch.float64, device='cuda')
        self.kern = [(np.ascontiguousarray(x), len(x)) for x in kernels_of(len(A))]

    def restore(self):
        self.W.copy_(self.W0)
        self.H.copy_(self.H0)
        self.acc.copy_(self.acc0)
        for name in ('NP', 'tap', 'obj', 'ab', 'a', 'B', 'out', 'C', 'R', 'neg', 'pos'):
            if hasattr(self, name):
                getattr(self, name).fill_(PATTERN)


@functools.lru_cache(maxsize=None)
def slot(op, which):
    return Slot(op, which)


def kernel_args(s, k):
    """(kernel0, len0, kernel1, len1, kernel2, len2) of tnmf_hip_update_H_ex for k shift axes."""
    out = []
    for i in range(3):
        if i < k:
            arr, n = s.kern[i]
            out += [arr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n]
        else:
            out += [None, 0]
    return out


def stop_on_device_error(rc):
    """A positive return code is a hipError_t, and so is a failed synchronisation: nothing more runs on the device."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device error: {e}', returncode=3)
    if rc > 0:
        pytest.exit(f'HIP error {rc} from the library', returncode=3)


def call(lib, ctx, cfg, op, which, n_ops=None):
    """One call of `op` on the operand set `which` -> (return code, last path, {output: bytes})."""
    s = slot(op, which)
    s.restore()
    N, C, D, M, A = s.geometry
    kind, code = op.kind, 0 if op.T == 'f' else 1
    geom = _lib.make_geom(N, M, C, D, A, code)
    g = ctypes.byref(geom)
    out = {}
    if kind in HALF_STEPS:
        _lib.check(lib.tnmf_hip_ctx_set_objective_tap(ctx, p(s.tap) if cfg.tap else None), 'set_objective_tap')
    if kind == 'energy':
        e = ctypes.c_double(PATTERN)
        rc = lib.tnmf_hip_energy(ctx, g, p(s.V), p(s.W), p(s.H), ctypes.byref(e), None)
        out['energy'] = np.array([e.value])
    elif kind in ('energy_beta', 'energy_weighted'):
        e = ctypes.c_double(PATTERN)
        if kind == 'energy_beta':
            rc = lib.tnmf_hip_energy_beta(ctx, g, cx.BETA, EPS, p(s.V), p(s.W), p(s.H), ctypes.byref(e), None)
        else:
            rc = lib.tnmf_hip_energy_weighted(ctx, g, cx.BETA, EPS, p(s.V), p(s.G), p(s.W), p(s.H), ctypes.byref(e), None)
        out['energy'] = np.array([e.value])
    elif kind == 'reconstruct':
        rc = lib.tnmf_hip_reconstruct(ctx, g, p(s.W), p(s.H), p(s.R), None)
        out['R'] = s.R
    elif kind == 'grad_H':
        rc = lib.tnmf_hip_grad_H(ctx, g, p(s.V), None, p(s.W), p(s.H), p(s.neg), p(s.pos), None)
        out['neg'], out['pos'] = s.neg, s.pos
    elif kind == 'grad_W_unfused':
        rc = lib.tnmf_hip_grad_W(ctx, g, p(s.V), None, p(s.W), p(s.H), p(s.NP[0]), p(s.NP[1]), None)
        out['NP'] = s.NP
    elif kind == 'grad_W_weighted':
        rc = lib.tnmf_hip_grad_W_weighted(ctx, g, p(s.V), p(s.G), p(s.W), p(s.H), None, 0, p(s.NP), cx.BETA, EPS, None)
        out['NP'] = s.NP
    elif kind == 'update_H_weighted':
        rc = lib.tnmf_hip_update_H_weighted(ctx, g, 0, p(s.V), p(s.G), p(s.W), p(s.H), None, EPS, SPARSITY, 0., 0., None, 0, None, 0,
                                            None, 0, cx.BETA, None)
        out['H'] = s.H
    elif kind == 'grad_W':
        rc = lib.tnmf_hip_grad_W_fused(ctx, g, p(s.V), p(s.W), p(s.H), None, 0, p(s.NP), None)
        out['NP'] = s.NP
    elif kind == 'grad_W_beta':
        rc = lib.tnmf_hip_grad_W_beta(ctx, g, p(s.V), p(s.W), p(s.H), None, 0, p(s.NP), cx.BETA, EPS, None)
        out['NP'] = s.NP
    elif kind == 'update_H':
        rc = lib.tnmf_hip_update_H(ctx, g, p(s.V), p(s.W), p(s.H), None, 0, EPS, SPARSITY, None)
        out['H'] = s.H
    elif kind in ('lateral', 'lateral_fallback', 'modes'):
        inh, cross = cx.STRENGTHS
        rc = lib.tnmf_hip_update_H_ex(ctx, g, _lib.MODES['circular' if kind == 'modes' else 'valid'], p(s.V), p(s.W), p(s.H), None,
                                      EPS, SPARSITY, inh, cross, *kernel_args(s, len(A)), None)
        out['H'] = s.H
    elif kind == 'update_H_beta':
        rc = lib.tnmf_hip_update_H_beta(ctx, g, 0, p(s.V), p(s.W), p(s.H), None, EPS, SPARSITY, 0., 0., None, 0, None, 0, None, 0,
                                        cx.BETA, None)
        out['H'] = s.H
    elif kind == 'sample_objective':
        rc = lib.tnmf_hip_sample_objective(ctx, g, 2., EPS, p(s.V), None, p(s.W), p(s.H), p(s.obj), None)
        out['objective'] = s.obj
    elif kind == 'atom_terms':
        rc = lib.tnmf_hip_atom_terms(ctx, g, 1, p(s.V), None, None, p(s.W), p(s.H), p(s.ab), None)
        out['ab'] = s.ab
    elif kind == 'atom_gram':
        rc = lib.tnmf_hip_atom_gram(ctx, g, 1, p(s.V), None, None, p(s.W), p(s.H), p(s.a), p(s.B), None)
        out['a'], out['B'] = s.a, s.B
    elif kind == 'atom_sources':
        rc = lib.tnmf_hip_atom_sources(ctx, g, len(s.sets), p(s.order), int(s.order.numel()), p(s.start), srd.EMIT['masked'], EPS,
                                       p(s.V), p(s.W), p(s.H), p(s.out), None, None, None)
        out['masked'] = s.out
    elif kind == 'correlogram':
        hg = _lib.make_geom(N, M, 1, cx.shift_shape(s.geometry), (1,) * len(A), code)
        lags = (ctypes.c_int * 3)(*((cx.CORR_LAG,) * len(A)))
        rc = lib.tnmf_hip_activation_correlogram(ctx, ctypes.byref(hg), p(s.H), lags, 0, p(s.C), None)
        out['C'] = s.C
    elif kind == 'schedule':
        ops = cx.schedule_list(len(cx.SCHEDULE_OPS) if n_ops is None else n_ops, N)
        arr = (_lib.Op * len(ops))()
        for i, o in enumerate(ops):
            arr[i].kind = sd.KINDS[o[0]]
            arr[i].n0, arr[i].n1 = sd.rng_of(o)
            if o[0] == 'G':
                arr[i].a, arr[i].b = float(o[3]), float(o[4])
        rc = lib.tnmf_hip_run_schedule(ctx, g, p(s.V), p(s.W), p(s.H), None, p(s.acc), arr, len(ops), EPS, SPARSITY, None)
        out['W'], out['H'], out['acc'] = s.W, s.H, s.acc
    else:
        raise KeyError(kind)
    stop_on_device_error(rc)
    if kind in HALF_STEPS:
        out['tap'] = s.tap
    path = lib.tnmf_hip_ctx_last_path(ctx).decode()
    return rc, path, {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()).copy() for k, v in out.items()}


def refuse(lib, ctx, which):
    """One call an argument check refuses -> (return code, whether every output still holds what it held)."""
    s = slot(cx.Op('atom_terms', '2d', cx.SMALL, 'f'), 'own')
    s.restore()
    N, C, D, M, A = s.geometry
    if which == 'correlogram_lag_beyond_limit':
        c = slot(cx.Op('correlogram', '2d', cx.SMALL, 'f'), 'own')
        c.restore()
        hg = _lib.make_geom(N, M, 1, cx.shift_shape(c.geometry), (1, 1), 0)
        rc = lib.tnmf_hip_activation_correlogram(ctx, ctypes.byref(hg), p(c.H), (ctypes.c_int * 3)(64, 1, 0), 0, p(c.C), None)
        torch.cuda.synchronize()
        return rc, bool((c.C == PATTERN).all())
    if which == 'atom_terms_group_not_dividing_M':
        geom = _lib.make_geom(N, M, C, D, A, 0)
        rc = lib.tnmf_hip_atom_terms(ctx, ctypes.byref(geom), 2, p(s.V), None, None, p(s.W), p(s.H), p(s.ab), None)
    elif which == 'atom_terms_of_a_volume':
        geom = _lib.make_geom(1, 1, 1, (2, 2, 2), (1, 1, 1), 0)
        rc = lib.tnmf_hip_atom_terms(ctx, ctypes.byref(geom), 1, p(s.V), None, None, p(s.W), p(s.H), p(s.ab), None)
    elif which == 'update_H_mfma_row_padded':
        Hx = cx.shift_shape(s.geometry)[-1]
        geom = _lib.make_geom(1, M, C, D, A, 0, Hx + 1)       # (one sample: the two of H hold its padded rows)
        rc = lib.tnmf_hip_update_H(ctx, ctypes.byref(geom), p(s.V), p(s.W), p(s.H), None, 0, EPS, SPARSITY, None)
        torch.cuda.synchronize()
        return rc, bool(torch.equal(s.H, s.H0))
    else:
        raise KeyError(which)
    torch.cuda.synchronize()
    return rc, bool((s.ab == PATTERN).all())


class Ctx:
    def __init__(self, lib):
        self.lib = lib
        self.ctx = ctypes.c_void_p()
        _lib.check(lib.tnmf_hip_ctx_create(torch.cuda.current_device(), ctypes.byref(self.ctx)), 'ctx_create')
        self.cfg = Config('auto', 1, 1, 0)

    def control(self, c):
        lib, ctx = self.lib, self.ctx
        if c.what == 'set_path':
            self.cfg = self.cfg._replace(path=c.value)
            return lib.tnmf_hip_ctx_set_path(ctx, _lib.PATHS[c.value])
        if c.what == 'set_split':
            self.cfg = self.cfg._replace(split=c.value)
            return lib.tnmf_hip_ctx_set_split(ctx, c.value)
        if c.what == 'set_persistent':
            self.cfg = self.cfg._replace(persistent=c.value)
            return lib.tnmf_hip_ctx_set_persistent(ctx, c.value)
        if c.what == 'tap':
            self.cfg = self.cfg._replace(tap=int(c.value))
            return 0
        if c.what == 'reserve':
            fam, T = c.value
            N, C, D, M, A = cx.GEOMETRY[(fam, cx.LARGE)]
            geom = _lib.make_geom(N, M, C, D, A, 0 if T == 'f' else 1)
            return lib.tnmf_hip_ctx_reserve(ctx, ctypes.byref(geom))
        if c.what == 'mark_reserved':
            return 0
        raise KeyError(c.what)

    def close(self):
        self.lib.tnmf_hip_ctx_set_objective_tap(self.ctx, None)
        _lib.check(self.lib.tnmf_hip_ctx_destroy(self.ctx), 'ctx_destroy')


def fresh(lib, cfg):
    c = Ctx(lib)
    for what, value in (('set_path', cfg.path), ('set_split', cfg.split), ('set_persistent', cfg.persistent), ('tap', cfg.tap)):
        assert c.control(cx.Ctl(what, value)) == 0
    return c


@functools.lru_cache(maxsize=None)
def baseline(op, which, cfg, n_ops=None):
    """(return code, last path, outputs) of `op` on a context made for this call alone; a second such context gives the
    same bits."""
    lib = _lib.load()
    got = []
    for _ in range(2):
        c = fresh(lib, cfg)
        try:
            got.append(call(lib, c.ctx, cfg, op, which, n_ops))
        finally:
            c.close()
    (rc, path, out), (rc2, path2, out2) = got
    assert (rc, path) == (rc2, path2), ('two fresh contexts disagree', op, which, cfg)
    for k in out:
        assert out[k].tobytes() == out2[k].tobytes(), ('two fresh contexts give different bits', op, which, cfg, k)
    return rc, path, out


def default_cfg(op):
    return Config(cx.default_path(op), 1, 1, 0)


# ---- the references -------------------------------------------------------------------------------------------------------
def check(name, got, want, bar):
    err = relmax(got, want)
    print(f'    {name}: {err:.2e} (bar {bar:.1e})')
    assert np.all(np.isfinite(got)) and err < bar, (name, err, bar)


def against_reference(op, cfg, out):
    """The outputs of a baseline against the float64 reference of the op's family, at that family's own bar."""
    V, W, H, acc, *G = host_operands(op.kind, op.family, op.size, 'own')
    geometry = N, C, D, M, A = cx.geometry_of(op)
    T, kind, impl = op.T, op.kind, impl_of(cx.geometry_of(op))
    tol = FFT_TOL[T] if cfg.path in ('hybrid', 'fft') else TOL[T]
    if kind == 'energy':
        want = orc.energy(V, W, H, impl)
        check('energy', out['energy'], want, FFT_TOL[T] if cfg.path in ('hybrid', 'fft') else ENERGY_BAR[NP[T]])
    elif kind in ('energy_beta', 'energy_weighted'):
        with beta_impl(impl):
            want = bref.energy(V, W, H, cx.BETA, EPS) if kind == 'energy_beta' else wref.energy(V, G[0], W, H, cx.BETA, EPS)
        err = abs(out['energy'][0] - want) / abs(want)
        print(f'    {kind}: {err:.2e}')
        assert err <= (1e-12 if T == 'd' else 1e-5), (kind, err)          # (tests/test_hip_beta.py, tests/test_hip_weights.py)
    elif kind == 'reconstruct':
        check('R', out['R'], orc.reconstruct(W, H, impl), tol)
    elif kind == 'grad_H':
        neg, pos = orc.gradient_H(V, W, H, slice(None), impl)
        check('neg_H', out['neg'], neg, tol)
        check('pos_H', out['pos'], pos, tol)
    elif kind == 'grad_W_weighted':
        with beta_impl(impl):
            neg, pos = wref.gradient_W(V, G[0], W, H, slice(None), beta=cx.BETA, eps=EPS)
        check('neg_W', out['NP'][0], neg, TOL[T])
        check('pos_W', out['NP'][1], pos, TOL[T])
    elif kind == 'update_H_weighted':
        want = H.copy()
        with beta_impl(impl):
            wref.update_H(V, G[0], W, want, slice(None), beta=cx.BETA, eps=EPS, sparsity=SPARSITY)
        check('H', out['H'], want, TOL[T])
        assert np.all(out['tap'] == PATTERN)
    elif kind in ('grad_W', 'grad_W_unfused'):
        neg, pos = orc.gradient_W(V, W, H, slice(None), impl)
        check('neg_W', out['NP'][0], neg, tol)
        check('pos_W', out['NP'][1], pos, tol)
    elif kind == 'grad_W_beta':
        with beta_impl(impl):
            neg, pos = bref.gradient_W(V, W, H, slice(None), beta=cx.BETA, eps=EPS)
        check('neg_W', out['NP'][0], neg, TOL[T])
        check('pos_W', out['NP'][1], pos, TOL[T])
    elif kind in HALF_STEPS and kind != 'update_H_weighted':
        want = step_reference(op, V, W, H, 'circular' if kind == 'modes' else 'valid', kind in ('lateral', 'lateral_fallback', 'modes'),
                              cx.BETA if kind == 'update_H_beta' else None)
        if not (T == 'f' and cfg.path == 'fft'):      # (float32 activations under path 'fft' carry no parity claim: DESIGN 4b)
            check('H', out['H'], want, TOL[T] if kind == 'update_H_beta' else (tol if cfg.path in ('hybrid', 'fft') else 2 * TOL[T]))
        assert np.all(out['tap'] == PATTERN)
    elif kind == 'sample_objective':
        check('objective', out['objective'], per_sample_objective(op, V, W, H), ENERGY_BAR[NP[T]])
    elif kind in ('atom_terms', 'atom_gram'):
        parts = aref.parts_valid(W, H, 1)
        R = parts.sum(axis=1)
        a, b, scale = aref.terms(parts, V, None, R)
        n = int(np.prod(A))
        if kind == 'atom_terms':
            ra, rb = atom_terms_ratios(out['ab'], dict(a=a, b=b, scale=scale, n=n), U[T], n=M * n + n)
        else:
            flat = parts.reshape(N, M, -1)
            ops = dict(a=a, B=np.einsum('nmx,nkx->nmk', flat, flat), scale=scale, n=n)
            ra, rb = atom_gram_ratios(out['a'], out['B'], ops, 'f32' if T == 'f' else 'f64', n_a=M * n + n)
        print(f'    {kind}: largest error / bound {ra:.3f}, {rb:.3f}')
        assert ra <= 1. and rb <= 1., (kind, ra, rb)
    elif kind == 'atom_sources':
        sets = source_sets(M)
        want = sref.outputs(W, H, V, sets, float(NP[T](EPS)))
        bound = srd.bounds(want, C, M, A, sets, 'f32' if T == 'f' else 'f64')
        r = sources_ratio(out['masked'], want['masked'], bound['masked'])
        print(f'    masked: largest error / bound {r:.3f}')
        assert r <= 1., r
    elif kind == 'correlogram':
        L = (cx.CORR_LAG,) * len(A)
        want = activation_correlogram_numpy(H, L, False)
        r = cref.within_bar(out['C'], want, cx.shift_shape(geometry), L, N)
        print(f'    correlogram: largest error / bar {r:.3f}')
        assert np.all(np.isfinite(out['C'])) and r <= 1., r
    elif kind == 'schedule':
        ops = sd.to_slices(cx.schedule_list(len(cx.SCHEDULE_OPS), N))
        wW, wH, wacc, ch = sr.run(V, W, H, acc, ops, EPS, SPARSITY)
        for name, want in (('W', wW), ('H', wH), ('acc', wacc)):
            check(name, out[name], want, 2 * TOL[T] * max(ch[name], 1))
    else:
        raise KeyError(kind)


# ---- the tests -------------------------------------------------------------------------------------------------------------
def op_id(op):
    return f'{op.kind}-{op.family}-{op.size}-{op.T}'


@pytest.fixture(scope='module', autouse=True)
def timing():
    t0 = time.time()
    yield
    worst = max(SLOWEST.items(), key=lambda kv: kv[1], default=('-', 0.))
    print(f'context matrix: {time.time() - t0:.1f} s in all; slowest test {worst[0]}: {worst[1]:.2f} s')


@pytest.fixture(autouse=True)
def timed(request):
    t0 = time.time()
    yield
    SLOWEST[request.node.name] = time.time() - t0


def test_the_model_is_asked_about_this_device():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f'{cus} compute units')
    assert cx.missing(cus=cus) == [] and cx.check_sizes(cus)
    assert cx.HISTORY_DEPENDENT == {}


@pytest.mark.parametrize('op', cx.OPS, ids=op_id)
def test_baseline(op):
    cfg = default_cfg(op)
    rc, path, out = baseline(op, 'own', cfg)
    print(f'{op_id(op)} under {cfg.path}: rc {rc}, last path {path}')
    assert rc == 0
    for v in out.values():
        assert v.dtype.kind != 'f' or not np.any(np.isnan(v))
    for k, v in out.items():
        if k != 'tap':
            assert not np.any(v == PATTERN), (k, 'the pattern survived')
    against_reference(op, cfg, out)


TAPPED = [op for op in cx.OPS if op.kind in HALF_STEPS]


@pytest.mark.parametrize('op', TAPPED, ids=op_id)
def test_baseline_with_the_objective_tap(op):
    """The tapped half step writes the per-sample objective of the activations it was handed, and steps as without the tap."""
    cfg = default_cfg(op)
    rc, path, out = baseline(op, 'own', cfg._replace(tap=1))
    plain = baseline(op, 'own', cfg)
    assert rc == 0 and path == plain[1] and out['H'].tobytes() == plain[2]['H'].tobytes()
    V, W, H, _, *G = host_operands(op.kind, op.family, op.size, 'own')
    if G:
        R = orc.reconstruct(W, H, impl_of(cx.geometry_of(op)))
        want = np.array([wref.divergence(V[n], G[0][n], R[n], cx.BETA, EPS) for n in range(V.shape[0])])
    else:
        want = per_sample_objective(op, V, W, H, 'circular' if op.kind == 'modes' else 'valid',
                                    cx.BETA if op.kind == 'update_H_beta' else 2.)
    check('tap', out['tap'], want, ENERGY_BAR[NP[op.T]])


@pytest.mark.parametrize('name', sorted(cx.SEQUENCES))
def test_history(name):
    seq = cx.SEQUENCES[name]
    lib = _lib.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    model, _ = cx.run(seq, cus)
    ctxs = {False: Ctx(lib), True: None}
    n_calls = sum(1 for it in seq.items if not isinstance(it[1] if it[0] == 'other' else it, cx.Ctl))
    k = 0
    last_path = {False: 'none', True: 'none'}
    try:
        for i, (item, (rc_model, _)) in enumerate(zip(seq.items, model)):
            other = isinstance(item, tuple) and item[0] == 'other'
            if other and ctxs[True] is None:
                ctxs[True] = Ctx(lib)
            c, item = ctxs[other], (item[1] if other else item)
            where = f'{name} item {i} {"(second context) " if other else ""}{item}'
            if isinstance(item, cx.Ctl):
                if item.what == 'refuse':
                    rc, untouched = refuse(lib, c.ctx, item.value)
                    assert rc == rc_model and untouched, (where, rc, untouched)
                else:
                    assert c.control(item) == rc_model, where
                continue
            op, n_ops = (item[1], item[2]) if item[0] == 'schedule_n' else (item, None)
            which = 'own' if (n_calls - 1 - k) % 2 == 0 else 'other'
            k += 1
            want_rc, want_path, want = baseline(op, which, c.cfg, n_ops)
            rc, path, out = call(lib, c.ctx, c.cfg, op, which, n_ops)
            assert rc == rc_model == want_rc, (where, rc, rc_model, want_rc)
            # (the two entry points that dispatch to no kernel family leave the name of the last primitive call alone)
            assert path == (last_path[other] if op.kind in cx.NO_DISPATCH else want_path), (where, path, want_path)
            last_path[other] = path
            for key in want:
                if op.kind in cx.HISTORY_DEPENDENT:
                    continue
                assert out[key].tobytes() == want[key].tobytes(), (
                    where, which, key, 'differs from a fresh context', float(relmax(out[key], want[key].astype(np.float64))))
    finally:
        for c in ctxs.values():
            if c is not None:
                c.close()
