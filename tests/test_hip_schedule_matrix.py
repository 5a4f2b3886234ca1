"""
The schedule executor, every route of it: tnmf_hip_run_schedule, its persistent kernel k_schedule, the
fused tail k_finalize_blend_apply and the volume variant.  Each case of schedule_dispatch.MATRIX is chosen with the host
mirror so that together they reach every route, every edge of k_schedule's block loops, every fusion and every form of
the accumulator blend (tests/test_schedule_dispatch_cpu.py checks that without a GPU).  A case runs its operation list on
planted positive operands (float64 images of float32 values) and compares W, H AND the gradient accumulator

  * with tests/schedule_reference.py (float64, the list as written) under the project's bar of one fused half step,
    2 * 2e-5 (float32) / 2 * 1e-10 (float64) of the output's maximum, times the longest chain of dependent half steps
    behind that output (counted from the list; at most eight);
  * with the same list handed over one operation per call on the same route: bit for bit where that runs the same device
    functions in the same order (the persistent kernel against itself; the generic kernels in float64), else to the bar;
  * persistent=1 with persistent=2, bit for bit;

then once more on the state the first run left (the accumulator persists, as in ASAG / GSAG).  After every call the route
and the kernel family are the mirror's, samples no H step names are bit-identical, pad columns are zero.  float32 under
path='fft' makes no claim on H, as everywhere in this project.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import schedule_dispatch as sd
import schedule_reference as sr
from oracle import tnmf_oracle as orc
from test_hip_direct_matrix import padded
from test_hip_parity import dev, relmax
from tnmf_amd import _lib
from tnmf_amd.backends.HIP import HIP_Backend

pytestmark = pytest.mark.gpu

TOL = {'f': 2e-5, 'd': 1e-10}          # the project's bar of a primitive; a fused half step: twice that
NP = {'f': np.float32, 'd': np.float64}
BITS = {'f': np.uint32, 'd': np.uint64}
EPS, SPARSITY = 1e-9, 0.05
E_CODE = {'E_UNSUPPORTED': _lib.E_UNSUPPORTED, 'E_GEOM': _lib.E_GEOM, None: 0}
WORST = {}


def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def operands(geometry):
    """(V, W, H, acc) of a geometry, float64 images of float32 values, read-only: V planted (reconstruction of a sparse
    H* under a random dictionary plus a floor), W positive and normalised, H and the accumulator positive."""
    N, C, D, M, A = geometry
    k = len(A)
    orc.set_threads(orc.default_threads(cap=16))
    rng = np.random.default_rng(sum(D) * 1000 + N * 10 + M)
    Hs = tuple(d + a - 1 for d, a in zip(D, A))
    Wt = rng.random((M, C) + A)
    Wt /= Wt.sum(axis=tuple(range(-k, 0)), keepdims=True)
    Ht = rng.random((N, M) + Hs) * (rng.random((N, M) + Hs) < 0.05)
    V = orc.reconstruct(Wt, Ht, 'c' if k < 3 else 'contract') + 0.01 + 0.01 * rng.random((N, C) + D)
    W = 0.1 + rng.random((M, C) + A)
    W /= W.sum(axis=tuple(range(-k, 0)), keepdims=True)
    H = 0.05 + rng.random((N, M) + Hs)
    acc = 0.5 + rng.random((2, M, C) + A)
    out = tuple(f32(x) for x in (V, W, H, acc))
    for x in out:
        x.setflags(write=False)
    return out


def bits_equal(a, b):
    """Bit for bit (NaN payloads included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(BITS['f' if a.dtype == np.float32 else 'd']),
                                                                        b.view(BITS['f' if b.dtype == np.float32 else 'd']))


class Problem:
    """A fresh backend with the geometry's V resident, and device copies of W, H and the accumulator."""

    def __init__(self, geometry, T, path='auto', mode=1, poison=False, pad=False):
        self.geometry, self.T, self.dt = geometry, T, NP[T]
        M, A = geometry[3], geometry[4]
        V, W, H, acc = operands(geometry)
        self.V = V.astype(self.dt)
        self.be = HIP_Backend(path=path, persistent=mode)
        np.random.seed(1)
        self.be.initialize(self.V, tuple(A), M, None, tuple(range(-len(A), 0)))
        self.W, self.acc = dev(W, self.dt), dev(acc, self.dt)
        self.H = padded(dev(H, self.dt)) if pad else dev(H, self.dt)
        self.pad = pad
        if poison:
            self.acc.fill_(float('nan'))

    def raw(self, ops, r_scratch=True, eps=EPS):
        """tnmf_hip_run_schedule through ctypes: the forms the backend never makes.  -> return code."""
        be = self.be
        arr = (_lib.Op * max(1, len(ops)))()
        for i, op in enumerate(ops):
            arr[i].kind = sd.KINDS[op[0]]
            arr[i].n0, arr[i].n1 = sd.rng_of(op)
            if op[0] == 'G':
                arr[i].a, arr[i].b = float(op[3]), float(op[4])
        ld = 0 if self.H.is_contiguous() else self.H.stride(2)
        be._foreign_H()
        geom = be._geom(self.H.shape[0], self.W.shape[0], ld)
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        rc = be._lib.tnmf_hip_run_schedule(be._ctx, ctypes.byref(geom), p(be._V_dev), p(self.W), p(self.H),
                                           p(be._R_scratch) if r_scratch else None, p(self.acc), arr, len(ops), eps, SPARSITY,
                                           be._stream())
        be._foreign_H()
        return rc

    def run(self, ops, r_scratch=True, eps=EPS):
        plain = all(op[0] in 'HG' or op == ('W',) for op in ops)
        if plain and r_scratch:
            self.be.run_schedule(self.V, self.W, self.H, sd.to_slices(ops), self.acc, sparsity=SPARSITY, eps=eps)
            return 0
        return self.raw(ops, r_scratch, eps)

    def state(self):
        torch.cuda.synchronize()
        if self.pad:
            assert not self.H._base[..., self.H.shape[-1]:].any(), 'pad columns written'
        return tuple(t.cpu().numpy() for t in (self.W, self.H, self.acc))


@pytest.fixture(scope='module', autouse=True)
def worst_deviations():
    """After the module: the worst deviation per route, dtype and output next to its bar (DESIGN section 4e quotes them)."""
    yield
    for key, (err, bar) in sorted(WORST.items()):
        print(f'worst {key}: {err:.2e} of {bar:.1e}')


def note(route, T, name, err, bar):
    key = (route, T, name)
    if key not in WORST or err / bar > WORST[key][0] / WORST[key][1]:
        WORST[key] = (err, bar)


def against_reference(tag, route, T, path, geometry, got, start, ops):
    """W, H and acc against the float64 interpreter started from `start`, each under its own bar."""
    N = geometry[0]
    want = sr.run(operands(geometry)[0], *start, sd.to_slices(ops), EPS, SPARSITY)
    ch = want[3]
    for name, g, w in zip(('W', 'H', 'acc'), got, want[:3]):
        if name == 'H' and T == 'f' and path == 'fft':
            continue          # (float32 transform noise in the quotient of two small gradients: no claim)
        bar = 2 * TOL[T] * max(ch[name], 1)
        err = relmax(g, w)
        note(route, T, name, err, bar)
        print(f'    {tag} {name}: {err:.2e} (bar {bar:.1e} = {max(ch[name], 1)} x {2 * TOL[T]:.0e})')
        assert err < bar, (tag, name, err, bar)
    # samples no H step names: bit-identical
    touched = np.zeros(N, dtype=bool)
    for op in ops:
        if op[0] == 'H':
            touched[op[1]:op[2]] = True
    s = np.asarray(start[1]).astype(got[1].dtype)
    assert bits_equal(got[1][~touched], s[~touched]), (tag, 'samples outside every H step were written')
    if not any(op[0] == 'W' for op in ops):
        assert bits_equal(got[0], np.asarray(start[0]).astype(got[0].dtype)), (tag, 'W written without a W update')
    return want


def run_case(geometry, T, path, modes, ops, poison, pad, r_scratch, tag):
    """The three comparisons, twice."""
    N = geometry[0]
    start = operands(geometry)[1:]
    cu = device_cus()
    res = {}
    for mode in modes:
        cl = sd.cell(geometry, T, path, mode, list(ops), pad, r_scratch, cu)
        print(f'  {tag} persistent={mode} on {cu} compute units: {cl.route}, {sorted(cl.edges)}')
        route = cl.route if path in ('auto', 'generic') else f'{cl.route}/{path}'
        pr = Problem(geometry, T, path, mode, poison, pad)
        single = Problem(geometry, T, path, mode, poison, pad)
        first = None
        for rnd in (1, 2):
            rc = pr.run(ops, r_scratch)
            assert rc == 0, (tag, mode, rc)
            assert pr.be.last_schedule_persistent is (cl.route == 'persistent'), (tag, mode, cl.route)
            if cl.last_path is not None:
                assert pr.be.last_path == cl.last_path, (tag, mode, cl.last_path, pr.be.last_path)
            got = pr.state()
            ref_start = start if rnd == 1 else tuple(x.astype(np.float64) for x in first)
            if rnd == 1 and poison:
                ref_start = start[:2] + (np.full_like(start[2], np.nan),)
            against_reference(f'{tag} persistent={mode} run {rnd}', route, T, path, geometry, got, ref_start, ops)
            # the same list, one operation per call
            for op in ops:
                assert single.run([op], r_scratch) == 0
            alone = single.state()
            exact = sd.same_functions(geometry, T, ops) and (
                cl.route == 'persistent' or (cl.route == 'per_op' and T == 'd' and path in ('auto', 'generic')))
            for name, a, b in zip(('W', 'H', 'acc'), got, alone):
                if exact:
                    assert bits_equal(a, b), (tag, mode, rnd, name, 'one call against one operation per call', relmax(a, b))
                elif not (name == 'H' and T == 'f' and path == 'fft'):
                    ch = sr.chains(sd.to_slices(ops), N)
                    bar = 2 * TOL[T] * max(ch[name], 1) * (2 if rnd == 2 else 1)
                    err = relmax(a, b)
                    note(route + ' vs per call', T, name, err, bar)
                    print(f'    {tag} persistent={mode} run {rnd} {name} against one operation per call: {err:.2e} (bar {bar:.1e})')
                    assert err < bar, (tag, mode, rnd, name, err, bar)
            if rnd == 1:
                first = got
            res[(mode, rnd)] = got
        del pr, single
    if 1 in modes and 2 in modes:
        for rnd in (1, 2):
            for a, b in zip(res[(1, rnd)], res[(2, rnd)]):
                assert bits_equal(a, b), (tag, rnd, 'plain against cooperative launch')


CASES = [(cid, T) for cid, c in sd.MATRIX.items() for T in c.dtypes]


@pytest.mark.parametrize('cid,T', CASES, ids=[f'{c}-{t}' for c, t in CASES])
def test_schedule_case(cid, T):
    c = sd.MATRIX[cid]
    print(f'{cid}-{T}: {c.geometry} path={c.path} modes={c.modes}')
    run_case(c.geometry, T, c.path, c.modes, c.ops, c.poison, c.padded, c.r_scratch, f'{cid}-{T}')


@pytest.mark.parametrize('where', ['tiny', 'big'])
@pytest.mark.parametrize('seed', sd.RANDOM_SEEDS)
def test_random_lists(seed, where):
    geometry, modes = (sd.T2, (1, 2, 0)) if where == 'tiny' else (sd.BIG, (1,))
    ops, poison = sd.random_list(seed, geometry[0])
    print(f'seed {seed} on {where}: poison={poison} {ops}')
    for T in 'fd':
        run_case(geometry, T, 'auto', modes, ops, poison, False, True, f'seed {seed} {where}-{T}')


@pytest.mark.parametrize('T', ['f', 'd'])
@pytest.mark.parametrize('where,mode', [('tiny', 1), ('tiny', 0), ('big', 1), ('volume', 1)])
def test_empty_slices_scale_the_accumulator_exactly(where, mode, T):
    """An empty W-gradient slice contributes zeros: acc becomes a * acc EXACTLY in the element type (a == 1: unchanged,
    a == 0: zeros whatever it held), and W and H stay bit-identical; an empty H step changes nothing."""
    geometry = {'tiny': sd.T2, 'big': sd.BIG, 'volume': sd.VOL}[where]
    dt, N, L = NP[T], geometry[0], sd.LAMBDA
    acc0 = operands(geometry)[3].astype(dt)
    for ops, want, poison in (
            ((('G', 3, 3, 1., 1.), ('H', N, N)), acc0, False),
            ((('G', N, N, 1 - L, L),), dt(1 - L) * acc0, False),
            ((('G', 0, 0, 0., L),), np.zeros_like(acc0), True),
            ((('H', 2, 2), ('G', 1, 1, 0., 1.)), np.zeros_like(acc0), True),
            ((('G', 2, 2, 0., 1.), ('G', 1, 1, 1., 1.), ('G', 4, 4, 1 - L, L)), np.zeros_like(acc0), True)):
        pr = Problem(geometry, T, 'auto', mode, poison)
        W0, H0 = pr.W.cpu().numpy(), pr.H.cpu().numpy()
        pr.run(ops)
        W, H, acc = pr.state()
        assert bits_equal(acc, want), (where, mode, T, ops, relmax(acc, want))
        assert bits_equal(W, W0) and bits_equal(H, H0), (where, mode, T, ops)
        assert pr.be.last_schedule_persistent is (where == 'tiny' and mode == 1 and any(op[0] == 'G' for op in ops))


@pytest.mark.parametrize('T', ['f', 'd'])
@pytest.mark.parametrize('where,mode', [('tiny', 1), ('tiny', 0), ('big', 1), ('volume', 1)])
def test_w_update_leaves_acc_pos_incremented_by_eps(where, mode, T):
    """include/tnmf_hip.h: a W update leaves acc_pos incremented by eps (the reference's :232; ASAG / GSAG blend onto that
    across calls).  With eps = 2^-10, which both element types add visibly: after k W updates acc_pos is the old one
    plus eps, k times, each sum rounded once -- bit for bit -- and acc_neg is untouched; the same for the update fused
    behind a W gradient, against the gradient alone."""
    geometry = {'tiny': sd.T2, 'big': sd.BIG, 'volume': sd.VOL}[where]
    dt, eps = NP[T], 2. ** -10
    V, W0, H0, acc0 = operands(geometry)
    for ops, k in (((('W',),), 1), ((('W',), ('W',)), 2), ((('W',), ('G', 1, 1, 1., 1.), ('W',), ('H', 0, 0)), 2)):
        pr = Problem(geometry, T, 'auto', mode)
        pr.run(ops, eps=eps)
        W, H, acc = pr.state()
        want = acc0[1].astype(dt)
        for _ in range(k):
            want = (want + dt(eps)).astype(dt)
        assert bits_equal(acc[1], want), (where, mode, T, ops, relmax(acc[1], want))
        assert bits_equal(acc[0], acc0[0].astype(dt)) and bits_equal(H, H0.astype(dt))
        ref = sr.run(V, W0, H0, acc0, sd.to_slices(ops), eps, SPARSITY)
        assert relmax(W, ref[0]) < 2 * TOL[T], (where, mode, T, ops, relmax(W, ref[0]))
    fused, alone = Problem(geometry, T, 'auto', mode, True), Problem(geometry, T, 'auto', mode, True)
    fused.run((('G', 0, 2, 0., 1.), ('W',)), eps=eps)
    alone.run((('G', 0, 2, 0., 1.),), eps=eps)
    a, b = fused.state()[2], alone.state()[2]
    assert bits_equal(a[0], b[0]) and bits_equal(a[1], (b[1] + dt(eps)).astype(dt))
    ref = sr.run(V, W0, H0, acc0, sd.to_slices((('G', 0, 2, 0., 1.), ('W',))), eps, SPARSITY)
    assert relmax(fused.state()[0], ref[0]) < 2 * TOL[T] and relmax(a, ref[2]) < 2 * TOL[T]


@pytest.mark.parametrize('T', ['f', 'd'])
def test_six_calls_in_flight_on_the_ring_of_pinned_slots(T):
    """Six calls back to back with no synchronisation between them, lists of 3, 200, 5, 130, 1 and 129 operations on the
    tiny route: the fifth and sixth reuse the pinned slots of the first and second (kOpSlots = 4), the lists of 200 and 130
    operations regrow theirs past 4096 bytes (32 bytes per operation).  The fillers are empty W gradients with
    (a, b) = (1, 1): exact no-ops the joining does not drop.  Same bits as with a synchronisation after every call."""
    G, L, N = sd.T2, sd.LAMBDA, sd.T2[0]
    heads = ((('H', 0, 3), ('G', 0, 3, 0., 1.), ('W',)), (('H', 3, 6),), (('G', 3, 6, 1 - L, L), ('W',)), (('H', 6, 10),),
             (('G', 6, 10, 1., 1.),), (('W',),))
    lists = [tuple(h) + tuple(('G', k % (N + 1), k % (N + 1), 1., 1.) for k in range(n - len(h)))
             for h, n in zip(heads, sd.RING_LENGTHS)]
    assert tuple(len(x) for x in lists) == sd.RING_LENGTHS
    plan = sd.ring(sd.RING_LENGTHS)
    assert [p[1] for p in plan] == [False] * 4 + [True] * 2 and sum(p[2] > sd.SLOT_GROWTH for p in plan) == 2
    for mode in (1, 2):
        flight, synced = Problem(G, T, 'auto', mode, True), Problem(G, T, 'auto', mode, True)
        for ops in lists:
            flight.run(ops)
            assert flight.be.last_schedule_persistent
        for ops in lists:
            synced.run(ops)
            torch.cuda.synchronize()
        got, want = flight.state(), synced.state()
        for a, b in zip(got, want):
            assert bits_equal(a, b), (mode, 'calls in flight against synchronised calls')
        start = operands(G)[1:3] + (np.full_like(operands(G)[3], np.nan),)
        flat = tuple(op for ops in lists for op in ops)
        against_reference(f'ring-{T} persistent={mode}', 'persistent', T, 'auto', G, got, start, flat)


REFUSALS = [(kind, name) for kind in sd.REFUSAL_GEOMETRIES for name in sd.REFUSED_LISTS]


@pytest.mark.parametrize('T', ['f', 'd'])
@pytest.mark.parametrize('kind,name', REFUSALS, ids=[f'{k}-{n}' for k, n in REFUSALS])
def test_refusals_come_before_anything_runs(kind, name, T):
    """Every refusal is the host's, for the whole list, before any launch: W, H and acc are bit-identical to copies taken
    before the call.  An unknown kind (first or last in the list) is TNMF_E_UNSUPPORTED, a bad range TNMF_E_GEOM; a W update
    names no samples, so the range it carries is not read; an empty list is TNMF_OK and changes nothing."""
    geometry = sd.REFUSAL_GEOMETRIES[kind]
    ops, err = sd.REFUSED_LISTS[name]
    assert sd.validate(ops, geometry[0]) == err
    for mode in ((1, 0) if kind == 'refusal_2d' else (1,)):
        pr = Problem(geometry, T, 'auto', mode)
        before = pr.state()
        rc = pr.raw(ops)
        after = pr.state()
        assert rc == E_CODE[err], (kind, name, mode, rc)
        if err is not None or not ops:
            for a, b in zip(before, after):
                assert bits_equal(a, b), (kind, name, mode, 'a refused list wrote its operands')
        else:
            # the list runs: the same bits as with a W update that carries no range
            twin = Problem(geometry, T, 'auto', mode)
            assert twin.raw(tuple(('W',) if op[0] == 'W' else op for op in ops)) == 0
            for a, b in zip(after, twin.state()):
                assert bits_equal(a, b), (kind, name, mode)
            assert not bits_equal(after[0], before[0])
        # and the context still works
        assert pr.raw((('H', 0, 1),)) == 0
        assert not bits_equal(pr.state()[1], after[1])
