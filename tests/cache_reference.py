"""
Float64 host evaluation of the sequences of tests/cache_dispatch.py, built from the oracle's pieces (reconstruct,
_correlate_with_W, _correlate_H_with, multiplicative_update, pad / fold, the lateral convolution) and numpy for the fields
of the beta-divergence.  Shared by tests/test_cache_dispatch_cpu.py (is a stale spectrum far from the right answer?) and
tests/test_hip_cache_matrix.py (the oracle carried along every sequence).

Every step is written in terms of the operands *as the spectra see them* (Hs, Vs, Ws) next to the operands in memory:
with Hs = H, Vs = V, Ws = W it is the oracle's answer; with one of them replaced by what the buffer held when its spectra
were last computed it is the answer a stale cache hit would give.
"""
import numpy as np

import cache_dispatch as cd
import transform_reference as tref
from oracle import tnmf_oracle as orc

EPS = 1e-9
BETA = 1.0                       # the beta-divergence steps of the sequences are Kullback-Leibler steps
INHIBITION, CROSS = 0.1, 0.05    # the lateral step (the project's usual strengths)
LARGE = 292                      # samples of the buffers HL / VL: 292 x 3 x 24 x 25 >= 2^19 > 291 x 3 x 24 x 25


def relmax(got, want):
    want = np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max()
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / (scale if scale > 0 else 1.0))


def kernels():
    return orc.inhibition_kernels(tuple(a - 1 for a in cd.A0))


def capacities(seq):
    """elements of every buffer a sequence may name, in units of its own geometry."""
    g = cd.geo(seq.cls, seq.dtype, 1)
    h1 = g.M * cd.shift(g)[0] * cd.shift(g)[1]
    v1 = 3 * g.D[0] * g.D[1]                 # (room for the calls with C = 3)
    w = g.M * 3 * g.A[0] * g.A[1]
    cap = {'H': 8 * h1, 'V': 8 * v1, 'G': 3 * h1, 'U': 3 * v1, 'HC': 2 * g.M * g.D[0] * g.D[1], 'W': w, 'W2': w,
           'R': 8 * v1, 'NP': 2 * w, 'GX': 3 * h1, 'WX': w, 'RX': 8 * v1,
           # the effective dictionary of the flip group (2 x M atoms), a gradient of its shape, weights shaped like V
           'WE': 2 * w, 'NPE': 4 * w, 'GW': 8 * v1}
    if any('HL' in (kw.get('H') or ()) for _, kw in seq.ops):
        cap['HL'] = LARGE * h1
        cap['R'] = LARGE * v1
    return cap


def initial(seq, seed=5):
    """name -> flat float64 array: positive activations, samples and (unnormalised) dictionaries."""
    rng = np.random.default_rng(seed)
    buf = {name: rng.random(n) + 0.05 for name, n in sorted(capacities(seq).items())}
    buf['U'] *= 3.0     # (sums over a whole sample tell two draws of one distribution apart by 1e-3 only)
    # (values that float32 holds exactly: the float32 kernels and the float64 oracle start from the same numbers)
    return {name: a.astype(np.float32).astype(np.float64) for name, a in buf.items()}


def view(flat, first, shape, row=None):
    """The elements of `flat` from `first` on as an array of `shape`, its rows `row` elements apart."""
    if row is None or row == shape[-1]:
        n = int(np.prod(shape))
        return flat[first:first + n].reshape(shape)
    padded = tuple(shape[:-1]) + (row,)
    n = int(np.prod(padded))
    return flat[first:first + n].reshape(padded)[..., :shape[-1]]


def fields(V, R, beta):
    Rt = np.maximum(R, 0.) + EPS
    return V * Rt ** (beta - 2.), Rt ** (beta - 1.)


class Host:
    def __init__(self, seq):
        self.seq = seq
        self.buf = initial(seq)
        self.es = cd.ESIZE[seq.dtype]
        # what a buffer held when its spectra were last computed: {(kind, buffer, first element, shape): copy}
        self.seen = {}

    # -- operands of one operation
    def operands(self, kw):
        seq = self.seq
        g, dtype, H, V, W = cd.call_of(seq, kw)
        es = cd.ESIZE[seq.dtype]     # (pointers are in units of the sequence's own element size)
        out = {'g': g}
        if H is not None:
            name = H[0] if dtype == seq.dtype else 'GX'
            # (a mode other than 'valid': the activations have the mode's own shift shape, 'circular': the sample's)
            shape = cd.shift(g) if kw.get('mode', 'valid') == 'valid' else g.D
            out['H'] = (name, H[1] // es, (g.N, g.M) + shape, cd.stride(g) if kw.get('mode', 'valid') == 'valid' else None)
        if V is not None:
            out['V'] = (V[0], V[1] // es, (g.N, g.C) + g.D, None)
        if W is not None:
            name = W[0] if dtype == seq.dtype else 'WX'
            out['W'] = (name, 0, (g.M, g.C) + g.A, None)
        return out

    def get(self, ref):
        name, first, shape, row = ref
        return view(self.buf[name], first, shape, row)

    def samples(self, ref):
        """The per-sample keys of an H or V operand."""
        name, first, shape, row = ref
        per = int(np.prod(shape[1:-1])) * (row or shape[-1])
        return [(name, first + i * per, shape[1:], row) for i in range(shape[0])]

    def stale(self, kind, ref, slot=None):
        """The operand as its last computed spectra saw it, or None when nothing differs (or nothing was computed)."""
        cur = self.get(ref)
        if kind == 'W':
            old = self.seen.get(('W', ref[0], ref[2]))
            return None if old is None or np.array_equal(old, cur) else old
        out, differs = cur.copy(), False
        for i, key in enumerate(self.samples(ref) if slot is None else [('slot', slot[0], slot[1] + j) for j in range(len(cur))]):
            old = self.seen.get((kind,) + key)
            if old is not None and old.shape != cur[i].shape:
                old = None
            if old is not None and not np.array_equal(old, cur[i]):
                out[i], differs = old, True
        return out if differs else None

    def note(self, kind, ref, slot=None):
        cur = self.get(ref)
        if slot is not None:
            for i in range(len(cur)):
                self.seen[(kind, 'slot', slot[0], slot[1] + i)] = cur[i].copy()
        if kind == 'W':
            self.seen[('W', ref[0], ref[2])] = cur.copy()
            return
        for i, key in enumerate(self.samples(ref)):
            self.seen[(kind,) + key] = cur[i].copy()

    # -- the arithmetic of one operation; -> {output name: array or float}
    def evaluate(self, step, Hs=None, Vs=None, Ws=None, commit=True):
        name, kw = step
        o = self.operands(kw)
        g = o['g']
        H = self.get(o['H']) if 'H' in o else None
        V = self.get(o['V']) if 'V' in o else None
        W = self.get(o['W']) if 'W' in o else None
        Hs = H if Hs is None else Hs
        Vs = V if Vs is None else Vs
        Ws = W if Ws is None else Ws
        A = g.A
        if name in ('reconstruct', 'energy'):
            R = orc.reconstruct(Ws, Hs)
            return {'R': R} if name == 'reconstruct' else {'energy': float(0.5 * np.sum(np.square(V - R)))}
        if name == 'grad_H':
            R = orc.reconstruct(W, H) if kw.get('r_given') else orc.reconstruct(Ws, Hs)
            return {'neg': orc._correlate_with_W(W, Vs), 'pos': orc._correlate_with_W(W, R)}
        if name == 'grad_W':
            R = orc.reconstruct(W, H) if kw.get('r_is_valid') else orc.reconstruct(Ws, Hs)
            Q, P = fields(V, R, BETA) if kw.get('beta') else (Vs, R)
            NP = np.stack([orc._correlate_H_with(Q, Hs, A), orc._correlate_H_with(P, Hs, A)])
            if commit:
                self.buf['NP'][:NP.size] = NP.ravel()
            return {'NP': NP}
        if name == 'update_H':
            mode = kw.get('mode', 'valid')
            if mode != 'valid':
                Hp = orc.pad_activations(H, A, mode)
                R = orc.reconstruct(W, Hp)
                Q, P = fields(V, R, BETA) if kw.get('beta') else (V, R)
                neg = orc.fold_gradient(orc._correlate_with_W(W, Q), H.shape[2:], A, mode)
                pos = orc.fold_gradient(orc._correlate_with_W(W, P), H.shape[2:], A, mode)
            else:
                R = orc.reconstruct(W, H) if kw.get('r_is_valid') else orc.reconstruct(Ws, Hs)
                # (under 'hybrid' the direct kernels read V itself; under 'fft' its spectra)
                Q, P = fields(V, R, BETA) if kw.get('beta') else (Vs if self.seq.path == 'fft' else V, R)
                if kw.get('weighted'):      # the weighted Kullback-Leibler step: the beta fields times the weights
                    G = self.get(('GW',) + o['V'][1:])
                    Q, P = (G * f for f in fields(V, R, BETA))
                neg, pos = orc._correlate_with_W(W, Q), orc._correlate_with_W(W, P)
            if kw.get('lateral'):
                conv = orc.convolve_multi_1d(H, kernels(), range(-2, 0))
                pos = pos + INHIBITION * (conv - H) + (CROSS / (g.M - 1)) * (conv.sum(axis=1, keepdims=True) - conv)
            new = H * neg / (pos + EPS)
            if commit:
                H[...] = new
            return {'H': new}
        if name == 'mu_update':
            ref = self.arr_of(kw)
            new = self.get(ref) * 0.5
            if commit:
                self.get(ref)[...] = new
            return {'arr': new}
        if name == 'normalize_W':
            new = W / W.sum(axis=(-2, -1), keepdims=True)
            if commit:
                W[...] = new
            return {'W': new}
        if name == 'apply_W':
            NP = self.buf['NP'][:2 * W.size].reshape((2,) + W.shape)
            new = W * NP[0] / (NP[1] + EPS)
            new = new / new.sum(axis=(-2, -1), keepdims=True)
            if commit:
                W[...] = new
            return {'W': new}
        if name in ('group_expand_W', 'ops_expand_W', 'group_apply_W', 'ops_apply_W'):
            # the flip group, and the same two maps as an atom-operator handle: W_eff[2m] = W[m], W_eff[2m + 1] = W[m] mirrored
            new = W
            if name.endswith('apply_W'):
                NPE = self.buf['NPE'][:4 * W.size].reshape((2, 2 * g.M, g.C) + g.A)
                new = W * tref.fold(NPE[0], 'flip') / (tref.fold(NPE[1], 'flip') + EPS)
                new = new / new.sum(axis=(-2, -1), keepdims=True)
            WE = tref.expand(new, 'flip')
            if commit:
                W[...] = new
                self.buf['WE'][:WE.size] = WE.ravel()
            return {'W': new, 'WE': WE}
        if name == 'run_schedule':
            assert commit
            for kind, n0, n1 in kw['ops']:
                sub = dict(N=n1 - n0, H=('H', n0), V=('V', n0), W='W')
                if kind == 'update_H':
                    self.evaluate(('update_H', sub))
                elif kind == 'grad_W':
                    self.evaluate(('grad_W', sub))            # (a, b) = (0, 1): acc = the gradient
                else:
                    self.evaluate(('apply_W', dict(W='W')))
            full = cd.geo(self.seq.cls, self.seq.dtype, cd.NB)
            return {'H': view(self.buf['H'], 0, (full.N, full.M) + cd.shift(full)).copy(),
                    'W': view(self.buf['W'], 0, (full.M, full.C) + full.A).copy()}
        if name == 'host_write':
            Wb = view(self.buf[kw['buf']], 0, (cd.M0, cd.channels(self.seq.cls, self.seq.dtype)) + cd.A0)
            Wb[[0, 1]] = Wb[[1, 0]]
            return {}
        return {}

    def arr_of(self, kw):
        """The operand of a mu_update: `n` samples of activations, or raw = (buffer, first element, count)."""
        if 'raw' in kw:
            buf, first, count = kw['raw']
            return (buf, first, (count,), None)
        buf, sample = kw['arr']
        g = cd.geo(self.seq.cls, self.seq.dtype, kw.get('n', 1))
        per = g.M * cd.shift(g)[0] * cd.shift(g)[1]
        return (buf, sample * per, (g.N, g.M) + cd.shift(g), None)

    # -- one operation: the oracle's outputs, and per recomputed spectrum how far the stale answer would have been
    def step(self, step, model_step, far=True):
        name, kw = step
        o = self.operands(kw) if name not in ('mu_update', 'host_write', 'run_schedule') else {}
        gaps = {}
        if far and name in ('reconstruct', 'energy', 'grad_H', 'grad_W', 'update_H') and kw.get('mode', 'valid') == 'valid':
            right = None
            for what, kind, arg in ((cd.H_ROWS, 'H', 'Hs'), (cd.V_ROWS, 'V', 'Vs'), (cd.W_SPEC, 'W', 'Ws')):
                if what in model_step.recomputed and kind in o:
                    # what this buffer held when it was last transformed, and (samples) what went last through the
                    # sample slots of the binding this call works on
                    for old in (self.stale(kind, o[kind]), self.stale(kind, o[kind], model_step.v_slot) if kind == 'V' and model_step.v_slot else None):
                        if old is None:
                            continue
                        if right is None:
                            right = self.evaluate(step, commit=False)
                        wrong = self.evaluate(step, commit=False, **{arg: old})
                        gaps[what] = min(gaps.get(what, np.inf), max(relmax(wrong[k], right[k]) for k in right))
        # the spectra this call leaves behind belong to the operands as they are NOW ...
        for what, kind in ((cd.H_ROWS, 'H'), (cd.V_ROWS, 'V'), (cd.W_SPEC, 'W')):
            if what in model_step.recomputed and kind in o and not (kind == 'V' and kw.get('beta')):
                self.note(kind, o[kind])
                if kind == 'V' and model_step.v_slot:
                    self.note(kind, o[kind], model_step.v_slot)
        out = self.evaluate(step)
        # ... except the rows k_fft_rows_mu writes: they are the rows of the NEW activations
        if (name == 'update_H' and self.seq.path == 'fft' and kw.get('mode', 'valid') == 'valid' and not kw.get('lateral')
                and 'H' in o):
            self.note('H', o['H'])
        return out, gaps
