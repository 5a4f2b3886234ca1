#!/usr/bin/env python
"""
Times tnmf_hip_atom_terms_beta and tnmf_hip_atom_gram_beta (R given) at beta 1, 0 and 1.5 on two problems, float32, H after a
short Kullback-Leibler fit:

  config3        BASELINE config 3: 256 x 1 x 256^2 samples, 32 atoms of 12 x 12
  spectrogram    8 samples of 4096 frames, 257 channels, 16 atoms of 8 taps (one shift axis)

beside two yardsticks on the same operands:

  frobenius      tnmf_hip_atom_terms / tnmf_hip_atom_gram: the same walk over H without the divergence's pixel factors and
                 without the gain epilogue -- what the kernels cost before this entry existed
  per_atom_loop  the route the entry replaces for the gain: partial_reconstruct per atom and the two divergences in torch
                 (float64 on the device), one pass over V per atom

HIP events on the launch stream around `--repeats` back-to-back calls after `--warmup` calls; the mean per call is reported.
Appends one JSON line per (problem, beta) to --out (default profiles/atom_divergence_bench.jsonl).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tnmf_amd import _lib  # noqa: E402
from tnmf_amd.backends.HIP import _ptr  # noqa: E402
from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF  # noqa: E402


def timed(fn, warmup, repeats):
    """Mean milliseconds of fn() over `repeats` calls between two events, after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / repeats


def divergence(V, x, beta):
    """sum over a sample of d_beta(V | x), float64 on the device."""
    if beta == 1:
        d = V * torch.log(V / x) - V + x
    elif beta == 0:
        q = V / x
        d = q - torch.log(q) - 1
    else:
        d = (V ** beta + (beta - 1) * x ** beta - beta * V * x ** (beta - 1)) / (beta * (beta - 1))
    return d.sum(dim=tuple(range(1, V.dim())))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--cases', default='config3,spectrogram')
    ap.add_argument('--betas', default='1,0,1.5')
    ap.add_argument('--samples', type=int, default=256)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--fit-iterations', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--loop-repeats', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'atom_divergence_bench.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'atom_divergence_bench.py measures on the GPU: there is no fallback'
    torch.cuda.set_device(0)
    cases = {'config3': ((args.samples, 1, args.size, args.size), 32, (12, 12)), 'spectrogram': ((8, 257, 4096), 16, (8,))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.cases.split(','):
        shape_V, M, A = cases[name]
        V = np.random.default_rng(0).random(shape_V, dtype=np.float32) + np.float32(0.05)
        np.random.seed(42)
        nmf = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip', beta_loss=1.)
        nmf.fit(V, n_iterations=args.fit_iterations, sparsity_H=0.1)
        be, W, H, eps = nmf._backend, nmf._W_dict, nmf._H, float(nmf.eps)
        lib, ctx, Vd = be._lib, be._ctx, be._V_dev
        R = be.reconstruct(W, H)
        N = int(H.shape[0])
        geom = be._geom(N, M, be._row_stride(H) or 0)
        ab = torch.empty((N, M, 2), dtype=torch.float64, device=H.device)
        abg = torch.empty((N, M, 3), dtype=torch.float64, device=H.device)
        a = torch.empty((N, M), dtype=torch.float64, device=H.device)
        B = torch.empty((N, M, M), dtype=torch.float64, device=H.device)
        ops = (_ptr(Vd), None, _ptr(R), _ptr(W), _ptr(H))

        def terms_frobenius():
            _lib.check(lib.tnmf_hip_atom_terms(ctx, ctypes.byref(geom), 1, *ops, _ptr(ab), be._stream()), 'tnmf_hip_atom_terms')

        def gram_frobenius():
            _lib.check(lib.tnmf_hip_atom_gram(ctx, ctypes.byref(geom), 1, *ops, _ptr(a), _ptr(B), be._stream()),
                       'tnmf_hip_atom_gram')

        t_terms2, t_gram2 = timed(terms_frobenius, args.warmup, args.repeats), timed(gram_frobenius, args.warmup, args.repeats)
        V64, R64 = Vd.double(), R.double()
        for beta in (float(b) for b in args.betas.split(',')):
            def terms():
                _lib.check(lib.tnmf_hip_atom_terms_beta(ctx, ctypes.byref(geom), 1, beta, eps, *ops, _ptr(abg), be._stream()),
                           'tnmf_hip_atom_terms_beta')

            def gram():
                _lib.check(lib.tnmf_hip_atom_gram_beta(ctx, ctypes.byref(geom), 1, beta, eps, *ops, _ptr(a), _ptr(B),
                                                       be._stream()), 'tnmf_hip_atom_gram_beta')

            loop_gain = torch.empty((N, M), dtype=torch.float64, device=H.device)

            def per_atom_loop():
                base = divergence(V64, R64.clamp(min=0) + eps, beta)
                for m in range(M):
                    Rm = be.partial_reconstruct(W, H, m).double()
                    loop_gain[:, m] = divergence(V64, (R64 - Rm).clamp(min=0) + eps, beta) - base

            t_terms, t_gram = timed(terms, args.warmup, args.repeats), timed(gram, args.warmup, args.repeats)
            t_loop = timed(per_atom_loop, 1, args.loop_repeats)
            got, want = abg[..., 2].cpu().numpy(), loop_gain.cpu().numpy()
            diff = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
            line = dict(tool='atom_divergence_bench', config=name, dtype='float32', shape_V=list(shape_V), A=list(A), atoms=M,
                        beta=beta, eps=eps, fit_iterations=args.fit_iterations, warmup=args.warmup, repeats=args.repeats,
                        loop_repeats=args.loop_repeats, atom_terms_beta_ms=round(t_terms, 4),
                        atom_terms_frobenius_ms=round(t_terms2, 4), terms_beta_over_frobenius=round(t_terms / t_terms2, 3),
                        atom_gram_beta_ms=round(t_gram, 4), atom_gram_frobenius_ms=round(t_gram2, 4),
                        gram_beta_over_frobenius=round(t_gram / t_gram2, 3), per_atom_loop_ms=round(t_loop, 3),
                        per_atom_loop_over_terms_beta=round(t_loop / t_terms, 2),
                        largest_gain_difference_to_the_loop_over_largest_gain=diff, device=torch.cuda.get_device_name(0))
            print(json.dumps(line), flush=True)
            with open(args.out, 'a') as f:
                f.write(json.dumps(line) + '\n')
        del nmf, H, R, V64, R64
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
