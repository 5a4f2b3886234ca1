#!/usr/bin/env python
"""
Times tnmf_hip_activation_correlogram at BASELINE config 3 -- 256 x 1 x 256^2 samples, 32 planes of 12 x 12, float32, H after
a short fit -- as 32 atoms and as 8 atoms in the four orientations of 'rot90', for the default lags (atom_shape - 1 per axis:
23 x 23) and for max_lag = 3, beside the route it replaces on the same activations:

  torch_lag_loop        a Python loop over the half of the lags that is >= 0 in C order of
                        einsum('npyx,nqyx->pq') on shifted views of H, in H's float32, all on the device

HIP events on the launch stream around `--repeats` back-to-back calls after `--warmup` calls; the mean per call is reported.
The share of the f64 matrix peak is the algorithmic flops, 2 N P^2 prod(S) (lags computed), over the kernel's time and
`--f64-matrix-peak-tflops` (the vendor's published figure for the MI355X: 78.6).  Appends one JSON line per measurement to
--out (default profiles/correlogram_bench.jsonl).
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


def half_plane(L, S):
    """The lags >= 0 in C order that can be non-zero."""
    Ly, Lx = min(L[0], S[0] - 1), min(L[1], S[1] - 1)
    return [(0, dx) for dx in range(Lx + 1)] + [(dy, dx) for dy in range(1, Ly + 1) for dx in range(-Lx, Lx + 1)]


def torch_lag_loop(H, L):
    """C[P, P, 2 Ly + 1, 2 Lx + 1] in H's dtype: one einsum per lag of the half plane, the other half its mirror."""
    P, (Sy, Sx) = H.shape[1], H.shape[2:]
    C = torch.zeros((P, P, 2 * L[0] + 1, 2 * L[1] + 1), dtype=H.dtype, device=H.device)
    for dy, dx in half_plane(L, (Sy, Sx)):
        a = H[:, :, :Sy - dy, max(0, -dx):Sx - max(0, dx)]
        b = H[:, :, dy:, max(0, dx):Sx - max(0, -dx)]
        c = torch.einsum('npyx,nqyx->pq', a, b)
        C[:, :, L[0] + dy, L[1] + dx] = c
        C[:, :, L[0] - dy, L[1] - dx] = c.t()
    return C


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--samples', type=int, default=256)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--planes', type=int, default=32)
    ap.add_argument('--atom', type=int, default=12)
    ap.add_argument('--fit-iterations', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--loop-repeats', type=int, default=2)
    ap.add_argument('--f64-matrix-peak-tflops', type=float, default=78.6)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'correlogram_bench.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'correlogram_bench.py measures on the GPU: there is no fallback'
    torch.cuda.set_device(0)
    N, D, A, P = args.samples, (args.size, args.size), (args.atom, args.atom), args.planes
    V = np.random.default_rng(0).random((N, 1) + D, dtype=np.float32)
    lines = []
    for name, transforms, group in (('config3', None, 1), ('config3-rot90', 'rot90', 4)):
        np.random.seed(42)
        nmf = TransformInvariantNMF(n_atoms=P // group, atom_shape=A, backend='hip', transforms=transforms)
        nmf.fit(V, n_iterations=args.fit_iterations, sparsity_H=0.1)
        be, H = nmf._backend, nmf._H
        S = tuple(int(x) for x in H.shape[2:])
        stride = be._row_stride(H) or 0
        geom = _lib.make_geom(N, P, 1, S, (1, 1), be._dtype_code, stride)
        density = float((H > 0).float().mean().item())
        for L in (tuple(a - 1 for a in A), (3, 3)):
            C = torch.empty((P, P, 2 * L[0] + 1, 2 * L[1] + 1), dtype=torch.float64, device=H.device)
            lags = (ctypes.c_int * 3)(*L)

            def kernel():
                _lib.check(be._lib.tnmf_hip_activation_correlogram(be._ctx, ctypes.byref(geom), _ptr(H), lags, 0, _ptr(C),
                                                                   be._stream()), 'tnmf_hip_activation_correlogram')

            t_kernel = timed(kernel, args.warmup, args.repeats)
            loop = [None]

            def torch_route():
                loop[0] = torch_lag_loop(H, L)

            t_loop = timed(torch_route, 1, args.loop_repeats)
            got, want = C.cpu().numpy(), loop[0].double().cpu().numpy()
            diff = float(np.max(np.abs(got - want)) / np.max(np.abs(got)))
            n_lags = len(half_plane(L, S))
            flops = 2. * N * P * P * S[0] * S[1] * n_lags
            tflops = flops / t_kernel / 1e9
            line = dict(tool='correlogram_bench', config=name, dtype='float32', N=N, planes=P, group=group, shift_shape=list(S),
                        A=list(A), max_lag=list(L), lags_computed=n_lags, fit_iterations=args.fit_iterations,
                        h_density=round(density, 4), h_row_stride=int(stride), warmup=args.warmup, repeats=args.repeats,
                        loop_repeats=args.loop_repeats, correlogram_ms=round(t_kernel, 3), torch_lag_loop_ms=round(t_loop, 3),
                        torch_lag_loop_over_correlogram=round(t_loop / t_kernel, 3), algorithmic_flops=flops,
                        correlogram_tflops=round(tflops, 3), f64_matrix_peak_tflops=args.f64_matrix_peak_tflops,
                        share_of_f64_matrix_peak=round(tflops / args.f64_matrix_peak_tflops, 4),
                        largest_difference_to_the_float32_loop_over_largest_entry=diff,
                        device=torch.cuda.get_device_name(0))
            print(json.dumps(line))
            lines.append(line)
        del nmf, H
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
