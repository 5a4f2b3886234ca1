#!/usr/bin/env python
"""
Times tnmf_hip_atom_gram (R given) at BASELINE config 3 -- 256 x 1 x 256^2 samples, 32 planes of 12 x 12, float32 -- as 32
atoms and as 8 atoms in the four orientations of 'rot90', beside two yardsticks on the same operands in the same process:

  atom_terms            tnmf_hip_atom_terms: the same multiply-adds, the diagonal of B only
  stack_and_gram        the only route to B without the entry point: partial_reconstruct per atom (with transforms:
                        reconstruct of the atom's planes, as R_partial does) into a stacked buffer [N, atoms, pixels], then
                        one torch batched matrix product of the stack with itself (float32) and one with the residual

HIP events on the launch stream around `--repeats` back-to-back calls after `--warmup` calls; the mean per call is reported.
Appends one JSON line per configuration to --out (default profiles/atom_gram_bench.jsonl).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tnmf_amd import _lib  # noqa: E402
from tnmf_amd.backends.HIP import HIP_Backend, _ptr  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--samples', type=int, default=256)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--planes', type=int, default=32)
    ap.add_argument('--atom', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'atom_gram_bench.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'atom_gram_bench.py measures on the GPU: there is no fallback'
    torch.cuda.set_device(0)
    N, C, D, A, P = args.samples, 1, (args.size, args.size), (args.atom, args.atom), args.planes
    rng = np.random.default_rng(0)
    V = rng.random((N, C) + D, dtype=np.float32)
    be = HIP_Backend(path='generic', init='device')
    W, H = be.initialize(V, A, P, None, (-2, -1))
    lib, ctx = be._lib, be._ctx
    R = be.reconstruct(W, H)
    Vd = be._V_dev
    d = (Vd - R).reshape(N, -1, 1)
    stride = be._row_stride(H) or 0
    geom = be._geom(N, P, stride)
    taps = A[0] * A[1]
    pixels = C * D[0] * D[1]
    lines = []
    for name, group in (('config3', 1), ('config3-rot90', 4)):
        Mo = P // group
        a = torch.empty((N, Mo), dtype=torch.float64, device=be.device)
        B = torch.empty((N, Mo, Mo), dtype=torch.float64, device=be.device)
        ab = torch.empty((N, Mo, 2), dtype=torch.float64, device=be.device)

        def gram():
            _lib.check(lib.tnmf_hip_atom_gram(ctx, ctypes.byref(geom), group, _ptr(Vd), None, _ptr(R), _ptr(W), _ptr(H),
                                              _ptr(a), _ptr(B), be._stream()), 'tnmf_hip_atom_gram')

        def terms():
            _lib.check(lib.tnmf_hip_atom_terms(ctx, ctypes.byref(geom), group, _ptr(Vd), None, _ptr(R), _ptr(W), _ptr(H),
                                               _ptr(ab), be._stream()), 'tnmf_hip_atom_terms')

        stack = torch.empty((N, Mo, pixels), dtype=torch.float32, device=be.device)
        loop = {}

        def stack_and_gram():
            for m in range(Mo):
                if group == 1:
                    Rm = be.partial_reconstruct(W, H, m)
                else:
                    Rm = be.reconstruct(W[m * group:(m + 1) * group], H[:, m * group:(m + 1) * group])
                stack[:, m] = Rm.reshape(N, pixels)
            loop['B'] = torch.bmm(stack, stack.transpose(1, 2))
            loop['a'] = torch.bmm(stack, d)

        t_gram = timed(gram, args.warmup, args.repeats)
        t_terms = timed(terms, args.warmup, args.repeats)
        t_loop = timed(stack_and_gram, 1, max(2, args.repeats // 3))
        got, want = B.cpu().numpy(), loop['B'].double().cpu().numpy()
        diff = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        diag = float(np.max(np.abs(np.diagonal(got, axis1=1, axis2=2) - ab[..., 1].cpu().numpy())
                            / np.diagonal(got, axis1=1, axis2=2).max()))
        flops = 2. * N * C * D[0] * D[1] * P * taps
        gram_flops = 2. * N * C * D[0] * D[1] * Mo * Mo
        line = dict(tool='atom_gram_bench', config=name, dtype='float32', N=N, C=C, D=list(D), A=list(A), planes=P, group=group,
                    atoms=Mo, warmup=args.warmup, repeats=args.repeats, atom_gram_ms=round(t_gram, 4),
                    atom_terms_ms=round(t_terms, 4), stack_and_gram_ms=round(t_loop, 4),
                    atom_gram_over_atom_terms=round(t_gram / t_terms, 3),
                    stack_and_gram_over_atom_gram=round(t_loop / t_gram, 3),
                    multiply_add_flops=flops, contraction_flops_float64=gram_flops,
                    atom_gram_tflops=round((flops + gram_flops) / t_gram / 1e9, 3), h_row_stride=int(stride),
                    largest_relative_difference_to_the_stacked_product=diff,
                    largest_relative_difference_of_the_diagonal_to_atom_terms=diag,
                    device=torch.cuda.get_device_name(0))
        print(json.dumps(line))
        lines.append(line)
        del stack, loop
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
