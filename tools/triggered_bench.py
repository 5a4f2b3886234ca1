#!/usr/bin/env python
"""
Times tnmf_hip_triggered_sums, float32, on H after a short fit and the residual field of that fit:

  config3            256 x 1 x 256^2 samples, 32 atoms of 12 x 12, the default margin (window 24 x 24)
  config3-margin0    the same, margin 0 (window 12 x 12: the W gradient's own correlation)
  config3-rot90      8 atoms in the four orientations of 'rot90' (32 planes), the default margin
  spectrogram        8 x 257 x 4096 frames, 16 atoms of 8 taps, the default margin (window 16, 257 fields)

beside the routes it replaces on the same operands, each on a line of its own:

  torch_loop         a Python loop over the window positions of einsum('npu,nfu->pf') on shifted views, in float32
                     (minutes on the two-axis shapes; `--loop-from FILE` takes its time from the torch_loop line of the same
                     case in an earlier output of this tool instead of running it again -- the loop does not involve the
                     kernel -- and says so in the line; a case without such a line is recorded as not run)
  torch_conv2d       one grouped torch.nn.functional.conv2d with the (sample, field) pairs as groups (`--conv2d`; a shape
                     the library refuses or that needs more than `--conv2d-max-gib` of weights is recorded as such)

HIP events on the launch stream around `--repeats` back-to-back calls after `--warmup` calls; the mean per call is reported.
The share of the f64 matrix peak is the algorithmic flops, 2 N P F prod(S) prod(window), over the kernel's time and
`--f64-matrix-peak-tflops` (the vendor's published figure for the MI355X: 78.6).  Appends one JSON line per measurement to
--out (default profiles/triggered_bench.jsonl).
"""
import argparse
import ctypes
import itertools
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


def views(Hp, Y, A, m, j):
    """The two shifted views of window position j, or None where it has no term."""
    S, D = Hp.shape[2:], Y.shape[2:]
    off = tuple(jk - (a - 1) - x for jk, a, x in zip(j, A, m))
    lo = tuple(max(0, -o) for o in off)
    hi = tuple(min(s, d - o) for s, d, o in zip(S, D, off))
    if any(h <= l for l, h in zip(lo, hi)):
        return None
    lead = (slice(None), slice(None))
    return (Hp[lead + tuple(slice(l, u) for l, u in zip(lo, hi))],
            Y[lead + tuple(slice(l + o, u + o) for l, u, o in zip(lo, hi, off))])


def torch_loop(Hp, Y, A, m):
    """X[P, F, *(A + 2 m)] in the operands' dtype: one einsum per window position."""
    win = tuple(a + 2 * x for a, x in zip(A, m))
    X = torch.zeros((Hp.shape[1], Y.shape[1]) + win, dtype=Hp.dtype, device=Hp.device)
    sub = 'npu,nfu->pf' if len(A) == 1 else 'npyx,nfyx->pf'
    for j in itertools.product(*(range(w) for w in win)):
        v = views(Hp, Y, A, m, j)
        if v is not None:
            X[(Ellipsis,) + j] = torch.einsum(sub, *v)
    return X


def torch_conv2d(Hp, Y, A, m):
    """The same sums as one grouped cross-correlation: the (sample, field) pairs are the groups, the planes of H the filters."""
    one_axis = len(A) == 1
    if one_axis:
        Hp, Y, A, m = Hp[:, :, None], Y[:, :, None], (1,) + tuple(A), (0,) + tuple(m)
    N, P, F = Hp.shape[0], Hp.shape[1], Y.shape[1]
    pad = [a - 1 + x for a, x in zip(A, m)]
    inp = torch.nn.functional.pad(Y.reshape((1, N * F) + Y.shape[2:]), (pad[1], pad[1], pad[0], pad[0]))
    w = Hp[:, None].expand(N, F, P, *Hp.shape[2:]).reshape((N * F * P, 1) + Hp.shape[2:])
    out = torch.nn.functional.conv2d(inp, w, groups=N * F)
    out = out.reshape((N, F, P) + out.shape[2:]).sum(dim=0).transpose(0, 1)
    return out[:, :, 0] if one_axis else out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--cases', default='config3,config3-margin0,config3-rot90,spectrogram')
    ap.add_argument('--samples', type=int, default=256)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--fit-iterations', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--loop-repeats', type=int, default=1)
    ap.add_argument('--conv2d', action='store_true')
    ap.add_argument('--no-loop', action='store_true', help='time the kernel alone')
    ap.add_argument('--loop-from', default=None, help='an earlier output of this tool: its torch_loop lines are not measured again')
    ap.add_argument('--conv2d-max-gib', type=float, default=4.)
    ap.add_argument('--f64-matrix-peak-tflops', type=float, default=78.6)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'triggered_bench.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'triggered_bench.py measures on the GPU: there is no fallback'
    torch.cuda.set_device(0)
    image = (args.samples, 1, args.size, args.size)
    cases = {'config3': (image, 32, (12, 12), None, None), 'config3-margin0': (image, 32, (12, 12), None, 0),
             'config3-rot90': (image, 8, (12, 12), 'rot90', None), 'spectrogram': ((8, 257, 4096), 16, (8,), None, None)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    earlier = []
    if args.loop_from is not None:
        with open(args.loop_from) as f:
            earlier = [json.loads(line) for line in f if line.strip()]
    fitted = {}
    for name in args.cases.split(','):
        shape_V, n_atoms, A, transforms, margin = cases[name]
        key = (shape_V, n_atoms, transforms)
        if key not in fitted:
            fitted.clear()
            torch.cuda.empty_cache()
            V = np.random.default_rng(0).random(shape_V, dtype=np.float32)
            np.random.seed(42)
            nmf = TransformInvariantNMF(n_atoms=n_atoms, atom_shape=A, backend='hip', transforms=transforms)
            nmf.fit(V, n_iterations=args.fit_iterations, sparsity_H=0.1)
            fitted[key] = nmf
        nmf = fitted[key]
        be = nmf._backend
        m = nmf._margin(margin)
        Hp = be._pad(nmf._H)
        Y = be.triggered_field(nmf._V, nmf._W_dict, nmf._H, 'residual').contiguous()
        N, P, F = int(Hp.shape[0]), int(Hp.shape[1]), int(Y.shape[1])
        S, win = tuple(int(x) for x in Hp.shape[2:]), tuple(a + 2 * x for a, x in zip(A, m))
        stride = be._row_stride(Hp) or 0
        Hc = Hp if be._row_stride(Hp) is not None else Hp.contiguous()
        geom = be._geom(N, P, stride)
        mc = (ctypes.c_int * 3)(*m)
        need = ctypes.c_size_t(0)
        _lib.check(be._lib.tnmf_hip_triggered_sums_plan(be._ctx, ctypes.byref(geom), F, mc, 0, ctypes.byref(need)),
                   'tnmf_hip_triggered_sums_plan')
        work = torch.empty(max(1, need.value), dtype=torch.uint8, device=Hp.device)
        X = torch.empty((P, F) + win, dtype=torch.float64, device=Hp.device)

        def kernel():
            _lib.check(be._lib.tnmf_hip_triggered_sums(be._ctx, ctypes.byref(geom), _ptr(Hc), _ptr(Y), F, mc, 1, 0, _ptr(work),
                                                       need.value, _ptr(X), be._stream()), 'tnmf_hip_triggered_sums')

        t_kernel = timed(kernel, args.warmup, args.repeats)
        got = X.cpu().numpy()
        flops = 2. * N * P * F * float(np.prod(S)) * float(np.prod(win))
        tflops = flops / t_kernel / 1e9
        base = dict(tool='triggered_bench', config=name, dtype='float32', N=N, planes=P, fields=F, padded_shape=list(S),
                    A=list(A), margin=list(m), window=list(win), fit_iterations=args.fit_iterations,
                    h_density=round(float((Hp > 0).float().mean().item()), 4), h_row_stride=int(stride),
                    work_bytes=int(need.value), device=torch.cuda.get_device_name(0))
        lines = [dict(base, route='triggered_sums', warmup=args.warmup, repeats=args.repeats, ms=round(t_kernel, 3),
                      algorithmic_flops=flops, tflops=round(tflops, 3), f64_matrix_peak_tflops=args.f64_matrix_peak_tflops,
                      share_of_f64_matrix_peak=round(tflops / args.f64_matrix_peak_tflops, 4))]
        Hd = Hc[..., :S[-1]]
        routes = ([] if args.no_loop else [('torch_loop', torch_loop)]) + ([('torch_conv2d', torch_conv2d)] if args.conv2d else [])
        for route, fn in routes:
            line = dict(base, route=route, repeats=args.loop_repeats)
            weights_gib = N * F * P * float(np.prod(S)) * 4 / 2 ** 30
            same = ('config', 'route', 'dtype', 'N', 'planes', 'fields', 'padded_shape', 'A', 'margin', 'window',
                    'fit_iterations', 'device')
            if route == 'torch_conv2d' and weights_gib > args.conv2d_max_gib:
                line.update(ms=None, note=f'not run: {weights_gib:.1f} GiB of filters')
            elif route == 'torch_loop' and args.loop_from is not None:
                found = [e for e in earlier if e.get('ms') is not None and all(e.get(k) == line[k] for k in same)]
                if found:
                    e = found[-1]
                    line.update(repeats=e['repeats'], ms=e['ms'], over_triggered_sums=round(e['ms'] / t_kernel, 3),
                                largest_difference_to_the_kernel_over_largest_entry=e.get(
                                    'largest_difference_to_the_kernel_over_largest_entry'),
                                note=f'not measured in this run: ms and the difference are those of {os.path.basename(args.loop_from)}, '
                                     'the ratio is to this run\'s kernel time')
                else:
                    line.update(ms=None, note=f'not run: no torch_loop line of this case in {os.path.basename(args.loop_from)}')
            else:
                try:
                    res = [None]

                    def run():
                        res[0] = fn(Hd, Y, A, m)

                    t = timed(run, 1, args.loop_repeats)
                    want = res[0].double().cpu().numpy()
                    line.update(ms=round(t, 3), over_triggered_sums=round(t / t_kernel, 3),
                                largest_difference_to_the_kernel_over_largest_entry=float(
                                    np.max(np.abs(got - want)) / np.max(np.abs(got))))
                except RuntimeError as exc:   # (a shape the library does not take)
                    line.update(ms=None, note=f'refused: {str(exc)[:200]}')
            lines.append(line)
        with open(args.out, 'a') as f:
            for line in lines:
                print(json.dumps(line))
                f.write(json.dumps(line) + '\n')
        del Hp, Hc, Hd, Y, work, X


if __name__ == '__main__':
    main()
