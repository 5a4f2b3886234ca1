#!/usr/bin/env python
"""
Times tnmf_hip_events_patches ('cleaned', R given) and tnmf_hip_patch_moments on its output at BASELINE config 3 -- 256 x 1 x
256^2 samples, 32 planes of 12 x 12, float32 -- on a planted list of 12 800 distinct rows ('valid' mode, every occurrence one
image wholly inside its sample), as 32 atoms and as 8 atoms in the four orientations of 'rot90' (the fold table then in use),
beside two yardsticks on the same operands in the same process:

  events_gain     tnmf_hip_events_gain: it reads the same pixels; the patches kernel also stores K * D doubles
  torch_route     what a caller could do for such rows without the entry points: an advanced-index gather of V and R under
                  every row into [K, D] float64 (+ h * W_eff[p], and with 'rot90' the inverse permutation), then one
                  torch.einsum per atom for S and one matrix-vector product for g

HIP events on the launch stream around `--calls` back-to-back calls after `--warmup` calls, `--repeats` times: min / mean / max
of the per-call milliseconds.  Appends one JSON line per configuration to --out (default profiles/patches_bench.jsonl).
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

from tnmf_amd import _lib, transforms as tr  # noqa: E402
from tnmf_amd.backends.HIP import HIP_Backend, _ptr  # noqa: E402


def timed(fn, warmup, calls, repeats):
    """(min, mean, max) milliseconds per call of fn(): `repeats` times `calls` back-to-back calls between two events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return [round(x, 4) for x in (min(out), sum(out) / len(out), max(out))]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--samples', type=int, default=256)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--planes', type=int, default=32)
    ap.add_argument('--atom', type=int, default=12)
    ap.add_argument('--rows', type=int, default=12800)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'patches_bench.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'patches_bench.py measures on the GPU: there is no fallback'
    torch.cuda.set_device(0)
    N, C, D, A, P, K = args.samples, 1, (args.size, args.size), (args.atom, args.atom), args.planes, args.rows
    nA = A[0] * A[1]
    rng = np.random.default_rng(0)
    V = rng.random((N, C) + D, dtype=np.float32)
    be = HIP_Backend(path='generic', init='device')
    W = be.initialize(V, A, P, None, (-2, -1))[0]      # (the dense activations are not an operand here)
    torch.cuda.empty_cache()
    lib, ctx = be._lib, be._ctx
    # distinct rows, every occurrence one image wholly inside its sample: shift = origin + A - 1 in 'valid' mode
    flat = rng.choice(N * P * (D[0] - A[0] + 1) * (D[1] - A[1] + 1), K, replace=False)
    n, p, oy, ox = np.unravel_index(flat, (N, P, D[0] - A[0] + 1, D[1] - A[1] + 1))
    shift = np.stack([oy + A[0] - 1, ox + A[1] - 1], axis=1)
    h = (rng.random(K) + 0.5).astype(np.float32)
    _, _, events, strength, R = be._prepared_events('patches_bench', P, n, p, shift, h, render=W)
    Vd = be._V_dev
    geom = be._geom(N, P)
    lines = []
    for name, transforms in (('config3', None), ('config3-rot90', 'rot90')):
        table = be._fold_table(transforms)
        T = table[3]
        M, Dp = P // T, C * nA
        out = torch.empty((K, C) + A, dtype=torch.float64, device=be.device)
        atom = torch.div(events[:, 1].to(torch.int64), T, rounding_mode='floor')
        sorted_atom, order = torch.sort(atom, stable=True)
        start = torch.searchsorted(sorted_atom, torch.arange(M + 1, device=be.device)).to(torch.int32)
        by_atom = order.to(torch.int32).contiguous()
        strength_d = strength.to(torch.float64)
        mom = (torch.empty((M, Dp, Dp), dtype=torch.float64, device=be.device),
               torch.empty((M, Dp), dtype=torch.float64, device=be.device),
               torch.empty(M, dtype=torch.float64, device=be.device), torch.empty(M, dtype=torch.float64, device=be.device))
        gain = torch.empty(K, dtype=torch.float64, device=be.device)

        def patches():
            be.patch_event_list(W, events, strength, R, 'cleaned', table, out=out)

        def moments():
            be.moments_patch_list(out.reshape(K, Dp), strength_d, by_atom, start, K, False, mom)

        def gains():
            _lib.check(lib.tnmf_hip_events_gain(ctx, ctypes.byref(geom), be._mode, _ptr(W), _ptr(events), _ptr(strength), K,
                                                _ptr(Vd), _ptr(R), _ptr(gain), None, be._stream()), 'tnmf_hip_events_gain')

        # the torch route: flat pixel indices [K, D] under every row, the inverse permutation of the row's orientation
        jy, jx = torch.meshgrid(torch.arange(A[0], device=be.device), torch.arange(A[1], device=be.device), indexing='ij')
        ev = events.to(torch.int64)
        base = (ev[:, 0] * C * D[0] + (ev[:, 2] - (A[0] - 1))) * D[1] + (ev[:, 3] - (A[1] - 1))
        pix = base[:, None] + (jy.reshape(-1) * D[1] + jx.reshape(-1))[None, :]
        perm = None
        if transforms is not None:
            ptr, src = table[0].cpu().numpy(), table[1].cpu().numpy()
            assert np.all(np.diff(ptr) == 1), 'a permutation: one entry per pixel'
            perm = torch.from_numpy(src.reshape(T, nA).astype(np.int64)).to(be.device)[ev[:, 1] % T]
        Wf = W.reshape(P, Dp).to(torch.float64)
        t_S = torch.empty((M, Dp, Dp), dtype=torch.float64, device=be.device)
        t_g = torch.empty((M, Dp), dtype=torch.float64, device=be.device)
        bounds = start.cpu().tolist()

        def torch_route():
            Y = Vd.reshape(-1)[pix].to(torch.float64) - R.reshape(-1)[pix].to(torch.float64)
            Y = Y + strength_d[:, None] * Wf[ev[:, 1]]
            if perm is not None:
                Y = torch.gather(Y, 1, perm)
            Ys, hs = Y[order], strength_d[order]
            for m in range(M):
                a, b = bounds[m], bounds[m + 1]
                t_S[m] = torch.einsum('ki,kj->ij', Ys[a:b], Ys[a:b])
                t_g[m] = hs[a:b] @ Ys[a:b]
            return Y

        t_patches = timed(patches, args.warmup, args.calls, args.repeats)
        t_moments = timed(moments, args.warmup, args.calls, args.repeats)
        both = timed(lambda: (patches(), moments()), args.warmup, args.calls, args.repeats)
        t_gain = timed(gains, args.warmup, args.calls, args.repeats)
        t_torch = timed(torch_route, args.warmup, max(2, args.calls // 3), args.repeats)
        Y = torch_route()
        diff_Y = float((Y - out.reshape(K, Dp)).abs().max() / Y.abs().max())
        diff_S = float((t_S - mom[0]).abs().max() / t_S.abs().max())
        diff_g = float((t_g - mom[1]).abs().max() / t_g.abs().max())
        spread = t_torch[2] - t_torch[0]
        line = dict(tool='patches_bench', config=name, dtype='float32', N=N, C=C, D=list(D), A=list(A), planes=P, T=T, atoms=M,
                    rows=K, patch_doubles=Dp, warmup=args.warmup, calls=args.calls, repeats=args.repeats,
                    patches_ms_min_mean_max=t_patches, moments_ms_min_mean_max=t_moments, both_ms_min_mean_max=both,
                    events_gain_ms_min_mean_max=t_gain, torch_route_ms_min_mean_max=t_torch,
                    patch_store_mbytes=round(8. * K * Dp / 1e6, 2), patches_over_gain=round(t_patches[1] / t_gain[1], 3),
                    torch_route_over_both=round(t_torch[0] / both[1], 3),
                    bar_both_below_torch_min_by_more_than_its_spread=bool(both[1] < t_torch[0] - spread),
                    largest_relative_difference_of_the_patches=diff_Y, of_S=diff_S, of_g=diff_g,
                    device=torch.cuda.get_device_name(0))
        print(json.dumps(line))
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
