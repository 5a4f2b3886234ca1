#!/usr/bin/env python
"""
Times the fused source separation (HIP_Backend.source_parts, output 'masked' -> tnmf_hip_atom_sources) beside the only
route there was before it, all on the device: reconstruct(W[planes], H[:, planes]) per source on the default path, one
reconstruct for R, and ``V * r / (R + eps)`` in torch.

  (a) BASELINE config 3 -- 256 x 1 x 256^2 samples, 32 planes of 12 x 12, float32 -- as 32, 4 and 2 sources of 32 atoms,
      and as 8 atoms in the four orientations of 'rot90', one source each;
  (b) a spectrogram-shaped problem on one shift axis: 8 samples of 4096 frames, 257 channels, 16 atoms of 8 taps, 2 sources.

HIP events on the launch stream around `--repeats` back-to-back calls after `--warmup` calls give one mean per call; every
case is measured `--rounds` times, both routes alternating, and reported as the median with the spread (largest minus
smallest) of the rounds.  Appends one JSON line per case to --out (default profiles/separate_bench.jsonl).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tnmf_amd.backends.HIP import HIP_Backend  # noqa: E402
from tnmf_amd.sources_host import source_tables  # noqa: E402

EPS = 1e-9


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


def measure(name, V, A, P, plane_sets, args):
    """One case: plane_sets are S runs of adjacent planes (the loop slices W and H, as R_partial does)."""
    N, C, D = V.shape[0], V.shape[1], V.shape[2:]
    be = HIP_Backend(init='device')
    W, H = be.initialize(V, A, P, None, tuple(range(-len(A), 0)))
    Vd = be._V_dev
    order, start = source_tables(plane_sets)
    S = len(plane_sets)
    kept = {}

    def fused():
        kept['fused'] = be.source_parts(V, W, H, order, start, 'masked', eps=EPS)

    def loop():
        den = be.reconstruct(W, H) + EPS
        out = torch.empty((N, S, C) + tuple(D), dtype=Vd.dtype, device=Vd.device)
        for g, planes in enumerate(plane_sets):
            a, b = planes[0], planes[-1] + 1
            out[:, g] = Vd * be.reconstruct(W[a:b], H[:, a:b]) / den
        kept['loop'] = out

    t_fused, t_loop = [], []
    for _ in range(args.rounds):
        t_fused.append(timed(fused, args.warmup, args.repeats))
        t_loop.append(timed(loop, args.warmup, args.repeats))
    loop_path = be.last_path
    got, want = kept['fused'], kept['loop']
    diff = float(torch.max(torch.abs(got - want)) / torch.max(torch.abs(want)))
    in_range = bool(torch.all(got >= 0) and torch.all(got <= Vd[:, None]))
    loop_in_range = bool(torch.all(want >= 0) and torch.all(want <= Vd[:, None]))
    fused_ms, loop_ms = statistics.median(t_fused), statistics.median(t_loop)
    spread = max(t_loop) - min(t_loop)
    taps = int(np.prod(A))
    line = dict(tool='separate_bench', case=name, dtype='float32', N=N, C=C, D=list(D), A=list(A), planes=P, sources=S,
                warmup=args.warmup, repeats=args.repeats, rounds=args.rounds,
                fused_ms=round(fused_ms, 4), fused_spread_ms=round(max(t_fused) - min(t_fused), 4),
                loop_ms=round(loop_ms, 4), loop_spread_ms=round(spread, 4), loop_path=loop_path,
                loop_over_fused=round(loop_ms / fused_ms, 3),
                fused_ahead_by_spreads=round((loop_ms - fused_ms) / spread, 1) if spread > 0 else None,
                multiply_add_flops=2. * N * C * int(np.prod(D)) * P * taps,
                output_bytes=4. * N * S * C * int(np.prod(D)),
                largest_difference_to_the_loop_over_largest_value=diff,
                fused_within_0_and_V=in_range, loop_within_0_and_V=loop_in_range,
                device=torch.cuda.get_device_name(0))
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--cases', default='config3-S32,config3-S4,config3-S2,config3-rot90-S8,spectrogram-S2')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'separate_bench.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'separate_bench.py measures on the GPU: there is no fallback'
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    blocks = lambda P, S: [list(range(g * (P // S), (g + 1) * (P // S))) for g in range(S)]   # noqa: E731
    cases = {}
    for S in (32, 4, 2):
        cases[f'config3-S{S}'] = ((256, 1, 256, 256), (12, 12), 32, blocks(32, S))
    cases['config3-rot90-S8'] = ((256, 1, 256, 256), (12, 12), 32, blocks(32, 8))   # (8 atoms x 4 orientations)
    cases['spectrogram-S2'] = ((8, 257, 4096), (8,), 16, blocks(16, 2))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.cases.split(','):
        shape_V, A, P, sets = cases[name]
        line = measure(name, rng.random(shape_V, dtype=np.float32), A, P, sets, args)
        with open(args.out, 'a') as f:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
