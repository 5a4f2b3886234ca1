"""What finding the events of a scene costs by forward selection, next to the route through a dense fit of H (float32,
path='auto'; not part of bench.py).

    python tools/probes/pursuit_bench.py [--config 3] [--events 50] [--min-gain 1e-3] [--dense-iterations 300]
                                         [--threshold-frac 0.05] [--warmup 1] [--repeats 3] [--lib LIB.so] [--out FILE]

A scene is planted on the device: a random normalised dictionary of the BASELINE config's shape (bench.py's CONFIGS) and
`events` events per sample at random shifts with strengths 1 .. 2, rendered with the product's own kernel, plus noise of 1e-3.
JSON lines (printed; --out appends them to FILE):
    what='pursuit'        pursue_detections(min_gain) on a model that holds the dictionary: wall-clock median of `repeats` runs
                          after `warmup` (host work included: the rows are chosen there), rounds, rows, the objective of the
                          returned list, and the device time per round by kernel group (one more run under the backend's
                          timeline, with n_iterations=0: the rounds without the final refit): correlate, score, peaks, pick, render + refit
                          (event lists included)
    what='dense_route'    the route without it: fit_batch(update_W=False, keep_W=True, tol=1e-4), detections(threshold),
                          prune_detections(min_gain); wall-clock median of `repeats` runs after `warmup`, like the pursuit
                          (every run is a whole fit from a fresh initialisation), iterations, rows, the objective of its list
                          -- the two routes do NOT end at the same objective: both are reported
    what='pursuit_score'  tnmf_hip_pursuit_score alone on the map of the scene (device median): GB/s over the bytes it must move
                          (map read and written, table read once per sample), and that as a fraction of the best read-only
                          streaming rate recorded in profiles/r02_read_probe.txt (6.43 TB/s; the file holds no copy rate)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

READ_RATE_TBS = 6.43   # profiles/r02_read_probe.txt, the best line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=int, default=3)
    ap.add_argument('--events', type=int, default=50)
    ap.add_argument('--min-gain', type=float, default=1e-3)
    ap.add_argument('--dense-iterations', type=int, default=300)
    ap.add_argument('--threshold-frac', type=float, default=0.05)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--skip-dense', action='store_true')
    ap.add_argument('--lib', default=None, help='an A/B build of the library under tnmf_amd/lib (make VARIANT=...)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import ctypes

    import numpy as np
    import torch
    from bench import CONFIGS
    from tnmf_amd import _lib
    if args.lib:
        _lib.LIB_PATH = args.lib if os.path.isabs(args.lib) else os.path.join(ROOT, 'tnmf_amd', 'lib', args.lib)
    from tnmf_amd.backends.HIP import _ptr
    from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

    torch.cuda.set_device(0)
    cfg = CONFIGS[args.config]
    N, C, D, M, A = cfg['N'], cfg['C'], tuple(cfg['D']), cfg['M'], tuple(cfg['A'])
    rng = np.random.default_rng(0)
    W = rng.random((M, C) + A).astype(np.float32) ** 4 + 0.01
    W /= W.sum(axis=tuple(range(2, W.ndim)), keepdims=True)
    S = tuple(d + a - 1 for d, a in zip(D, A))
    K = N * args.events
    sample = np.repeat(np.arange(N), args.events)
    plane = rng.integers(M, size=K)
    shift = np.stack([rng.integers(a - 1, d, size=K) for a, d in zip(A, D)], axis=1)   # (wholly inside the sample)
    strength = (1. + rng.random(K)).astype(np.float32)

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(json.dumps(line) + '\n')

    def model(V):
        nmf = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip', path='auto', init='device')
        nmf._W = torch.from_numpy(W).cuda()
        nmf.fit_batch(V, n_iterations=0, keep_W=True)
        return nmf

    torch.cuda.manual_seed(1)
    nmf = model(np.zeros((N, C) + D, dtype=np.float32))
    be = nmf._backend
    V = be.render_events(nmf._W, sample, plane, shift, strength)
    V = (V + 1e-3 * torch.rand_like(V)).cpu().numpy()
    nmf = model(V)
    be = nmf._backend
    half_norm = 0.5 * float(np.sum(V.astype(np.float64) ** 2))
    common = dict(library=os.path.basename(_lib.LIB_PATH), config=args.config, dtype='float32', path='auto', planted=K,
                  events_per_sample=args.events, min_gain=args.min_gain, half_norm_V=round(half_norm, 3))

    def objective_of(det):
        R = nmf.reconstruct_detections(det).astype(np.float64)
        return 0.5 * float(np.sum((V - R) ** 2))

    # -- forward selection
    walls = []
    for i in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        det, gains = nmf.pursue_detections(args.min_gain)
        torch.cuda.synchronize()
        if i >= args.warmup:
            walls.append(time.perf_counter() - t0)
    hist = nmf.pursuit_history_
    be.start_timeline()
    nmf.pursue_detections(args.min_gain, n_iterations=0)     # (the rounds alone: without the final refit's renders and updates)
    spans = be.stop_timeline()
    rounds = max(len(hist), 1)
    group = {'correlate': ('pursuit_correlate',), 'score': ('pursuit_score',), 'peaks': ('find_peaks',),
             'pick': ('pursuit_pick',), 'render_refit': ('events_render', 'events_update', 'event_list'),
             'final_gains': ('events_gain',), 'norms': ('events_norms',)}
    per_round = {k: round(sum(sum(spans.get(n, [])) for n in names) / rounds, 4) for k, names in group.items()}
    planted_rows = set(map(tuple, np.column_stack([sample, plane, shift]).tolist()))
    found = set(map(tuple, np.column_stack([det.sample, det.atom, det.shift]).tolist()))
    emit(dict(what='pursuit', wall_ms=round(1e3 * statistics.median(walls), 2),
              wall_ms_runs=[round(1e3 * w, 2) for w in walls], rounds=len(hist), rows=len(det),
              planted_found=len(planted_rows & found), added_per_round=hist[:, 1].astype(int).tolist(),
              objective=round(objective_of(det), 5), device_ms_per_round=per_round, family=be.last_path,
              repeats=args.repeats, **common))

    # -- the score kernel alone
    P = int(nmf._W.shape[0])
    a = torch.randn((be.n_local_samples, P) + S, dtype=torch.float32, device='cuda')
    b = be.event_norms(nmf._W)
    out = torch.empty_like(a)
    g = _lib.make_geom(int(a.shape[0]), P, C, S, (1,) * len(S), 0, 0)
    times = []
    for i in range(3 + 9):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(be._lib.tnmf_hip_pursuit_score(be._ctx, ctypes.byref(g), _ptr(a), _ptr(b), _ptr(out), None, 0,
                                                  be._stream()), 'tnmf_hip_pursuit_score')
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            times.append(e0.elapsed_time(e1))
    ms = statistics.median(times)
    moved = 2 * a.numel() * 4 + a.shape[0] * b.numel() * 8
    emit(dict(what='pursuit_score', map_shape=list(a.shape), ms=round(ms, 4), GBps=round(moved / ms / 1e6, 1),
              fraction_of_read_rate=round(moved / ms / 1e9 / READ_RATE_TBS, 3), read_rate_TBps=READ_RATE_TBS, **common))
    del a, out

    # -- the route through a dense fit
    if not args.skip_dense:
        legs = []
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nmf.fit_batch(V, n_iterations=args.dense_iterations, update_W=False, keep_W=True, tol=1e-4,
                          progress_callback=lambda *_: True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            h_max = float(nmf._H.max().item())
            dense = nmf.detections(threshold=args.threshold_frac * h_max)
            t2 = time.perf_counter()
            pruned, _ = nmf.prune_detections(dense, args.min_gain)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if i >= args.warmup:
                legs.append((t3 - t0, t1 - t0, t2 - t1, t3 - t2))
        wall, fit, peaks, prune = (1e3 * np.array(legs)).T
        found = set(map(tuple, np.column_stack([pruned.sample, pruned.atom, pruned.shift]).tolist()))
        emit(dict(what='dense_route', wall_ms=round(float(np.median(wall)), 2), wall_ms_runs=np.round(wall, 2).tolist(),
                  fit_ms=round(float(np.median(fit)), 2), detections_ms=round(float(np.median(peaks)), 2),
                  prune_ms=round(float(np.median(prune)), 2), iterations=int(nmf.n_iter_), converged=bool(nmf.converged_),
                  threshold_frac_of_max=args.threshold_frac, detections=len(dense), rows=len(pruned),
                  planted_found=len(planted_rows & found), objective=round(objective_of(pruned), 5), repeats=args.repeats,
                  **common))

if __name__ == '__main__':
    main()
