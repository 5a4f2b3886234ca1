"""What the exact strengths of a list cost, next to the multiplicative refit (float32, path='auto'; not part of bench.py).

    python tools/probes/solve_bench.py [--config 3] [--events 50] [--decoys] [--tol 1e-8] [--warmup 1] [--repeats 3]
                                       [--mu-cap 5000] [--out FILE]

The scene is tools/probes/pursuit_bench.py's: a random normalised dictionary of the BASELINE config's shape (bench.py's
CONFIGS) and `events` events per sample at random shifts with strengths 1 .. 2, rendered with the product's own kernel, plus
noise of 1e-3.  The list is the planted rows; with --decoys also their four one-pixel neighbours and the same place under the
next atom (strongly coupled rows: the Gram matrix is far from diagonal).  Every strength starts at 1.  A call is one
process: run it under a time limit of its own (`timeout -k 10 300 python tools/probes/solve_bench.py ...`).  The objective of a list
is taken from its quadratic form on the device, E(h) = 1/2 |V|^2 - c'h + 1/2 h'Gh in float64, for both methods.
JSON lines (printed; --out appends them to FILE):
    what='solve'   solve_events(tol): wall-clock median of `repeats` runs after `warmup`; from one more run under the backend's
                   timeline the device time of the event lists, of the three kernels alone (pairs, Gram, projection), of the
                   torch work between them (unique, sort, CSR), and of the whole solver call (its three set-up kernels, one
                   launch pair per iteration plus the one whose step is discarded, and the host's reads); the cost of one
                   more iteration, from solver calls that cannot converge (tol 1e-300) at 10 and 210 iterations: the
                   difference of their medians / 200; nnz, iterations, kkt and the objective reached
    what='refit'   refit_events at 50 steps: wall-clock median, the objective reached, and the number of steps (in chunks of
                   `--mu-chunk`, capped at `--mu-cap`) after which its objective is within 1e-6 relative of the solved one
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=int, default=3)
    ap.add_argument('--events', type=int, default=50)
    ap.add_argument('--decoys', action='store_true')
    ap.add_argument('--tol', type=float, default=1e-8)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--mu-cap', type=int, default=5000)
    ap.add_argument('--mu-chunk', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from bench import CONFIGS
    from tnmf_amd import _lib
    from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

    torch.cuda.set_device(0)
    cfg = CONFIGS[args.config]
    N, C, D, M, A = cfg['N'], cfg['C'], tuple(cfg['D']), cfg['M'], tuple(cfg['A'])
    k = len(A)
    rng = np.random.default_rng(0)
    W = rng.random((M, C) + A).astype(np.float32) ** 4 + 0.01
    W /= W.sum(axis=tuple(range(2, W.ndim)), keepdims=True)
    S = tuple(d + a - 1 for d, a in zip(D, A))
    K0 = N * args.events
    sample = np.repeat(np.arange(N), args.events)
    plane = rng.integers(M, size=K0)
    shift = np.stack([rng.integers(a - 1, d, size=K0) for a, d in zip(A, D)], axis=1)   # (wholly inside the sample)
    strength = (1. + rng.random(K0)).astype(np.float32)

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
    V = nmf._backend.render_events(nmf._W, sample, plane, shift, strength)
    V = (V + 1e-3 * torch.rand_like(V)).cpu().numpy()
    nmf = model(V)
    be, Wd = nmf._backend, nmf._W
    half_norm = 0.5 * float(np.sum(V.astype(np.float64) ** 2))

    rows = np.column_stack([sample, plane, shift])
    if args.decoys:
        more = [rows]
        for axis in range(k):
            for step in (-1, 1):
                r = rows.copy()
                r[:, 2 + axis] += step
                more.append(r)
        r = rows.copy()
        r[:, 1] = (r[:, 1] + 1) % M
        more.append(r)
        rows = np.concatenate(more)
        inside = np.all((rows[:, 2:] >= 0) & (rows[:, 2:] < np.array(S)), axis=1)
        rows = rows[inside]
        _, first = np.unique(rows, axis=0, return_index=True)
        rows = rows[np.sort(first)]
    K = len(rows)
    s_, p_, u_ = rows[:, 0], rows[:, 1], rows[:, 2:]
    start = np.ones(K, dtype=np.float32)
    common = dict(library=os.path.basename(_lib.LIB_PATH), config=args.config, dtype='float32', planted=K0, rows=K,
                  decoys=bool(args.decoys), events_per_sample=args.events, half_norm_V=round(half_norm, 3))

    # the quadratic form of the list, once, for the objectives of both methods
    sd, pd, ud, _ = be._check_events(int(Wd.shape[0]), s_, p_, u_, start)
    images, cell_start, events = be.event_list(sd, pd, ud)
    row_start, col, val = be.gram_event_list(Wd, images, cell_start, events)
    c = be.project_event_list(Wd, events)
    row = torch.repeat_interleave(torch.arange(K, device=c.device), (row_start[1:] - row_start[:-1]).long())

    def objective(h):
        h = torch.as_tensor(h).to(c.device, torch.float64)
        Gh = torch.zeros(K, dtype=torch.float64, device=c.device).index_add_(0, row, val * h[col.long()])
        return half_norm - float(c @ h) + 0.5 * float(h @ Gh)

    # -- the solver
    walls = []
    for i in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h, info = be.solve_events(None, Wd, s_, p_, u_, start, args.tol, 10000)
        torch.cuda.synchronize()
        if i >= args.warmup:
            walls.append(time.perf_counter() - t0)
    be.start_timeline()
    h, info = be.solve_events(None, Wd, s_, p_, u_, start, args.tol, 10000)
    spans = be.stop_timeline()
    total = {name: sum(spans.get(name, [])) for name in ('event_list', 'events_pairs', 'events_gram', 'events_project',
                                                         'events_gram_lists', 'events_nnls')}
    start64 = torch.ones(K, dtype=torch.float64, device=c.device)
    fixed = {}
    for n in (10, 210):
        times = []
        for _ in range(1 + args.repeats):
            be.start_timeline()
            be.nnls_event_list((row_start, col, val), c, start64, 1e-300, n)
            times.append(sum(be.stop_timeline()['events_nnls']))
        fixed[n] = statistics.median(times[1:])
    E_solve = objective(h)
    emit(dict(what='solve', tol=args.tol, wall_ms=round(1e3 * statistics.median(walls), 2),
              wall_ms_runs=[round(1e3 * w, 2) for w in walls], nnz=info['nnz'], iterations=info['iterations'],
              kkt=info['kkt'], converged=info['converged'], zeros=int((h == 0).sum().item()),
              event_list_ms=round(total['event_list'], 3),
              pairs_kernel_ms=round(total['events_pairs'], 3), gram_kernel_ms=round(total['events_gram'], 3),
              project_kernel_ms=round(total['events_project'], 3), gram_lists_ms=round(total['events_gram_lists'], 3),
              nnls_ms=round(total['events_nnls'], 3), nnls_ms_10_iterations=round(fixed[10], 4),
              nnls_ms_210_iterations=round(fixed[210], 4), ms_per_more_iteration=round((fixed[210] - fixed[10]) / 200, 5),
              objective=E_solve, objective_rounded_f32=objective(h.to(torch.float32)), repeats=args.repeats, **common))

    # -- the multiplicative refit
    walls = []
    for i in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h50 = be.refit_events(None, Wd, s_, p_, u_, start, 50, 0., nmf.eps)
        torch.cuda.synchronize()
        if i >= args.warmup:
            walls.append(time.perf_counter() - t0)
    E50 = objective(h50)
    target = E_solve * (1. + 1e-6)
    steps, hmu, E = 0, torch.from_numpy(start).cuda(), objective(start)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while E > target and steps < args.mu_cap:
        hmu = be.refit_events(None, Wd, s_, p_, u_, hmu, args.mu_chunk, 0., nmf.eps)
        steps += args.mu_chunk
        E = objective(hmu)
    torch.cuda.synchronize()
    emit(dict(what='refit', wall_ms_50_steps=round(1e3 * statistics.median(walls), 2),
              wall_ms_runs=[round(1e3 * w, 2) for w in walls], objective_50_steps=E50,
              steps_to_1e6th_of_solved=steps if E <= target else None, mu_cap=args.mu_cap, mu_chunk=args.mu_chunk,
              objective_at_stop=E, wall_ms_to_stop=round(1e3 * (time.perf_counter() - t0), 2),
              solved_objective=E_solve, repeats=args.repeats, **common))


if __name__ == '__main__':
    main()
