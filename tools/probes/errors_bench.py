"""What the diagonal of the inverse Gram matrix of a list costs, next to the Gram matrix itself (float32, path='auto'; not part
of bench.py).

    python tools/probes/errors_bench.py [--config 3] [--events 50] [--warmup 1] [--repeats 5] [--out profiles/errors_bench.jsonl]

Three lists, every row active:
    what='planted'  the planted list of tools/probes/solve_bench.py: a random normalised dictionary of the BASELINE config's
                    shape (bench.py's CONFIGS) and `events` events per sample at random shifts -- 12 800 rows at the defaults,
                    two thirds of them components of one row, the others in components of a few rows
    what='isolated' as many rows on a grid two atom extents apart: every component is one row, the elementwise path alone
    what='chain'    one sample of 1 x 3000 with atoms of 7 taps and TNMF_EVENTS_INVERSE_LDS + 1 rows three cells apart: ONE
                    component just above the LDS path, factored on a tile of the scratch by one workgroup
Per list, from `repeats` runs under the backend's timeline after `warmup`: the medians of the device times of 'events_gram'
(the kernel alone), 'events_components' (the torch work that labels the components and builds their lists) and
'events_inverse_diag' (every launch of tnmf_hip_events_inverse_diag), the component sizes, and the wall-clock median of
event_errors as a whole.  A call is one process: run it under a time limit of its own
(`timeout -k 10 300 python tools/probes/errors_bench.py ...`).  JSON lines (printed; --out appends them to FILE).
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
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from bench import CONFIGS
    from tnmf_amd import _lib
    from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(json.dumps(line) + '\n')

    def run(what, N, C, D, M, A, sample, plane, shift, **more):
        W = rng.random((M, C) + A).astype(np.float32) ** 4 + 0.01
        W /= W.sum(axis=tuple(range(2, W.ndim)), keepdims=True)
        nmf = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip', path='auto', init='device')
        nmf._W = torch.from_numpy(W).cuda()
        nmf.fit_batch(np.zeros((N, C) + D, dtype=np.float32), n_iterations=0, keep_W=True)
        be, Wd = nmf._backend, nmf._W
        strength = (1. + rng.random(len(sample))).astype(np.float32)
        V = be.render_events(Wd, sample, plane, shift, strength)
        be._V_dev.copy_(V + 1e-3 * torch.rand_like(V))
        spans, walls, info = [], [], None
        for i in range(args.warmup + args.repeats):
            be.start_timeline()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, _, info = be.event_errors(None, Wd, sample, plane, shift, strength)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            timeline = be.stop_timeline()
            if i >= args.warmup:
                walls.append(wall)
                spans.append({name: sum(timeline.get(name, [])) for name in ('events_gram', 'events_components',
                                                                             'events_inverse_diag')})
        median = {name: round(statistics.median(s[name] for s in spans), 4) for name in spans[0]}
        sizes = info['sizes']
        emit(dict(what=what, library=os.path.basename(_lib.LIB_PATH), dtype='float32', rows=len(sample),
                  n_components=int(info['n_components']), components_of_one_row=int((sizes == 1).sum()),
                  largest_component=int(info['largest_component']), n_singular=int(info['n_singular']),
                  rounds=int(info['rounds']), gram_kernel_ms=median['events_gram'],
                  components_ms=median['events_components'], inverse_diag_ms=median['events_inverse_diag'],
                  inverse_diag_below_gram=bool(median['events_inverse_diag'] < median['events_gram']),
                  event_errors_wall_ms=round(1e3 * statistics.median(walls), 2), repeats=args.repeats, **more))

    cfg = CONFIGS[args.config]
    N, C, D, M, A = cfg['N'], cfg['C'], tuple(cfg['D']), cfg['M'], tuple(cfg['A'])
    K = N * args.events
    run('planted', N, C, D, M, A, np.repeat(np.arange(N), args.events), rng.integers(M, size=K),
        np.stack([rng.integers(a - 1, d, size=K) for a, d in zip(A, D)], axis=1), config=args.config,
        events_per_sample=args.events)
    # the same number of rows on a grid two atom extents apart: no two footprints meet
    grid = np.stack(np.meshgrid(*[np.arange(a - 1, d - 2 * a, 2 * a) for a, d in zip(A, D)], indexing='ij'), -1).reshape(-1, len(A))
    assert len(grid) >= args.events
    run('isolated', N, C, D, M, A, np.repeat(np.arange(N), args.events), rng.integers(M, size=K),
        np.concatenate([grid[rng.permutation(len(grid))[:args.events]] for _ in range(N)]), config=args.config,
        events_per_sample=args.events)
    n = _lib.EVENT_INVERSE_LDS + 1
    run('chain', 1, 1, (3000,), 2, (7,), np.zeros(n, dtype=np.int64), rng.integers(2, size=n),
        (6 + 3 * np.arange(n)).reshape(n, 1))


if __name__ == '__main__':
    main()
