"""Iteration rate of fit_batch with elementwise weights against the same objective without them (path='auto').

    python tools/probes/weights_bench.py [--configs 2 3] [--betas 2 1] [--steps 30] [--warmup 3] [--repeats 3]
                                         [--out FILE] [--weighted-only]

For each BASELINE config (bench.py's CONFIGS, planted synthetic samples of bench.py) and beta: one unweighted and one
weighted model (a 0/1 mask with 10 % zeros, drawn once per config), `warmup` full-batch iterations each, then `repeats`
rounds that time `steps` iterations of each model in turn (host clock around a synchronised loop of the front end's
_iteration); the best round of each counts.  Prints one JSON line per (config, beta) with both rates and the cost of the
weights; --out also writes them to FILE.  --weighted-only runs the weighted models alone (for a kernel trace).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', type=int, nargs='+', default=[2, 3])
    ap.add_argument('--betas', type=float, nargs='+', default=[2., 1.])
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--zeros', type=float, default=0.1, help='fraction of zero weights in the mask')
    ap.add_argument('--weighted-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from bench import CONFIGS, synth_V_on_device
    from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    h_args = dict(sparsity=0., inhibition=0., cross_inhibition=0.)
    lines = []
    for cfg_id in args.configs:
        cfg = CONFIGS[cfg_id]
        V = synth_V_on_device(cfg, cfg['N'], seed=0, device=dev)
        mask = (np.random.default_rng(1).random(V.shape) >= args.zeros).astype(V.dtype)
        for beta in args.betas:
            legs = {}
            for name, weights in (('unweighted', None), ('weighted', mask)):
                if name == 'unweighted' and args.weighted_only:
                    continue
                nmf = TransformInvariantNMF(n_atoms=cfg['M'], atom_shape=cfg['A'], backend='hip', beta_loss=beta,
                                            path='auto', init='device')
                nmf.fit_batch(V, n_iterations=args.warmup, progress_callback=lambda *_: True, weights=weights)
                legs[name] = [nmf, float('inf')]
            for _ in range(args.repeats):
                for leg in legs.values():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        leg[0]._iteration(h_args)
                    torch.cuda.synchronize()
                    leg[1] = min(leg[1], (time.perf_counter() - t0) / args.steps)
            line = dict(config=cfg_id, beta=beta, path='auto', zeros=args.zeros, steps=args.steps,
                        repeats=args.repeats)
            for name, (nmf, sec) in legs.items():
                line[f'{name}_ms_per_it'] = round(1e3 * sec, 4)
                line[f'{name}_energy'] = nmf._energy_function()
            if len(legs) == 2:
                line['cost_of_weights'] = round(legs['weighted'][1] / legs['unweighted'][1], 4)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del legs
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
