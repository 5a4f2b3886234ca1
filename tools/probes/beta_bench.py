"""Iteration rate of fit_batch under the beta-divergence objectives against the Frobenius one (path='auto').

    python tools/probes/beta_bench.py [--configs 2 3] [--steps 20] [--warmup 3] [--out FILE]

For each BASELINE config (bench.py's CONFIGS, planted synthetic samples of bench.py) and beta in {2, 1, 0}: one model,
`warmup` full-batch iterations, then `steps` timed iterations (host clock around a synchronised loop of the front end's
_iteration).  Prints one JSON line per (config, beta) with it/s and the ratio to beta = 2; --out also writes them to FILE.
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
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from bench import CONFIGS, synth_V_on_device
    from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    lines = []
    for cfg_id in args.configs:
        cfg = CONFIGS[cfg_id]
        # (the planted model's noise may hit an exact zero; Itakura-Saito needs V > 0)
        V = np.maximum(synth_V_on_device(cfg, cfg['N'], seed=0, device=dev), np.float32(1e-6))
        base = None
        for beta in (2., 1., 0.):
            nmf = TransformInvariantNMF(n_atoms=cfg['M'], atom_shape=cfg['A'], backend='hip', beta_loss=beta,
                                        path='auto', init='device')
            nmf.fit_batch(V, n_iterations=args.warmup, progress_callback=lambda *_: True)
            h_args = dict(sparsity=0., inhibition=0., cross_inhibition=0.)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                nmf._iteration(h_args)
            torch.cuda.synchronize()
            its = args.steps / (time.perf_counter() - t0)
            base = its if beta == 2. else base
            line = dict(config=cfg_id, beta=beta, path='auto', steps=args.steps, it_per_s=round(its, 2),
                        ms_per_it=round(1e3 / its, 3), cost_vs_frobenius=round(base / its, 3),
                        energy=nmf._energy_function())
            print(json.dumps(line), flush=True)
            lines.append(line)
            del nmf
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
