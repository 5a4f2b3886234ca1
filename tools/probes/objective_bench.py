"""What watching the objective costs per full-batch iteration (float32, path='auto').

    python tools/probes/objective_bench.py [--configs 2 3] [--steps 30] [--warmup 3] [--repeats 3] [--out FILE]

For each BASELINE config (bench.py's CONFIGS, planted synthetic samples of bench.py) four models step the front end's
_iteration the way fit_batch does:
    plain       no objective (a no-op progress callback)
    every_1     objective_every=1: the tap in the H half step, read after every iteration
    every_10    objective_every=10
    callback    the route before the tap: a progress callback that calls _energy_function() after every iteration
`warmup` iterations each, then `repeats` rounds that time `steps` iterations of each model in turn (host clock around a
synchronised loop); the best round of each counts.  Prints one JSON line per config with the four ms/iteration and
tap_over_callback = (every_1 - plain) / (callback - plain); --out also writes the lines to FILE.
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
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from bench import CONFIGS, synth_V_on_device
    from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    h_args = dict(sparsity=0., inhibition=0., cross_inhibition=0.)

    def step_plain(nmf, i):
        nmf._iteration(h_args)

    def step_every(k):
        def step(nmf, i):
            value = nmf._iteration(h_args, record=i % k == 0)
            assert (value is not None) == (i % k == 0)
        return step

    def step_callback(nmf, i):
        nmf._iteration(h_args)
        nmf._energy_function()

    lines = []
    for cfg_id in args.configs:
        cfg = CONFIGS[cfg_id]
        V = synth_V_on_device(cfg, cfg['N'], seed=0, device=dev)
        legs = {}
        for name, step in (('plain', step_plain), ('every_1', step_every(1)), ('every_10', step_every(10)),
                           ('callback', step_callback)):
            nmf = TransformInvariantNMF(n_atoms=cfg['M'], atom_shape=cfg['A'], backend='hip', path='auto', init='device')
            nmf.fit_batch(V, n_iterations=args.warmup, progress_callback=lambda *_: True,
                          **({'objective_every': 1} if name.startswith('every') else {}))
            nmf._begin_history()
            legs[name] = [nmf, step, float('inf')]
        for _ in range(args.repeats):
            for leg in legs.values():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.steps):
                    leg[1](leg[0], i)
                torch.cuda.synchronize()
                leg[2] = min(leg[2], (time.perf_counter() - t0) / args.steps)
        line = dict(config=cfg_id, dtype='float32', path='auto', steps=args.steps, repeats=args.repeats,
                    family=legs['plain'][0]._backend.last_path)
        for name, (_, _, sec) in legs.items():
            line[f'{name}_ms_per_it'] = round(1e3 * sec, 4)
        a, b, d = (legs[k][2] for k in ('plain', 'every_1', 'callback'))
        line['tap_over_callback'] = round((b - a) / (d - a), 4)
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
