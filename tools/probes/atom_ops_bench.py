"""Iteration rate of a fit_batch with atom operators against a plain fit with the same number of effective atoms
(path='auto').

    python tools/probes/atom_ops_bench.py [--cases 3:rot8 2:rot8xscales2] [--steps 20] [--warmup 3] [--repeats 3]
                                          [--out FILE] [--operators-only]

A case is CONFIG:OPERATORS: a BASELINE config of bench.py (its geometry and planted synthetic samples) and an operator set
of T maps on its atoms -- rot8 = rotations(A, 8), rot8xscales2 = compose(rotations(A, 8), scales(A, [1, 0.8])).  For each
case: one plain model of M atoms and one operator model of M / T atoms, i.e. M effective ones (M = --effective, default
128), `warmup` full-batch iterations each, then `repeats` rounds that time `steps` iterations of each model in turn (host
clock around a synchronised loop of the front end's _iteration); the best round of each counts.  Prints one JSON line per
case with both rates and the cost of the operators; --out also writes them to FILE.  --operators-only runs the operator
models alone (for a kernel trace).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def make_ops(name, A):
    from tnmf_amd import transforms as tr
    if name == 'rot8':
        return tr.rotations(A, 8)
    if name == 'rot8xscales2':
        return tr.compose(tr.rotations(A, 8), tr.scales(A, [1., .8]))
    raise ValueError(f'unknown operator set {name!r}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=['3:rot8', '2:rot8xscales2'])
    ap.add_argument('--effective', type=int, default=128, help='effective atoms of both models')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--operators-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from bench import CONFIGS, synth_V_on_device
    from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    h_args = dict(sparsity=0., inhibition=0., cross_inhibition=0.)
    lines = []
    for case in args.cases:
        cfg_id, ops_name = case.split(':')
        cfg = CONFIGS[int(cfg_id)]
        ops = make_ops(ops_name, cfg['A'])
        assert args.effective % ops.T == 0
        V = synth_V_on_device(cfg, cfg['N'], seed=0, device=dev)
        legs = {}
        for name, n_atoms, transforms in (('plain', args.effective, None),
                                          ('operators', args.effective // ops.T, ops)):
            if name == 'plain' and args.operators_only:
                continue
            nmf = TransformInvariantNMF(n_atoms=n_atoms, atom_shape=cfg['A'], backend='hip', path='auto', init='device',
                                        transforms=transforms)
            nmf.fit_batch(V, n_iterations=args.warmup, progress_callback=lambda *_: True)
            legs[name] = [nmf, float('inf')]
        for _ in range(args.repeats):
            for leg in legs.values():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    leg[0]._iteration(h_args)
                torch.cuda.synchronize()
                leg[1] = min(leg[1], (time.perf_counter() - t0) / args.steps)
        line = dict(config=int(cfg_id), operators=ops_name, T=ops.T, nnz=ops.nnz, effective_atoms=args.effective,
                    path='auto', steps=args.steps, repeats=args.repeats)
        for name, (nmf, sec) in legs.items():
            line[f'{name}_ms_per_it'] = round(1e3 * sec, 4)
            line[f'{name}_energy'] = nmf._energy_function()
        if len(legs) == 2:
            line['cost_of_operators'] = round(legs['operators'][1] / legs['plain'][1], 4)
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
