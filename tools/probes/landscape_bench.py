"""What the landscape of a list costs next to its gains, and what moving a displaced list back costs (float32, path='auto';
not part of bench.py).

    python tools/probes/landscape_bench.py [--config 3] [--events 50] [--calls 200] [--rounds 7] [--warmup 1] [--repeats 3]
                                           [--ab-lib LIB.so] [--parent-tree DIR] [--step-timeout 240] [--out FILE]

Without --step this process only drives: it never opens the GPU.  Every GPU step is a child process of its own under
`timeout -k 10 <--step-timeout>`, one after the other, and the first child that fails, faults or runs out of time ends the
probe -- nothing more is started on the GPU after it.  The steps, in order:
    --step kernels                     on the product library
    --step relocate                    on the product library
    --step kernels --lib <--ab-lib>    with --ab-lib: an A/B build under tnmf_amd/lib (make VARIANT=lswalk
                                       VFLAGS=-DTNMF_LANDSCAPE_WALK_ONLY: the landscape without its staged path), then the
                                       product's kernels step and the A/B build's once more, so that the two alternate
    bench.py --gpus 1 --steps 30 --warmup 5    with --parent-tree: in this tree, then in DIR (a built checkout of the parent
                                       commit), twice, alternating; what='bench_headline' lines with tree='this' / 'parent'

The scene is that of tools/probes/pursuit_bench.py: a random normalised dictionary of the BASELINE config's shape (bench.py's
CONFIGS) and `events` events per sample at random shifts wholly inside the sample, strengths 1 .. 2, rendered with the
product's own kernel, plus noise of 1e-3.  JSON lines (printed; --out appends them to FILE):
    what='landscape_vs_gain'  tnmf_hip_events_landscape (a, b and mag written) against tnmf_hip_events_gain (gain and mag) on
                              the planted list against the same render, in the same process: `rounds` rounds that alternate
                              the two, each timing `calls` back-to-back launches between two device events; the medians per
                              call, their ratio, the quartiles of the per-round ratios, and which path the rows take (the
                              host mirror of the rule in landscape.hip).  Nine plain walks would cost about 9 x the gain.
    what='relocate'           relocate_detections on the planted list with every row displaced by one pixel (each by its own
                              nonzero offset): wall-clock median of `repeats` runs after `warmup` (host work included: the
                              hops are chosen there), rounds, hops per round, rows back at their planted place, objective.
    what='bench_headline'     ms per step and iterations per second of one bench.py run, and the tree it ran in.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=int, default=3)
    ap.add_argument('--events', type=int, default=50)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--step', choices=['kernels', 'relocate'], default=None, help='run this one step here (a child)')
    ap.add_argument('--lib', default=None, help='--step: an A/B build of the library under tnmf_amd/lib')
    ap.add_argument('--ab-lib', default=None, help='driver: also time the kernels on this A/B build, alternating')
    ap.add_argument('--parent-tree', default=None, help="driver: also run bench.py here and in this built checkout")
    ap.add_argument('--step-timeout', type=int, default=240, help='driver: the time limit of every child, in seconds')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.step is None:
        return drive(args)

    import ctypes
    import itertools

    import numpy as np
    import torch
    from bench import CONFIGS
    from tnmf_amd import _lib
    if args.lib:
        _lib.LIB_PATH = args.lib if os.path.isabs(args.lib) else os.path.join(ROOT, 'tnmf_amd', 'lib', args.lib)
    from tnmf_amd.backends.HIP import _ptr
    from tnmf_amd.TransformInvariantNMF import Detections, TransformInvariantNMF

    torch.cuda.set_device(0)
    cfg = CONFIGS[args.config]
    N, C, D, M, A = cfg['N'], cfg['C'], tuple(cfg['D']), cfg['M'], tuple(cfg['A'])
    k = len(A)
    rng = np.random.default_rng(0)
    W = rng.random((M, C) + A).astype(np.float32) ** 4 + 0.01
    W /= W.sum(axis=tuple(range(2, W.ndim)), keepdims=True)
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
    common = dict(library=os.path.basename(_lib.LIB_PATH), config=args.config, dtype='float32', planted=K,
                  events_per_sample=args.events, taps=C * int(np.prod(A)), half_norm_V=round(half_norm, 3))

    # -- the two kernels on the same list against the same render ('valid' mode: the occurrence starts at shift - (A - 1))
    if args.step == 'kernels':
        origin = shift - (np.array(A) - 1)
        whole = np.all((origin - 1 >= 0) & (origin + 1 + np.array(A) <= np.array(D)), axis=1)
        staged = whole & (C * int(np.prod([a + 2 for a in A])) <= 2048)
        s, p, u, h = be._check_events(M, sample, plane, shift, strength)
        images, cell_start, events = be.event_list(s, p, u)
        R = be.render_event_list(nmf._W, images, cell_start, h)
        geom = ctypes.byref(be._geom(be.n_local_samples, M))
        nb = 3 ** k
        gain, gmag = (torch.empty(K, dtype=torch.float64, device='cuda') for _ in range(2))
        a, b, mag = (torch.empty((K, nb), dtype=torch.float64, device='cuda') for _ in range(3))

        def call_gain():
            _lib.check(be._lib.tnmf_hip_events_gain(be._ctx, geom, be._mode, _ptr(nmf._W), _ptr(events), _ptr(h), K,
                                                    _ptr(be._V_dev), _ptr(R), _ptr(gain), _ptr(gmag), be._stream()),
                       'tnmf_hip_events_gain')

        def call_landscape():
            _lib.check(be._lib.tnmf_hip_events_landscape(be._ctx, geom, be._mode, _ptr(nmf._W), _ptr(events), _ptr(h), K,
                                                         _ptr(be._V_dev), _ptr(R), _ptr(a), _ptr(b), _ptr(mag), be._stream()),
                       'tnmf_hip_events_landscape')

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.calls

        for fn in (call_gain, call_landscape):       # warm-up of both
            timed(fn)
        rounds = [(timed(call_gain), timed(call_landscape)) for _ in range(args.rounds)]
        g_ms, l_ms = (statistics.median(x) for x in zip(*rounds))
        ratios = sorted(ll / gg for gg, ll in rounds)
        centre = (nb - 1) // 2
        hv = h.double()
        identity = float(((hv * (a[:, centre] - hv * b[:, centre]) + 0.5 * hv * hv * b[:, centre] - gain).abs() / gmag).max())
        emit(dict(what='landscape_vs_gain', gain_ms=round(g_ms, 5), landscape_ms=round(l_ms, 5), ratio=round(l_ms / g_ms, 3),
                  ratio_quartiles=[round(ratios[len(ratios) // 4], 3), round(ratios[(3 * len(ratios)) // 4], 3)],
                  calls_per_timing=args.calls, rounds=args.rounds, rows_staged=int(staged.sum()), rows_walk=int(K - staged.sum()),
                  neighbours=nb, gain_identity_rel_mag=identity, **common))

    # -- the planted list, every row one pixel off, moved back
    if args.step == 'relocate':
        S = np.array([d + x - 1 for d, x in zip(D, A)])
        nonzero = np.array([d for d in itertools.product((-1, 0, 1), repeat=k) if any(d)])
        moved = np.clip(shift + nonzero[rng.integers(len(nonzero), size=K)], 0, S - 1)
        rows = np.column_stack([sample, plane, moved])
        keep = np.sort(np.unique(rows, axis=0, return_index=True)[1])       # (the list must stay distinct)
        off = np.array(A) - 1
        start = Detections(sample=sample[keep], atom=plane[keep], transform=np.zeros(len(keep), dtype=np.int64),
                           shift=moved[keep], origin=moved[keep] - off, strength=strength[keep])
        walls = []
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            det, gains = nmf.relocate_detections(start)
            torch.cuda.synchronize()
            if i >= args.warmup:
                walls.append(time.perf_counter() - t0)
        hist = nmf.relocation_history_
        be.start_timeline()
        nmf.relocate_detections(start)
        spans = be.stop_timeline()
        device_ms = {name: round(sum(spans.get(name, [])), 3) for name in ('events_landscape', 'events_render',
                                                                           'events_update', 'events_gain', 'event_list')}
        R_end = nmf.reconstruct_detections(det).astype(np.float64)
        R_start = nmf.reconstruct_detections(nmf.refit_detections(start)).astype(np.float64)
        emit(dict(what='relocate', wall_ms=round(1e3 * statistics.median(walls), 2),
                  wall_ms_runs=[round(1e3 * w, 2) for w in walls], rows=len(det),
                  displaced=int(np.any(moved != shift, axis=1).sum()),
                  rounds=len(hist), hops_per_round=hist[:, 1].astype(int).tolist(),
                  candidates_per_round=hist[:, 0].astype(int).tolist(),
                  back_at_planted=int(np.all(det.shift == shift[keep], axis=1).sum()),
                  objective_refit_only=round(0.5 * float(np.sum((V - R_start) ** 2)), 5),
                  objective=round(0.5 * float(np.sum((V - R_end) ** 2)), 5), device_ms_total=device_ms,
                  repeats=args.repeats, **common))


def drive(args):
    """The steps as children, each under its own time limit; the first failure ends the probe."""
    here = os.path.abspath(__file__)
    scene = ['--config', str(args.config), '--events', str(args.events), '--calls', str(args.calls), '--rounds',
             str(args.rounds), '--warmup', str(args.warmup), '--repeats', str(args.repeats)]
    scene += ['--out', args.out] if args.out else []

    def child(command, cwd=ROOT, capture=False):
        command = ['timeout', '-k', '10', str(args.step_timeout)] + command
        print('== ' + ' '.join(command) + (f'   (in {cwd})' if cwd != ROOT else ''), file=sys.stderr, flush=True)
        done = subprocess.run(command, cwd=cwd, stdout=subprocess.PIPE if capture else None, text=True)
        if done.returncode != 0:
            sys.exit(f'landscape_bench: the step above ended with status {done.returncode}; nothing more is started')
        return done.stdout

    def step(name, lib=None):
        child([sys.executable, here, '--step', name] + (['--lib', lib] if lib else []) + scene)

    step('kernels')
    step('relocate')
    if args.ab_lib:
        step('kernels', args.ab_lib)
        step('kernels')
        step('kernels', args.ab_lib)
    if args.parent_tree:
        parent = os.path.abspath(args.parent_tree)
        for run in (1, 2):
            for tree, cwd in (('this', ROOT), ('parent', parent)):
                out = child([sys.executable, 'bench.py', '--gpus', '1', '--steps', '30', '--warmup', '5'], cwd, capture=True)
                d = json.loads([line for line in out.splitlines() if line.startswith('{')][-1])
                line = dict(what='bench_headline', tree=tree, run=run, ms_per_step=round(d['ms_per_step'], 4),
                            value=round(d['value'], 2), unit=d['unit'], steps=d['steps'], warmup=d['warmup'],
                            n_gpus=d['n_gpus'])
                print(json.dumps(line), flush=True)
                if args.out:
                    with open(args.out, 'a') as f:
                        f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
