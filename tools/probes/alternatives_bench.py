"""What the alternatives of a list cost next to its gains and its landscape, and what relabelling a list whose every
orientation is wrong costs (float32, path='auto'; not part of bench.py).

    python tools/probes/alternatives_bench.py [--config 3] [--events 50] [--calls 200] [--rounds 7] [--warmup 1] [--repeats 3]
                                              [--ab-lib LIB.so] [--parent-tree DIR] [--step-timeout 240] [--out FILE]

Without --step this process only drives: it never opens the GPU.  Every GPU step is a child process of its own under
`timeout -k 10 <--step-timeout>`, one after the other, and the first child that fails, faults or runs out of time ends the
probe -- nothing more is started on the GPU after it.  The steps, in order:
    --step kernels                     on the product library: every plane of the plain model (n_alt = M, stride 1)
    --step kernels-rot90               on the product library: the 4 orientations of a 'rot90' model of M / 4 atoms
    --step relabel                     on the product library
    --step kernels --lib <--ab-lib>    with --ab-lib: an A/B build under tnmf_amd/lib (make VARIANT=alwalk
                                       VFLAGS=-DTNMF_ALTERNATIVES_WALK_ONLY: the alternatives without their staged path), then
                                       the product's kernels step and the A/B build's once more, so that the two alternate
    bench.py --gpus 1 --steps 30 --warmup 5    with --parent-tree: in this tree, then in DIR (a built checkout of the parent
                                       commit), twice, alternating; what='bench_headline' lines with tree='this' / 'parent'

The scene is that of tools/probes/landscape_bench.py: a random normalised dictionary of the BASELINE config's shape (bench.py's
CONFIGS) and `events` events per sample at random shifts wholly inside the sample, strengths 1 .. 2, rendered with the
product's own kernel, plus noise of 1e-3.  JSON lines (printed; --out appends them to FILE):
    what='alternatives_vs_gain'  tnmf_hip_events_alternatives (a, b and mag written) against tnmf_hip_events_gain (gain and mag)
                              and tnmf_hip_events_landscape (a, b and mag) on the planted list against the same render, in the
                              same process: `rounds` rounds that alternate the three, each timing `calls` back-to-back launches
                              between two device events; the medians per call, the ratios, the quartiles of the per-round
                              ratios, and which path the rows take (the host mirror of the rule in alternatives.hip).  n_alt
                              plain walks would cost about n_alt x the gain.
    what='relabel'            relabel_detections on the planted list of the 'rot90' model with every orientation wrong:
                              wall-clock median of `repeats` runs after `warmup` (host work included: the hops are chosen
                              there), rounds, hops per round, rows back at their planted orientation, objective, and the
                              device spans of its legs.
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
    ap.add_argument('--step', choices=['kernels', 'kernels-rot90', 'relabel'], default=None,
                    help='run this one step here (a child)')
    ap.add_argument('--lib', default=None, help='--step: an A/B build of the library under tnmf_amd/lib')
    ap.add_argument('--ab-lib', default=None, help='driver: also time the kernels on this A/B build, alternating')
    ap.add_argument('--parent-tree', default=None, help="driver: also run bench.py here and in this built checkout")
    ap.add_argument('--step-timeout', type=int, default=240, help='driver: the time limit of every child, in seconds')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.step is None:
        return drive(args)

    import ctypes

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
    rot90 = args.step != 'kernels'
    T = 4 if rot90 else 1
    M = M // T                      # the same number of planes either way
    rng = np.random.default_rng(0)
    W = rng.random((M, C) + A).astype(np.float32) ** 4 + 0.01
    W /= W.sum(axis=tuple(range(2, W.ndim)), keepdims=True)
    K = N * args.events
    sample = np.repeat(np.arange(N), args.events)
    plane = rng.integers(M * T, size=K)
    shift = np.stack([rng.integers(a - 1, d, size=K) for a, d in zip(A, D)], axis=1)   # (wholly inside the sample)
    strength = (1. + rng.random(K)).astype(np.float32)

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(json.dumps(line) + '\n')

    def model(V):
        nmf = TransformInvariantNMF(n_atoms=M, atom_shape=A, backend='hip', path='auto', init='device',
                                    transforms='rot90' if rot90 else None)
        nmf._W = torch.from_numpy(W).cuda()
        nmf.fit_batch(V, n_iterations=0, keep_W=True)
        return nmf

    torch.cuda.manual_seed(1)
    nmf = model(np.zeros((N, C) + D, dtype=np.float32))
    be = nmf._backend
    V = be.render_events(nmf._W_dict, sample, plane, shift, strength)
    V = (V + 1e-3 * torch.rand_like(V)).cpu().numpy()
    nmf = model(V)
    be = nmf._backend
    W_dict = nmf._W_dict
    half_norm = 0.5 * float(np.sum(V.astype(np.float64) ** 2))
    common = dict(library=os.path.basename(_lib.LIB_PATH), config=args.config, dtype='float32', planted=K,
                  events_per_sample=args.events, taps=C * int(np.prod(A)), transforms='rot90' if rot90 else None,
                  planes=M * T, half_norm_V=round(half_norm, 3))

    # -- the three kernels on the same list against the same render ('valid' mode: the occurrence starts at shift - (A - 1))
    if args.step in ('kernels', 'kernels-rot90'):
        n_alt, stride = (T, 1) if rot90 else (M, 1)
        origin = shift - (np.array(A) - 1)
        whole = np.all((origin >= 0) & (origin + np.array(A) <= np.array(D)), axis=1)
        staged = whole & (C * int(np.prod(A)) <= 2048)
        s, p, u, h = be._check_events(M * T, sample, plane, shift, strength)
        images, cell_start, events = be.event_list(s, p, u)
        R = be.render_event_list(W_dict, images, cell_start, h)
        geom = ctypes.byref(be._geom(be.n_local_samples, M * T))
        nb = 3 ** k
        gain, gmag = (torch.empty(K, dtype=torch.float64, device='cuda') for _ in range(2))
        la, lb, lmag = (torch.empty((K, nb), dtype=torch.float64, device='cuda') for _ in range(3))
        a, b, mag = (torch.empty((K, n_alt), dtype=torch.float64, device='cuda') for _ in range(3))

        def call_gain():
            _lib.check(be._lib.tnmf_hip_events_gain(be._ctx, geom, be._mode, _ptr(W_dict), _ptr(events), _ptr(h), K,
                                                    _ptr(be._V_dev), _ptr(R), _ptr(gain), _ptr(gmag), be._stream()),
                       'tnmf_hip_events_gain')

        def call_landscape():
            _lib.check(be._lib.tnmf_hip_events_landscape(be._ctx, geom, be._mode, _ptr(W_dict), _ptr(events), _ptr(h), K,
                                                         _ptr(be._V_dev), _ptr(R), _ptr(la), _ptr(lb), _ptr(lmag),
                                                         be._stream()), 'tnmf_hip_events_landscape')

        def call_alternatives():
            _lib.check(be._lib.tnmf_hip_events_alternatives(be._ctx, geom, be._mode, _ptr(W_dict), _ptr(events), _ptr(h), K,
                                                            _ptr(be._V_dev), _ptr(R), n_alt, stride, _ptr(a), _ptr(b),
                                                            _ptr(mag), be._stream()), 'tnmf_hip_events_alternatives')

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.calls

        for fn in (call_gain, call_landscape, call_alternatives):       # warm-up of all three
            timed(fn)
        rounds = [(timed(call_gain), timed(call_landscape), timed(call_alternatives)) for _ in range(args.rounds)]
        g_ms, l_ms, a_ms = (statistics.median(x) for x in zip(*rounds))
        vs_gain = sorted(aa / gg for gg, ll, aa in rounds)
        vs_landscape = sorted(aa / ll for gg, ll, aa in rounds)
        quartiles = lambda r: [round(r[len(r) // 4], 3), round(r[(3 * len(r)) // 4], 3)]   # noqa: E731
        own = (p - p // (n_alt * stride) * (n_alt * stride) - p % stride) // stride
        every = torch.arange(K, device='cuda')
        a0, b0 = a[every, own], b[every, own]
        hv = h.double()
        identity = float(((hv * (a0 - hv * b0) + 0.5 * hv * hv * b0 - gain).abs() / gmag).max())
        centre = (nb - 1) // 2
        emit(dict(what='alternatives_vs_gain', n_alt=n_alt, stride=stride, gain_ms=round(g_ms, 5),
                  landscape_ms=round(l_ms, 5), alternatives_ms=round(a_ms, 5), ratio_to_gain=round(a_ms / g_ms, 3),
                  ratio_to_gain_quartiles=quartiles(vs_gain), ratio_to_landscape=round(a_ms / l_ms, 3),
                  ratio_to_landscape_quartiles=quartiles(vs_landscape), calls_per_timing=args.calls, rounds=args.rounds,
                  rows_staged=int(staged.sum()), rows_walk=int(K - staged.sum()), gain_identity_rel_mag=identity,
                  own_column_equals_landscape_centre=bool(torch.equal(a0, la[:, centre]) and torch.equal(b0, lb[:, centre])),
                  **common))

    # -- the planted list of the 'rot90' model, every orientation wrong, relabelled
    if args.step == 'relabel':
        rows = np.column_stack([sample, plane, shift])
        keep = np.sort(np.unique(rows, axis=0, return_index=True)[1])       # (the list must be distinct)
        atom, true = plane[keep] // T, plane[keep] % T
        wrong = (true + rng.integers(1, T, size=len(keep))) % T
        off = np.array(A) - 1
        start = Detections(sample=sample[keep], atom=atom, transform=wrong, shift=shift[keep], origin=shift[keep] - off,
                           strength=strength[keep])
        walls = []
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            det, gains = nmf.relabel_detections(start)
            torch.cuda.synchronize()
            if i >= args.warmup:
                walls.append(time.perf_counter() - t0)
        hist = nmf.relabel_history_
        be.start_timeline()
        nmf.relabel_detections(start)
        spans = be.stop_timeline()
        device_ms = {name: round(sum(spans.get(name, [])), 3) for name in ('events_alternatives', 'events_render',
                                                                           'events_update', 'events_gain', 'event_list')}
        R_end = nmf.reconstruct_detections(det).astype(np.float64)
        R_start = nmf.reconstruct_detections(nmf.refit_detections(start)).astype(np.float64)
        emit(dict(what='relabel', over='transforms', wall_ms=round(1e3 * statistics.median(walls), 2),
                  wall_ms_runs=[round(1e3 * w, 2) for w in walls], rows=len(det), rounds=len(hist),
                  hops_per_round=hist[:, 1].astype(int).tolist(), candidates_per_round=hist[:, 0].astype(int).tolist(),
                  back_at_planted=int(np.sum(det.transform == true)),
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
            sys.exit(f'alternatives_bench: the step above ended with status {done.returncode}; nothing more is started')
        return done.stdout

    def step(name, lib=None):
        child([sys.executable, here, '--step', name] + (['--lib', lib] if lib else []) + scene)

    step('kernels')
    step('kernels-rot90')
    step('relabel')
    if args.ab_lib:
        step('kernels', args.ab_lib)
        step('kernels')
        step('kernels', args.ab_lib)
        step('kernels-rot90', args.ab_lib)
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
