"""What rendering and refitting the detections of a fitted model costs, next to the dense H side (float32, path='auto'; not
part of bench.py).

    python tools/probes/events_bench.py [--config 3] [--iterations 20] [--sparsity 0.1] [--threshold-fracs 0.2 0.05]
                                        [--warmup 3] [--repeats 9] [--lib LIB.so] [--out FILE]

A model of the BASELINE config (bench.py's CONFIGS, planted synthetic samples of bench.py) is fitted for `iterations`
iterations with sparsity_H > 0 from a seeded device initialisation.  Per threshold (a fraction of the largest activation,
min_distance the default) one JSON line (printed; --out appends it to FILE), every time the median of `repeats` runs after
`warmup`:
    list_build_ms     the one-time list build of a support (checks, expansion to images, sort, cell offsets), host clock
                      around a synchronised call
    render_ms         tnmf_hip_events_render alone, between two HIP events
    update_ms         tnmf_hip_events_update alone
    refit_step_ms     one refit step: render + update, between two HIP events
and, measured in the same run on the model's own H:
    dense_update_H_ms one dense H half step (fused_update_H, no inhibition)
    dense_reconstruct_ms  one dense reconstruct
The refit step is there to be cheaper than the dense H half step: `refit_step_below_dense_update_H` says whether it is.
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
    ap.add_argument('--iterations', type=int, default=20)
    ap.add_argument('--sparsity', type=float, default=0.1)
    ap.add_argument('--threshold-fracs', type=float, nargs='+', default=[0.2, 0.05])
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--lib', default=None, help='an A/B build of the library under tnmf_amd/lib (make VARIANT=...)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from bench import CONFIGS, synth_V_on_device
    from tnmf_amd import _lib
    if args.lib:
        _lib.LIB_PATH = args.lib if os.path.isabs(args.lib) else os.path.join(ROOT, 'tnmf_amd', 'lib', args.lib)
    from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    cfg = CONFIGS[args.config]
    V = synth_V_on_device(cfg, cfg['N'], seed=0, device=dev)

    def device_ms(fn):
        """median ms of fn() between two HIP events"""
        times = []
        for i in range(args.warmup + args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times.append(e0.elapsed_time(e1))
        return statistics.median(times)

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(json.dumps(line) + '\n')

    torch.cuda.manual_seed(1)   # (init='device' draws from the device generator)
    nmf = TransformInvariantNMF(n_atoms=cfg['M'], atom_shape=cfg['A'], backend='hip', path='auto', init='device')
    nmf.fit_batch(V, n_iterations=args.iterations, sparsity_H=args.sparsity, progress_callback=lambda *_: True)
    be, H, W = nmf._backend, nmf._H, nmf._W_dict
    h_max = float(H.max().item())
    common = dict(library=os.path.basename(_lib.LIB_PATH), config=args.config, dtype='float32', path='auto',
                  iterations=args.iterations, sparsity_H=args.sparsity, H_shape=list(H.shape),
                  R_MB=round(be._V_dev.numel() * be._V_dev.element_size() / 1e6, 1), repeats=args.repeats)
    legs = []
    for frac in args.threshold_fracs:
        det = nmf.detections(threshold=frac * h_max)
        legs.append((frac, det))

    R = torch.empty_like(be._V_dev)
    results = []
    for frac, det in legs:
        plane = det.atom * nmf.n_transforms + det.transform
        build = []
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s, p, u, h = be._check_events(W.shape[0], det.sample, plane, det.shift, det.strength)
            images, cell_start, events = be.event_list(s, p, u)
            torch.cuda.synchronize()
            if i >= args.warmup:
                build.append(1e3 * (time.perf_counter() - t0))
        strength = h.clone()
        render_ms = device_ms(lambda: be.render_event_list(W, images, cell_start, strength, R))
        update_ms = device_ms(lambda: be.update_event_list(W, events, strength, R, args.sparsity, nmf.eps))

        def step():
            be.render_event_list(W, images, cell_start, strength, R)
            be.update_event_list(W, events, strength, R, args.sparsity, nmf.eps)
        strength.copy_(h)
        step_ms = device_ms(step)
        assert bool(torch.isfinite(strength).all())
        results.append(dict(what='events', threshold_frac_of_max=frac, threshold=frac * h_max, events=len(det),
                            images=int(images.shape[0]), cells=int(cell_start.numel() - 1),
                            list_build_ms=round(statistics.median(build), 3), render_ms=round(render_ms, 4),
                            update_ms=round(update_ms, 4), refit_step_ms=round(step_ms, 4)))

    # the dense H side of the same run, on the model's own H (the half step changes it: measured last)
    dense_reconstruct_ms = device_ms(lambda: be.reconstruct(W, H))
    dense_update_ms = device_ms(lambda: be.fused_update_H(V, W, H, sparsity=args.sparsity, eps=nmf.eps))
    for r in results:
        emit(dict(**r, dense_update_H_ms=round(dense_update_ms, 4), dense_reconstruct_ms=round(dense_reconstruct_ms, 4),
                  refit_step_below_dense_update_H=bool(r['refit_step_ms'] < dense_update_ms), **common))


if __name__ == '__main__':
    main()
