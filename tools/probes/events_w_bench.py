"""What a W half step on the detections of a fitted model costs, next to the dense W half step (float32, path='auto'; not part
of bench.py).

    python tools/probes/events_w_bench.py [--config 3] [--iterations 20] [--sparsity 0.1] [--threshold-fracs 0.2 0.05]
                                          [--warmup 3] [--repeats 9] [--lib LIB.so] [--segment N] [--out FILE]

The model and the thresholds are those of tools/probes/events_bench.py: a model of the BASELINE config is fitted for
`iterations` iterations with sparsity_H > 0 from a seeded device initialisation.  Per threshold (a fraction of the largest
activation, min_distance the default) one JSON line (printed; --out appends it to FILE), every time the median of `repeats`
runs after `warmup`:
    plane_list_build_ms  the one-time build of the plane list of a support (sort by plane, offsets, workspace), host clock
                         around a synchronised call
    grad_W_ms            tnmf_hip_events_grad_W alone (both kernels), between two HIP events
    sparse_W_step_ms     one whole W step on the list: render + gradient + the tail of the dense W half step
    fit_iteration_ms     one whole fit_events iteration: render + update of the strengths, then the W step
and, measured in the same run on the model's own H:
    dense_update_W_ms    one dense W half step (fused_update_W)
    dense_iteration_ms   one dense full iteration (fused_update_H + fused_update_W)
The W step on the list is there to be cheaper than the dense W half step: `sparse_W_step_below_dense_update_W` says whether
it is.  --lib / --segment: an A/B build of the library with another TNMF_EVENTS_SEGMENT (make VARIANT=seg128
VFLAGS=-DTNMF_EVENTS_SEGMENT=128) and the same value for the workspace here.
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
    ap.add_argument('--segment', type=int, default=None, help='TNMF_EVENTS_SEGMENT of the --lib build')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from bench import CONFIGS, synth_V_on_device
    from tnmf_amd import _lib
    if args.lib:
        _lib.LIB_PATH = args.lib if os.path.isabs(args.lib) else os.path.join(ROOT, 'tnmf_amd', 'lib', args.lib)
    if args.segment:
        _lib.EVENT_SEGMENT = args.segment
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
    be, H = nmf._backend, nmf._H
    W0 = nmf._W.clone()
    h_max = float(H.max().item())
    common = dict(library=os.path.basename(_lib.LIB_PATH), segment=_lib.EVENT_SEGMENT, config=args.config, dtype='float32',
                  path='auto', iterations=args.iterations, sparsity_H=args.sparsity, H_shape=list(H.shape),
                  repeats=args.repeats)
    legs = [(frac, nmf.detections(threshold=frac * h_max)) for frac in args.threshold_fracs]

    R = torch.empty_like(be._V_dev)
    results = []
    for frac, det in legs:
        W = W0.clone()      # every leg from the fitted dictionary
        plane = det.atom * nmf.n_transforms + det.transform
        s, p, u, h = be._check_events(W.shape[0], det.sample, plane, det.shift, det.strength)
        images, cell_start, events = be.event_list(s, p, u)
        build = []
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lists = be.event_plane_list(p, W.shape[0])
            torch.cuda.synchronize()
            if i >= args.warmup:
                build.append(1e3 * (time.perf_counter() - t0))
        strength = h.clone()
        be.render_event_list(W, images, cell_start, strength, R)
        grad_ms = device_ms(lambda: be.gradient_W_event_list(W, events, lists, strength, R))

        def w_step():
            be.render_event_list(W, images, cell_start, strength, R)
            be.update_W_event_list(W, None, None, be.gradient_W_event_list(W, events, lists, strength, R), nmf.eps)

        def iteration():
            be.render_event_list(W, images, cell_start, strength, R)
            be.update_event_list(W, events, strength, R, args.sparsity, nmf.eps)
            w_step()
        w_step_ms = device_ms(w_step)
        W.copy_(W0)
        iteration_ms = device_ms(iteration)
        assert bool(torch.isfinite(strength).all()) and bool(torch.isfinite(W).all())
        n_seg = int(torch.div(lists[1][1:] - lists[1][:-1] + _lib.EVENT_SEGMENT - 1, _lib.EVENT_SEGMENT,
                              rounding_mode='floor').sum().item())
        results.append(dict(what='events_w', threshold_frac_of_max=frac, threshold=frac * h_max, events=len(det),
                            segments=n_seg, workspace_MB=round(lists[2].numel() * 8 / 1e6, 2),
                            plane_list_build_ms=round(statistics.median(build), 3), grad_W_ms=round(grad_ms, 4),
                            sparse_W_step_ms=round(w_step_ms, 4), fit_iteration_ms=round(iteration_ms, 4)))

    # the dense side of the same run, on the model's own W and H (the steps change them: measured last)
    W = nmf._W
    dense_W_ms = device_ms(lambda: be.fused_update_W(V, W, H, eps=nmf.eps))

    def dense_iteration():
        be.fused_update_H(V, W, H, sparsity=args.sparsity, eps=nmf.eps)
        be.fused_update_W(V, W, H, eps=nmf.eps)
    dense_iteration_ms = device_ms(dense_iteration)
    for r in results:
        emit(dict(**r, dense_update_W_ms=round(dense_W_ms, 4), dense_iteration_ms=round(dense_iteration_ms, 4),
                  sparse_W_step_below_dense_update_W=bool(r['sparse_W_step_ms'] < dense_W_ms), **common))


if __name__ == '__main__':
    main()
