"""What scoring the detections of a fitted model costs, next to one refit update of the same list (float32, path='auto'; not
part of bench.py).

    python tools/probes/events_gain_bench.py [--config 3] [--iterations 20] [--sparsity 0.1] [--threshold-fracs 0.2 0.05]
                                             [--warmup 3] [--repeats 9] [--lib LIB.so] [--out FILE]

A model of the BASELINE config (bench.py's CONFIGS, planted synthetic samples of bench.py) is fitted for `iterations`
iterations with sparsity_H > 0 from a seeded device initialisation, as in tools/probes/events_bench.py.  Per threshold (a
fraction of the largest activation, min_distance the default) one JSON line (printed; --out appends it to FILE), every time
the median of `repeats` runs after `warmup`, each between two HIP events, on the same lists and the same render R:
    update_ms         tnmf_hip_events_update alone (on a copy of the strengths, restored between the runs)
    gain_ms           tnmf_hip_events_gain alone, gain and mag written
    gain_no_mag_ms    ... with mag = NULL
    gain_over_update  gain_ms / update_ms: both kernels gather V and R under the images of every event, one wave per event
    render_ms         tnmf_hip_events_render alone, for scale: a call of detection_gains is one render and one gain
`images` above `events` says how many rows take the inner loop over the images (none in 'valid' mode, the configs' mode).
"""
import argparse
import json
import os
import statistics
import sys

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

    import ctypes

    import torch
    from bench import CONFIGS, synth_V_on_device
    from tnmf_amd import _lib
    if args.lib:
        _lib.LIB_PATH = args.lib if os.path.isabs(args.lib) else os.path.join(ROOT, 'tnmf_amd', 'lib', args.lib)
    from tnmf_amd.backends.HIP import _ptr
    from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF

    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    cfg = CONFIGS[args.config]
    V = synth_V_on_device(cfg, cfg['N'], seed=0, device=dev)

    def device_ms(fn, before=None):
        """median ms of fn() between two HIP events"""
        times = []
        for i in range(args.warmup + args.repeats):
            if before is not None:
                before()
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
                  taps=int(W[0].numel()), R_MB=round(be._V_dev.numel() * be._V_dev.element_size() / 1e6, 1),
                  repeats=args.repeats)
    R = torch.empty_like(be._V_dev)
    for frac in args.threshold_fracs:
        det = nmf.detections(threshold=frac * h_max)
        plane = det.atom * nmf.n_transforms + det.transform
        s, p, u, h = be._check_events(W.shape[0], det.sample, plane, det.shift, det.strength)
        images, cell_start, events = be.event_list(s, p, u)
        K = h.numel()
        render_ms = device_ms(lambda: be.render_event_list(W, images, cell_start, h, R))
        strength = h.clone()
        update_ms = device_ms(lambda: be.update_event_list(W, events, strength, R, args.sparsity, nmf.eps),
                              before=lambda: strength.copy_(h))
        gain, mag = (torch.empty(K, dtype=torch.float64, device=dev) for _ in range(2))
        geom = be._geom(be.n_local_samples, W.shape[0])

        def score(mag_out):
            _lib.check(be._lib.tnmf_hip_events_gain(be._ctx, ctypes.byref(geom), be._mode, _ptr(W), _ptr(events), _ptr(h), K,
                                                    _ptr(be._V_dev), _ptr(R), _ptr(gain), _ptr(mag_out), be._stream()),
                       'tnmf_hip_events_gain')
        gain_ms = device_ms(lambda: score(mag))
        gain_no_mag_ms = device_ms(lambda: score(None))
        full = be.gain_event_list(W, events, h, R)
        assert torch.equal(full, gain) and bool(torch.isfinite(full).all())
        assert bool((mag * (1 + 1e-12) >= full.abs()).all())
        emit(dict(what='events_gain', threshold_frac_of_max=frac, threshold=frac * h_max, events=K,
                  images=int(images.shape[0]), update_ms=round(update_ms, 4),
                  gain_ms=round(gain_ms, 4), gain_no_mag_ms=round(gain_no_mag_ms, 4),
                  gain_over_update=round(gain_ms / update_ms, 3), render_ms=round(render_ms, 4),
                  positive_gains=int((full > 0).sum().item()), **common))


if __name__ == '__main__':
    main()
