"""What reading the detections off a fitted model costs (float32, path='auto'; not part of bench.py).

    python tools/probes/peaks_bench.py [--config 3] [--iterations 20] [--sparsity 0.1] [--threshold-frac 0.05]
                                       [--warmup 3] [--repeats 9] [--host-samples 8] [--lib LIB.so] [--out FILE]

A model of the BASELINE config (bench.py's CONFIGS, planted synthetic samples of bench.py) is fitted for `iterations`
iterations with sparsity_H > 0; the threshold is `threshold-frac` of the largest activation, min_distance the default
(the model's inhibition_range).  JSON lines (printed; --out appends them to FILE):
    detections_device   tnmf_hip_find_peaks alone between two HIP events (median of `repeats` after `warmup`), its GB/s over
                        one read of the logical H, and the whole detections() call -- kernel, count read-back, sort on the
                        device, copy of the compact list, unravelling on the host -- by the host clock around a synchronised
                        call (median)
    host_route          what a user had before detections(): the H property (the whole tensor to the host; timed in full)
                        and a NumPy search that visits candidates only (find_peaks_numpy, timed on the first
                        `host-samples` samples and scaled to all of them -- it is minutes long otherwise); its detections of
                        those samples are compared with the device's
    kernel_at_threshold the kernel alone at 20 % of the maximum, and at the maximum itself: nothing passes, the streaming floor
    dense_worst_case    the kernel on the H of a fresh initialisation with threshold 0: every entry is a candidate
--lib: the same with another build of the library, e.g. the LDS-tiled window walk of
`make -C tnmf_amd/csrc VARIANT=peakstiled VFLAGS=-DTNMF_PEAKS_TILED` -> libtnmf_hip_peakstiled.so.
"""
import argparse
import ctypes
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
    ap.add_argument('--threshold-frac', type=float, default=0.05)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--host-samples', type=int, default=8)
    ap.add_argument('--lib', default=None, help='an A/B build of the library under tnmf_amd/lib (make VARIANT=...)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from bench import CONFIGS, synth_V_on_device
    from tnmf_amd import _lib
    if args.lib:
        _lib.LIB_PATH = args.lib if os.path.isabs(args.lib) else os.path.join(ROOT, 'tnmf_amd', 'lib', args.lib)
    from tnmf_amd.TransformInvariantNMF import TransformInvariantNMF, find_peaks_numpy

    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    cfg = CONFIGS[args.config]
    V = synth_V_on_device(cfg, cfg['N'], seed=0, device=dev)

    def kernel_ms(nmf, threshold, radius, capacity, warmup, repeats):
        """(median ms of tnmf_hip_find_peaks alone, count)"""
        be, H = nmf._backend, nmf._H
        ld = be._row_stride(H)
        assert ld is not None
        k = len(nmf.atom_shape)
        g = _lib.make_geom(H.shape[0], H.shape[1], be.n_channels, tuple(H.shape[2:]), (1,) * k, be._dtype_code, ld)
        rad = (ctypes.c_int * 3)(*radius)
        idx = torch.empty(capacity, dtype=torch.int64, device=dev)
        val = torch.empty(capacity, dtype=H.dtype, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        times = []
        for i in range(warmup + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(be._lib.tnmf_hip_find_peaks(be._ctx, ctypes.byref(g), ctypes.c_void_p(H.data_ptr()),
                                                   float(threshold), rad, 1, ctypes.c_void_p(idx.data_ptr()),
                                                   ctypes.c_void_p(val.data_ptr()), capacity,
                                                   ctypes.c_void_p(count.data_ptr()), stream), 'tnmf_hip_find_peaks')
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times.append(e0.elapsed_time(e1))
        return statistics.median(times), int(count.item())

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(json.dumps(line) + '\n')

    torch.cuda.manual_seed(1)   # (init='device' draws from the device generator: the same H for every library build)
    nmf = TransformInvariantNMF(n_atoms=cfg['M'], atom_shape=cfg['A'], backend='hip', path='auto', init='device')
    nmf.fit_batch(V, n_iterations=args.iterations, sparsity_H=args.sparsity, progress_callback=lambda *_: True)
    H = nmf._H
    h_bytes = H.numel() * H.element_size()
    h_max = float(H.max().item())
    t = args.threshold_frac * h_max
    radius = nmf._inhibition_range
    candidates = int((H > t).sum().item())
    common = dict(library=os.path.basename(_lib.LIB_PATH), config=args.config, dtype='float32', path='auto',
                  iterations=args.iterations, sparsity_H=args.sparsity,
                  H_shape=list(H.shape), H_row_stride=int(nmf._backend._row_stride(H) or H.shape[-1]),
                  H_logical_GB=round(h_bytes / 1e9, 4), threshold=t, threshold_frac_of_max=args.threshold_frac,
                  min_distance=list(radius), candidates=candidates, entries=H.numel())

    ms, count = kernel_ms(nmf, t, radius, max(4096, H.numel() // 256), args.warmup, args.repeats)
    whole = []
    det = None
    for i in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        det = nmf.detections(threshold=t)
        torch.cuda.synchronize()
        if i >= args.warmup:
            whole.append(1e3 * (time.perf_counter() - t0))
    assert len(det) == count
    emit(dict(what='detections_device', detections=count, kernel_ms=round(ms, 4),
              kernel_GBps_over_one_read_of_H=round(h_bytes / 1e6 / ms, 1),
              detections_call_ms=round(statistics.median(whole), 3), repeats=args.repeats, **common))

    # the same kernel where it has less to examine: a higher threshold, and one nothing passes (the streaming floor)
    for frac in (0.2, 1.0):
        ms_f, count_f = kernel_ms(nmf, frac * h_max, radius, max(4096, H.numel() // 256), 1, 5)
        emit(dict(what='kernel_at_threshold', threshold_frac_of_max=frac, candidates=int((H > frac * h_max).sum().item()),
                  detections=count_f, kernel_ms=round(ms_f, 4), kernel_GBps_over_one_read_of_H=round(h_bytes / 1e6 / ms_f, 1),
                  library=common['library'], config=args.config, repeats=5))

    # the route of a user without detections(): the whole H to the host, then NumPy on the candidates
    t0 = time.perf_counter()
    H_host = nmf.H
    copy_s = time.perf_counter() - t0
    n_host = max(1, min(args.host_samples, H_host.shape[0]))
    t0 = time.perf_counter()
    idx, val = find_peaks_numpy(H_host[:n_host], t, radius, 1)
    search_s = time.perf_counter() - t0
    same = det.sample < n_host
    at = np.unravel_index(idx, H_host[:n_host].shape)
    assert np.array_equal(at[0], det.sample[same]) and np.array_equal(at[1], det.atom[same])
    assert np.array_equal(np.stack(at[2:], 1), det.shift[same]) and val.tobytes() == det.strength[same].tobytes()
    scaled = search_s * H_host.shape[0] / n_host
    emit(dict(what='host_route', H_copy_s=round(copy_s, 3), search_samples=n_host, search_s=round(search_s, 3),
              search_s_scaled_to_all_samples=round(scaled, 2), total_s_scaled=round(copy_s + scaled, 2),
              detections_in_searched_samples=int(len(idx)), **common))
    del H_host

    # worst case: a dense H (fresh initialisation), every entry a candidate
    nmf.fit_batch(V, n_iterations=0, progress_callback=lambda *_: True)
    H = nmf._H
    ms, count = kernel_ms(nmf, 0., radius, max(4096, H.numel() // 256), 1, 3)
    emit(dict(what='dense_worst_case', detections=count, kernel_ms=round(ms, 3),
              kernel_GBps_over_one_read_of_H=round(h_bytes / 1e6 / ms, 1), threshold=0., repeats=3,
              **{k: v for k, v in common.items() if k not in ('threshold', 'threshold_frac_of_max', 'candidates',
                                                               'iterations', 'sparsity_H')},
              candidates=int((H > 0).sum().item())))


if __name__ == '__main__':
    main()
