// events.hip -- the sparse H side: a list of events (sample, plane, shift, strength) in the place of the activations
// (include/tnmf_hip.h, "events").
//
// k_events_render is a gather, not a scatter: no float atomics, so the same list gives the same bits run after run.  An
// event stands for its images in the padded activation frame (one, or up to four where a 'circular' / 'reflect' shift lies
// in the wrap / mirror zone of both axes); the caller sorts the images once per support by (sample, cell of the image's
// padded position), cells being the size of an output tile.  A workgroup owns one output tile of one sample, a thread one
// pixel of it.  An image at padded position q covers the pixels q - (A - 1) .. q, so the tile with first pixel t0 is reached
// by the positions t0 .. t0 + tile - 1 + A - 1: the cells t .. (t0 + tile + A - 2) / tile per axis, whose images form ONE run
// of the list per cell row.  The workgroup stages such a run in LDS 256 images at a time -- every thread fetches one image
// and the strength of its event, so the two dependent loads of an image are paid once per chunk, not once per image -- and
// then walks the chunk in list order: each thread adds what lands on its pixel in registers, up to four channels at a time
// (the atom entry comes from W through the cache: a dictionary is a few KB).  Then it writes the pixel, zeros included: no
// memset pass and no read of R.  Measured against the walk that loads each image through a wave-uniform address straight
// from the list: 0.72 ms against 0.97 ms at 939 k events, 0.175 ms against 0.197 ms at 34 k.
//
// k_events_update: one wave per event.  The images are derived from the event itself (the table of the header, Occurrence
// of event_walk.h); the lanes stride over the C * Ay * Ax atom entries (for_each_tap), gather V and R under each image,
// clipped per pixel, into double partial sums, reduce them with a butterfly of fixed order (wave_sum) and lane 0 applies
// the multiplicative update to the strength in place.  It writes the K strengths and nothing else.
//
// k_events_gain: the same walk, one wave per event, for what the event explains: gain_e = E(list without e) - E(list)
// = h a + h^2 b / 2 with a = <phi_e, V - R>, b = |phi_e|^2, phi_e the sum of the event's images clipped to the sample.  The
// images of one event can overlap, so phi_e at a pixel is summed over the images (phi_at; skipped for the single-image
// event, where it is the tap itself).  All in double; the sum of the terms' magnitudes goes out beside the gain as the scale
// of its rounding error.  It writes the K gains (and magnitudes), zeros for a row outside the contract, and nothing else.
//
// k_events_grad_W / k_events_grad_W_sum: the W gradient of the list, many events onto few destinations (P * C * Ay * Ax
// entries), without float atomics: a store pass and an ordered per-destination sum.  The caller sorts the events once per
// support by plane (a permutation and plane_start); each plane's run is cut into segments of TNMF_EVENTS_SEGMENT events, a
// constant of the list contract, so the order of the additions does not depend on the device.  One workgroup per segment
// stages the rows and strengths of its events in LDS, images derived (event_walk.h); a thread owns a tap t = c * Ay * Ax + j
// and walks the events in list order, loading V and R under each image through one address (consecutive jx are contiguous
// in x) into double partial sums.  With at most 128 taps floor(256 / taps) sub-lanes share a tap, sub-lane s taking the
// events s, s + L, ... of the segment, and are added through LDS in sub-lane order; with more than 256 taps the threads
// loop over the taps.  The segment's [2, taps] slab of doubles is stored once; the second kernel adds the slabs of a plane
// in segment order and rounds once to the element type, zeros for a plane without events: negpos is never read.
#include <algorithm>

#include "event_walk.h"

namespace {

constexpr int kChan = 4;    // channels a thread of the render accumulates at a time
constexpr int kWaves = kEventThreads / 64;

template <typename T>
__global__ __launch_bounds__(kEventThreads) void k_events_render(EventGeo g, int tx_log, int nty, int ntx,
                                                                  const T *__restrict__ W, const int4 *__restrict__ img,
                                                                  int n_images, const int *__restrict__ cell_start,
                                                                  const T *__restrict__ h, int n_events,
                                                                  T *__restrict__ R) {
    __shared__ int4 s_img[kEventThreads];   // a chunk of the run: (plane, qy, qx, event), plane -1 for a row to skip
    __shared__ T s_h[kEventThreads];        // ... and the strengths of its events
    const int ly = threadIdx.x >> tx_log, lx = threadIdx.x & (g.tx - 1);
    const int AA = g.Ay * g.Ax;
    const long long tiles = (long long)g.N * nty * ntx;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int tile_x = (int)(tile % ntx), tile_y = (int)(tile / ntx % nty);
        const int n = (int)(tile / ((long long)ntx * nty));
        const int y = tile_y * g.ty + ly, x = tile_x * g.tx + lx;
        const bool inside = y < g.Dy && x < g.Dx;
        // the cells whose images can reach this tile (a cell is a tile's size, so the tile's own cell comes first)
        const int cy1 = min((tile_y * g.ty + g.ty + g.Ay - 2) / g.ty, g.ncy - 1);
        const int cx1 = min((tile_x * g.tx + g.tx + g.Ax - 2) / g.tx, g.ncx - 1);
        for (int c0 = 0; c0 < g.C; c0 += kChan) {
            T acc[kChan];
#pragma unroll
            for (int cc = 0; cc < kChan; ++cc) acc[cc] = (T)0;
            for (int cy = tile_y; cy <= cy1; ++cy) {
                const long long row = ((long long)n * g.ncy + cy) * g.ncx;
                const int i0 = max(cell_start[row + tile_x], 0), i1 = min(cell_start[row + cx1 + 1], n_images);
                for (int base = i0; base < i1; base += kEventThreads) {
                    __syncthreads();   // (the previous chunk has been walked)
                    const int mine = base + (int)threadIdx.x;
                    if (mine < i1) {
                        int4 im = img[mine];   // plane, qy, qx, event
                        const bool ok = (unsigned)im.x < (unsigned)g.P && (unsigned)im.w < (unsigned)n_events;
                        s_h[threadIdx.x] = ok ? h[im.w] : (T)0;
                        if (!ok) im.x = -1;
                        s_img[threadIdx.x] = im;
                    }
                    __syncthreads();
                    const int count = min(i1 - base, kEventThreads);
                    for (int j = 0; j < count; ++j) {
                        const int4 im = s_img[j];
                        if (im.x < 0) continue;
                        const int jy = y - (im.y - (g.Ay - 1)), jx = x - (im.z - (g.Ax - 1));
                        if ((unsigned)jy < (unsigned)g.Ay && (unsigned)jx < (unsigned)g.Ax) {
                            const T hv = s_h[j];
                            const T *w = W + ((size_t)im.x * g.C + c0) * AA + jy * g.Ax + jx;
#pragma unroll
                            for (int cc = 0; cc < kChan; ++cc)
                                if (c0 + cc < g.C) acc[cc] += hv * w[(size_t)cc * AA];
                        }
                    }
                }
            }
            if (inside) {
#pragma unroll
                for (int cc = 0; cc < kChan; ++cc)
                    if (c0 + cc < g.C) R[(((size_t)n * g.C + c0 + cc) * g.Dy + y) * g.Dx + x] = acc[cc];
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kEventThreads) void k_events_update(EventGeo g, int mode, int Sy, int Sx,
                                                                  const T *__restrict__ W, const int4 *__restrict__ ev,
                                                                  T *h, long long n_events, const T *__restrict__ V,
                                                                  const T *__restrict__ R, double reg) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int taps = g.C * g.Ay * g.Ax;
    for (long long e = (long long)blockIdx.x * kWaves + wave; e < n_events; e += (long long)gridDim.x * kWaves) {
        const int4 v = ev[e];   // sample, plane, uy, ux
        if ((unsigned)v.x >= (unsigned)g.N || (unsigned)v.y >= (unsigned)g.P || (unsigned)v.z >= (unsigned)Sy ||
            (unsigned)v.w >= (unsigned)Sx)
            continue;   // (wave-uniform: outside the contract, neither read nor written)
        const Occurrence o(g, mode, Sy, Sx, v.z, v.w);
        const T *w = W + (size_t)v.y * taps;
        const size_t sample = (size_t)v.x * g.C * g.Dy * g.Dx;
        double neg = 0., pos = 0.;
        for_each_tap(g, o, lane, 64, [&](int t, int c, int y, int x) {
            const size_t at = sample + ((size_t)c * g.Dy + y) * g.Dx + x;
            const double wv = (double)w[t];
            neg += wv * (double)V[at];
            pos += wv * (double)R[at];
        });
        neg = wave_sum(neg), pos = wave_sum(pos);
        if (lane == 0) h[e] = (T)((double)h[e] * neg / (pos + reg));
    }
}

template <typename T>
__global__ __launch_bounds__(kEventThreads) void k_events_gain(EventGeo g, int mode, int Sy, int Sx,
                                                                const T *__restrict__ W, const int4 *__restrict__ ev,
                                                                const T *__restrict__ h, long long n_events,
                                                                const T *__restrict__ V, const T *__restrict__ R,
                                                                double *__restrict__ gain, double *__restrict__ mag) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int AA = g.Ay * g.Ax, taps = g.C * AA;
    for (long long e = (long long)blockIdx.x * kWaves + wave; e < n_events; e += (long long)gridDim.x * kWaves) {
        const int4 v = ev[e];   // sample, plane, uy, ux
        if ((unsigned)v.x >= (unsigned)g.N || (unsigned)v.y >= (unsigned)g.P || (unsigned)v.z >= (unsigned)Sy ||
            (unsigned)v.w >= (unsigned)Sx) {   // (wave-uniform: outside the contract, no sample data is read)
            if (lane == 0) {
                gain[e] = 0.;
                if (mag) mag[e] = 0.;
            }
            continue;
        }
        const Occurrence o(g, mode, Sy, Sx, v.z, v.w);
        const bool single = o.single();   // (wave-uniform)
        const T *w = W + (size_t)v.y * taps;
        const size_t sample = (size_t)v.x * g.C * g.Dy * g.Dx;
        const double hv = (double)h[e], hh = 0.5 * hv * hv;
        double a = 0., b = 0., m = 0.;
        for_each_tap(g, o, lane, 64, [&](int t, int c, int y, int x) {
            const size_t at = sample + ((size_t)c * g.Dy + y) * g.Dx + x;
            const double wv = (double)w[t];
            const double phi = single ? wv : phi_at(g, o, w, c * AA, y, x);
            const double wd = wv * ((double)V[at] - (double)R[at]), wp = wv * phi;
            a += wd;
            b += wp;
            m += fma(hh, fabs(wp), hv * fabs(wd));   // (hv |wd| + hh |wp|, the contraction spelled out as for the gain below)
        });
        a = wave_sum(a), b = wave_sum(b), m = wave_sum(m);
        if (lane == 0) {
            gain[e] = fma(hh, b, hv * a);   // (hv * a + hh * b with the contraction spelled out: the compiler may pick either)
            if (mag) mag[e] = m;
        }
    }
}

// The segments are numbered through the planes in plane order: plane p owns ceil(count_p / TNMF_EVENTS_SEGMENT) consecutive
// slabs.  -> the run of plane p in by_plane, [*first, *first + *count), from plane_start clamped to [0, K]; a run that ends
// before it begins is empty.
__device__ __forceinline__ void plane_run(const int *__restrict__ plane_start, int p, int K, int *first, int *count) {
    if (K <= 0) {   // (no events: plane_start is not read)
        *first = *count = 0;
        return;
    }
    const int a = min(max(plane_start[p], 0), K), b = min(max(plane_start[p + 1], 0), K);
    *first = a;
    *count = max(b - a, 0);
}

template <typename T>
__global__ __launch_bounds__(kEventThreads) void k_events_grad_W(EventGeo g, int mode, int Sy, int Sx,
                                                                  const int4 *__restrict__ ev,
                                                                  const int *__restrict__ by_plane,
                                                                  const int *__restrict__ plane_start,
                                                                  const T *__restrict__ h, int K,
                                                                  const T *__restrict__ V, const T *__restrict__ R,
                                                                  double *__restrict__ slabs) {
    __shared__ int4 s_q[TNMF_EVENTS_SEGMENT];      // (qy0, qy1, qx0, qx1): the padded positions of the images per axis
    __shared__ int s_n[TNMF_EVENTS_SEGMENT];       // the sample; -1 for a row to skip
    __shared__ int s_cnt[TNMF_EVENTS_SEGMENT];     // images per axis: ny | nx << 2
    __shared__ double s_h[TNMF_EVENTS_SEGMENT];
    __shared__ double s_part[2][kEventThreads];    // the partial sums of the sub-lanes
    // which plane, which of its segments (the same walk in every thread: scalar loads of a few cached ints)
    const int slab = blockIdx.x;
    int plane = -1, first = 0, count = 0;
    long long acc = 0;   // (64 bits: overlapping runs of a plane_start outside the contract may add up beyond K)
    for (int p = 0; p < g.P; ++p) {
        int a, c;
        plane_run(plane_start, p, K, &a, &c);
        const int ns = (c + TNMF_EVENTS_SEGMENT - 1) / TNMF_EVENTS_SEGMENT;
        if (slab < acc + ns) {
            plane = p;
            first = a + (int)(slab - acc) * TNMF_EVENTS_SEGMENT;
            count = min(TNMF_EVENTS_SEGMENT, a + c - first);
            break;
        }
        acc += ns;
    }
    if (plane < 0) return;   // (workgroup-uniform: a slab beyond the last segment)
    for (int i = threadIdx.x; i < count; i += kEventThreads) {
        const int e = by_plane[first + i];
        int n = -1, cnt = 0;
        int4 q = make_int4(0, 0, 0, 0);
        double hv = 0.;
        if ((unsigned)e < (unsigned)K) {
            const int4 v = ev[e];   // sample, plane, uy, ux
            if ((unsigned)v.x < (unsigned)g.N && v.y == plane && (unsigned)v.z < (unsigned)Sy &&
                (unsigned)v.w < (unsigned)Sx) {
                int qy[2] = {0, 0}, qx[2] = {0, 0};
                const int ny = axis_images(mode, v.z, g.Ay, Sy, qy), nx = axis_images(mode, v.w, g.Ax, Sx, qx);
                n = v.x, cnt = ny | nx << 2, q = make_int4(qy[0], qy[1], qx[0], qx[1]);
                hv = (double)h[e];
            }
        }
        s_n[i] = n, s_cnt[i] = cnt, s_q[i] = q, s_h[i] = hv;
    }
    __syncthreads();
    const int AA = g.Ay * g.Ax, taps = g.C * AA;
    const int L = max(1, kEventThreads / taps);   // sub-lanes per tap
    const size_t plane_size = (size_t)g.Dy * g.Dx;
    double *out = slabs + (size_t)slab * 2 * taps;
    for (int t0 = 0; t0 < taps; t0 += kEventThreads) {
        const int sub = L > 1 ? (int)threadIdx.x / taps : 0;
        const int t = L > 1 ? (int)threadIdx.x - sub * taps : t0 + (int)threadIdx.x;
        const bool active = t < taps && sub < L;
        double neg = 0., pos = 0.;
        if (active) {
            const int c = t / AA, r = t - c * AA;
            const int jy = r / g.Ax, jx = r - jy * g.Ax;
            for (int i = sub; i < count; i += L) {
                const int n = s_n[i];
                if (n < 0) continue;
                const int4 q = s_q[i];
                const int cnt = s_cnt[i], ny = cnt & 3, nx = cnt >> 2;
                const double hv = s_h[i];
                const size_t base = ((size_t)n * g.C + c) * plane_size;
                double a = 0., b = 0.;
                for (int iy = 0; iy < ny; ++iy) {
                    const int y = (iy ? q.y : q.x) - (g.Ay - 1) + jy;
                    for (int ix = 0; ix < nx; ++ix) {
                        const int x = (ix ? q.w : q.z) - (g.Ax - 1) + jx;
                        if ((unsigned)y < (unsigned)g.Dy && (unsigned)x < (unsigned)g.Dx) {
                            const size_t at = base + (size_t)y * g.Dx + x;
                            a += (double)V[at];
                            b += (double)R[at];
                        }
                    }
                }
                neg += hv * a;
                pos += hv * b;
            }
        }
        if (L > 1) {   // (taps < 256: one pass, t0 == 0)
            s_part[0][threadIdx.x] = neg, s_part[1][threadIdx.x] = pos;
            __syncthreads();
            if (active && sub == 0) {
                for (int s = 1; s < L; ++s) neg += s_part[0][s * taps + t], pos += s_part[1][s * taps + t];
            }
        }
        if (active && sub == 0) out[t] = neg, out[taps + t] = pos;
    }
}

// negpos[2, P, taps] = per plane the sum of its slabs in segment order, rounded once; one thread per (plane, tap)
template <typename T>
__global__ __launch_bounds__(kEventThreads) void k_events_grad_W_sum(int P, int taps, const int *__restrict__ plane_start,
                                                                      int K, long long n_slabs,
                                                                      const double *__restrict__ slabs,
                                                                      T *__restrict__ negpos) {
    const int chunks = (taps + kEventThreads - 1) / kEventThreads;
    const int p = blockIdx.x / chunks, t = (blockIdx.x - p * chunks) * kEventThreads + threadIdx.x;
    if (t >= taps) return;
    long long s0 = 0;
    int a, c;
    for (int pp = 0; pp < p; ++pp) {
        plane_run(plane_start, pp, K, &a, &c);
        s0 += (c + TNMF_EVENTS_SEGMENT - 1) / TNMF_EVENTS_SEGMENT;
    }
    plane_run(plane_start, p, K, &a, &c);
    const long long s1 = std::min<long long>(s0 + (c + TNMF_EVENTS_SEGMENT - 1) / TNMF_EVENTS_SEGMENT, n_slabs);
    double neg = 0., pos = 0.;
    for (long long s = s0; s < s1; ++s) {
        const double *slab = slabs + (size_t)s * 2 * taps;
        neg += slab[t];
        pos += slab[taps + t];
    }
    negpos[(size_t)p * taps + t] = (T)neg;
    negpos[((size_t)P + p) * taps + t] = (T)pos;
}

}  // namespace

int events_render(tnmf_hip_ctx *ctx, const EventGeo &g, int dtype, const void *W, const int *images, long long n_images,
                  const int *cell_start, const void *strength, long long n_events, void *R, hipStream_t s) {
    if (g.N <= 0) return TNMF_OK;
    int tx_log = 0;
    while ((1 << tx_log) < g.tx) ++tx_log;
    const int nty = cdiv(g.Dy, g.ty), ntx = cdiv(g.Dx, g.tx);
    const unsigned grid = events_grid(ctx, (long long)g.N * nty * ntx);
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_events_render<T>, dim3(grid), dim3(kEventThreads), 0, s, g, tx_log, nty, ntx, (const T *)W,
                           (const int4 *)images, (int)n_images, cell_start, (const T *)strength, (int)n_events, (T *)R);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

int events_update(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const void *W, const int *events, void *strength,
                  long long n_events, const void *V, const void *R, double reg, hipStream_t s) {
    if (n_events <= 0 || f.g.N <= 0) return TNMF_OK;
    const unsigned grid = events_grid(ctx, (n_events + kWaves - 1) / kWaves);
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_events_update<T>, dim3(grid), dim3(kEventThreads), 0, s, f.g, f.mode, f.Sy, f.Sx, (const T *)W,
                           (const int4 *)events, (T *)strength, n_events, (const T *)V, (const T *)R, reg);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

int events_gain(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const void *W, const int *events, const void *strength,
                long long n_events, const void *V, const void *R, double *gain, double *mag, hipStream_t s) {
    if (n_events <= 0 || f.g.N <= 0) return TNMF_OK;
    const unsigned grid = events_grid(ctx, (n_events + kWaves - 1) / kWaves);
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_events_gain<T>, dim3(grid), dim3(kEventThreads), 0, s, f.g, f.mode, f.Sy, f.Sx, (const T *)W,
                           (const int4 *)events, (const T *)strength, n_events, (const T *)V, (const T *)R, gain, mag);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

long long events_grad_W_slabs(long long n_events, int P) { return n_events / TNMF_EVENTS_SEGMENT + P; }

int events_grad_W(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const int *events, const int *by_plane,
                  const int *plane_start, const void *strength, long long n_events, const void *V, const void *R,
                  void *workspace, void *negpos, hipStream_t s) {
    const EventGeo &g = f.g;
    const int taps = g.C * g.Ay * g.Ax;
    const long long n_slabs = events_grad_W_slabs(n_events, g.P);
    if (n_events > 0 && g.N > 0) {
        with_dtype(dtype, [&](auto zero) {
            using T = decltype(zero);
            hipLaunchKernelGGL(k_events_grad_W<T>, dim3((unsigned)n_slabs), dim3(kEventThreads), 0, s, g, f.mode, f.Sy, f.Sx,
                               (const int4 *)events, by_plane, plane_start, (const T *)strength, (int)n_events,
                               (const T *)V, (const T *)R, (double *)workspace);
        });
        TNMF_LAUNCH_CHECK();
    }
    // (without events or samples no slab exists: K = 0 makes every run empty, whatever plane_start holds)
    const int K = g.N > 0 ? (int)n_events : 0;
    const dim3 grid((unsigned)((long long)cdiv(taps, kEventThreads) * g.P));
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_events_grad_W_sum<T>, grid, dim3(kEventThreads), 0, s, g.P, taps, plane_start, K, n_slabs,
                           (const double *)workspace, (T *)negpos);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}
