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
// k_events_update: one wave per event.  The images are derived from the event itself (the table of the header); the lanes
// stride over the C * Ay * Ax atom entries, gather V and R under each image, clipped per pixel, into double partial sums,
// reduce them with a butterfly of fixed order and lane 0 applies the multiplicative update to the strength in place.  It
// writes the K strengths and nothing else.
#include <algorithm>

#include "events.h"

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

// the images of the shift u on one axis (atom extent a, shift extent S): their padded positions, at most two
__device__ __forceinline__ int axis_images(int mode, int u, int a, int S, int q[2]) {
    if (mode == TNMF_MODE_VALID) {
        q[0] = u;
        return 1;
    }
    q[0] = u + a - 1;
    if (mode == TNMF_MODE_CIRCULAR && u >= S - (a - 1)) {
        q[1] = u - (S - (a - 1));
        return 2;
    }
    if (mode == TNMF_MODE_REFLECT && u >= 1 && u <= a - 1) {
        q[1] = (a - 1) - u;
        return 2;
    }
    return 1;
}

template <typename T>
__global__ __launch_bounds__(kEventThreads) void k_events_update(EventGeo g, int mode, int Sy, int Sx,
                                                                  const T *__restrict__ W, const int4 *__restrict__ ev,
                                                                  T *h, long long n_events, const T *__restrict__ V,
                                                                  const T *__restrict__ R, double reg) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int AA = g.Ay * g.Ax, taps = g.C * AA;
    for (long long e = (long long)blockIdx.x * kWaves + wave; e < n_events; e += (long long)gridDim.x * kWaves) {
        const int4 v = ev[e];   // sample, plane, uy, ux
        if ((unsigned)v.x >= (unsigned)g.N || (unsigned)v.y >= (unsigned)g.P || (unsigned)v.z >= (unsigned)Sy ||
            (unsigned)v.w >= (unsigned)Sx)
            continue;   // (wave-uniform: outside the contract, neither read nor written)
        int qy[2], qx[2];
        const int ny = axis_images(mode, v.z, g.Ay, Sy, qy), nx = axis_images(mode, v.w, g.Ax, Sx, qx);
        const T *w = W + (size_t)v.y * taps;
        const size_t sample = (size_t)v.x * g.C * g.Dy * g.Dx;
        double neg = 0., pos = 0.;
        for (int iy = 0; iy < ny; ++iy) {
            for (int ix = 0; ix < nx; ++ix) {
                const int oy = qy[iy] - (g.Ay - 1), ox = qx[ix] - (g.Ax - 1);
                for (int t = lane; t < taps; t += 64) {
                    const int c = t / AA, r = t - c * AA;
                    const int jy = r / g.Ax, jx = r - jy * g.Ax;
                    const int y = oy + jy, x = ox + jx;
                    if ((unsigned)y < (unsigned)g.Dy && (unsigned)x < (unsigned)g.Dx) {
                        const size_t at = sample + ((size_t)c * g.Dy + y) * g.Dx + x;
                        const double wv = (double)w[t];
                        neg += wv * (double)V[at];
                        pos += wv * (double)R[at];
                    }
                }
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {   // a butterfly: the same order of additions in every lane and run
            neg += __shfl_xor(neg, off, 64);
            pos += __shfl_xor(pos, off, 64);
        }
        if (lane == 0) h[e] = (T)((double)h[e] * neg / (pos + reg));
    }
}

unsigned grid_for(const tnmf_hip_ctx *ctx, long long blocks) {
    return (unsigned)std::max<long long>(1, std::min<long long>(blocks, (long long)ctx->num_cu * 64));
}

}  // namespace

int events_render(tnmf_hip_ctx *ctx, const EventGeo &g, int dtype, const void *W, const int *images, long long n_images,
                  const int *cell_start, const void *strength, long long n_events, void *R, hipStream_t s) {
    if (g.N <= 0) return TNMF_OK;
    int tx_log = 0;
    while ((1 << tx_log) < g.tx) ++tx_log;
    const int nty = cdiv(g.Dy, g.ty), ntx = cdiv(g.Dx, g.tx);
    const unsigned grid = grid_for(ctx, (long long)g.N * nty * ntx);
    if (dtype == 0)
        hipLaunchKernelGGL(k_events_render<float>, dim3(grid), dim3(kEventThreads), 0, s, g, tx_log, nty, ntx,
                           (const float *)W, (const int4 *)images, (int)n_images, cell_start, (const float *)strength,
                           (int)n_events, (float *)R);
    else
        hipLaunchKernelGGL(k_events_render<double>, dim3(grid), dim3(kEventThreads), 0, s, g, tx_log, nty, ntx,
                           (const double *)W, (const int4 *)images, (int)n_images, cell_start, (const double *)strength,
                           (int)n_events, (double *)R);
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

int events_update(tnmf_hip_ctx *ctx, const EventGeo &g, int dtype, int mode, int Sy, int Sx, const void *W,
                  const int *events, void *strength, long long n_events, const void *V, const void *R, double reg,
                  hipStream_t s) {
    if (n_events <= 0 || g.N <= 0) return TNMF_OK;
    const unsigned grid = grid_for(ctx, (n_events + kWaves - 1) / kWaves);
    if (dtype == 0)
        hipLaunchKernelGGL(k_events_update<float>, dim3(grid), dim3(kEventThreads), 0, s, g, mode, Sy, Sx,
                           (const float *)W, (const int4 *)events, (float *)strength, n_events, (const float *)V,
                           (const float *)R, reg);
    else
        hipLaunchKernelGGL(k_events_update<double>, dim3(grid), dim3(kEventThreads), 0, s, g, mode, Sy, Sx,
                           (const double *)W, (const int4 *)events, (double *)strength, n_events, (const double *)V,
                           (const double *)R, reg);
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}
