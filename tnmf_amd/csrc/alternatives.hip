// alternatives.hip -- every event of a list scored under other planes at its own shift (include/tnmf_hip.h, "alternatives"):
// the landscape turned by 90 degrees.  For every row e = (n, p, u, h_e) and every plane p'_j of an arithmetic progression
// through p -- p'_j = first + j * stride, first = (p / block) * block + p % stride, block = n_alt * stride -- the sums of
// tnmf_hip_events_landscape at delta = 0 with the taps of p'_j, against the residual of the list WITHOUT the row,
// d_e = V - R + h_e * phi_e:  a = <phi', d_e>, b = |phi'|^2 and mag = sum |w' d_e|, phi' the occurrence of plane p'_j at u
// (event_walk.h: all images, clipped to the sample, images that overlap added).
//
// k_events_alternatives: one wave per row, two paths, chosen by the geometry of the row alone (alternatives_staged):
//   staged  where the row's occurrence is a single image wholly inside the sample: the wave writes the C x Ay x Ax patch of
//           d_e into its slice of LDS once -- V and R are read once per row, not n_alt times -- and every candidate plane
//           takes its taps from the patch: tap t meets cell t.  b is the plane's sum of squares in the same lane order.
//   walk    every other row -- clipped, wrapped or mirrored, or a patch that does not fit: one Occurrence per row, every
//           tap of every image through for_each_tap, d_e at its pixel from residual_without() of V, R and phi_at of the
//           row's OWN plane, then phi' = phi_at of each candidate plane.
// The candidates are taken kBatch at a time: per tap one d_e and kBatch multiply-adds, and the 3 * kBatch sums of a batch
// reduced together (wave_sum_many).  Both paths add the same terms to the same lane in the same order -- tap t goes to lane
// t % 64, ascending t, images in image order, then the butterfly of wave_sum -- and build each term with the same
// spelled-out operations (residual_without, fma), so a row gives the same bits on either path; the patch holds doubles for
// that reason.  No atomics, no workspace.  A wave's LDS slice is its own: the LDS operations of one wave complete in
// order, so a fence and a wave barrier separate staging from use.
#include <algorithm>

#include "event_walk.h"

namespace {

constexpr int kWaves = kEventThreads / 64;
constexpr int kPatchMax = 2048;   // doubles of LDS per wave the staged path may use: 16 KiB, 64 KiB per workgroup
constexpr int kBatch = 4;         // candidate planes per pass over the taps: 12 sums in registers
#ifndef TNMF_ALTERNATIVES_BLOCKS_PER_CU
#define TNMF_ALTERNATIVES_BLOCKS_PER_CU 4   // the grid: at most this many workgroups per CU, each wave looping over its rows
#endif

// the rule of the staged path: geometry only
__device__ __forceinline__ bool alternatives_staged(const EventGeo &g, int mode, int Sy, int Sx, int uy, int ux, int patch) {
    if (patch <= 0) return false;   // (the patch of this geometry does not fit: every row walks)
    return axis_whole(mode, uy, g.Ay, Sy, g.Dy) && axis_whole(mode, ux, g.Ax, Sx, g.Dx);
}

// the sums of a batch reduced together and stored: a of the kBatch planes, then b, then mag; `live` of them exist
__device__ __forceinline__ void store_batch(double (&abm)[3 * kBatch], int lane, int live, double *ao, double *bo, double *mo) {
    int k;
    if (wave_sum_many(abm, lane, &k)) {
        const int j = k % kBatch;
        if (j < live) {
            if (k < kBatch)
                ao[j] = abm[0];
            else if (k < 2 * kBatch)
                bo[j] = abm[0];
            else if (mo)
                mo[j] = abm[0];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kEventThreads) void k_events_alternatives(EventGeo g, int mode, int Sy, int Sx, int patch,
                                                                        int n_alt, int stride, const T *__restrict__ W,
                                                                        const int4 *__restrict__ ev,
                                                                        const T *__restrict__ h, long long n_events,
                                                                        const T *__restrict__ V, const T *__restrict__ R,
                                                                        double *__restrict__ a_out,
                                                                        double *__restrict__ b_out,
                                                                        double *__restrict__ mag_out) {
    extern __shared__ double s_patch[];   // kWaves slices of `patch` doubles
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int AA = g.Ay * g.Ax, taps = g.C * AA;
    const int block = n_alt * stride;   // (divides P: every candidate is a plane)
    double *mine = s_patch + (size_t)wave * patch;
    for (long long e = (long long)blockIdx.x * kWaves + wave; e < n_events; e += (long long)gridDim.x * kWaves) {
        const int4 v = ev[e];   // sample, plane, uy, ux
        double *ao = a_out + e * n_alt, *bo = b_out + e * n_alt, *mo = mag_out ? mag_out + e * n_alt : nullptr;
        if ((unsigned)v.x >= (unsigned)g.N || (unsigned)v.y >= (unsigned)g.P || (unsigned)v.z >= (unsigned)Sy ||
            (unsigned)v.w >= (unsigned)Sx) {   // (wave-uniform: outside the contract, no sample data is read)
            for (int j = lane; j < n_alt; j += 64) {
                ao[j] = 0., bo[j] = 0.;
                if (mo) mo[j] = 0.;
            }
            continue;
        }
        const T *w = W + (size_t)v.y * taps;                                          // the row's own plane
        const T *w0 = W + (size_t)(v.y / block * block + v.y % stride) * taps;        // the first candidate
        const size_t hop = (size_t)stride * taps;                                     // from one candidate to the next
        const size_t sample = (size_t)v.x * g.C * g.Dy * g.Dx;
        const double hv = (double)h[e];
        if (alternatives_staged(g, mode, Sy, Sx, v.z, v.w, patch)) {   // (wave-uniform)
            // the patch: the pixels oy .. oy + Ay - 1, ox .. ox + Ax - 1 of every channel, all inside the sample by the rule;
            // cell t is the pixel under tap t
            const int oy = mode == TNMF_MODE_VALID ? v.z - (g.Ay - 1) : v.z;
            const int ox = mode == TNMF_MODE_VALID ? v.w - (g.Ax - 1) : v.w;
            const unsigned uAA = AA, uAx = g.Ax;
            for (int t = lane; t < taps; t += 64) {
                const int c = t / uAA, r = t - c * AA;
                const int jy = r / uAx, jx = r - jy * g.Ax;
                const size_t at = sample + ((size_t)c * g.Dy + (oy + jy)) * g.Dx + (ox + jx);
                mine[t] = residual_without(V[at], R[at], hv, (double)w[t]);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            for (int j0 = 0; j0 < n_alt; j0 += kBatch) {
                const int live = min(kBatch, n_alt - j0);   // (wave-uniform)
                const T *wb = w0 + (size_t)j0 * hop;
                double abm[3 * kBatch];
#pragma unroll
                for (int k = 0; k < 3 * kBatch; ++k) abm[k] = 0.;
                for (int t = lane; t < taps; t += 64) {
                    const double d = mine[t];
#pragma unroll
                    for (int k = 0; k < kBatch; ++k) {
                        const double wv = k < live ? (double)wb[k * hop + t] : 0.;
                        abm[k] = fma(wv, d, abm[k]);
                        abm[kBatch + k] = fma(wv, wv, abm[kBatch + k]);
                        abm[2 * kBatch + k] += fabs(wv * d);
                    }
                }
                store_batch(abm, lane, live, ao + j0, bo + j0, mo ? mo + j0 : nullptr);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // (the patch is read before the next row overwrites it)
            __builtin_amdgcn_wave_barrier();
            continue;
        }
        const Occurrence o(g, mode, Sy, Sx, v.z, v.w);
        const bool single = o.single();
        for (int j0 = 0; j0 < n_alt; j0 += kBatch) {
            const int live = min(kBatch, n_alt - j0);
            const T *wb = w0 + (size_t)j0 * hop;
            double abm[3 * kBatch];
#pragma unroll
            for (int k = 0; k < 3 * kBatch; ++k) abm[k] = 0.;
            for_each_tap(g, o, lane, 64, [&](int t, int c, int y, int x) {
                const size_t at = sample + ((size_t)c * g.Dy + y) * g.Dx + x;
                const double d = residual_without(V[at], R[at], hv, phi_at(g, o, w, c * AA, y, x));
#pragma unroll
                for (int k = 0; k < kBatch; ++k) {
                    double wv = 0., phi = 0.;
                    if (k < live) {
                        wv = (double)wb[k * hop + t];
                        phi = single ? wv : phi_at(g, o, wb + k * hop, c * AA, y, x);
                    }
                    abm[k] = fma(wv, d, abm[k]);
                    abm[kBatch + k] = fma(wv, phi, abm[kBatch + k]);
                    abm[2 * kBatch + k] += fabs(wv * d);
                }
            });
            store_batch(abm, lane, live, ao + j0, bo + j0, mo ? mo + j0 : nullptr);
        }
    }
}

}  // namespace

int events_alternatives(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const void *W, const int *events,
                        const void *strength, long long n_events, const void *V, const void *R, int n_alt, int stride,
                        double *a, double *b, double *mag, hipStream_t s) {
    const EventGeo &g = f.g;
    if (n_events <= 0 || g.N <= 0) return TNMF_OK;
    const long long cells = (long long)g.C * g.Ay * g.Ax;
#ifdef TNMF_ALTERNATIVES_WALK_ONLY   // (an A/B build for tools/probes/alternatives_bench.py: every row walks)
    const bool stage = false;
#else
    const bool stage = true;
#endif
    const int patch = stage && cells <= kPatchMax ? (int)cells : 0;
    const size_t lds = (size_t)kWaves * patch * sizeof(double);
    const unsigned grid = events_grid(ctx, (n_events + kWaves - 1) / kWaves, TNMF_ALTERNATIVES_BLOCKS_PER_CU);
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_events_alternatives<T>, dim3(grid), dim3(kEventThreads), lds, s, g, f.mode, f.Sy, f.Sx, patch,
                           n_alt, stride, (const T *)W, (const int4 *)events, (const T *)strength, n_events, (const T *)V,
                           (const T *)R, a, b, mag);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}
