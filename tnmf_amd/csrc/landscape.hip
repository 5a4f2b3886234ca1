// landscape.hip -- the local gain landscape of a list of events (include/tnmf_hip.h, "landscape"): for every row e and every
// neighbour shift u' = u + delta, delta in {-1, 0, +1}^ndim, the sums of tnmf_hip_pursuit_pick against the residual of the
// list WITHOUT the row, d_e = V - R + h_e * phi_e:  a = <phi', d_e>, b = |phi'|^2 and mag = sum |w d_e|, phi' the occurrence
// of the row's plane at u' (event_walk.h: all images, clipped to the sample, images that overlap added).
//
// k_events_landscape: one wave per row, two paths, chosen by the geometry of the row alone (landscape_staged):
//   walk    every neighbour in turn through for_each_tap, lanes striding over its taps; d_e at a pixel is residual_without()
//           of V, R and phi_at of the CENTRE occurrence.  Border, wrapped, mirrored and clipped rows, and rows with a
//           neighbour outside the shift shape (which gets zeros), go here.
//   staged  where the row and all its 3^ndim neighbours are single images wholly inside the sample: the wave writes the
//           (A + 2)-sized patch of d_e per channel into its slice of LDS once -- V and R are read once, not 3^ndim times --
//           and every neighbour takes its taps from the patch.  b is the plane's sum of squares, taken once.
// Both paths add the same terms to the same lane in the same order -- tap t goes to lane t % 64, ascending t, then the
// butterfly of wave_sum, taken of all the sums of a row at once (wave_sum_many: the same bits, a fifth of the exchanges) --
// and build each term with the same spelled-out operations (residual_without, fma), so a row gives the same bits on either
// path; the patch holds doubles for that reason.  No atomics, no workspace.  A wave's LDS slice is its own: the LDS
// operations of one wave complete in order, so a fence and a wave barrier separate staging from use.
#include <algorithm>

#include "event_walk.h"

namespace {

constexpr int kWaves = kEventThreads / 64;
constexpr int kPatchMax = 2048;   // doubles of LDS per wave the staged path may use: 16 KiB, 64 KiB per workgroup
#ifndef TNMF_LANDSCAPE_BLOCKS_PER_CU
#define TNMF_LANDSCAPE_BLOCKS_PER_CU 4   // the grid: at most this many workgroups per CU, each wave looping over its rows
#endif

// the rule of the staged path: geometry only.  ry = 1 with two shift axes, 0 with one (no neighbours on the leading axis).
__device__ __forceinline__ bool landscape_staged(const EventGeo &g, int mode, int Sy, int Sx, int ry, int uy, int ux,
                                                 int patch) {
    if (patch <= 0) return false;   // (the patch of this geometry does not fit: every row walks)
    for (int d = -ry; d <= ry; ++d)
        if (!axis_whole(mode, uy + d, g.Ay, Sy, g.Dy)) return false;
    for (int d = -1; d <= 1; ++d)
        if (!axis_whole(mode, ux + d, g.Ax, Sx, g.Dx)) return false;
    return true;
}

template <typename T>
__global__ __launch_bounds__(kEventThreads) void k_events_landscape(EventGeo g, int mode, int Sy, int Sx, int ry, int patch,
                                                                     const T *__restrict__ W, const int4 *__restrict__ ev,
                                                                     const T *__restrict__ h, long long n_events,
                                                                     const T *__restrict__ V, const T *__restrict__ R,
                                                                     double *__restrict__ a_out, double *__restrict__ b_out,
                                                                     double *__restrict__ mag_out) {
    extern __shared__ double s_patch[];   // kWaves slices of `patch` doubles
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int AA = g.Ay * g.Ax, taps = g.C * AA;
    const int nb = ry ? 9 : 3;
    const unsigned uAA = AA, uAx = g.Ax;
    double *mine = s_patch + (size_t)wave * patch;
    for (long long e = (long long)blockIdx.x * kWaves + wave; e < n_events; e += (long long)gridDim.x * kWaves) {
        const int4 v = ev[e];   // sample, plane, uy, ux
        double *ao = a_out + e * nb, *bo = b_out + e * nb, *mo = mag_out ? mag_out + e * nb : nullptr;
        if ((unsigned)v.x >= (unsigned)g.N || (unsigned)v.y >= (unsigned)g.P || (unsigned)v.z >= (unsigned)Sy ||
            (unsigned)v.w >= (unsigned)Sx) {   // (wave-uniform: outside the contract, no sample data is read)
            if (lane < nb) {
                ao[lane] = 0., bo[lane] = 0.;
                if (mo) mo[lane] = 0.;
            }
            continue;
        }
        const T *w = W + (size_t)v.y * taps;
        const size_t sample = (size_t)v.x * g.C * g.Dy * g.Dx;
        const double hv = (double)h[e];
        if (landscape_staged(g, mode, Sy, Sx, ry, v.z, v.w, patch)) {   // (wave-uniform)
            // the patch: rows oy - ry .. oy + Ay - 1 + ry, columns ox - 1 .. ox + Ax, all inside the sample by the rule
            const int oy = (mode == TNMF_MODE_VALID ? v.z - (g.Ay - 1) : v.z) - ry;
            const int ox = (mode == TNMF_MODE_VALID ? v.w - (g.Ax - 1) : v.w) - 1;
            const int Py = g.Ay + 2 * ry, Px = g.Ax + 2;
            const unsigned uPP = Py * Px, uPx = Px;
            const int cells = g.C * Py * Px;   // (<= patch)
            for (int i = lane; i < cells; i += 64) {
                const int c = i / uPP, r = i - c * (int)uPP;
                const int py = r / uPx, px = r - py * Px;
                const int jy = py - ry, jx = px - 1;   // the tap of the row itself on this pixel, if any
                const bool on = (unsigned)jy < (unsigned)g.Ay && (unsigned)jx < (unsigned)g.Ax;
                const double phi = on ? (double)w[c * AA + jy * g.Ax + jx] : 0.;
                const size_t at = sample + ((size_t)c * g.Dy + (oy + py)) * g.Dx + (ox + px);
                mine[i] = residual_without(V[at], R[at], hv, phi);
            }
            double b = 0.;
            for (int t = lane; t < taps; t += 64) {
                const double wv = (double)w[t];
                b = fma(wv, wv, b);
            }
            b = wave_sum(b);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            // every tap once: its 3^ndim neighbours in the patch, each into its own pair of sums (registers: the loops over
            // the neighbours are unrolled) -- per neighbour and lane the taps still arrive in ascending t
            if (ry) {
                double am[18];   // a of the 9 neighbours, then mag
#pragma unroll
                for (int k = 0; k < 18; ++k) am[k] = 0.;
                for (int t = lane; t < taps; t += 64) {
                    const int c = t / uAA, r = t - c * AA;
                    const int jy = r / uAx, jx = r - jy * g.Ax;
                    const double wv = (double)w[t];
                    const double *at = mine + c * (int)uPP + (jy + 1) * Px + (jx + 1);
#pragma unroll
                    for (int k = 0; k < 9; ++k) {
                        const double d = at[(k / 3 - 1) * Px + (k % 3 - 1)];
                        am[k] = fma(wv, d, am[k]);
                        am[9 + k] += fabs(wv * d);
                    }
                }
                int k;
                if (wave_sum_many(am, lane, &k)) {
                    if (k < 9)
                        ao[k] = am[0], bo[k] = b;
                    else if (mo)
                        mo[k - 9] = am[0];
                }
            } else {
                double am[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) am[k] = 0.;
                for (int t = lane; t < taps; t += 64) {
                    const int c = t / uAx, jx = t - c * g.Ax;   // (Ay == 1)
                    const double wv = (double)w[t];
                    const double *at = mine + c * Px + (jx + 1);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double d = at[k - 1];
                        am[k] = fma(wv, d, am[k]);
                        am[3 + k] += fabs(wv * d);
                    }
                }
                int k;
                if (wave_sum_many(am, lane, &k)) {
                    if (k < 3)
                        ao[k] = am[0], bo[k] = b;
                    else if (mo)
                        mo[k - 3] = am[0];
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // (the patch is read before the next row overwrites it)
            __builtin_amdgcn_wave_barrier();
            continue;
        }
        const Occurrence centre(g, mode, Sy, Sx, v.z, v.w);
        for (int k = 0; k < nb; ++k) {
            const int uy = v.z + (ry ? k / 3 - 1 : 0), ux = v.w + k - (ry ? k / 3 * 3 : 0) - 1;
            double a = 0., b = 0., m = 0.;
            if ((unsigned)uy < (unsigned)Sy && (unsigned)ux < (unsigned)Sx) {   // (wave-uniform; else zeros)
                const Occurrence o(g, mode, Sy, Sx, uy, ux);
                const bool single = o.single();
                for_each_tap(g, o, lane, 64, [&](int t, int c, int y, int x) {
                    const size_t at = sample + ((size_t)c * g.Dy + y) * g.Dx + x;
                    const double wv = (double)w[t];
                    const double phi = single ? wv : phi_at(g, o, w, c * AA, y, x);
                    const double d = residual_without(V[at], R[at], hv, phi_at(g, centre, w, c * AA, y, x));
                    a = fma(wv, d, a);
                    b = fma(wv, phi, b);
                    m += fabs(wv * d);
                });
            }
            double abm[3] = {a, b, m};   // (zeros for a neighbour outside the shift shape)
            int which;
            if (wave_sum_many(abm, lane, &which)) {
                if (which == 0)
                    ao[k] = abm[0];
                else if (which == 1)
                    bo[k] = abm[0];
                else if (mo)
                    mo[k] = abm[0];
            }
        }
    }
}

}  // namespace

int events_landscape(tnmf_hip_ctx *ctx, const EventFrame &f, int ndim, int dtype, const void *W, const int *events,
                     const void *strength, long long n_events, const void *V, const void *R, double *a, double *b,
                     double *mag, hipStream_t s) {
    const EventGeo &g = f.g;
    if (n_events <= 0 || g.N <= 0) return TNMF_OK;
    const int ry = ndim == 2 ? 1 : 0;
    const long long cells = (long long)g.C * (g.Ay + 2 * ry) * (g.Ax + 2);
#ifdef TNMF_LANDSCAPE_WALK_ONLY   // (an A/B build for tools/probes/landscape_bench.py: every row walks)
    const bool stage = false;
#else
    const bool stage = true;
#endif
    const int patch = stage && cells <= kPatchMax ? (int)cells : 0;
    const size_t lds = (size_t)kWaves * patch * sizeof(double);
    const unsigned grid = events_grid(ctx, (n_events + kWaves - 1) / kWaves, TNMF_LANDSCAPE_BLOCKS_PER_CU);
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_events_landscape<T>, dim3(grid), dim3(kEventThreads), lds, s, g, f.mode, f.Sy, f.Sx, ry, patch,
                           (const T *)W, (const int4 *)events, (const T *)strength, n_events, (const T *)V, (const T *)R, a,
                           b, mag);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}
