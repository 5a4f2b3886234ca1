// pursuit.hip -- forward selection of events (include/tnmf_hip.h, "pursuit"): the table of norms, the gain map of a round
// and the exact score of the candidates a round keeps.  The correlation that feeds the map is the H gradient's; the render
// and the refit of the list are those of events.hip, the occurrence of a shift and the walk over its taps those of
// event_walk.h.
//
// k_events_norms: b[p, u] = |phi_{p,u}|^2 for every plane and shift, in double.  grid.y is the plane; every workgroup first
// sums the squares of its plane's taps (256 partial sums in tap order, then a tree of fixed shape through LDS), which IS the
// norm of every shift whose single image lies wholly inside the sample.  Any other shift -- clipped by the border, wrapped
// or mirrored -- goes through the walk of k_events_gain in one thread (for_each_tap from tap 0 in steps of 1): the taps in
// (image, channel, row, column) order, phi at a pixel summed over the images that cover it (phi_at).  A plane has
// O(perimeter * atom) such shifts.
//
// k_pursuit_score: g = a^2 / (2 b) where a > 0 and b > 0, else 0 -- a streaming pass over the map, rows `Hs` apart.  A
// thread owns 16 bytes of a row (four floats, two doubles) and walks the map with a grid stride; it derives (row, column)
// once and advances them by the stride's quotient and remainder, so the loop holds no division.  Where the rows start on
// 16-byte boundaries (base pointers and row stride) a whole chunk is one 16-byte load and one 16-byte store; the chunk
// that holds the end of a row, and every chunk of an unaligned map, goes element by element.  A C-contiguous map is taken
// as one row per sample, as long as the table, so its alignment does not depend on the shift width.  Pad columns are
// neither read nor written.  b is read through the cache: P planes of doubles against N * P planes of the map.  k_pursuit_taken then
// zeroes the entries already in the list, on the same stream.
//
// k_pursuit_pick: one wave per picked flat index, the walk of k_events_gain against the residual V - R: a = <phi, V - R>,
// b = |phi|^2 and the magnitude sum |w (V - R)|, in double with the same butterfly (wave_sum); lane 0 writes the event's row,
// the strength max(a, 0) / b that minimises the energy along phi, rounded once, and the gain a^2 / (2 b) of adding it.
#include <algorithm>

#include "event_walk.h"

namespace {

constexpr int kWaves = kEventThreads / 64;

template <typename T>
__global__ __launch_bounds__(kEventThreads) void k_events_norms(EventGeo g, int mode, int Sy, int Sx,
                                                                 const T *__restrict__ W, double *__restrict__ b) {
    __shared__ double s_part[kEventThreads];
    const int p = blockIdx.y;
    const int AA = g.Ay * g.Ax, taps = g.C * AA;
    const T *w = W + (size_t)p * taps;
    double sq = 0.;
    for (int t = threadIdx.x; t < taps; t += kEventThreads) sq += (double)w[t] * (double)w[t];
    s_part[threadIdx.x] = sq;
    __syncthreads();
    for (int off = kEventThreads / 2; off >= 1; off >>= 1) {   // a tree of fixed shape: the same bits in every workgroup
        if ((int)threadIdx.x < off) s_part[threadIdx.x] += s_part[threadIdx.x + off];
        __syncthreads();
    }
    const double whole = s_part[0];
    const int entries = Sy * Sx;   // (checked by the caller: fits 31 bits)
    for (int e = blockIdx.x * kEventThreads + threadIdx.x; e < entries; e += gridDim.x * kEventThreads) {
        const int uy = e / Sx, ux = e - uy * Sx;
        const Occurrence o(g, mode, Sy, Sx, uy, ux);
        const int oy0 = o.qy[0] - (g.Ay - 1), ox0 = o.qx[0] - (g.Ax - 1);
        double out = whole;
        if (!o.single() || oy0 < 0 || ox0 < 0 || oy0 + g.Ay > g.Dy || ox0 + g.Ax > g.Dx) {
            out = 0.;
            for_each_tap(g, o, 0, 1, [&](int t, int c, int y, int x) {
                const double phi = phi_at(g, o, w, c * AA, y, x);
                out += (double)w[t] * phi;
            });
        }
        b[(size_t)p * entries + e] = out;
    }
}

template <typename T>
struct alignas(16) Chunk {
    T v[16 / sizeof(T)];
};

template <typename T>
__device__ __forceinline__ T score_of(T a, double b) {
    const double av = (double)a;
    return av > 0. && b > 0. ? (T)(av * av / (2. * b)) : (T)0;   // (NaN compares false)
}

// rows: N * P * Sy rows of the map; brows = P * Sy rows of b; cpr chunks per row
template <typename T, bool kAligned>
__global__ __launch_bounds__(kEventThreads) void k_pursuit_score(long long rows, int brows, int Sx, int Hs, int cpr,
                                                                  const T *a, const double *__restrict__ b,
                                                                  T *gain) {   // (gain may be a: a thread reads what it writes)
    constexpr int kV = 16 / sizeof(T);
    const long long stride = (long long)gridDim.x * kEventThreads;
    const long long first = (long long)blockIdx.x * kEventThreads + threadIdx.x;
    const long long row_step = stride / cpr;
    const int chunk_step = (int)(stride - row_step * cpr), brow_step = (int)(row_step % brows);
    long long row = first / cpr;
    int chunk = (int)(first - row * cpr), brow = (int)(row % brows);
    while (row < rows) {
        const int x0 = chunk * kV;
        const T *src = a + (size_t)row * Hs + x0;
        T *dst = gain + (size_t)row * Hs + x0;
        const double *bs = b + (size_t)brow * Sx + x0;
        if (kAligned && x0 + kV <= Sx) {
            const Chunk<T> in = *reinterpret_cast<const Chunk<T> *>(src);
            Chunk<T> out;
#pragma unroll
            for (int i = 0; i < kV; ++i) out.v[i] = score_of(in.v[i], bs[i]);
            *reinterpret_cast<Chunk<T> *>(dst) = out;
        } else {
            for (int i = 0; i < kV && x0 + i < Sx; ++i) dst[i] = score_of(src[i], bs[i]);
        }
        row += row_step, chunk += chunk_step, brow += brow_step;
        if (chunk >= cpr) chunk -= cpr, ++row, ++brow;
        if (brow >= brows) brow -= brows;
    }
}

template <typename T>
__global__ __launch_bounds__(kEventThreads) void k_pursuit_taken(long long entries, int Sx, int Hs,
                                                                  const long long *__restrict__ taken, long long n_taken,
                                                                  T *__restrict__ gain) {
    for (long long i = (long long)blockIdx.x * kEventThreads + threadIdx.x; i < n_taken;
         i += (long long)gridDim.x * kEventThreads) {
        const long long f = taken[i];
        if (f < 0 || f >= entries) continue;
        const long long row = f / Sx;
        gain[(size_t)row * Hs + (f - row * Sx)] = (T)0;
    }
}

template <typename T>
__global__ __launch_bounds__(kEventThreads) void k_pursuit_pick(EventGeo g, int mode, int Sy, int Sx,
                                                                 const T *__restrict__ W, const long long *__restrict__ idx,
                                                                 long long n_picked, const T *__restrict__ V,
                                                                 const T *__restrict__ R, int4 *__restrict__ ev,
                                                                 T *__restrict__ strength, double *__restrict__ gain,
                                                                 double *__restrict__ mag) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int AA = g.Ay * g.Ax, taps = g.C * AA;
    const long long plane = (long long)Sy * Sx, entries = (long long)g.N * g.P * plane;
    for (long long e = (long long)blockIdx.x * kWaves + wave; e < n_picked; e += (long long)gridDim.x * kWaves) {
        const long long f = idx[e];
        if (f < 0 || f >= entries) {   // (wave-uniform: outside the contract, no sample data is read)
            if (lane == 0) {
                ev[e] = make_int4(-1, -1, -1, -1);
                strength[e] = (T)0;
                gain[e] = 0.;
                if (mag) mag[e] = 0.;
            }
            continue;
        }
        const long long np = f / plane;
        const int u = (int)(f - np * plane);
        const int4 v = make_int4((int)(np / g.P), (int)(np % g.P), u / Sx, u % Sx);   // sample, plane, uy, ux
        const Occurrence o(g, mode, Sy, Sx, v.z, v.w);
        const bool single = o.single();   // (wave-uniform)
        const T *w = W + (size_t)v.y * taps;
        const size_t sample = (size_t)v.x * g.C * g.Dy * g.Dx;
        double a = 0., b = 0., m = 0.;
        for_each_tap(g, o, lane, 64, [&](int t, int c, int y, int x) {
            const size_t at = sample + ((size_t)c * g.Dy + y) * g.Dx + x;
            const double wv = (double)w[t];
            const double phi = single ? wv : phi_at(g, o, w, c * AA, y, x);
            const double wd = wv * ((double)V[at] - (double)R[at]);
            a += wd;
            b += wv * phi;
            m += fabs(wd);
        });
        a = wave_sum(a), b = wave_sum(b), m = wave_sum(m);
        if (lane == 0) {
            const bool live = a > 0. && b > 0.;
            ev[e] = v;
            strength[e] = live ? (T)(a / b) : (T)0;
            gain[e] = live ? a * a / (2. * b) : 0.;
            if (mag) mag[e] = m;
        }
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int events_norms(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const void *W, double *b, hipStream_t s) {
    const int entries = f.Sy * f.Sx;
    const dim3 grid(events_grid(ctx, cdiv(entries, kEventThreads), 8), (unsigned)f.g.P);
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_events_norms<T>, grid, dim3(kEventThreads), 0, s, f.g, f.mode, f.Sy, f.Sx, (const T *)W, b);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

template <typename T>
static int pursuit_score_t(tnmf_hip_ctx *ctx, long long planes, int P, int Sy, int Sx, int Hs, const T *a, const double *b,
                           T *gain, const long long *taken, long long n_taken, hipStream_t s) {
    constexpr int kV = 16 / sizeof(T);
    const long long entries = planes * Sy * Sx;
    long long rows = planes * Sy;
    if (rows > 0) {
        const long long per_sample = (long long)P * Sy * Sx;
        int brows = P * Sy;
        if (Hs == Sx && per_sample <= 0x7fffffffLL && per_sample % kV == 0) {
            // a C-contiguous map is one long row per sample over the whole table: 16-byte accesses whatever the shift width
            rows = planes / P, brows = 1, Sx = Hs = (int)per_sample;
        }
        const int cpr = cdiv(Sx, kV);
        const unsigned grid = events_grid(ctx, (rows * cpr + kEventThreads - 1) / kEventThreads, 8);
        const bool aligned = aligned16(a) && aligned16(gain) && Hs % kV == 0;
        if (aligned)
            hipLaunchKernelGGL((k_pursuit_score<T, true>), dim3(grid), dim3(kEventThreads), 0, s, rows, brows, Sx, Hs, cpr,
                               a, b, gain);
        else
            hipLaunchKernelGGL((k_pursuit_score<T, false>), dim3(grid), dim3(kEventThreads), 0, s, rows, brows, Sx, Hs, cpr,
                               a, b, gain);
        TNMF_LAUNCH_CHECK();
        if (n_taken > 0) {
            const unsigned tgrid = events_grid(ctx, (n_taken + kEventThreads - 1) / kEventThreads, 8);
            // (entries = rows * Sx in either view, and a flat index splits into row and column of either alike)
            hipLaunchKernelGGL(k_pursuit_taken<T>, dim3(tgrid), dim3(kEventThreads), 0, s, entries, Sx, Hs, taken, n_taken,
                               gain);
            TNMF_LAUNCH_CHECK();
        }
    }
    return TNMF_OK;
}

int pursuit_score(tnmf_hip_ctx *ctx, int dtype, long long planes, int P, int Sy, int Sx, int Hs, const void *a,
                  const double *b, void *gain, const long long *taken, long long n_taken, hipStream_t s) {
    return with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        return pursuit_score_t<T>(ctx, planes, P, Sy, Sx, Hs, (const T *)a, b, (T *)gain, taken, n_taken, s);
    });
}

int pursuit_pick(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const void *W, const long long *idx,
                 long long n_picked, const void *V, const void *R, int *events, void *strength, double *gain, double *mag,
                 hipStream_t s) {
    if (n_picked <= 0) return TNMF_OK;
    const unsigned grid = events_grid(ctx, (n_picked + kWaves - 1) / kWaves, 64);
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_pursuit_pick<T>, dim3(grid), dim3(kEventThreads), 0, s, f.g, f.mode, f.Sy, f.Sx, (const T *)W,
                           idx, n_picked, (const T *)V, (const T *)R, (int4 *)events, (T *)strength, gain, mag);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}
