// patches.hip -- the data under each event, and how the occurrences of an atom vary (include/tnmf_hip.h, "patches").
//
// k_events_patches: one wave per event, the walk of k_events_gain (event_walk.h: Occurrence, for_each_tap, phi_at) -- tap t of
// an image in lane t % 64, images in image order.  Where k_events_gain multiplies the signal under a tap by the tap and sums
// over the wave, this kernel keeps the signal: x_e[t] = the sum over the images of s at the tap's pixel, s one of V, V - R and
// V - R + h_e phi_e.  A tap belongs to one lane, so the lane adds the images of its taps in place, without a neighbour: in
// the row of `out` itself when no fold follows (the row is zeroed first unless the occurrence is one image wholly inside the
// sample, whose every tap is stored once), else in the wave's slice of LDS, from which the fold L_t^T gathers y_e by the
// caller's table in table order.  It writes the n_events * C * prod(A) doubles and nothing else; no atomics.
//
// k_patch_moments: S[m] = sum_e y_e y_e^T over the rows of atom m, a batched symmetric rank-K update on
// v_mfma_f64_16x16x4_f64 (operand layout as in atom_gram.hip: lane (i, k) = (lane & 15, lane >> 4) holds row i of A and column
// i of B at depth k; C/D col = lane & 15, row = (lane >> 4) + 4 * reg).  One wave owns one pair (I <= J) of 16 x 16 blocks of
// one atom and walks that atom's run of by_atom four entries at a time, the fours aligned to the position in by_atom so that
// a chunk that begins at a multiple of four continues the bits of the chunk before it; entries of a four outside the run and
// columns beyond D are zeros.  The waves of the diagonal blocks also hold what g needs -- they pass the four rows round with
// shuffles and add them one entry at a time -- and the first of them takes s2 and count.  Nothing is split over the entries
// and nothing is atomic.  The waves of a workgroup are independent (no LDS, no barrier): four pairs to a workgroup.
#include <algorithm>

#include "event_walk.h"
#include "patches.h"

namespace {

constexpr int kWaves = kEventThreads / 64;
constexpr int kMomentAhead = 4;   // fours of entries whose loads a trip of k_patch_moments issues together
using Acc = double __attribute__((ext_vector_type(4)));
static_assert(kMomentBlock == 16 && kMomentDepth == 4, "the operand layout below is that of v_mfma_f64_16x16x4_f64");
static_assert((size_t)kWaves * TNMF_PATCH_STAGE_MAX * sizeof(double) <= 64 * 1024, "the staged patches of a workgroup fit 64 KiB");

template <typename T>
__global__ __launch_bounds__(kEventThreads) void k_events_patches(EventGeo g, int mode, int Sy, int Sx, int source,
                                                                   const T *__restrict__ W, const int4 *__restrict__ ev,
                                                                   const T *__restrict__ h, long long n_events,
                                                                   const T *__restrict__ V, const T *__restrict__ R,
                                                                   const int *__restrict__ fold_ptr,
                                                                   const int *__restrict__ fold_src,
                                                                   const double *__restrict__ fold_w, int n_fold,
                                                                   double *out) {
    extern __shared__ double s_stage[];   // with a fold table: kWaves slices of `taps` doubles
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int AA = g.Ay * g.Ax, taps = g.C * AA;
    const unsigned uAA = AA;
    double *mine = s_stage + (size_t)wave * taps;
    for (long long e = (long long)blockIdx.x * kWaves + wave; e < n_events; e += (long long)gridDim.x * kWaves) {
        const int4 v = ev[e];   // sample, plane, uy, ux
        double *oe = out + (size_t)e * taps;
        if ((unsigned)v.x >= (unsigned)g.N || (unsigned)v.y >= (unsigned)g.P || (unsigned)v.z >= (unsigned)Sy ||
            (unsigned)v.w >= (unsigned)Sx) {   // (wave-uniform: outside the contract, no sample data is read)
            for (int t = lane; t < taps; t += 64) oe[t] = 0.;
            continue;
        }
        const Occurrence o(g, mode, Sy, Sx, v.z, v.w);
        const bool single = o.single();   // (wave-uniform)
        const int oy = o.qy[0] - (g.Ay - 1), ox = o.qx[0] - (g.Ax - 1);
        const bool whole = single && oy >= 0 && oy + g.Ay <= g.Dy && ox >= 0 && ox + g.Ax <= g.Dx;
        const bool cleaned = source == TNMF_PATCH_CLEANED;
        const T *w = cleaned ? W + (size_t)v.y * taps : nullptr;
        const double hv = cleaned ? (double)h[e] : 0.;
        const size_t sample = (size_t)v.x * g.C * g.Dy * g.Dx;
        // x_e into dst (the row of out, or the wave's slice of LDS): every tap belongs to one lane, which adds its images
        auto gather = [&](double *dst) {
            if (!whole)
                for (int t = lane; t < taps; t += 64) dst[t] = 0.;
            for_each_tap(g, o, lane, 64, [&](int t, int c, int y, int x) {
                const size_t at = sample + ((size_t)c * g.Dy + y) * g.Dx + x;
                double sv;
                if (source == TNMF_PATCH_DATA)
                    sv = (double)V[at];
                else if (!cleaned)
                    sv = (double)V[at] - (double)R[at];
                else
                    sv = residual_without(V[at], R[at], hv, single ? (double)w[t] : phi_at(g, o, w, c * AA, y, x));
                dst[t] = single ? sv : dst[t] + sv;   // (one image: the tap is met once)
            });
        };
        if (!fold_ptr) {
            gather(oe);
            continue;
        }
        gather(mine);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int *ptr = fold_ptr + (size_t)(v.y % n_fold) * AA;   // the rows of L_t^T, t = p % T
        for (int t = lane; t < taps; t += 64) {
            const int c = t / uAA, i = t - c * AA;
            const double *xc = mine + c * AA;
            const int k1 = ptr[i + 1];
            double y = 0.;
            for (int k = max(ptr[i], 0); k < k1; ++k) {
                const int src = fold_src[k];
                if ((unsigned)src < uAA) y += fold_w[k] * xc[src];
            }
            oe[t] = y;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // (the slice is read before the next row overwrites it)
        __builtin_amdgcn_wave_barrier();
    }
}

// the pair (I, J), I <= J < nb, of index `pair` in the order (0,0) (0,1) .. (0,nb-1) (1,1) ..
__host__ __device__ inline void moment_blocks(int pair, int nb, int &I, int &J) {
    I = 0;
    while (pair >= nb - I) {
        pair -= nb - I;
        ++I;
    }
    J = I + pair;
}

__global__ __launch_bounds__(kEventThreads) void k_patch_moments(int D, int n_atoms, int nb, int pairs,
                                                                  const double *__restrict__ Y, const double *__restrict__ h,
                                                                  const int *__restrict__ by_atom,
                                                                  const int *__restrict__ atom_start, int n_rows,
                                                                  int accumulate, double *__restrict__ S,
                                                                  double *__restrict__ g, double *__restrict__ s2,
                                                                  double *__restrict__ count) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long unit = (long long)blockIdx.x * kWaves + wave;   // (atom, pair of blocks): one wave each
    if (unit >= (long long)n_atoms * pairs) return;                // (wave-uniform; the kernel has no barrier)
    const int m = (int)(unit / pairs);
    int I, J;
    moment_blocks((int)(unit - (long long)m * pairs), nb, I, J);
    const int a = min(max(atom_start[m], 0), n_rows), b = min(max(atom_start[m + 1], 0), n_rows);
    const int li = lane & 15, lk = lane >> 4;
    const int ci = I * kMomentBlock + li, cj = J * kMomentBlock + li;   // the columns of Y this lane feeds as A and as B
    const bool diag = I == J, first = diag && I == 0;                   // (wave-uniform)
    double *Sm = S + (size_t)m * D * D;
    Acc acc = Acc(0.);
    double gs = 0., ss = 0.;
    if (accumulate) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = I * kMomentBlock + lk + 4 * reg;
            if (row < D && cj < D) acc[reg] = Sm[(size_t)row * D + cj];
        }
        if (diag && ci < D) gs = g[(size_t)m * D + ci];
        if (first) ss = s2[m];
    }
    // the fours begin at the multiples of four of the position in by_atom: a chunk cut there continues the same MFMAs
    // kMomentAhead fours per trip: their entries, then their rows, are loaded before the first MFMA, so a trip pays the two
    // dependent loads once (a four beyond the run is zeros: it leaves every sum as it is)
    for (long long r0 = b > a ? (a & ~(kMomentDepth - 1)) : b; r0 < b; r0 += kMomentDepth * kMomentAhead) {
        int row[kMomentAhead];
        double ya[kMomentAhead], yb[kMomentAhead], hv[kMomentAhead];
#pragma unroll
        for (int u = 0; u < kMomentAhead; ++u) {
            const long long r = r0 + u * kMomentDepth + lk;
            row[u] = r >= a && r < b ? by_atom[r] : -1;
        }
#pragma unroll
        for (int u = 0; u < kMomentAhead; ++u) {
            const bool ok = (unsigned)row[u] < (unsigned)n_rows;   // (an entry out of range is fed as zeros)
            ya[u] = ok && ci < D ? Y[(size_t)row[u] * D + ci] : 0.;
            yb[u] = diag ? ya[u] : ok && cj < D ? Y[(size_t)row[u] * D + cj] : 0.;
            hv[u] = diag && ok ? h[row[u]] : 0.;
        }
#pragma unroll
        for (int u = 0; u < kMomentAhead; ++u) {
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[u], yb[u], acc, 0, 0, 0);
            if (diag) {   // g of the block's columns (and s2): the four entries one after the other, in every lane of a column
#pragma unroll
                for (int k = 0; k < kMomentDepth; ++k) {
                    const double hk = __shfl(hv[u], k * 16 + li, 64), yk = __shfl(ya[u], k * 16 + li, 64);
                    gs = fma(hk, yk, gs);
                    ss = fma(hk, hk, ss);
                }
            }
        }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int row = I * kMomentBlock + lk + 4 * reg;
        if (row < D && cj < D && (!diag || row <= cj)) {   // (a diagonal block: the upper triangle and its mirror image)
            Sm[(size_t)row * D + cj] = acc[reg];
            Sm[(size_t)cj * D + row] = acc[reg];
        }
    }
    if (diag && lk == 0 && ci < D) g[(size_t)m * D + ci] = gs;
    if (first && lane == 0) {
        s2[m] = ss;
        count[m] = (accumulate ? count[m] : 0.) + (double)(b > a ? b - a : 0);
    }
}

}  // namespace

int events_patches(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, int source, const void *W, const int *events,
                   const void *strength, long long n_events, const void *V, const void *R, const int *fold_ptr,
                   const int *fold_src, const double *fold_w, int n_fold, double *out, hipStream_t s) {
    const EventGeo &g = f.g;
    if (n_events <= 0 || g.N <= 0) return TNMF_OK;
    const long long taps = (long long)g.C * g.Ay * g.Ax;
    if (fold_ptr && !patches_stage_fits(taps)) return TNMF_E_GEOM;
    const size_t lds = fold_ptr ? (size_t)kWaves * taps * sizeof(double) : 0;
    const unsigned grid = events_grid(ctx, (n_events + kWaves - 1) / kWaves, TNMF_PATCHES_BLOCKS_PER_CU);
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_events_patches<T>, dim3(grid), dim3(kEventThreads), lds, s, g, f.mode, f.Sy, f.Sx, source,
                           (const T *)W, (const int4 *)events, (const T *)strength, n_events, (const T *)V, (const T *)R,
                           fold_ptr, fold_src, fold_w, n_fold, out);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

int patch_moments(tnmf_hip_ctx *ctx, int D, int n_atoms, const double *Y, const double *h, const int *by_atom,
                  const int *atom_start, int n_rows, int accumulate, double *S, double *g, double *s2, double *count,
                  hipStream_t s) {
    const int nb = cdiv(D, kMomentBlock), pairs = nb * (nb + 1) / 2;
    const long long units = (long long)n_atoms * pairs;
    hipLaunchKernelGGL(k_patch_moments, dim3((unsigned)((units + kWaves - 1) / kWaves)), dim3(kEventThreads), 0, s, D, n_atoms,
                       nb, pairs, Y, h, by_atom, atom_start, n_rows, accumulate, S, g, s2, count);
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}
