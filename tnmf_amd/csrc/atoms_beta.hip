// atoms_beta.hip -- what each atom explains under a beta-divergence, in one pass over the activations
// (tnmf_hip_atom_terms_beta).
//
// The walk of atoms.hip -- one workgroup per (sample, pixel tile, channel chunk), the planes of H streamed through LDS, r_m
// of kAtomPix adjacent pixels per thread (atom_walk.h) -- with the pixel factors and the epilogue of atom_beta.h.  With
// x = max(R, 0) + eps and x_m = max(R - r_m, 0) + eps:
//   a[n, m]    = sum G r_m (V x^(beta-2) - x^(beta-1))
//   b[n, m]    = sum G r_m^2 c,          c = (beta-1) x^(beta-2) + (2-beta) V x^(beta-3)
//   gain[n, m] = sum G (D_beta(V | x_m) - D_beta(V | x))
// The two factors are formed in double when the pixels are loaded and rounded once to the element type; V, R and the
// clipped G of the thread's pixels stay in registers next to them, and after the last plane of an atom every pixel with
// r != 0 and G > 0 adds its gain term, evaluated in double (R - r in double).  Every other pixel adds an exact 0 and
// evaluates nothing.
//
// Three doubles per (sample, tile, atom) through the shuffle tree and the wave-order sum of atoms.hip;
// k_atom_terms_beta_finalize adds the tiles in tile order.  No atomics: the same bits every run.
#include <algorithm>
#include <cmath>

#include "atom_beta.h"
#include "atom_walk.h"

namespace {

constexpr int kStage = 10;   // tile elements per thread that the register stage holds; larger tiles: the plain loop
// atoms whose wave sums wait in LDS before they are combined and written: three doubles each where atoms.hip keeps two, so
// fewer of them than there -- the array stays inside the 4 KiB that atom_terms_check() leaves beside the tile of H, and
// every shape tnmf_hip_atom_terms serves is served here
constexpr int kBetaChunk = 42;
static_assert(kBetaChunk * (kAtomThreads / 64) * 3 * sizeof(double) <= 4096, "the waves' sums have 4 KiB of the 64");

template <typename T, int CH, int K>
__global__ __launch_bounds__(kAtomThreads) void k_atom_terms_beta(Geo g, AtomPlan p, int group, double beta, double eps,
                                                                  const T *__restrict__ V, const T *__restrict__ G,
                                                                  const T *__restrict__ R, const T *__restrict__ Wf,
                                                                  const T *__restrict__ H, double *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(32))) unsigned char smem_raw[];
    __shared__ double red[kBetaChunk][kAtomThreads / 64][3];
    T *Hs = reinterpret_cast<T *>(smem_raw);
    const int Mo = g.M / group;

    ATOM_TERMS_BLOCK();
    ATOM_WALK_PIXELS();

    // V, R and the clipped G of this thread's pixels, every channel of the chunk, and the two factors of atom_beta.h: read
    // and formed once, kept in registers.  Pixels outside the sample, channels past the last one and entries of weight
    // <= 0 (whatever V holds there) carry exact zeros, and nothing is evaluated for them.
    T vv[CH][kAtomPix], rr[CH][kAtomPix], gg[CH][kAtomPix];
    T gd[CH][kAtomPix], gw[CH][kAtomPix];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
#pragma unroll
        for (int px = 0; px < kAtomPix; ++px) {
            const bool in = c < nc && y < g.Dy && xb + px < g.Dx;
            T w = T(0), v = T(0), rv = T(0);
            if (in) {
                const size_t o = (((size_t)n * g.C + c0 + c) * g.Dy + y) * g.Dx + xb + px;
                w = G ? G[o] : T(1);
                v = V[o];
                rv = R[o];
            }
            double d = 0.0, cw = 0.0;
            if (w > T(0)) beta_pixel<K>((double)v, (double)rv, (double)w, eps, beta, d, cw);
            vv[c][px] = v;
            rr[c][px] = rv;
            gg[c][px] = w > T(0) ? w : T(0);
            gd[c][px] = (T)d;
            gw[c][px] = (T)cw;
        }
    }
    ATOM_WALK_TILE();
    const bool pre_ok = nel <= kStage * kAtomThreads;   // the tile fits the register stage (uniform)
    ATOM_WALK_FETCH();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    Pair<T> r[CH][kAtomPix];   // (r of pixel px is r[c][px].x + r[c][px].y)
    if (pre_ok) fetch(0);
    for (int plane = 0; plane < g.M; ++plane) {
        ATOM_TERMS_PLANE(plane, r);
        if (t != group - 1) continue;
        // r_m is complete: fold into the three sums, in double
        double pa = 0.0, pb = 0.0, pg = 0.0;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
#pragma unroll
            for (int px = 0; px < kAtomPix; ++px) {
                const double rv = (double)(r[c][px].x + r[c][px].y);
                pa += rv * (double)gd[c][px];
                pb += (double)gw[c][px] * (rv * rv);
                if (gg[c][px] > T(0) && rv != 0.0)
                    pg += (double)gg[c][px] * beta_gain<K>((double)vv[c][px], (double)rr[c][px], rv, eps, beta);
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            pa += __shfl_down(pa, o, 64);
            pb += __shfl_down(pb, o, 64);
            pg += __shfl_down(pg, o, 64);
        }
        const int ml = mo % kBetaChunk;
        if (lane == 0) {
            red[ml][wave][0] = pa;
            red[ml][wave][1] = pb;
            red[ml][wave][2] = pg;
        }
        if (ml == kBetaChunk - 1 || mo == Mo - 1) {
            __syncthreads();
            if ((int)threadIdx.x <= ml) {
                double sa = 0.0, sb = 0.0, sg = 0.0;
#pragma unroll
                for (int wv = 0; wv < kAtomThreads / 64; ++wv) {   // wave order: fixed
                    sa += red[threadIdx.x][wv][0];
                    sb += red[threadIdx.x][wv][1];
                    sg += red[threadIdx.x][wv][2];
                }
                double *out = partials + (((size_t)n * p.slots + slot) * Mo + (mo - ml) + threadIdx.x) * 3;
                out[0] = sa;
                out[1] = sb;
                out[2] = sg;
            }
            __syncthreads();
        }
    }
}

// abg[n, m] = the sum of the slots' partial sums in slot order
__global__ __launch_bounds__(kAtomThreads) void k_atom_terms_beta_finalize(size_t rows, int slots, int Mo,
                                                                           const double *__restrict__ partials,
                                                                           double *__restrict__ abg) {
    const size_t i = (size_t)blockIdx.x * kAtomThreads + threadIdx.x;
    if (i >= rows) return;
    const size_t n = i / Mo, m = i - n * Mo;
    const double *in = partials + (n * slots * Mo + m) * 3;
    double sa = 0.0, sb = 0.0, sg = 0.0;
    for (int s = 0; s < slots; ++s) {
        const double *v = in + (size_t)s * Mo * 3;
        sa += v[0];
        sb += v[1];
        sg += v[2];
    }
    abg[3 * i] = sa;
    abg[3 * i + 1] = sb;
    abg[3 * i + 2] = sg;
}

__global__ __launch_bounds__(kAtomThreads) void k_atom_terms_widen(size_t rows, const double *__restrict__ ab,
                                                                   double *__restrict__ abg) {
    const size_t i = (size_t)blockIdx.x * kAtomThreads + threadIdx.x;
    if (i >= rows) return;
    const double a = ab[2 * i], b = ab[2 * i + 1];
    abg[3 * i] = a;
    abg[3 * i + 1] = b;
    abg[3 * i + 2] = a + b / 2;
}

template <typename T, int CH>
void launch_chunked(const Geo &g, const AtomPlan &p, int group, double beta, double eps, unsigned blocks, size_t lds,
                    const void *V, const void *G, const void *R, const void *Wf, const void *H, double *partials,
                    hipStream_t s) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kAtomThreads), lds, s, g, p, group, beta, eps, (const T *)V,
                           (const T *)G, (const T *)R, (const T *)Wf, (const T *)H, partials);
    };
    switch (beta_kind(beta)) {
        case 0: go(k_atom_terms_beta<T, CH, 0>); break;
        case 1: go(k_atom_terms_beta<T, CH, 1>); break;
        default: go(k_atom_terms_beta<T, CH, 3>); break;
    }
}

}  // namespace

size_t atom_terms_beta_partial_bytes(const Geo &g, int group) {
    return align_up((size_t)g.N * atom_terms_plan(g).slots * (g.M / group) * 3 * sizeof(double), 256);
}

int launch_atom_terms_beta(const tnmf_hip_ctx *ctx, const Geo &g, int dtype, int group, double beta, double eps,
                           const void *V, const void *G, const void *R, const void *W, const void *H, double *partials,
                           void *taps, double *abg, hipStream_t s) {
    const int rc = atom_terms_check(g, dtype);
    if (rc != TNMF_OK) return rc;
    const AtomPlan p = atom_terms_plan(g);
    const size_t lds = (size_t)p.SH * p.SW * esize(dtype);
    const size_t blocks = (size_t)g.N * p.slots;
    const int trc = launch_atom_taps(ctx, g, dtype, W, taps, s);
    if (trc != TNMF_OK) return trc;
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        switch (p.CH) {
            case 1: launch_chunked<T, 1>(g, p, group, beta, eps, (unsigned)blocks, lds, V, G, R, taps, H, partials, s); break;
            case 2: launch_chunked<T, 2>(g, p, group, beta, eps, (unsigned)blocks, lds, V, G, R, taps, H, partials, s); break;
            case 3: launch_chunked<T, 3>(g, p, group, beta, eps, (unsigned)blocks, lds, V, G, R, taps, H, partials, s); break;
            default: launch_chunked<T, 4>(g, p, group, beta, eps, (unsigned)blocks, lds, V, G, R, taps, H, partials, s); break;
        }
    });
    TNMF_LAUNCH_CHECK();
    const size_t out_rows = (size_t)g.N * (g.M / group);
    hipLaunchKernelGGL(k_atom_terms_beta_finalize, dim3((unsigned)((out_rows + kAtomThreads - 1) / kAtomThreads)),
                       dim3(kAtomThreads), 0, s, out_rows, p.slots, g.M / group, (const double *)partials, abg);
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

int launch_atom_terms_widen(const double *ab, size_t rows, double *abg, hipStream_t s) {
    if (rows == 0) return TNMF_OK;
    hipLaunchKernelGGL(k_atom_terms_widen, dim3((unsigned)((rows + kAtomThreads - 1) / kAtomThreads)), dim3(kAtomThreads),
                       0, s, rows, ab, abg);
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

extern "C" {

int tnmf_hip_atom_terms_beta(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int group, double beta, double eps, const void *V,
                             const void *G_or_null, const void *R_or_null, const void *W, const void *H, double *abg,
                             void *stream) {
    if (!ctx || !geom) return TNMF_E_NULL;
    Geo g;
    int rc = atom_entry_geo(geom, &g);
    if (rc != TNMF_OK) return rc;
    const int dtype = geom->dtype;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    if (group < 1 || g.M % group != 0 || !std::isfinite(beta) || !(eps >= 0.0)) return TNMF_E_GEOM;
    if (g.N == 0) return TNMF_OK;
    if (!V || !W || !H || !abg) return TNMF_E_NULL;
    rc = atom_terms_check(g, dtype);
    if (rc != TNMF_OK) return rc;
    // work buffer: [partial sums per (sample, tile, atom) | the taps of the flipped dictionary | beta 2: (a, b) of the
    // Frobenius kernels, which take the first two parts as tnmf_hip_atom_terms lays them out]
    const bool frob = beta == 2.0;
    const size_t rows = (size_t)g.N * (g.M / group);
    const size_t p_bytes = frob ? atom_terms_partial_bytes(g, group) : atom_terms_beta_partial_bytes(g, group);
    const size_t t_bytes = atom_terms_taps_bytes(g, dtype);
    const void *R = R_or_null;
    void *buf = nullptr;
    rc = atom_entry_buffers(ctx, g, dtype, p_bytes + t_bytes + (frob ? rows * 2 * sizeof(double) : 0), W, H, &R, &buf, s);
    if (rc != TNMF_OK) return rc;
    char *work = static_cast<char *>(buf);
    if (!frob)
        return launch_atom_terms_beta(ctx, g, dtype, group, beta, eps, V, G_or_null, R, W, H,
                                      reinterpret_cast<double *>(work), work + p_bytes, abg, s);
    double *ab = reinterpret_cast<double *>(work + p_bytes + t_bytes);
    rc = launch_atom_terms(ctx, g, dtype, group, V, G_or_null, R, W, H, reinterpret_cast<double *>(work), work + p_bytes, ab,
                           s);
    if (rc != TNMF_OK) return rc;
    return launch_atom_terms_widen(ab, rows, abg, s);
}

}  // extern "C"
