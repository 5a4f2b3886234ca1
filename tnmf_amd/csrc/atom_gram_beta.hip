// atom_gram_beta.hip -- how atoms overlap under a beta-divergence, in one pass over the activations
// (tnmf_hip_atom_gram_beta).
//
// The kernel of atom_gram.hip -- one workgroup per (sample, strip of pixel tiles, pair of atom blocks), r_m of the tile
// parked in LDS and contracted over the pixels on the matrix cores (v_mfma_f64_16x16x4_f64): the same body,
// atom_gram_kernel.h -- with the pixel factors of atom_beta.h in the place of G d and G (ATOM_GRAM_PIXEL).  With
// x = max(R, 0) + eps:
//   a[n, m]     = sum G R_m (V x^(beta-2) - x^(beta-1))
//   B[n, m, m'] = sum G c R_m R_m',       c = (beta-1) x^(beta-2) + (2-beta) V x^(beta-3)
// The weights G c of the contraction are signed (c < 0 occurs outside 1 <= beta <= 2): nothing clamps them at 0, and only
// G <= 0 selects an exact zero.  Both factors are formed in double and rounded once to the element type.
//
// The plan, the partial sums, the taps and the finalize kernel are those of atom_gram.hip (launch_atom_gram_finalize); B is
// symmetric to the bit and the same from run to run for the same reasons.
#include <algorithm>
#include <cmath>

#include "atom_beta.h"
#include "atom_gram_kernel.h"

namespace {

// the two factors of atom_beta.h, formed in double and rounded once: signed; an entry of weight <= 0 evaluates nothing
#define ATOM_GRAM_PIXEL(in, offset)                                                           \
    double d = 0.0, cw = 0.0;                                                                 \
    if (in) {                                                                                 \
        const size_t o = offset;                                                              \
        const T w = G ? G[o] : T(1);                                                          \
        if (w > T(0)) beta_pixel<K>((double)V[o], (double)R[o], (double)w, eps, beta, d, cw); \
    }                                                                                         \
    gw[px] = (T)cw;                                                                           \
    gd[px] = (T)d

template <typename T, int NBLK, int HALVES, int K>   // NBLK = cap / 16; K: the beta_kind of atom_beta.h
__global__ __launch_bounds__(kAtomThreads * HALVES) void k_atom_gram_beta(Geo g, GramPlan p, int group, double beta,
                                                                          double eps, const T *__restrict__ V,
                                                                          const T *__restrict__ G, const T *__restrict__ R,
                                                                          const T *__restrict__ Wf, const T *__restrict__ H,
                                                                          double *__restrict__ partials) {
#define ATOM_GRAM_KERNEL_BODY
#include "atom_gram_kernel.h"
#undef ATOM_GRAM_KERNEL_BODY
}

template <typename T, int NBLK, int HALVES, int K>
int launch_gram_kind(const tnmf_hip_ctx *ctx, const GramPlan &p, unsigned blocks, hipStream_t s, Geo g, int group, double beta,
                     double eps, const T *V, const T *G, const T *R, const T *Wf, const T *H, double *partials) {
    // more than 64 KiB of dynamic LDS is an attribute of the (function, device) pair: set once for each
    static bool opted_in[64] = {};
    const int dev = ctx->device;
    if (p.lds > 64 * 1024 && !(dev >= 0 && dev < 64 && opted_in[dev])) {
        TNMF_HIP_TRY(hipFuncSetAttribute((const void *)k_atom_gram_beta<T, NBLK, HALVES, K>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGramLds));
        if (dev >= 0 && dev < 64) opted_in[dev] = true;
    }
    hipLaunchKernelGGL((k_atom_gram_beta<T, NBLK, HALVES, K>), dim3(blocks), dim3(kAtomThreads * HALVES), p.lds, s, g, p,
                       group, beta, eps, V, G, R, Wf, H, partials);
    return TNMF_OK;
}

template <typename T, int NBLK, int HALVES>
int launch_gram(const tnmf_hip_ctx *ctx, const Geo &g, const GramPlan &p, int group, double beta, double eps,
                unsigned blocks, const void *V, const void *G, const void *R, const void *Wf, const void *H,
                double *partials, hipStream_t s) {
    const T *v = (const T *)V, *gp = (const T *)G, *r = (const T *)R, *wf = (const T *)Wf, *h = (const T *)H;
    switch (beta_kind(beta)) {
        case 0: return launch_gram_kind<T, NBLK, HALVES, 0>(ctx, p, blocks, s, g, group, beta, eps, v, gp, r, wf, h, partials);
        case 1: return launch_gram_kind<T, NBLK, HALVES, 1>(ctx, p, blocks, s, g, group, beta, eps, v, gp, r, wf, h, partials);
        default: return launch_gram_kind<T, NBLK, HALVES, 3>(ctx, p, blocks, s, g, group, beta, eps, v, gp, r, wf, h, partials);
    }
}

}  // namespace

int launch_atom_gram_beta(const tnmf_hip_ctx *ctx, const Geo &g, int dtype, int group, double beta, double eps,
                          const void *V, const void *G, const void *R, const void *W, const void *H, double *partials,
                          void *taps, double *a, double *B, hipStream_t s) {
    const int rc = atom_gram_check(g, dtype, group);
    if (rc != TNMF_OK) return rc;
    const GramPlan p = atom_gram_plan(g, dtype, group);
    const size_t blocks = (size_t)g.N * p.strips * p.pairs;
    const int trc = launch_atom_taps(ctx, g, dtype, W, taps, s);
    if (trc != TNMF_OK) return trc;
    const int lrc = with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        if constexpr (sizeof(T) == sizeof(float)) {   // (32 rows of doubles never fit: those kernels do not exist)
            if (p.halves == 2)
                return launch_gram<T, 2, 2>(ctx, g, p, group, beta, eps, (unsigned)blocks, V, G, R, taps, H, partials, s);
            if (p.cap == 32)
                return launch_gram<T, 2, 1>(ctx, g, p, group, beta, eps, (unsigned)blocks, V, G, R, taps, H, partials, s);
        }
        if (p.cap != 16) return (int)TNMF_E_UNSUPPORTED;
        return launch_gram<T, 1, 1>(ctx, g, p, group, beta, eps, (unsigned)blocks, V, G, R, taps, H, partials, s);
    });
    if (lrc != TNMF_OK) return lrc;
    TNMF_LAUNCH_CHECK();
    return launch_atom_gram_finalize(g, p, group, partials, a, B, s);
}

extern "C" {

int tnmf_hip_atom_gram_beta(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int group, double beta, double eps, const void *V,
                            const void *G_or_null, const void *R_or_null, const void *W, const void *H, double *a, double *B,
                            void *stream) {
    if (!ctx || !geom) return TNMF_E_NULL;
    Geo g;
    int rc = atom_entry_geo(geom, &g);
    if (rc != TNMF_OK) return rc;
    const int dtype = geom->dtype;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    if (group < 1 || g.M % group != 0 || !std::isfinite(beta) || !(eps >= 0.0)) return TNMF_E_GEOM;
    if (beta == 2.0) return tnmf_hip_atom_gram(ctx, geom, group, V, G_or_null, R_or_null, W, H, a, B, stream);
    if (g.N == 0) return TNMF_OK;
    if (!V || !W || !H || !a || !B) return TNMF_E_NULL;
    rc = atom_gram_check(g, dtype, group);
    if (rc != TNMF_OK) return rc;
    // work buffer: as tnmf_hip_atom_gram
    const size_t p_bytes = atom_gram_partial_bytes(g, dtype, group);
    const void *R = R_or_null;
    void *buf = nullptr;
    rc = atom_entry_buffers(ctx, g, dtype, p_bytes + atom_terms_taps_bytes(g, dtype), W, H, &R, &buf, s);
    if (rc != TNMF_OK) return rc;
    return launch_atom_gram_beta(ctx, g, dtype, group, beta, eps, V, G_or_null, R, W, H, static_cast<double *>(buf),
                                 static_cast<char *>(buf) + p_bytes, a, B, s);
}

}  // extern "C"
