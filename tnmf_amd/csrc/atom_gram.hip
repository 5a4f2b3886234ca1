// atom_gram.hip -- how atoms overlap, in one pass over the activations (tnmf_hip_atom_gram).
//
// With R_m the contribution of atom m in its `group` orientations (planes m * group + t of H and W) and d = V - R:
//   a[n, m] = sum G * R_m * d        B[n, m, m'] = sum G * R_m * R_m'        (G = 1 without weights)
// diag(B) is the b of atoms.hip; with a and B the objective is an exact quadratic in per-atom scale factors.
//
// One workgroup = one (sample, strip of kGramStripTiles pixel tiles, pair (I, J) of atom blocks).  Per tile and channel it
// builds r_m of the atoms of its two blocks exactly as k_atom_terms does -- planes of H streamed through LDS, taps through
// the scalar cache from the flipped copy, packed f32 pairs -- and, when an atom's last plane is in, parks r_m of the tile in
// LDS (and folds r * (G d) into a double, as k_atom_terms).  Then the four waves contract the parked rows over the tile's
// pixels on the matrix cores: v_mfma_f64_16x16x4_f64 on 16 x 16 blocks of atom pairs, operands G * r_m (the product in
// double) and r_m' converted to double, a quarter of the pixels per wave.  The accumulators stay in registers over the
// tiles and channels of the strip; at its end the waves' blocks are added in wave order and written once per workgroup.
//
// Only blocks on or above the diagonal are accumulated, and k_atom_gram_finalize reads entry (m, m') and (m', m) from the
// same place: B is symmetric to the bit.  It adds the strips in strip order.  No atomics: the same bits every run.
//
// With 32 rows parked only one workgroup fits a CU, so there the workgroup has 512 threads where the LDS allows: two halves
// of 256 that build different atoms of the same tile at the same time, each from a tile of H of its own (HALVES = 2; the
// contraction then gives every one of the eight waves an eighth of the pixels).
//
// M / group <= cap: one pair, blocks 0 and 1 are the atoms in order.  More atoms: every pair I < J of blocks of cap / 2
// atoms is a workgroup of its own that builds r of both blocks again; the diagonal block of I (and a) is taken from the pair
// (I, I + 1), of the last block from (I - 1, I).
//
// The body of the kernel is atom_gram_kernel.h, shared as text with atom_gram_beta.hip; this file has the signature, the
// two factors of a pixel (ATOM_GRAM_PIXEL), the plan and the launchers.
#include <algorithm>

#include "atom_gram_kernel.h"

namespace {

// G * d and G: an entry of weight <= 0 carries exact zeros like a pixel outside the sample
#define ATOM_GRAM_PIXEL(in, offset) \
    T w = T(0), d = T(0);           \
    if (in) {                       \
        const size_t o = offset;    \
        w = G ? G[o] : T(1);        \
        d = V[o] - R[o];            \
    }                               \
    gw[px] = w > T(0) ? w : T(0);   \
    gd[px] = w > T(0) ? w * d : T(0)

template <typename T, int NBLK, int HALVES>   // NBLK = cap / 16
__global__ __launch_bounds__(kAtomThreads * HALVES) void k_atom_gram(Geo g, GramPlan p, int group,
                                                                     const T *__restrict__ V, const T *__restrict__ G,
                                                                     const T *__restrict__ R, const T *__restrict__ Wf,
                                                                     const T *__restrict__ H, double *__restrict__ partials) {
#define ATOM_GRAM_KERNEL_BODY
#include "atom_gram_kernel.h"
#undef ATOM_GRAM_KERNEL_BODY
}

// B[n, m, m'] = B[n, m', m] = the strips' sums of the entry (min, max) in strip order; a[n, m] next to the diagonal
__global__ __launch_bounds__(kAtomThreads) void k_atom_gram_finalize(size_t total, GramPlan p, int Mo,
                                                                     const double *__restrict__ partials,
                                                                     double *__restrict__ a, double *__restrict__ B) {
    const size_t i = (size_t)blockIdx.x * kAtomThreads + threadIdx.x;
    if (i >= total) return;
    const int m2 = (int)(i % Mo);
    const size_t rest = i / Mo;
    const int m1 = (int)(rest % Mo);
    const size_t n = rest / Mo;
    const int lo = m1 < m2 ? m1 : m2, hi = m1 < m2 ? m2 : m1;
    int I = lo / p.hb, J = hi / p.hb;
    if (I == J) {
        if (I + 1 < p.nbk) J = I + 1;
        else I = J - 1;
    }
    int pair = J - I - 1;
    for (int k = 0; k < I; ++k) pair += p.nbk - 1 - k;
    const int si = lo / p.hb == I ? lo - I * p.hb : p.hb + lo - J * p.hb;
    const int sj = hi / p.hb == I ? hi - I * p.hb : p.hb + hi - J * p.hb;
    const double *in = partials + ((size_t)n * p.strips * p.pairs + pair) * p.wg_doubles;
    double sb = 0.0, sa = 0.0;
    for (int s = 0; s < p.strips; ++s) {
        const double *wg = in + (size_t)s * p.pairs * p.wg_doubles;
        sb += wg[si * p.cap + sj];
        if (m1 == m2) sa += wg[p.cap * p.cap + si];
    }
    B[i] = sb;
    if (m1 == m2) a[n * Mo + m1] = sa;
}

template <typename T, int NBLK, int HALVES>
int launch_gram(const tnmf_hip_ctx *ctx, const Geo &g, const GramPlan &p, int group, unsigned blocks, const void *V,
                const void *G, const void *R,
                const void *Wf, const void *H, double *partials, hipStream_t s) {
    // more than 64 KiB of dynamic LDS is an attribute of the (function, device) pair: set once for each
    static bool opted_in[64] = {};
    const int dev = ctx->device;
    if (p.lds > 64 * 1024 && !(dev >= 0 && dev < 64 && opted_in[dev])) {
        TNMF_HIP_TRY(hipFuncSetAttribute((const void *)k_atom_gram<T, NBLK, HALVES>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGramLds));
        if (dev >= 0 && dev < 64) opted_in[dev] = true;
    }
    hipLaunchKernelGGL((k_atom_gram<T, NBLK, HALVES>), dim3(blocks), dim3(kAtomThreads * HALVES), p.lds, s, g, p, group,
                       (const T *)V,
                       (const T *)G, (const T *)R, (const T *)Wf, (const T *)H, partials);
    return TNMF_OK;
}

}  // namespace

GramPlan atom_gram_plan(const Geo &g, int dtype, int group) {
    GramPlan p;
    p.ap = atom_terms_plan(g);
    const int Mo = g.M / group;
    const size_t es = esize(dtype);
    const size_t h_bytes = align_up((size_t)p.ap.SH * p.ap.SW * es, 32);
    auto lds_of = [&](int cap, int halves) {
        return ((size_t)cap * kGramStride + kGramTilePix) * es + halves * h_bytes + (size_t)cap * kWaves * sizeof(double);
    };
    p.cap = Mo > 16 && lds_of(32, 1) <= kGramLds ? 32 : lds_of(16, 1) <= kGramLds ? 16 : 0;
    p.halves = p.cap == 32 && lds_of(32, 2) <= kGramLds ? 2 : 1;   // (16 rows leave room for two workgroups per CU as it is)
    p.h_elems = h_bytes / es;
    p.hb = p.cap / 2;
    p.nbk = p.cap ? std::max(2, cdiv(Mo, p.hb)) : 2;
    p.pairs = p.nbk * (p.nbk - 1) / 2;
    p.tiles = p.ap.tiles_y * p.ap.tiles_x;
    p.strips = cdiv(p.tiles, kGramStripTiles);
    p.red_off = ((size_t)p.cap * kGramStride + kGramTilePix) * es + p.halves * h_bytes;
    p.lds = lds_of(p.cap, p.halves);
    p.wg_doubles = (size_t)p.cap * p.cap + p.cap;
    return p;
}

size_t atom_gram_partial_bytes(const Geo &g, int dtype, int group) {
    const GramPlan p = atom_gram_plan(g, dtype, group);
    return align_up((size_t)g.N * p.strips * p.pairs * p.wg_doubles * sizeof(double), 256);
}

int atom_gram_check(const Geo &g, int dtype, int group) {
    const GramPlan p = atom_gram_plan(g, dtype, group);
    if (p.cap == 0) return TNMF_E_UNSUPPORTED;
    if ((size_t)g.N * p.strips * p.pairs > 0x7fffffffull) return TNMF_E_GEOM;
    return TNMF_OK;
}

int launch_atom_gram(const tnmf_hip_ctx *ctx, const Geo &g, int dtype, int group, const void *V, const void *G,
                     const void *R, const void *W, const void *H, double *partials, void *taps, double *a, double *B,
                     hipStream_t s) {
    const int rc = atom_gram_check(g, dtype, group);
    if (rc != TNMF_OK) return rc;
    const GramPlan p = atom_gram_plan(g, dtype, group);
    const size_t blocks = (size_t)g.N * p.strips * p.pairs;
    const int trc = launch_atom_taps(ctx, g, dtype, W, taps, s);
    if (trc != TNMF_OK) return trc;
    const int lrc = with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        if constexpr (sizeof(T) == sizeof(float)) {   // (32 rows of doubles never fit: those kernels do not exist)
            if (p.halves == 2) return launch_gram<T, 2, 2>(ctx, g, p, group, (unsigned)blocks, V, G, R, taps, H, partials, s);
            if (p.cap == 32) return launch_gram<T, 2, 1>(ctx, g, p, group, (unsigned)blocks, V, G, R, taps, H, partials, s);
        }
        if (p.cap != 16) return (int)TNMF_E_UNSUPPORTED;
        return launch_gram<T, 1, 1>(ctx, g, p, group, (unsigned)blocks, V, G, R, taps, H, partials, s);
    });
    if (lrc != TNMF_OK) return lrc;
    TNMF_LAUNCH_CHECK();
    return launch_atom_gram_finalize(g, p, group, partials, a, B, s);
}

int launch_atom_gram_finalize(const Geo &g, const GramPlan &p, int group, const double *partials, double *a, double *B,
                              hipStream_t s) {
    const int Mo = g.M / group;
    const size_t total = (size_t)g.N * Mo * Mo;
    hipLaunchKernelGGL(k_atom_gram_finalize, dim3((unsigned)((total + kAtomThreads - 1) / kAtomThreads)), dim3(kAtomThreads),
                       0, s, total, p, Mo, partials, a, B);
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}
