// api.hip -- the extern "C" surface of libtnmf_hip.so (include/tnmf_hip.h): argument checks, scratch management and
// dispatch between the kernel families.  No torch types, no exceptions, no allocation inside a call once
// tnmf_hip_ctx_reserve() has sized the scratch.
#include <cstdlib>
#include <cstring>
#include <new>
#include <algorithm>
#include <vector>

#include "atom_beta.h"
#include "atom_gram.h"
#include "correlogram.h"
#include "sources.h"
#include "atoms.h"
#include "beta.h"
#include "events.h"
#include "solve.h"
#include "covariance.h"
#include "fft.h"
#include "generic.h"
#include "mfma.h"
#include "modes.h"
#include "patches.h"
#include "peaks.h"
#include "split.h"
#include "triggered.h"
#include "volume.h"

namespace {

int to_geo(const tnmf_hip_geom *in, Geo *g) {
    if (!in) return TNMF_E_NULL;
    if (in->dtype != 0 && in->dtype != 1) return TNMF_E_DTYPE;
    if (in->ndim != 1 && in->ndim != 2) return TNMF_E_GEOM;
    g->N = in->N;
    g->M = in->M;
    g->C = in->C;
    if (in->ndim == 1) {
        g->Dy = 1;
        g->Dx = in->D[0];
        g->Ay = 1;
        g->Ax = in->A[0];
    } else {
        g->Dy = in->D[0];
        g->Dx = in->D[1];
        g->Ay = in->A[0];
        g->Ax = in->A[1];
    }
    if (g->N < 0 || g->M <= 0 || g->C <= 0 || g->Dy <= 0 || g->Dx <= 0 || g->Ay <= 0 || g->Ax <= 0)
        return TNMF_E_GEOM;
    g->Hy = g->Dy + g->Ay - 1;
    g->Hx = g->Dx + g->Ax - 1;
    g->Hs = in->h_row_stride > 0 ? in->h_row_stride : g->Hx;
    if (g->Hs < g->Hx) return TNMF_E_GEOM;
    return TNMF_OK;
}

// what the H update adds to its denominator (TransformInvariantNMF.py:227-230)
inline double reg_of(double eps, double sparsity) { return eps + (sparsity > 0 ? sparsity : 0.0); }
// the weight of the other atoms' gradients in the lateral term (TransformInvariantNMF.py:266-268)
inline double cross_weight(double cross_inhibition, int M) {
    return cross_inhibition > 0 && M > 1 ? cross_inhibition / (M - 1) : 0.0;
}

// the operation list of a schedule on N samples, whole, before anything runs: kinds and slices (the W update names no samples)
int check_ops(const tnmf_hip_op *ops, int n_ops, int N) {
    for (int i = 0; i < n_ops; ++i) {
        if (ops[i].kind != TNMF_OP_UPDATE_H && ops[i].kind != TNMF_OP_GRAD_W && ops[i].kind != TNMF_OP_APPLY_W)
            return TNMF_E_UNSUPPORTED;
        if (ops[i].kind == TNMF_OP_APPLY_W) continue;
        if (ops[i].n0 < 0 || ops[i].n1 < ops[i].n0 || ops[i].n1 > N) return TNMF_E_GEOM;
    }
    return TNMF_OK;
}

// three shift axes (volumes): a kernel family of its own (volume.hip); H is C-contiguous there
inline bool is_vol(const tnmf_hip_geom *in) { return in && in->ndim == 3; }

int to_vol(const tnmf_hip_geom *in, Vol *v) {
    if (!in) return TNMF_E_NULL;
    if (in->dtype != 0 && in->dtype != 1) return TNMF_E_DTYPE;
    v->N = in->N;
    v->M = in->M;
    v->C = in->C;
    if (v->N < 0 || v->M <= 0 || v->C <= 0) return TNMF_E_GEOM;
    for (int i = 0; i < 3; ++i) {
        v->D[i] = in->D[i];
        v->A[i] = in->A[i];
        if (v->D[i] <= 0 || v->A[i] <= 0) return TNMF_E_GEOM;
        v->H[i] = v->D[i] + v->A[i] - 1;
    }
    if (in->h_row_stride > 0 && in->h_row_stride != v->H[2]) return TNMF_E_STRIDE;
    return TNMF_OK;
}
inline size_t vol_vox(const Vol &v) { return (size_t)v.D[0] * v.D[1] * v.D[2]; }
inline size_t vol_hvox(const Vol &v) { return (size_t)v.H[0] * v.H[1] * v.H[2]; }
inline size_t vol_avox(const Vol &v) { return (size_t)v.A[0] * v.A[1] * v.A[2]; }
// the dictionary of a volume problem as the (M, C, flattened atom) rows the normalisation kernel works on
inline Geo vol_dict_geo(const Vol &v) {
    Geo g = {};
    g.N = v.N;
    g.M = v.M;
    g.C = v.C;
    g.Ay = v.A[0] * v.A[1];
    g.Ax = v.A[2];
    return g;
}

// scratch layout: [R (N*C*D elements)] [split-K partials (doubles)] [energy partials + result (doubles)]
struct Scratch {
    size_t r_off, r_bytes;
    size_t part_off, part_bytes;
    size_t red_off, red_bytes;
    size_t total;
    int P;
};

Scratch plan_scratch(const tnmf_hip_ctx *ctx, const Geo &g, int dtype) {
    Scratch s;
    s.r_off = 0;
    s.r_bytes = align_up((size_t)g.N * g.C * g.Dy * g.Dx * esize(dtype), 256);
    int P = generic_corr_H_chunks(ctx, g);
    const int Pm = mfma_corr_H_chunks(ctx, g);
    if (Pm > P) P = Pm;
    s.P = P;
    s.part_off = s.r_off + s.r_bytes;
    s.part_bytes = align_up((size_t)P * g.M * g.C * g.Ay * g.Ax * 2 * sizeof(double), 256);
    s.red_off = s.part_off + s.part_bytes;
    s.red_bytes = align_up((size_t)(kEnergyPartials + 8) * sizeof(double), 256);
    s.total = s.red_off + s.red_bytes;
    return s;
}

int ensure_buffer(void **buf, size_t *have, size_t bytes, bool slack);

int ensure_scratch(tnmf_hip_ctx *ctx, size_t bytes) { return ensure_buffer(&ctx->ws, &ctx->ws_bytes, bytes, true); }
int ensure_hwork(tnmf_hip_ctx *ctx, size_t bytes) { return ensure_buffer(&ctx->hw, &ctx->hw_bytes, bytes, false); }

int ensure_buffer(void **buf, size_t *have, size_t bytes, bool slack) {
    if (bytes <= *have) return TNMF_OK;
    // the larger buffer is allocated BEFORE the current one is released, so a failure leaves the working one in place;
    // when both do not fit side by side the old order (release, then allocate) is tried once
    const size_t want = align_up(bytes + (slack ? bytes / 8 : 0), 1 << 20);
    void *bigger = nullptr;
    if (hipMalloc(&bigger, want) != hipSuccess) {
        (void)hipGetLastError();
        bigger = nullptr;
        if (!*buf) return TNMF_E_WORKSPACE;
    }
    if (*buf) {
        TNMF_HIP_TRY(hipDeviceSynchronize());
        TNMF_HIP_TRY(hipFree(*buf));
        *buf = nullptr;
        *have = 0;
    }
    if (!bigger && hipMalloc(&bigger, want) != hipSuccess) {
        (void)hipGetLastError();
        return TNMF_E_WORKSPACE;
    }
    *buf = bigger;
    *have = want;
    return TNMF_OK;
}

inline char *ws_at(tnmf_hip_ctx *ctx, size_t off) { return static_cast<char *>(ctx->ws) + off; }

enum Prim { kReconstruct, kCorrW, kCorrH };

// FFT family for reconstruct and the W gradient (the hybrid dispatch): forced by TNMF_PATH_HYBRID wherever the family
// covers the shape; chosen by TNMF_PATH_AUTO for float32 problems that are not tiny (the family costs ~20 launches per iteration).
// Measured: W, H and the energy stay as close to the float64 oracle as with the direct kernels alone,
// because the H gradient -- the only place where float32 transform error matters -- stays on the direct kernels.
// A mini-batch slice decides by its OWN size: small batches of a large resident problem (the stochastic schedules with
// batch_size 3) take the direct kernels -- 6 launches per batch step instead of ~40 -- and find the resident problem's
// row-padded H readable there: the generic kernels and the split kernel take the row stride, only the f32 MFMA kernels
// want C-contiguous rows and are skipped for padded ones.
bool use_fft_hybrid(const tnmf_hip_ctx *ctx, const Geo &g, int dtype) {
    if (ctx->path == TNMF_PATH_HYBRID) return fft_has(g, dtype);
    if (ctx->path != TNMF_PATH_AUTO || dtype != 0 || !fft_has(g, dtype)) return false;
    // measured crossover against the direct kernels at 128x128 samples, 16 atoms: one sample (2^18 entries) is a tie,
    // two are 20 % ahead, 64 samples (config 2) 1.9x
    return (size_t)g.N * g.M * g.Hy * g.Hx >= ((size_t)1 << 19);
}

// H gradient on the bf16 matrix cores with exact 3 x bf16 operand splits: forced by TNMF_PATH_SPLIT, default under AUTO
// and HYBRID (tnmf_hip_ctx_set_split), never under MFMA (the exact-f32 family), GENERIC or FFT.
bool use_split(const tnmf_hip_ctx *ctx, const Geo &g, int dtype) {
    if (ctx->path == TNMF_PATH_SPLIT) return split_has_corr_W(g, dtype);
    if (ctx->path != TNMF_PATH_AUTO && ctx->path != TNMF_PATH_HYBRID) return false;
    // (tiny calls -- the batches of the stochastic schedules -- are launch latency: the split kernel needs an operand
    // preparation launch in front of it, the generic kernel does not)
    if (ctx->path == TNMF_PATH_AUTO && (size_t)g.N * g.M * g.Hy * g.Hx < ((size_t)1 << 16)) return false;
    return ctx->split && split_has_corr_W(g, dtype, true);
}

bool use_mfma(const tnmf_hip_ctx *ctx, const Geo &g, int dtype, Prim prim) {
    if (ctx->path == TNMF_PATH_GENERIC || ctx->path == TNMF_PATH_FFT) return false;   // (FFT never gets here)
    switch (prim) {
        case kReconstruct: return mfma_has_reconstruct(g, dtype);
        case kCorrW: return mfma_has_corr_W(g, dtype);
        default: return mfma_has_corr_H(g, dtype);
    }
}

#define ENTER(ctx, geom)                                   \
    if (!(ctx)) return TNMF_E_NULL;                        \
    Geo g;                                                 \
    {                                                      \
        const int _rc = to_geo((geom), &g);                \
        if (_rc != TNMF_OK) return _rc;                    \
    }                                                      \
    const int dtype = (geom)->dtype;                       \
    hipStream_t s = static_cast<hipStream_t>(stream);      \
    TNMF_HIP_TRY(hipSetDevice((ctx)->device));

#define CHECK(rc_expr)                  \
    do {                                \
        const int _rc = (rc_expr);      \
        if (_rc != TNMF_OK) return _rc; \
    } while (0)

#define VOL_ENTER(ctx, geom)                               \
    if (!(ctx)) return TNMF_E_NULL;                        \
    Vol v;                                                 \
    {                                                      \
        const int _rc = to_vol((geom), &v);                \
        if (_rc != TNMF_OK) return _rc;                    \
    }                                                      \
    const int dtype = (geom)->dtype;                       \
    hipStream_t s = static_cast<hipStream_t>(stream);      \
    TNMF_HIP_TRY(hipSetDevice((ctx)->device));             \
    (ctx)->last_path = "volume";

// scratch of a volume call: [R of the slice | energy partials + result | partial sums of the W gradient]
int vol_scratch(tnmf_hip_ctx *ctx, const Vol &v, int dtype, void **R, double **red, double **part = nullptr,
                int *P = nullptr, size_t extra = 0) {
    const size_t r_bytes = align_up((size_t)v.N * v.C * vol_vox(v) * esize(dtype), 256);
    const size_t e_bytes = align_up((size_t)(kEnergyPartials + 8) * sizeof(double), 256);
    const int chunks = vol_corr_H_chunks(ctx, v);
    const size_t p_bytes = align_up((size_t)chunks * v.M * v.C * vol_avox(v) * 2 * sizeof(double), 256);
    const int rc = ensure_scratch(ctx, r_bytes + e_bytes + p_bytes + extra);   // (extra: behind the partial sums)
    if (rc != TNMF_OK) return rc;
    if (R) *R = ws_at(ctx, 0);
    if (red) *red = reinterpret_cast<double *>(ws_at(ctx, r_bytes));
    if (part) *part = reinterpret_cast<double *>(ws_at(ctx, r_bytes + e_bytes));
    if (P) *P = chunks;
    return TNMF_OK;
}

int do_reconstruct(tnmf_hip_ctx *ctx, const Geo &g, int dtype, const void *W, const void *H, void *R, hipStream_t s) {
    if (g.N == 0) return TNMF_OK;
    // the FFT family serves non-negative factorisations: outputs that are non-negative by construction are clamped
    if (ctx->path == TNMF_PATH_FFT || use_fft_hybrid(ctx, g, dtype)) {
        const int rc = fft_reconstruct(ctx, g, dtype, W, H, R, true, s);
        // AUTO only chose the family for speed: when its workspace does not fit, the direct kernels still do the job
        if (!(rc == TNMF_E_WORKSPACE && ctx->path == TNMF_PATH_AUTO)) return rc;
    }
    // (the f32 MFMA kernels read C-contiguous H; the generic kernels take the row stride)
    if (g.Hs == g.Hx && use_mfma(ctx, g, dtype, kReconstruct)) {
        ctx->last_path = "mfma";
        return mfma_reconstruct(ctx, g, (const float *)W, (const float *)H, (float *)R, s);
    }
    if (ctx->path == TNMF_PATH_MFMA) return g.Hs != g.Hx ? TNMF_E_STRIDE : TNMF_E_UNSUPPORTED;
    ctx->last_path = "generic";
    return generic_reconstruct(ctx, g, dtype, W, H, R, s);
}

// extra (fused only, may be NULL): a further term of the denominator, laid out like H (the lateral inhibition terms).
// Kernel families without an epilogue for it answer TNMF_E_UNSUPPORTED / TNMF_E_STRIDE before touching anything; the
// caller then takes the unfused gradient and launch_mu_update_extra.
int do_corr_W(tnmf_hip_ctx *ctx, const Geo &g, int dtype, const void *V, const void *R, const void *W, void *Hio,
              void *neg, void *pos, bool fused, double reg, hipStream_t s, const void *extra = nullptr) {
    if (g.N == 0) return TNMF_OK;
    if (extra && (!fused || ctx->path == TNMF_PATH_FFT)) return TNMF_E_UNSUPPORTED;
    // (AUTO never takes the FFT family here, although it is the faster one for heavy atoms -- 46 vs 53 ms per iteration
    // at config 5's shard, C*Ay*Ax = 768: its float32 transform noise leaves 4e-4 of max|H| in the activations, and the
    // parity bar of the default path is 1e-5 on W AND H.  path = FFT is the opt-in.)
    if (ctx->path == TNMF_PATH_FFT)
        return fused ? fft_update_H(ctx, g, dtype, V, R, W, Hio, reg, s) : fft_grad_H(ctx, g, dtype, V, R, W, neg, pos, s);
    if (fused) fft_invalidate_H(ctx, g, dtype, Hio);   // the direct kernels are about to change H: its cached spectra are stale
    if (use_split(ctx, g, dtype)) {
        const int rc = split_corr_W(ctx, g, (const float *)V, (const float *)R, (const float *)W, (float *)Hio,
                                    (float *)neg, (float *)pos, fused, (float)reg, s, (const float *)extra);
        if (rc == TNMF_OK) ctx->last_path = "split";
        if (rc != TNMF_E_UNSUPPORTED) return rc;
    }
    if ((!fused || g.Hs == g.Hx) && use_mfma(ctx, g, dtype, kCorrW)) {
        if (extra) return TNMF_E_UNSUPPORTED;   // (the f32 MFMA kernel has no extra-term epilogue)
        ctx->last_path = "mfma";
        return mfma_corr_W(ctx, g, (const float *)V, (const float *)R, (const float *)W, (float *)Hio, (float *)neg,
                           (float *)pos, fused, (float)reg, s);
    }
    if (ctx->path == TNMF_PATH_MFMA || ctx->path == TNMF_PATH_SPLIT)
        return fused && g.Hs != g.Hx ? TNMF_E_STRIDE : TNMF_E_UNSUPPORTED;   // (nothing has been written)
    ctx->last_path = "generic";
    return generic_corr_W(ctx, g, dtype, V, R, W, Hio, neg, pos, fused, reg, s, extra);
}

// the split-K kernel of the direct families alone: partials[P][M*C][Ay*Ax][2] (doubles), P returned.  g.N > 0.
int do_corr_H_partials(tnmf_hip_ctx *ctx, const Geo &g, int dtype, const void *V, const void *R, const void *H,
                       double *partials, int *P_out, hipStream_t s) {
    if (g.Hs == g.Hx && use_mfma(ctx, g, dtype, kCorrH)) {
        ctx->last_path = "mfma";
        *P_out = mfma_corr_H_chunks(ctx, g);
        return mfma_corr_H(ctx, g, (const float *)V, (const float *)R, (const float *)H, partials, *P_out, s);
    }
    if (ctx->path == TNMF_PATH_MFMA) return g.Hs != g.Hx ? TNMF_E_STRIDE : TNMF_E_UNSUPPORTED;
    ctx->last_path = "generic";
    *P_out = generic_corr_H_chunks(ctx, g);
    return generic_corr_H(ctx, g, dtype, V, R, H, partials, *P_out, s);
}

bool corr_H_on_fft(const tnmf_hip_ctx *ctx, const Geo &g, int dtype) {
    return ctx->path == TNMF_PATH_FFT || use_fft_hybrid(ctx, g, dtype);
}

int do_corr_H(tnmf_hip_ctx *ctx, const Geo &g, int dtype, const Scratch &sc, const void *V, const void *R,
              const void *H, void *neg, void *pos, hipStream_t s) {
    double *partials = reinterpret_cast<double *>(ws_at(ctx, sc.part_off));
    int P;
    if (g.N == 0) {
        // empty slice: the sums are zero
        TNMF_HIP_TRY(hipMemsetAsync(neg, 0, (size_t)g.M * g.C * g.Ay * g.Ax * esize(dtype), s));
        TNMF_HIP_TRY(hipMemsetAsync(pos, 0, (size_t)g.M * g.C * g.Ay * g.Ax * esize(dtype), s));
        return TNMF_OK;
    }
    if (corr_H_on_fft(ctx, g, dtype)) {
        const int rc = fft_grad_W(ctx, g, dtype, V, R, H, neg, pos, true, s);
        if (!(rc == TNMF_E_WORKSPACE && ctx->path == TNMF_PATH_AUTO)) return rc;
    }
    CHECK(do_corr_H_partials(ctx, g, dtype, V, R, H, partials, &P, s));
    return finalize_corr_H(g, dtype, partials, P, neg, pos, s);
}


// beta-divergence (beta != NULL, *beta != 2) and weighted (G != NULL, any beta) steps: the fields of R (ctx->qb receives Q,
// R is overwritten with P); *Q_out = Q.  Q sits at a fixed address with new contents every call: the FFT family is told
// never to take it for the samples it caches.
int beta_fields_of(tnmf_hip_ctx *ctx, const Geo &g, int dtype, const double *beta, double eps, const void *V,
                   const void *G, void *R, const void **Q_out, hipStream_t s) {
    const size_t n = (size_t)g.N * g.C * g.Dy * g.Dx;
    CHECK(ensure_buffer(&ctx->qb, &ctx->qb_bytes, align_up(n * esize(dtype), 256), false));
    ctx->fft.V_volatile = ctx->qb;
    CHECK(launch_beta_fields(ctx, dtype, beta ? *beta : 2.0, eps, V, G, R, ctx->qb, R, n, s));
    *Q_out = ctx->qb;
    return TNMF_OK;
}

// the per-sample objective of (V, R[, G]): N samples of L elements each into out (N doubles on the device).  beta == NULL:
// the Frobenius objective (weighted with G != NULL).  Asynchronous on s.
int sample_objective_of(tnmf_hip_ctx *ctx, int dtype, const double *beta, double eps, const void *V, const void *G,
                        const void *R, size_t N, size_t L, double *out, hipStream_t s) {
    const size_t B = objective_blocks(L);
    if (B > 1) CHECK(ensure_buffer(&ctx->ob, &ctx->ob_bytes, align_up(N * B * sizeof(double), 256), false));
    return launch_sample_objective(dtype, beta ? *beta : 2.0, eps, V, G, R, N, L, static_cast<double *>(ctx->ob), out, s);
}

// the objective tap of the H half steps (tnmf_hip_ctx_set_objective_tap): R holds the reconstruction of the activations
// as they were passed in; reads only, so the step computes what it computes without the tap
inline int tap_objective(tnmf_hip_ctx *ctx, int dtype, const double *beta, double eps, const void *V, const void *G,
                         const void *R, size_t N, size_t L, hipStream_t s) {
    if (!ctx->obj_tap) return TNMF_OK;
    return sample_objective_of(ctx, dtype, beta, eps, V, G, R, N, L, ctx->obj_tap, s);
}

static_assert(kBetaPartials <= kEnergyPartials, "the energy words of the scratch hold the beta partials");

inline bool beta_ok(double beta) { return beta == beta && beta - beta == 0.0; }   // finite

// ---- three shift axes: the entry points below hand over to these (same argument meaning, C-contiguous H)
int vol_api_reconstruct(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *W, const void *H, void *R, void *stream) {
    VOL_ENTER(ctx, geom);
    if (!W || (v.N > 0 && (!H || !R))) return TNMF_E_NULL;
    return vol_reconstruct(v, dtype, W, H, R, s);
}

int vol_api_grad_H(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *R_or_null, const void *W,
                   const void *H, void *neg, void *pos, void *stream) {
    VOL_ENTER(ctx, geom);
    if (!W || (v.N > 0 && (!V || !neg || !pos))) return TNMF_E_NULL;
    const void *R = R_or_null;
    if (!R && v.N > 0) {
        if (!H) return TNMF_E_NULL;
        void *Rs;
        CHECK(vol_scratch(ctx, v, dtype, &Rs, nullptr));
        CHECK(vol_reconstruct(v, dtype, W, H, Rs, s));
        R = Rs;
    }
    return vol_corr_W(v, dtype, V, R, W, nullptr, neg, pos, false, 0.0, s);
}

int vol_api_grad_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *R_scratch, int r_is_valid,
                   const void *W, const void *H, void *neg, void *pos, void *stream) {
    VOL_ENTER(ctx, geom);
    if (!neg || !pos || (v.N > 0 && (!V || !H))) return TNMF_E_NULL;
    const void *R = R_scratch;
    void *Rws;
    double *part;
    int P;
    CHECK(vol_scratch(ctx, v, dtype, &Rws, nullptr, &part, &P));
    if (v.N > 0 && !r_is_valid) {
        if (!W) return TNMF_E_NULL;
        void *Rs = R_scratch ? const_cast<void *>(R_scratch) : Rws;
        CHECK(vol_reconstruct(v, dtype, W, H, Rs, s));
        R = Rs;
    }
    return vol_corr_H(v, dtype, V, R, H, neg, pos, part, P, s);
}

int vol_api_energy(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *W, const void *H,
                   double *out_host, void *stream) {
    VOL_ENTER(ctx, geom);
    if (!out_host) return TNMF_E_NULL;
    *out_host = 0.0;
    if (v.N == 0) return TNMF_OK;
    if (!V || !W || !H) return TNMF_E_NULL;
    void *Rs;
    double *red;
    CHECK(vol_scratch(ctx, v, dtype, &Rs, &red));
    CHECK(vol_reconstruct(v, dtype, W, H, Rs, s));
    CHECK(launch_half_sqdiff(ctx, dtype, V, Rs, (size_t)v.N * v.C * vol_vox(v), red, red + kEnergyPartials, s));
    TNMF_HIP_TRY(hipMemcpyAsync(out_host, red + kEnergyPartials, sizeof(double), hipMemcpyDeviceToHost, s));
    TNMF_HIP_TRY(hipStreamSynchronize(s));
    return TNMF_OK;
}

int vol_api_update_H(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *W, void *H_inout,
                     void *R_scratch, int r_is_valid, double eps, double sparsity, void *stream) {
    VOL_ENTER(ctx, geom);
    if (v.N == 0) return TNMF_OK;
    if (!V || !W || !H_inout) return TNMF_E_NULL;
    void *Rs = R_scratch;
    if (!Rs) {
        if (r_is_valid) return TNMF_E_NULL;
        CHECK(vol_scratch(ctx, v, dtype, &Rs, nullptr));
    }
    if (!r_is_valid) CHECK(vol_reconstruct(v, dtype, W, H_inout, Rs, s));
    CHECK(tap_objective(ctx, dtype, nullptr, eps, V, nullptr, Rs, (size_t)v.N, (size_t)v.C * vol_vox(v), s));
    const double reg = reg_of(eps, sparsity);
    return vol_corr_W(v, dtype, V, Rs, W, H_inout, nullptr, nullptr, true, reg, s);
}

// TransformInvariantNMF._update_H in full for volumes: the lateral terms (three passes of the 1-D convolution, then
// k_vol_lateral) and the padded modes (pad, 'valid' kernels, fold) on work arrays of the library, one update kernel
int vol_api_update_H_ex(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *V, const void *W,
                        void *H_inout, void *R_scratch, double eps, double sparsity, double inhibition,
                        double cross_inhibition, const double *const kern[3], const int klen[3], void *stream) {
    VOL_ENTER(ctx, geom);
    if (!mode_known(mode)) return TNMF_E_UNSUPPORTED;
    if (v.N == 0) return TNMF_OK;
    if (!V || !W || !H_inout) return TNMF_E_NULL;
    if (inhibition < 0 || cross_inhibition < 0) return TNMF_E_GEOM;
    const bool lateral = inhibition > 0 || cross_inhibition > 0;
    if (lateral)
        for (int i = 0; i < 3; ++i) {
            if (!kern[i]) return TNMF_E_NULL;
            if (klen[i] < 1 || klen[i] > kMaxTaps || !(klen[i] & 1)) return TNMF_E_UNSUPPORTED;
        }
    const double reg = reg_of(eps, sparsity);
    const double xc = cross_weight(cross_inhibition, v.M);
    if (mode == TNMF_MODE_VALID && !lateral)
        return vol_api_update_H(ctx, geom, V, W, H_inout, R_scratch, 0, eps, sparsity, stream);
    int S[3];
    for (int i = 0; i < 3; ++i) {
        S[i] = mode_shift_len(mode, v.D[i], v.A[i]);
        if (S[i] < 1) return TNMF_E_GEOM;
    }
    const size_t es = esize(dtype), planes = (size_t)v.N * v.M;
    const size_t svox = (size_t)S[0] * S[1] * S[2];
    const size_t nS = align_up(planes * svox * es, 256), nP = align_up(planes * vol_hvox(v) * es, 256);
    // work arrays: [G0 | G1] (lateral), [neg | pos] in the mode's shape, and for the padded modes [Hp | negp | posp]
    const size_t lat = lateral ? 2 * nS : 0, pad = mode == TNMF_MODE_VALID ? 0 : 3 * nP;
    CHECK(ensure_hwork(ctx, lat + 2 * nS + pad));
    char *G0 = static_cast<char *>(ctx->hw), *G1 = G0 + nS;
    char *neg = static_cast<char *>(ctx->hw) + lat, *pos = neg + nS;
    char *Hp = pos + nS, *negp = Hp + nP, *posp = negp + nP;
    void *Rs = R_scratch;
    if (!Rs) CHECK(vol_scratch(ctx, v, dtype, &Rs, nullptr));
    const void *E = nullptr;
    if (lateral) {
        // first shift axis first (_NumPyBackend.py:60-62): H -> G0 -> G1 -> G0
        CHECK(launch_convolve_axis(ctx, dtype, H_inout, G0, planes, S[0], S[1] * S[2], kern[0], klen[0], s));
        CHECK(launch_convolve_axis(ctx, dtype, G0, G1, planes * S[0], S[1], S[2], kern[1], klen[1], s));
        CHECK(launch_convolve_axis(ctx, dtype, G1, G0, planes * S[0] * S[1], S[2], 1, kern[2], klen[2], s));
        CHECK(vol_lateral(ctx, dtype, (size_t)v.N, v.M, svox, G0, H_inout, inhibition, xc, s));
        E = G0;
    }
    if (mode == TNMF_MODE_VALID) {
        CHECK(vol_reconstruct(v, dtype, W, H_inout, Rs, s));
        CHECK(tap_objective(ctx, dtype, nullptr, eps, V, nullptr, Rs, (size_t)v.N, (size_t)v.C * vol_vox(v), s));
        CHECK(vol_corr_W(v, dtype, V, Rs, W, nullptr, neg, pos, false, 0.0, s));
    } else {
        CHECK(vol_pad_fold(ctx, v, dtype, mode, false, H_inout, Hp, s));
        CHECK(vol_reconstruct(v, dtype, W, Hp, Rs, s));
        CHECK(tap_objective(ctx, dtype, nullptr, eps, V, nullptr, Rs, (size_t)v.N, (size_t)v.C * vol_vox(v), s));
        CHECK(vol_corr_W(v, dtype, V, Rs, W, nullptr, negp, posp, false, 0.0, s));
        CHECK(vol_pad_fold(ctx, v, dtype, mode, true, negp, neg, s));
        CHECK(vol_pad_fold(ctx, v, dtype, mode, true, posp, pos, s));
    }
    // H <- H * neg / (pos + E + reg): every array is C-contiguous in the mode's shift shape (rows of S[2] elements)
    return launch_mu_update_extra(ctx, dtype, H_inout, neg, pos, E, planes * S[0] * S[1], S[2], S[2], reg, s);
}

// a list of operations on slices of the resident volume problem (tnmf_hip_run_schedule): one host call, one launch chain
int vol_api_run_schedule(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, void *W_inout, void *H_inout,
                         void *R_scratch, void *acc, const tnmf_hip_op *ops, int n_ops, double eps, double sparsity,
                         void *stream) {
    VOL_ENTER(ctx, geom);
    if (n_ops < 0 || (n_ops > 0 && !ops)) return TNMF_E_NULL;
    if (!V || !W_inout || !H_inout || !acc) return TNMF_E_NULL;
    const size_t es = esize(dtype);
    const size_t vs = (size_t)v.C * vol_vox(v) * es, hs = (size_t)v.M * vol_hvox(v) * es;
    const size_t wn = (size_t)v.M * v.C * vol_avox(v);
    CHECK(check_ops(ops, n_ops, v.N));
    int nmax = 0;
    for (int i = 0; i < n_ops; ++i)
        if (ops[i].kind != TNMF_OP_APPLY_W && ops[i].n1 - ops[i].n0 > nmax) nmax = ops[i].n1 - ops[i].n0;
    const double reg = reg_of(eps, sparsity);
    // scratch for the largest slice: [R | energy words | partial sums of the W gradient], and one gradient behind it
    Vol vmax = v;
    vmax.N = nmax;
    void *Rws;
    double *part;
    int Pmax;
    CHECK(vol_scratch(ctx, vmax, dtype, &Rws, nullptr, &part, &Pmax, align_up(2 * wn * es, 256)));
    char *grad = reinterpret_cast<char *>(part) + align_up((size_t)Pmax * wn * 2 * sizeof(double), 256);
    const Geo dict = vol_dict_geo(v);
    for (int i = 0; i < n_ops; ++i) {
        const tnmf_hip_op &op = ops[i];
        Vol vs_ = v;
        vs_.N = op.n1 - op.n0;
        const char *Vb = static_cast<const char *>(V) + (size_t)op.n0 * vs;
        char *Hb = static_cast<char *>(H_inout) + (size_t)op.n0 * hs;
        void *Rb = R_scratch ? static_cast<void *>(static_cast<char *>(R_scratch) + (size_t)op.n0 * vs) : Rws;
        switch (op.kind) {
            case TNMF_OP_UPDATE_H:
                if (vs_.N == 0) break;
                CHECK(vol_reconstruct(vs_, dtype, W_inout, Hb, Rb, s));
                CHECK(vol_corr_W(vs_, dtype, Vb, Rb, W_inout, Hb, nullptr, nullptr, true, reg, s));
                break;
            case TNMF_OP_GRAD_W: {
                if (vs_.N > 0) CHECK(vol_reconstruct(vs_, dtype, W_inout, Hb, Rb, s));
                int P = vol_corr_H_chunks(ctx, vs_);
                if (P > Pmax) P = Pmax;   // (the chunk count grows with the slice: never beyond the largest one's)
                CHECK(vol_corr_H(vs_, dtype, Vb, Rb, Hb, grad, grad + wn * es, part, P, s));
                CHECK(launch_axpby(ctx, dtype, acc, grad, op.a, op.b, 2 * wn, s));
                break;
            }
            case TNMF_OP_APPLY_W: {
                char *np = static_cast<char *>(acc);
                CHECK(launch_apply_normalize_W(dict, dtype, W_inout, np, np + wn * es, eps, true, s));
                break;
            }
            default: return TNMF_E_UNSUPPORTED;
        }
    }
    return TNMF_OK;
}

int vol_api_pad_fold(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, bool fold, const void *in, void *out,
                     void *stream) {
    VOL_ENTER(ctx, geom);
    if (!mode_known(mode)) return TNMF_E_UNSUPPORTED;
    if (v.N > 0 && (!in || !out)) return TNMF_E_NULL;
    return vol_pad_fold(ctx, v, dtype, mode, fold, in, out, s);
}

}  // namespace

// ---- the context's side of the atom entries that live beside their kernels (atom_beta.h)
int atom_entry_geo(const tnmf_hip_geom *geom, Geo *g) {
    if (!geom) return TNMF_E_NULL;
    if (is_vol(geom)) return TNMF_E_UNSUPPORTED;
    return to_geo(geom, g);
}

int atom_entry_buffers(tnmf_hip_ctx *ctx, const Geo &g, int dtype, size_t work_bytes, const void *W, const void *H,
                       const void **R, void **work, hipStream_t s) {
    CHECK(ensure_buffer(&ctx->ob, &ctx->ob_bytes, work_bytes, false));
    *work = ctx->ob;
    if (!*R) {
        const Scratch sc = plan_scratch(ctx, g, dtype);
        CHECK(ensure_scratch(ctx, sc.total));
        void *Rs = ws_at(ctx, sc.r_off);
        CHECK(do_reconstruct(ctx, g, dtype, W, H, Rs, s));
        *R = Rs;
    }
    return TNMF_OK;
}

extern "C" {

int tnmf_hip_abi_version(void) { return TNMF_HIP_ABI_VERSION; }

int tnmf_hip_ctx_h_row_stride(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int *stride_out) {
    if (!ctx || !stride_out) return TNMF_E_NULL;
    if (is_vol(geom)) {   // volumes: C-contiguous
        Vol v;
        const int vrc = to_vol(geom, &v);
        if (vrc != TNMF_OK) return vrc;
        *stride_out = v.H[2];
        return TNMF_OK;
    }
    Geo g;
    const int rc = to_geo(geom, &g);
    if (rc != TNMF_OK) return rc;
    const int dtype = geom->dtype;
    *stride_out = g.Hx;
    // padded rows pay where the split kernel reads and writes H in 32-pixel tiles and every other reader of H is the
    // FFT family's row transform; a whole number of 128-byte lines per row
    const bool hybrid = ctx->path == TNMF_PATH_AUTO || ctx->path == TNMF_PATH_HYBRID;
    if (hybrid && g.N > 0 && use_fft_hybrid(ctx, g, dtype) && use_split(ctx, g, dtype))
        *stride_out = (int)align_up((size_t)g.Hx, 32);
    return TNMF_OK;
}

const char *tnmf_hip_strerror(int code) {
    switch (code) {
        case TNMF_OK: return "ok";
        case TNMF_E_NULL: return "tnmf_hip: required pointer is NULL";
        case TNMF_E_GEOM: return "tnmf_hip: bad geometry";
        case TNMF_E_DTYPE: return "tnmf_hip: dtype must be 0 (f32) or 1 (f64)";
        case TNMF_E_WORKSPACE: return "tnmf_hip: scratch allocation failed";
        case TNMF_E_UNSUPPORTED: return "tnmf_hip: shape not supported by the selected kernel family";
        case TNMF_E_STRIDE: return "tnmf_hip: this kernel family wants C-contiguous H (h_row_stride == shift width)";
        default: break;
    }
    if (code > 0) return hipGetErrorString(static_cast<hipError_t>(code));
    return "tnmf_hip: unknown error";
}

int tnmf_hip_ctx_create(int device_id, tnmf_hip_ctx **out) {
    if (!out) return TNMF_E_NULL;
    *out = nullptr;
    TNMF_HIP_TRY(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    TNMF_HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    {
        int rc = mfma_prepare_device();   // per device, hence per context
        if (rc == TNMF_OK) rc = split_prepare_device();
        if (rc != TNMF_OK) return rc;
    }
    tnmf_hip_ctx *ctx = new (std::nothrow) tnmf_hip_ctx();
    if (!ctx) return TNMF_E_WORKSPACE;
    ctx->device = device_id;
    ctx->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    ctx->path = TNMF_PATH_AUTO;
    ctx->last_path = "none";
    {
        const char *ab = tnmf_diag_env("TNMF_HIP_ABLATE");   // -DTNMF_DIAG builds only; nullptr in the product
        ctx->ablate = ab ? atoi(ab) : 0;
    }
    ctx->ws = nullptr;
    ctx->ws_bytes = 0;
    ctx->split = 1;
    ctx->wimg = nullptr;
    ctx->wimg_bytes = 0;
    ctx->fft = FftState();
    *out = ctx;
    return TNMF_OK;
}

int tnmf_hip_ctx_destroy(tnmf_hip_ctx *ctx) {
    if (!ctx) return TNMF_OK;
    int rc = TNMF_OK;
    if (ctx->ws || ctx->fft.ws || ctx->wimg || ctx->hw || ctx->qb || ctx->ob) {
        (void)hipSetDevice(ctx->device);
        (void)hipDeviceSynchronize();
    }
    fft_release(ctx);
    split_release(ctx);
    if (ctx->hw) (void)hipFree(ctx->hw);
    if (ctx->qb) (void)hipFree(ctx->qb);
    if (ctx->ob) (void)hipFree(ctx->ob);
    for (int i = 0; i < tnmf_hip_ctx::kOpSlots; ++i) {
        if (ctx->ops_done[i]) (void)hipEventDestroy(ctx->ops_done[i]);
        if (ctx->ops_pinned[i]) (void)hipHostFree(ctx->ops_pinned[i]);
    }
    if (ctx->ws) {
        const hipError_t e = hipFree(ctx->ws);
        if (e != hipSuccess) rc = (int)e;
    }
    delete ctx;
    return rc;
}

int tnmf_hip_ctx_reserve(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom) {
    void *stream = nullptr;
    if (is_vol(geom)) {
        VOL_ENTER(ctx, geom);
        (void)s;
        return vol_scratch(ctx, v, dtype, nullptr, nullptr);
    }
    ENTER(ctx, geom);
    (void)s;
    if (g.N > 0 && ctx->path == TNMF_PATH_FFT) CHECK(fft_reserve(ctx, g, dtype, true));
    if (g.N > 0 && use_fft_hybrid(ctx, g, dtype)) {
        const int rc = fft_reserve(ctx, g, dtype, false);
        if (rc != TNMF_OK && !(rc == TNMF_E_WORKSPACE && ctx->path == TNMF_PATH_AUTO)) return rc;
    }
    return ensure_scratch(ctx, plan_scratch(ctx, g, dtype).total);
}

int tnmf_hip_ctx_set_path(tnmf_hip_ctx *ctx, int path) {
    if (!ctx) return TNMF_E_NULL;
    if (path < TNMF_PATH_AUTO || path > TNMF_PATH_SPLIT) return TNMF_E_UNSUPPORTED;
    if (path != ctx->path) fft_invalidate(ctx);   // (the FFT family's workspace layout follows the path: column lengths)
    ctx->path = path;
    return TNMF_OK;
}

int tnmf_hip_ctx_set_split(tnmf_hip_ctx *ctx, int enable) {
    if (!ctx) return TNMF_E_NULL;
    ctx->split = enable != 0;
    return TNMF_OK;
}

int tnmf_hip_ctx_set_persistent(tnmf_hip_ctx *ctx, int mode) {
    if (!ctx) return TNMF_E_NULL;
    if (mode < 0 || mode > 2) return TNMF_E_UNSUPPORTED;
    ctx->persistent = mode;
    return TNMF_OK;
}

int tnmf_hip_ctx_last_schedule_persistent(const tnmf_hip_ctx *ctx) { return ctx && ctx->last_schedule_persistent ? 1 : 0; }

int tnmf_hip_ctx_set_cache(tnmf_hip_ctx *ctx, int enable) {
    if (!ctx) return TNMF_E_NULL;
    ctx->fft.cache_enabled = enable != 0;
    fft_invalidate(ctx);
    return TNMF_OK;
}

int tnmf_hip_ctx_bind(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *H, const void *V) {
    if (!ctx) return TNMF_E_NULL;
    if (!geom || !H) {
        fft_unbind(ctx);
        return TNMF_OK;
    }
    if (is_vol(geom)) {   // (the spectrum cache belongs to the FFT family: nothing to bind for volumes)
        fft_unbind(ctx);
        return TNMF_OK;
    }
    Geo g;
    const int rc = to_geo(geom, &g);
    if (rc != TNMF_OK) return rc;
    fft_bind(ctx, g, geom->dtype, H, V);
    return TNMF_OK;
}

int tnmf_hip_ctx_cache_counters(const tnmf_hip_ctx *ctx, unsigned long long out[4]) {
    if (!ctx || !out) return TNMF_E_NULL;
    out[0] = ctx->fft.h_runs;
    out[1] = ctx->fft.h_hits;
    out[2] = ctx->fft.v_runs;
    out[3] = ctx->fft.v_hits;
    return TNMF_OK;
}

int tnmf_hip_ctx_invalidate(tnmf_hip_ctx *ctx) {
    if (!ctx) return TNMF_E_NULL;
    fft_invalidate(ctx);
    return TNMF_OK;
}

const char *tnmf_hip_ctx_last_path(const tnmf_hip_ctx *ctx) { return ctx ? ctx->last_path : "none"; }

#ifdef TNMF_DIAG
// diagnostic library only (not part of the ABI of include/tnmf_hip.h): change the ablation mask of a live context
int tnmf_hip_diag_set_ablate(tnmf_hip_ctx *ctx, int mask) {
    if (!ctx) return TNMF_E_NULL;
    ctx->ablate = mask;
    return TNMF_OK;
}
#endif

int tnmf_hip_reconstruct(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *W, const void *H, void *R,
                         void *stream) {
    if (is_vol(geom)) return vol_api_reconstruct(ctx, geom, W, H, R, stream);
    ENTER(ctx, geom);
    if (!W || (g.N > 0 && (!H || !R))) return TNMF_E_NULL;
    return do_reconstruct(ctx, g, dtype, W, H, R, s);
}

int tnmf_hip_grad_H(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *R_or_null,
                    const void *W, const void *H, void *neg, void *pos, void *stream) {
    if (is_vol(geom)) return vol_api_grad_H(ctx, geom, V, R_or_null, W, H, neg, pos, stream);
    ENTER(ctx, geom);
    if (!W || (g.N > 0 && (!V || !neg || !pos))) return TNMF_E_NULL;
    const void *R = R_or_null;
    if (!R && g.N > 0) {
        if (!H) return TNMF_E_NULL;
        const Scratch sc = plan_scratch(ctx, g, dtype);
        CHECK(ensure_scratch(ctx, sc.total));
        void *Rs = ws_at(ctx, sc.r_off);
        CHECK(do_reconstruct(ctx, g, dtype, W, H, Rs, s));
        R = Rs;
    }
    return do_corr_W(ctx, g, dtype, V, R, W, nullptr, neg, pos, false, 0.0, s);
}

int tnmf_hip_grad_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *R_or_null,
                    const void *W, const void *H, void *neg, void *pos, void *stream) {
    if (is_vol(geom)) return vol_api_grad_W(ctx, geom, V, R_or_null, R_or_null != nullptr, W, H, neg, pos, stream);
    ENTER(ctx, geom);
    if (!neg || !pos || (g.N > 0 && (!V || !H))) return TNMF_E_NULL;
    const Scratch sc = plan_scratch(ctx, g, dtype);
    CHECK(ensure_scratch(ctx, sc.total));
    const void *R = R_or_null;
    if (!R && g.N > 0) {
        if (!W) return TNMF_E_NULL;
        void *Rs = ws_at(ctx, sc.r_off);
        CHECK(do_reconstruct(ctx, g, dtype, W, H, Rs, s));
        R = Rs;
    }
    return do_corr_H(ctx, g, dtype, sc, V, R, H, neg, pos, s);
}

int tnmf_hip_mu_update(tnmf_hip_ctx *ctx, int dtype, void *arr, const void *neg, void *pos, double reg,
                       size_t n_elems, void *stream) {
    if (!ctx) return TNMF_E_NULL;
    if (dtype != 0 && dtype != 1) return TNMF_E_DTYPE;
    if (n_elems > 0 && (!arr || !neg || !pos)) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    fft_invalidate(ctx);   // arr may be (part of) the activations whose row spectra are cached
    return launch_mu_update(ctx, dtype, arr, neg, pos, reg, n_elems, static_cast<hipStream_t>(stream));
}

int tnmf_hip_normalize_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, void *W, void *stream) {
    if (is_vol(geom)) {
        VOL_ENTER(ctx, geom);
        if (!W) return TNMF_E_NULL;
        return launch_apply_normalize_W(vol_dict_geo(v), dtype, W, nullptr, nullptr, 0.0, false, s);
    }
    ENTER(ctx, geom);
    if (!W) return TNMF_E_NULL;
    fft_invalidate_W(ctx);
    return launch_apply_normalize_W(g, dtype, W, nullptr, nullptr, 0.0, false, s);
}

// the energy on one or two shift axes: 1/2 sum (V - R)^2, or with beta != NULL sum D_beta(V | R + eps) (*beta != 2); with
// G != NULL the weighted sum of either
static int energy_2d(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *G, const void *W,
                     const void *H, double *out_host, const double *beta, double eps, void *stream) {
    ENTER(ctx, geom);
    if (!out_host) return TNMF_E_NULL;
    if (g.N == 0) {
        *out_host = 0.0;
        return TNMF_OK;
    }
    if (!V || !W || !H) return TNMF_E_NULL;
    const Scratch sc = plan_scratch(ctx, g, dtype);
    CHECK(ensure_scratch(ctx, sc.total));
    void *Rs = ws_at(ctx, sc.r_off);
    CHECK(do_reconstruct(ctx, g, dtype, W, H, Rs, s));
    double *red = reinterpret_cast<double *>(ws_at(ctx, sc.red_off));   // (kEnergyPartials >= kBetaPartials words + result)
    const size_t n = (size_t)g.N * g.C * g.Dy * g.Dx;
    CHECK(beta || G ? launch_beta_energy(ctx, dtype, beta ? *beta : 2.0, eps, V, G, Rs, n, red, red + kEnergyPartials, s)
                    : launch_half_sqdiff(ctx, dtype, V, Rs, n, red, red + kEnergyPartials, s));
    TNMF_HIP_TRY(hipMemcpyAsync(out_host, red + kEnergyPartials, sizeof(double), hipMemcpyDeviceToHost, s));
    TNMF_HIP_TRY(hipStreamSynchronize(s));
    return TNMF_OK;
}

int tnmf_hip_energy(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *W, const void *H,
                    double *out_host, void *stream) {
    if (is_vol(geom)) return vol_api_energy(ctx, geom, V, W, H, out_host, stream);
    return energy_2d(ctx, geom, V, nullptr, W, H, out_host, nullptr, 0.0, stream);
}

int tnmf_hip_energy_beta(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, double beta, double eps, const void *V,
                         const void *W, const void *H, double *out_host, void *stream) {
    if (beta == 2.0) return tnmf_hip_energy(ctx, geom, V, W, H, out_host, stream);
    if (!ctx || !geom) return TNMF_E_NULL;
    if (is_vol(geom) || !beta_ok(beta)) return TNMF_E_UNSUPPORTED;
    return energy_2d(ctx, geom, V, nullptr, W, H, out_host, &beta, eps, stream);
}

int tnmf_hip_energy_weighted(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, double beta, double eps, const void *V,
                             const void *G, const void *W, const void *H, double *out_host, void *stream) {
    if (!G) return tnmf_hip_energy_beta(ctx, geom, beta, eps, V, W, H, out_host, stream);
    if (!ctx || !geom) return TNMF_E_NULL;
    if (is_vol(geom) || !beta_ok(beta)) return TNMF_E_UNSUPPORTED;
    return energy_2d(ctx, geom, V, G, W, H, out_host, beta == 2.0 ? nullptr : &beta, eps, stream);
}

int tnmf_hip_ctx_set_objective_tap(tnmf_hip_ctx *ctx, double *per_sample_dev) {
    if (!ctx) return TNMF_E_NULL;
    ctx->obj_tap = per_sample_dev;
    return TNMF_OK;
}

int tnmf_hip_sample_objective(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, double beta, double eps, const void *V,
                              const void *G_or_null, const void *W, const void *H, double *per_sample_dev, void *stream) {
    if (!ctx || !geom) return TNMF_E_NULL;
    if (!beta_ok(beta)) return TNMF_E_UNSUPPORTED;
    const double *bp = beta == 2.0 ? nullptr : &beta;
    if (is_vol(geom)) {
        if (bp || G_or_null) return TNMF_E_UNSUPPORTED;   // (volumes: the Frobenius objective, unweighted)
        VOL_ENTER(ctx, geom);
        if (v.N == 0) return TNMF_OK;
        if (!V || !W || !H || !per_sample_dev) return TNMF_E_NULL;
        void *Rs;
        CHECK(vol_scratch(ctx, v, dtype, &Rs, nullptr));
        CHECK(vol_reconstruct(v, dtype, W, H, Rs, s));
        return sample_objective_of(ctx, dtype, nullptr, eps, V, nullptr, Rs, (size_t)v.N, (size_t)v.C * vol_vox(v),
                                   per_sample_dev, s);
    }
    ENTER(ctx, geom);
    if (g.N == 0) return TNMF_OK;
    if (!V || !W || !H || !per_sample_dev) return TNMF_E_NULL;
    const Scratch sc = plan_scratch(ctx, g, dtype);
    CHECK(ensure_scratch(ctx, sc.total));
    void *Rs = ws_at(ctx, sc.r_off);
    CHECK(do_reconstruct(ctx, g, dtype, W, H, Rs, s));
    return sample_objective_of(ctx, dtype, bp, eps, V, G_or_null, Rs, (size_t)g.N, (size_t)g.C * g.Dy * g.Dx,
                               per_sample_dev, s);
}

int tnmf_hip_atom_terms(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int group, const void *V, const void *G_or_null,
                        const void *R_or_null, const void *W, const void *H, double *ab, void *stream) {
    if (!ctx || !geom) return TNMF_E_NULL;
    if (is_vol(geom)) return TNMF_E_UNSUPPORTED;
    ENTER(ctx, geom);
    if (group < 1 || g.M % group != 0) return TNMF_E_GEOM;
    if (g.N == 0) return TNMF_OK;
    if (!V || !W || !H || !ab) return TNMF_E_NULL;
    CHECK(atom_terms_check(g, dtype));
    // work buffer: [partial sums per (sample, tile, atom) | the taps of the flipped dictionary]
    const size_t p_bytes = atom_terms_partial_bytes(g, group);
    CHECK(ensure_buffer(&ctx->ob, &ctx->ob_bytes, p_bytes + atom_terms_taps_bytes(g, dtype), false));
    const void *R = R_or_null;
    if (!R) {
        const Scratch sc = plan_scratch(ctx, g, dtype);
        CHECK(ensure_scratch(ctx, sc.total));
        void *Rs = ws_at(ctx, sc.r_off);
        CHECK(do_reconstruct(ctx, g, dtype, W, H, Rs, s));
        R = Rs;
    }
    return launch_atom_terms(ctx, g, dtype, group, V, G_or_null, R, W, H, static_cast<double *>(ctx->ob),
                             static_cast<char *>(ctx->ob) + p_bytes, ab, s);
}

int tnmf_hip_atom_gram(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int group, const void *V, const void *G_or_null,
                       const void *R_or_null, const void *W, const void *H, double *a, double *B, void *stream) {
    if (!ctx || !geom) return TNMF_E_NULL;
    if (is_vol(geom)) return TNMF_E_UNSUPPORTED;
    ENTER(ctx, geom);
    if (group < 1 || g.M % group != 0) return TNMF_E_GEOM;
    if (g.N == 0) return TNMF_OK;
    if (!V || !W || !H || !a || !B) return TNMF_E_NULL;
    CHECK(atom_gram_check(g, dtype, group));
    // work buffer: [partial sums per (sample, strip, pair of atom blocks) | the taps of the flipped dictionary]
    const size_t p_bytes = atom_gram_partial_bytes(g, dtype, group);
    CHECK(ensure_buffer(&ctx->ob, &ctx->ob_bytes, p_bytes + atom_terms_taps_bytes(g, dtype), false));
    const void *R = R_or_null;
    if (!R) {
        const Scratch sc = plan_scratch(ctx, g, dtype);
        CHECK(ensure_scratch(ctx, sc.total));
        void *Rs = ws_at(ctx, sc.r_off);
        CHECK(do_reconstruct(ctx, g, dtype, W, H, Rs, s));
        R = Rs;
    }
    return launch_atom_gram(ctx, g, dtype, group, V, G_or_null, R, W, H, static_cast<double *>(ctx->ob),
                            static_cast<char *>(ctx->ob) + p_bytes, a, B, s);
}

int tnmf_hip_atom_sources(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int n_sources, const int *plane_order, int n_listed,
                          const int *source_start, int emit, double eps, const void *V, const void *W, const void *H,
                          void *out, int *label, void *share, void *stream) {
    if (!ctx || !geom) return TNMF_E_NULL;
    if (is_vol(geom)) return TNMF_E_UNSUPPORTED;
    ENTER(ctx, geom);
    if (emit < TNMF_SOURCES_CONTRIBUTION || emit > TNMF_SOURCES_DOMINANT || !(eps >= 0.0)) return TNMF_E_GEOM;
    if (n_sources < 1 || n_listed < n_sources || n_listed > g.M) return TNMF_E_GEOM;
    if (g.N == 0) return TNMF_OK;
    const bool dom = emit == TNMF_SOURCES_DOMINANT;
    if (!plane_order || !source_start || !W || !H || (emit == TNMF_SOURCES_MASKED && !V)) return TNMF_E_NULL;
    if (dom ? (!label || !share) : !out) return TNMF_E_NULL;
    {
        Geo g1 = g;
        if (dom) g1.C = 1;
        CHECK(atom_terms_check(g1, dtype));
    }
    // the two tables, wherever they live: checked and completed here, before anything is written
    std::vector<int> order((size_t)g.M), start((size_t)n_sources + 2);
    TNMF_HIP_TRY(hipMemcpyAsync(order.data(), plane_order, (size_t)n_listed * sizeof(int), hipMemcpyDefault, s));
    TNMF_HIP_TRY(hipMemcpyAsync(start.data(), source_start, ((size_t)n_sources + 1) * sizeof(int), hipMemcpyDefault, s));
    TNMF_HIP_TRY(hipStreamSynchronize(s));
    if (start[0] != 0 || start[n_sources] != n_listed) return TNMF_E_GEOM;
    for (int k = 0; k < n_sources; ++k)
        if (start[k + 1] <= start[k]) return TNMF_E_GEOM;
    std::vector<char> listed((size_t)g.M, 0);
    for (int i = 0; i < n_listed; ++i) {
        if (order[i] < 0 || order[i] >= g.M || listed[order[i]]) return TNMF_E_GEOM;
        listed[order[i]] = 1;
    }
    int fill = n_listed;
    for (int m = 0; m < g.M; ++m)
        if (!listed[m]) order[fill++] = m;
    start[n_sources + 1] = g.M;
    const SourcesWork wk = atom_sources_work(g, dtype, n_sources, emit);
    CHECK(ensure_buffer(&ctx->ob, &ctx->ob_bytes, wk.total, false));
    char *work = static_cast<char *>(ctx->ob);
    TNMF_HIP_TRY(hipMemcpyAsync(work + wk.order_off, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice, s));
    TNMF_HIP_TRY(hipMemcpyAsync(work + wk.start_off, start.data(), start.size() * sizeof(int), hipMemcpyHostToDevice, s));
    TNMF_HIP_TRY(hipStreamSynchronize(s));   // (the two vectors end with this call)
    return launch_atom_sources(ctx, g, dtype, n_sources, emit, eps, work, V, W, H, out, label, share, s);
}

int tnmf_hip_beta_fields(tnmf_hip_ctx *ctx, int dtype, double beta, double eps, const void *V, const void *R, void *Q,
                         void *P, size_t n_elems, void *stream) {
    if (!ctx) return TNMF_E_NULL;
    if (dtype != 0 && dtype != 1) return TNMF_E_DTYPE;
    if (!beta_ok(beta)) return TNMF_E_UNSUPPORTED;
    if (n_elems > 0 && (!V || !R || !Q || !P)) return TNMF_E_NULL;
    if (n_elems > 0 && (Q == V || Q == R || P == V)) return TNMF_E_NULL;   // (only P may alias R)
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return launch_beta_fields(ctx, dtype, beta, eps, V, nullptr, R, Q, P, n_elems, static_cast<hipStream_t>(stream));
}

int tnmf_hip_weighted_fields(tnmf_hip_ctx *ctx, int dtype, double beta, double eps, const void *V, const void *G,
                             const void *R, void *Q, void *P, size_t n_elems, void *stream) {
    if (!ctx || !G) return TNMF_E_NULL;
    if (dtype != 0 && dtype != 1) return TNMF_E_DTYPE;
    if (!beta_ok(beta)) return TNMF_E_UNSUPPORTED;
    if (n_elems > 0 && (!V || !R || !Q || !P)) return TNMF_E_NULL;
    if (n_elems > 0 && (Q == V || Q == G || Q == R || P == V || P == G)) return TNMF_E_NULL;   // (only P may alias R)
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return launch_beta_fields(ctx, dtype, beta, eps, V, G, R, Q, P, n_elems, static_cast<hipStream_t>(stream));
}

int tnmf_hip_convolve_multi_1d(tnmf_hip_ctx *ctx, int dtype, int ndim, size_t rows, const int *shape,
                               const void *in, void *out, void *tmp, const double *kernel0, int len0,
                               const double *kernel1, int len1, void *stream) {
    if (!ctx || !shape || !kernel0) return TNMF_E_NULL;
    if (dtype != 0 && dtype != 1) return TNMF_E_DTYPE;
    if (ndim != 1 && ndim != 2) return TNMF_E_GEOM;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    if (rows == 0) return TNMF_OK;
    if (!in || !out) return TNMF_E_NULL;
    if (ndim == 1) return launch_convolve_axis(ctx, dtype, in, out, rows, shape[0], 1, kernel0, len0, s);
    if (!tmp || !kernel1) return TNMF_E_NULL;
    // reference order: axis -2 first, then axis -1 (TransformInvariantNMF.py:254; _NumPyBackend.py:60-62)
    CHECK(launch_convolve_axis(ctx, dtype, in, tmp, rows, shape[0], shape[1], kernel0, len0, s));
    return launch_convolve_axis(ctx, dtype, tmp, out, rows * (size_t)shape[0], shape[1], 1, kernel1, len1, s);
}

int tnmf_hip_convolve_axis(tnmf_hip_ctx *ctx, int dtype, size_t rows, int len, size_t inner, const void *in, void *out,
                           const double *kernel, int klen, void *stream) {
    if (!ctx || !kernel) return TNMF_E_NULL;
    if (dtype != 0 && dtype != 1) return TNMF_E_DTYPE;
    if (len < 0 || inner > 0x7fffffffu) return TNMF_E_GEOM;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    if (rows == 0 || len == 0 || inner == 0) return TNMF_OK;
    if (!in || !out || in == out) return TNMF_E_NULL;
    return launch_convolve_axis(ctx, dtype, in, out, rows, len, (int)inner, kernel, klen, static_cast<hipStream_t>(stream));
}

int tnmf_hip_pad_H(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *H, void *Hpad, void *stream) {
    if (is_vol(geom)) return vol_api_pad_fold(ctx, geom, mode, false, H, Hpad, stream);
    ENTER(ctx, geom);
    if (!mode_known(mode)) return TNMF_E_UNSUPPORTED;
    if (g.N > 0 && (!H || !Hpad)) return TNMF_E_NULL;
    if (g.Hs != g.Hx) return TNMF_E_STRIDE;
    return launch_pad_fold(ctx, g, dtype, mode, false, H, Hpad, s);
}

int tnmf_hip_fold_H(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *Gpad, void *G, void *stream) {
    if (is_vol(geom)) return vol_api_pad_fold(ctx, geom, mode, true, Gpad, G, stream);
    ENTER(ctx, geom);
    if (!mode_known(mode)) return TNMF_E_UNSUPPORTED;
    if (g.N > 0 && (!Gpad || !G)) return TNMF_E_NULL;
    return launch_pad_fold(ctx, g, dtype, mode, true, Gpad, G, s);
}

// the H half step of tnmf_hip_update_H / _update_H_ex on one or two shift axes; beta != NULL: of the beta-divergence
// (*beta != 2), G != NULL: of the weighted objective -- either way the fields (Q, P) of the reconstruction standing in for
// (V, R) in every correlation.  r_is_valid ('valid' mode only): R_scratch already holds the reconstruction of H_inout
static int update_H_2d(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *V, const void *G,
                       const void *W, void *H_inout, void *R_scratch, int r_is_valid, double eps, double sparsity,
                       double inhibition, double cross_inhibition, const double *kernel0, int len0,
                       const double *kernel1, int len1, const double *beta, void *stream) {
    ENTER(ctx, geom);
    if (!mode_known(mode)) return TNMF_E_UNSUPPORTED;
    if (g.N == 0) return TNMF_OK;
    if (!V || !W || !H_inout) return TNMF_E_NULL;
    const bool lateral = inhibition > 0 || cross_inhibition > 0;
    if (lateral && (!kernel0 || (geom->ndim == 2 && !kernel1))) return TNMF_E_NULL;
    if (inhibition < 0 || cross_inhibition < 0) return TNMF_E_GEOM;
    const double reg = reg_of(eps, sparsity);
    const size_t es = esize(dtype);
    void *Rs = R_scratch;
    if (!Rs) {
        if (r_is_valid) return TNMF_E_NULL;
        const Scratch sc = plan_scratch(ctx, g, dtype);
        CHECK(ensure_scratch(ctx, sc.total));
        Rs = ws_at(ctx, sc.r_off);
    }
    // the reference's kernels come one per shift axis (TransformInvariantNMF.py:163): 1-D problems have the x kernel only
    const double one = 1.0;
    const double *ky = geom->ndim == 2 ? kernel0 : &one, *kx = geom->ndim == 2 ? kernel1 : kernel0;
    const int ly = geom->ndim == 2 ? len0 : 1, lx = geom->ndim == 2 ? len1 : len0;
    const double xc = cross_weight(cross_inhibition, g.M);

    if (mode == TNMF_MODE_VALID) {
        const size_t nE = align_up((size_t)g.N * g.M * g.Hy * g.Hs * es, 256);
        const size_t nG = align_up((size_t)g.N * g.M * g.Hy * g.Hx * es, 256);
        void *E = nullptr;
        if (lateral) {
            CHECK(ensure_hwork(ctx, nE));
            E = ctx->hw;
            CHECK(launch_inhibition(ctx, dtype, g.N, g.M, g.Hy, g.Hs, H_inout, E, ky, ly, kx, lx, inhibition, xc, s));
        }
        if (!r_is_valid) CHECK(do_reconstruct(ctx, g, dtype, W, H_inout, Rs, s));
        CHECK(tap_objective(ctx, dtype, beta, eps, V, G, Rs, (size_t)g.N, (size_t)g.C * g.Dy * g.Dx, s));
        if (beta || G) CHECK(beta_fields_of(ctx, g, dtype, beta, eps, V, G, Rs, &V, s));
        int rc = do_corr_W(ctx, g, dtype, V, Rs, W, H_inout, nullptr, nullptr, true, reg, s, E);
        if (!E || (rc != TNMF_E_UNSUPPORTED && rc != TNMF_E_STRIDE)) return rc;
        // this kernel family has no epilogue for the extra term (nothing has been written): unfused gradient into the
        // work arrays, then one update kernel
        if (ctx->hw_bytes < nE + 2 * nG) {
            // (growing the buffer would lose E: take the larger buffer first, then compute E again)
            CHECK(ensure_hwork(ctx, nE + 2 * nG));
            E = ctx->hw;
            CHECK(launch_inhibition(ctx, dtype, g.N, g.M, g.Hy, g.Hs, H_inout, E, ky, ly, kx, lx, inhibition, xc, s));
        }
        char *neg = static_cast<char *>(ctx->hw) + nE, *pos = neg + nG;
        CHECK(do_corr_W(ctx, g, dtype, V, Rs, W, nullptr, neg, pos, false, 0.0, s));
        fft_invalidate_H(ctx, g, dtype, H_inout);
        return launch_mu_update_extra(ctx, dtype, H_inout, neg, pos, E, (size_t)g.N * g.M * g.Hy, g.Hx, g.Hs, reg, s);
    }

    // reconstruction modes: a 'valid' half step on the padded activations, folded back (adjoint of the pad) inside the
    // update kernel.  H is C-contiguous with the shift shape of the mode.
    if (g.Hs != g.Hx) return TNMF_E_STRIDE;
    const int Sy = geom->ndim == 1 ? 1 : mode_shift_len(mode, g.Dy, g.Ay), Sx = mode_shift_len(mode, g.Dx, g.Ax);
    if (Sy < 1 || Sx < 1) return TNMF_E_GEOM;
    const size_t nP = align_up((size_t)g.N * g.M * g.Hy * g.Hx * es, 256);
    const size_t nE = lateral ? align_up((size_t)g.N * g.M * Sy * Sx * es, 256) : 0;
    CHECK(ensure_hwork(ctx, 3 * nP + nE));
    char *Hp = static_cast<char *>(ctx->hw), *negp = Hp + nP, *posp = negp + nP;
    void *E = lateral ? posp + nP : nullptr;
    fft_invalidate(ctx);   // the padded copy lives at the same address every call, with new contents
    CHECK(launch_pad_fold(ctx, g, dtype, mode, false, H_inout, Hp, s));
    CHECK(do_reconstruct(ctx, g, dtype, W, Hp, Rs, s));
    CHECK(tap_objective(ctx, dtype, beta, eps, V, G, Rs, (size_t)g.N, (size_t)g.C * g.Dy * g.Dx, s));
    if (beta || G) CHECK(beta_fields_of(ctx, g, dtype, beta, eps, V, G, Rs, &V, s));
    CHECK(do_corr_W(ctx, g, dtype, V, Rs, W, nullptr, negp, posp, false, 0.0, s));
    if (lateral) CHECK(launch_inhibition(ctx, dtype, g.N, g.M, Sy, Sx, H_inout, E, ky, ly, kx, lx, inhibition, xc, s));
    fft_invalidate(ctx);
    return launch_fold_update(ctx, g, dtype, mode, Sy, Sx, H_inout, negp, posp, E, reg, s);
}

int tnmf_hip_update_H(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *W, void *H_inout,
                      void *R_scratch, int r_is_valid, double eps, double sparsity, void *stream) {
    if (is_vol(geom)) return vol_api_update_H(ctx, geom, V, W, H_inout, R_scratch, r_is_valid, eps, sparsity, stream);
    return update_H_2d(ctx, geom, TNMF_MODE_VALID, V, nullptr, W, H_inout, R_scratch, r_is_valid, eps, sparsity, 0.0, 0.0,
                       nullptr, 0, nullptr, 0, nullptr, stream);
}

int tnmf_hip_update_H_ex(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *V, const void *W,
                         void *H_inout, void *R_scratch, double eps, double sparsity, double inhibition,
                         double cross_inhibition, const double *kernel0, int len0, const double *kernel1, int len1,
                         const double *kernel2, int len2, void *stream) {
    if (is_vol(geom)) {
        const double *const kern[3] = {kernel0, kernel1, kernel2};
        const int klen[3] = {len0, len1, len2};
        return vol_api_update_H_ex(ctx, geom, mode, V, W, H_inout, R_scratch, eps, sparsity, inhibition, cross_inhibition,
                                   kern, klen, stream);
    }
    return update_H_2d(ctx, geom, mode, V, nullptr, W, H_inout, R_scratch, 0, eps, sparsity, inhibition,
                       cross_inhibition, kernel0, len0, kernel1, len1, nullptr, stream);
}

int tnmf_hip_update_H_beta(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *V, const void *W,
                           void *H_inout, void *R_scratch, double eps, double sparsity, double inhibition,
                           double cross_inhibition, const double *kernel0, int len0, const double *kernel1, int len1,
                           const double *kernel2, int len2, double beta, void *stream) {
    if (beta == 2.0)
        return tnmf_hip_update_H_ex(ctx, geom, mode, V, W, H_inout, R_scratch, eps, sparsity, inhibition,
                                    cross_inhibition, kernel0, len0, kernel1, len1, kernel2, len2, stream);
    if (!ctx || !geom) return TNMF_E_NULL;
    if (is_vol(geom) || !beta_ok(beta)) return TNMF_E_UNSUPPORTED;
    return update_H_2d(ctx, geom, mode, V, nullptr, W, H_inout, R_scratch, 0, eps, sparsity, inhibition,
                       cross_inhibition, kernel0, len0, kernel1, len1, &beta, stream);
}

int tnmf_hip_update_H_weighted(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *V, const void *G,
                               const void *W, void *H_inout, void *R_scratch, double eps, double sparsity,
                               double inhibition, double cross_inhibition, const double *kernel0, int len0,
                               const double *kernel1, int len1, const double *kernel2, int len2, double beta,
                               void *stream) {
    if (!G)
        return tnmf_hip_update_H_beta(ctx, geom, mode, V, W, H_inout, R_scratch, eps, sparsity, inhibition,
                                      cross_inhibition, kernel0, len0, kernel1, len1, kernel2, len2, beta, stream);
    if (!ctx || !geom) return TNMF_E_NULL;
    if (is_vol(geom) || !beta_ok(beta)) return TNMF_E_UNSUPPORTED;
    return update_H_2d(ctx, geom, mode, V, G, W, H_inout, R_scratch, 0, eps, sparsity, inhibition, cross_inhibition,
                       kernel0, len0, kernel1, len1, beta == 2.0 ? nullptr : &beta, stream);
}

// the W gradient into [neg | pos] on one or two shift axes; beta != NULL: of the beta-divergence (*beta != 2), G != NULL:
// of the weighted objective -- the fields (Q, P) of the reconstruction standing in for (V, R)
static int grad_W_2d(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *G, const void *W,
                     const void *H, void *R_scratch, int r_is_valid, void *negpos, const double *beta, double eps,
                     void *stream) {
    ENTER(ctx, geom);
    if (!negpos || !W || (g.N > 0 && (!V || !H))) return TNMF_E_NULL;
    const Scratch sc = plan_scratch(ctx, g, dtype);
    CHECK(ensure_scratch(ctx, sc.total));
    if (r_is_valid && !R_scratch) return TNMF_E_NULL;
    void *Rs = R_scratch ? R_scratch : ws_at(ctx, sc.r_off);
    if (!r_is_valid) CHECK(do_reconstruct(ctx, g, dtype, W, H, Rs, s));
    if ((beta || G) && g.N > 0) CHECK(beta_fields_of(ctx, g, dtype, beta, eps, V, G, Rs, &V, s));
    char *np = static_cast<char *>(negpos);
    const size_t wbytes = (size_t)g.M * g.C * g.Ay * g.Ax * esize(dtype);
    return do_corr_H(ctx, g, dtype, sc, V, Rs, H, np, np + wbytes, s);
}

int tnmf_hip_grad_W_fused(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *W, const void *H,
                          void *R_scratch, int r_is_valid, void *negpos, void *stream) {
    if (is_vol(geom)) {
        if (!negpos || (r_is_valid && !R_scratch)) return TNMF_E_NULL;
        Vol vv;
        CHECK(to_vol(geom, &vv));
        char *np3 = static_cast<char *>(negpos);
        return vol_api_grad_W(ctx, geom, V, R_scratch, r_is_valid, W, H, np3,
                              np3 + (size_t)vv.M * vv.C * vol_avox(vv) * esize(geom->dtype), stream);
    }
    return grad_W_2d(ctx, geom, V, nullptr, W, H, R_scratch, r_is_valid, negpos, nullptr, 0.0, stream);
}

int tnmf_hip_grad_W_beta(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *W, const void *H,
                         void *R_scratch, int r_is_valid, void *negpos, double beta, double eps, void *stream) {
    if (beta == 2.0) return tnmf_hip_grad_W_fused(ctx, geom, V, W, H, R_scratch, r_is_valid, negpos, stream);
    if (!ctx || !geom) return TNMF_E_NULL;
    if (is_vol(geom) || !beta_ok(beta)) return TNMF_E_UNSUPPORTED;
    return grad_W_2d(ctx, geom, V, nullptr, W, H, R_scratch, r_is_valid, negpos, &beta, eps, stream);
}

int tnmf_hip_grad_W_weighted(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, const void *G, const void *W,
                             const void *H, void *R_scratch, int r_is_valid, void *negpos, double beta, double eps,
                             void *stream) {
    if (!G) return tnmf_hip_grad_W_beta(ctx, geom, V, W, H, R_scratch, r_is_valid, negpos, beta, eps, stream);
    if (!ctx || !geom) return TNMF_E_NULL;
    if (is_vol(geom) || !beta_ok(beta)) return TNMF_E_UNSUPPORTED;
    return grad_W_2d(ctx, geom, V, G, W, H, R_scratch, r_is_valid, negpos, beta == 2.0 ? nullptr : &beta, eps, stream);
}

int tnmf_hip_run_schedule(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *V, void *W_inout, void *H_inout,
                          void *R_scratch, void *acc, const tnmf_hip_op *ops, int n_ops, double eps, double sparsity,
                          void *stream) {
    if (is_vol(geom))
        return vol_api_run_schedule(ctx, geom, V, W_inout, H_inout, R_scratch, acc, ops, n_ops, eps, sparsity, stream);
    ENTER(ctx, geom);
    if (n_ops < 0 || (n_ops > 0 && !ops)) return TNMF_E_NULL;
    if (!V || !W_inout || !H_inout || !acc) return TNMF_E_NULL;
    const size_t es = esize(dtype);
    const size_t vs = (size_t)g.C * g.Dy * g.Dx * es, hs = (size_t)g.M * g.Hy * g.Hs * es;
    const size_t wn = (size_t)g.M * g.C * g.Ay * g.Ax;
    CHECK(check_ops(ops, n_ops, g.N));
    // Consecutive H half steps commute when their slices are disjoint -- the H update of a sample reads that sample and W
    // only (NumPy.py:93-120), and W does not change between them -- so a RUN of them is executed as the H half step of the
    // union: the slices sorted and joined where they touch.  GSG-MU / GSAG-MU (TransformInvariantNMF.py:474-479,493-504: H for
    // every shuffled batch, W from the last one only) become ONE H half step over all samples + one W step per epoch instead
    // of 256 x 2 launches of three samples each.  Runs with overlapping slices are left as they are (an H step is not
    // idempotent).  Same arithmetic per sample; the kernel family follows the size of the joined slice.
    std::vector<tnmf_hip_op> joined;
    joined.reserve(n_ops);
    for (int i = 0; i < n_ops;) {
        if (ops[i].kind != TNMF_OP_UPDATE_H) {
            joined.push_back(ops[i++]);
            continue;
        }
        int j = i;
        while (j < n_ops && ops[j].kind == TNMF_OP_UPDATE_H) ++j;
        std::vector<tnmf_hip_op> run(ops + i, ops + j);
        run.erase(std::remove_if(run.begin(), run.end(), [](const tnmf_hip_op &o) { return o.n1 <= o.n0; }), run.end());
        std::vector<tnmf_hip_op> sorted_run = run;
        std::sort(sorted_run.begin(), sorted_run.end(), [](const tnmf_hip_op &a, const tnmf_hip_op &b) { return a.n0 < b.n0; });
        bool disjoint = true;
        for (size_t k = 1; k < sorted_run.size(); ++k) disjoint = disjoint && sorted_run[k].n0 >= sorted_run[k - 1].n1;
        if (!disjoint) {
            joined.insert(joined.end(), run.begin(), run.end());
        } else {
            for (size_t k = 0; k < sorted_run.size(); ++k) {
                if (!joined.empty() && joined.back().kind == TNMF_OP_UPDATE_H && k > 0 && joined.back().n1 == sorted_run[k].n0)
                    joined.back().n1 = sorted_run[k].n1;
                else
                    joined.push_back(sorted_run[k]);
            }
        }
        i = j;
    }
    ops = joined.data();
    n_ops = (int)joined.size();
    int nmax = 1;
    for (int i = 0; i < n_ops; ++i)
        if (ops[i].kind != TNMF_OP_APPLY_W && ops[i].n1 - ops[i].n0 > nmax) nmax = ops[i].n1 - ops[i].n0;
    const double reg = reg_of(eps, sparsity);
    // A whole problem that is tiny (BASELINE config 1): every kernel would run for a few microseconds and the list would be
    // launch latency -- the persistent schedule kernel walks it in ONE launch.  (Small batches of a LARGE problem stay on
    // the per-operation path below: measured on the reference's mini-batch geometry, 768 x 1 x 32 x 32 with batch_size 3,
    // the grid barriers of the persistent kernel -- agent-scope release / acquire across eight L2s -- cost as much as
    // the launches they replace: 28.5 ms per ASG epoch against 26.7 ms.)
    // (Round 4 built an XCD-local flavour of that kernel for exactly that case -- the workgroups of ONE XCD, barriers without
    // the L2 write-back: 22.3 ms per ASG epoch against 12.0 on the per-operation path below, profiles/r04_xcd_local_schedule_kernel.txt.)
    const bool tiny = (size_t)g.N * g.M * g.Hy * g.Hx <= ((size_t)1 << 18);
    if (n_ops > 0 && tiny && ctx->persistent != 0 && (ctx->path == TNMF_PATH_AUTO || ctx->path == TNMF_PATH_GENERIC) &&
        generic_schedule_fits(ctx, g, dtype)) {
        const int P = generic_schedule_chunks(ctx, g);
        const size_t r_bytes = R_scratch ? 0 : align_up((size_t)g.N * vs, 256);
        const size_t p_bytes = align_up((size_t)P * wn * 2 * sizeof(double), 256);
        const size_t o_bytes = align_up((size_t)n_ops * sizeof(tnmf_hip_op), 256);
        CHECK(ensure_scratch(ctx, r_bytes + p_bytes + o_bytes + 1024));
        void *Rs = R_scratch ? R_scratch : static_cast<void *>(ws_at(ctx, 0));
        double *partials = reinterpret_cast<double *>(ws_at(ctx, r_bytes));
        tnmf_hip_op *ops_dev = reinterpret_cast<tnmf_hip_op *>(ws_at(ctx, r_bytes + p_bytes));
        unsigned *counter = reinterpret_cast<unsigned *>(ws_at(ctx, r_bytes + p_bytes + o_bytes));
        {
            const int slot = ctx->ops_next;
            ctx->ops_next = (slot + 1) % tnmf_hip_ctx::kOpSlots;
            const size_t need = (size_t)n_ops * sizeof(tnmf_hip_op);
            if (ctx->ops_done[slot]) TNMF_HIP_TRY(hipEventSynchronize(ctx->ops_done[slot]));   // (4 calls ago: long done)
            else TNMF_HIP_TRY(hipEventCreateWithFlags(&ctx->ops_done[slot], hipEventDisableTiming));
            if (ctx->ops_cap[slot] < need) {
                if (ctx->ops_pinned[slot]) TNMF_HIP_TRY(hipHostFree(ctx->ops_pinned[slot]));
                ctx->ops_pinned[slot] = nullptr;
                ctx->ops_cap[slot] = 0;
                if (hipHostMalloc(&ctx->ops_pinned[slot], align_up(need, 4096), hipHostMallocDefault) != hipSuccess) {
                    (void)hipGetLastError();
                    return TNMF_E_WORKSPACE;
                }
                ctx->ops_cap[slot] = align_up(need, 4096);
            }
            memcpy(ctx->ops_pinned[slot], ops, need);
            TNMF_HIP_TRY(hipMemcpyAsync(ops_dev, ctx->ops_pinned[slot], need, hipMemcpyHostToDevice, s));
            TNMF_HIP_TRY(hipEventRecord(ctx->ops_done[slot], s));
        }
        fft_invalidate(ctx);   // H and W change under the family's caches
        ctx->last_path = "generic";
        const int rc = generic_run_schedule(ctx, g, dtype, V, W_inout, H_inout, Rs, acc, partials, P, ops_dev, n_ops, reg,
                                            eps, counter, s);
        // TNMF_E_UNSUPPORTED: the grid cannot be co-resident on this device right now (occupancy query / cooperative
        // launch refused) -- nothing was launched; the list is walked operation by operation below
        if (rc != TNMF_E_UNSUPPORTED) {
            ctx->last_schedule_persistent = rc == TNMF_OK;
            return rc;
        }
    }
    ctx->last_schedule_persistent = false;
    Geo gmax = g;
    gmax.N = nmax;
    const Scratch scm = plan_scratch(ctx, gmax, dtype);
    const size_t grad_off = scm.total;
    CHECK(ensure_scratch(ctx, scm.total + align_up(2 * wn * es, 256)));
    char *grad = ws_at(ctx, grad_off);
    for (int i = 0; i < n_ops; ++i) {
        const tnmf_hip_op &op = ops[i];
        Geo gs = g;
        gs.N = op.n1 - op.n0;
        const char *Vb = static_cast<const char *>(V) + (size_t)op.n0 * vs;
        char *Hb = static_cast<char *>(H_inout) + (size_t)op.n0 * hs;
        void *Rb = R_scratch ? static_cast<void *>(static_cast<char *>(R_scratch) + (size_t)op.n0 * vs)
                             : static_cast<void *>(ws_at(ctx, scm.r_off));
        switch (op.kind) {
            case TNMF_OP_UPDATE_H:
                if (gs.N == 0) break;
                CHECK(do_reconstruct(ctx, gs, dtype, W_inout, Hb, Rb, s));
                CHECK(do_corr_W(ctx, gs, dtype, Vb, Rb, W_inout, Hb, nullptr, nullptr, true, reg, s));
                break;
            case TNMF_OP_GRAD_W: {
                // (the partials of the slice live where plan_scratch(gmax) put them: sized for the largest slice)
                Scratch sc = plan_scratch(ctx, gs, dtype);
                sc.part_off = scm.part_off;
                if (gs.N > 0) CHECK(do_reconstruct(ctx, gs, dtype, W_inout, Hb, Rb, s));
                if (gs.N > 0 && !corr_H_on_fft(ctx, gs, dtype)) {
                    // direct kernels: split-K partials, then ONE launch for their fixed-order sum, the blend into the
                    // accumulator and -- when the W update is the next operation -- that update as well
                    int P = 1;
                    double *partials = reinterpret_cast<double *>(ws_at(ctx, scm.part_off));
                    CHECK(do_corr_H_partials(ctx, gs, dtype, Vb, Rb, Hb, partials, &P, s));
                    const bool apply_now = i + 1 < n_ops && ops[i + 1].kind == TNMF_OP_APPLY_W;
                    if (apply_now) fft_invalidate_W(ctx);
                    CHECK(launch_finalize_blend_apply(g, dtype, partials, P, acc, op.a, op.b, apply_now, W_inout, eps, s));
                    if (apply_now) ++i;
                    break;
                }
                CHECK(do_corr_H(ctx, gs, dtype, sc, Vb, Rb, Hb, grad, grad + wn * es, s));
                CHECK(launch_axpby(ctx, dtype, acc, grad, op.a, op.b, 2 * wn, s));
                break;
            }
            case TNMF_OP_APPLY_W: {
                fft_invalidate_W(ctx);
                char *np = static_cast<char *>(acc);
                CHECK(launch_apply_normalize_W(g, dtype, W_inout, np, np + wn * es, eps, true, s));
                break;
            }
            default: return TNMF_E_UNSUPPORTED;
        }
    }
    return TNMF_OK;
}

int tnmf_hip_axpby(tnmf_hip_ctx *ctx, int dtype, void *acc, const void *g, double a, double b, size_t n_elems,
                   void *stream) {
    if (!ctx) return TNMF_E_NULL;
    if (dtype != 0 && dtype != 1) return TNMF_E_DTYPE;
    if (n_elems > 0 && (!acc || !g)) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return launch_axpby(ctx, dtype, acc, g, a, b, n_elems, static_cast<hipStream_t>(stream));
}

int tnmf_hip_sum_parts(tnmf_hip_ctx *ctx, int dtype, const void *parts, int n_parts, size_t n_elems, void *out,
                       void *stream) {
    if (!ctx) return TNMF_E_NULL;
    if (dtype != 0 && dtype != 1) return TNMF_E_DTYPE;
    if (n_parts < 1) return TNMF_E_GEOM;
    if (n_elems > 0 && (!parts || !out)) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return launch_sum_parts(ctx, dtype, parts, n_parts, n_elems, out, static_cast<hipStream_t>(stream));
}

int tnmf_hip_apply_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, void *W_inout, void *negpos, double eps,
                     void *stream) {
    if (is_vol(geom)) {
        VOL_ENTER(ctx, geom);
        if (!W_inout || !negpos) return TNMF_E_NULL;
        char *np3 = static_cast<char *>(negpos);
        return launch_apply_normalize_W(vol_dict_geo(v), dtype, W_inout, np3,
                                        np3 + (size_t)v.M * v.C * vol_avox(v) * esize(dtype), eps, true, s);
    }
    ENTER(ctx, geom);
    if (!W_inout || !negpos) return TNMF_E_NULL;
    fft_invalidate_W(ctx);
    char *np = static_cast<char *>(negpos);
    const size_t wbytes = (size_t)g.M * g.C * g.Ay * g.Ax * esize(dtype);
    return launch_apply_normalize_W(g, dtype, W_inout, np, np + wbytes, eps, true, s);
}

int tnmf_hip_find_peaks(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *H, double threshold, const int *radius,
                        int group, long long *idx_out, void *val_out, size_t capacity, unsigned long long *count_out,
                        void *stream) {
    if (!ctx || !geom || !radius) return TNMF_E_NULL;
    if (geom->dtype != 0 && geom->dtype != 1) return TNMF_E_DTYPE;
    if (geom->ndim < 1 || geom->ndim > 3 || geom->N < 0 || geom->M <= 0) return TNMF_E_GEOM;
    int S[3] = {1, 1, 1}, r[3] = {0, 0, 0};   // leading axes of extent 1: one scheme for 1, 2 and 3 shift axes
    for (int i = 0; i < geom->ndim; ++i) {
        const int k = 3 - geom->ndim + i;
        if (geom->D[i] <= 0 || geom->A[i] <= 0 || radius[i] < 0) return TNMF_E_GEOM;
        S[k] = geom->D[i] + geom->A[i] - 1;
        r[k] = std::min(radius[i], S[k] - 1);   // (a radius at or beyond the extent: the whole axis)
    }
    if (group < 1 || geom->M % group != 0) return TNMF_E_GEOM;
    if (geom->h_row_stride > 0 && geom->h_row_stride < S[2]) return TNMF_E_GEOM;
    if (!(threshold >= 0) || (long long)S[0] * S[1] > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    if (!count_out || (geom->N > 0 && !H) || (capacity > 0 && (!idx_out || !val_out))) return TNMF_E_NULL;
    PeakGeo g;
    g.planes = (long long)geom->N * geom->M;
    g.P = geom->M;
    g.Sz = S[0], g.Sy = S[1], g.Sx = S[2];
    g.Hs = geom->h_row_stride > 0 ? geom->h_row_stride : S[2];
    g.rz = r[0], g.ry = r[1], g.rx = r[2];
    g.group = group;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return peaks_find(ctx, g, geom->dtype, H, threshold, idx_out, val_out, capacity, count_out,
                      static_cast<hipStream_t>(stream));
}

int tnmf_hip_activation_correlogram(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *H, const int *max_lag,
                                    int per_sample, double *C_out, void *stream) {
    if (!ctx || !geom || !max_lag) return TNMF_E_NULL;
    if (geom->dtype != 0 && geom->dtype != 1) return TNMF_E_DTYPE;
    if (geom->ndim == 3) return TNMF_E_UNSUPPORTED;
    if ((geom->ndim != 1 && geom->ndim != 2) || geom->N < 0 || geom->M <= 0) return TNMF_E_GEOM;
    int S[2] = {1, 1};   // one shift axis: a single row
    for (int i = 0; i < geom->ndim; ++i) {
        if (geom->D[i] <= 0 || geom->A[i] <= 0) return TNMF_E_GEOM;
        if ((long long)geom->D[i] + geom->A[i] - 1 > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
        S[2 - geom->ndim + i] = geom->D[i] + geom->A[i] - 1;
    }
    if (geom->h_row_stride > 0 && geom->h_row_stride < S[1]) return TNMF_E_GEOM;
    const int Hs = geom->h_row_stride > 0 ? geom->h_row_stride : S[1];
    CorrPlan p;
    CHECK(correlogram_plan(geom->N, geom->M, S[0], S[1], Hs, geom->ndim, max_lag, per_sample != 0, geom->dtype, &p));
    if (!C_out || (geom->N > 0 && !H)) return TNMF_E_NULL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    if (geom->N == 0) {   // no sample: nothing per sample, and sums of nothing
        if (!per_sample)
            TNMF_HIP_TRY(hipMemsetAsync(C_out, 0, (size_t)p.P * p.P * (2 * p.Ly + 1) * (2 * p.Lx + 1) * sizeof(double), s));
        return TNMF_OK;
    }
    // work buffer: the partial sums per (segment, strip, pair of plane blocks, lag)
    CHECK(ensure_buffer(&ctx->ob, &ctx->ob_bytes, correlogram_partial_bytes(p), false));
    return launch_correlogram(p, geom->dtype, H, static_cast<double *>(ctx->ob), C_out, s);
}

// the arguments tnmf_hip_triggered_sums and its _plan share, checked, and the plan of the call
static int triggered_args(const tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int n_fields, const int *margin, int power,
                          int per_sample, TrigPlan *p) {
    if (!ctx || !geom || !margin) return TNMF_E_NULL;
    if (geom->dtype != 0 && geom->dtype != 1) return TNMF_E_DTYPE;
    if (geom->ndim == 3) return TNMF_E_UNSUPPORTED;
    if ((geom->ndim != 1 && geom->ndim != 2) || geom->N < 0 || geom->M <= 0) return TNMF_E_GEOM;
    for (int i = 0; i < geom->ndim; ++i)
        if (geom->D[i] <= 0 || geom->A[i] <= 0 || margin[i] < 0) return TNMF_E_GEOM;
    if (n_fields < 1 || (power != 1 && power != 2)) return TNMF_E_GEOM;
    const int last = geom->ndim - 1;
    if ((long long)geom->D[last] + geom->A[last] - 1 > 0x7fffffffLL || (long long)geom->D[0] + geom->A[0] - 1 > 0x7fffffffLL)
        return TNMF_E_UNSUPPORTED;
    const int Sx = geom->D[last] + geom->A[last] - 1;
    if (geom->h_row_stride > 0 && geom->h_row_stride < Sx) return TNMF_E_GEOM;
    return triggered_plan(geom->N, geom->M, n_fields, geom->D, geom->A, geom->h_row_stride > 0 ? geom->h_row_stride : Sx,
                          geom->ndim, margin, power, per_sample != 0, geom->dtype, p);
}

int tnmf_hip_triggered_sums_plan(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int n_fields, const int *margin,
                                 int per_sample, size_t *work_bytes) {
    TrigPlan p;
    CHECK(triggered_args(ctx, geom, n_fields, margin, 1, per_sample, &p));
    if (!work_bytes) return TNMF_E_NULL;
    *work_bytes = geom->N == 0 ? 0 : triggered_partial_bytes(p);
    return TNMF_OK;
}

int tnmf_hip_triggered_sums(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *H, const void *Y, int n_fields,
                            const int *margin, int power, int per_sample, void *work, size_t work_bytes,
                            double *X_out, void *stream) {
    TrigPlan p;
    CHECK(triggered_args(ctx, geom, n_fields, margin, power, per_sample, &p));
    if (!X_out || (work_bytes > 0 && !work) || (geom->N > 0 && (!H || !Y))) return TNMF_E_NULL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    if (geom->N == 0) {   // no sample: nothing per sample, and sums of nothing
        if (!per_sample)
            TNMF_HIP_TRY(hipMemsetAsync(X_out, 0, (size_t)p.P * p.F * p.Wy * p.Wx * sizeof(double), s));
        return TNMF_OK;
    }
    // the partial sums per (segment, strip, block of planes, cell) live in the caller's work buffer
    if (work_bytes < triggered_partial_bytes(p)) return TNMF_E_WORKSPACE;
    return launch_triggered(p, geom->dtype, H, Y, static_cast<double *>(work), X_out, s);
}

// the geometry of the events entry points, checked: ndim 1 or 2 (3: TNMF_E_UNSUPPORTED), every size positive
static int events_geo(const tnmf_hip_geom *geom, EventGeo *g) {
    if (geom->dtype != 0 && geom->dtype != 1) return TNMF_E_DTYPE;
    if (geom->ndim == 3) return TNMF_E_UNSUPPORTED;
    if (geom->ndim != 1 && geom->ndim != 2) return TNMF_E_GEOM;
    if (geom->N < 0 || geom->M <= 0 || geom->C <= 0) return TNMF_E_GEOM;
    for (int i = 0; i < geom->ndim; ++i)
        if (geom->D[i] <= 0 || geom->A[i] <= 0) return TNMF_E_GEOM;
    const bool two = geom->ndim == 2;
    g->N = geom->N, g->P = geom->M, g->C = geom->C;
    g->Dy = two ? geom->D[0] : 1, g->Dx = geom->D[two ? 1 : 0];
    g->Ay = two ? geom->A[0] : 1, g->Ax = geom->A[two ? 1 : 0];
    if ((long long)g->Dy + g->Ay > 0x7fffffffLL || (long long)g->Dx + g->Ax > 0x7fffffffLL ||
        (long long)g->C * g->Ay * g->Ax > 0x7fffffffLL)
        return TNMF_E_UNSUPPORTED;
    events_tile(geom->ndim, &g->ty, &g->tx);
    g->ncy = cdiv(g->Dy + g->Ay - 1, g->ty), g->ncx = cdiv(g->Dx + g->Ax - 1, g->tx);
    return TNMF_OK;
}

// the shift shape of a reconstruction mode, checked against the limits of modes.h, per axis
static int events_shift_shape(const EventGeo &g, int mode, int S[2]) {
    if (!mode_known(mode)) return TNMF_E_GEOM;
    S[0] = mode_shift_len(mode, g.Dy, g.Ay), S[1] = mode_shift_len(mode, g.Dx, g.Ax);
    return mode_axis_ok(mode, S[0], g.Ay) && mode_axis_ok(mode, S[1], g.Ax) ? TNMF_OK : TNMF_E_GEOM;
}

// the preamble of the events entry points that take a mode: the arguments that must be there, the geometry, the shift shape
// (a mode out of range is events_shift_shape's TNMF_E_GEOM)
static int events_enter(const tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, EventFrame *f) {
    if (!ctx || !geom) return TNMF_E_NULL;
    int S[2] = {0, 0};
    int rc = events_geo(geom, &f->g);
    if (rc == TNMF_OK) rc = events_shift_shape(f->g, mode, S);
    f->mode = mode, f->Sy = S[0], f->Sx = S[1];
    return rc;
}

int tnmf_hip_events_render(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *W_eff, const int *images,
                           long long n_images, const int *cell_start, const void *strength, long long n_events, void *R,
                           void *stream) {
    if (!ctx || !geom) return TNMF_E_NULL;
    EventGeo g;
    const int rc = events_geo(geom, &g);
    if (rc != TNMF_OK) return rc;
    if (n_images < 0 || n_events < 0) return TNMF_E_GEOM;
    if (n_images > 0x7fffffffLL || n_events > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    if (g.N > 0 && (!W_eff || !cell_start || !R || (n_images > 0 && (!images || !strength)))) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return events_render(ctx, g, geom->dtype, W_eff, images, n_images, cell_start, strength, n_events, R,
                         static_cast<hipStream_t>(stream));
}

int tnmf_hip_events_update(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff, const int *events,
                           void *strength_inout, long long n_events, const void *V, const void *R, double eps,
                           double sparsity, void *stream) {
    EventFrame f;
    const int rc = events_enter(ctx, geom, mode, &f);
    if (rc != TNMF_OK) return rc;
    if (n_events < 0) return TNMF_E_GEOM;
    if (!(eps >= 0) || !(sparsity >= 0)) return TNMF_E_UNSUPPORTED;
    if (n_events > 0 && f.g.N > 0 && (!W_eff || !events || !strength_inout || !V || !R)) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return events_update(ctx, f, geom->dtype, W_eff, events, strength_inout, n_events, V, R,
                         reg_of(eps, sparsity), static_cast<hipStream_t>(stream));
}

int tnmf_hip_events_gain(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff, const int *events,
                         const void *strength, long long n_events, const void *V, const void *R, double *gain, double *mag,
                         void *stream) {
    EventFrame f;
    const int rc = events_enter(ctx, geom, mode, &f);
    if (rc != TNMF_OK) return rc;
    if (n_events < 0) return TNMF_E_GEOM;
    if (n_events > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    if (n_events > 0 && f.g.N > 0 && (!W_eff || !events || !strength || !V || !R || !gain)) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return events_gain(ctx, f, geom->dtype, W_eff, events, strength, n_events, V, R, gain, mag,
                       static_cast<hipStream_t>(stream));
}

int tnmf_hip_events_grad_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const int *events, const int *by_plane,
                           const int *plane_start, const void *strength, long long n_events, const void *V, const void *R,
                           void *workspace, void *negpos_eff, void *stream) {
    EventFrame f;
    const int rc = events_enter(ctx, geom, mode, &f);
    if (rc != TNMF_OK) return rc;
    if (n_events < 0) return TNMF_E_GEOM;
    if (n_events > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    if (!negpos_eff) return TNMF_E_NULL;
    if (n_events > 0 && f.g.N > 0 && (!events || !by_plane || !plane_start || !strength || !V || !R || !workspace))
        return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return events_grad_W(ctx, f, geom->dtype, events, by_plane, plane_start, strength, n_events, V, R,
                         workspace, negpos_eff, static_cast<hipStream_t>(stream));
}

int tnmf_hip_events_norms(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff, double *b,
                          void *stream) {
    EventFrame f;
    const int rc = events_enter(ctx, geom, mode, &f);
    if (rc != TNMF_OK) return rc;
    if ((long long)f.Sy * f.Sx > 0x7fffffffLL || f.g.P > 65535) return TNMF_E_UNSUPPORTED;
    if (!W_eff || !b) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return events_norms(ctx, f, geom->dtype, W_eff, b, static_cast<hipStream_t>(stream));
}

int tnmf_hip_pursuit_score(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const void *a, const double *b, void *gain_out,
                           const long long *taken, long long n_taken, void *stream) {
    if (!ctx || !geom) return TNMF_E_NULL;
    if (geom->dtype != 0 && geom->dtype != 1) return TNMF_E_DTYPE;
    if (geom->ndim == 3) return TNMF_E_UNSUPPORTED;
    if (geom->ndim != 1 && geom->ndim != 2) return TNMF_E_GEOM;
    if (geom->N < 0 || geom->M <= 0 || n_taken < 0) return TNMF_E_GEOM;
    int S[2] = {1, 1};   // a leading axis of extent 1: one scheme for 1 and 2 shift axes
    for (int i = 0; i < geom->ndim; ++i) {
        if (geom->D[i] <= 0 || geom->A[i] <= 0) return TNMF_E_GEOM;
        if ((long long)geom->D[i] + geom->A[i] - 1 > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
        S[2 - geom->ndim + i] = geom->D[i] + geom->A[i] - 1;
    }
    if (geom->h_row_stride > 0 && geom->h_row_stride < S[1]) return TNMF_E_GEOM;
    if ((long long)geom->M * S[0] > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    if (geom->N > 0 && (!a || !b || !gain_out || (n_taken > 0 && !taken))) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return pursuit_score(ctx, geom->dtype, (long long)geom->N * geom->M, geom->M, S[0], S[1],
                         geom->h_row_stride > 0 ? geom->h_row_stride : S[1], a, b, gain_out, taken, n_taken,
                         static_cast<hipStream_t>(stream));
}

int tnmf_hip_pursuit_pick(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff, const long long *idx,
                          long long n_picked, const void *V, const void *R, int *events_out, void *strength_out,
                          double *gain_out, double *mag_out, void *stream) {
    EventFrame f;
    const int rc = events_enter(ctx, geom, mode, &f);
    if (rc != TNMF_OK) return rc;
    if (n_picked < 0) return TNMF_E_GEOM;
    if (n_picked > 0x7fffffffLL || (long long)f.Sy * f.Sx > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    if (n_picked > 0 && (!idx || !events_out || !strength_out || !gain_out || (f.g.N > 0 && (!W_eff || !V || !R))))
        return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return pursuit_pick(ctx, f, geom->dtype, W_eff, idx, n_picked, V, R, events_out, strength_out,
                        gain_out, mag_out, static_cast<hipStream_t>(stream));
}

int tnmf_hip_events_landscape(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff, const int *events,
                              const void *strength, long long n_events, const void *V, const void *R, double *a_out,
                              double *b_out, double *mag_out, void *stream) {
    EventFrame f;
    const int rc = events_enter(ctx, geom, mode, &f);
    if (rc != TNMF_OK) return rc;
    if (n_events < 0) return TNMF_E_GEOM;
    if (n_events > 0x7fffffffLL / 9) return TNMF_E_UNSUPPORTED;
    if (n_events > 0 && f.g.N > 0 && (!W_eff || !events || !strength || !V || !R || !a_out || !b_out)) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return events_landscape(ctx, f, geom->ndim, geom->dtype, W_eff, events, strength, n_events, V, R,
                            a_out, b_out, mag_out, static_cast<hipStream_t>(stream));
}

int tnmf_hip_events_alternatives(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff,
                                 const int *events, const void *strength, long long n_events, const void *V, const void *R,
                                 int n_alt, int stride, double *a_out, double *b_out, double *mag_out, void *stream) {
    EventFrame f;
    const int rc = events_enter(ctx, geom, mode, &f);
    if (rc != TNMF_OK) return rc;
    if (n_events < 0 || n_alt < 1 || stride < 1) return TNMF_E_GEOM;
    if ((long long)n_alt * stride > f.g.P || f.g.P % (n_alt * stride) != 0) return TNMF_E_GEOM;
    if (n_events > 0x7fffffffLL / n_alt) return TNMF_E_UNSUPPORTED;
    if (n_events > 0 && f.g.N > 0 && (!W_eff || !events || !strength || !V || !R || !a_out || !b_out)) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return events_alternatives(ctx, f, geom->dtype, W_eff, events, strength, n_events, V, R, n_alt,
                               stride, a_out, b_out, mag_out, static_cast<hipStream_t>(stream));
}

int tnmf_hip_events_pairs(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const int *images, long long n_images,
                          const int *cell_start, const int *events, long long n_events, long long *pairs_out,
                          size_t capacity, unsigned long long *count_out, void *stream) {
    if (!ctx || !geom) return TNMF_E_NULL;
    EventGeo g;
    const int rc = events_geo(geom, &g);
    if (rc != TNMF_OK) return rc;
    if (n_images < 0 || n_events < 0) return TNMF_E_GEOM;
    if (n_images > 0x7fffffffLL || n_events > 0x7fffffffLL || capacity > 0x7fffffffULL) return TNMF_E_UNSUPPORTED;
    if (!count_out || (capacity > 0 && !pairs_out)) return TNMF_E_NULL;
    if (n_images > 0 && n_events > 0 && g.N > 0 && (!images || !cell_start || !events)) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return events_pairs(ctx, g, images, n_images, cell_start, events, n_events, pairs_out, capacity, count_out,
                        static_cast<hipStream_t>(stream));
}

int tnmf_hip_events_gram(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff, const int *events,
                         long long n_events, const int *row_i, const int *row_j, long long n_pairs, double *val_out,
                         void *stream) {
    EventFrame f;
    const int rc = events_enter(ctx, geom, mode, &f);
    if (rc != TNMF_OK) return rc;
    if (n_events < 0 || n_pairs < 0) return TNMF_E_GEOM;
    if (n_events > 0x7fffffffLL || n_pairs > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    if (n_pairs > 0 && (!row_i || !row_j || !val_out || (n_events > 0 && (!W_eff || !events)))) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return events_gram(ctx, f, geom->dtype, W_eff, events, n_events, row_i, row_j, n_pairs, val_out,
                       static_cast<hipStream_t>(stream));
}

int tnmf_hip_events_project(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, const void *W_eff, const int *events,
                            long long n_events, const void *V, double *c_out, void *stream) {
    EventFrame f;
    const int rc = events_enter(ctx, geom, mode, &f);
    if (rc != TNMF_OK) return rc;
    if (n_events < 0) return TNMF_E_GEOM;
    if (n_events > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    if (n_events > 0 && (!events || !c_out || (f.g.N > 0 && (!W_eff || !V)))) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return events_project(ctx, f, geom->dtype, W_eff, events, n_events, V, c_out, static_cast<hipStream_t>(stream));
}

int tnmf_hip_events_nnls(tnmf_hip_ctx *ctx, long long n_rows, long long nnz, const int *row_start, const int *col,
                         const double *val, const double *c, double *h_inout, double tol, int max_iterations,
                         int check_every, double *workspace, int *iterations_out, double *kkt_out, int *converged_out,
                         double *history_out, int history_capacity, int *n_history_out, void *stream) {
    if (!ctx || !iterations_out || !kkt_out || !converged_out) return TNMF_E_NULL;
    if (n_rows < 0 || nnz < 0 || max_iterations < 0 || check_every < 1 || history_capacity < 0) return TNMF_E_GEOM;
    if (!(tol > 0) || !std::isfinite(tol) || n_rows > 0x7fffffffLL || nnz > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    if (history_capacity > 0 && !history_out) return TNMF_E_NULL;
    if (n_rows > 0 && (!row_start || !c || !h_inout || !workspace || (nnz > 0 && (!col || !val)))) return TNMF_E_NULL;
    if (n_rows == 0) {
        *iterations_out = 0, *kkt_out = 0., *converged_out = 1;
        if (n_history_out) *n_history_out = 0;
        return TNMF_OK;
    }
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return events_nnls(ctx, (int)n_rows, (int)nnz, row_start, col, val, c, h_inout, tol, max_iterations, check_every,
                       workspace, iterations_out, kkt_out, converged_out, history_out, history_capacity, n_history_out,
                       static_cast<hipStream_t>(stream));
}

int tnmf_hip_events_inverse_diag(tnmf_hip_ctx *ctx, long long n_rows, long long nnz, const int *row_start, const int *col,
                                 const double *val, long long n_comp, const int *comp_start, const int *comp_sizes,
                                 long long n_active, const int *member, const int *local, double *scratch,
                                 long long scratch_doubles, double *d_out, int *status_out, void *stream) {
    if (!ctx) return TNMF_E_NULL;
    if (n_rows < 0 || nnz < 0 || n_comp < 0 || n_active < 0 || scratch_doubles < 0) return TNMF_E_NULL;
    if (n_rows > 0 && (!row_start || !local || !d_out || (nnz > 0 && (!col || !val)))) return TNMF_E_NULL;
    if (n_comp > 0 && (!comp_start || !comp_sizes || !member || !status_out)) return TNMF_E_NULL;
    if (n_rows > 0x7fffffffLL || nnz > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    if (n_active > n_rows || n_comp > n_active) return TNMF_E_GEOM;
    long long total = 0, previous = 1;
    for (long long c = 0; c < n_comp; ++c) {   // (the host copy of the sizes: every launch is planned from it)
        const long long n = comp_sizes[c];
        if (n < previous) return TNMF_E_GEOM;
        previous = n, total += n;
        if (total > n_active) return TNMF_E_GEOM;
    }
    if (total != n_active) return TNMF_E_GEOM;
    if (n_comp > 0 && previous > kInverseDiagLds) {
        if (events_inverse_diag_tile(previous) > scratch_doubles) return TNMF_E_GEOM;
        if (!scratch) return TNMF_E_NULL;
    }
    if (n_rows == 0) return TNMF_OK;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return events_inverse_diag(ctx, (int)n_rows, (int)nnz, row_start, col, val, (int)n_comp, comp_start, comp_sizes,
                               (int)n_active, member, local, scratch, scratch_doubles, d_out, status_out,
                               static_cast<hipStream_t>(stream));
}

int tnmf_hip_events_patches(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int mode, int source, const void *W_eff,
                            const int *events, const void *strength, long long n_events, const void *V, const void *R,
                            const int *fold_ptr, const int *fold_src, const double *fold_w, int T, double *out,
                            void *stream) {
    EventFrame f;
    const int rc = events_enter(ctx, geom, mode, &f);
    if (rc != TNMF_OK) return rc;
    if (n_events < 0 || source < TNMF_PATCH_DATA || source > TNMF_PATCH_CLEANED || T < 1 || f.g.P % T != 0) return TNMF_E_GEOM;
    const long long taps = (long long)f.g.C * f.g.Ay * f.g.Ax;
    if (fold_ptr && !patches_stage_fits(taps)) return TNMF_E_GEOM;
    if (n_events > 0x7fffffffLL || n_events > 0x7fffffffLL / taps) return TNMF_E_UNSUPPORTED;
    if (n_events > 0 && f.g.N > 0) {
        if (!events || !V || !out || (fold_ptr && (!fold_src || !fold_w))) return TNMF_E_NULL;
        if (source != TNMF_PATCH_DATA && (!R || !W_eff || !strength)) return TNMF_E_NULL;
    }
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return events_patches(ctx, f, geom->dtype, source, W_eff, events, strength, n_events, V, R, fold_ptr, fold_src, fold_w, T,
                          out, static_cast<hipStream_t>(stream));
}

int tnmf_hip_patch_moments(tnmf_hip_ctx *ctx, int D, int n_atoms, const double *Y, const double *strength_d,
                           const int *by_atom, const int *atom_start, long long n_rows, int accumulate, double *S, double *g,
                           double *s2, double *count, void *stream) {
    if (!ctx || !atom_start || !S || !g || !s2 || !count) return TNMF_E_NULL;
    if (D <= 0 || n_atoms <= 0 || n_rows < 0) return TNMF_E_GEOM;
    if ((long long)n_atoms * D > 0x7fffffffLL / D || n_rows > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    if (n_rows > 0 && (!Y || !strength_d || !by_atom)) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    return patch_moments(ctx, D, n_atoms, Y, strength_d, by_atom, atom_start, (int)n_rows, accumulate, S, g, s2, count,
                         static_cast<hipStream_t>(stream));
}

}  // extern "C"
