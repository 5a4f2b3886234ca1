// atom_ops.hip -- atom operators (include/tnmf_hip.h, "atom operators"): the dictionary W of M atoms stands for M * T
// effective atoms W_eff[m * T + t, c] = L_t W[m, c], every L_t a non-negative linear map of the atom's pixels (a rotation
// by any angle, a rescaling, ...; the permutations of group.hip are the special case of one tap of weight 1).  The H half
// step, the reconstruction and the energy run unchanged on W_eff; the W half step folds the gradient of W_eff back onto W
// with the transpose, neg[m, c] = sum_t L_t^T neg_eff[m * T + t, c] (pos likewise).
//
// A handle holds the maps as two gather tables resident on the device (nA = pixels of an atom):
//   forward  per (t, out pixel) q, row t * nA + q:  its taps (in pixel, weight), ascending in pixel
//   adjoint  per in pixel p:                        its entries (t * nA + out pixel, weight), ascending (t, out pixel)
// Every output element is the sum of its products weight * (double)x in table order, in double with separate multiplies
// and adds (this file is compiled with -ffp-contract=off: the float64 reference forms the same sums), rounded once to the
// element type.  A table of one
// tap of weight 1.0 per (t, q) -- a group -- gives exactly group.hip's bits.
//
// The buffers are tiny (M * T * C * nA elements, a few taps each): these kernels are a few microseconds of dependent
// launches, so they are written for a short chain, not for bandwidth.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "common.h"
#include "fft.h"
#include "rowsum.h"

struct tnmf_hip_atom_ops {
    tnmf_hip_ctx *ctx;   // the context it was made for (entry points on another context are refused)
    int device;
    int ndim, A[2];      // atom shape (ndim 1 or 2)
    int T, nA, nnz;
    void *dev;           // one device allocation: the six arrays below
    const int *fwd_ptr;  // [T * nA + 1]
    const int *fwd_in;   // [nnz]
    const double *fwd_w; // [nnz]
    const int *adj_ptr;  // [nA + 1]
    const int *adj_tq;   // [nnz]  t * nA + out pixel
    const double *adj_w; // [nnz]
};

namespace {

constexpr int kBlock = 256;                 // (the workgroup of apply_normalize_row: the fused update reduces rows in the
                                            // same order)
constexpr size_t kMaxLdsBytes = 64 * 1024;  // LDS of the fused update: the normalised row (and the [neg | pos] slice)

struct Tables {
    int T, nA;
    const int *fwd_ptr, *fwd_in;
    const double *fwd_w;
    const int *adj_ptr, *adj_tq;
    const double *adj_w;
};

struct Dict {
    int M, C;
};

Tables tables_of(const tnmf_hip_atom_ops *o) {
    return Tables{o->T, o->nA, o->fwd_ptr, o->fwd_in, o->fwd_w, o->adj_ptr, o->adj_tq, o->adj_w};
}

// the dictionary geometry of a call, checked against the handle
int to_dict(const tnmf_hip_ctx *ctx, const tnmf_hip_geom *in, const tnmf_hip_atom_ops *ops, Dict *d) {
    if (!in || !ops) return TNMF_E_NULL;
    if (in->dtype != 0 && in->dtype != 1) return TNMF_E_DTYPE;
    if (in->ndim == 3) return TNMF_E_UNSUPPORTED;   // (no transforms for volumes)
    if (ops->ctx != ctx) return TNMF_E_UNSUPPORTED; // (a handle of another context)
    if (in->ndim != ops->ndim) return TNMF_E_GEOM;
    for (int i = 0; i < in->ndim; ++i)
        if (in->A[i] != ops->A[i]) return TNMF_E_GEOM;
    if (in->M <= 0 || in->C <= 0) return TNMF_E_GEOM;
    // (every index below is an int: refuse what would not fit)
    if ((long long)in->M * std::max(ops->T, 2) * in->C * ops->nA >= (1LL << 31)) return TNMF_E_GEOM;
    d->M = in->M;
    d->C = in->C;
    return TNMF_OK;
}

// sum of w[k] * x(k) over k in [k0, k1), in double, multiplies and adds rounded separately (the float64 reference's sums)
template <typename F>
__device__ __forceinline__ double dot_ordered(int k0, int k1, const double *__restrict__ w, F x) {
    double s = 0.0;
    for (int k = k0; k < k1; ++k) {
        const double prod = w[k] * x(k);
        s = s + prod;
    }
    return s;
}

// the same for two sequences over one table row (the fold of neg and of pos): each entry's index and weight read once
template <typename F>
__device__ __forceinline__ void dot2_ordered(int k0, int k1, const int *__restrict__ idx, const double *__restrict__ w,
                                             F x, double &sa, double &sb) {
    double a = 0.0, b = 0.0;
#pragma unroll 4
    for (int k = k0; k < k1; ++k) {
        const double wk = w[k];
        double xa, xb;
        x(idx[k], xa, xb);
        const double pa = wk * xa, pb = wk * xb;
        a = a + pa;
        b = b + pb;
    }
    sa = a;
    sb = b;
}

// W_eff[(m*T + t)*C + c][q] = L_t row (m, c) at q: one thread per element of W_eff (the writes are coalesced)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ops_expand(Tables tb, Dict d, const T *__restrict__ W, T *__restrict__ W_eff) {
    const int nA = tb.nA, total = d.M * tb.T * d.C * nA;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < total; i += gridDim.x * kBlock) {
        const int q = i % nA, row = i / nA;   // row = (m*T + t)*C + c
        const int c = row % d.C, mt = row / d.C;
        const int t = mt % tb.T, m = mt / tb.T;
        const T *src = W + (size_t)(m * d.C + c) * nA;
        const int r = t * nA + q;
        W_eff[i] = (T)dot_ordered(tb.fwd_ptr[r], tb.fwd_ptr[r + 1], tb.fwd_w,
                                  [&](int k) { return (double)src[tb.fwd_in[k]]; });
    }
}

// (sum_t L_t^T X[m*T + t, c]) at pixel p: the adjoint entries of p in table order
template <typename T>
__device__ __forceinline__ double fold_at(const Tables &tb, const Dict &d, const T *__restrict__ X, int m, int c, int p) {
    const int nA = tb.nA;
    return dot_ordered(tb.adj_ptr[p], tb.adj_ptr[p + 1], tb.adj_w, [&](int k) {
        const int tq = tb.adj_tq[k], t = tq / nA, q = tq % nA;
        return (double)X[(size_t)((m * tb.T + t) * d.C + c) * nA + q];
    });
}

// [neg | pos] of W_eff ([2][M*T][C][nA]) -> [neg | pos] of W ([2][M][C][nA]), every element rounded once
template <typename T>
__global__ __launch_bounds__(kBlock) void k_ops_fold(Tables tb, Dict d, const T *__restrict__ negpos_eff,
                                                     T *__restrict__ negpos) {
    const int nA = tb.nA, half = d.M * d.C * nA;
    const size_t half_eff = (size_t)half * tb.T;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < 2 * half; i += gridDim.x * kBlock) {
        const int h = i / half, e = i % half;
        const int p = e % nA, row = e / nA;
        negpos[i] = (T)fold_at(tb, d, negpos_eff + h * half_eff, row / d.C, row % d.C, p);
    }
}

// The single-rank W step after the gradient of W_eff, in one launch: fold, W = W * neg / (pos + eps), W /= its sum over
// the atom axes (the arithmetic and the reduction order of apply_normalize_row), the new row staged in LDS, then its T
// images gathered into W_eff.  One workgroup per (m, c) row.  STAGE: the row's slice of [neg | pos] of W_eff (2 * T * nA
// elements) is first copied into LDS with coalesced loads and folded from there (the adjoint table's t * nA + q indexes
// it directly) -- the same values in the same order, so the same bits -- instead of T scattered global loads per pixel.
template <typename T, bool STAGE>
__global__ __launch_bounds__(kBlock) void k_ops_apply(Tables tb, Dict d, T *__restrict__ W, T *__restrict__ W_eff,
                                                      const T *__restrict__ negpos_eff, T eps) {
    __shared__ double sh[kBlock / 64];
    extern __shared__ unsigned char lds_raw[];
    T *row_lds = reinterpret_cast<T *>(lds_raw);   // [nA]; then with STAGE: neg [T * nA], pos [T * nA]
    const int nA = tb.nA, TA = tb.T * nA;
    const size_t half_eff = (size_t)d.M * tb.T * d.C * nA;
    const int row = blockIdx.x, m = row / d.C, c = row % d.C;
    const size_t base = (size_t)row * nA;
    T *neg_lds = row_lds + nA, *pos_lds = row_lds + nA + TA;
    if (STAGE) {
        for (int j = threadIdx.x; j < TA; j += kBlock) {
            const size_t g = (size_t)((m * tb.T + j / nA) * d.C + c) * nA + j % nA;
            neg_lds[j] = negpos_eff[g];
            pos_lds[j] = negpos_eff[half_eff + g];
        }
        __syncthreads();
    }
    double part = 0.0;
    for (int i = threadIdx.x; i < nA; i += kBlock) {
        T neg, p;
        if (STAGE) {
            double sn, sp;
            dot2_ordered(tb.adj_ptr[i], tb.adj_ptr[i + 1], tb.adj_tq, tb.adj_w,
                         [&](int tq, double &xn, double &xp) {
                             xn = (double)neg_lds[tq];
                             xp = (double)pos_lds[tq];
                         },
                         sn, sp);
            neg = (T)sn;
            p = (T)sp + eps;
        } else {
            neg = (T)fold_at(tb, d, negpos_eff, m, c, i);
            p = (T)fold_at(tb, d, negpos_eff + half_eff, m, c, i) + eps;
        }
        const T w = (W[base + i] * neg) / p;
        W[base + i] = w;
        part += (double)w;
    }
    const T tot = (T)block_sum<T>(part, sh);
    for (int i = threadIdx.x; i < nA; i += kBlock) {
        const T w = W[base + i] / tot;
        W[base + i] = w;
        row_lds[i] = w;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < TA; j += kBlock) {
        const int t = j / nA, q = j % nA;
        W_eff[(size_t)((m * tb.T + t) * d.C + c) * nA + q] =
            (T)dot_ordered(tb.fwd_ptr[j], tb.fwd_ptr[j + 1], tb.fwd_w, [&](int k) { return (double)row_lds[tb.fwd_in[k]]; });
    }
}

template <typename T>
void launch_apply(hipStream_t s, const Tables &tb, const Dict &d, T *W, T *W_eff, const T *negpos_eff, T eps) {
    const size_t row = (size_t)tb.nA * sizeof(T), staged = row * (1 + 2 * (size_t)tb.T);
    if (staged <= kMaxLdsBytes)
        hipLaunchKernelGGL((k_ops_apply<T, true>), dim3(d.M * d.C), dim3(kBlock), staged, s, tb, d, W, W_eff,
                           negpos_eff, eps);
    else
        hipLaunchKernelGGL((k_ops_apply<T, false>), dim3(d.M * d.C), dim3(kBlock), row, s, tb, d, W, W_eff, negpos_eff,
                           eps);
}

#define CHECK_RC(rc_expr)               \
    do {                                \
        const int _rc = (rc_expr);      \
        if (_rc != TNMF_OK) return _rc; \
    } while (0)

int grid_of(int n) { return n <= 0 ? 1 : std::min(cdiv(n, kBlock), 1024); }

}  // namespace

extern "C" {

int tnmf_hip_atom_ops_create(tnmf_hip_ctx *ctx, int ndim, const int *A, int T, int nnz, const int *t,
                             const int *out_px, const int *in_px, const double *w, tnmf_hip_atom_ops **out) {
    if (!ctx || !out || !A) return TNMF_E_NULL;
    if (ndim == 3) return TNMF_E_UNSUPPORTED;   // (no transforms for volumes)
    if (ndim != 1 && ndim != 2) return TNMF_E_GEOM;
    for (int i = 0; i < ndim; ++i)
        if (A[i] <= 0) return TNMF_E_GEOM;
    const long long nA = ndim == 1 ? A[0] : (long long)A[0] * A[1];
    if (T <= 0 || nnz < 0 || (long long)T * nA >= (1LL << 31)) return TNMF_E_GEOM;
    if (nnz > 0 && (!t || !out_px || !in_px || !w)) return TNMF_E_NULL;
    for (int k = 0; k < nnz; ++k) {
        if (t[k] < 0 || t[k] >= T || out_px[k] < 0 || out_px[k] >= nA || in_px[k] < 0 || in_px[k] >= nA)
            return TNMF_E_GEOM;
        if (!std::isfinite(w[k]) || w[k] < 0.0) return TNMF_E_UNSUPPORTED;
    }
    // forward order: (t, out, in); a repeated triple is refused
    auto key = [&](int k) { return ((long long)t[k] * nA + out_px[k]) * nA + in_px[k]; };
    std::vector<int> fwd(nnz);
    std::iota(fwd.begin(), fwd.end(), 0);
    std::sort(fwd.begin(), fwd.end(), [&](int a, int b) { return key(a) < key(b); });
    for (int k = 1; k < nnz; ++k)
        if (key(fwd[k]) == key(fwd[k - 1])) return TNMF_E_GEOM;
    // adjoint order: (in, t, out)
    std::vector<int> adj(fwd);
    std::stable_sort(adj.begin(), adj.end(), [&](int a, int b) { return in_px[a] < in_px[b]; });

    const int nR = (int)(T * nA), nP = (int)nA;
    std::vector<int> fwd_ptr(nR + 1, 0), fwd_in(nnz), adj_ptr(nP + 1, 0), adj_tq(nnz);
    std::vector<double> fwd_w(nnz), adj_w(nnz);
    for (int k = 0; k < nnz; ++k) {
        const int e = fwd[k];
        ++fwd_ptr[t[e] * nA + out_px[e] + 1];
        fwd_in[k] = in_px[e];
        fwd_w[k] = w[e];
        const int a = adj[k];
        ++adj_ptr[in_px[a] + 1];
        adj_tq[k] = (int)(t[a] * nA + out_px[a]);
        adj_w[k] = w[a];
    }
    std::partial_sum(fwd_ptr.begin(), fwd_ptr.end(), fwd_ptr.begin());
    std::partial_sum(adj_ptr.begin(), adj_ptr.end(), adj_ptr.begin());

    // one allocation: doubles first (8-byte aligned), then the ints
    const size_t n_dbl = 2 * (size_t)nnz, n_int = (size_t)(nR + 1) + (size_t)(nP + 1) + 2 * (size_t)nnz;
    std::vector<unsigned char> host(n_dbl * sizeof(double) + n_int * sizeof(int));
    double *hd = reinterpret_cast<double *>(host.data());
    int *hi = reinterpret_cast<int *>(host.data() + n_dbl * sizeof(double));
    std::copy(fwd_w.begin(), fwd_w.end(), hd);
    std::copy(adj_w.begin(), adj_w.end(), hd + nnz);
    int *p = hi;
    p = std::copy(fwd_ptr.begin(), fwd_ptr.end(), p);
    p = std::copy(fwd_in.begin(), fwd_in.end(), p);
    p = std::copy(adj_ptr.begin(), adj_ptr.end(), p);
    std::copy(adj_tq.begin(), adj_tq.end(), p);

    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    void *dev = nullptr;
    if (hipMalloc(&dev, host.size()) != hipSuccess) return TNMF_E_WORKSPACE;
    const hipError_t e = hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(dev);
        return (int)e;
    }
    auto *o = new tnmf_hip_atom_ops;
    o->ctx = ctx;
    o->device = ctx->device;
    o->ndim = ndim;
    o->A[0] = A[0];
    o->A[1] = ndim == 2 ? A[1] : 0;
    o->T = T;
    o->nA = nP;
    o->nnz = nnz;
    o->dev = dev;
    const double *dd = static_cast<const double *>(dev);
    const int *di = reinterpret_cast<const int *>(static_cast<const unsigned char *>(dev) + n_dbl * sizeof(double));
    o->fwd_w = dd;
    o->adj_w = dd + nnz;
    o->fwd_ptr = di;
    o->fwd_in = di + nR + 1;
    o->adj_ptr = di + nR + 1 + nnz;
    o->adj_tq = di + nR + 1 + nnz + nP + 1;
    *out = o;
    return TNMF_OK;
}

int tnmf_hip_atom_ops_destroy(tnmf_hip_atom_ops *ops) {
    if (!ops) return TNMF_OK;
    int rc = TNMF_OK;
    if (hipSetDevice(ops->device) == hipSuccess) {
        const hipError_t e = hipFree(ops->dev);
        if (e != hipSuccess) rc = (int)e;
    }
    delete ops;
    return rc;
}

int tnmf_hip_ops_expand_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const tnmf_hip_atom_ops *ops, const void *W,
                          void *W_eff, void *stream) {
    if (!ctx) return TNMF_E_NULL;
    Dict d;
    CHECK_RC(to_dict(ctx, geom, ops, &d));
    if (!W || !W_eff) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    fft_invalidate_W(ctx);   // (W_eff: a fixed address with new contents -- its cached spectra are stale)
    const Tables tb = tables_of(ops);
    const int n = d.M * tb.T * d.C * tb.nA;
    with_dtype(geom->dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_ops_expand<T>, dim3(grid_of(n)), dim3(kBlock), 0, s, tb, d, (const T *)W, (T *)W_eff);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

int tnmf_hip_ops_fold_grad_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const tnmf_hip_atom_ops *ops,
                             const void *negpos_eff, void *negpos, void *stream) {
    if (!ctx) return TNMF_E_NULL;
    Dict d;
    CHECK_RC(to_dict(ctx, geom, ops, &d));
    if (!negpos_eff || !negpos) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Tables tb = tables_of(ops);
    const int n = 2 * d.M * d.C * tb.nA;
    with_dtype(geom->dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_ops_fold<T>, dim3(grid_of(n)), dim3(kBlock), 0, s, tb, d, (const T *)negpos_eff, (T *)negpos);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

int tnmf_hip_ops_apply_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, const tnmf_hip_atom_ops *ops, void *W_inout,
                         void *W_eff_out, const void *negpos_eff, double eps, void *stream) {
    if (!ctx) return TNMF_E_NULL;
    Dict d;
    CHECK_RC(to_dict(ctx, geom, ops, &d));
    if (!W_inout || !W_eff_out || !negpos_eff) return TNMF_E_NULL;
    const size_t lds = (size_t)ops->nA * esize(geom->dtype);
    if (lds > kMaxLdsBytes) return TNMF_E_GEOM;   // (a row larger than the LDS staging)
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    fft_invalidate_W(ctx);
    const Tables tb = tables_of(ops);
    with_dtype(geom->dtype, [&](auto zero) {
        using T = decltype(zero);
        launch_apply<T>(s, tb, d, (T *)W_inout, (T *)W_eff_out, (const T *)negpos_eff, (T)eps);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

}  // extern "C"
