// beta.hip -- the elementwise kernels of the beta-divergence and weighted objectives (beta.h): the fields Q, P that stand
// in for V, R in the correlations of a multiplicative update, the (weighted) D_beta energy and the same objective per sample.
// Streaming kernels: 16-byte loads and stores for aligned operands, a scalar tail for lengths that are not a whole number of vectors.
#include <cmath>
#include <cstdint>

#include "beta.h"

namespace {

constexpr int kBlock = 256;

// K: 0 = Itakura-Saito (beta 0), 1 = Kullback-Leibler (beta 1), 2 = Frobenius (beta 2), 3 = any other beta (pow)
template <int K, typename T>
__device__ __forceinline__ void field(T v, T r, T eps, T bm2, T bm1, T &q, T &p) {
    const T rt = (r > T(0) ? r : T(0)) + eps;
    if constexpr (K == 0) {
        p = T(1) / rt;
        q = v / (rt * rt);
    } else if constexpr (K == 1) {
        p = T(1);
        q = v / rt;
    } else if constexpr (K == 2) {
        p = rt;
        q = v;
    } else {
        p = pow(rt, bm1);
        q = v * pow(rt, bm2);
    }
}

// the weighted fields G * (Q, P); K == 2 is the weighted Frobenius step itself (Q = G V, P = G R: no clamp, no eps).
// g <= 0 selects 0: what V and R~^(beta-2) hold there (NaN, inf, an overflow) never reaches Q or P.
template <int K, typename T>
__device__ __forceinline__ void wfield(T v, T g, T r, T eps, T bm2, T bm1, T &q, T &p) {
    T q0, p0;
    if constexpr (K == 2) {
        q0 = g * v;
        p0 = g * r;
    } else {
        field<K, T>(v, r, eps, bm2, bm1, q0, p0);
        q0 = g * q0;
        p0 = K == 1 ? g : g * p0;
    }
    q = g > T(0) ? q0 : T(0);
    p = g > T(0) ? p0 : T(0);
}

template <typename T> struct Vec;
template <> struct Vec<float> { using type = float4; static constexpr int n = 4; };
template <> struct Vec<double> { using type = double2; static constexpr int n = 2; };

template <typename VT, typename T>
__device__ __forceinline__ T &lane(VT &v, int i) { return reinterpret_cast<T *>(&v)[i]; }

// vec: every operand 16-byte aligned -> n / L vector iterations, then the scalar tail; else everything scalar.
// kW: weighted (G read on the same path as V and R); else G is not read.
template <int K, typename T, bool kVec, bool kW>
__global__ __launch_bounds__(kBlock) void k_beta_fields(const T *__restrict__ V, const T *__restrict__ G, const T *R,
                                                        T *__restrict__ Q, T *P, size_t n, T eps, T bm2, T bm1) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t done = 0;
    if constexpr (kVec) {
        using VT = typename Vec<T>::type;
        constexpr int L = Vec<T>::n;
        const size_t nv = n / L;
        for (size_t i = tid; i < nv; i += stride) {
            VT v = reinterpret_cast<const VT *>(V)[i];
            VT r = reinterpret_cast<const VT *>(R)[i];   // (read once: P may alias R)
            VT q, p;
            if constexpr (kW) {
                VT g = reinterpret_cast<const VT *>(G)[i];
#pragma unroll
                for (int j = 0; j < L; ++j)
                    wfield<K, T>(lane<VT, T>(v, j), lane<VT, T>(g, j), lane<VT, T>(r, j), eps, bm2, bm1,
                                 lane<VT, T>(q, j), lane<VT, T>(p, j));
            } else {
#pragma unroll
                for (int j = 0; j < L; ++j)
                    field<K, T>(lane<VT, T>(v, j), lane<VT, T>(r, j), eps, bm2, bm1, lane<VT, T>(q, j),
                                lane<VT, T>(p, j));
            }
            reinterpret_cast<VT *>(Q)[i] = q;
            reinterpret_cast<VT *>(P)[i] = p;
        }
        done = nv * L;
    }
    for (size_t i = done + tid; i < n; i += stride) {
        T q, p;
        if constexpr (kW)
            wfield<K, T>(V[i], G[i], R[i], eps, bm2, bm1, q, p);
        else
            field<K, T>(V[i], R[i], eps, bm2, bm1, q, p);
        Q[i] = q;
        P[i] = p;
    }
}

__device__ __forceinline__ double block_sum(double x, double *sh) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    const int w = threadIdx.x / 64, l = threadIdx.x % 64;
    if (l == 0) sh[w] = x;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < kBlock / 64; ++i) t += sh[i];
    return t;
}

// D_beta(v | r~) of one element in double (r~ = max(r, 0) + eps)
template <int K>
__device__ __forceinline__ double divergence(double v, double r, double eps, double beta) {
    const double rt = (r > 0.0 ? r : 0.0) + eps;
    if constexpr (K == 0) {
        const double x = v / rt;
        return x - log(x) - 1.0;
    } else if constexpr (K == 1) {
        return (v > 0.0 ? v * log(v / rt) : 0.0) - v + rt;   // (0 log 0 = 0)
    } else {
        return (pow(v, beta) + (beta - 1.0) * pow(rt, beta) - beta * v * pow(rt, beta - 1.0)) / (beta * (beta - 1.0));
    }
}

// kW: G * D_beta, and K == 2 (weighted only) 1/2 G (V - R)^2; entries with G <= 0 add exactly 0 (selected, whatever V holds)
template <int K, typename T, bool kW>
__global__ __launch_bounds__(kBlock) void k_beta_energy(const T *__restrict__ V, const T *__restrict__ G,
                                                        const T *__restrict__ R, size_t n, double eps, double beta,
                                                        double *__restrict__ partial) {
    __shared__ double sh[kBlock / 64];
    double acc = 0.0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if constexpr (kW) {
            const double g = (double)G[i];
            double d;
            if constexpr (K == 2) {
                const double e = (double)V[i] - (double)R[i];
                d = 0.5 * e * e;
            } else {
                d = divergence<K>((double)V[i], (double)R[i], eps, beta);
            }
            acc += g > 0.0 ? g * d : 0.0;
        } else {
            acc += divergence<K>((double)V[i], (double)R[i], eps, beta);
        }
    }
    const double tot = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kBlock) void k_beta_sum(const double *__restrict__ partial, int n, double *__restrict__ out) {
    __shared__ double sh[kBlock / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) acc += partial[i];
    const double tot = block_sum(acc, sh);
    if (threadIdx.x == 0) *out = tot;
}

inline int grid_of(size_t work, const tnmf_hip_ctx *ctx) {
    const size_t want = (work + kBlock - 1) / kBlock;
    const size_t cap = (size_t)ctx->num_cu * 8;
    return (int)(want < cap ? (want ? want : 1) : cap);
}

template <int K, typename T, bool kW>
int fields_as(const tnmf_hip_ctx *ctx, double beta, double eps, const void *V, const void *G, const void *R, void *Q,
              void *P, size_t n, hipStream_t s) {
    const bool vec = ((reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(R) |
                       reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(P)) & 15) == 0;
    const int grid = grid_of(vec ? n / Vec<T>::n + 1 : n, ctx);
    const T e = (T)eps, bm2 = (T)(beta - 2.0), bm1 = (T)(beta - 1.0);
    if (vec)
        hipLaunchKernelGGL((k_beta_fields<K, T, true, kW>), dim3(grid), dim3(kBlock), 0, s, (const T *)V, (const T *)G,
                           (const T *)R, (T *)Q, (T *)P, n, e, bm2, bm1);
    else
        hipLaunchKernelGGL((k_beta_fields<K, T, false, kW>), dim3(grid), dim3(kBlock), 0, s, (const T *)V, (const T *)G,
                           (const T *)R, (T *)Q, (T *)P, n, e, bm2, bm1);
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

template <typename T, bool kW>
int fields_weighted_as(const tnmf_hip_ctx *ctx, double beta, double eps, const void *V, const void *G, const void *R,
                       void *Q, void *P, size_t n, hipStream_t s) {
    if (beta == 0.0) return fields_as<0, T, kW>(ctx, beta, eps, V, G, R, Q, P, n, s);
    if (beta == 1.0) return fields_as<1, T, kW>(ctx, beta, eps, V, G, R, Q, P, n, s);
    if (beta == 2.0) return fields_as<2, T, kW>(ctx, beta, eps, V, G, R, Q, P, n, s);
    return fields_as<3, T, kW>(ctx, beta, eps, V, G, R, Q, P, n, s);
}

template <typename T>
int fields_typed(const tnmf_hip_ctx *ctx, double beta, double eps, const void *V, const void *G, const void *R, void *Q,
                 void *P, size_t n, hipStream_t s) {
    return G ? fields_weighted_as<T, true>(ctx, beta, eps, V, G, R, Q, P, n, s)
             : fields_weighted_as<T, false>(ctx, beta, eps, V, G, R, Q, P, n, s);
}

template <int K, typename T, bool kW>
void energy_as(double beta, double eps, const void *V, const void *G, const void *R, size_t n, double *partials,
               int grid, hipStream_t s) {
    hipLaunchKernelGGL((k_beta_energy<K, T, kW>), dim3(grid), dim3(kBlock), 0, s, (const T *)V, (const T *)G,
                       (const T *)R, n, eps, beta, partials);
}

template <typename T>
int energy_typed(double beta, double eps, const void *V, const void *G, const void *R, size_t n, double *partials,
                 int grid, hipStream_t s) {
    if (G) {
        if (beta == 0.0) energy_as<0, T, true>(beta, eps, V, G, R, n, partials, grid, s);
        else if (beta == 1.0) energy_as<1, T, true>(beta, eps, V, G, R, n, partials, grid, s);
        else if (beta == 2.0) energy_as<2, T, true>(beta, eps, V, G, R, n, partials, grid, s);
        else energy_as<3, T, true>(beta, eps, V, G, R, n, partials, grid, s);
    } else {
        if (beta == 0.0) energy_as<0, T, false>(beta, eps, V, G, R, n, partials, grid, s);
        else if (beta == 1.0) energy_as<1, T, false>(beta, eps, V, G, R, n, partials, grid, s);
        else energy_as<3, T, false>(beta, eps, V, G, R, n, partials, grid, s);
    }
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

// ---- the objective of every sample of a call (beta.h: launch_sample_objective): the tap of the H half steps and
// tnmf_hip_sample_objective.  The same assignment of elements to threads with 16-byte loads and with scalar loads, so the
// value of a sample does not depend on the path.

// one element's term.  K: 0 = Itakura-Saito, 1 = Kullback-Leibler, 2 = Frobenius, 3 = any other beta.  Unweighted K == 2
// is (V - R)^2 with the difference taken in T (k_sqdiff_partial; the 1/2 is applied to the block's sum); weighted K == 2
// is 1/2 G (V - R)^2 in double, and G <= 0 selects exactly 0 whatever V and R hold (k_beta_energy).
template <int K, typename T, bool kW>
__device__ __forceinline__ double term(T v, T g, T r, double eps, double beta) {
    if constexpr (kW) {
        double d;
        if constexpr (K == 2) {
            const double e = (double)v - (double)r;
            d = 0.5 * e * e;
        } else {
            d = divergence<K>((double)v, (double)r, eps, beta);
        }
        const double gd = (double)g;
        return gd > 0.0 ? gd * d : 0.0;
    } else if constexpr (K == 2) {
        const T d = v - r;
        return (double)d * (double)d;
    } else {
        return divergence<K>((double)v, (double)r, eps, beta);
    }
}

// block (n, b) = blockIdx.x / B, blockIdx.x % B sums elements [b * kObjChunk, min(L, (b + 1) * kObjChunk)) of sample n;
// thread t takes the vectors t, t + kBlock, ... of the block.  kVec: every vector is whole and 16-byte aligned.
template <int K, typename T, bool kVec, bool kW>
__global__ __launch_bounds__(kBlock) void k_sample_objective(const T *__restrict__ V, const T *__restrict__ G,
                                                             const T *__restrict__ R, size_t L, unsigned B, double eps,
                                                             double beta, double *__restrict__ dst) {
    using VT = typename Vec<T>::type;
    constexpr int kL = Vec<T>::n;
    constexpr int kIter = kObjChunk / (kBlock * kL);
    static_assert(kIter * kBlock * kL == kObjChunk, "a block is a whole number of passes of its threads");
    __shared__ double sh[kBlock / 64];
    const size_t n = blockIdx.x / B, b = blockIdx.x % B;
    const size_t lo = b * kObjChunk;
    const size_t len = L - lo < (size_t)kObjChunk ? L - lo : (size_t)kObjChunk;
    const T *v = V + n * L + lo, *r = R + n * L + lo, *g = kW ? G + n * L + lo : nullptr;
    double acc = 0.0;
    if constexpr (kVec) {
        VT vv[kIter], rr[kIter], gg[kIter];
#pragma unroll
        for (int k = 0; k < kIter; ++k) {   // every load of the block in flight before the first term
            const size_t i = ((size_t)k * kBlock + threadIdx.x) * kL;
            if (i < len) {
                vv[k] = *reinterpret_cast<const VT *>(v + i);
                rr[k] = *reinterpret_cast<const VT *>(r + i);
                if constexpr (kW) gg[k] = *reinterpret_cast<const VT *>(g + i);
            }
        }
#pragma unroll
        for (int k = 0; k < kIter; ++k) {
            const size_t i = ((size_t)k * kBlock + threadIdx.x) * kL;
            if (i < len) {
#pragma unroll
                for (int j = 0; j < kL; ++j)
                    acc += term<K, T, kW>(reinterpret_cast<const T *>(&vv[k])[j],
                                          kW ? reinterpret_cast<const T *>(&gg[k])[j] : T(0),
                                          reinterpret_cast<const T *>(&rr[k])[j], eps, beta);
            }
        }
    } else {
        for (int k = 0; k < kIter; ++k) {
            const size_t i = ((size_t)k * kBlock + threadIdx.x) * kL;
            for (int j = 0; j < kL; ++j)
                if (i + j < len) acc += term<K, T, kW>(v[i + j], kW ? g[i + j] : T(0), r[i + j], eps, beta);
        }
    }
    const double tot = block_sum(acc, sh);
    if (threadIdx.x == 0) dst[blockIdx.x] = (!kW && K == 2) ? 0.5 * tot : tot;
}

// out[n] = the B partials of sample n in block order; one thread per sample
__global__ __launch_bounds__(kBlock) void k_objective_finish(const double *__restrict__ partials, size_t N, unsigned B,
                                                             double *__restrict__ out) {
    const size_t n = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    double acc = 0.0;
    for (unsigned b = 0; b < B; ++b) acc += partials[n * B + b];
    out[n] = acc;
}

template <int K, typename T, bool kW>
void objective_as(bool vec, double beta, double eps, const void *V, const void *G, const void *R, size_t L, unsigned B,
                  unsigned grid, double *dst, hipStream_t s) {
    if (vec)
        hipLaunchKernelGGL((k_sample_objective<K, T, true, kW>), dim3(grid), dim3(kBlock), 0, s, (const T *)V,
                           (const T *)G, (const T *)R, L, B, eps, beta, dst);
    else
        hipLaunchKernelGGL((k_sample_objective<K, T, false, kW>), dim3(grid), dim3(kBlock), 0, s, (const T *)V,
                           (const T *)G, (const T *)R, L, B, eps, beta, dst);
}

template <typename T, bool kW>
void objective_typed(bool vec, double beta, double eps, const void *V, const void *G, const void *R, size_t L,
                     unsigned B, unsigned grid, double *dst, hipStream_t s) {
    if (beta == 0.0) objective_as<0, T, kW>(vec, beta, eps, V, G, R, L, B, grid, dst, s);
    else if (beta == 1.0) objective_as<1, T, kW>(vec, beta, eps, V, G, R, L, B, grid, dst, s);
    else if (beta == 2.0) objective_as<2, T, kW>(vec, beta, eps, V, G, R, L, B, grid, dst, s);
    else objective_as<3, T, kW>(vec, beta, eps, V, G, R, L, B, grid, dst, s);
}

}  // namespace

int launch_beta_fields(const tnmf_hip_ctx *ctx, int dtype, double beta, double eps, const void *V, const void *G,
                       const void *R, void *Q, void *P, size_t n, hipStream_t s) {
    if (n == 0) return TNMF_OK;
    return with_dtype(dtype, [&](auto zero) { return fields_typed<decltype(zero)>(ctx, beta, eps, V, G, R, Q, P, n, s); });
}

int launch_beta_energy(const tnmf_hip_ctx *ctx, int dtype, double beta, double eps, const void *V, const void *G,
                       const void *R, size_t n, double *partials, double *out_dev, hipStream_t s) {
    int grid = grid_of(n, ctx);
    if (grid > kBetaPartials) grid = kBetaPartials;
    const int rc = with_dtype(
        dtype, [&](auto zero) { return energy_typed<decltype(zero)>(beta, eps, V, G, R, n, partials, grid, s); });
    if (rc != TNMF_OK) return rc;
    hipLaunchKernelGGL(k_beta_sum, dim3(1), dim3(kBlock), 0, s, partials, grid, out_dev);
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

int launch_sample_objective(int dtype, double beta, double eps, const void *V, const void *G, const void *R, size_t N,
                            size_t L, double *partials, double *out, hipStream_t s) {
    if (N == 0) return TNMF_OK;
    if (L == 0) {
        TNMF_HIP_TRY(hipMemsetAsync(out, 0, N * sizeof(double), s));
        return TNMF_OK;
    }
    const size_t B = objective_blocks(L);
    if (N * B > 0x7fffffffu) return TNMF_E_GEOM;   // (one block index per (sample, block))
    // whole, aligned vectors: 16-byte aligned bases and samples that are a whole number of vectors (kObjChunk is one)
    const bool vec = ((reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(R)) & 15) == 0 &&
                     (L * esize(dtype)) % 16 == 0;
    double *dst = B == 1 ? out : partials;
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        if (G) objective_typed<T, true>(vec, beta, eps, V, G, R, L, (unsigned)B, (unsigned)(N * B), dst, s);
        else objective_typed<T, false>(vec, beta, eps, V, G, R, L, (unsigned)B, (unsigned)(N * B), dst, s);
    });
    TNMF_LAUNCH_CHECK();
    if (B > 1) {
        hipLaunchKernelGGL(k_objective_finish, dim3((unsigned)((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, partials, N,
                           (unsigned)B, out);
        TNMF_LAUNCH_CHECK();
    }
    return TNMF_OK;
}
