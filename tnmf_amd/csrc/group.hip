// group.hip -- rotation and mirror invariance (include/tnmf_hip.h, "transform groups"): the dictionary W of M atoms stands
// for M * T effective atoms W_eff[m * T + t] = T_t(W[m]), every T_t a permutation of the atom's pixels (a mirror, a
// rotation by a multiple of 90 degrees, or one followed by the other).  The H half step, the reconstruction and the energy
// run unchanged on W_eff; the W half step folds the gradient of W_eff back onto W with the adjoint of the expansion.
//
// Every T_t is coded as three bits: out[y][x] = in[sy][sx] with (u, v) = SWAP ? (x, y) : (y, x),
// sy = FLIP_Y ? Ay-1-u : u, sx = FLIP_X ? Ax-1-v : v.  SWAP (a transpose) needs square atoms.  The tables below list,
// in the order t of the public interface, the codes of numpy's
//   flip      a, a[..., ::-1]
//   mirrors   a, a[:, ::-1], a[::-1, :], a[::-1, ::-1]
//   rot90     np.rot90(a, k), k = 0..3
//   dihedral  np.rot90(a, k), k = 0..3, then np.rot90(a[:, ::-1], k), k = 0..3
//
// The buffers are tiny (M * T * C * Ay * Ax elements): these kernels are a few microseconds of dependent launches, so they
// are written for a short chain, not for bandwidth.
#include <algorithm>

#include "common.h"
#include "fft.h"
#include "rowsum.h"

namespace {

constexpr int kBlock = 256;   // (the workgroup of apply_normalize_row: the fused update reduces rows in the same order)
constexpr int kFX = 1, kFY = 2, kSW = 4;
constexpr int kMaxT = 8;

struct Group {
    int T;
    int code[kMaxT];
};

// TNMF_GROUP_* -> codes; false for an unknown id
bool group_of(int id, Group *out) {
    static const Group tables[] = {
        {2, {0, kFX}},
        {4, {0, kFX, kFY, kFY | kFX}},
        {4, {0, kSW | kFX, kFY | kFX, kSW | kFY}},
        {8, {0, kSW | kFX, kFY | kFX, kSW | kFY, kFX, kSW, kFY, kSW | kFY | kFX}},
    };
    if (id < 0 || id >= (int)(sizeof(tables) / sizeof(tables[0]))) return false;
    *out = tables[id];
    return true;
}

// dictionary geometry of a group call: M atoms of C channels, atom Ay x Ax (1-D: Ay = 1); the sample shape is not used
struct Dict {
    int M, C, Ay, Ax;
};

int to_dict(const tnmf_hip_geom *in, int group, Dict *d, Group *grp) {
    if (!in) return TNMF_E_NULL;
    if (in->dtype != 0 && in->dtype != 1) return TNMF_E_DTYPE;
    if (in->ndim == 3) return TNMF_E_UNSUPPORTED;   // (no transforms for volumes)
    if (in->ndim != 1 && in->ndim != 2) return TNMF_E_GEOM;
    d->M = in->M;
    d->C = in->C;
    d->Ay = in->ndim == 1 ? 1 : in->A[0];
    d->Ax = in->ndim == 1 ? in->A[0] : in->A[1];
    if (d->M <= 0 || d->C <= 0 || d->Ay <= 0 || d->Ax <= 0) return TNMF_E_GEOM;
    if (!group_of(group, grp)) return TNMF_E_UNSUPPORTED;
    if (in->ndim == 1 && group != TNMF_GROUP_FLIP) return TNMF_E_UNSUPPORTED;   // (one axis: only its mirror)
    bool swaps = false;
    for (int t = 0; t < grp->T; ++t) swaps |= (grp->code[t] & kSW) != 0;
    if (swaps && d->Ay != d->Ax) return TNMF_E_UNSUPPORTED;                     // (a transpose needs square atoms)
    // (every index below is an int: refuse what would not fit)
    if ((long long)d->M * grp->T * d->C * d->Ay * d->Ax >= (1LL << 31)) return TNMF_E_GEOM;
    return TNMF_OK;
}

// pixel of the atom read by T_code at pixel (y, x) of the transformed atom
__device__ __forceinline__ int src_pixel(int code, int y, int x, int Ay, int Ax) {
    const int u = (code & kSW) ? x : y, v = (code & kSW) ? y : x;
    const int sy = (code & kFY) ? Ay - 1 - u : u, sx = (code & kFX) ? Ax - 1 - v : v;
    return sy * Ax + sx;
}

// pixel of the transformed atom that T_code fills from pixel (py, px) of the atom (the inverse permutation)
__device__ __forceinline__ int dst_pixel(int code, int py, int px, int Ay, int Ax) {
    const int u = (code & kFY) ? Ay - 1 - py : py, v = (code & kFX) ? Ax - 1 - px : px;
    return (code & kSW) ? v * Ax + u : u * Ax + v;
}

// W_eff[(m*T + t)*C + c][q] = W[m*C + c][src_t(q)]: one thread per element of W_eff (a gather; the writes are coalesced)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_group_expand(Group grp, Dict d, const T *__restrict__ W,
                                                         T *__restrict__ W_eff) {
    const int nA = d.Ay * d.Ax, total = d.M * grp.T * d.C * nA;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < total; i += gridDim.x * kBlock) {
        const int q = i % nA, row = i / nA;             // row = (m*T + t)*C + c
        const int c = row % d.C, mt = row / d.C;
        const int t = mt % grp.T, m = mt / grp.T;
        W_eff[i] = W[(m * d.C + c) * nA + src_pixel(grp.code[t], q / d.Ax, q % d.Ax, d.Ay, d.Ax)];
    }
}

// sum over t of X[(m*T + t)*C + c][dst_t(p)], ascending t, in double: the adjoint of the expansion at pixel p of row (m, c)
template <typename T>
__device__ __forceinline__ double fold_at(const Group &grp, const Dict &d, const T *__restrict__ X, int m, int c, int p) {
    const int nA = d.Ay * d.Ax, py = p / d.Ax, px = p % d.Ax;
    double s = 0.0;
    for (int t = 0; t < grp.T; ++t)
        s += (double)X[((m * grp.T + t) * d.C + c) * nA + dst_pixel(grp.code[t], py, px, d.Ay, d.Ax)];
    return s;
}

// [neg | pos] of W_eff ([2][M*T][C][nA]) -> [neg | pos] of W ([2][M][C][nA]), every element rounded once
template <typename T>
__global__ __launch_bounds__(kBlock) void k_group_fold(Group grp, Dict d, const T *__restrict__ negpos_eff,
                                                       T *__restrict__ negpos) {
    const int nA = d.Ay * d.Ax, half = d.M * d.C * nA, half_eff = half * grp.T;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < 2 * half; i += gridDim.x * kBlock) {
        const int h = i / half, e = i % half;
        const int p = e % nA, row = e / nA;
        negpos[i] = (T)fold_at(grp, d, negpos_eff + (size_t)h * half_eff, row / d.C, row % d.C, p);
    }
}

// The single-rank W step after the gradient of W_eff, in one launch: fold, W = W * neg / (pos + eps), W /= its sum over
// the atom axes (the arithmetic and the reduction order of apply_normalize_row), then the new row into its T places of
// W_eff.  One workgroup per (m, c) row.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_group_apply(Group grp, Dict d, T *__restrict__ W, T *__restrict__ W_eff,
                                                        const T *__restrict__ negpos_eff, T eps) {
    __shared__ double sh[kBlock / 64];
    const int nA = d.Ay * d.Ax, half_eff = d.M * grp.T * d.C * nA;
    const int row = blockIdx.x, m = row / d.C, c = row % d.C;
    const size_t base = (size_t)row * nA;
    double part = 0.0;
    for (int i = threadIdx.x; i < nA; i += kBlock) {
        const T neg = (T)fold_at(grp, d, negpos_eff, m, c, i);
        const T p = (T)fold_at(grp, d, negpos_eff + half_eff, m, c, i) + eps;
        const T w = (W[base + i] * neg) / p;
        W[base + i] = w;
        part += (double)w;
    }
    const T tot = (T)block_sum<T>(part, sh);
    for (int i = threadIdx.x; i < nA; i += kBlock) {
        const T w = W[base + i] / tot;
        W[base + i] = w;
        const int py = i / d.Ax, px = i % d.Ax;
        for (int t = 0; t < grp.T; ++t)
            W_eff[((m * grp.T + t) * d.C + c) * nA + dst_pixel(grp.code[t], py, px, d.Ay, d.Ax)] = w;
    }
}

#define CHECK_RC(rc_expr)               \
    do {                                \
        const int _rc = (rc_expr);      \
        if (_rc != TNMF_OK) return _rc; \
    } while (0)

int grid_of(int n) { return n <= 0 ? 1 : std::min(cdiv(n, kBlock), 1024); }

}  // namespace

extern "C" {

int tnmf_hip_group_expand_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int group, const void *W, void *W_eff,
                            void *stream) {
    if (!ctx) return TNMF_E_NULL;
    Dict d;
    Group grp;
    CHECK_RC(to_dict(geom, group, &d, &grp));
    if (!W || !W_eff) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    fft_invalidate_W(ctx);   // (W_eff: a fixed address with new contents -- its cached spectra are stale)
    const int n = d.M * grp.T * d.C * d.Ay * d.Ax;
    with_dtype(geom->dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_group_expand<T>, dim3(grid_of(n)), dim3(kBlock), 0, s, grp, d, (const T *)W, (T *)W_eff);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

int tnmf_hip_group_fold_grad_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int group, const void *negpos_eff,
                               void *negpos, void *stream) {
    if (!ctx) return TNMF_E_NULL;
    Dict d;
    Group grp;
    CHECK_RC(to_dict(geom, group, &d, &grp));
    if (!negpos_eff || !negpos) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n = 2 * d.M * d.C * d.Ay * d.Ax;
    with_dtype(geom->dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_group_fold<T>, dim3(grid_of(n)), dim3(kBlock), 0, s, grp, d, (const T *)negpos_eff,
                           (T *)negpos);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

int tnmf_hip_group_apply_W(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int group, void *W_inout, void *W_eff_out,
                           const void *negpos_eff, double eps, void *stream) {
    if (!ctx) return TNMF_E_NULL;
    Dict d;
    Group grp;
    CHECK_RC(to_dict(geom, group, &d, &grp));
    if (!W_inout || !W_eff_out || !negpos_eff) return TNMF_E_NULL;
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    fft_invalidate_W(ctx);
    const int rows = d.M * d.C;
    with_dtype(geom->dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_group_apply<T>, dim3(rows), dim3(kBlock), 0, s, grp, d, (T *)W_inout, (T *)W_eff_out,
                           (const T *)negpos_eff, (T)eps);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

}  // extern "C"
