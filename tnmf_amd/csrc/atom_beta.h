// atom_beta.h -- the atom terms and the atom Gram under the beta-divergence objectives (tnmf_hip_atom_terms_beta,
// tnmf_hip_atom_gram_beta; include/tnmf_hip.h, "atom terms, beta").  Host-side entry points of atoms_beta.hip and
// atom_gram_beta.hip, and the per-pixel arithmetic the two kernels share (device code, in double).
#pragma once
#include "atom_gram.h"

// partials: N * slots * (M / group) * 3 doubles (a, b, gain); the taps are those of atom_terms_taps_bytes()
size_t atom_terms_beta_partial_bytes(const Geo &g, int group);
// abg[(n * (M / group) + m) * 3 + {0, 1, 2}] = (a, b, gain); beta finite and not 2, eps >= 0; otherwise as
// launch_atom_terms, whose checks (atom_terms_check) it answers before anything is launched
int launch_atom_terms_beta(const tnmf_hip_ctx *ctx, const Geo &g, int dtype, int group, double beta, double eps,
                           const void *V, const void *G, const void *R, const void *W, const void *H, double *partials,
                           void *taps, double *abg, hipStream_t s);
// abg[3 i + {0, 1, 2}] = (ab[2 i], ab[2 i + 1], ab[2 i] + ab[2 i + 1] / 2), i < rows: the Frobenius terms in the layout above
int launch_atom_terms_widen(const double *ab, size_t rows, double *abg, hipStream_t s);
// a, B as launch_atom_gram (same plan, same partial sums, same finalize), the pixel factors those of the beta-divergence
int launch_atom_gram_beta(const tnmf_hip_ctx *ctx, const Geo &g, int dtype, int group, double beta, double eps,
                          const void *V, const void *G, const void *R, const void *W, const void *H, double *partials,
                          void *taps, double *a, double *B, hipStream_t s);

// The context's side of the two entry points (api.hip, which alone lays out the buffers of a context): the geometry of a
// call -- TNMF_E_UNSUPPORTED for three shift axes, else the checks of every entry -- and its buffers: the work buffer of
// tnmf_hip_atom_terms grown to work_bytes (*work), and, where *R is NULL, the reconstruction by the context's kernel
// family in the context's scratch (*R).
int atom_entry_geo(const tnmf_hip_geom *geom, Geo *g);
int atom_entry_buffers(tnmf_hip_ctx *ctx, const Geo &g, int dtype, size_t work_bytes, const void *W, const void *H,
                       const void **R, void **work, hipStream_t s);

#ifdef __HIPCC__
namespace {

// K of beta.hip: 0 = Itakura-Saito (beta 0), 1 = Kullback-Leibler (beta 1), 3 = any other beta (pow); 2 has kernels of its own
constexpr int beta_kind(double beta) { return beta == 0.0 ? 0 : beta == 1.0 ? 1 : 3; }

// The two pixel factors of an entry of weight g > 0, x = max(R, 0) + eps:
//   gd = g (v x^(beta-2) - x^(beta-1))        gw = g c,   c = (beta-1) x^(beta-2) + (2-beta) v x^(beta-3)
// (Q - P of beta.h, and the curvature of D_beta(v | x) in x: signed outside 1 <= beta <= 2), evaluated as
// (v - x) x^(beta-2) and ((beta-1) x + (2-beta) v) x^(beta-3): one difference, not two powers' difference.  No pow for
// beta 0 and 1.
template <int K>
__device__ __forceinline__ void beta_pixel(double v, double R, double g, double eps, double beta, double &gd, double &gw) {
    const double x = (R > 0.0 ? R : 0.0) + eps;
    if constexpr (K == 0) {
        const double inv = 1.0 / x;
        gd = g * ((v - x) * (inv * inv));
        gw = g * ((2.0 * v - x) * (inv * inv * inv));
    } else if constexpr (K == 1) {
        gd = g * ((v - x) / x);
        gw = g * (v / (x * x));
    } else {
        const double p3 = pow(x, beta - 3.0);
        gd = g * ((v - x) * (p3 * x));
        gw = g * (((beta - 1.0) * x + (2.0 - beta) * v) * p3);
    }
}

// D_beta(v | x_m) - D_beta(v | x) with x = max(R, 0) + eps and x_m = max(R - r, 0) + eps: what the pixel's divergence rises
// by when r is taken out of R.  Written on dx = x - x_m (the difference of the two clamped values: eps drops out, and
// where neither clamp acts it is r itself) and
// L = log(x_m / x) = -log1p(dx / x_m), so that nothing cancels where r is small beside R:
//   beta 1:  v log(x / x_m) + (x_m - x)                            (x_m - x where v == 0: 0 log 0 = 0)
//   beta 0:  v (1 / x_m - 1 / x) + log(x_m / x)
//   else:    [(beta-1) (x_m^beta - x^beta) - beta v (x_m^(beta-1) - x^(beta-1))] / (beta (beta-1)),
//            x_m^p - x^p = x^p expm1(p L)
template <int K>
__device__ __forceinline__ double beta_gain(double v, double R, double r, double eps, double beta) {
    const double c0 = R > 0.0 ? R : 0.0, rm = R - r, c1 = rm > 0.0 ? rm : 0.0;
    // (dx from r itself where neither clamp acts: the rounding of R - r is of the size of R, not of r)
    const double x = c0 + eps, xm = c1 + eps, dx = rm > 0.0 ? (R > 0.0 ? r : -rm) : c0;
    const double l1p = log1p(dx / xm);   // log(x / x_m)
    if constexpr (K == 0) {
        return v * (dx / (x * xm)) - l1p;
    } else if constexpr (K == 1) {
        return (v > 0.0 ? v * l1p : 0.0) - dx;
    } else {
        const double p1 = pow(x, beta - 1.0);
        return ((beta - 1.0) * (p1 * x) * expm1(-beta * l1p) - beta * v * p1 * expm1((1.0 - beta) * l1p)) /
               (beta * (beta - 1.0));
    }
}

}  // namespace
#endif
