// Host-side entry points of beta.hip: the elementwise fields and the energy of the beta-divergence objective.
//
// The multiplicative updates of D_beta (Serizel et al. 2016) have the form of the Frobenius ones with the samples and the
// reconstruction replaced by two fields of R~ = max(R, 0) + eps:
//   Q = V * R~^(beta - 2),   P = R~^(beta - 1)
// (beta = 2: Q = V, P = R~).  Every correlation kernel of the library takes the sample operand and the reconstruction
// operand separately, so the beta step is reconstruct -> fields -> the existing correlations on (Q, P).
#pragma once
#include "common.h"

//
// The weighted objective sum G * D_beta(V | R) (G >= 0 elementwise, of V's type) multiplies both fields by G:
//   Q = G * V * R~^(beta - 2),  P = G * R~^(beta - 1)   (beta = 2: Q = G * V, P = G * R -- no clamp, no eps)
// and entries with G == 0 give Q = P = 0 by selection, whatever V and R hold there.

// beta in {0, 1, 2} runs exact arithmetic (divisions and products, no pow); beta = 1 writes P = 1 (weighted: P = G)
// without reading R for it.  G == nullptr: unweighted (beta != 2); else weighted, any finite beta.  P may alias R.
// n elements of type dtype.
int launch_beta_fields(const tnmf_hip_ctx *ctx, int dtype, double beta, double eps, const void *V, const void *G,
                       const void *R, void *Q, void *P, size_t n, hipStream_t s);
// *out_dev = D_beta(V | max(R, 0) + eps) summed in double (G == nullptr: beta != 2; else sum G * D_beta, at beta = 2
// 1/2 G (V - R)^2, with G == 0 entries adding exactly 0), deterministic: per-block partials, then one block sums them in a
// fixed order.  partials: at least kBetaPartials doubles.
constexpr int kBetaPartials = 2048;
int launch_beta_energy(const tnmf_hip_ctx *ctx, int dtype, double beta, double eps, const void *V, const void *G,
                       const void *R, size_t n, double *partials, double *out_dev, hipStream_t s);

// The objective of every sample of a call, out[n] = sum over the sample's L = C * D elements of the data term -- 1/2 (V - R)^2
// (beta == 2, G == nullptr: the element formula of launch_half_sqdiff), D_beta(V | max(R, 0) + eps) (beta != 2) or G times
// either (G != nullptr; G <= 0 selects exactly 0: launch_beta_energy's formulas).  Their sum over n is what the energy
// entry points return for the same (V, R[, G]).  A segmented two-stage reduction in double without atomics: a sample is
// cut into blocks of kObjChunk elements -- a function of L alone, never of N, so a sample's value does not depend on which
// samples share the call -- each block leaves one partial, and the partials of a sample are added in block order.
// Asynchronous on s.
constexpr int kObjChunk = 4096;   // elements of one sample per block

inline size_t objective_blocks(size_t L) { return L ? (L + kObjChunk - 1) / kObjChunk : 1; }

// V, R (and G) hold N samples of L elements of type dtype; out: N doubles on the device; partials: N * objective_blocks(L)
// doubles on the device (not touched when a sample is one block).
int launch_sample_objective(int dtype, double beta, double eps, const void *V, const void *G, const void *R, size_t N,
                            size_t L, double *partials, double *out, hipStream_t s);
