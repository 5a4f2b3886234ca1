// The diagonal of the inverse of the active block of a list's Gram matrix (covariance.hip; tnmf_hip_events_inverse_diag).
#pragma once

#include "events.h"

// The largest component factored in LDS: its packed lower triangle, n (n + 1) / 2 doubles, plus the n original diagonal
// entries (the singularity bar of every pivot) must fit the 160 KB = 20 480 doubles a workgroup may ask for:
// n (n + 3) / 2 <= 20 480 holds up to n = 200 (20 300 doubles; 201 needs 20 502).
constexpr int kInverseDiagLds = TNMF_EVENTS_INVERSE_LDS;
static_assert(kInverseDiagLds * (kInverseDiagLds + 3) / 2 * 8 <= 160 * 1024, "the triangle and the diagonal fit the LDS");
static_assert((kInverseDiagLds + 1) * (kInverseDiagLds + 4) / 2 * 8 > 160 * 1024, "and one row more does not");
static_assert(kInverseDiagLds <= kEventThreads, "one thread per row of a component in LDS");

// doubles of scratch a component of n > kInverseDiagLds rows takes: a dense n x n tile and one column
inline long long events_inverse_diag_tile(long long n) { return n * n + n; }

// d[i] = (G_AA^-1)_ii for the active rows, NaN for the others; status[c] = 0, or 1 where component c is numerically
// singular (its rows get +inf).  sizes: the HOST copy of the component sizes, ascending (checked by the caller); the
// kernels read the device lists alone and skip what does not fit the path they were launched for.
int events_inverse_diag(tnmf_hip_ctx *ctx, int K, int nnz, const int *row_start, const int *col, const double *val,
                        int n_comp, const int *comp_start, const int *sizes, int n_active, const int *member,
                        const int *local, double *scratch, long long scratch_doubles, double *d, int *status,
                        hipStream_t s);
