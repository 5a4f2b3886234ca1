// Exact strengths of a list of events (solve.hip; tnmf_hip_events_pairs / _gram / _project / _nnls).
#pragma once

#include "events.h"

// pairs[slot] = i * n_events + j for the candidate row pairs i < j of one sample with an image pair closer than the atom
// extent on every axis, in no particular order, duplicates included, while slot < capacity; *count (zeroed on the stream)
// counts every one.  images / cell_start: the list of events_render; events: the rows (n, p, uy, ux).
int events_pairs(tnmf_hip_ctx *ctx, const EventGeo &g, const int *images, long long n_images, const int *cell_start,
                 const int *events, long long n_events, long long *pairs, size_t capacity, unsigned long long *count,
                 hipStream_t s);

// val[p] = <phi_i, phi_j> for the pair (row_i[p], row_j[p]), in double; 0 for a row outside the contract and for rows of two
// samples.  Every element is written.
int events_gram(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const void *W, const int *events, long long n_events,
                const int *row_i, const int *row_j, long long n_pairs, double *val, hipStream_t s);

// c[e] = <phi_e, V>, in double; 0 for a row outside the contract.  Every element is written.
int events_project(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const void *W, const int *events, long long n_events,
                   const void *V, double *c, hipStream_t s);

// min 1/2 h'Gh - c'h over h >= 0 on a CSR matrix, from the start h projected; synchronises the stream at every check.
// workspace: events_nnls_workspace(K) doubles on the device; iterations, kkt_out, converged, history, n_history on the host.
long long events_nnls_workspace(long long n_rows);
int events_nnls(tnmf_hip_ctx *ctx, int K, int nnz, const int *row_start, const int *col, const double *val, const double *c,
                double *h, double tol, int max_iterations, int check_every, double *workspace, int *iterations,
                double *kkt_out, int *converged, double *history, int history_capacity, int *n_history, hipStream_t s);
