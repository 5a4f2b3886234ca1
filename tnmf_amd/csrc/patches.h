// Patches: the data under each event in the image or the atom frame, and the second moments of the patches per atom
// (patches.hip; tnmf_hip_events_patches / tnmf_hip_patch_moments; include/tnmf_hip.h, "patches").
// tests/patches_dispatch.py mirrors the constants and the launch rules below.
#pragma once

#include "events.h"

#ifndef TNMF_PATCHES_BLOCKS_PER_CU
#define TNMF_PATCHES_BLOCKS_PER_CU 8   // the grid: at most this many workgroups per CU (what 256 threads allow), each wave looping over its rows
#endif

constexpr int kMomentBlock = 16;   // S is tiled in kMomentBlock x kMomentBlock blocks: the output of one MFMA
constexpr int kMomentDepth = 4;    // entries of by_atom one MFMA contracts

// whether a wave's share of the workgroup's LDS holds x_e of `taps` = C * prod(A) doubles (asked only with a fold table)
inline bool patches_stage_fits(long long taps) { return taps <= TNMF_PATCH_STAGE_MAX; }

// out[n_events, C, Ay, Ax] (DOUBLES) = the patch of every event of source TNMF_PATCH_*, folded by the table (fold_ptr, fold_src,
// fold_w) of n_fold transforms into the atom frame, or with fold_ptr == NULL in the image frame.  Every element is written,
// zeros for a row out of range.  W and strength are read for TNMF_PATCH_CLEANED only, R unless TNMF_PATCH_DATA.
int events_patches(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, int source, const void *W, const int *events,
                   const void *strength, long long n_events, const void *V, const void *R, const int *fold_ptr,
                   const int *fold_src, const double *fold_w, int n_fold, double *out, hipStream_t s);

// S[n_atoms, D, D], g[n_atoms, D], s2[n_atoms], count[n_atoms] of the rows Y[n_rows, D] with strengths h, the rows of atom m
// being by_atom[atom_start[m] .. atom_start[m + 1]); added to with accumulate != 0, written otherwise.
int patch_moments(tnmf_hip_ctx *ctx, int D, int n_atoms, const double *Y, const double *h, const int *by_atom,
                  const int *atom_start, int n_rows, int accumulate, double *S, double *g, double *s2, double *count,
                  hipStream_t s);
