// Host-side entry points of atoms.hip: what each atom explains (tnmf_hip_atom_terms; include/tnmf_hip.h, "atom terms").
#pragma once
#include "common.h"

// One workgroup of kAtomThreads threads owns one (sample, pixel tile, channel chunk): kAtomTileY x kAtomTileX pixels on two
// shift axes, 1 x kAtomTile1D on one, every thread kAtomPix adjacent pixels along x; up to kAtomChannels channels per chunk
// (C <= kAtomChannels: one chunk, H is read once).  tests/atoms_dispatch.py mirrors these.
constexpr int kAtomThreads = 256;
constexpr int kAtomPix = 4;
constexpr int kAtomTileY = 16, kAtomTileX = 64;
constexpr int kAtomTile1D = kAtomThreads * kAtomPix;
constexpr int kAtomChannels = 4;
constexpr int kAtomChunk = 64;   // atoms whose wave sums wait in LDS before they are combined and written

struct AtomPlan {
    int TY, TX;            // pixel tile
    int tiles_y, tiles_x;
    int CH, chunks;        // channels per chunk, channel chunks
    int NB, NBO;           // runs of kAtomPix taps per atom row: ceil(Ax / 4), and of the row shifted by one: ceil((Ax + 1) / 4)
    int SW, SH;            // LDS tile of H: SH = TY + Ay - 1 rows of SW = TX + kAtomPix * NBO elements
    int slots;             // partial sums per (sample, atom): tiles_y * tiles_x * chunks
};

AtomPlan atom_terms_plan(const Geo &g);
// partials: N * slots * (M / group) * 2 doubles; taps: the flipped dictionary, every row twice (plain and shifted by one), padded to NBO runs
size_t atom_terms_partial_bytes(const Geo &g, int group);
size_t atom_terms_taps_bytes(const Geo &g, int dtype);
// TNMF_E_UNSUPPORTED: the tile of H does not fit the LDS; TNMF_E_GEOM: more than 2^31 - 1 workgroups
int atom_terms_check(const Geo &g, int dtype);
// ab[(n * (M / group) + m) * 2 + {0, 1}] = (a, b); g.N > 0, group >= 1, g.M % group == 0.  Answers atom_terms_check()
// before anything is launched.
int launch_atom_terms(const tnmf_hip_ctx *ctx, const Geo &g, int dtype, int group, const void *V, const void *G,
                      const void *R, const void *W, const void *H, double *partials, void *taps, double *ab,
                      hipStream_t s);
// taps (atom_terms_taps_bytes) = the flipped copy of W[g.M, g.C, *A] that the walk of atom_walk.h reads: what
// launch_atom_terms does first, for the other kernels on that walk (sources.hip)
int launch_atom_taps(const tnmf_hip_ctx *ctx, const Geo &g, int dtype, const void *W, void *taps, hipStream_t s);
