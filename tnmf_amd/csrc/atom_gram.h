// Host-side entry points of atom_gram.hip: how atoms overlap (tnmf_hip_atom_gram; include/tnmf_hip.h, "atom Gram").
#pragma once
#include "atoms.h"

// One workgroup of kAtomThreads threads (twice as many where two halves fit) owns one (sample, strip of kGramStripTiles
// pixel tiles, pair of atom blocks).  The pixel tile and the multiply-adds are those of atoms.h, one channel per pass; r of
// up to `cap` atoms (two blocks of cap / 2) of the tile waits in LDS, rows of kGramStride elements, for the contraction on
// the matrix cores.
// tests/atom_gram_dispatch.py mirrors these.
constexpr int kGramTilePix = kAtomThreads * kAtomPix;   // pixels of a tile: 16 x 64 or 1 x 1024
constexpr int kGramStride = kGramTilePix + 16;          // (16 lanes of an MFMA operand read: 16 elements apart in the banks)
constexpr int kGramStripTiles = 16;                     // tiles whose sums stay in one workgroup's accumulators
constexpr size_t kGramLds = 160 * 1024;                 // LDS of a CU

struct GramPlan {
    AtomPlan ap;           // tile, halo and tap runs (its CH and chunks are not used: one channel per pass)
    int cap, hb;           // atoms staged per workgroup (16 or 32; 0: nothing fits) and atoms per block: cap / 2
    int halves;            // halves of 256 threads that build different atoms at the same time: 2 with 32 rows where it fits
    int h_elems;           // elements of a half's tile of H (rounded up to 32 bytes)
    int nbk, pairs;        // atom blocks (at least 2: the second may be empty) and pairs I < J of them
    int tiles, strips;     // pixel tiles per sample, strips of kGramStripTiles of them
    size_t red_off, lds;   // LDS: [r: cap rows | G of the tile | tile of H + halo per half | the waves' sums of a], bytes
    size_t wg_doubles;     // partial sums per workgroup: cap * cap of B, cap of a
};

GramPlan atom_gram_plan(const Geo &g, int dtype, int group);
// partial sums: N * strips * pairs * (cap * cap + cap) doubles; the taps are those of atom_terms_taps_bytes()
size_t atom_gram_partial_bytes(const Geo &g, int dtype, int group);
// TNMF_E_UNSUPPORTED: 16 atoms of a tile and the tile of H do not fit the LDS; TNMF_E_GEOM: more than 2^31 - 1 workgroups
int atom_gram_check(const Geo &g, int dtype, int group);
// a[n * Mo + m], B[(n * Mo + m) * Mo + m'] with Mo = M / group; g.N > 0, group >= 1, g.M % group == 0.  Answers
// atom_gram_check() before anything is launched.
int launch_atom_gram(const tnmf_hip_ctx *ctx, const Geo &g, int dtype, int group, const void *V, const void *G,
                     const void *R, const void *W, const void *H, double *partials, void *taps, double *a, double *B,
                     hipStream_t s);
// a and B from the partial sums that a kernel on the plan p has written (what launch_atom_gram does last; atom_gram_beta.hip)
int launch_atom_gram_finalize(const Geo &g, const GramPlan &p, int group, const double *partials, double *a, double *B,
                              hipStream_t s);
