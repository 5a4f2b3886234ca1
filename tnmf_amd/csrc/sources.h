// Host-side entry points of sources.hip: the per-source signals of a fitted model (tnmf_hip_atom_sources;
// include/tnmf_hip.h, "sources").
#pragma once
#include "atoms.h"

// work buffer of a call: [the taps of the flipped dictionary | for 'dominant' the channel sums of W | the plane order,
// M ints | the group bounds, n_sources + 2 ints]
struct SourcesWork {
    size_t taps_off, wsum_off, order_off, start_off, total;
};
SourcesWork atom_sources_work(const Geo &g, int dtype, int n_sources, int emit);

// order[M]: the planes in the order of the walk, the listed ones first, then the others ascending; start[n_sources + 2]:
// group k (a source, or last the hidden group of the unlisted planes, which may be empty) is order[start[k] .. start[k + 1]).
// Both on the device, inside the work buffer `work` laid out by atom_sources_work.  emit: TNMF_SOURCES_*.  out
// [N, n_sources, C, *D] for the three signals, label / share [N, *D] for TNMF_SOURCES_DOMINANT.  Answers
// atom_terms_check() before anything is launched.
int launch_atom_sources(const tnmf_hip_ctx *ctx, const Geo &g, int dtype, int n_sources, int emit, double eps, char *work,
                        const void *V, const void *W, const void *H, void *out, int *label, void *share, hipStream_t s);
