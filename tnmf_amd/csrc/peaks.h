// Detections: thresholded, non-maximum-suppressed peaks of the activations (peaks.hip; tnmf_hip_find_peaks).
#pragma once

#include "common.h"

// H viewed as `planes` planes of Sz * Sy rows of Sx entries, row stride Hs: row ((n * P + p) * Sz + z) * Sy + y.  One and
// two shift axes run as Sz = 1 (and Sy = 1).
struct PeakGeo {
    long long planes; // N * P
    int P;            // planes (effective atoms) per sample
    int Sz, Sy, Sx;   // shift shape
    int Hs;           // row stride in elements (>= Sx)
    int rz, ry, rx;   // suppression radius per axis, clipped to the plane extent - 1
    int group;        // consecutive planes that compete (divides P)
};

// Appends (flat C-order index in [N, P, *S], value) of every detection to idx / val while slot < capacity; *count (zeroed
// on the stream first) ends as the number of detections, whatever the capacity.
int peaks_find(tnmf_hip_ctx *ctx, const PeakGeo &g, int dtype, const void *H, double threshold, long long *idx,
               void *val, size_t capacity, unsigned long long *count, hipStream_t s);
