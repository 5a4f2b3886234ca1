// modes.h -- the reconstruction modes, per shift axis: the one statement of the rule that the pad / fold kernels (generic.hip,
// inhibit.hip, volume.hip), the occurrence walk (event_walk.h) and the entries of api.hip follow.  Reference:
// backends/_PyTorchBackend.py:42-52 (the pad), backends/_Backend.py:60-73 (the shift shape).
//
// An axis has D samples and an atom of a taps.  The S activations of a mode are padded by l = a - 1 in front ('full': and
// behind) to the padded length D + a - 1 -- always that -- and the padded row goes through the 'valid' kernels:
//
//   mode       S            padded position j copies activation ...         activation u is also copied to ...
//   valid      D + a - 1    (no pad: the activations are the padded row)
//   full       D - a + 1    j - l where that is in [0, S), else a zero       nowhere
//   circular   D            j - l; in the pad S - l + j (wrapped)            u - (S - l)   where u >= S - l
//   reflect    D            j - l; in the pad l - j (mirrored, no edge)      l - u         where 1 <= u <= l
//
// 'circular' wraps at most once: l <= S.  'reflect' does not repeat the edge: l < S (at l == S the mirror would read one
// element past the activation row).  torch's pad raises in both cases; 'full' pads zeros and has no limit.
// Host + device, nothing beyond include/tnmf_hip.h: tests/native/modes_check.cpp runs these functions on the CPU.
#pragma once

#include "tnmf_hip.h"

#ifndef TNMF_HD
#if defined(__HIPCC__)
#define TNMF_HD __host__ __device__ __forceinline__
#else
#define TNMF_HD inline
#endif
#endif

TNMF_HD bool mode_known(int mode) { return mode >= TNMF_MODE_VALID && mode <= TNMF_MODE_REFLECT; }

// activation length of an axis of D samples and a taps
TNMF_HD int mode_shift_len(int mode, int D, int a) {
    return mode == TNMF_MODE_VALID ? D + a - 1 : (mode == TNMF_MODE_FULL ? D - a + 1 : D);
}

// an axis of S activations and a taps exists in this mode (callers answer TNMF_E_GEOM where it does not)
TNMF_HD bool mode_axis_ok(int mode, int S, int a) {
    return S >= 1 && (mode != TNMF_MODE_CIRCULAR || a - 1 <= S) && (mode != TNMF_MODE_REFLECT || a - 1 < S);
}

// activation index copied to padded position j (-1: a zero); a padded mode
TNMF_HD int pad_src(int j, int S, int a, int mode) {
    const int l = a - 1;
    if (mode == TNMF_MODE_FULL) {
        const int u = j - l;
        return (u >= 0 && u < S) ? u : -1;
    }
    if (j >= l) return j - l;
    return mode == TNMF_MODE_CIRCULAR ? S - l + j : l - j;
}

// second padded position (besides u + a - 1) that copies activation u, or -1
TNMF_HD int pad_dup(int u, int S, int a, int mode) {
    const int l = a - 1;
    if (mode == TNMF_MODE_CIRCULAR) return u >= S - l ? u - (S - l) : -1;
    if (mode == TNMF_MODE_REFLECT) return (u >= 1 && u <= l) ? l - u : -1;
    return -1;
}

// the images of the shift u: their padded positions q, at most two ('valid': the shift itself).  The second is pad_dup written
// out (through its -1 the kernels that walk occurrences change: a compare more per axis); modes_check.cpp ties the two
TNMF_HD int axis_images(int mode, int u, int a, int S, int q[2]) {
    if (mode == TNMF_MODE_VALID) {
        q[0] = u;
        return 1;
    }
    q[0] = u + a - 1;
    if (mode == TNMF_MODE_CIRCULAR && u >= S - (a - 1)) {
        q[1] = u - (S - (a - 1));
        return 2;
    }
    if (mode == TNMF_MODE_REFLECT && u >= 1 && u <= a - 1) {
        q[1] = (a - 1) - u;
        return 2;
    }
    return 1;
}

// the shift u is in range and its occurrence is one image wholly inside the D samples
TNMF_HD bool axis_whole(int mode, int u, int a, int S, int D) {
    if ((unsigned)u >= (unsigned)S) return false;
    int q[2];
    if (axis_images(mode, u, a, S, q) != 1) return false;
    const int o = q[0] - (a - 1);
    return o >= 0 && o + a <= D;
}
