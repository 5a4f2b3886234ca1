// atom_walk.h -- the walk over the planes of H that atoms.hip and atoms_beta.hip (what each atom explains) and sources.hip
// (the per-source signals) share: device code only, included by those three (and, for the vector aliases alone, by
// atom_gram_kernel.h).
//
// One workgroup of kAtomThreads threads owns a pixel tile of one sample and a chunk of up to CH channels.  A plane's tile +
// halo goes through LDS (the next plane's is fetched into registers under the multiply-adds), every thread accumulates the
// plane's contribution to kAtomPix adjacent pixels -- one 16-byte LDS read feeds kAtomPix x kAtomPix multiply-adds per
// channel; the atom's taps are the same for every thread and come through the scalar cache, from the flipped copy of W that
// k_atom_taps (atoms.hip) writes.
//
// The multiply-adds are written on pairs, for the packed f32 instruction: r of a pixel is kept as two sums, over the even
// and the odd elements of the thread's window X of the LDS row, and added up by the kernel when its group of planes is
// complete.  A pair of X sits in an aligned register pair only at an even offset, so the taps come in two copies:
// E[i] = t[i] for the even pixels (r[px] = sum_i X[px + i] E[i]) and O[i] = t[i - 1], O[0] = 0, for the odd ones
// (r[px] = sum_i X[px - 1 + i] O[i]).
//
// The steps are statement macros, not functions: tnmf_hip_atom_terms is pinned to its device code (tools/
// device_code_diff.py), and every function boundary tried around these lines -- a struct with inlined members, a single
// inlined function around the multiply-adds alone, the whole body of k_atom_gram as an inlined template under a thin
// __global__ wrapper -- changed the register allocation of the kernel.  Text pasted into the kernel does not: neither these
// macros nor a body that the kernel #includes (atom_gram_kernel.h).  A kernel that uses them is a template over
// <typename T, int CH> with these names in scope:
//   Geo g, AtomPlan p; const T *H, *Wf (the flipped taps); T *Hs (LDS, p.SH * p.SW elements, 32-byte aligned);
//   int n, tyi, txi (sample, tile row, tile column); int c0, nc (first channel and channels of the chunk, uniform);
//   constexpr int kStage, the kernel file's own: tile elements per thread that the register stage holds (what its
//   register budget allows; larger tiles take the plain loop).
#pragma once
#include "atoms.h"

namespace {

static_assert(kAtomPix == 4, "the multiply-adds below are written for four pixels per thread");
template <typename T>
using Quad = T __attribute__((ext_vector_type(4)));
template <typename T>
using Pair = T __attribute__((ext_vector_type(2)));
template <typename T>
using Oct = T __attribute__((ext_vector_type(8)));

}  // namespace

// 1. The thread's place: thread (tx, ty) of the tile at (y0, x0) owns the pixels (y, xb .. xb + kAtomPix - 1).
#define ATOM_WALK_PIXELS()                                              \
    const int txt = p.TX / kAtomPix;                                    \
    const int tx = (int)threadIdx.x % txt, ty = (int)threadIdx.x / txt; \
    const int y0 = tyi * p.TY, x0 = txi * p.TX;                         \
    const int y = y0 + ty, xb = x0 + tx * kAtomPix;

// 2. The rows of taps of the chunk's channels (a channel past the last one reads the last one's: the kernel multiplies its
// sums by zero or drops them) and the tile of a plane: element tid + 256 k sits at row and column (r_first, q_first) +
// k * (dr, dq).  The kernel then says whether the tile fits its stage (uniform):
//   const bool pre_ok = nel <= kStage * kAtomThreads;
#define ATOM_WALK_TILE()                                                                                         \
    size_t wrow[CH];                                                                                             \
    _Pragma("unroll") for (int c = 0; c < CH; ++c) wrow[c] = (size_t)(c < nc ? c0 + c : g.C - 1) * g.Ay * p.NBO; \
    const int nel = p.SH * p.SW;                                                                                 \
    const int dr = kAtomThreads / p.SW, dq = kAtomThreads - dr * p.SW;                                           \
    const int r_first = (int)threadIdx.x / p.SW, q_first = (int)threadIdx.x - r_first * p.SW;

// fetch(plane): the thread's elements of that plane's tile into the register stage `pre`, zeros outside H (rows of H may be
// padded: g.Hs >= g.Hx).
#define ATOM_WALK_FETCH()                                                                                              \
    T pre[kStage];                                                                                                     \
    auto fetch = [&](int plane) {                                                                                      \
        const T *h = H + ((size_t)n * g.M + plane) * g.Hy * g.Hs;                                                      \
        int rr = r_first, q = q_first;                                                                                 \
        _Pragma("unroll") for (int k = 0; k < kStage; ++k) {                                                           \
            const int hy = y0 + rr, hx = x0 + q;                                                                       \
            pre[k] = (k * kAtomThreads + (int)threadIdx.x < nel && hy < g.Hy && hx < g.Hx) ? h[(size_t)hy * g.Hs + hx] \
                                                                                            : T(0);                    \
            rr += dr;                                                                                                  \
            q += dq;                                                                                                   \
            if (q >= p.SW) {                                                                                           \
                q -= p.SW;                                                                                             \
                ++rr;                                                                                                  \
            }                                                                                                          \
        }                                                                                                              \
    };

// 3. `plane` into LDS, from the stage or, beyond it, straight from H (the first barrier: every wave is done with the
// previous plane); then, when `more`, the plane `next` into the stage: in flight under the multiply-adds.
#define ATOM_WALK_STAGE(plane, more, next)                                       \
    __syncthreads();                                                             \
    if (pre_ok) {                                                                \
        _Pragma("unroll") for (int k = 0; k < kStage; ++k) {                     \
            const int i = k * kAtomThreads + threadIdx.x;                        \
            if (i < nel) Hs[i] = pre[k];                                         \
        }                                                                        \
    } else {                                                                     \
        const T *h = H + ((size_t)n * g.M + plane) * g.Hy * g.Hs;                \
        for (int i = threadIdx.x; i < nel; i += kAtomThreads) {                  \
            const int rr = i / p.SW, q = i - rr * p.SW;                          \
            const int hy = y0 + rr, hx = x0 + q;                                 \
            Hs[i] = (hy < g.Hy && hx < g.Hx) ? h[(size_t)hy * g.Hs + hx] : T(0); \
        }                                                                        \
    }                                                                            \
    __syncthreads();                                                             \
    if (pre_ok && more) fetch(next);

// 4. r[CH][kAtomPix] (Pair<T>) += what the plane in LDS adds to the thread's pixels, every channel of the chunk.  The taps
// of a run are the same address in every thread; the next run's are loaded under this run's multiply-adds.  E is one run
// shorter than O when Ax is a multiple of kAtomPix (j < p.NB).  X[4j .. 4j + 5] = (x0, x1, x2).
#define ATOM_WALK_MACS(plane, r)                                                                  \
    const Oct<T> *wq = reinterpret_cast<const Oct<T> *>(Wf) + (size_t)plane * g.C * g.Ay * p.NBO; \
    for (int a = 0; a < g.Ay; ++a) {                                                              \
        const Quad<T> *row = reinterpret_cast<const Quad<T> *>(Hs + (ty + a) * p.SW) + tx;        \
        const Oct<T> *taps[CH];                                                                   \
        Oct<T> eo_next[CH];                                                                       \
        _Pragma("unroll") for (int c = 0; c < CH; ++c) {                                          \
            taps[c] = wq + wrow[c] + (size_t)a * p.NBO;                                           \
            eo_next[c] = taps[c][0];                                                              \
        }                                                                                         \
        Quad<T> cur = row[0];                                                                     \
        _Pragma("unroll 2") for (int j = 0; j < p.NBO; ++j) {                                     \
            const Quad<T> nxt = row[j + 1];                                                       \
            const Pair<T> x0 = cur.xy, x1 = cur.zw, x2 = nxt.xy;                                  \
            const int jn = j + 1 < p.NBO ? j + 1 : j;                                             \
            _Pragma("unroll") for (int c = 0; c < CH; ++c) {                                      \
                const Oct<T> eo = eo_next[c];                                                     \
                eo_next[c] = taps[c][jn];                                                         \
                const Quad<T> e = eo.lo, o = eo.hi;                                               \
                r[c][1] += x0 * o.xy;                                                             \
                r[c][1] += x1 * o.zw;                                                             \
                r[c][3] += x1 * o.xy;                                                             \
                r[c][3] += x2 * o.zw;                                                             \
                if (j < p.NB) {                                                                   \
                    r[c][0] += x0 * e.xy;                                                         \
                    r[c][0] += x1 * e.zw;                                                         \
                    r[c][2] += x1 * e.xy;                                                         \
                    r[c][2] += x2 * e.zw;                                                         \
                }                                                                                 \
            }                                                                                     \
            cur = nxt;                                                                            \
        }                                                                                         \
    }

// ---- The two steps that only the terms kernels take (atoms.hip, atoms_beta.hip) ----
//
// 0. The workgroup's place, before step 1: sample n, tile (tyi, txi) and channel chunk from blockIdx.x; `slot` numbers the
// partial sums of a (sample, atom).
#define ATOM_TERMS_BLOCK()                                       \
    unsigned bid = blockIdx.x;                                   \
    const int chunk = bid % p.chunks;                            \
    bid /= p.chunks;                                             \
    const int txi = bid % p.tiles_x;                             \
    bid /= p.tiles_x;                                            \
    const int tyi = bid % p.tiles_y;                             \
    const int n = bid / p.tiles_y;                               \
    const int slot = (tyi * p.tiles_x + txi) * p.chunks + chunk; \
    const int c0 = chunk * CH;                                   \
    const int nc = g.C - c0 < CH ? g.C - c0 : CH;

// 5. Inside the loop over the planes, after `if (pre_ok) fetch(0);`: plane = orientation t of atom mo; r starts from zero at
// an atom's first plane; steps 3 and 4.  After its last plane (t == group - 1) the kernel folds r_m into its sums.  Needs
// int group (planes per atom) besides the names above.
#define ATOM_TERMS_PLANE(plane, r)                                                            \
    const int mo = plane / group, t = plane - mo * group;                                     \
    if (t == 0) {                                                                             \
        _Pragma("unroll") for (int c = 0; c < CH; ++c)                                        \
            _Pragma("unroll") for (int px = 0; px < kAtomPix; ++px) r[c][px] = Pair<T>(T(0)); \
    }                                                                                         \
    ATOM_WALK_STAGE(plane, plane + 1 < g.M, plane + 1);                                       \
    ATOM_WALK_MACS(plane, r);

// The reduction of those sums -- a shuffle tree over the wave, the waves' sums through LDS, added in wave order and written
// every kAtomChunk (kBetaChunk) atoms -- is written out in both kernels, on named doubles.  Written once on double ps[NS]
// it reproduces the device code of k_atom_terms (NS = 2) but not of k_atom_terms_beta (NS = 3): the shuffle tree on an
// array element changes the register allocation of 3 to 24 of its 24 instances, in either loop order, with and without
// an unroll pragma.  Do not retry without a new idea.
