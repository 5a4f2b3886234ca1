// atoms.hip -- what each atom explains, in one pass over the activations (tnmf_hip_atom_terms).
//
// With R_m the contribution of atom m in its `group` orientations (planes m * group + t of H and W) and d = V - R:
//   a[n, m] = sum G * R_m * d        b[n, m] = sum G * R_m^2        (G = 1 without weights)
// so that 1/2 ||V - (R - R_m)||^2 - 1/2 ||V - R||^2 = a + b / 2 (weighted norms with G).
//
// One workgroup = one (sample, pixel tile, chunk of up to kAtomChannels channels).  It loads G * d and G of its pixels
// once into registers, then streams the planes of H: a plane's tile + halo goes through LDS (the next plane's is fetched
// into registers under the multiply-adds), every thread accumulates r_m of kAtomPix adjacent pixels -- one 16-byte LDS read
// feeds kAtomPix x kAtomPix multiply-adds per channel; the atom's taps are the same for every thread and come through the
// scalar cache, from a flipped copy of W (k_atom_taps) -- and after the last plane of an atom folds r * (G d) and G * r^2
// into two doubles.
//
// The walk itself -- the staging of H, the taps in two copies, the multiply-adds on pairs -- is atom_walk.h, shared with
// sources.hip.
//
// The two doubles are summed over the wave by a shuffle tree and over the waves in wave order: partial sums per (sample,
// tile, atom); k_atom_terms_finalize adds the tiles in tile order.  No atomics: the same bits every run.
#include <algorithm>

#include "atom_walk.h"

namespace {

constexpr int kStage = 10;   // tile elements per thread that the register stage holds; larger tiles: the plain loop

// With t[b] = W[plane, c, Ay-1-a, Ax-1-b] the taps of a row of the flipped atom, run j of kAtomPix elements i = 4 j + e:
//   Wf[plane, c, a, j, 0, e] = E[i] = t[i]       (i < Ax, else 0)
//   Wf[plane, c, a, j, 1, e] = O[i] = t[i - 1]   (1 <= i <= Ax, else 0)          j < NBO
// (E and O of a run side by side: one scalar load of eight words per run)
template <typename T>
__global__ __launch_bounds__(kAtomThreads) void k_atom_taps(int rows, int Ay, int Ax, int NBO, const T *__restrict__ W,
                                                            T *__restrict__ Wf) {
    const size_t total = (size_t)rows * Ay * NBO * 2 * kAtomPix;
    const int nA = Ay * Ax;
    for (size_t i = (size_t)blockIdx.x * kAtomThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kAtomThreads) {
        const int e = (int)(i % kAtomPix);
        size_t rest = i / kAtomPix;
        const int odd = (int)(rest % 2);
        rest /= 2;
        const int j = (int)(rest % NBO);
        rest /= NBO;
        const int a = (int)(rest % Ay);
        const size_t mc = rest / Ay;
        const int b = j * kAtomPix + e - odd;
        Wf[i] = (b >= 0 && b < Ax) ? W[mc * nA + (nA - 1 - (a * Ax + b))] : T(0);
    }
}

template <typename T, int CH>
__global__ __launch_bounds__(kAtomThreads) void k_atom_terms(Geo g, AtomPlan p, int group, const T *__restrict__ V,
                                                             const T *__restrict__ G, const T *__restrict__ R,
                                                             const T *__restrict__ Wf, const T *__restrict__ H,
                                                             double *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(32))) unsigned char smem_raw[];
    __shared__ double red[kAtomChunk][kAtomThreads / 64][2];
    T *Hs = reinterpret_cast<T *>(smem_raw);
    const int Mo = g.M / group;

    ATOM_TERMS_BLOCK();
    ATOM_WALK_PIXELS();

    // G * d and G of this thread's pixels, every channel of the chunk: read once, kept in registers.  Pixels outside the
    // sample, channels past the last one and entries of weight 0 (whatever V holds there) carry exact zeros.
    T gd[CH][kAtomPix], gw[CH][kAtomPix];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
#pragma unroll
        for (int px = 0; px < kAtomPix; ++px) {
            const bool in = c < nc && y < g.Dy && xb + px < g.Dx;
            T w = T(0), d = T(0);
            if (in) {
                const size_t o = (((size_t)n * g.C + c0 + c) * g.Dy + y) * g.Dx + xb + px;
                w = G ? G[o] : T(1);
                d = V[o] - R[o];
            }
            gw[c][px] = w > T(0) ? w : T(0);
            gd[c][px] = w > T(0) ? w * d : T(0);
        }
    }
    ATOM_WALK_TILE();
    const bool pre_ok = nel <= kStage * kAtomThreads;   // the tile fits the register stage (uniform)
    ATOM_WALK_FETCH();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    Pair<T> r[CH][kAtomPix];   // (r of pixel px is r[c][px].x + r[c][px].y)
    if (pre_ok) fetch(0);
    for (int plane = 0; plane < g.M; ++plane) {
        ATOM_TERMS_PLANE(plane, r);
        if (t != group - 1) continue;
        // r_m is complete: fold into the two sums, in double
        double pa = 0.0, pb = 0.0;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
#pragma unroll
            for (int px = 0; px < kAtomPix; ++px) {
                const double rv = (double)(r[c][px].x + r[c][px].y);
                pa += rv * (double)gd[c][px];
                pb += (double)gw[c][px] * (rv * rv);
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            pa += __shfl_down(pa, o, 64);
            pb += __shfl_down(pb, o, 64);
        }
        const int ml = mo % kAtomChunk;
        if (lane == 0) {
            red[ml][wave][0] = pa;
            red[ml][wave][1] = pb;
        }
        if (ml == kAtomChunk - 1 || mo == Mo - 1) {
            __syncthreads();
            if ((int)threadIdx.x <= ml) {
                double sa = 0.0, sb = 0.0;
#pragma unroll
                for (int wv = 0; wv < kAtomThreads / 64; ++wv) {   // wave order: fixed
                    sa += red[threadIdx.x][wv][0];
                    sb += red[threadIdx.x][wv][1];
                }
                double *out = partials + (((size_t)n * p.slots + slot) * Mo + (mo - ml) + threadIdx.x) * 2;
                out[0] = sa;
                out[1] = sb;
            }
            __syncthreads();
        }
    }
}

// ab[n, m] = the sum of the slots' partial sums in slot order
__global__ __launch_bounds__(kAtomThreads) void k_atom_terms_finalize(size_t rows, int slots, int Mo,
                                                                      const double *__restrict__ partials,
                                                                      double *__restrict__ ab) {
    const size_t i = (size_t)blockIdx.x * kAtomThreads + threadIdx.x;
    if (i >= rows) return;
    const size_t n = i / Mo, m = i - n * Mo;
    const double2 *in = reinterpret_cast<const double2 *>(partials) + n * slots * Mo + m;
    double sa = 0.0, sb = 0.0;
    for (int s = 0; s < slots; ++s) {
        const double2 v = in[(size_t)s * Mo];
        sa += v.x;
        sb += v.y;
    }
    ab[2 * i] = sa;
    ab[2 * i + 1] = sb;
}

template <typename T, int CH>
void launch_chunked(const Geo &g, const AtomPlan &p, int group, unsigned blocks, size_t lds, const void *V, const void *G,
                    const void *R, const void *Wf, const void *H, double *partials, hipStream_t s) {
    hipLaunchKernelGGL((k_atom_terms<T, CH>), dim3(blocks), dim3(kAtomThreads), lds, s, g, p, group, (const T *)V,
                       (const T *)G, (const T *)R, (const T *)Wf, (const T *)H, partials);
}

}  // namespace

AtomPlan atom_terms_plan(const Geo &g) {
    AtomPlan p;
    if (g.Dy == 1 && g.Ay == 1) {   // one shift axis
        p.TY = 1;
        p.TX = kAtomTile1D;
    } else {
        p.TY = kAtomTileY;
        p.TX = kAtomTileX;
    }
    p.tiles_y = cdiv(g.Dy, p.TY);
    p.tiles_x = cdiv(g.Dx, p.TX);
    p.CH = g.C < kAtomChannels ? g.C : kAtomChannels;
    p.chunks = cdiv(g.C, p.CH);
    p.NB = cdiv(g.Ax, kAtomPix);
    p.NBO = cdiv(g.Ax + 1, kAtomPix);
    p.SW = p.TX + kAtomPix * p.NBO;
    p.SH = p.TY + g.Ay - 1;
    p.slots = p.tiles_y * p.tiles_x * p.chunks;
    return p;
}

size_t atom_terms_partial_bytes(const Geo &g, int group) {
    return align_up((size_t)g.N * atom_terms_plan(g).slots * (g.M / group) * 2 * sizeof(double), 256);
}

size_t atom_terms_taps_bytes(const Geo &g, int dtype) {
    return align_up((size_t)g.M * g.C * g.Ay * 2 * atom_terms_plan(g).NBO * kAtomPix * esize(dtype), 256);
}

int atom_terms_check(const Geo &g, int dtype) {
    const AtomPlan p = atom_terms_plan(g);
    const size_t lds = (size_t)p.SH * p.SW * esize(dtype);
    if (lds > 60 * 1024) return TNMF_E_UNSUPPORTED;   // (4 KiB of the 64 hold the waves' sums)
    if ((size_t)g.N * p.slots > 0x7fffffffull) return TNMF_E_GEOM;
    return TNMF_OK;
}

int launch_atom_terms(const tnmf_hip_ctx *ctx, const Geo &g, int dtype, int group, const void *V, const void *G,
                      const void *R, const void *W, const void *H, double *partials, void *taps, double *ab,
                      hipStream_t s) {
    const int rc = atom_terms_check(g, dtype);
    if (rc != TNMF_OK) return rc;
    const AtomPlan p = atom_terms_plan(g);
    const size_t lds = (size_t)p.SH * p.SW * esize(dtype);
    const size_t blocks = (size_t)g.N * p.slots;
    const int trc = launch_atom_taps(ctx, g, dtype, W, taps, s);
    if (trc != TNMF_OK) return trc;
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        switch (p.CH) {
            case 1: launch_chunked<T, 1>(g, p, group, (unsigned)blocks, lds, V, G, R, taps, H, partials, s); break;
            case 2: launch_chunked<T, 2>(g, p, group, (unsigned)blocks, lds, V, G, R, taps, H, partials, s); break;
            case 3: launch_chunked<T, 3>(g, p, group, (unsigned)blocks, lds, V, G, R, taps, H, partials, s); break;
            default: launch_chunked<T, 4>(g, p, group, (unsigned)blocks, lds, V, G, R, taps, H, partials, s); break;
        }
    });
    TNMF_LAUNCH_CHECK();
    const size_t out_rows = (size_t)g.N * (g.M / group);
    hipLaunchKernelGGL(k_atom_terms_finalize, dim3((unsigned)((out_rows + kAtomThreads - 1) / kAtomThreads)),
                       dim3(kAtomThreads), 0, s, out_rows, p.slots, g.M / group, (const double *)partials, ab);
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

int launch_atom_taps(const tnmf_hip_ctx *ctx, const Geo &g, int dtype, const void *W, void *taps, hipStream_t s) {
    const AtomPlan p = atom_terms_plan(g);
    const int rows = g.M * g.C;
    const size_t n_taps = (size_t)rows * g.Ay * p.NBO * 2 * kAtomPix;
    const unsigned tap_blocks = (unsigned)std::min<size_t>((n_taps + kAtomThreads - 1) / kAtomThreads, (size_t)ctx->num_cu * 8);
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_atom_taps<T>, dim3(tap_blocks), dim3(kAtomThreads), 0, s, rows, g.Ay, g.Ax, p.NBO, (const T *)W,
                           (T *)taps);
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}
