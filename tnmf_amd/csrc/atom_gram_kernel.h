// atom_gram_kernel.h -- the text of the atom Gram kernel, once, for atom_gram.hip (k_atom_gram) and atom_gram_beta.hip
// (k_atom_gram_beta): device code only.
//
// Included at file scope it gives what the two files share by name: the vector aliases (atom_walk.h), kStage, kWaves, Acc
// and pair_blocks.  Included again with ATOM_GRAM_KERNEL_BODY defined, between a kernel's signature and its closing brace,
// it gives the kernel's body: the pair and strip decode, the two halves, the register stage, the multiply-adds on pairs,
// the parking of r_m, the contraction on the matrix cores and the write-out in wave order (atom_gram.hip describes them).
// Shared as text, not through a function: the kernels are pinned to their device code (tools/device_code_diff.py), and a
// body moved into an inlined function template changed the register allocation of every instance (atom_walk.h).
//
// The kernel that includes the body is a template over <typename T, int NBLK, int HALVES, ...> (NBLK = cap / 16) with
// these names in scope:
//   Geo g, GramPlan p, int group; const T *V, *G, *R, *Wf (the flipped taps), *H; double *partials;
//   ATOM_GRAM_PIXEL(in, offset), the including file's own: a statement that sets gd[px] (what r_m is folded with into a)
//   and gw[px] (the weight of the contraction) of the pixel at `offset` of V, G and R -- exact zeros unless `in`, which
//   says that the pixel is inside the sample; `offset` is evaluated only then.
// The multiply-adds are not ATOM_WALK_MACS: one channel, the half's own tid and Hs.
#ifndef ATOM_GRAM_KERNEL_BODY
#ifndef ATOM_GRAM_KERNEL_H   // (no #pragma once: the file is included twice)
#define ATOM_GRAM_KERNEL_H
#include "atom_gram.h"
#include "atom_walk.h"

namespace {

constexpr int kStage = 10;   // tile elements per thread that the register stage holds; larger tiles: the plain loop
constexpr int kWaves = kAtomThreads / 64;   // waves of a half
using Acc = Quad<double>;

// the pair (I, J), I < J < nbk, of index `pair` in the order (0,1) (0,2) .. (1,2) ..
__host__ __device__ inline void pair_blocks(int pair, int nbk, int &I, int &J) {
    I = 0;
    while (pair >= nbk - 1 - I) {
        pair -= nbk - 1 - I;
        ++I;
    }
    J = I + 1 + pair;
}

}  // namespace

#endif
#else   // ---- the body of the kernel ----
    extern __shared__ __attribute__((aligned(32))) unsigned char smem_raw[];
    constexpr int CAP = 16 * NBLK, HB = CAP / 2, NU = NBLK * (NBLK + 1) / 2;
    T *rs = reinterpret_cast<T *>(smem_raw);   // r[slot][pixel]
    T *Gs = rs + CAP * kGramStride;            // gw of the tile's pixels (0: outside the sample or weight <= 0)
    // the half is the same for a whole wave; read through lane 0 so that the compiler knows it too: the plane, and with it
    // the address of the taps, is then uniform and the taps come through the scalar cache
    const int half = HALVES == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)threadIdx.x / kAtomThreads);
    const int tid = (int)threadIdx.x - half * kAtomThreads;
    T *Hs = Gs + kGramTilePix + (size_t)half * p.h_elems;   // this half's tile of a plane of H with its halo
    constexpr int THREADS = kAtomThreads * HALVES, WAVES = kWaves * HALVES;
    double *red = reinterpret_cast<double *>(smem_raw + p.red_off);   // [slot][wave]: the waves' sums of r * (G d)
    const AtomPlan &ap = p.ap;
    const int Mo = g.M / group;

    unsigned bid = blockIdx.x;
    const int pair = bid % p.pairs;
    bid /= p.pairs;
    const int strip = bid % p.strips;
    const int n = bid / p.strips;
    int I, J;
    pair_blocks(pair, p.nbk, I, J);
    // atoms of the two blocks that exist; atom I * HB + i sits in slot i, atom J * HB + j in slot HB + j
    const int nI = max(0, min(HB, Mo - I * HB)), nJ = max(0, min(HB, Mo - J * HB));
    // half h builds the atoms h, h + HALVES, ... of the nI + nJ; both halves make the same number of trips (the barriers)
    const int nst = nI + nJ;
    const int planes = (nst + HALVES - 1) / HALVES * group;
    auto plane_of = [&](int q, int &slot, int &t) {   // -1: no atom left for this half
        const int sa = q / group * HALVES + half;
        t = q - q / group * group;
        if (sa >= nst) return -1;
        slot = sa < nI ? sa : HB + sa - nI;
        return (sa < nI ? I * HB + sa : J * HB + sa - nI) * group + t;
    };

    const int lane = tid & 63, wave = tid >> 6;   // (wave: within the half)
    const int txt = ap.TX / kAtomPix;   // threads along x
    const int tx = tid % txt, ty = tid / txt;

    // rows of atoms that do not exist are read by the matrix cores: zeros; so are their sums
    for (int i = threadIdx.x; i < CAP * kGramStride; i += THREADS) rs[i] = T(0);
    for (int i = threadIdx.x; i < CAP * kWaves; i += THREADS) red[i] = 0.0;

    const int nel = ap.SH * ap.SW;
    const int dr = kAtomThreads / ap.SW, dq = kAtomThreads - dr * ap.SW;
    const int r_first = tid / ap.SW, q_first = tid - r_first * ap.SW;
    const bool pre_ok = nel <= kStage * kAtomThreads;   // (uniform)

    Acc acc[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) acc[u] = Acc(0.0);
    double acc_a = 0.0;   // thread `slot`: a of the slot's atom over the strip

    const int t_end = min(p.tiles, (strip + 1) * kGramStripTiles);
    for (int ti = strip * kGramStripTiles; ti < t_end; ++ti) {
        const int tyi = ti / ap.tiles_x, txi = ti - tyi * ap.tiles_x;
        const int y0 = tyi * ap.TY, x0 = txi * ap.TX;
        const int y = y0 + ty, xb = x0 + tx * kAtomPix;
        for (int c = 0; c < g.C; ++c) {
            // the two factors of this thread's pixels, from the hook: pixels outside the sample and entries of weight <= 0
            // (whatever V holds there) carry exact zeros
            T gd[kAtomPix];
            Quad<T> gw;
#pragma unroll
            for (int px = 0; px < kAtomPix; ++px) {
                const bool in = y < g.Dy && xb + px < g.Dx;
                ATOM_GRAM_PIXEL(in, (((size_t)n * g.C + c) * g.Dy + y) * g.Dx + xb + px);
            }
            // (the previous pass's contraction is behind the barrier that ends it)
            if (half == 0) reinterpret_cast<Quad<T> *>(Gs)[tid] = gw;
            const size_t wrow = (size_t)c * g.Ay * ap.NBO;

            T pre[kStage];
            auto fetch = [&](int plane) {
                const T *h = H + ((size_t)n * g.M + plane) * g.Hy * g.Hs;   // (rows of H may be padded: g.Hs >= g.Hx)
                int rr = r_first, q = q_first;
#pragma unroll
                for (int k = 0; k < kStage; ++k) {
                    const int hy = y0 + rr, hx = x0 + q;
                    pre[k] = (k * kAtomThreads + tid < nel && hy < g.Hy && hx < g.Hx) ? h[(size_t)hy * g.Hs + hx] : T(0);
                    rr += dr;
                    q += dq;
                    if (q >= ap.SW) {
                        q -= ap.SW;
                        ++rr;
                    }
                }
            };

            Pair<T> r[kAtomPix];   // (r of pixel px is r[px].x + r[px].y)
            int slot, t;
            int plane = plane_of(0, slot, t);
            if (pre_ok && plane >= 0) fetch(plane);
            for (int q = 0; q < planes; ++q) {
                plane = plane_of(q, slot, t);
                const bool live = plane >= 0;   // (a half that is out of atoms goes through the barriers and does nothing)
                if (live && t == 0) {
#pragma unroll
                    for (int px = 0; px < kAtomPix; ++px) r[px] = Pair<T>(T(0));
                }
                __syncthreads();   // every wave is done with the previous plane
                if (!live) {
                } else if (pre_ok) {
#pragma unroll
                    for (int k = 0; k < kStage; ++k) {
                        const int i = k * kAtomThreads + tid;
                        if (i < nel) Hs[i] = pre[k];
                    }
                } else {
                    const T *h = H + ((size_t)n * g.M + plane) * g.Hy * g.Hs;
                    for (int i = tid; i < nel; i += kAtomThreads) {
                        const int rr = i / ap.SW, qq = i - rr * ap.SW;
                        const int hy = y0 + rr, hx = x0 + qq;
                        Hs[i] = (hy < g.Hy && hx < g.Hx) ? h[(size_t)hy * g.Hs + hx] : T(0);
                    }
                }
                __syncthreads();
                if (!live) continue;   // (no barrier below this line inside the loop)
                if (pre_ok && q + 1 < planes) {   // in flight under the multiply-adds
                    int s1, t1;
                    const int next = plane_of(q + 1, s1, t1);
                    if (next >= 0) fetch(next);
                }
                const Oct<T> *wq = reinterpret_cast<const Oct<T> *>(Wf) + (size_t)plane * g.C * g.Ay * ap.NBO + wrow;
                for (int a = 0; a < g.Ay; ++a) {
                    const Quad<T> *row = reinterpret_cast<const Quad<T> *>(Hs + (ty + a) * ap.SW) + tx;
                    // (the taps of a run: the same address in every thread; the next run's are loaded under this run's)
                    const Oct<T> *taps = wq + (size_t)a * ap.NBO;
                    Oct<T> eo_next = taps[0];
                    Quad<T> cur = row[0];
#pragma unroll 2
                    for (int j = 0; j < ap.NBO; ++j) {
                        const Quad<T> nxt = row[j + 1];
                        const Pair<T> x0p = cur.xy, x1p = cur.zw, x2p = nxt.xy;   // X[4j .. 4j + 5]
                        const int jn = j + 1 < ap.NBO ? j + 1 : j;
                        const Oct<T> eo = eo_next;
                        eo_next = taps[jn];
                        const Quad<T> e = eo.lo, o = eo.hi;
                        r[1] += x0p * o.xy;
                        r[1] += x1p * o.zw;
                        r[3] += x1p * o.xy;
                        r[3] += x2p * o.zw;
                        if (j < ap.NB) {   // (E is one run shorter than O when Ax is a multiple of kAtomPix)
                            r[0] += x0p * e.xy;
                            r[0] += x1p * e.zw;
                            r[2] += x1p * e.xy;
                            r[2] += x2p * e.zw;
                        }
                        cur = nxt;
                    }
                }
                if (t != group - 1) continue;
                // r_m is complete: park it, and fold r * (G d) in double
                Quad<T> rv;
                double pa = 0.0;
#pragma unroll
                for (int px = 0; px < kAtomPix; ++px) {
                    rv[px] = r[px].x + r[px].y;
                    pa += (double)rv[px] * (double)gd[px];
                }
                reinterpret_cast<Quad<T> *>(rs + (size_t)slot * kGramStride)[tid] = rv;
                for (int o = 32; o > 0; o >>= 1) pa += __shfl_down(pa, o, 64);
                if (lane == 0) red[slot * kWaves + wave] = pa;
            }
            __syncthreads();   // the rows, G and the waves' sums are in
            if (threadIdx.x < CAP) {
#pragma unroll
                for (int wv = 0; wv < kWaves; ++wv) acc_a += red[tid * kWaves + wv];   // wave order: fixed
            }
            // the contraction over this wave's share (a quarter, with two halves an eighth) of the tile: lane (i, k) =
            // (lane & 15, lane >> 4) holds row i of A and column i of B at the pixel of k-slot k
            const int li = lane & 15, lk = lane >> 4;
            const int gwave = half * kWaves + wave;
            for (int it = 0; it < kGramTilePix / WAVES / 16; ++it) {
                const int pix = gwave * (kGramTilePix / WAVES) + it * 16 + 4 * lk;
                const Quad<T> gq = *reinterpret_cast<const Quad<T> *>(Gs + pix);
                Quad<T> rq[NBLK];
#pragma unroll
                for (int b = 0; b < NBLK; ++b)
                    rq[b] = *reinterpret_cast<const Quad<T> *>(rs + (size_t)(b * 16 + li) * kGramStride + pix);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    double bop[NBLK], aop[NBLK];
#pragma unroll
                    for (int b = 0; b < NBLK; ++b) {
                        bop[b] = (double)rq[b][e];
                        aop[b] = (double)gq[e] * bop[b];
                    }
                    int u = 0;
#pragma unroll
                    for (int bi = 0; bi < NBLK; ++bi)
#pragma unroll
                        for (int bj = bi; bj < NBLK; ++bj, ++u)
                            acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[bi], bop[bj], acc[u], 0, 0, 0);
                }
            }
            __syncthreads();   // every wave is done with the rows and G
        }
    }

    // the waves' blocks through LDS (over the rows, which are done with), added in wave order
    double *sc = reinterpret_cast<double *>(smem_raw);
    {
        const int col = lane & 15, row0 = lane >> 4;
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
                sc[(((half * kWaves + wave) * NU + u) * 16 + row0 + 4 * reg) * 16 + col] = acc[u][reg];
    }
    __syncthreads();
    double *out = partials + (size_t)blockIdx.x * p.wg_doubles;
    for (int i = threadIdx.x; i < NU * 256; i += THREADS) {
        const int u = i >> 8, row = (i >> 4) & 15, col = i & 15;
        double sum = 0.0;
#pragma unroll
        for (int wv = 0; wv < WAVES; ++wv) sum += sc[(wv * NU + u) * 256 + (i & 255)];
        int bi = 0, bj = u;   // u -> (bi, bj), bi <= bj, in the order of the accumulators
        while (bj >= NBLK - bi) {
            bj -= NBLK - bi;
            ++bi;
        }
        bj += bi;
        out[(bi * 16 + row) * CAP + bj * 16 + col] = sum;
    }
    if (threadIdx.x < CAP) out[CAP * CAP + tid] = acc_a;
#endif
