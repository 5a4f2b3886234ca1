// atom_gram_beta.hip -- how atoms overlap under a beta-divergence, in one pass over the activations
// (tnmf_hip_atom_gram_beta).
//
// The kernel of atom_gram.hip -- one workgroup per (sample, strip of pixel tiles, pair of atom blocks), r_m of the tile
// parked in LDS and contracted over the pixels on the matrix cores (v_mfma_f64_16x16x4_f64) -- with the pixel factors of
// atom_beta.h in the place of G d and G.  With x = max(R, 0) + eps:
//   a[n, m]     = sum G R_m (V x^(beta-2) - x^(beta-1))
//   B[n, m, m'] = sum G c R_m R_m',       c = (beta-1) x^(beta-2) + (2-beta) V x^(beta-3)
// The weights G c of the contraction are signed (c < 0 occurs outside 1 <= beta <= 2): nothing clamps them at 0, and only
// G <= 0 selects an exact zero.  Both factors are formed in double and rounded once to the element type.
//
// The plan, the partial sums, the taps and the finalize kernel are those of atom_gram.hip (launch_atom_gram_finalize); B is
// symmetric to the bit and the same from run to run for the same reasons.
#include <algorithm>
#include <cmath>

#include "atom_beta.h"

namespace {

constexpr int kStage = 10;   // tile elements per thread that the register stage holds; larger tiles: the plain loop
constexpr int kWaves = kAtomThreads / 64;   // waves of a half

static_assert(kAtomPix == 4, "the multiply-adds below are written for four pixels per thread");
template <typename T>
using Quad = T __attribute__((ext_vector_type(4)));
template <typename T>
using Pair = T __attribute__((ext_vector_type(2)));
template <typename T>
using Oct = T __attribute__((ext_vector_type(8)));
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

template <typename T, int NBLK, int HALVES, int K>   // NBLK = cap / 16; K: the beta_kind of atom_beta.h
__global__ __launch_bounds__(kAtomThreads * HALVES) void k_atom_gram_beta(Geo g, GramPlan p, int group, double beta,
                                                                          double eps, const T *__restrict__ V,
                                                                          const T *__restrict__ G, const T *__restrict__ R,
                                                                          const T *__restrict__ Wf, const T *__restrict__ H,
                                                                          double *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(32))) unsigned char smem_raw[];
    constexpr int CAP = 16 * NBLK, HB = CAP / 2, NU = NBLK * (NBLK + 1) / 2;
    T *rs = reinterpret_cast<T *>(smem_raw);   // r[slot][pixel]
    T *Gs = rs + CAP * kGramStride;            // G c of the tile's pixels, signed (0: outside the sample or weight <= 0)
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
            // the two factors of atom_beta.h at this thread's pixels, formed in double: pixels outside the sample and
            // entries of weight <= 0 (whatever V holds there) carry exact zeros and evaluate nothing
            T gd[kAtomPix];
            Quad<T> gw;
#pragma unroll
            for (int px = 0; px < kAtomPix; ++px) {
                const bool in = y < g.Dy && xb + px < g.Dx;
                double d = 0.0, cw = 0.0;
                if (in) {
                    const size_t o = (((size_t)n * g.C + c) * g.Dy + y) * g.Dx + xb + px;
                    const T w = G ? G[o] : T(1);
                    if (w > T(0)) beta_pixel<K>((double)V[o], (double)R[o], (double)w, eps, beta, d, cw);
                }
                gw[px] = (T)cw;
                gd[px] = (T)d;
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
}

template <typename T, int NBLK, int HALVES, int K>
int launch_gram_kind(const tnmf_hip_ctx *ctx, const GramPlan &p, unsigned blocks, hipStream_t s, Geo g, int group, double beta,
                     double eps, const T *V, const T *G, const T *R, const T *Wf, const T *H, double *partials) {
    // more than 64 KiB of dynamic LDS is an attribute of the (function, device) pair: set once for each
    static bool opted_in[64] = {};
    const int dev = ctx->device;
    if (p.lds > 64 * 1024 && !(dev >= 0 && dev < 64 && opted_in[dev])) {
        TNMF_HIP_TRY(hipFuncSetAttribute((const void *)k_atom_gram_beta<T, NBLK, HALVES, K>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGramLds));
        if (dev >= 0 && dev < 64) opted_in[dev] = true;
    }
    hipLaunchKernelGGL((k_atom_gram_beta<T, NBLK, HALVES, K>), dim3(blocks), dim3(kAtomThreads * HALVES), p.lds, s, g, p,
                       group, beta, eps, V, G, R, Wf, H, partials);
    return TNMF_OK;
}

template <typename T, int NBLK, int HALVES>
int launch_gram(const tnmf_hip_ctx *ctx, const Geo &g, const GramPlan &p, int group, double beta, double eps,
                unsigned blocks, const void *V, const void *G, const void *R, const void *Wf, const void *H,
                double *partials, hipStream_t s) {
    const T *v = (const T *)V, *gp = (const T *)G, *r = (const T *)R, *wf = (const T *)Wf, *h = (const T *)H;
    switch (beta_kind(beta)) {
        case 0: return launch_gram_kind<T, NBLK, HALVES, 0>(ctx, p, blocks, s, g, group, beta, eps, v, gp, r, wf, h, partials);
        case 1: return launch_gram_kind<T, NBLK, HALVES, 1>(ctx, p, blocks, s, g, group, beta, eps, v, gp, r, wf, h, partials);
        default: return launch_gram_kind<T, NBLK, HALVES, 3>(ctx, p, blocks, s, g, group, beta, eps, v, gp, r, wf, h, partials);
    }
}

}  // namespace

int launch_atom_gram_beta(const tnmf_hip_ctx *ctx, const Geo &g, int dtype, int group, double beta, double eps,
                          const void *V, const void *G, const void *R, const void *W, const void *H, double *partials,
                          void *taps, double *a, double *B, hipStream_t s) {
    const int rc = atom_gram_check(g, dtype, group);
    if (rc != TNMF_OK) return rc;
    const GramPlan p = atom_gram_plan(g, dtype, group);
    const size_t blocks = (size_t)g.N * p.strips * p.pairs;
    const int trc = launch_atom_taps(ctx, g, dtype, W, taps, s);
    if (trc != TNMF_OK) return trc;
    const int lrc = with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        if constexpr (sizeof(T) == sizeof(float)) {   // (32 rows of doubles never fit: those kernels do not exist)
            if (p.halves == 2)
                return launch_gram<T, 2, 2>(ctx, g, p, group, beta, eps, (unsigned)blocks, V, G, R, taps, H, partials, s);
            if (p.cap == 32)
                return launch_gram<T, 2, 1>(ctx, g, p, group, beta, eps, (unsigned)blocks, V, G, R, taps, H, partials, s);
        }
        if (p.cap != 16) return (int)TNMF_E_UNSUPPORTED;
        return launch_gram<T, 1, 1>(ctx, g, p, group, beta, eps, (unsigned)blocks, V, G, R, taps, H, partials, s);
    });
    if (lrc != TNMF_OK) return lrc;
    TNMF_LAUNCH_CHECK();
    return launch_atom_gram_finalize(g, p, group, partials, a, B, s);
}

extern "C" {

int tnmf_hip_atom_gram_beta(tnmf_hip_ctx *ctx, const tnmf_hip_geom *geom, int group, double beta, double eps, const void *V,
                            const void *G_or_null, const void *R_or_null, const void *W, const void *H, double *a, double *B,
                            void *stream) {
    if (!ctx || !geom) return TNMF_E_NULL;
    Geo g;
    int rc = atom_entry_geo(geom, &g);
    if (rc != TNMF_OK) return rc;
    const int dtype = geom->dtype;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TNMF_HIP_TRY(hipSetDevice(ctx->device));
    if (group < 1 || g.M % group != 0 || !std::isfinite(beta) || !(eps >= 0.0)) return TNMF_E_GEOM;
    if (beta == 2.0) return tnmf_hip_atom_gram(ctx, geom, group, V, G_or_null, R_or_null, W, H, a, B, stream);
    if (g.N == 0) return TNMF_OK;
    if (!V || !W || !H || !a || !B) return TNMF_E_NULL;
    rc = atom_gram_check(g, dtype, group);
    if (rc != TNMF_OK) return rc;
    // work buffer: as tnmf_hip_atom_gram
    const size_t p_bytes = atom_gram_partial_bytes(g, dtype, group);
    const void *R = R_or_null;
    void *buf = nullptr;
    rc = atom_entry_buffers(ctx, g, dtype, p_bytes + atom_terms_taps_bytes(g, dtype), W, H, &R, &buf, s);
    if (rc != TNMF_OK) return rc;
    return launch_atom_gram_beta(ctx, g, dtype, group, beta, eps, V, G_or_null, R, W, H, static_cast<double *>(buf),
                                 static_cast<char *>(buf) + p_bytes, a, B, s);
}

}  // extern "C"
