// atom_gram.hip -- how atoms overlap, in one pass over the activations (tnmf_hip_atom_gram).
//
// With R_m the contribution of atom m in its `group` orientations (planes m * group + t of H and W) and d = V - R:
//   a[n, m] = sum G * R_m * d        B[n, m, m'] = sum G * R_m * R_m'        (G = 1 without weights)
// diag(B) is the b of atoms.hip; with a and B the objective is an exact quadratic in per-atom scale factors.
//
// One workgroup = one (sample, strip of kGramStripTiles pixel tiles, pair (I, J) of atom blocks).  Per tile and channel it
// builds r_m of the atoms of its two blocks exactly as k_atom_terms does -- planes of H streamed through LDS, taps through
// the scalar cache from the flipped copy, packed f32 pairs -- and, when an atom's last plane is in, parks r_m of the tile in
// LDS (and folds r * (G d) into a double, as k_atom_terms).  Then the four waves contract the parked rows over the tile's
// pixels on the matrix cores: v_mfma_f64_16x16x4_f64 on 16 x 16 blocks of atom pairs, operands G * r_m (the product in
// double) and r_m' converted to double, a quarter of the pixels per wave.  The accumulators stay in registers over the
// tiles and channels of the strip; at its end the waves' blocks are added in wave order and written once per workgroup.
//
// Only blocks on or above the diagonal are accumulated, and k_atom_gram_finalize reads entry (m, m') and (m', m) from the
// same place: B is symmetric to the bit.  It adds the strips in strip order.  No atomics: the same bits every run.
//
// With 32 rows parked only one workgroup fits a CU, so there the workgroup has 512 threads where the LDS allows: two halves
// of 256 that build different atoms of the same tile at the same time, each from a tile of H of its own (HALVES = 2; the
// contraction then gives every one of the eight waves an eighth of the pixels).
//
// M / group <= cap: one pair, blocks 0 and 1 are the atoms in order.  More atoms: every pair I < J of blocks of cap / 2
// atoms is a workgroup of its own that builds r of both blocks again; the diagonal block of I (and a) is taken from the pair
// (I, I + 1), of the last block from (I - 1, I).
#include <algorithm>

#include "atom_gram.h"

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

// the flipped dictionary in runs of kAtomPix taps, plain (E) and shifted by one (O): the layout of k_atom_taps (atoms.hip)
template <typename T>
__global__ __launch_bounds__(kAtomThreads) void k_gram_taps(int rows, int Ay, int Ax, int NBO, const T *__restrict__ W,
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

// the pair (I, J), I < J < nbk, of index `pair` in the order (0,1) (0,2) .. (1,2) ..
__host__ __device__ inline void pair_blocks(int pair, int nbk, int &I, int &J) {
    I = 0;
    while (pair >= nbk - 1 - I) {
        pair -= nbk - 1 - I;
        ++I;
    }
    J = I + 1 + pair;
}

template <typename T, int NBLK, int HALVES>   // NBLK = cap / 16
__global__ __launch_bounds__(kAtomThreads * HALVES) void k_atom_gram(Geo g, GramPlan p, int group,
                                                                     const T *__restrict__ V, const T *__restrict__ G,
                                                                     const T *__restrict__ R, const T *__restrict__ Wf,
                                                                     const T *__restrict__ H, double *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(32))) unsigned char smem_raw[];
    constexpr int CAP = 16 * NBLK, HB = CAP / 2, NU = NBLK * (NBLK + 1) / 2;
    T *rs = reinterpret_cast<T *>(smem_raw);   // r[slot][pixel]
    T *Gs = rs + CAP * kGramStride;            // G of the tile's pixels (0: outside the sample or weight <= 0)
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
            // G * d and G of this thread's pixels: pixels outside the sample and entries of weight <= 0 (whatever V holds
            // there) carry exact zeros
            T gd[kAtomPix];
            Quad<T> gw;
#pragma unroll
            for (int px = 0; px < kAtomPix; ++px) {
                const bool in = y < g.Dy && xb + px < g.Dx;
                T w = T(0), d = T(0);
                if (in) {
                    const size_t o = (((size_t)n * g.C + c) * g.Dy + y) * g.Dx + xb + px;
                    w = G ? G[o] : T(1);
                    d = V[o] - R[o];
                }
                gw[px] = w > T(0) ? w : T(0);
                gd[px] = w > T(0) ? w * d : T(0);
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

// B[n, m, m'] = B[n, m', m] = the strips' sums of the entry (min, max) in strip order; a[n, m] next to the diagonal
__global__ __launch_bounds__(kAtomThreads) void k_atom_gram_finalize(size_t total, GramPlan p, int Mo,
                                                                     const double *__restrict__ partials,
                                                                     double *__restrict__ a, double *__restrict__ B) {
    const size_t i = (size_t)blockIdx.x * kAtomThreads + threadIdx.x;
    if (i >= total) return;
    const int m2 = (int)(i % Mo);
    const size_t rest = i / Mo;
    const int m1 = (int)(rest % Mo);
    const size_t n = rest / Mo;
    const int lo = m1 < m2 ? m1 : m2, hi = m1 < m2 ? m2 : m1;
    int I = lo / p.hb, J = hi / p.hb;
    if (I == J) {
        if (I + 1 < p.nbk) J = I + 1;
        else I = J - 1;
    }
    int pair = J - I - 1;
    for (int k = 0; k < I; ++k) pair += p.nbk - 1 - k;
    const int si = lo / p.hb == I ? lo - I * p.hb : p.hb + lo - J * p.hb;
    const int sj = hi / p.hb == I ? hi - I * p.hb : p.hb + hi - J * p.hb;
    const double *in = partials + ((size_t)n * p.strips * p.pairs + pair) * p.wg_doubles;
    double sb = 0.0, sa = 0.0;
    for (int s = 0; s < p.strips; ++s) {
        const double *wg = in + (size_t)s * p.pairs * p.wg_doubles;
        sb += wg[si * p.cap + sj];
        if (m1 == m2) sa += wg[p.cap * p.cap + si];
    }
    B[i] = sb;
    if (m1 == m2) a[n * Mo + m1] = sa;
}

template <typename T, int NBLK, int HALVES>
int launch_gram(const tnmf_hip_ctx *ctx, const Geo &g, const GramPlan &p, int group, unsigned blocks, const void *V,
                const void *G, const void *R,
                const void *Wf, const void *H, double *partials, hipStream_t s) {
    // more than 64 KiB of dynamic LDS is an attribute of the (function, device) pair: set once for each
    static bool opted_in[64] = {};
    const int dev = ctx->device;
    if (p.lds > 64 * 1024 && !(dev >= 0 && dev < 64 && opted_in[dev])) {
        TNMF_HIP_TRY(hipFuncSetAttribute((const void *)k_atom_gram<T, NBLK, HALVES>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGramLds));
        if (dev >= 0 && dev < 64) opted_in[dev] = true;
    }
    hipLaunchKernelGGL((k_atom_gram<T, NBLK, HALVES>), dim3(blocks), dim3(kAtomThreads * HALVES), p.lds, s, g, p, group,
                       (const T *)V,
                       (const T *)G, (const T *)R, (const T *)Wf, (const T *)H, partials);
    return TNMF_OK;
}

}  // namespace

GramPlan atom_gram_plan(const Geo &g, int dtype, int group) {
    GramPlan p;
    p.ap = atom_terms_plan(g);
    const int Mo = g.M / group;
    const size_t es = esize(dtype);
    const size_t h_bytes = align_up((size_t)p.ap.SH * p.ap.SW * es, 32);
    auto lds_of = [&](int cap, int halves) {
        return ((size_t)cap * kGramStride + kGramTilePix) * es + halves * h_bytes + (size_t)cap * kWaves * sizeof(double);
    };
    p.cap = Mo > 16 && lds_of(32, 1) <= kGramLds ? 32 : lds_of(16, 1) <= kGramLds ? 16 : 0;
    p.halves = p.cap == 32 && lds_of(32, 2) <= kGramLds ? 2 : 1;   // (16 rows leave room for two workgroups per CU as it is)
    p.h_elems = h_bytes / es;
    p.hb = p.cap / 2;
    p.nbk = p.cap ? std::max(2, cdiv(Mo, p.hb)) : 2;
    p.pairs = p.nbk * (p.nbk - 1) / 2;
    p.tiles = p.ap.tiles_y * p.ap.tiles_x;
    p.strips = cdiv(p.tiles, kGramStripTiles);
    p.red_off = ((size_t)p.cap * kGramStride + kGramTilePix) * es + p.halves * h_bytes;
    p.lds = lds_of(p.cap, p.halves);
    p.wg_doubles = (size_t)p.cap * p.cap + p.cap;
    return p;
}

size_t atom_gram_partial_bytes(const Geo &g, int dtype, int group) {
    const GramPlan p = atom_gram_plan(g, dtype, group);
    return align_up((size_t)g.N * p.strips * p.pairs * p.wg_doubles * sizeof(double), 256);
}

int atom_gram_check(const Geo &g, int dtype, int group) {
    const GramPlan p = atom_gram_plan(g, dtype, group);
    if (p.cap == 0) return TNMF_E_UNSUPPORTED;
    if ((size_t)g.N * p.strips * p.pairs > 0x7fffffffull) return TNMF_E_GEOM;
    return TNMF_OK;
}

int launch_atom_gram(const tnmf_hip_ctx *ctx, const Geo &g, int dtype, int group, const void *V, const void *G,
                     const void *R, const void *W, const void *H, double *partials, void *taps, double *a, double *B,
                     hipStream_t s) {
    const int rc = atom_gram_check(g, dtype, group);
    if (rc != TNMF_OK) return rc;
    const GramPlan p = atom_gram_plan(g, dtype, group);
    const size_t blocks = (size_t)g.N * p.strips * p.pairs;
    const int rows = g.M * g.C;
    const size_t n_taps = (size_t)rows * g.Ay * p.ap.NBO * 2 * kAtomPix;
    const unsigned tap_blocks = (unsigned)std::min<size_t>((n_taps + kAtomThreads - 1) / kAtomThreads, (size_t)ctx->num_cu * 8);
    const int lrc = with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL(k_gram_taps<T>, dim3(tap_blocks), dim3(kAtomThreads), 0, s, rows, g.Ay, g.Ax, p.ap.NBO,
                           (const T *)W, (T *)taps);
        if constexpr (sizeof(T) == sizeof(float)) {   // (32 rows of doubles never fit: those kernels do not exist)
            if (p.halves == 2) return launch_gram<T, 2, 2>(ctx, g, p, group, (unsigned)blocks, V, G, R, taps, H, partials, s);
            if (p.cap == 32) return launch_gram<T, 2, 1>(ctx, g, p, group, (unsigned)blocks, V, G, R, taps, H, partials, s);
        }
        if (p.cap != 16) return (int)TNMF_E_UNSUPPORTED;
        return launch_gram<T, 1, 1>(ctx, g, p, group, (unsigned)blocks, V, G, R, taps, H, partials, s);
    });
    if (lrc != TNMF_OK) return lrc;
    TNMF_LAUNCH_CHECK();
    const int Mo = g.M / group;
    const size_t total = (size_t)g.N * Mo * Mo;
    hipLaunchKernelGGL(k_atom_gram_finalize, dim3((unsigned)((total + kAtomThreads - 1) / kAtomThreads)), dim3(kAtomThreads),
                       0, s, total, p, Mo, (const double *)partials, a, B);
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}
