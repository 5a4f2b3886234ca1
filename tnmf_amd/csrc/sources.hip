// sources.hip -- the per-source signals of a fitted model, in one pass over the activations (tnmf_hip_atom_sources).
//
// With r_g the part of the reconstruction that the planes of source g add, and total = sum_g r_g over every plane:
//   contribution  r_g          mask  r_g / (total + eps)          masked  V * (r_g / (total + eps))
//   dominant      per pixel the source with the largest sum_c r_g, and that sum over sum_c total + eps
//
// The walk is that of atoms.hip (atom_walk.h): one workgroup = one (sample, pixel tile, chunk of up to kAtomChannels
// channels), the planes of H stream through LDS once, r_g lives in registers as a chain of non-negative products.  The
// planes come in `order`: source after source, then the planes in no source as a hidden last group.  When the last plane
// of a group is in, the thread adds r_g to its total and stores r_g raw; after the last group it reads its own stores back
// (same thread, same addresses: program order, no barrier) and rewrites them with the total now in its registers.  Every
// denominator is the pass's own ordered sum of what it divides, so r_g <= total holds in the element type -- a sum of
// non-negative terms, each add rounded monotonically, is never below a term -- and with it 0 <= mask <= 1 and
// 0 <= masked <= V, without a clamp.  Where total + eps is 0 the mask is 0.
//
// sum_c r_g is the walk on one channel whose taps are sum_c W (k_source_wsum, the channels added in channel order): the
// dominant source needs no second channel.  No atomics, no dependence on which workgroup runs when: every output element
// has one writer.
#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "atom_walk.h"
#include "sources.h"

namespace {

// tile elements per thread that the register stage holds, as in atoms.hip: 145 VGPRs with four float channels, no scratch
constexpr int kStage = 10;

// Ws[plane, a] = sum_c W[plane, c, a], in channel order
template <typename T>
__global__ __launch_bounds__(kAtomThreads) void k_source_wsum(size_t total, int C, int nA, const T *__restrict__ W,
                                                              T *__restrict__ Ws) {
    for (size_t i = (size_t)blockIdx.x * kAtomThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kAtomThreads) {
        const size_t plane = i / nA, a = i - plane * nA;
        T sum = T(0);
        for (int c = 0; c < C; ++c) sum += W[(plane * C + c) * nA + a];
        Ws[i] = sum;
    }
}

// DOM: g.C == 1 and Wf holds the taps of the channel sums; out is not touched.  Else label and share are not touched.
// vec: D_x is a multiple of kAtomPix and `out` is aligned to kAtomPix elements, so a thread's pixels are one aligned store.
template <typename T, int CH, bool DOM>
__global__ __launch_bounds__(kAtomThreads) void k_atom_sources(Geo g, AtomPlan p, int S, int emit, T eps, bool vec,
                                                               const int *__restrict__ order,
                                                               const int *__restrict__ start, const T *__restrict__ V,
                                                               const T *__restrict__ Wf, const T *__restrict__ H, T *out,
                                                               int *__restrict__ label, T *__restrict__ share) {
    extern __shared__ __attribute__((aligned(32))) unsigned char smem_raw[];
    T *Hs = reinterpret_cast<T *>(smem_raw);

    unsigned bid = blockIdx.x;
    const int chunk = bid % p.chunks;
    bid /= p.chunks;
    const int txi = bid % p.tiles_x;
    bid /= p.tiles_x;
    const int tyi = bid % p.tiles_y;
    const int n = bid / p.tiles_y;
    const int c0 = chunk * CH;
    const int nc = g.C - c0 < CH ? g.C - c0 : CH;   // channels of this chunk (uniform)

    ATOM_WALK_PIXELS();
    ATOM_WALK_TILE();
    const bool pre_ok = nel <= kStage * kAtomThreads;   // the tile fits the register stage (uniform)
    ATOM_WALK_FETCH();

    // the thread's kAtomPix pixels of channel c0 + c of source gi: element offset, and the moves that touch no pixel
    // outside the sample (with vec a thread's pixels are all inside or all outside)
    const bool row_in = y < g.Dy;
    auto at = [&](int gi, int c) { return ((((size_t)n * S + gi) * g.C + c0 + c) * g.Dy + y) * g.Dx + xb; };
    auto put = [&](T *q, const T (&v)[kAtomPix]) {
        if (vec) {
            if (xb < g.Dx) *reinterpret_cast<Quad<T> *>(q) = Quad<T>{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int px = 0; px < kAtomPix; ++px)
                if (xb + px < g.Dx) q[px] = v[px];
        }
    };
    auto get = [&](const T *q, T (&v)[kAtomPix]) {
        if (vec) {
            const Quad<T> w = xb < g.Dx ? *reinterpret_cast<const Quad<T> *>(q) : Quad<T>(T(0));
#pragma unroll
            for (int px = 0; px < kAtomPix; ++px) v[px] = w[px];
        } else {
#pragma unroll
            for (int px = 0; px < kAtomPix; ++px) v[px] = xb + px < g.Dx ? q[px] : T(0);
        }
    };

    Pair<T> r[CH][kAtomPix];   // (r of pixel px is r[c][px].x + r[c][px].y)
    T total[CH][kAtomPix];
    T best[kAtomPix];          // DOM: the largest r_g so far and its source; the first source starts, then strict >
    int arg[kAtomPix];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int px = 0; px < kAtomPix; ++px) {
            r[c][px] = Pair<T>(T(0));
            total[c][px] = T(0);
        }
#pragma unroll
    for (int px = 0; px < kAtomPix; ++px) {
        best[px] = T(0);
        arg[px] = 0;
    }

    if (pre_ok) fetch(order[0]);
    int gi = 0, end = start[1];
    for (int i = 0; i < g.M; ++i) {
        const int plane = order[i];
        ATOM_WALK_STAGE(plane, i + 1 < g.M, order[i + 1]);
        ATOM_WALK_MACS(plane, r);
        if (i + 1 != end) continue;
        // r of group gi is complete (gi == S: the hidden group, which counts in the total only)
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            T rv[kAtomPix];
#pragma unroll
            for (int px = 0; px < kAtomPix; ++px) {
                rv[px] = r[c][px].x + r[c][px].y;
                total[c][px] += rv[px];
                r[c][px] = Pair<T>(T(0));
            }
            if (DOM) {
#pragma unroll
                for (int px = 0; px < kAtomPix; ++px)
                    if (gi < S && (gi == 0 || rv[px] > best[px])) {
                        best[px] = rv[px];
                        arg[px] = gi;
                    }
            } else if (gi < S && c < nc && row_in) {
                put(out + at(gi, c), rv);
            }
        }
        ++gi;
        end = gi <= S ? start[gi + 1] : -1;
    }

    if (!row_in) return;
    if (DOM) {
#pragma unroll
        for (int px = 0; px < kAtomPix; ++px) {
            if (xb + px >= g.Dx) continue;
            const size_t o = ((size_t)n * g.Dy + y) * g.Dx + xb + px;
            const T den = total[0][px] + eps;
            label[o] = total[0][px] > T(0) ? arg[px] : -1;
            share[o] = den > T(0) ? best[px] / den : T(0);
        }
        return;
    }
    if (emit == TNMF_SOURCES_CONTRIBUTION) return;
    // the thread's own stores again, now over the total: mask, or V times the mask
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        if (c >= nc) continue;
        T scale[kAtomPix];   // (what the mask is multiplied by)
        if (emit == TNMF_SOURCES_MASKED) {
            get(V + (((size_t)n * g.C + c0 + c) * g.Dy + y) * g.Dx + xb, scale);
        } else {
#pragma unroll
            for (int px = 0; px < kAtomPix; ++px) scale[px] = T(1);
        }
        T den[kAtomPix];
#pragma unroll
        for (int px = 0; px < kAtomPix; ++px) den[px] = total[c][px] + eps;
        for (int k = 0; k < S; ++k) {
            T *q = out + at(k, c);
            T v[kAtomPix];
            get(q, v);
#pragma unroll
            for (int px = 0; px < kAtomPix; ++px) {
                const T m = den[px] > T(0) ? v[px] / den[px] : T(0);
                v[px] = emit == TNMF_SOURCES_MASKED ? scale[px] * m : m;
            }
            put(q, v);
        }
    }
}

}  // namespace

SourcesWork atom_sources_work(const Geo &g, int dtype, int n_sources, int emit) {
    SourcesWork w;
    w.taps_off = 0;
    w.wsum_off = atom_terms_taps_bytes(g, dtype);
    const size_t wsum = emit == TNMF_SOURCES_DOMINANT ? (size_t)g.M * g.Ay * g.Ax * esize(dtype) : 0;
    w.order_off = w.wsum_off + align_up(wsum, 256);
    w.start_off = w.order_off + align_up((size_t)g.M * sizeof(int), 256);
    w.total = w.start_off + align_up((size_t)(n_sources + 2) * sizeof(int), 256);
    return w;
}

int launch_atom_sources(const tnmf_hip_ctx *ctx, const Geo &g_in, int dtype, int n_sources, int emit, double eps, char *work,
                        const void *V, const void *W, const void *H, void *out, int *label, void *share, hipStream_t s) {
    const bool dom = emit == TNMF_SOURCES_DOMINANT;
    const SourcesWork wk = atom_sources_work(g_in, dtype, n_sources, emit);
    Geo g = g_in;
    if (dom) g.C = 1;   // the walk on the channel sums of W
    const int rc = atom_terms_check(g, dtype);
    if (rc != TNMF_OK) return rc;
    const AtomPlan p = atom_terms_plan(g);
    const size_t lds = (size_t)p.SH * p.SW * esize(dtype);
    const size_t blocks = (size_t)g.N * p.slots;
    const int *order = reinterpret_cast<const int *>(work + wk.order_off);
    const int *start = reinterpret_cast<const int *>(work + wk.start_off);
    void *taps = work + wk.taps_off;
    const bool vec = g.Dx % kAtomPix == 0 && reinterpret_cast<uintptr_t>(out) % (kAtomPix * esize(dtype)) == 0 &&
                     reinterpret_cast<uintptr_t>(V) % (kAtomPix * esize(dtype)) == 0;
    const void *Wt = W;
    if (dom) {
        const size_t n_sum = (size_t)g.M * g.Ay * g.Ax;
        const unsigned sum_blocks =
            (unsigned)std::min<size_t>((n_sum + kAtomThreads - 1) / kAtomThreads, (size_t)ctx->num_cu * 8);
        with_dtype(dtype, [&](auto zero) {
            using T = decltype(zero);
            hipLaunchKernelGGL(k_source_wsum<T>, dim3(sum_blocks), dim3(kAtomThreads), 0, s, n_sum, g_in.C, g.Ay * g.Ax,
                               (const T *)W, (T *)(work + wk.wsum_off));
        });
        TNMF_LAUNCH_CHECK();
        Wt = work + wk.wsum_off;
    }
    const int rt = launch_atom_taps(ctx, g, dtype, Wt, taps, s);
    if (rt != TNMF_OK) return rt;
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        auto launch = [&](auto ch, auto dominant) {
            hipLaunchKernelGGL((k_atom_sources<T, decltype(ch)::value, decltype(dominant)::value>), dim3((unsigned)blocks),
                               dim3(kAtomThreads), lds, s, g, p, n_sources, emit, (T)eps, vec, order, start, (const T *)V,
                               (const T *)taps, (const T *)H, (T *)out, label, (T *)share);
        };
        using std::integral_constant;
        using std::false_type;
        if (dom) return launch(integral_constant<int, 1>{}, std::true_type{});
        switch (p.CH) {
            case 1: return launch(integral_constant<int, 1>{}, false_type{});
            case 2: return launch(integral_constant<int, 2>{}, false_type{});
            case 3: return launch(integral_constant<int, 3>{}, false_type{});
            default: return launch(integral_constant<int, 4>{}, false_type{});
        }
    });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}
