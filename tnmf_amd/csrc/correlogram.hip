// correlogram.hip -- which planes of H co-occur, and at what offset (tnmf_hip_activation_correlogram).
//
//   C[n, p, q, D] = sum_u H[n, p, u] * H[n, q, u + D]        over the u with u and u + D inside the plane, |D_k| <= L_k
//
// For one lag D, C[:, :, D] is a P x P product contracted over the pixels: A * B_D^T with B_D the planes shifted by D.
// One workgroup = one (segment, strip of (sample, pixel tile) items, ordered pair (I, J) of blocks of 16 planes, lag
// chunk).  A lag chunk is one dy >= 0 and up to kCorrChunk consecutive dx; only the half of the lags that is >= 0 in C
// order (dy > 0, or dy == 0 and dx >= 0) is computed.  Per item the workgroup stages the TY x TX tile of the planes of
// block I in LDS, and the TY x (TX + kCorrChunk) window of the planes of block J that the tile meets under the lags of the
// chunk: rows y0 + dy .., columns x0 + dx0 ..; whatever lies outside the plane -- pad columns included -- is an exact
// zero and never read.  Wave w then contracts the tile for the lags w, w + 4, ... of the chunk on the matrix cores:
// v_mfma_f64_16x16x4_f64, four pixels a step, both operands converted to double (the products of floats are exact), one
// accumulator of 16 x 16 sums per lag in registers over all the items of the strip.  No two waves share a sum.
// The tile is a template parameter, so the stage is a fixed set of registers: a wave loads its rows of the next item before
// it starts the matrix work on the current one and stores them to LDS behind the barrier that ends it.
//
// The accumulators go to the partial sums [segment][strip][pair][lag][16][16]; k_correlogram_finalize adds the strips in
// strip order and writes every element of C: C[p, q, D] for D >= 0 from the pair (block of p, block of q), C[p, q, D] for
// D < 0 from the entry (q, p, -D) of the transposed pair -- the same sum, so C[p, q, D] == C[q, p, -D] to the bit -- and
// zeros where |D_k| >= S_k.  At D = 0 both orders of a pair would be computed: there only p <= q is (a pair of blocks
// below the diagonal skips the lag; inside a diagonal block the entries p > q are not read).  No atomics: the same bits
// every run.
#include <algorithm>

#include "correlogram.h"

namespace {

using Acc = double __attribute__((ext_vector_type(4)));
constexpr int kWaves = kCorrThreads / 64;
constexpr int kLagsPerWave = kCorrChunk / kWaves;

// lag chunk c: its row dy, its first dx and how many lags it holds
__host__ __device__ inline void corr_chunk(const CorrPlan &p, int c, int &dy, int &dx0, int &nl) {
    if (c < p.c0) {
        dy = 0;
        dx0 = c * kCorrChunk;
    } else {
        dy = 1 + (c - p.c0) / p.cr;
        dx0 = -p.Lxe + (c - p.c0) % p.cr * kCorrChunk;
    }
    nl = p.Lxe - dx0 + 1 < kCorrChunk ? p.Lxe - dx0 + 1 : kCorrChunk;
}

// the place of the lag (dy, dx) >= 0 among the lags computed
__host__ __device__ inline int corr_lag_index(const CorrPlan &p, int dy, int dx) {
    return dy == 0 ? dx : p.Lxe + 1 + (dy - 1) * (2 * p.Lxe + 1) + dx + p.Lxe;
}

template <typename T, int TY, int TX>
__global__ __launch_bounds__(kCorrThreads) void k_correlogram(CorrPlan p, const T *__restrict__ H,
                                                              double *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int SA = TX + kCorrPad, WB = TX + kCorrChunk, SB = WB + kCorrPad;
    constexpr int ROWS = TY * kCorrBlock / kWaves;      // staged rows of each block per wave: (row of the tile, plane)
    constexpr int NA = TX / 64, NB = (WB + 63) / 64;    // loads of 64 lanes per row of the tile, of the window
    static_assert(TX % 64 == 0 && TY * kCorrBlock % kWaves == 0, "whole waves per staged row");
    T *As = reinterpret_cast<T *>(smem_raw);   // [row of the tile][plane of I][column]
    T *Bs = As + TY * kCorrBlock * SA;         // [row of the tile][plane of J][column of the window]

    unsigned bid = blockIdx.x;
    const int chunk = bid % p.chunks;
    bid /= p.chunks;
    const int pair = bid % p.pairs;
    bid /= p.pairs;
    const int strip = bid % p.strips;
    const int seg = bid / p.strips;
    const int I = pair / p.nb, J = pair - I * p.nb;
    int dy, dx0, nl;
    corr_chunk(p, chunk, dy, dx0, nl);
    // lag 0 of a pair of blocks below the diagonal is the transposed pair's: not computed, never read
    const int skip = (I > J && dy == 0 && dx0 == 0) ? 0 : -1;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lk = lane >> 4;   // operand lane: plane li of its block at the pixel of k-slot lk

    Acc acc[kLagsPerWave];
#pragma unroll
    for (int j = 0; j < kLagsPerWave; ++j) acc[j] = Acc(0.0);

    // item `it` of the segment: its sample and the corner of its tile
    auto locate = [&](long long it, int &n, int &y0, int &x0) {
        const long long item = (long long)seg * p.seglen + it;
        n = (int)(item / p.tiles);
        const int tile = (int)(item - (long long)n * p.tiles);
        const int tyi = tile / p.tiles_x;
        y0 = tyi * TY, x0 = (tile - tyi * p.tiles_x) * TX;
    };
    // the register stage: wave w holds the staged rows w, w + 4, ... of both blocks, one element per lane and load;
    // whatever lies outside the plane is a zero and is not read
    T pa[ROWS][NA], pb[ROWS][NB];
    auto fetch = [&](long long it) {
        int n, y0, x0;
        locate(it, n, y0, x0);
        const T *Hn = H + (size_t)n * p.P * p.Sy * p.Hs;
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const int rp = wave + kWaves * k, r = rp / kCorrBlock, pl = rp - r * kCorrBlock;
            {
                const int plane = I * kCorrBlock + pl;
                const bool row_in = plane < p.P && y0 + r < p.Sy;
                const T *h = Hn + (row_in ? ((size_t)plane * p.Sy + y0 + r) * p.Hs : 0);
#pragma unroll
                for (int c = 0; c < NA; ++c) {
                    const int x = x0 + c * 64 + lane;
                    pa[k][c] = (row_in && x < p.Sx) ? h[x] : T(0);
                }
            }
            {
                const int plane = J * kCorrBlock + pl, y = y0 + dy + r;
                const bool row_in = plane < p.P && y0 + r < p.Sy && y < p.Sy;
                const T *h = Hn + (row_in ? ((size_t)plane * p.Sy + y) * p.Hs : 0);
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    const int x = x0 + dx0 + c * 64 + lane;
                    pb[k][c] = (row_in && x >= 0 && x < p.Sx) ? h[x] : T(0);
                }
            }
        }
    };

    const long long i0 = (long long)strip * p.ipg;
    const long long i1 = i0 + p.ipg < p.seglen ? i0 + p.ipg : p.seglen;
    if (i0 < i1) fetch(i0);
    for (long long it = i0; it < i1; ++it) {
        int n, y0, x0;
        locate(it, n, y0, x0);
        const int rn = min(TY, p.Sy - y0), cn = min(TX, p.Sx - x0);   // rows and columns of the tile inside the plane
        __syncthreads();   // every wave is done with the previous item
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const int rp = wave + kWaves * k;
#pragma unroll
            for (int c = 0; c < NA; ++c) As[rp * SA + c * 64 + lane] = pa[k][c];
#pragma unroll
            for (int c = 0; c < NB; ++c)
                if (c * 64 + 64 <= WB || c * 64 + lane < WB) Bs[rp * SB + c * 64 + lane] = pb[k][c];
        }
        __syncthreads();
        if (it + 1 < i1) fetch(it + 1);   // in flight under the matrix work
        const int gn = (cn + 3) / 4;      // steps of four pixels along a row
        for (int r = 0; r < rn; ++r) {
            const T *arow = As + (r * kCorrBlock + li) * SA + lk;
            const T *brow = Bs + (r * kCorrBlock + li) * SB + lk + wave;
            for (int gx = 0; gx < gn; ++gx) {
                const double a = (double)arow[4 * gx];
#pragma unroll
                for (int j = 0; j < kLagsPerWave; ++j) {
                    const int l = wave + kWaves * j;   // (uniform over the wave)
                    if (l < nl && l != skip)
                        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)brow[4 * gx + kWaves * j], acc[j], 0, 0, 0);
                }
            }
        }
    }

    // accumulator register reg of lane (li, lk) is the sum of row (plane of I) lk + 4 reg, column (plane of J) li
    double *out = partials + ((((size_t)seg * p.strips + strip) * p.pairs + pair) * p.nh + corr_lag_index(p, dy, dx0)) * 256;
#pragma unroll
    for (int j = 0; j < kLagsPerWave; ++j) {
        const int l = wave + kWaves * j;
        if (l >= nl) continue;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) out[(size_t)l * 256 + (lk + 4 * reg) * kCorrBlock + li] = acc[j][reg];
    }
}

// every element of C: the strips' sums in strip order, the mirror from the same partial sums, zeros beyond the extent
__global__ __launch_bounds__(kCorrThreads) void k_correlogram_finalize(size_t total, CorrPlan p,
                                                                       const double *__restrict__ partials,
                                                                       double *__restrict__ C) {
    const size_t i = (size_t)blockIdx.x * kCorrThreads + threadIdx.x;
    if (i >= total) return;
    const int wx = 2 * p.Lx + 1, wy = 2 * p.Ly + 1;
    size_t rest = i;
    int dx = (int)(rest % wx) - p.Lx;
    rest /= wx;
    int dy = (int)(rest % wy) - p.Ly;
    rest /= wy;
    int q = (int)(rest % p.P);
    rest /= p.P;
    int pp = (int)(rest % p.P);
    const size_t seg = rest / p.P;
    if (dy > p.Lye || -dy > p.Lye || dx > p.Lxe || -dx > p.Lxe) {   // at or beyond the extent of an axis
        C[i] = 0.0;
        return;
    }
    const bool mirror = dy < 0 || (dy == 0 && (dx < 0 || (dx == 0 && pp > q)));
    if (mirror) {
        const int t = pp;
        pp = q, q = t;
        dy = -dy, dx = -dx;
    }
    const int pair = pp / kCorrBlock * p.nb + q / kCorrBlock;
    const int e = pp % kCorrBlock * kCorrBlock + q % kCorrBlock;
    const size_t stride = (size_t)p.pairs * p.nh * 256;
    const double *in = partials + seg * p.strips * stride + ((size_t)pair * p.nh + corr_lag_index(p, dy, dx)) * 256 + e;
    double sum = 0.0;
    for (int s = 0; s < p.strips; ++s) sum += in[(size_t)s * stride];
    C[i] = sum;
}

}  // namespace

int correlogram_plan(int N, int P, int Sy, int Sx, int Hs, int ndim, const int *max_lag, int per_sample, int dtype,
                     CorrPlan *out) {
    CorrPlan p;
    p.P = P, p.Sy = Sy, p.Sx = Sx, p.Hs = Hs;
    p.Ly = ndim == 2 ? max_lag[0] : 0;
    p.Lx = max_lag[ndim - 1];
    if (p.Ly < 0 || p.Lx < 0) return TNMF_E_GEOM;
    const int limit = ndim == 2 ? kCorrMaxLag2 : kCorrMaxLag1;
    if (p.Ly > limit || p.Lx > limit) return TNMF_E_UNSUPPORTED;
    p.Lye = std::min(p.Ly, Sy - 1);
    p.Lxe = std::min(p.Lx, Sx - 1);
    p.TY = ndim == 1 ? 1 : dtype == 0 ? kCorrTileYFloat : kCorrTileYDouble;
    p.TX = ndim == 2 ? kCorrTileX : dtype == 0 ? kCorrTile1Float : kCorrTile1Double;
    p.tiles_y = (int)(((long long)Sy + p.TY - 1) / p.TY);   // (an extent near 2^31: no overflow)
    p.tiles_x = (int)(((long long)Sx + p.TX - 1) / p.TX);
    if ((long long)p.tiles_y * p.tiles_x > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    p.tiles = p.tiles_y * p.tiles_x;
    p.nb = cdiv(P, kCorrBlock);
    if ((long long)p.nb * p.nb > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    p.pairs = p.nb * p.nb;
    p.c0 = cdiv(p.Lxe + 1, kCorrChunk);
    p.cr = cdiv(2 * p.Lxe + 1, kCorrChunk);
    p.chunks = p.c0 + p.Lye * p.cr;
    p.nh = p.Lxe + 1 + p.Lye * (2 * p.Lxe + 1);
    p.nseg = per_sample ? N : 1;
    p.seglen = per_sample ? (long long)p.tiles : (long long)N * p.tiles;
    // (sizes no memory holds, in double so that nothing below overflows: the finalize's grid, the workgroups)
    const double outputs = (double)p.nseg * P * P * (2 * p.Ly + 1) * (2 * p.Lx + 1);
    if (outputs / kCorrThreads >= 2147483647.0 || (double)p.nseg * p.pairs * p.chunks >= 2147483647.0)
        return TNMF_E_UNSUPPORTED;
    // strips: enough workgroups to fill the device, no more partial sums than kCorrPartialCap, at least one item each
    // (no sample: no item and, per sample, no segment -- one empty strip, nothing to divide by)
    const long long units = std::max<long long>(1, (long long)p.nseg * p.pairs * p.chunks);
    const long long want = (kCorrTargetGroups + units - 1) / units;
    const unsigned long long strip_bytes = std::max<unsigned long long>(1, (unsigned long long)p.nseg * p.pairs * p.nh * 256 * sizeof(double));
    const long long cap = std::max<long long>(1, (long long)(kCorrPartialCap / strip_bytes));
    const long long strips = std::max<long long>(1, std::min(std::min(want, cap), p.seglen));
    p.ipg = std::max<long long>(1, (p.seglen + strips - 1) / strips);
    p.strips = (int)((p.seglen + p.ipg - 1) / p.ipg);   // (no strip without an item)
    if (units * p.strips > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    p.lds = (size_t)p.TY * kCorrBlock * (2 * p.TX + kCorrChunk + 2 * kCorrPad) * esize(dtype);
    *out = p;
    return TNMF_OK;
}

size_t correlogram_partial_bytes(const CorrPlan &p) {
    return align_up((size_t)p.nseg * p.strips * p.pairs * p.nh * 256 * sizeof(double), 256);
}

int launch_correlogram(const CorrPlan &p, int dtype, const void *H, double *partials, double *C_out, hipStream_t s) {
    const unsigned blocks = (unsigned)((size_t)p.nseg * p.strips * p.pairs * p.chunks);
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        constexpr bool f = sizeof(T) == sizeof(float);
        constexpr int T1 = f ? kCorrTile1Float : kCorrTile1Double, TY2 = f ? kCorrTileYFloat : kCorrTileYDouble;
        if (p.TY == 1)   // (one shift axis)
            hipLaunchKernelGGL((k_correlogram<T, 1, T1>), dim3(blocks), dim3(kCorrThreads), p.lds, s, p, (const T *)H, partials);
        else
            hipLaunchKernelGGL((k_correlogram<T, TY2, kCorrTileX>), dim3(blocks), dim3(kCorrThreads), p.lds, s, p,
                               (const T *)H, partials);
    });
    TNMF_LAUNCH_CHECK();
    const size_t total = (size_t)p.nseg * p.P * p.P * (2 * p.Ly + 1) * (2 * p.Lx + 1);
    hipLaunchKernelGGL(k_correlogram_finalize, dim3((unsigned)((total + kCorrThreads - 1) / kCorrThreads)),
                       dim3(kCorrThreads), 0, s, total, p, (const double *)partials, C_out);
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}
