// triggered.hip -- activation-triggered sums: the data around the places where a plane of H fires, on a window larger
// than the atom (tnmf_hip_triggered_sums).
//
//   X[p, f, j] = sum_n sum_q H[n, p, q]^power * Y[n, f, q - (A - 1) - m + j]        0 <= j_k < A_k + 2 m_k
//
// H the padded activations, Y a field of the samples' shape; terms whose index falls outside the sample are absent.
// For one (field, window row jy), X[:, f, jy, :] is a P x Wx product contracted over the pixels: the B operand is the
// Toeplitz matrix of one row of Y.  v_mfma_f64_16x16x4_f64 gets 16 planes of H as its rows, 16 consecutive window columns
// jx (a CELL) as its columns and 4 consecutive pixels along x as k: the B element of lane (li, lk) is the row of Y at
// column x + lk + li + const, a read of 17 consecutive elements per half wave.
// One workgroup = one (segment, strip of (sample, pixel tile) items, block of 16 planes, chunk of cells).  A chunk is CF
// fields, CJ window rows and CB cells along jx (several fields only where the whole window of a field fits a chunk).  Per
// item the workgroup stages the TY x TX tile of its planes in LDS, and per field of the chunk the (TY + CJ - 1) x
// (TX + 16 CB) patch of Y that the tile meets under the chunk; whatever lies outside the plane or the sample -- pad
// columns included -- is an exact zero and never read.  Wave w then contracts the tile for the cells w,
// w + 4, ... of the chunk, one accumulator of 16 x 16 sums per cell in registers over all the items of the strip; a
// chunk of fewer than 4 cells is contracted by every wave for every fourth step of four pixels instead, and the waves'
// accumulators are added in wave order through LDS.  Both operands are converted to double, the square of power = 2 is
// taken in double.  The stage is a fixed set of registers: a wave loads its share of the next item before it starts the
// matrix work on the current one and stores it to LDS behind the barrier that ends it.
//
// The accumulators go to the partial sums [segment][strip][plane block][cell][16][16]; k_triggered_finalize adds the
// strips in strip order and writes every element of X.  No atomics: the same bits every run.
#include <algorithm>
#include <type_traits>

#include "triggered.h"

namespace {

using Acc = double __attribute__((ext_vector_type(4)));
constexpr int kWaves = kTrigThreads / 64;
constexpr int kCellsPerWave = kTrigChunk / kWaves;

// the most elements a staged patch of Y has with this tile, over the chunk shapes the plan chooses
constexpr int trig_patch_max(int TY, int TX) {
    int worst = 0;
    for (int cb = 1; cb <= kTrigChunk; ++cb)
        for (int cj = 1; cj <= kTrigChunk / cb; ++cj) {
            const int e = kTrigChunk / (cb * cj) * (TY + cj - 1) * (TX + kTrigBlock * cb);
            worst = e > worst ? e : worst;
        }
    return worst;
}

template <typename T, int TY, int TX>
__global__ __launch_bounds__(kTrigThreads) void k_triggered(TrigPlan p, const T *__restrict__ H, const T *__restrict__ Y,
                                                            double *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int SA = TX + kTrigPad;
    constexpr int ROWS = TY * kTrigBlock / kWaves;   // staged rows of H per wave: (row of the tile, plane)
    constexpr int NA = TX / 64;                      // loads of 64 lanes per row of the tile
    constexpr int NY = (trig_patch_max(TY, TX) + kTrigThreads - 1) / kTrigThreads;   // elements of the patch per thread
    static_assert(TX % 64 == 0 && TY * kTrigBlock % kWaves == 0, "whole waves per staged row");
    // ycode packs (field, row of the patch, column) into 15 + 6 + 10 bits: the widest chunk of every shape must fit
    static_assert(kTrigChunk <= (1 << 15), "field of the chunk in the bits above 16");
    static_assert(TY + kTrigChunk - 1 <= 64, "row of the patch in 6 bits");
    static_assert(TX + kTrigBlock * kTrigChunk <= 1024, "column of the patch in 10 bits");
    static_assert(NY * kTrigThreads >= trig_patch_max(TY, TX), "the register stage holds the widest patches");
    static_assert((TY * kTrigBlock * SA + trig_patch_max(TY, TX)) * sizeof(T) <= 64 * 1024, "tile and patches within 64 KiB of LDS");
    static_assert(kCellsPerWave == 8 && kWaves == 4, "contract() is instantiated for 1..8 cells; a split chunk has at most 3");
    static_assert(TY * kTrigBlock * SA * sizeof(T) >= 3 * 256 * sizeof(double), "the tile holds a wave's sums of a split chunk");
    T *As = reinterpret_cast<T *>(smem_raw);   // [row of the tile][plane][column]
    T *Ys = As + TY * kTrigBlock * SA;         // [field of the chunk][row of the patch][column of the patch]

    unsigned bid = blockIdx.x;
    const int chunk = bid % p.chunks;
    bid /= p.chunks;
    const int pb = bid % p.nbp;
    bid /= p.nbp;
    const int strip = bid % p.strips;
    const int seg = bid / p.strips;
    const int cx = chunk % p.chunks_x, cy = chunk / p.chunks_x % p.chunks_y, cf = chunk / (p.chunks_x * p.chunks_y);
    const int f0 = cf * p.CF, jy0 = cy * p.CJ, jxb0 = cx * p.CB;
    // fields, window rows and cells along jx of this chunk
    const int nf = min(p.CF, p.F - f0), nj = min(p.CJ, p.Wy - jy0), nb = min(p.CB, p.nxb - jxb0);
    const int npf = nj * nb, ncl = nf * npf;
    const int YC = p.YC, PS = (TY + p.CJ - 1) * YC, ny = p.CF * PS;   // a field's patch, the patches of the chunk

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lk = lane >> 4;   // operand lane: plane li (window column li of the cell) at k-slot lk
    const bool split = p.split != 0, square = p.power == 2;
    const int g0 = split ? wave : 0, gs = split ? kWaves : 1;   // the steps of four pixels this wave takes

    Acc acc[kCellsPerWave];
    int boff[kCellsPerWave];   // where cell j of this wave starts in the patches: its field, its window row, its first column
    int nv = 0;                // the cells of this wave: the first nv accumulators (uniform over the wave)
#pragma unroll
    for (int j = 0; j < kCellsPerWave; ++j) {
        acc[j] = Acc(0.0);
        const int l = split ? j : wave + kWaves * j, fl = l / npf, rem = l - fl * npf;
        boff[j] = l < ncl ? fl * PS + rem / nb * YC + rem % nb * kTrigBlock : 0;
        nv += l < ncl ? 1 : 0;
    }

    // item `it` of the segment: its sample and the corner of its tile
    auto locate = [&](long long it, int &n, int &y0, int &x0) {
        const long long item = (long long)seg * p.seglen + it;
        n = (int)(item / p.tiles);
        const int tile = (int)(item - (long long)n * p.tiles);
        const int tyi = tile / p.tiles_x;
        y0 = tyi * TY, x0 = (tile - tyi * p.tiles_x) * TX;
    };
    // the register stage: wave w holds the staged rows w, w + 4, ... of H, thread t the elements t, t + 256, ... of the
    // patches of Y; whatever lies outside the plane or the sample is a zero and is not read
    T pa[ROWS][NA], py[NY];
    int ycode[NY];   // where element k of this thread lies: field << 16 | row of the patch << 10 | column; -1: no element
#pragma unroll
    for (int k = 0; k < NY; ++k) {
        const int e = tid + kTrigThreads * k, fl = e / PS, r2 = e - fl * PS, ry = r2 / YC;
        ycode[k] = (e < ny && fl < nf) ? fl << 16 | ry << 10 | (r2 - ry * YC) : -1;
    }
    auto fetch = [&](long long it) {
        int n, y0, x0;
        locate(it, n, y0, x0);
        const T *Hn = H + (size_t)n * p.P * p.Sy * p.Hs;
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const int rp = wave + kWaves * k, r = rp / kTrigBlock, plane = pb * kTrigBlock + rp - r * kTrigBlock;
            const bool row_in = plane < p.P && y0 + r < p.Sy;
            const T *h = Hn + (row_in ? ((size_t)plane * p.Sy + y0 + r) * p.Hs : 0);
#pragma unroll
            for (int c = 0; c < NA; ++c) {
                const int x = x0 + c * 64 + lane;
                pa[k][c] = (row_in && x < p.Sx) ? h[x] : T(0);
            }
        }
        const T *Yn = Y + ((size_t)n * p.F + f0) * p.Dy * p.Dx;
        const long long ybase = (long long)y0 + p.offy + jy0, xbase = (long long)x0 + p.offx + jxb0 * kTrigBlock;
#pragma unroll
        for (int k = 0; k < NY; ++k) {
            if (kTrigThreads * k >= ny) break;   // (uniform over the workgroup: the patches of this plan end here)
            const int code = ycode[k];
            const long long yy = ybase + ((code >> 10) & 63), xx = xbase + (code & 1023);
            py[k] = (code >= 0 && yy >= 0 && yy < p.Dy && xx >= 0 && xx < p.Dx)
                        ? Yn[((size_t)(code >> 16) * p.Dy + yy) * p.Dx + xx] : T(0);
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
        }
#pragma unroll
        for (int k = 0; k < NY; ++k) {
            if (kTrigThreads * k >= ny) break;   // (uniform)
            if (tid + kTrigThreads * k < ny) Ys[tid + kTrigThreads * k] = py[k];
        }
        __syncthreads();
        if (it + 1 < i1) fetch(it + 1);   // in flight under the matrix work
        const int gn = (cn + 3) / 4;      // steps of four pixels along a row
        // the tile against the first NV cells of this wave, NV a constant: no branch between the reads and the MFMAs of a step
        auto contract = [&](auto count) {
            constexpr int NV = decltype(count)::value;
            for (int r = 0; r < rn; ++r) {
                const T *arow = As + (r * kTrigBlock + li) * SA + lk;
                const T *yrow = Ys + r * YC + lk + li;
                for (int gx = g0; gx < gn; gx += gs) {
                    double a = (double)arow[4 * gx];
                    a = square ? a * a : a;
                    double b[NV];
#pragma unroll
                    for (int j = 0; j < NV; ++j) b[j] = (double)yrow[4 * gx + boff[j]];
#pragma unroll
                    for (int j = 0; j < NV; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[j], acc[j], 0, 0, 0);
                }
            }
        };
        switch (nv) {   // (uniform over the wave; a wave without a cell only stages)
            case 1: contract(std::integral_constant<int, 1>{}); break;
            case 2: contract(std::integral_constant<int, 2>{}); break;
            case 3: contract(std::integral_constant<int, 3>{}); break;
            case 4: contract(std::integral_constant<int, 4>{}); break;
            case 5: contract(std::integral_constant<int, 5>{}); break;
            case 6: contract(std::integral_constant<int, 6>{}); break;
            case 7: contract(std::integral_constant<int, 7>{}); break;
            case 8: contract(std::integral_constant<int, 8>{}); break;
            default: break;
        }
    }

    if (split) {   // at most 3 cells, every wave a part of each: wave 0 adds them in wave order
        double *red = reinterpret_cast<double *>(smem_raw);
        for (int w = 1; w < kWaves; ++w) {
            __syncthreads();   // the tile, or the sums of wave w - 1, are done with
            if (wave == w) {
#pragma unroll
                for (int j = 0; j < kWaves - 1; ++j)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) red[(j * 4 + reg) * 64 + lane] = acc[j][reg];
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int j = 0; j < kWaves - 1; ++j)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) acc[j][reg] += red[(j * 4 + reg) * 64 + lane];
            }
        }
        if (wave != 0) return;
    }

    // accumulator register reg of lane (li, lk) is the sum of row (plane) lk + 4 reg, column (window column of the cell) li
    double *out = partials + (((size_t)seg * p.strips + strip) * p.nbp + pb) * p.cells * 256;
#pragma unroll
    for (int j = 0; j < kCellsPerWave; ++j) {
        const int l = split ? j : wave + kWaves * j;
        if (l >= ncl) continue;
        const int fl = l / npf, rem = l - fl * npf;
        const size_t cell = ((size_t)(f0 + fl) * p.Wy + jy0 + rem / nb) * p.nxb + jxb0 + rem % nb;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) out[cell * 256 + (lk + 4 * reg) * kTrigBlock + li] = acc[j][reg];
    }
}

// every element of X: the strips' sums in strip order
__global__ __launch_bounds__(kTrigThreads) void k_triggered_finalize(size_t total, TrigPlan p,
                                                                     const double *__restrict__ partials,
                                                                     double *__restrict__ X) {
    const size_t i = (size_t)blockIdx.x * kTrigThreads + threadIdx.x;
    if (i >= total) return;
    size_t rest = i;
    const int jx = (int)(rest % p.Wx);
    rest /= p.Wx;
    const int jy = (int)(rest % p.Wy);
    rest /= p.Wy;
    const int f = (int)(rest % p.F);
    rest /= p.F;
    const int pp = (int)(rest % p.P);
    const size_t seg = rest / p.P;
    const size_t cell = ((size_t)f * p.Wy + jy) * p.nxb + jx / kTrigBlock;
    const int e = pp % kTrigBlock * kTrigBlock + jx % kTrigBlock;
    const size_t stride = (size_t)p.nbp * p.cells * 256;
    const double *in = partials + seg * p.strips * stride + ((size_t)(pp / kTrigBlock) * p.cells + cell) * 256 + e;
    double sum = 0.0;
    for (int s = 0; s < p.strips; ++s) sum += in[(size_t)s * stride];
    X[i] = sum;
}

}  // namespace

int triggered_plan(int N, int P, int F, const int *D, const int *A, int Hs, int ndim, const int *margin, int power,
                   int per_sample, int dtype, TrigPlan *out) {
    TrigPlan p;
    if (F < 1 || (power != 1 && power != 2)) return TNMF_E_GEOM;
    for (int i = 0; i < ndim; ++i)
        if (margin[i] < 0) return TNMF_E_GEOM;
    const int limit = ndim == 2 ? kTrigMaxWindow2 : kTrigMaxWindow1;
    for (int i = 0; i < ndim; ++i)
        if ((long long)A[i] + 2LL * margin[i] > limit) return TNMF_E_UNSUPPORTED;
    const int Ay = ndim == 2 ? A[0] : 1, Ax = A[ndim - 1];
    const int my = ndim == 2 ? margin[0] : 0, mx = margin[ndim - 1];
    p.P = P, p.F = F, p.Hs = Hs, p.power = power;
    p.Dy = ndim == 2 ? D[0] : 1, p.Dx = D[ndim - 1];
    p.Sy = p.Dy + Ay - 1, p.Sx = p.Dx + Ax - 1;
    p.Wy = Ay + 2 * my, p.Wx = Ax + 2 * mx;
    p.offy = -(Ay - 1) - my, p.offx = -(Ax - 1) - mx;
    p.TY = ndim == 1 ? 1 : dtype == 0 ? kTrigTileYFloat : kTrigTileYDouble;
    p.TX = ndim == 2 ? kTrigTileX : dtype == 0 ? kTrigTile1Float : kTrigTile1Double;
    p.tiles_y = (int)(((long long)p.Sy + p.TY - 1) / p.TY);   // (an extent near 2^31: no overflow)
    p.tiles_x = (int)(((long long)p.Sx + p.TX - 1) / p.TX);
    if ((long long)p.tiles_y * p.tiles_x > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    p.tiles = p.tiles_y * p.tiles_x;
    p.nbp = cdiv(P, kTrigBlock);
    p.nxb = cdiv(p.Wx, kTrigBlock);
    if ((long long)F * p.Wy * p.nxb > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    p.cells = F * p.Wy * p.nxb;
    p.CB = std::min(p.nxb, kTrigChunk);
    p.CJ = std::min(p.Wy, kTrigChunk / p.CB);
    p.CJ = cdiv(p.Wy, cdiv(p.Wy, p.CJ));   // (as many chunks along jy, of even size)
    p.CF = std::min(F, kTrigChunk / (p.CB * p.CJ));
    p.YC = p.TX + kTrigBlock * p.CB;
    p.chunks_x = cdiv(p.nxb, p.CB);
    p.chunks_y = cdiv(p.Wy, p.CJ);
    p.chunks_f = cdiv(F, p.CF);
    if ((long long)p.chunks_f * p.chunks_y * p.chunks_x > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    p.chunks = p.chunks_f * p.chunks_y * p.chunks_x;
    p.split = p.CF * p.CJ * p.CB < kWaves ? 1 : 0;
    p.nseg = per_sample ? N : 1;
    p.seglen = per_sample ? (long long)p.tiles : (long long)N * p.tiles;
    // (sizes no memory holds, in double so that nothing below overflows: the outputs, the workgroups)
    const double outputs = (double)p.nseg * P * F * p.Wy * p.Wx;
    if (outputs >= 2147483648.0 || (double)p.nseg * p.nbp * p.chunks >= 2147483647.0) return TNMF_E_UNSUPPORTED;
    // strips: enough workgroups to fill the device, no more partial sums than kTrigPartialCap, at least one item each
    // (no sample: no item and, per sample, no segment -- one empty strip, nothing to divide by)
    const long long units = std::max<long long>(1, (long long)p.nseg * p.nbp * p.chunks);
    const long long want = (kTrigTargetGroups + units - 1) / units;
    const unsigned long long strip_bytes =
        std::max<unsigned long long>(1, (unsigned long long)p.nseg * p.nbp * p.cells * 256 * sizeof(double));
    const long long cap = std::max<long long>(1, (long long)(kTrigPartialCap / strip_bytes));
    const long long strips = std::max<long long>(1, std::min(std::min(want, cap), p.seglen));
    p.ipg = std::max<long long>(1, (p.seglen + strips - 1) / strips);
    p.strips = (int)std::max<long long>(1, (p.seglen + p.ipg - 1) / p.ipg);   // (no strip without an item)
    if (units * p.strips > 0x7fffffffLL) return TNMF_E_UNSUPPORTED;
    p.lds = ((size_t)p.TY * kTrigBlock * (p.TX + kTrigPad) + (size_t)p.CF * (p.TY + p.CJ - 1) * p.YC) * esize(dtype);
    if (p.lds > 64 * 1024) return TNMF_E_UNSUPPORTED;   // (no plan of today's constants: the kernel's static_asserts bound it)
    *out = p;
    return TNMF_OK;
}

size_t triggered_partial_bytes(const TrigPlan &p) {
    return align_up((size_t)p.nseg * p.strips * p.nbp * p.cells * 256 * sizeof(double), 256);
}

int launch_triggered(const TrigPlan &p, int dtype, const void *H, const void *Y, double *partials, double *X_out,
                     hipStream_t s) {
    const unsigned blocks = (unsigned)((size_t)p.nseg * p.strips * p.nbp * p.chunks);
    with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        constexpr bool f = sizeof(T) == sizeof(float);
        constexpr int T1 = f ? kTrigTile1Float : kTrigTile1Double, TY2 = f ? kTrigTileYFloat : kTrigTileYDouble;
        if (p.TY == 1)   // (one shift axis)
            hipLaunchKernelGGL((k_triggered<T, 1, T1>), dim3(blocks), dim3(kTrigThreads), p.lds, s, p, (const T *)H,
                               (const T *)Y, partials);
        else
            hipLaunchKernelGGL((k_triggered<T, TY2, kTrigTileX>), dim3(blocks), dim3(kTrigThreads), p.lds, s, p,
                               (const T *)H, (const T *)Y, partials);
    });
    TNMF_LAUNCH_CHECK();
    const size_t total = (size_t)p.nseg * p.P * p.F * p.Wy * p.Wx;
    hipLaunchKernelGGL(k_triggered_finalize, dim3((unsigned)((total + kTrigThreads - 1) / kTrigThreads)),
                       dim3(kTrigThreads), 0, s, total, p, (const double *)partials, X_out);
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}
