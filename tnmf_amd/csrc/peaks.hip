// peaks.hip -- detections: the entries of H above a threshold that no competitor of their neighbourhood suppresses
// (include/tnmf_hip.h, tnmf_hip_find_peaks), compacted into a list on the device.
//
// One pass over H.  A workgroup of four waves owns 16 consecutive rows of one plane, a wave four of them, and walks
// them in tiles of 64 columns: plane, row and column come from the launch geometry and loop counters, there is no
// division on the way.  A wave loads its four tiles before it looks at any.  Most tiles end at the ballot of
// `h > threshold`: a fitted H is sparse there.  What is left is thinned in registers first -- an entry whose left, right,
// upper or lower neighbour (a lane shuffle, the neighbouring row's register) suppresses it is no detection, whatever else
// the window holds; activations come as blobs, so this removes most of them without a memory access.  Each survivor is
// then checked by the WHOLE wave: its window (every plane of its suppression group x the clipped box of the radius) is
// walked in slabs of 64 entries, lanes along x first and, for windows narrower than 64, over several window rows at
// once, the candidate's own row first and outwards from it; four slabs are loaded before one ballot says whether any of
// their entries suppresses the candidate, and the walk ends at the first that does.  The survivors of a tile take their
// slots with one atomicAdd per wave.
//
// Two forms of the window walk: the plain one above reads the window from global memory (mostly L2: neighbouring tiles
// stream the same lines) and is what the product runs.  The tiled one (two shift axes, group 1, a halo that fits) stages
// the workgroup's 16 x 64 entries with their halo of `radius` in LDS once per tile, with a bitmap of the entries above the
// threshold, and visits only those (examine_tile); it was built because the plain form stays far below the streaming
// rate, measured slower still, and is compiled into the launch only with -DTNMF_PEAKS_TILED.
#include <math.h>

#include <algorithm>

#include "peaks.h"

namespace {

constexpr int kWaves = 4;         // waves per workgroup
constexpr int kRowsPerWave = 4;   // rows a wave loads before it examines them
constexpr int kBlockRows = kWaves * kRowsPerWave;
constexpr int kSlabBatch = 4;     // slabs of a window in flight before the ballot
constexpr size_t kMaxTileBytes = 48 << 10;

struct Window {
    int lw;   // log2 of the lanes along x in a slab: 64 >> lw window rows per slab
};

// the window of a candidate read from global memory: Hg = the first plane of its suppression group
template <typename T>
struct GlobalWindow {
    const T *Hg;
    int Sz, Sy, Hs;
    __device__ __forceinline__ T at(int qi, int zz, int yy, int xx) const {
        return Hg[(((size_t)qi * Sz + zz) * Sy + yy) * Hs + xx];
    }
};

// The tiled form's walk (one plane of two shift axes, group 1).  The workgroup's LDS holds its 16 x 64 entries with their
// halo (`tile`, rows of `pitch` entries from plane row ty0 and column tx0, zeros outside the plane) and one bit per entry
// that says `entry > threshold` (`bits`, nw 64-bit words per tile row).  Only such entries can suppress a candidate, so
// each lane takes one row of the candidate's window, cuts that row's words to the window's columns and visits the set
// bits alone -- about one per row in a fitted H; one ballot per candidate.
template <typename T>
__device__ bool examine_tile(const PeakGeo &g, const T *tile, const unsigned long long *bits, int pitch, int nw, int ty0,
                             int tx0, int y, int xb, T h, unsigned long long m) {
    const int lane = threadIdx.x & 63;
    const int ty_c = y - ty0;
    const int ty_lo = max(y - g.ry, 0) - ty0, n_rows = min(y + g.ry, g.Sy - 1) - ty0 - ty_lo + 1;
    bool peak = false;
    while (m) {
        const int c = __ffsll((long long)m) - 1;
        m &= m - 1;
        const T hc = __shfl(h, c, 64);
        const int xc = xb + c, tx_c = xc - tx0;
        const int tx_lo = max(xc - g.rx, 0) - tx0, tx_hi = min(xc + g.rx, g.Sx - 1) - tx0;
        bool s = false;
        for (int rr = lane; rr < n_rows; rr += 64) {
            const int ty = ty_lo + rr;
            for (int k = tx_lo >> 6; k <= tx_hi >> 6; ++k) {
                const int lo = max(tx_lo - k * 64, 0), hi = min(tx_hi - k * 64, 63);
                unsigned long long b = bits[ty * nw + k] & (~0ull << lo) & (~0ull >> (63 - hi));
                while (b) {
                    const int tx = k * 64 + __ffsll((long long)b) - 1;
                    b &= b - 1;
                    const T v = tile[ty * pitch + tx];
                    s |= v > hc || (v == hc && (ty < ty_c || (ty == ty_c && tx < tx_c)));
                }
            }
        }
        if (!__ballot(s) && lane == c) peak = true;
    }
    return peak;
}

// The candidates `m` (a ballot) of the tile at plane qc of its group, rows (z, y), columns xb .. xb + 63; h: this lane's
// entry.  Returns whether this lane's entry is a detection.  Wave-uniform control flow throughout.
// An entry (value v, row key kk, column xx) suppresses the candidate (hc, kc, xc) when it is larger, or equal with the
// lower flat index -- the row key orders everything in front of the last axis.  NaN compares false.
template <typename T>
__device__ bool examine(const PeakGeo &g, const Window &w, const GlobalWindow<T> &win, int qc, int z, int y, int xb, T h,
                        unsigned long long m) {
    const int lane = threadIdx.x & 63;
    const int wpad = 1 << w.lw, rpi = 64 >> w.lw;
    const int sub = lane >> w.lw, dx = lane & (wpad - 1);
    const int z0 = max(z - g.rz, 0), z1 = min(z + g.rz, g.Sz - 1);
    const int y0 = max(y - g.ry, 0), y1 = min(y + g.ry, g.Sy - 1);
    const int below = y1 - y, n_rows = y1 - y0 + 1;   // window rows in the order y, y + 1, .. y1, y - 1, .. y0
    const long long kc = ((long long)qc * g.Sz + z) * g.Sy + y;
    bool peak = false;
    while (m) {
        const int c = __ffsll((long long)m) - 1;
        m &= m - 1;
        const T hc = __shfl(h, c, 64);
        const int xc = xb + c;
        const int x0 = max(xc - g.rx, 0), x1 = min(xc + g.rx, g.Sx - 1);
        bool suppressed = false;
        for (int qq = 0; qq < g.group && !suppressed; ++qq) {   // the candidate's own plane first
            const int qi = qc + qq < g.group ? qc + qq : qc + qq - g.group;
            for (int zz = z0; zz <= z1 && !suppressed; ++zz) {
                const long long k0 = ((long long)qi * g.Sz + zz) * g.Sy;
                for (int xs = x0; xs <= x1 && !suppressed; xs += wpad) {
                    const int xx = xs + dx;
                    for (int j0 = 0; j0 < n_rows; j0 += kSlabBatch * rpi) {
                        T v[kSlabBatch];
                        int yy[kSlabBatch];
                        bool in[kSlabBatch];
#pragma unroll
                        for (int b = 0; b < kSlabBatch; ++b) {
                            const int j = j0 + b * rpi + sub;
                            yy[b] = j <= below ? y + j : y - (j - below);
                            in[b] = j < n_rows && xx <= x1;   // (inside the clipped box: inside the plane)
                            v[b] = in[b] ? win.at(qi, zz, yy[b], xx) : (T)0;
                        }
                        bool s = false;
#pragma unroll
                        for (int b = 0; b < kSlabBatch; ++b) {
                            const long long kk = k0 + yy[b];
                            s |= in[b] && (v[b] > hc || (v[b] == hc && (kk < kc || (kk == kc && xx < xc))));
                        }
                        if (__ballot(s)) {
                            suppressed = true;
                            break;
                        }
                    }
                }
            }
        }
        if (!suppressed && lane == c) peak = true;
    }
    return peak;
}

template <typename T, bool kTiled>
__global__ __launch_bounds__(kWaves * 64) void k_find_peaks(PeakGeo g, Window w, const T *__restrict__ H, T thr,
                                                            long long *__restrict__ idx, T *__restrict__ val,
                                                            unsigned long long capacity, unsigned long long *count) {
    extern __shared__ __align__(16) unsigned char peaks_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rpp = g.Sz * g.Sy;   // rows per plane
    const int pitch = 64 + 2 * g.rx, nw = (pitch + 63) >> 6, tile_rows = kBlockRows + 2 * g.ry;
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(peaks_lds);   // [tile_rows][nw], then the tile
    T *tile = reinterpret_cast<T *>(bits + tile_rows * nw);
    for (long long plane = blockIdx.y; plane < g.planes; plane += gridDim.y) {
        const T *Hp = H + (size_t)plane * rpp * g.Hs;
        int qc = 0;   // the plane's place in its suppression group
        if (g.group > 1) qc = (int)(plane % g.P) % g.group;
        for (int rb = blockIdx.x * kBlockRows; rb < rpp; rb += gridDim.x * kBlockRows) {
            const int rp0 = rb + wave * kRowsPerWave;
            for (int xb = 0; xb < g.Sx; xb += 64) {
                const int x = xb + lane;
                T h[kRowsPerWave];
                const int ty0 = rb - g.ry, tx0 = xb - g.rx;
                if (kTiled) {
                    // rows rb - ry .. rb + 15 + ry, columns xb - rx .. xb + 63 + rx; zeros (never above a threshold >= 0)
                    // where they leave the plane
                    __syncthreads();   // (the previous tile's windows have been walked)
                    for (int ty = wave; ty < tile_rows; ty += kWaves) {
                        const int yy = ty0 + ty;
                        for (int k = 0; k < nw; ++k) {
                            const int tx = k * 64 + lane, xx = tx0 + tx;
                            const bool in = tx < pitch && yy >= 0 && yy < g.Sy && xx >= 0 && xx < g.Sx;
                            const T v = in ? Hp[(size_t)yy * g.Hs + xx] : (T)0;
                            if (tx < pitch) tile[ty * pitch + tx] = v;
                            const unsigned long long above = __ballot(v > thr);
                            if (lane == 0) bits[ty * nw + k] = above;
                        }
                    }
                    __syncthreads();
#pragma unroll
                    for (int u = 0; u < kRowsPerWave; ++u)   // (0 is never above a threshold >= 0)
                        h[u] = (rp0 + u < rpp && x < g.Sx) ? tile[(rp0 + u - ty0) * pitch + g.rx + lane] : (T)0;
                } else {
#pragma unroll
                    for (int u = 0; u < kRowsPerWave; ++u)
                        h[u] = (rp0 + u < rpp && x < g.Sx) ? Hp[(size_t)(rp0 + u) * g.Hs + x] : (T)0;
                }
#pragma unroll
                for (int u = 0; u < kRowsPerWave; ++u) {
                    bool cand = h[u] > thr;
                    if (!__ballot(cand)) continue;
                    // neighbours at hand: the lower flat index suppresses on a tie (left, up), the higher only when larger
                    if (g.rx >= 1) {
                        const T left = __shfl_up(h[u], 1, 64), right = __shfl_down(h[u], 1, 64);
                        if ((lane > 0 && left >= h[u]) || (lane < 63 && right > h[u])) cand = false;
                    }
                    if (g.ry >= 1 && g.Sz == 1) {   // (one plane of two axes: the wave's rows are neighbours in y)
                        const T up = h[u > 0 ? u - 1 : u], down = h[u + 1 < kRowsPerWave ? u + 1 : u];
                        if ((u > 0 && up >= h[u]) || (u + 1 < kRowsPerWave && down > h[u])) cand = false;
                    }
                    const unsigned long long m = __ballot(cand);
                    if (!m) continue;
                    const int rp = rp0 + u;
                    int z = 0, y = rp;
                    if (g.Sz > 1) z = rp / g.Sy, y = rp - z * g.Sy;
                    bool peak;
                    if (kTiled) {
                        peak = examine_tile<T>(g, tile, bits, pitch, nw, ty0, tx0, y, xb, h[u], m);
                    } else {
                        const GlobalWindow<T> win = {Hp - (size_t)qc * rpp * g.Hs, g.Sz, g.Sy, g.Hs};
                        peak = examine<T>(g, w, win, qc, z, y, xb, h[u], m);
                    }
                    const unsigned long long pm = __ballot(peak);
                    if (!pm) continue;
                    unsigned long long base = 0;
                    if (lane == 0) base = atomicAdd(count, (unsigned long long)__popcll(pm));
                    base = __shfl(base, 0, 64);
                    if (peak) {
                        const unsigned long long slot = base + __popcll(pm & ((1ull << lane) - 1ull));
                        if (slot < capacity) {
                            idx[slot] = (plane * rpp + rp) * g.Sx + x;
                            val[slot] = h[u];
                        }
                    }
                }
            }
        }
    }
}

// the largest T not above t: for every T h, h > t exactly when h > floor_to<T>(t)
template <typename T>
T floor_to(double t);
template <>
double floor_to<double>(double t) { return t; }
template <>
float floor_to<float>(double t) {
    float f = (float)t;
    if ((double)f > t) f = nextafterf(f, -INFINITY);
    return f;
}

template <typename T>
void launch(const tnmf_hip_ctx *ctx, const PeakGeo &g_in, const void *H, double threshold, long long *idx, void *val,
            size_t capacity, unsigned long long *count, hipStream_t s) {
    Window w;
    const int width = std::min(2 * g_in.rx + 1, g_in.Sx);
    w.lw = 0;
    while (w.lw < 6 && (1 << w.lw) < width) ++w.lw;
    PeakGeo g = g_in;
    // the tiled form: one plane of two shift axes per window, a real halo, and a tile that fits
    const size_t tile_bytes = (size_t)(kBlockRows + 2 * g.ry) * ((64 + 2 * g.rx) * sizeof(T) + (64 + 2 * g.rx + 63) / 64 * 8);
#ifdef TNMF_PEAKS_TILED   // (an A/B flavour of the library for tools/probes/peaks_bench.py: make VARIANT=peakstiled ...)
    const bool tiled = g.Sz == 1 && g.Sy > 1 && g.group == 1 && (g.rx > 0 || g.ry > 0) && tile_bytes <= kMaxTileBytes;
#else   // measured slower than the plain walk, on a fitted H and on a dense one: the product does not use it
    const bool tiled = false && tile_bytes <= kMaxTileBytes;
#endif
    // one shift axis, every plane for itself: the planes are the rows of ONE plane whose windows never leave their row
    // (ry = 0) -- sixteen signals per workgroup instead of one
    if (g.Sz == 1 && g.Sy == 1 && g.group == 1 && g.planes <= 0x7fffffffLL) {
        g.Sy = (int)g.planes;
        g.planes = 1;
    }
    const int rpp = g.Sz * g.Sy;
    const unsigned gx = (unsigned)std::min((rpp + kBlockRows - 1) / kBlockRows, 1024);
    const long long budget = std::max<long long>(1, (long long)ctx->num_cu * 64 / gx);
    const unsigned gy = (unsigned)std::max<long long>(1, std::min<long long>(std::min<long long>(g.planes, budget), 65535));
    if (tiled)
        hipLaunchKernelGGL((k_find_peaks<T, true>), dim3(gx, gy), dim3(kWaves * 64), tile_bytes, s, g, w, (const T *)H,
                           floor_to<T>(threshold), idx, (T *)val, (unsigned long long)capacity, count);
    else
        hipLaunchKernelGGL((k_find_peaks<T, false>), dim3(gx, gy), dim3(kWaves * 64), 0, s, g, w, (const T *)H,
                           floor_to<T>(threshold), idx, (T *)val, (unsigned long long)capacity, count);
}

}  // namespace

int peaks_find(tnmf_hip_ctx *ctx, const PeakGeo &g, int dtype, const void *H, double threshold, long long *idx,
               void *val, size_t capacity, unsigned long long *count, hipStream_t s) {
    TNMF_HIP_TRY(hipMemsetAsync(count, 0, sizeof(unsigned long long), s));
    if (g.planes <= 0) return TNMF_OK;
    with_dtype(dtype, [&](auto zero) { launch<decltype(zero)>(ctx, g, H, threshold, idx, val, capacity, count, s); });
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}
