// fft_mixed.hip -- "mixed" contractions of the FFT family: transform along x only, the few taps along y directly.
//
// After the row transforms an atom is only Ay rows tall, so the contraction over (atom, atom row) costs Ay complex
// multiply-adds per row-spectrum entry -- fewer issue slots than the column transform it replaces (two LDS round trips
// per radix stage) as long as C*Ay stays small -- and needs no LDS and no barrier at all:
//
//   reconstruct   OT[n,c,y,kx]  = sum_m sum_a T[n,m,y+a,kx] * WT[m,c,Ay-1-a,kx]          (then C2R along x, crop)
//   W gradient    GT[m,c,a,kx]  = sum_n sum_y T[n,m,y+a,kx] * conj(VT[n,c,y,kx])        (then C2R along x, crop, flip)
//
// T, VT, WT = row spectra (fft_kernels.h).  Same mathematics as NumPy.py:122-132 / 69-91 of the reference with the
// x axis in the frequency domain.  Lanes run along kx (coalesced 128-byte segments), everything else is registers.
#include "fft.h"

namespace {

// float only: a complex value is one 64-bit register pair and every complex multiply-add is two packed FMAs whose
// operand broadcasts, swaps and sign flips ride on the op_sel / neg modifiers (left to itself hipcc materialises the
// broadcast and swapped operand pairs in extra registers: 300-400 VGPRs for these kernels instead of ~130).
//   D.lo = A[op_sel[0]] * B[op_sel[1]] + C[op_sel[2]],  D.hi likewise with op_sel_hi
typedef float f2v __attribute__((ext_vector_type(2)));
template <typename T>
struct cplx_of;
template <>
struct cplx_of<float> {
    using type = f2v;
};
template <typename T>
using cplx = typename cplx_of<T>::type;

// acc += a * b
__device__ __forceinline__ void cfma(f2v &acc, f2v a, f2v b) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(a), "v"(b));
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]" : "+v"(acc) : "v"(a), "v"(b));
}
// acc += a * conj(b)
__device__ __forceinline__ void cfmac(f2v &acc, f2v a, f2v b) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1] neg_hi:[0,1,0]" : "+v"(acc) : "v"(a), "v"(b));
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(a), "v"(b));
}
// acc += x * s, both halves of x (two streams) by the same scalar: s = b.lo / s = b.hi
__device__ __forceinline__ void pfma_lo(f2v &acc, f2v x, f2v b) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(x), "v"(b));
}
__device__ __forceinline__ void pfma_hi(f2v &acc, f2v x, f2v b) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(x), "v"(b));
}

#define CHECK(rc_expr)                  \
    do {                                \
        const int _rc = (rc_expr);      \
        if (_rc != TNMF_OK) return _rc; \
    } while (0)

constexpr int kMixCols = 16;   // kx per block row group: 16 lanes x 8 bytes = one 128-byte segment

// ---- reconstruct ---------------------------------------------------------------------------------------------------
// block = 16 kx x STRIPS strips of S output rows; a thread keeps S outputs per channel in registers and, per atom, the
// S+AY-1 row-spectrum entries they depend on.  grid (kx tiles, row blocks, samples)
template <typename T, int AY, int CG, int S, int STRIPS>
__global__ __launch_bounds__(kMixCols *STRIPS, 2) void k_mix_reconstruct(const cplx<T> *Tsp, const cplx<T> *WT,
                                                                      cplx<T> *OT, int M, int C, int Hy, int Dy, int KX,
                                                                      int KXP) {
    const int col = threadIdx.x & (kMixCols - 1), strip = threadIdx.x / kMixCols;
    const int kx = blockIdx.x * kMixCols + col, kxc = min(kx, KX - 1);
    const int y0 = (blockIdx.y * STRIPS + strip) * S, n = blockIdx.z;
    cplx<T> acc[CG][S];
#pragma unroll
    for (int c = 0; c < CG; ++c)
#pragma unroll
        for (int y = 0; y < S; ++y) acc[c][y] = {0, 0};
    // Addresses: a buffer descriptor per plane (wave-uniform, scalar registers), a scalar row offset, and ONE per-lane
    // byte offset (first row of the strip, kx) that never changes -- no vector address arithmetic and no offset
    // registers.  Rows past the plane (y0 + r >= Hy) are read only under outputs that are never stored (output row y needs
    // rows up to y + AY - 1 <= Hy - 1 whenever y < Dy).  The descriptor's range check does NOT catch them -- on gfx9 raw
    // buffers it covers the vector offset only, not the scalar one -- so they come from the next plane or, behind the last
    // plane, from the slack rows the workspace layout keeps after T (fft.hip: make_layout); whatever they hold only
    // reaches accumulators that are dropped.  The rows of the next atom are fetched while the current ones are multiplied.
    static_assert(sizeof(cplx<T>) == 8, "float spectra");
    typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
    auto ld = [](const __amdgpu_buffer_rsrc_t &rs, int lane_off, int row_off) {
        const u32x2v w2 = __builtin_amdgcn_raw_buffer_load_b64(rs, lane_off, row_off, 0);
        const unsigned re = w2[0], im = w2[1];   // (bit_cast straight on a vector element reads element 0: hipcc 7.2)
        return cplx<T>{__builtin_bit_cast(float, re), __builtin_bit_cast(float, im)};
    };
    const int rowb = KXP * 8;
    const long tplane = (long)Hy * KXP, wplane = (long)AY * KXP;
    const int lane_t = (y0 * KXP + kxc) * 8, lane_w = kxc * 8;
    const __amdgpu_buffer_rsrc_t wrs =
        __builtin_amdgcn_make_buffer_rsrc((void *)WT, 0, (int)((long)M * C * wplane * 8), 0x00020000);
    auto plane = [&](int m) {
        return __builtin_amdgcn_make_buffer_rsrc((void *)(Tsp + ((long)n * M + m) * tplane), 0, (int)(tplane * 8),
                                                 0x00020000);
    };
    cplx<T> t[S + AY - 1], tn[S + AY - 1];
    {
        const __amdgpu_buffer_rsrc_t rs = plane(0);
#pragma unroll
        for (int r = 0; r < S + AY - 1; ++r) t[r] = ld(rs, lane_t, r * rowb);
    }
    if constexpr (CG == 1) {
        // One channel: the AY rows of W spectra of an atom are the same for all STRIPS strips of the workgroup.  Loaded
        // per thread they were 12 of the 39 memory instructions of an atom step and -- although they hit in L2 -- a
        // fifth of the kernel (measured with constants in their place: 0.69 -> 0.575 ms).  They are staged through LDS in
        // chunks of MC atoms: 16-byte loads one chunk ahead (in flight under the atoms of the current chunk), one
        // barrier per chunk, and an atom step reads its rows with AY ds_read_b64 (all strips of a wave read the same
        // addresses: a broadcast).
        constexpr int MC = 8, NT = kMixCols * STRIPS, ROWS = MC * AY, PIECES = ROWS * (kMixCols / 2);
        constexpr int NPP = (PIECES + NT - 1) / NT;
        typedef float f4v __attribute__((ext_vector_type(4)));
        __shared__ __align__(16) cplx<T> wl[2][ROWS * kMixCols];
        const cplx<T> *wsrc = WT + blockIdx.x * kMixCols;   // (KXP is a multiple of 16 entries: whole 128-byte segments)
        const int wrows = M * AY;
        f4v pre[NPP];
        auto wfetch = [&](int chunk) {
#pragma unroll
            for (int k = 0; k < NPP; ++k) {
                const int p = threadIdx.x + k * NT, row = min(chunk * ROWS + (p >> 3), wrows - 1);
                pre[k] = *reinterpret_cast<const f4v *>(wsrc + (long)row * KXP + 2 * (p & 7));
            }
        };
        auto wpark = [&](int buf) {
#pragma unroll
            for (int k = 0; k < NPP; ++k) {
                const int p = threadIdx.x + k * NT;
                if (p < PIECES) *reinterpret_cast<f4v *>(&wl[buf][(p >> 3) * kMixCols + 2 * (p & 7)]) = pre[k];
            }
        };
        wfetch(0);
        wpark(0);
        __syncthreads();
#pragma unroll 1
        for (int m0 = 0, ch = 0; m0 < M; m0 += MC, ++ch) {
            const int buf = ch & 1;
            const bool more = m0 + MC < M;
            if (more) wfetch(ch + 1);
#pragma unroll 1
            for (int mi = 0; mi < MC; ++mi) {
                const int m = m0 + mi;
                if (m >= M) break;
                cplx<T> w[AY];
#pragma unroll
                for (int a = 0; a < AY; ++a) w[a] = wl[buf][(mi * AY + (AY - 1 - a)) * kMixCols + col];
                {
                    const __amdgpu_buffer_rsrc_t rs = plane(min(m + 1, M - 1));
#pragma unroll
                    for (int r = 0; r < S + AY - 1; ++r) tn[r] = ld(rs, lane_t, r * rowb);
                }
#pragma unroll
                for (int a = 0; a < AY; ++a)
#pragma unroll
                    for (int y = 0; y < S; ++y) cfma(acc[0][y], t[y + a], w[a]);
#pragma unroll
                for (int r = 0; r < S + AY - 1; ++r) t[r] = tn[r];
            }
            if (more) wpark(buf ^ 1);
            __syncthreads();
        }
    } else {
#pragma unroll 1
    for (int m = 0; m < M; ++m) {
        cplx<T> w[CG][AY];
#pragma unroll
        for (int c = 0; c < CG; ++c) {
            const int wbase = ((m * C + min(c, C - 1)) * AY) * rowb;
#pragma unroll
            for (int a = 0; a < AY; ++a) w[c][a] = ld(wrs, lane_w, wbase + (AY - 1 - a) * rowb);
        }
        {
            const __amdgpu_buffer_rsrc_t rs = plane(min(m + 1, M - 1));
#pragma unroll
            for (int r = 0; r < S + AY - 1; ++r) tn[r] = ld(rs, lane_t, r * rowb);
        }
#pragma unroll
        for (int c = 0; c < CG; ++c)
#pragma unroll
            for (int a = 0; a < AY; ++a)
#pragma unroll
                for (int y = 0; y < S; ++y) cfma(acc[c][y], t[y + a], w[c][a]);
#pragma unroll
        for (int r = 0; r < S + AY - 1; ++r) t[r] = tn[r];
    }
    }
    if (kx >= KX) return;
#pragma unroll
    for (int c = 0; c < CG; ++c) {
        if (c >= C) break;
#pragma unroll
        for (int y = 0; y < S; ++y)
            if (y0 + y < Dy) OT[((long)n * C + c) * ((long)Dy * KXP) + (long)(y0 + y) * KXP + kx] = acc[c][y];
    }
}

// Kernels that read their operands from LDS one ds_read_b64 at a time are compiled (device pass) without hipcc's pairing
// of DS accesses: a ds_read2_b64 / ds_read2st64_b64 moves half the bytes per LDS clock.
#if defined(__HIP_DEVICE_COMPILE__)
#define TNMF_MIX_NO_DS_PAIRING __attribute__((target("no-load-store-opt")))
#else
#define TNMF_MIX_NO_DS_PAIRING
#endif

// Large one-channel 2-D calls (mixed_reconstruct_sh_takes): the arithmetic of k_mix_reconstruct<T, AY, 1, 16, 8>, the same
// packed multiply-adds on the same values in the same order per output -- bit-identical results -- with the row spectra
// staged through LDS.  There a thread loads the S + AY - 1 rows its strip depends on itself, and since neighbouring strips
// overlap by AY - 1 rows every entry of T is asked for (S + AY - 1) / S = 1.69 times (AY = 12) by 8-byte loads.  Here the
// workgroup -- 16 kx x STRIPS strips -- loads the S * STRIPS + AY - 1 rows of its tile ONCE per atom, 16 bytes per lane
// (eight lanes per 128-byte row segment), together with the AY rows of W spectra of that atom, one atom ahead: the loads of
// atom m + 1 are in flight, in registers, under the multiply-adds of atom m, and are written to LDS behind them.  With
// TILES = 2 they go to the other tile (its readers passed the barrier of the previous atom step): one barrier per atom;
// with TILES = 1 a barrier before and one after the write.  A thread then takes its rows with S + AY - 1 ds_read_b64 and
// the atom rows with AY broadcast ds_read_b64.  The tile's row pitch is 17 entries (136 bytes): the two strips of a
// 32-lane half are 16 tile rows apart, 16 * 136 bytes = 8 * 256 + 128, so they fall into different halves of the 256-byte
// bank row (a pitch of 128 bytes puts them on the same banks: a two-way conflict on every read).
// Addresses: a wave-uniform buffer descriptor per plane of T (and per atom of W spectra) and ONE constant per-lane byte
// offset per piece, row index clamped to the plane: rows past the plane are needed only by outputs that are never
// stored, so nothing beyond a plane is read (the slack rows behind T are not touched by this kernel); the padding
// columns KX .. KXP - 1 of a row segment are loaded like any other (KXP is whole segments), a thread reads column
// min(kx, KX - 1).  The loads of T carry the non-temporal hint (kMixRShAux): an entry is used once per launch, and keeping
// it out of the way of the W spectra in L2 measured 3 % of the kernel.  grid (kx tiles, row blocks of S * STRIPS, samples)
template <typename T, int AY, int STRIPS, int TILES>
__global__ __launch_bounds__(kMixCols *STRIPS, kMixRShWaves) TNMF_MIX_NO_DS_PAIRING void k_mix_reconstruct_sh(
    const cplx<T> *Tsp, const cplx<T> *WT, cplx<T> *OT, int M, int Hy, int Dy, int KX, int KXP) {
    constexpr int S = 16, NT = kMixCols * STRIPS, ROWS = S * STRIPS + AY - 1, PITCH = kMixCols + 1;
    constexpr int SEG = kMixCols / 2;                                    // 16-byte pieces per row segment
    constexpr int PIECES = ROWS * SEG, NPP = (PIECES + NT - 1) / NT, WPIECES = AY * SEG;
    constexpr int TROWS = (ROWS * PITCH + 1) / 2 * 2, TILE = TROWS + AY * kMixCols;   // entries: rows of T, rows of W
    static_assert(sizeof(cplx<T>) == 8 && WPIECES <= NT && (TILES == 1 || TILES == 2), "float spectra, one W piece per thread");
    static_assert(STRIPS != kMixRShStrips || TILES != kMixRShTiles || TILES * TILE * 8 == mix_rsh_lds_bytes(AY), "fft.h");
    typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
    typedef float f4v __attribute__((ext_vector_type(4)));
    __shared__ __align__(16) cplx<T> tile[TILES][TILE];
    const int col = threadIdx.x & (kMixCols - 1), strip = threadIdx.x / kMixCols;
    const int kx = blockIdx.x * kMixCols + col, colc = min(kx, KX - 1) - blockIdx.x * kMixCols;
    const int yb = blockIdx.y * (S * STRIPS), y0 = yb + strip * S, n = blockIdx.z;
    cplx<T> acc[S];
#pragma unroll
    for (int y = 0; y < S; ++y) acc[y] = {0, 0};
    const long tplane = (long)Hy * KXP, wplane = (long)AY * KXP;
    // loader: piece p = (tile row p / 8, kx pair p % 8); the host checks that a plane's bytes fit 31 bits.  Pieces past
    // the tile (and past the atom's rows) repeat the last row's: the same bytes to the same place, so that neither a load
    // nor a write sits in a branch (hipcc sinks a load into the branch of its only use and waits for it there)
    auto trow = [](int k) { return min((int)(threadIdx.x + k * NT) / SEG, ROWS - 1); };
    const int pcol = (blockIdx.x * kMixCols + 2 * (threadIdx.x & (SEG - 1))) * 8;
    int toff[NPP];
#pragma unroll
    for (int k = 0; k < NPP; ++k) toff[k] = min(yb + trow(k), Hy - 1) * (KXP * 8) + pcol;
    const int wrow = min((int)threadIdx.x / SEG, AY - 1), woff = wrow * (KXP * 8) + pcol;
    f4v pre[NPP], wpre;
    auto fetch = [&](int m) {   // unconditional loads on clamped addresses
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(Tsp + ((long)n * M + m) * tplane), 0, (int)(tplane * 8), 0x00020000);
        const __amdgpu_buffer_rsrc_t ws =
            __builtin_amdgcn_make_buffer_rsrc((void *)(WT + m * wplane), 0, (int)(wplane * 8), 0x00020000);
#pragma unroll
        for (int k = 0; k < NPP; ++k)
            pre[k] = __builtin_bit_cast(f4v, (u32x4v)__builtin_amdgcn_raw_buffer_load_b128(rs, toff[k], 0, kMixRShAux));
        wpre = __builtin_bit_cast(f4v, (u32x4v)__builtin_amdgcn_raw_buffer_load_b128(ws, woff, 0, 0));
    };
    auto park = [&](int buf) {
        cplx<T> *tl = tile[buf];
#pragma unroll
        for (int k = 0; k < NPP; ++k) {
            const int e = trow(k) * PITCH + 2 * (threadIdx.x & (SEG - 1));   // (8-byte aligned: the pitch is odd)
            tl[e] = cplx<T>{pre[k][0], pre[k][1]};
            tl[e + 1] = cplx<T>{pre[k][2], pre[k][3]};
        }
        *reinterpret_cast<f4v *>(&tl[TROWS + wrow * kMixCols + 2 * (threadIdx.x & (SEG - 1))]) = wpre;
    };
    fetch(0);
    park(0);
    __syncthreads();
    const int mine = strip * S * PITCH + colc;
#pragma unroll 1
    for (int m = 0; m < M; ++m) {
        const int buf = TILES == 2 ? (m & 1) : 0;
        fetch(min(m + 1, M - 1));
        const cplx<T> *tl = &tile[buf][mine], *wl = &tile[buf][TROWS + colc];
        cplx<T> w[AY], t[S + AY - 1];
        // LDS reads in the order the multiply-adds want them.  kMixRShFence > 0 (an A/B flavour): nothing is scheduled
        // across a fence behind the first 16 + kMixRShFence rows, so those reads are issued before any multiply-add --
        // it pays only where registers are plentiful (two waves per SIMD); by default hipcc places each read itself
#pragma unroll
        for (int r = 0; r < S; ++r) t[r] = tl[r * PITCH];
        w[0] = wl[(AY - 1) * kMixCols];
#pragma unroll
        for (int a = 1; a < AY; ++a) {
            t[S - 1 + a] = tl[(S - 1 + a) * PITCH];
            w[a] = wl[(AY - 1 - a) * kMixCols];
            if (a == kMixRShFence) __builtin_amdgcn_sched_barrier(0);
        }
        if (kMixRShFence >= AY) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int a = 0; a < AY; ++a)
#pragma unroll
            for (int y = 0; y < S; ++y) cfma(acc[y], t[y + a], w[a]);
        if (TILES == 1) __syncthreads();   // the tile's readers are done
        park(TILES == 2 ? buf ^ 1 : 0);    // (the last step parks the last atom again: never read)
        __syncthreads();
    }
    if (kx >= KX) return;
#pragma unroll
    for (int y = 0; y < S; ++y)
        if (y0 + y < Dy) OT[(long)n * ((long)Dy * KXP) + (long)(y0 + y) * KXP + kx] = acc[y];
}

// 1-D signals (one row per plane): OT[n,c,kx] = sum_m T[n,m,kx] * WT[m,c,kx] -- a thread per (sample, kx), all channels
// of the sample in registers, the atom loop unrolled by four so that four loads of T are in flight.
template <typename T, int CG, int SAMPLES>
__global__ __launch_bounds__(kMixCols *SAMPLES) void k_mix_reconstruct_1d(const cplx<T> *Tsp, const cplx<T> *WT,
                                                                        cplx<T> *OT, int N, int M, int C, int KX,
                                                                        int KXP) {
    const int col = threadIdx.x & (kMixCols - 1), sub = threadIdx.x / kMixCols;
    const int kx = blockIdx.x * kMixCols + col, kxc = min(kx, KX - 1);
    const int n = blockIdx.y * SAMPLES + sub, nc = min(n, N - 1);
    cplx<T> acc[CG];
#pragma unroll
    for (int c = 0; c < CG; ++c) acc[c] = {0, 0};
    const cplx<T> *tp = Tsp + (long)nc * M * KXP + kxc;
    int m = 0;
    for (; m + 4 <= M; m += 4) {
        cplx<T> t[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = tp[(long)(m + q) * KXP];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < CG; ++c) cfma(acc[c], t[q], WT[((long)(m + q) * C + min(c, C - 1)) * KXP + kxc]);
    }
    for (; m < M; ++m) {
        const cplx<T> t = tp[(long)m * KXP];
#pragma unroll
        for (int c = 0; c < CG; ++c) cfma(acc[c], t, WT[((long)m * C + min(c, C - 1)) * KXP + kxc]);
    }
    if (kx >= KX || n >= N) return;
#pragma unroll
    for (int c = 0; c < CG; ++c) {
        if (c >= C) break;
        OT[((long)n * C + c) * KXP + kx] = acc[c];
    }
}

template <typename T, int AY>
int launch_mix_reconstruct(const void *Tsp, const void *WT, void *OT, const Geo &g, int KX, int KXP, hipStream_t s) {
    const unsigned tiles = (unsigned)cdiv(KX, kMixCols);
    if constexpr (AY == 1) {
        if (g.Dy == 1) {   // 1-D signals
            constexpr int SAMPLES = 16;
            hipLaunchKernelGGL((k_mix_reconstruct_1d<T, 3, SAMPLES>), dim3(tiles, (unsigned)cdiv(g.N, SAMPLES)),
                               dim3(kMixCols * SAMPLES), 0, s, (const cplx<T> *)Tsp, (const cplx<T> *)WT, (cplx<T> *)OT,
                               g.N, g.M, g.C, KX, KXP);
            TNMF_LAUNCH_CHECK();
            return TNMF_OK;
        }
    }
    if constexpr (AY <= kMixRShMaxAy) {
        // large calls: the same arithmetic with the row spectra staged through LDS, every entry loaded once
        if (mixed_reconstruct_sh_takes(g, KXP)) {
            // kMixRShPerCU workgroups per CU and no more: unused dynamic LDS tops the tiles up to just over a
            // (kMixRShPerCU + 1)-th of the CU's 160 KiB
            constexpr unsigned tiles_lds = mix_rsh_lds_bytes(AY), hold = (160u << 10) / (kMixRShPerCU + 1) + 1;
            static_assert(tiles_lds * kMixRShPerCU <= 160u << 10, "the tiles of kMixRShPerCU workgroups fit a CU");
            hipLaunchKernelGGL((k_mix_reconstruct_sh<T, AY, kMixRShStrips, kMixRShTiles>),
                               dim3(tiles, (unsigned)cdiv(g.Dy, 16 * kMixRShStrips), (unsigned)g.N),
                               dim3(kMixCols * kMixRShStrips), tiles_lds < hold ? hold - tiles_lds : 0u, s,
                               (const cplx<T> *)Tsp, (const cplx<T> *)WT,
                               (cplx<T> *)OT, g.M, g.Hy, g.Dy, KX, KXP);
            TNMF_LAUNCH_CHECK();
            return TNMF_OK;
        }
    }
    if (g.C == 1) {
        constexpr int S = 16, STRIPS = 8;
        hipLaunchKernelGGL((k_mix_reconstruct<T, AY, 1, S, STRIPS>),
                           dim3(tiles, (unsigned)cdiv(g.Dy, S * STRIPS), (unsigned)g.N), dim3(kMixCols * STRIPS), 0, s,
                           (const cplx<T> *)Tsp, (const cplx<T> *)WT, (cplx<T> *)OT, g.M, g.C, g.Hy, g.Dy, KX, KXP);
    } else {
        // up to three channels: shorter strips keep the three accumulator sets and the atom rows of three channels in
        // registers
        constexpr int S = 8, STRIPS = 8;
        hipLaunchKernelGGL((k_mix_reconstruct<T, AY, 3, S, STRIPS>),
                           dim3(tiles, (unsigned)cdiv(g.Dy, S * STRIPS), (unsigned)g.N), dim3(kMixCols * STRIPS), 0, s,
                           (const cplx<T> *)Tsp, (const cplx<T> *)WT, (cplx<T> *)OT, g.M, g.C, g.Hy, g.Dy, KX, KXP);
    }
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

// ---- W gradient ----------------------------------------------------------------------------------------------------
// block = 16 kx x GROUPS sample groups for one atom; a thread walks the rows of its samples with a rolling window of AY
// row-spectrum entries and accumulates the AY lags for neg (against VT) and pos (against RT).
// grid (atoms, kx tiles, sample-group blocks); partial sums [group][M*C][AY][KXP], summed in order afterwards
template <typename T, int AY, int CG, int GROUPS>
__global__ __launch_bounds__(kMixCols *GROUPS, 2) void k_mix_grad_W(const cplx<T> *Tsp, const cplx<T> *VT,
                                                                 const cplx<T> *RT, cplx<T> *Gn, cplx<T> *Gp, int N,
                                                                 int M, int C, int Hy, int Dy, int KX, int KXP,
                                                                 int nper) {
    const int col = threadIdx.x & (kMixCols - 1), sub = threadIdx.x / kMixCols;
    // the atom index runs fastest over the blocks: the blocks in flight share the V^/R^ rows of one kx tile (L2)
    const int kx = blockIdx.y * kMixCols + col, kxc = min(kx, KX - 1);
    const int m = blockIdx.x, grp = blockIdx.z * GROUPS + sub;
    cplx<T> an[CG][AY], ap[CG][AY];
#pragma unroll
    for (int c = 0; c < CG; ++c)
#pragma unroll
        for (int a = 0; a < AY; ++a) {
            an[c][a] = {0, 0};
            ap[c][a] = {0, 0};
        }
    const int nbeg = grp * nper, nend = min(N, nbeg + nper);
    const long tplane = (long)Hy * KXP, vplane = (long)Dy * KXP;
    static_assert(CG == 1, "one channel per thread");
#pragma unroll 1
    for (int n = nbeg; n < nend; ++n) {
        const cplx<T> *tp = Tsp + ((long)n * M + m) * tplane;   // uniform bases, 32-bit per-thread offsets
        const cplx<T> *vp = VT + (long)n * C * vplane, *rp = RT + (long)n * C * vplane;
        // Rows are taken in blocks of AY: the block [yb, yb+AY) needs T[yb .. yb+2AY-2] and V/R[yb .. yb+AY-1].  The
        // next block's AY new T rows and its V/R rows are fetched while the current block is accumulated.
        cplx<T> t[2 * AY - 1], v[AY], r[AY], tn[AY], vn[AY], rn[AY];
#pragma unroll
        for (int i = 0; i < 2 * AY - 1; ++i) t[i] = tp[(unsigned)(min(i, Hy - 1) * KXP + kxc)];
#pragma unroll
        for (int j = 0; j < AY; ++j) {
            const unsigned o = (unsigned)(min(j, Dy - 1) * KXP + kxc);
            v[j] = vp[o];
            r[j] = rp[o];
        }
#pragma unroll 1
        for (int yb = 0; yb < Dy; yb += AY) {
#pragma unroll
            for (int i = 0; i < AY; ++i) tn[i] = tp[(unsigned)(min(yb + 2 * AY - 1 + i, Hy - 1) * KXP + kxc)];
#pragma unroll
            for (int j = 0; j < AY; ++j) {
                const unsigned o = (unsigned)(min(yb + AY + j, Dy - 1) * KXP + kxc);
                vn[j] = vp[o];
                rn[j] = rp[o];
            }
#pragma unroll
            for (int j = 0; j < AY; ++j) {
                if (yb + j >= Dy) {   // rows past the data contribute nothing
                    v[j] = {0, 0};
                    r[j] = {0, 0};
                }
#pragma unroll
                for (int a = 0; a < AY; ++a) {
                    cfmac(an[0][a], t[j + a], v[j]);
                    cfmac(ap[0][a], t[j + a], r[j]);
                }
            }
#pragma unroll
            for (int i = 0; i < AY - 1; ++i) t[i] = t[i + AY];
#pragma unroll
            for (int i = 0; i < AY; ++i) t[AY - 1 + i] = tn[i];
#pragma unroll
            for (int j = 0; j < AY; ++j) {
                v[j] = vn[j];
                r[j] = rn[j];
            }
        }
    }
    if (kx >= KX) return;
    const long gplane = (long)AY * KXP, gsize = (long)M * C * gplane;
#pragma unroll
    for (int c = 0; c < CG; ++c) {
        if (c >= C) break;
#pragma unroll
        for (int a = 0; a < AY; ++a) {
            const long o = (long)grp * gsize + ((long)m * C + c) * gplane + (long)a * KXP + kx;
            Gn[o] = an[c][a];
            Gp[o] = ap[c][a];
        }
    }
}

// Two atoms per thread: the V^/R^ row entries -- the operand every atom block re-reads -- are loaded once for both, and
// the address arithmetic and loop overhead of a row are shared.  Rows are taken one at a time through register rings
// that are indexed statically (the row loop is unrolled over one ring period): RS >= AY + 4 slots per atom for the row
// spectra of H (row y needs T[y .. y+AY-1]; the rows behind them are in flight), VS = 8 slots for V^ and R^ (7 rows in
// flight); RS is a multiple of VS so that one period of RS rows serves both rings.
template <typename T, int AY, int GROUPS>
__global__ __launch_bounds__(kMixCols *GROUPS, 2) void k_mix_grad_W2(const cplx<T> *Tsp, const cplx<T> *VT,
                                                                  const cplx<T> *RT, cplx<T> *Gn, cplx<T> *Gp, int N,
                                                                  int M, int Hy, int Dy, int KX, int KXP, int nper,
                                                                  int gx, int gy, int gz) {
    constexpr int MA = 2, VS = 8, RS = (AY + 4 + VS - 1) / VS * VS, P = VS - 1;
    const int col = threadIdx.x & (kMixCols - 1), sub = threadIdx.x / kMixCols;
    // XCD-aware block order.  The logical grid is (atom pairs, kx tiles, group blocks), atom pairs fastest: the gx blocks
    // of one (kx tile, group block) read the SAME V^ / R^ rows.  The hardware deals consecutive workgroups round-robin to
    // the eight XCDs, each with an L2 of its own -- dealt in logical order the sixteen sharers landed on eight L2s and the
    // small operand was fetched eight times (PMC: 4.36 GB fetched for 2.8 GB of H spectra).  Launched as a 1-D grid and
    // remapped so that every XCD walks a contiguous chunk of the logical order, the sharers meet in one L2.
    int lin = blockIdx.x;
    {
        const int total = gx * gy * gz, whole = total / 8 * 8;
        if (lin < whole) lin = (lin & 7) * (whole / 8) + (lin >> 3);
    }
    const int bx = lin % gx, by = (lin / gx) % gy, bz = lin / (gx * gy);
    const int kx = by * kMixCols + col, kxc = min(kx, KX - 1);
    const int m0 = bx * MA, grp = bz * GROUPS + sub;
    const int m1 = min(m0 + 1, M - 1);   // odd M: the second atom of the last block repeats the first (not stored)
    cplx<T> an[MA][AY], ap[MA][AY];
#pragma unroll
    for (int q = 0; q < MA; ++q)
#pragma unroll
        for (int a = 0; a < AY; ++a) {
            an[q][a] = {0, 0};
            ap[q][a] = {0, 0};
        }
    // Addresses: a wave holds GROUPS sample groups, so the sample index differs from lane to lane.  Every address is
    // split into a wave-uniform part -- a buffer descriptor based at (sample nr of the block's first group, atom) plus
    // a scalar row offset -- and a per-lane 32-bit byte offset that never changes (group of the lane, kx).  With whole
    // per-lane 64-bit pointers the address arithmetic (20 64-bit vector operations per row next to 96 packed
    // multiply-adds) cost a third of the kernel.  The host checks that the offsets fit 31 bits.
    static_assert(sizeof(cplx<T>) == 8, "float spectra");
    typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
    const long tplane = (long)Hy * KXP, vplane = (long)Dy * KXP;
    const int nbeg0 = bz * GROUPS * nper, nbeg = nbeg0 + sub * nper;
    const int lane_t = (int)(((long)sub * nper * M * tplane + kxc) * 8);
    const int lane_v = (int)(((long)sub * nper * vplane + kxc) * 8);
    const int rowb = KXP * 8;   // bytes per row of spectra
    auto ld = [](const __amdgpu_buffer_rsrc_t &rs, int lane_off, int row_off) {
        const u32x2v w = __builtin_amdgcn_raw_buffer_load_b64(rs, lane_off, row_off, 0);
        const unsigned re = w[0], im = w[1];   // (bit_cast straight on a vector element reads element 0: hipcc 7.2)
        return cplx<T>{__builtin_bit_cast(float, re), __builtin_bit_cast(float, im)};
    };
#pragma unroll 1
    for (int nr = 0; nr < nper; ++nr) {
        if (nbeg0 + nr >= N) break;    // (uniform) no group of this block has a sample nr
        if (nbeg + nr >= N) continue;  // this lane's group has run out of samples
        const cplx<T> *tb = Tsp + ((long)(nbeg0 + nr) * M + m0) * tplane;
        const __amdgpu_buffer_rsrc_t t0 = __builtin_amdgcn_make_buffer_rsrc((void *)tb, 0, 0x7fffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t t1 =
            __builtin_amdgcn_make_buffer_rsrc((void *)(tb + (long)(m1 - m0) * tplane), 0, 0x7fffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t vb =
            __builtin_amdgcn_make_buffer_rsrc((void *)(VT + (long)(nbeg0 + nr) * vplane), 0, 0x7fffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t rb =
            __builtin_amdgcn_make_buffer_rsrc((void *)(RT + (long)(nbeg0 + nr) * vplane), 0, 0x7fffffff, 0x00020000);
        cplx<T> t[MA][RS], v[VS], r[VS];
        // rows 0 .. RS-2 of the H spectra, rows 0 .. P-1 of V^/R^ (row indices clamped: always legal addresses)
#pragma unroll
        for (int i = 0; i < RS - 1; ++i) {
            const int o = min(i, Hy - 1) * rowb;
            t[0][i] = ld(t0, lane_t, o);
            t[1][i] = ld(t1, lane_t, o);
        }
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const int o = min(i, Dy - 1) * rowb;
            v[i] = ld(vb, lane_v, o);
            r[i] = ld(rb, lane_v, o);
        }
#pragma unroll 1
        for (int yb = 0; yb < Dy; yb += RS) {
            // one period of both rings: every ring index below is a compile-time constant
#pragma unroll
            for (int i = 0; i < RS; ++i) {
                const int y = yb + i;
                if (y >= Dy) break;   // wave-uniform
                // fetch: H row y + RS - 1 into the slot row y - 1 left, V^/R^ row y + P into the slot row y - 1 left
                {
                    const int o = min(y + RS - 1, Hy - 1) * rowb;
                    t[0][(i + RS - 1) % RS] = ld(t0, lane_t, o);
                    t[1][(i + RS - 1) % RS] = ld(t1, lane_t, o);
                    const int ov = min(y + P, Dy - 1) * rowb;
                    v[(i + P) % VS] = ld(vb, lane_v, ov);
                    r[(i + P) % VS] = ld(rb, lane_v, ov);
                }
                const cplx<T> vy = v[i % VS], ry = r[i % VS];
#pragma unroll
                for (int a = 0; a < AY; ++a) {
                    cfmac(an[0][a], t[0][(i + a) % RS], vy);
                    cfmac(ap[0][a], t[0][(i + a) % RS], ry);
                    cfmac(an[1][a], t[1][(i + a) % RS], vy);
                    cfmac(ap[1][a], t[1][(i + a) % RS], ry);
                }
            }
        }
    }
    if (kx >= KX) return;
    const long gplane = (long)AY * KXP, gsize = (long)M * gplane;
#pragma unroll
    for (int q = 0; q < MA; ++q) {
        if (m0 + q >= M) break;
#pragma unroll
        for (int a = 0; a < AY; ++a) {
            const long o = (long)grp * gsize + (long)(m0 + q) * gplane + (long)a * KXP + kx;
            Gn[o] = an[q][a];
            Gp[o] = ap[q][a];
        }
    }
}

// Large calls (mixed_grad_W3_takes): three packed FMAs per lag where k_mix_grad_W2 issues four.  With t = p + iq from
// T, x = c + id from V^ or R^ and s = p + q (Gauss's three-multiplication form)
//   t * conj(x) = (pc + qd) + i(qc - pd),   pc + qd = c*s - q*(c - d),   qc - pd = c*s - p*(c + d)
// so three REAL sums per lag and stream are accumulated, A1 += c*s, A2 += (c + d)*p, A3 += (c - d)*q, and Re = A1 - A3,
// Im = A1 - A2 are formed once, in the epilogue.  The two streams ride in the two halves of a register pair --
// X1 = (c_V, c_R), X2 = (c_V + d_V, c_R + d_R), X3 = (c_V - d_V, c_R - d_R) -- so a lag costs three v_pk_fma_f32 for V^
// AND R^, the scalar (s, p or q) broadcast by op_sel.  The extra adds are one per T entry (s) and two per V^/R^ row.
//
// Three accumulator sets leave room for ONE atom per thread, so the V^/R^ rows, which every atom needs, are loaded
// once per workgroup: block = 16 kx x 16 atoms, all on the same sample group, walking the same samples and rows.  Per
// chunk of CH = 16 rows every thread loads 16 bytes of V^ or R^ (16 rows x 2 streams x 128 bytes = 256 x 16), trades
// one entry with its neighbour lane (the other stream of the same row and kx pair), forms X1, X2, X3 of one (row, kx)
// and writes them to an LDS ring of two chunks; one barrier per chunk, the next chunk's loads in flight under the
// current chunk's arithmetic, three broadcast ds_read_b64 per row (the four atoms of a wave read the same addresses).
// T: one wave-uniform descriptor per sample (based at the block's first atom), a scalar row offset, one constant
// per-lane byte offset (atom plane, kx); rows through a ring of RS = 16 statically indexed slots (row y needs
// T[y .. y+AY-1]; RS - AY >= 4 rows are in flight), s formed when a row enters the window -- two s per register pair,
// picked by op_sel like p and q.  One ring period = one chunk.
// grid: 1-D, logical (atom blocks, kx tiles, groups), atom blocks fastest, XCD remap as above; partial sums
// [group][M][AY][KXP] as k_fft_sum_groups reads them.  Groups without samples store zeros.
// (TNMF_MIX_NO_DS_PAIRING: a ds_read2_b64 of X1 and X2 moves half the bytes per LDS clock)
template <typename T, int AY>
__global__ __launch_bounds__(kMixCols *kMixW3Atoms, kMixW3Waves) TNMF_MIX_NO_DS_PAIRING void k_mix_grad_W3(
    const cplx<T> *Tsp, const cplx<T> *VT, const cplx<T> *RT, cplx<T> *Gn, cplx<T> *Gp, int N, int M, int Hy, int Dy,
    int KX, int KXP, int nper, int gx, int gy, int gz) {
    constexpr int NA = kMixW3Atoms, RS = 16, CH = RS, NT = kMixCols * NA;
    static_assert(AY + 4 <= RS && sizeof(cplx<T>) == 8 && NT == 2 * CH * (kMixCols / 2), "ring depth, float spectra");
    const int col = threadIdx.x & (kMixCols - 1), slot = threadIdx.x / kMixCols;
    int lin = blockIdx.x;
    {
        const int total = gx * gy * gz, whole = total / 8 * 8;
        if (lin < whole) lin = (lin & 7) * (whole / 8) + (lin >> 3);
    }
    const int bx = lin % gx, by = (lin / gx) % gy, grp = lin / (gx * gy);
    const int kx = by * kMixCols + col, kxc = min(kx, KX - 1);
    const int m = bx * NA + slot, mc = min(m, M - 1);   // atom slots past M repeat the last atom (not stored)
    f2v a1[AY], a2[AY], a3[AY];
#pragma unroll
    for (int a = 0; a < AY; ++a) a1[a] = a2[a] = a3[a] = {0, 0};
    typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
    typedef float f4v __attribute__((ext_vector_type(4)));
    const long tplane = (long)Hy * KXP, vplane = (long)Dy * KXP;
    const int nbeg = grp * nper, nend = min(N, nbeg + nper);
    const int lane_t = (int)(((long)(mc - bx * NA) * tplane + kxc) * 8);   // the host checks that it fits 31 bits
    const int rowb = KXP * 8;
    auto ld = [](const __amdgpu_buffer_rsrc_t &rs, int lane_off, int row_off) {
        const u32x2v w = __builtin_amdgcn_raw_buffer_load_b64(rs, lane_off, row_off, 0);
        const unsigned re = w[0], im = w[1];   // (bit_cast straight on a vector element reads element 0: hipcc 7.2)
        return cplx<T>{__builtin_bit_cast(float, re), __builtin_bit_cast(float, im)};
    };
    // V^ / R^ staging: thread = (row of the chunk, pair of kx, stream); even lanes load V^, odd lanes R^
    __shared__ __align__(16) f2v xl[2][3][CH * kMixCols];
    const int prow = threadIdx.x / kMixCols, ppair = (threadIdx.x >> 1) & (kMixCols / 2 - 1), pstream = threadIdx.x & 1;
    const cplx<T> *xsrc = (pstream ? RT : VT) + by * kMixCols + 2 * ppair;   // (KXP: whole 128-byte segments)
    f4v pre;
    auto xfetch = [&](int n, int chunk) {   // always a legal address: rows clamped, the caller clamps n
        pre = *reinterpret_cast<const f4v *>(xsrc + (long)n * vplane + (long)min(chunk * CH + prow, Dy - 1) * KXP);
    };
    auto xpark = [&](int buf) {
        // a V^ lane keeps its first entry and takes the R^ lane's first; the R^ lane keeps its second and takes V^'s
        auto swap1 = [](float v) {   // the value of lane ^ 1 (quad_perm [1,0,3,2]; every lane is active here)
            return __builtin_bit_cast(float,
                                      __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));
        };
        const float oc = swap1(pstream ? pre[0] : pre[2]), od = swap1(pstream ? pre[1] : pre[3]);
        const float cv = pstream ? oc : pre[0], dv = pstream ? od : pre[1];
        const float cr = pstream ? pre[2] : oc, dr = pstream ? pre[3] : od;
        const int e = prow * kMixCols + 2 * ppair + pstream;
        xl[buf][0][e] = f2v{cv, cr};
        xl[buf][1][e] = f2v{cv + dv, cr + dr};
        xl[buf][2][e] = f2v{cv - dv, cr - dr};
    };
    xfetch(min(nbeg, N - 1), 0);
    xpark(0);
    __syncthreads();
    int buf = 0;
#pragma unroll 1
    for (int n = nbeg; n < nend; ++n) {   // (uniform over the workgroup, like every branch below)
        const __amdgpu_buffer_rsrc_t t0 = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(Tsp + ((long)n * M + bx * NA) * tplane), 0, 0x7fffffff, 0x00020000);
        cplx<T> t[RS];
        f2v sp[RS / 2];   // s of ring slot j in half j & 1 of sp[j / 2]
        // rows 0 .. RS-2 (row indices clamped: always legal addresses), s of rows 0 .. AY-2
#pragma unroll
        for (int i = 0; i < RS - 1; ++i) t[i] = ld(t0, lane_t, min(i, Hy - 1) * rowb);
#pragma unroll
        for (int i = 0; i < AY - 1; ++i) sp[i / 2][i & 1] = t[i][0] + t[i][1];
#pragma unroll 1
        for (int yb = 0; yb < Dy; yb += CH) {
            // the chunk after this one: the next rows of the sample, or the first rows of the next sample
            {
                const bool last = yb + CH >= Dy;
                xfetch(last ? min(n + 1, nend - 1) : n, last ? 0 : yb / CH + 1);
            }
            const f2v *x1 = &xl[buf][0][col], *x2 = &xl[buf][1][col], *x3 = &xl[buf][2][col];
            // one ring period = one chunk: every ring index below is a compile-time constant
#pragma unroll
            for (int i = 0; i < RS; ++i) {
                const int y = yb + i;
                if (y >= Dy) break;
                t[(i + RS - 1) % RS] = ld(t0, lane_t, min(y + RS - 1, Hy - 1) * rowb);   // into the slot row y - 1 left
                {
                    const int j = (i + AY - 1) % RS;   // row y + AY - 1 enters the window
                    sp[j / 2][j & 1] = t[j][0] + t[j][1];
                }
                const f2v c = x1[i * kMixCols], cpd = x2[i * kMixCols], cmd = x3[i * kMixCols];
#pragma unroll
                for (int a = 0; a < AY; ++a) {
                    const int j = (i + a) % RS;
                    if (j & 1)
                        pfma_hi(a1[a], c, sp[j / 2]);
                    else
                        pfma_lo(a1[a], c, sp[j / 2]);
                    pfma_lo(a2[a], cpd, t[j]);
                    pfma_hi(a3[a], cmd, t[j]);
                }
            }
            xpark(buf ^ 1);   // (its last readers passed the barrier of the previous chunk)
            __syncthreads();
            buf ^= 1;
        }
    }
    if (kx >= KX || m >= M) return;
    const long gplane = (long)AY * KXP, gsize = (long)M * gplane;
#pragma unroll
    for (int a = 0; a < AY; ++a) {
        const long o = (long)grp * gsize + (long)m * gplane + (long)a * KXP + kx;
        Gn[o] = cplx<T>{a1[a][0] - a3[a][0], a1[a][0] - a2[a][0]};
        Gp[o] = cplx<T>{a1[a][1] - a3[a][1], a1[a][1] - a2[a][1]};
    }
}

// 1-D signals (one row per plane, AY == 1), up to CG channels per thread:
//   GT[m,c,kx] = sum_n T[n,m,kx] * conj(VT[n,c,kx])   (and with RT); no lags along y, one entry per (sample, atom, kx)
template <typename T, int CG, int GROUPS>
__global__ __launch_bounds__(kMixCols *GROUPS) void k_mix_grad_W_1d(const cplx<T> *Tsp, const cplx<T> *VT, const cplx<T> *RT,
                                                                  cplx<T> *Gn, cplx<T> *Gp, int N, int M, int C, int KX,
                                                                  int KXP, int nper) {
    const int col = threadIdx.x & (kMixCols - 1), sub = threadIdx.x / kMixCols;
    const int kx = blockIdx.y * kMixCols + col, kxc = min(kx, KX - 1);
    const int m = blockIdx.x, grp = blockIdx.z * GROUPS + sub;
    cplx<T> an[CG], ap[CG];
#pragma unroll
    for (int c = 0; c < CG; ++c) {
        an[c] = {0, 0};
        ap[c] = {0, 0};
    }
    const int nbeg = grp * nper, nend = min(N, nbeg + nper);
    for (int n = nbeg; n < nend; ++n) {
        const cplx<T> t = Tsp[((long)n * M + m) * KXP + kxc];
#pragma unroll
        for (int c = 0; c < CG; ++c) {
            const long o = ((long)n * C + min(c, C - 1)) * KXP + kxc;
            cfmac(an[c], t, VT[o]);
            cfmac(ap[c], t, RT[o]);
        }
    }
    if (kx >= KX) return;
    const long gsize = (long)M * C * KXP;
#pragma unroll
    for (int c = 0; c < CG; ++c) {
        if (c >= C) break;
        const long o = (long)grp * gsize + ((long)m * C + c) * KXP + kx;
        Gn[o] = an[c];
        Gp[o] = ap[c];
    }
}

template <typename T, int AY>
int launch_mix_grad_W(const void *Tsp, const void *VT, const void *RT, void *Gn, void *Gp, const Geo &g, int KX,
                      int KXP, int ngroups, int nper, hipStream_t s) {
    constexpr int GROUPS = 4;
    if constexpr (AY == 1) {
        if (g.Dy == 1) {   // 1-D signals: all channels of an atom in one thread
            const dim3 grid((unsigned)g.M, (unsigned)cdiv(KX, kMixCols), (unsigned)cdiv(ngroups, GROUPS));
            hipLaunchKernelGGL((k_mix_grad_W_1d<T, 4, GROUPS>), grid, dim3(kMixCols * GROUPS), 0, s, (const cplx<T> *)Tsp,
                               (const cplx<T> *)VT, (const cplx<T> *)RT, (cplx<T> *)Gn, (cplx<T> *)Gp, g.N, g.M, g.C, KX,
                               KXP, nper);
            TNMF_LAUNCH_CHECK();
            return TNMF_OK;
        }
    }
    if constexpr (AY <= kMixW3MaxAy) {
        // large calls: the three-multiply kernel; ngroups / nper are those of mix_groups_w3() (fft.hip), no padding
        if (mixed_grad_W3_takes(g, KXP)) {
            const int gx = cdiv(g.M, kMixW3Atoms), gy = cdiv(KX, kMixCols), gz = ngroups;
            // (kMixW3Waves == 2, an A/B flavour: 48 KiB of unused dynamic LDS keep a third workgroup off the CU)
            hipLaunchKernelGGL((k_mix_grad_W3<T, AY>), dim3((unsigned)(gx * gy * gz)), dim3(kMixCols * kMixW3Atoms),
                               kMixW3Waves == 2 ? 48u << 10 : 0u, s,
                               (const cplx<T> *)Tsp, (const cplx<T> *)VT, (const cplx<T> *)RT, (cplx<T> *)Gn,
                               (cplx<T> *)Gp, g.N, g.M, g.Hy, g.Dy, KX, KXP, nper, gx, gy, gz);
            TNMF_LAUNCH_CHECK();
            return TNMF_OK;
        }
    }
    if constexpr (AY <= 12) {   // (taller atoms: the two-atom variant no longer fits the register file)
        // per-lane byte offsets of the two-atom kernel: (group within the block) * nper samples of row spectra, plus
        // a scalar row offset -- they must stay below 2^31 (the single-atom kernel below has no such limit)
        const long span = ((long)(GROUPS - 1) * nper * g.M + 2) * g.Hy * KXP * 8;
        if (g.C == 1 && span < (1L << 31)) {
            const int gx = cdiv(g.M, 2), gy = cdiv(KX, kMixCols), gz = cdiv(ngroups, GROUPS);
            hipLaunchKernelGGL((k_mix_grad_W2<T, AY, GROUPS>), dim3((unsigned)(gx * gy * gz)), dim3(kMixCols * GROUPS), 0, s,
                               (const cplx<T> *)Tsp, (const cplx<T> *)VT, (const cplx<T> *)RT, (cplx<T> *)Gn,
                               (cplx<T> *)Gp, g.N, g.M, g.Hy, g.Dy, KX, KXP, nper, gx, gy, gz);
            TNMF_LAUNCH_CHECK();
            return TNMF_OK;
        }
    }
    const dim3 grid((unsigned)g.M, (unsigned)cdiv(KX, kMixCols), (unsigned)cdiv(ngroups, GROUPS));
    hipLaunchKernelGGL((k_mix_grad_W<T, AY, 1, GROUPS>), grid, dim3(kMixCols * GROUPS), 0, s, (const cplx<T> *)Tsp,
                       (const cplx<T> *)VT, (const cplx<T> *)RT, (cplx<T> *)Gn, (cplx<T> *)Gp, g.N, g.M, g.C, g.Hy, g.Dy,
                       KX, KXP, nper);
    TNMF_LAUNCH_CHECK();
    return TNMF_OK;
}

#define MIX_SWITCH(FN, ...)                                   \
    switch (g.Ay) {                                           \
        case 1: return FN<float, 1>(__VA_ARGS__);             \
        case 2: return FN<float, 2>(__VA_ARGS__);             \
        case 3: return FN<float, 3>(__VA_ARGS__);             \
        case 4: return FN<float, 4>(__VA_ARGS__);             \
        case 5: return FN<float, 5>(__VA_ARGS__);             \
        case 6: return FN<float, 6>(__VA_ARGS__);             \
        case 7: return FN<float, 7>(__VA_ARGS__);             \
        case 8: return FN<float, 8>(__VA_ARGS__);             \
        case 9: return FN<float, 9>(__VA_ARGS__);             \
        case 10: return FN<float, 10>(__VA_ARGS__);           \
        case 11: return FN<float, 11>(__VA_ARGS__);           \
        case 12: return FN<float, 12>(__VA_ARGS__);           \
        case 13: return FN<float, 13>(__VA_ARGS__);           \
        case 14: return FN<float, 14>(__VA_ARGS__);           \
        case 15: return FN<float, 15>(__VA_ARGS__);           \
        case 16: return FN<float, 16>(__VA_ARGS__);           \
        default: return TNMF_E_UNSUPPORTED;                   \
    }

}  // namespace

// float32, one channel, atoms up to 16 rows.  With several channels the column-transform kernels of fft_kernels.h,
// whose cost does not grow with C*Ay, are faster (measured with the three-channel variant of k_mix_reconstruct, which
// is kept instantiated: config 4 reconstruct 2.5 -> 3.3 ms, config 5 11.0 -> 15.5 ms), and the W gradient's two
// accumulator sets per channel no longer fit the registers.
// 1-D signals (Dy == Ay == 1): nothing to contract along y, so up to three / four channels fit as well.
bool mixed_has_reconstruct(const Geo &g, int dtype) {
    return dtype == 0 && g.Ay <= 16 && (g.C == 1 || (g.Dy == 1 && g.Ay == 1 && g.C <= 3));
}
bool mixed_has_grad_W(const Geo &g, int dtype) {
    return dtype == 0 && g.Ay <= 16 && (g.C == 1 || (g.Dy == 1 && g.Ay == 1 && g.C <= 4));
}

// k_mix_grad_W3 takes the 2-D one-channel calls with atoms up to 12 rows whose row spectra of H reach 24 MiB; below
// that the launch is a few microseconds and the grid of k_mix_grad_W2 (a wave per workgroup, four groups in it) fills
// the chip as well.  Its per-lane byte offsets (atom slot 15, last row) must fit 31 bits.
bool mixed_grad_W3_takes(const Geo &g, int KXP) {
#ifdef TNMF_MIX_NO_W3   // A/B flavour of the library (Makefile: VARIANT): every call stays on the older kernels
    return false;
#endif
    const long span = (long)kMixW3Atoms * g.Hy * KXP * 8;
    const long spectra = (long)g.N * g.M * g.Hy * KXP * 8;
    return g.C == 1 && g.Ay <= kMixW3MaxAy && !(g.Dy == 1 && g.Ay == 1) && span < (1L << 31) && spectra >= kMixW3MinBytes;
}

// k_mix_reconstruct_sh takes the 2-D one-channel calls with atoms up to 12 rows whose row spectra of H reach 24 MiB (the
// threshold of the W gradient's large-call kernel: the same calls run both); below that the grid of the register form
// fills the chip as well and every geometry of the FFT matrix stays on the kernel its mirror names.  Its per-lane byte
// offsets (last row of a plane) must fit 31 bits.
bool mixed_reconstruct_sh_takes(const Geo &g, int KXP) {
#ifdef TNMF_MIX_NO_RSH   // A/B flavour of the library (Makefile: VARIANT): every reconstruct stays on the register form
    return false;
#endif
    const long plane = (long)g.Hy * KXP * 8;
    const long spectra = (long)g.N * g.M * g.Hy * KXP * 8;
    return g.C == 1 && g.Ay <= kMixRShMaxAy && !(g.Dy == 1 && g.Ay == 1) && plane < (1L << 31) && spectra >= kMixRShMinBytes;
}

int mixed_reconstruct(const Geo &g, const void *Tsp, const void *WT, void *OT, int KX, int KXP, hipStream_t s) {
    MIX_SWITCH(launch_mix_reconstruct, Tsp, WT, OT, g, KX, KXP, s);
}

int mixed_grad_W(const Geo &g, const void *Tsp, const void *VT, const void *RT, void *Gn, void *Gp, int KX, int KXP,
                 int ngroups, int nper, hipStream_t s) {
    MIX_SWITCH(launch_mix_grad_W, Tsp, VT, RT, Gn, Gp, g, KX, KXP, ngroups, nper, s);
}
