// Host-side entry points of correlogram.hip: which planes of H co-occur, and at what offset
// (tnmf_hip_activation_correlogram; include/tnmf_hip.h, "activation correlogram").
#pragma once
#include "common.h"

// H is [N, P, Sy, Sx] (one shift axis: Sy = 1), rows Hs elements apart.  One workgroup of kCorrThreads threads owns one
// (segment, strip, ordered pair (I, J) of blocks of 16 planes, lag chunk): a lag chunk is one dy >= 0 and up to
// kCorrChunk consecutive dx of the half of the lags that is >= 0 in C order; the strip is a run of (sample, pixel tile)
// items whose sums stay in the workgroup's accumulators.  Per item it stages the TY x TX tile of block I and the
// TY x (TX + kCorrChunk) window of block J that the tile meets under the chunk's lags; wave w contracts the tile for
// the lags w, w + 4, ... of the chunk on the matrix cores.
// tests/correlogram_dispatch.py mirrors these.
constexpr int kCorrThreads = 256;
constexpr int kCorrBlock = 16;           // planes per block: one side of v_mfma_f64_16x16x4_f64
constexpr int kCorrChunk = 32;           // lags per chunk: 8 accumulators in each of the 4 waves
constexpr int kCorrTile1Float = 256;     // TX with one shift axis (TY = 1), float
constexpr int kCorrTile1Double = 128;    // TX with one shift axis, double: the same bytes of LDS
constexpr int kCorrTileX = 64;           // TX with two shift axes
constexpr int kCorrTileYFloat = 4;       // TY with two shift axes, float
constexpr int kCorrTileYDouble = 2;      // TY with two shift axes, double
constexpr int kCorrPad = 4;              // elements added to a staged row: 16 planes x 4 pixels land in 64 different banks
constexpr int kCorrMaxLag1 = 1023;       // the largest max_lag with one shift axis
constexpr int kCorrMaxLag2 = 63;         // the largest max_lag per axis with two shift axes
constexpr int kCorrTargetGroups = 2048;  // workgroups a call aims for when it cuts the items into strips
constexpr size_t kCorrPartialCap = (size_t)256 << 20;   // the strips are not cut finer than this many bytes of partial sums

struct CorrPlan {
    int P, Sy, Sx, Hs;       // planes, shift shape, row stride
    int Ly, Lx;              // the lags asked for (one shift axis: Ly = 0)
    int Lye, Lxe;            // the lags that can be non-zero: min(L, S - 1)
    int TY, TX;              // pixel tile
    int tiles_y, tiles_x, tiles;
    int nb, pairs;           // blocks of 16 planes, ordered pairs of them: nb * nb
    int c0, cr, chunks;      // lag chunks of the row dy = 0 (dx >= 0), of a row dy > 0 (every dx), in all
    int nh;                  // lags computed: Lxe + 1 + Lye * (2 Lxe + 1)
    int nseg;                // segments whose sums stay apart: N with per_sample, else 1
    long long seglen;        // (sample, tile) items per segment
    int strips;              // workgroups along a segment
    long long ipg;           // items per strip: cdiv(seglen, strips)
    size_t lds;              // bytes of LDS: [tile of I: TY x 16 rows of TX + pad | window of J: rows of TX + chunk + pad]
};

// TNMF_E_UNSUPPORTED: a lag beyond kCorrMaxLag1 / kCorrMaxLag2, more than 2^31 - 1 workgroups or output elements per
// segment; TNMF_E_GEOM: a negative lag.  Fills *p on TNMF_OK.  One shift axis: Sy = 1 and max_lag[0] is the lag along x.
int correlogram_plan(int N, int P, int Sy, int Sx, int Hs, int ndim, const int *max_lag, int per_sample, int dtype,
                     CorrPlan *p);
// partial sums: nseg * strips * pairs * nh blocks of 16 x 16 doubles
size_t correlogram_partial_bytes(const CorrPlan &p);
// C_out[(seg, p, q, ly, lx)] (double, device), every element written.  A plan of at least one sample.
int launch_correlogram(const CorrPlan &p, int dtype, const void *H, double *partials, double *C_out, hipStream_t s);
