// Host-side entry points of triggered.hip: activation-triggered sums on a window larger than the atom
// (tnmf_hip_triggered_sums, tnmf_hip_triggered_sums_plan; include/tnmf_hip.h, "triggered sums").
#pragma once
#include "common.h"

// H is the padded activations [N, P, Sy, Sx] (one shift axis: Sy = 1), rows Hs elements apart; Y is [N, F, Dy, Dx].
//   X[p, f, jy, jx] = sum_n sum_q H[n, p, qy, qx]^power * Y[n, f, qy + offy + jy, qx + offx + jx],  off = -(A - 1) - m
// A CELL is 16 consecutive window columns jx of one (field, jy).  One workgroup of kTrigThreads threads owns one
// (segment, strip, block of 16 planes, chunk of cells): a chunk is CF fields, CJ window rows and CB 16-column blocks,
// CF * CJ * CB <= kTrigChunk (CF > 1 only where the whole window of a field fits a chunk); the strip is a run of
// (sample, pixel tile) items whose sums stay in the workgroup's accumulators.  Per item it stages the TY x TX tile of
// the block of planes and, per field of the chunk, the (TY + CJ - 1) x (TX + 16 CB) patch of Y that the tile meets under
// the chunk; wave w contracts the tile for the cells w, w + 4, ... of the chunk on the matrix cores.  A chunk of fewer
// than 4 cells (split): every wave holds every cell and takes every fourth step of four pixels; the waves' sums are
// added in wave order.
// tests/triggered_dispatch.py mirrors these.
constexpr int kTrigThreads = 256;
constexpr int kTrigBlock = 16;           // planes per block, window columns per cell: the sides of v_mfma_f64_16x16x4_f64
constexpr int kTrigChunk = 32;           // cells per chunk: 8 accumulators in each of the 4 waves
constexpr int kTrigTile1Float = 256;     // TX with one shift axis (TY = 1), float
constexpr int kTrigTile1Double = 128;    // TX with one shift axis, double: the same bytes of LDS
constexpr int kTrigTileX = 64;           // TX with two shift axes
constexpr int kTrigTileYFloat = 4;       // TY with two shift axes, float
constexpr int kTrigTileYDouble = 2;      // TY with two shift axes, double
constexpr int kTrigPad = 4;              // elements added to a staged row of H: 16 planes x 4 pixels land in 64 different banks
constexpr int kTrigMaxWindow1 = 4096;    // the largest window A + 2 m with one shift axis
constexpr int kTrigMaxWindow2 = 128;     // the largest window per axis with two shift axes
constexpr int kTrigTargetGroups = 2048;  // workgroups a call aims for when it cuts the items into strips
constexpr size_t kTrigPartialCap = (size_t)256 << 20;   // the strips are not cut finer than this many bytes of partial sums

struct TrigPlan {
    int P, F, Sy, Sx, Hs;    // planes, fields, padded shift shape, row stride of H
    int Dy, Dx;              // sample shape: the shape of a field
    int Wy, Wx;              // window: A + 2 m (one shift axis: Wy = 1)
    int offy, offx;          // -(A - 1) - m: the row / column of Y under window position 0 at padded pixel 0
    int power;               // 1 or 2
    int TY, TX;              // pixel tile
    int tiles_y, tiles_x, tiles;
    int nbp;                 // blocks of 16 planes
    int nxb;                 // cells of a window row: cdiv(Wx, 16)
    int cells;               // F * Wy * nxb
    int CB, CJ, CF;          // a chunk: CB cells along jx times CJ window rows times CF fields
    int YC;                  // columns of the staged patch of Y: TX + 16 CB
    int chunks_x, chunks_y, chunks_f, chunks;   // chunks = chunks_f * chunks_y * chunks_x
    int split;               // 1: CF * CJ * CB < 4, the waves split the steps of the tile, not the cells
    int nseg;                // segments whose sums stay apart: N with per_sample, else 1
    long long seglen;        // (sample, tile) items per segment
    int strips;              // workgroups along a segment
    long long ipg;           // items per strip: cdiv(seglen, strips)
    size_t lds;              // bytes of LDS: [tile of H: TY x 16 rows of TX + pad | patches of Y: CF x (TY + CJ - 1) x YC]
};

// TNMF_E_UNSUPPORTED: a window beyond kTrigMaxWindow1 / kTrigMaxWindow2, more than 2^31 - 1 workgroups or output
// elements; TNMF_E_GEOM: a negative margin, power not 1 or 2, n_fields < 1.  Fills *p on TNMF_OK.  One shift axis:
// Sy = Dy = Ay = 1 and margin[0] is the margin along x.
int triggered_plan(int N, int P, int F, const int *D, const int *A, int Hs, int ndim, const int *margin, int power,
                   int per_sample, int dtype, TrigPlan *p);
// partial sums: nseg * strips * nbp * cells blocks of 16 x 16 doubles
size_t triggered_partial_bytes(const TrigPlan &p);
// X_out[(seg, p, f, jy, jx)] (double, device), every element written.  A plan of at least one sample.
int launch_triggered(const TrigPlan &p, int dtype, const void *H, const void *Y, double *partials, double *X_out,
                     hipStream_t s);
