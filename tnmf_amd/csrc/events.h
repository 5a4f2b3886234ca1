// Events: the sparse H side -- render a list of events into R, refit their strengths, score them, take their W gradient
// (events.hip; tnmf_hip_events_render / tnmf_hip_events_update / tnmf_hip_events_gain / tnmf_hip_events_grad_W).
#pragma once

#include <algorithm>

#include "common.h"

// One index scheme for one and two shift axes (signals run as Dy = Ay = 1).  An image sits at a position (qy, qx) of the
// padded activation frame [Dy + Ay - 1, Dx + Ax - 1]; cells of ty x tx positions tile that frame, ncy x ncx per sample.
struct EventGeo {
    int N, P, C;      // samples, planes of W_eff, channels
    int Dy, Dx;       // sample shape
    int Ay, Ax;       // atom shape
    int ty, tx;       // cell = output tile (ty * tx == kEventThreads)
    int ncy, ncx;     // cells per sample and axis
};

// What every kernel that walks an event's occurrence is told: the geometry, the reconstruction mode and the shift shape
// (Sy, Sx) of that mode.  Filled once per entry point (events_enter() of api.hip); the kernels take the four separately.
struct EventFrame {
    EventGeo g;
    int mode, Sy, Sx;
};

constexpr int kEventThreads = 256;

// grid of a grid-stride kernel of the events family: at least one workgroup, at most per_cu per CU
inline unsigned events_grid(const tnmf_hip_ctx *ctx, long long blocks, int per_cu = 64) {
    return (unsigned)std::max<long long>(1, std::min<long long>(blocks, (long long)ctx->num_cu * per_cu));
}

// the cell / tile shape the render works with: 16 x 16 for two shift axes, 1 x 256 for one
inline void events_tile(int ndim, int *ty, int *tx) {
    *ty = ndim == 2 ? TNMF_EVENTS_CELL_2D : 1;
    *tx = ndim == 2 ? TNMF_EVENTS_CELL_2D : TNMF_EVENTS_CELL_1D;
}
static_assert(TNMF_EVENTS_CELL_2D * TNMF_EVENTS_CELL_2D == kEventThreads && TNMF_EVENTS_CELL_1D == kEventThreads,
              "one thread per pixel of a tile");

// R[N,C,Dy,Dx] = the sum over the images of strength[event] * W_eff[plane] placed at their position; every pixel is
// written exactly once.  images: n_images x (plane, qy, qx, event), sorted by (sample, cell); cell_start: N * ncy * ncx + 1.
int events_render(tnmf_hip_ctx *ctx, const EventGeo &g, int dtype, const void *W, const int *images, long long n_images,
                  const int *cell_start, const void *strength, long long n_events, void *R, hipStream_t s);

// strength[e] *= neg_e / (pos_e + reg): V and R gathered under every image of event e = (sample, plane, uy, ux) of the
// reconstruction mode f.mode with shift shape (f.Sy, f.Sx).
int events_update(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const void *W, const int *events, void *strength,
                  long long n_events, const void *V, const void *R, double reg, hipStream_t s);

// gain[e] = E(list without e) - E(list) of the Frobenius energy, = h_e <phi_e, V - R> + h_e^2 |phi_e|^2 / 2 with phi_e the sum
// of the images of event e clipped to the sample, R the render of the list; mag[e] (may be NULL) = the sum of the magnitudes
// of the terms.  Doubles whatever the element type; every element is written, 0 for a row out of range.
int events_gain(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const void *W, const int *events, const void *strength,
                long long n_events, const void *V, const void *R, double *gain, double *mag, hipStream_t s);

// negpos[2, P, C, Ay, Ax] = the W gradient of the events against V (neg) and R (pos): the events sorted by plane
// (by_plane: n_events indices into `events`, plane_start: P + 1), summed in double per segment of TNMF_EVENTS_SEGMENT events
// into `workspace` (events_grad_W_slabs() slabs of 2 * C * Ay * Ax doubles), then per plane in segment order.
long long events_grad_W_slabs(long long n_events, int P);
int events_grad_W(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const int *events, const int *by_plane,
                  const int *plane_start, const void *strength, long long n_events, const void *V, const void *R,
                  void *workspace, void *negpos, hipStream_t s);

// Pursuit (pursuit.hip; tnmf_hip_events_norms / tnmf_hip_pursuit_score / tnmf_hip_pursuit_pick).
// b[P, Sy, Sx] = |phi_{p,u}|^2 in double: the norm of the occurrence of plane p at shift u, all images, clipped to the sample.
int events_norms(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const void *W, double *b, hipStream_t s);

// gain[planes, Sy, Sx] = a^2 / (2 b) where a > 0 and b > 0, else 0 (rows Hs apart; b[P, Sy, Sx] contiguous, planes a multiple
// of P), then the n_taken flat indices of `taken` zeroed.
int pursuit_score(tnmf_hip_ctx *ctx, int dtype, long long planes, int P, int Sy, int Sx, int Hs, const void *a,
                  const double *b, void *gain, const long long *taken, long long n_taken, hipStream_t s);

// per picked flat index of [N, P, Sy, Sx]: the row (n, p, uy, ux), a = <phi, V - R> and b = |phi|^2 in double, the strength
// max(a, 0) / b, the gain a^2 / (2 b) and mag (may be NULL) = sum |w (V - R)|; -1 / 0 for an index out of range.
int pursuit_pick(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const void *W, const long long *idx,
                 long long n_picked, const void *V, const void *R, int *events, void *strength, double *gain, double *mag,
                 hipStream_t s);

// Landscape (landscape.hip; tnmf_hip_events_landscape).
// a, b, mag[n_events, 3^ndim] (DOUBLES; mag may be NULL): per row and neighbour shift u + delta, delta in {-1, 0, 1}^ndim, the
// sums of pursuit_pick against the residual of the list without the row, V - R + h_e phi_e; zeros for a neighbour outside
// the shift shape and for a row out of range.  Every element is written.
int events_landscape(tnmf_hip_ctx *ctx, const EventFrame &f, int ndim, int dtype, const void *W, const int *events,
                     const void *strength, long long n_events, const void *V, const void *R, double *a, double *b,
                     double *mag, hipStream_t s);

// Alternatives (alternatives.hip; tnmf_hip_events_alternatives).
// a, b, mag[n_events, n_alt] (DOUBLES; mag may be NULL): per row and candidate plane p'_j = first + j * stride at the row's own
// shift, first = (p / (n_alt * stride)) * (n_alt * stride) + p % stride (n_alt * stride divides P), the sums of the landscape
// at delta = 0 with the taps of p'_j against the residual of the list without the row; zeros for a row out of range.  Every
// element is written.
int events_alternatives(tnmf_hip_ctx *ctx, const EventFrame &f, int dtype, const void *W, const int *events,
                        const void *strength, long long n_events, const void *V, const void *R, int n_alt, int stride,
                        double *a, double *b, double *mag, hipStream_t s);
