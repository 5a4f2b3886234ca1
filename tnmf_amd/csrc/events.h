// Events: the sparse H side -- render a list of events into R, refit their strengths, score them, take their W gradient
// (events.hip; tnmf_hip_events_render / tnmf_hip_events_update / tnmf_hip_events_gain / tnmf_hip_events_grad_W).
#pragma once

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

constexpr int kEventThreads = 256;

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
// reconstruction mode `mode` with shift shape (Sy, Sx).
int events_update(tnmf_hip_ctx *ctx, const EventGeo &g, int dtype, int mode, int Sy, int Sx, const void *W,
                  const int *events, void *strength, long long n_events, const void *V, const void *R, double reg,
                  hipStream_t s);

// gain[e] = E(list without e) - E(list) of the Frobenius energy, = h_e <phi_e, V - R> + h_e^2 |phi_e|^2 / 2 with phi_e the sum
// of the images of event e clipped to the sample, R the render of the list; mag[e] (may be NULL) = the sum of the magnitudes
// of the terms.  Doubles whatever the element type; every element is written, 0 for a row out of range.
int events_gain(tnmf_hip_ctx *ctx, const EventGeo &g, int dtype, int mode, int Sy, int Sx, const void *W, const int *events,
                const void *strength, long long n_events, const void *V, const void *R, double *gain, double *mag,
                hipStream_t s);

// negpos[2, P, C, Ay, Ax] = the W gradient of the events against V (neg) and R (pos): the events sorted by plane
// (by_plane: n_events indices into `events`, plane_start: P + 1), summed in double per segment of TNMF_EVENTS_SEGMENT events
// into `workspace` (events_grad_W_slabs() slabs of 2 * C * Ay * Ax doubles), then per plane in segment order.
long long events_grad_W_slabs(long long n_events, int P);
int events_grad_W(tnmf_hip_ctx *ctx, const EventGeo &g, int dtype, int mode, int Sy, int Sx, const int *events,
                  const int *by_plane, const int *plane_start, const void *strength, long long n_events, const void *V,
                  const void *R, void *workspace, void *negpos, hipStream_t s);
