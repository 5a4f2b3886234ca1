// The occurrence of an event on the device, shared by the kernels of events.hip and pursuit.hip: its images (per axis:
// axis_images of modes.h), the walk over the taps of every image clipped to the sample, the value phi of the occurrence at a
// pixel, and the wave's sum.  For landscape.hip and alternatives.hip also the residual of the list without a row and the sums
// of several values of a wave at once (the test for one image wholly inside the sample is axis_whole of modes.h).
// Device code only; everything is inlined into the kernel that calls it, the lambda of for_each_tap included.
#pragma once

#include "events.h"
#include "modes.h"

// the images of the shift (uy, ux) of the mode with shift shape (Sy, Sx): ny * nx of them, at (qy[iy], qx[ix])
struct Occurrence {
    int ny, nx, qy[2], qx[2];
    __device__ __forceinline__ Occurrence(const EventGeo &g, int mode, int Sy, int Sx, int uy, int ux)
        : qy{0, 0}, qx{0, 0} {   // (a second position that does not exist reads as 0, never as an unset value)
        ny = axis_images(mode, uy, g.Ay, Sy, qy);
        nx = axis_images(mode, ux, g.Ax, Sx, qx);
    }
    __device__ __forceinline__ bool single() const { return ny * nx == 1; }   // phi at a pixel is the tap itself
};

// f(t, c, y, x) for the taps t = first, first + step, ... of every image, in (iy, ix) order, whose pixel (y, x) of channel c
// lies inside the sample.  A wave passes (lane, 64), a single thread (0, 1).
template <typename F>
__device__ __forceinline__ void for_each_tap(const EventGeo &g, const Occurrence &o, int first, int step, F &&f) {
    const int AA = g.Ay * g.Ax, taps = g.C * AA;
    const unsigned uAA = AA, uAx = g.Ax;   // (t >= 0 is divided by positive extents: unsigned, no sign handling per tap)
    // (copies the loops may index: indexed by a loop variable inside `o`, the whole value leaves the registers for LDS;
    // tools/probes/kernel_resources.py --no-lds checks that it has not)
    const int qy[2] = {o.qy[0], o.qy[1]}, qx[2] = {o.qx[0], o.qx[1]};
    for (int iy = 0; iy < o.ny; ++iy) {
        for (int ix = 0; ix < o.nx; ++ix) {
            const int oy = qy[iy] - (g.Ay - 1), ox = qx[ix] - (g.Ax - 1);
            for (int t = first; t < taps; t += step) {
                const int c = t / uAA, r = t - c * AA;
                const int jy = r / uAx, jx = r - jy * g.Ax;
                const int y = oy + jy, x = ox + jx;
                if ((unsigned)y < (unsigned)g.Dy && (unsigned)x < (unsigned)g.Dx) f(t, c, y, x);
            }
        }
    }
}

// phi at pixel (y, x) of the channel whose taps start at w[cAA] (cAA = c * Ay * Ax, w the plane's taps):
// every image that covers this pixel, in image order
template <typename T>
__device__ __forceinline__ double phi_at(const EventGeo &g, const Occurrence &o, const T *w, int cAA, int y, int x) {
    const int qy[2] = {o.qy[0], o.qy[1]}, qx[2] = {o.qx[0], o.qx[1]};   // (as in for_each_tap)
    double phi = 0.;
    for (int ky = 0; ky < o.ny; ++ky) {
        const int ly = y - (qy[ky] - (g.Ay - 1));
        if ((unsigned)ly >= (unsigned)g.Ay) continue;
        for (int kx = 0; kx < o.nx; ++kx) {
            const int lx = x - (qx[kx] - (g.Ax - 1));
            if ((unsigned)lx < (unsigned)g.Ax) phi += (double)w[cAA + ly * g.Ax + lx];
        }
    }
    return phi;
}

// the sum over the 64 lanes, in every lane: a butterfly, the same order of additions in every lane and run
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// d_e at a pixel: the residual with the row's own contribution h * phi put back (phi = 0 off the row's occurrence)
template <typename T>
__device__ __forceinline__ double residual_without(T v, T r, double h, double phi) {
    return fma(h, phi, (double)v - (double)r);
}

// The sums over the 64 lanes of N values at once, each bit for bit the wave_sum of its value: the same butterfly (offsets
// 32 .. 1; a + b commutes, so every lane of wave_sum holds the same bits and which lane adds is free), but at every step a lane
// keeps half of the values it holds and hands the other half to its partner -- a step moves ceil(n / 2) values, not n, and
// they are independent of each other.  A value without a partner value is added the plain way, in both lanes.
template <int N, int OFF>
__device__ __forceinline__ void wave_sum_step(double *v, int lane) {
    constexpr int H = (N + 1) / 2;
    const bool upper = (lane & OFF) != 0;
#pragma unroll
    for (int i = 0; i < N - H; ++i) {   // the pair (i, i + H): the lower lane keeps i, the upper one i + H
        const double send = upper ? v[i] : v[i + H], keep = upper ? v[i + H] : v[i];
        v[i] = keep + __shfl_xor(send, OFF, 64);
    }
    if (N & 1) v[H - 1] += __shfl_xor(v[H - 1], OFF, 64);
    if constexpr (OFF > 1) wave_sum_step<H, OFF / 2>(v, lane);
}

// -> v[0] = the sum of the value *which; true in exactly one lane per value, the one that reports it.  Which value a lane
// ends with is read backwards off its bits: the slot s after a step came from s + H in an upper lane, from s in a lower one,
// and a slot without a partner is reported by the lower lane.
template <int N>
__device__ __forceinline__ bool wave_sum_many(double (&v)[N], int lane, int *which) {
    wave_sum_step<N, 32>(v, lane);
    int n[6] = {N, 0, 0, 0, 0, 0};   // the values a lane holds before the steps of offsets 32, 16, 8, 4, 2, 1
#pragma unroll
    for (int k = 1; k < 6; ++k) n[k] = (n[k - 1] + 1) / 2;
    int s = 0;
    bool own = true;
#pragma unroll
    for (int k = 5; k >= 0; --k) {
        const int H = (n[k] + 1) / 2;
        const bool upper = (lane & (32 >> k)) != 0;
        if (s < n[k] - H)
            s += upper ? H : 0;
        else
            own = own && !upper;
    }
    *which = s;
    return own;
}
