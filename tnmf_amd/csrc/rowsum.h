// The row reduction of the W updates: generic.hip (apply_normalize_row, the energy) and group.hip (the transformed W
// update, which must normalise with the same bits as tnmf_hip_apply_W).
#pragma once
#include <hip/hip_runtime.h>

// Sum of one double per thread over the workgroup: wave-level shuffle tree, then the waves' partials in wave order.  Every
// thread returns the same value.  sh: blockDim.x / 64 doubles of shared memory.
template <typename T>
__device__ double block_sum(double v, double *sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double tot = 0.0;
    const int nw = (blockDim.x + 63) >> 6;
    for (int w = 0; w < nw; ++w) tot += sh[w];  // every thread, same order
    return tot;
}
