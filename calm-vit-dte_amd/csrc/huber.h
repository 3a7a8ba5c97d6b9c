// The Huber pieces the token losses share (recon.hip, mim.hip): value and slope of one difference, and the one-workgroup
// final pass that adds the block sums of a forward in a fixed order.
#pragma once
#include "common.h"

#define HUBER_NT 256

__device__ __forceinline__ float huber_value(float d, float delta) {
    const float ad = fabsf(d);
    return ad <= delta ? 0.5f * d * d : (ad != ad ? d : delta * (ad - 0.5f * delta));
}
__device__ __forceinline__ float huber_slope(float d, float delta) {
    return d != d ? d : fminf(fmaxf(d, -delta), delta);              // (fminf / fmaxf drop a NaN: hand it on)
}

// ONE workgroup adds the G block sums in a fixed order (thread t takes t, t + 256, ... in increasing index, then a fixed
// tree over the 256 running sums) and overwrites the loss.
static __global__ __launch_bounds__(HUBER_NT) void huber_rows_final_kernel(const float* __restrict__ part, int G, float scale,
                                                                           float* __restrict__ loss) {
    __shared__ float red[8];
    float s = 0.f;
    for (int g = threadIdx.x; g < G; g += HUBER_NT) s += part[g];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) loss[0] = s * scale;
}
