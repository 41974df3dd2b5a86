// What the triplet-loss kernels of both models share: the fixed-order block sum, the two term types (x = d_positive - d_negative)
// and the kernel that adds per-row partials up. The library is built with -ffp-contract=off, so an expression evaluates to the
// same bits inside a member here as it would written out in the kernel.
#pragma once
#include "common.h"

namespace {

// Sum of v over a 256-thread block, the same on every thread and in one fixed order: the 64-lane butterfly, then the four wave
// totals through sh[4]. The leading barrier lets a kernel call it twice on one buffer.
__device__ __forceinline__ float block_sum_256(float v, float* sh) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// cvig_fov (model/cvig_fov.py:366-382): log(1+exp(a x)) as written, summed over the FULL matrix; the derivative's factor a is
// applied once, in the scale.
struct FovTerm {
    float alpha;
    static constexpr bool skip_diag = false;
    __device__ __forceinline__ float value(float x) const { return logf(1.f + expf(alpha * x)); }
    __device__ __forceinline__ float hard_value(float x) const { return value(x); }      // a NaN stays a NaN in value()
    __device__ __forceinline__ float deriv(float x) const { return 1.f / (1.f + expf(-(alpha * x))); }
    __device__ __forceinline__ float scale(float gloss, float norm) const { return gloss * alpha / norm; }
};

// cvig_baseline (exhaustive_minibatch_triplet_loss, model/cvig_baseline.py:286-315): soft margin or hinge, chosen at run time,
// summed over the off-diagonal entries.
struct BaselineTerm {
    int soft;
    float alpha, margin;
    static constexpr bool skip_diag = true;
    __device__ __forceinline__ float value(float x) const { return soft ? logf(1.f + expf(alpha * x)) : fmaxf(x + margin, 0.f); }
    // fmaxf drops a NaN; a NaN embedding must show in the batch-hard loss, as it does in max(x + margin, 0) of torch
    __device__ __forceinline__ float hard_value(float x) const { return x != x ? x : value(x); }
    __device__ __forceinline__ float deriv(float x) const {
        return soft ? alpha / (1.f + expf(-alpha * x)) : ((x + margin > 0.f) ? 1.f : 0.f);
    }
    __device__ __forceinline__ float scale(float gloss, float norm) const { return gloss / norm; }
};

// out[0] = (part[0] + ... + part[n-1]) / norm; one block
__global__ __launch_bounds__(256) void sum_parts_kernel(const float* __restrict__ part, float* __restrict__ out, int n, float norm) {
    __shared__ float sh[4];
    float s = 0.f;
    for (int t = threadIdx.x; t < n; t += 256) s += part[t];
    const float tot = block_sum_256(s, sh);
    if (threadIdx.x == 0) out[0] = tot / norm;
}

}  // namespace
