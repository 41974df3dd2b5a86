// The two norm kernels every match launch (match.hip, match_dft.hip) fills the head of its workspace with: wn [Bo,64], then
// sn [Bs]. One text for both files: the kernels that read the workspace afterwards (witw_match_pairs, the backward) rely on the
// direct and the spectral launch leaving the same numbers there.
#pragma once
#include "common.h"

namespace {

// wn[o][shift] = sqrt(sum_{ch} sum_{k<We} ov[o][ch][(k+shift)%64]^2): the L2 norm of the window
// that crop_overhead would cut at that shift (model/cvig_fov.py:335-341,350-351).
__global__ __launch_bounds__(256) void window_norm_kernel(const float* __restrict__ ov, float* __restrict__ wn, int We) {
    __shared__ float part[4][64];
    __shared__ float col[64];
    const int o = blockIdx.x, t = threadIdx.x, w = t & 63, g = t >> 6;
    const float* base = ov + (size_t)o * 4096;
    float s = 0.f;
    for (int ch = g * 16; ch < g * 16 + 16; ++ch) {
        const float v = base[ch * 64 + w];
        s += v * v;
    }
    part[g][w] = s;
    __syncthreads();
    if (t < 64) col[t] = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
    __syncthreads();
    if (t < 64) {
        float acc = 0.f;
        for (int k = 0; k < We; ++k) acc += col[(t + k) & 63];
        wn[(size_t)o * 64 + t] = sqrtf(acc);
    }
}

// sn[s] = |su[s]|_2 over all 64*We elements (model/cvig_fov.py:356-357).
__global__ __launch_bounds__(256) void row_norm_kernel(const float* __restrict__ x, float* __restrict__ out, int n) {
    __shared__ float part[4];
    const float* base = x + (size_t)blockIdx.x * n;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = base[i];
        s += v * v;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = sqrtf((part[0] + part[1]) + (part[2] + part[3]));
}

}  // namespace
