// Re-layout and pool-backward kernels of the 16-bit NHWC tensors, once for both formats. PLANES = 1: bf16 [.., C]; PLANES = 2:
// split-fp16 [.., C/8, 2, 8] (a hi and a lo octet per channel octet). One thread per (pixel, channel octet), 16-byte accesses.
#pragma once
#include "common.h"

namespace {

typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

// NHWC [B][HW][C/8][PLANES][8] -> batch-octet [ceil(B/8)][HW][C][PLANES][8 images] (images past B are zeros), the operand layout of
// conv3x3_wgrad_bf16_kernel / conv3x3_wgrad_f16x3_kernel. Per thread: 8 PLANES loads of 16 B (8 channels of one image), an 8x8
// transpose per plane in registers, 8 PLANES stores of 16 B (one channel, 8 images) = 128 PLANES contiguous bytes.
template <int PLANES>
__global__ void to_octet_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ y, int B, size_t HW, int C, size_t total) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int C8 = C >> 3;
    const int c8 = idx % C8;
    const size_t t = idx / C8;
    const size_t pix = t % HW;
    const size_t b8 = t / HW;
    u16x8 in[PLANES][8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const size_t b = b8 * 8 + i;
#pragma unroll
        for (int pl = 0; pl < PLANES; ++pl) {
            if (b < (size_t)B)
                in[pl][i] = *reinterpret_cast<const u16x8*>(x + (((b * HW + pix) * C8 + c8) * PLANES + pl) * 8);
            else
                in[pl][i] = (u16x8){0, 0, 0, 0, 0, 0, 0, 0};
        }
    }
    u16x8* out = reinterpret_cast<u16x8*>(y + (((b8 * HW + pix) * C + (size_t)c8 * 8) * PLANES) * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int pl = 0; pl < PLANES; ++pl) {
            u16x8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = in[pl][i][j];
            out[j * PLANES + pl] = o;
        }
}

// Backward of the fused MaxPool2d(2,2): dy [B,Hp,Wp,C/8,PLANES,8] is routed (every plane) to the position the forward recorded
// (code uint8 [B,Hp,Wp,C] = dy*2+dx); dx [B,H,W,C/8,PLANES,8], H >= 2Hp, W >= 2Wp (a dropped odd row / column keeps its memset zeros).
template <int PLANES>
__global__ void maxpool2x2_bwd16_kernel(const unsigned short* __restrict__ dy, const unsigned char* __restrict__ code,
                                        unsigned short* __restrict__ dx, int Hp, int Wp, int H, int W, int C, size_t total) {
    typedef unsigned char u8x8 __attribute__((ext_vector_type(8)));
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int C8 = C >> 3;
    const int c8 = idx % C8;
    size_t t = idx / C8;
    const int w = t % Wp;
    t /= Wp;
    const int h = t % Hp;
    const size_t b = t / Hp;
    const size_t pp = (b * Hp + h) * Wp + w;
    u16x8 g[PLANES];
#pragma unroll
    for (int pl = 0; pl < PLANES; ++pl) g[pl] = *reinterpret_cast<const u16x8*>(dy + ((pp * C8 + c8) * PLANES + pl) * 8);
    const u8x8 k = *reinterpret_cast<const u8x8*>(code + pp * C + (size_t)c8 * 8);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        u16x8* dst = reinterpret_cast<u16x8*>(dx + ((((b * H + 2 * h + (q >> 1)) * W + 2 * w + (q & 1)) * C8 + c8) * PLANES) * 8);
#pragma unroll
        for (int pl = 0; pl < PLANES; ++pl) {
            u16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (k[e] == q) ? g[pl][e] : (unsigned short)0;
            dst[pl] = o;
        }
    }
}

}  // namespace
