// Per-channel sums of cvig_baseline's training-mode BatchNorm2d and the element-wise pass of its backward, shared by the one-call
// entries (baseline.hip: witw_bn_train_stats, witw_bn_lrelu_bwd[_ex]) and the split ones that leave a seam for a collective between
// the sums and their use (baseline_bn_sync.hip). Every sum is combined in a fixed order: no atomics, the same bits on every call.
#pragma once
#include "common.h"

namespace {

// per-channel partial sums over the valid region: part[blk][0][c] = sum (a - p), part[blk][1][c] = sum (a - p)^2 about the pivot
// p[c] = pivot[c]: mean = p + s0/n and var = s1/n - (s0/n)^2 then subtract numbers of the size of the spread about the pivot, not of
// the mean (plain sums of a and a^2 lose r^2 x 6e-8 of the variance at |mean| = r x std: 4e-4 of invstd at r = 64, and block 7 of a
// training step, 3 values per channel, reaches r = 14). witw_bn_train_stats passes pivot = a, the channel's first valid value.
// (bwd form: g != nullptr -> sum g and sum g*xhat with xhat = (a - mean[c]) * invstd[c], g = second tensor)
__global__ __launch_bounds__(256) void channel_sums_kernel(const float* __restrict__ a, const float* __restrict__ g,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd,
                                                            const float* __restrict__ pivot, float* __restrict__ part, int Hp, int Wp,
                                                            int H, int W, int C, size_t npix, int rows_per_block, int g_cp) {
    __shared__ float sh[2][4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
    const size_t p0 = (size_t)blockIdx.y * rows_per_block, p1 = min(npix, p0 + (size_t)rows_per_block);
    float s0 = 0.f, s1 = 0.f;
    if (c < C) {
        const float mu = g ? mean[c] : 0.f, is = g ? invstd[c] : 0.f;
        const float pv = g ? 0.f : pivot[c];
        for (size_t px = p0 + ph; px < p1; px += 4) {      // px enumerates VALID pixels (b, h<H, w<W)
            const size_t w = px % W, t = px / W, h = t % H, b = t / H;
            const size_t off = ((b * Hp + h) * Wp + w) * C + c;
            const float v = a[off];
            if (g) {
                // g_cp > 0: the gradient is still in the space-to-depth layout the data-gradient conv wrote ([B,ceil(H/2),ceil(W/2),g_cp],
                // channel ((h&1)*2+(w&1))*C + c): read in place, no depth-to-space pass
                const float gv = g_cp ? g[((b * ((H + 1) >> 1) + (h >> 1)) * ((W + 1) >> 1) + (w >> 1)) * g_cp + ((h & 1) * 2 + (w & 1)) * C + c] : g[off];
                s0 += gv;
                s1 += gv * ((v - mu) * is);
            } else {
                const float d = v - pv;
                s0 += d;
                s1 += d * d;
            }
        }
    }
    sh[0][ph][threadIdx.x & 63] = s0;
    sh[1][ph][threadIdx.x & 63] = s1;
    __syncthreads();
    if (threadIdx.x < 64 && c < C) {
        const int l = threadIdx.x;
        part[((size_t)blockIdx.y * 2 + 0) * C + c] = (sh[0][0][l] + sh[0][1][l]) + (sh[0][2][l] + sh[0][3][l]);
        part[((size_t)blockIdx.y * 2 + 1) * C + c] = (sh[1][0][l] + sh[1][1][l]) + (sh[1][2][l] + sh[1][3][l]);
    }
}

// The same sums for channel counts with C % 4 == 0 and (C/4) | 256 (every layer of the reference's encoders): a block
// owns whole image rows (b, h) so the inner loop has no index arithmetic, a thread owns one channel quad (16-byte loads,
// a wave reads 1 KB contiguous) and every (256 / (C/4))-th pixel of the row; fixed-order combination through LDS.
__global__ __launch_bounds__(256) void channel_sums_rows_kernel(const float* __restrict__ a, const float* __restrict__ g,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                 const float* __restrict__ pivot, float* __restrict__ part, int Hp,
                                                                 int Wp, int H, int W, int C, int nrows, int rows_per_block, int g_cp) {
    __shared__ f32x4 sh[2][256];
    const int Q = C >> 2, phases = 256 / Q;
    const int q = threadIdx.x % Q, ph = threadIdx.x / Q;
    const int r0 = blockIdx.x * rows_per_block, r1 = min(nrows, r0 + rows_per_block);
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    f32x4 mu = {0.f, 0.f, 0.f, 0.f}, is = {0.f, 0.f, 0.f, 0.f};
    f32x4 pv = {0.f, 0.f, 0.f, 0.f};                      // the pivot of the forward form (see channel_sums_kernel)
    if (g) {
        mu = *reinterpret_cast<const f32x4*>(mean + 4 * q);
        is = *reinterpret_cast<const f32x4*>(invstd + 4 * q);
    } else {
        pv = *reinterpret_cast<const f32x4*>(pivot + 4 * q);
    }
    for (int r = r0; r < r1; ++r) {
        const int b = r / H, h = r - b * H;
        const size_t row = ((size_t)b * Hp + h) * Wp * C + 4 * q;
        const size_t grow = ((size_t)b * ((H + 1) >> 1) + (h >> 1)) * ((W + 1) >> 1) * g_cp + (h & 1) * 2 * C + 4 * q;      // s2d layout (g_cp > 0)
        for (int w = ph; w < W; w += phases) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(a + row + (size_t)w * C);
            if (g) {
                const f32x4 gv = *reinterpret_cast<const f32x4*>(g_cp ? g + grow + (size_t)(w >> 1) * g_cp + (w & 1) * C : g + row + (size_t)w * C);
                s0 += gv;
                s1 += gv * ((v - mu) * is);
            } else {
                const f32x4 d = v - pv;
                s0 += d;
                s1 += d * d;
            }
        }
    }
    sh[0][threadIdx.x] = s0;
    sh[1][threadIdx.x] = s1;
    __syncthreads();
    if (threadIdx.x < Q) {
        f32x4 t0 = sh[0][threadIdx.x], t1 = sh[1][threadIdx.x];
        for (int k = 1; k < phases; ++k) {
            t0 += sh[0][k * Q + threadIdx.x];
            t1 += sh[1][k * Q + threadIdx.x];
        }
        *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.x * 2 + 0) * C + 4 * threadIdx.x) = t0;
        *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.x * 2 + 1) * C + 4 * threadIdx.x) = t1;
    }
}

// Second stage of the per-channel sums: part [nparts][2][C] -> two sums per channel. A workgroup takes 32 channels; its 32 groups of 32
// lanes each add every 32nd partial row (loads of a group: 128 contiguous bytes, 8 in flight), then the group sums are added in a
// fixed order through LDS -- bit-reproducible, and 32x fewer dependent loads per thread than one thread per channel (the stage took
// 157 us of pure load latency per call at 1024 partial rows; 25-40 us with 8 groups).
constexpr int BNF_CH = 32, BNF_LANES = 32;
__device__ __forceinline__ bool bn_finish_sums(const float* __restrict__ part, int nparts, int C, int& c, float& s0, float& s1) {
    __shared__ float red[2][BNF_LANES][BNF_CH];
    const int cl = threadIdx.x % BNF_CH, pl = threadIdx.x / BNF_CH;
    c = blockIdx.x * BNF_CH + cl;
    float a0 = 0.f, a1 = 0.f;
    if (c < C)
#pragma unroll 8
        for (int k = pl; k < nparts; k += BNF_LANES) {
            a0 += part[((size_t)k * 2 + 0) * C + c];
            a1 += part[((size_t)k * 2 + 1) * C + c];
        }
    red[0][pl][cl] = a0;
    red[1][pl][cl] = a1;
    __syncthreads();
    if (pl != 0 || c >= C) return false;
    s0 = 0.f; s1 = 0.f;
#pragma unroll
    for (int j = 0; j < BNF_LANES; ++j) { s0 += red[0][j][cl]; s1 += red[1][j][cl]; }
    return true;
}

// dz = lrelu'(a) * gamma*invstd * (dy - sum_dy/n - xhat*sum_dyxhat/n) on the valid region, 0 elsewhere.
__global__ void bn_lrelu_bwd_apply_kernel(const float* __restrict__ a, const float* __restrict__ dy, float* __restrict__ dz,
                                          const float* __restrict__ mean, const float* __restrict__ invstd,
                                          const float* __restrict__ gamma, const float* __restrict__ sums, int Hp, int Wp, int H,
                                          int W, int C, float n, float slope, size_t total, int g_cp) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = idx % C;
    size_t t = idx / C;
    const int w = t % Wp;
    t /= Wp;
    const int h = t % Hp;
    float out = 0.f;
    if (h < H && w < W) {
        const float av = a[idx];
        const float xh = (av - mean[c]) * invstd[c];
        const size_t b = t / Hp;
        const float gy = g_cp ? dy[((b * ((H + 1) >> 1) + (h >> 1)) * ((W + 1) >> 1) + (w >> 1)) * g_cp + ((h & 1) * 2 + (w & 1)) * C + c] : dy[idx];
        const float da = gamma[c] * invstd[c] * (gy - sums[c] / n - xh * sums[C + c] / n);
        out = av > 0.f ? da : da * slope;
    }
    dz[idx] = out;
}

// The same for C % 4 == 0 (and g_cp % 4 == 0): one thread per channel quad, the same arithmetic per element.
__global__ void bn_lrelu_bwd_apply_quad_kernel(const float* __restrict__ a, const float* __restrict__ dy, float* __restrict__ dz,
                                               const float* __restrict__ mean, const float* __restrict__ invstd,
                                               const float* __restrict__ gamma, const float* __restrict__ sums, int Hp, int Wp, int H,
                                               int W, int C, float n, float slope, size_t total4, int g_cp) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total4) return;
    const int C4 = C >> 2;
    const int c = 4 * (int)(idx % C4);
    size_t t = idx / C4;
    const int w = t % Wp;
    t /= Wp;
    const int h = t % Hp;
    f32x4 out = {0.f, 0.f, 0.f, 0.f};
    if (h < H && w < W) {
        const size_t b = t / Hp;
        const f32x4 av = reinterpret_cast<const f32x4*>(a)[idx];
        const f32x4 gy = *reinterpret_cast<const f32x4*>(
            g_cp ? dy + ((b * ((H + 1) >> 1) + (h >> 1)) * ((W + 1) >> 1) + (w >> 1)) * g_cp + ((h & 1) * 2 + (w & 1)) * C + c : dy + 4 * idx);
        const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c), is = *reinterpret_cast<const f32x4*>(invstd + c);
        const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + c);
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sums + c), s1 = *reinterpret_cast<const f32x4*>(sums + C + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xh = (av[j] - mu[j]) * is[j];
            const float da = ga[j] * is[j] * (gy[j] - s0[j] / n - xh * s1[j] / n);
            out[j] = av[j] > 0.f ? da : da * slope;
        }
    }
    reinterpret_cast<f32x4*>(dz)[idx] = out;
}

// ---- host side: grid shapes of the sums (witw_bn_workspace_floats sizes the partials for either form)
int bl_rows(size_t npix) {
    size_t r = (npix + 127) / 128;
    return (int)(r < 64 ? 64 : r);
}

// row-based sums (channel_sums_rows_kernel): image rows per block for ~1024 blocks, and whether C qualifies
int bl_rows_per_block(int nrows) { return cdiv(nrows, 1024); }
bool bl_wide(int C) { return (C % 4) == 0 && C >= 4 && C <= 1024 && (256 % (C / 4)) == 0; }

// launches the partial sums (forward form about pivot when g == nullptr, else the backward form); returns the number of partials written
int bl_launch_sums(const float* a, const float* g, const float* mean, const float* invstd, const float* pivot, float* part, int B,
                   int Hp, int Wp, int H, int W, int C, hipStream_t st, int g_cp = 0) {
    const size_t npix = (size_t)B * H * W;
    if (bl_wide(C)) {
        const int nrows = B * H, rpb = bl_rows_per_block(nrows), nparts = cdiv(nrows, rpb);
        hipLaunchKernelGGL(channel_sums_rows_kernel, dim3(nparts), dim3(256), 0, st, a, g, mean, invstd, pivot, part, Hp, Wp, H, W, C,
                           nrows, rpb, g_cp);
        return nparts;
    }
    const int rows = bl_rows(npix), nparts = (int)((npix + rows - 1) / rows);
    hipLaunchKernelGGL(channel_sums_kernel, dim3(cdiv(C, 64), nparts), dim3(256), 0, st, a, g, mean, invstd, pivot, part, Hp, Wp, H, W,
                       C, npix, rows, g_cp);
    return nparts;
}

// launches dz of the BatchNorm + LeakyReLU backward from the finished sums [2][C] and the element count n they were taken over
void bl_launch_apply(const float* a, const float* dy, float* dz, const float* mean, const float* invstd, const float* gamma,
                     const float* sums, float n, int B, int Hp, int Wp, int H, int W, int C, float slope, int g_cp, hipStream_t st) {
    const size_t total = (size_t)B * Hp * Wp * C;
    if ((C & 3) == 0)
        hipLaunchKernelGGL(bn_lrelu_bwd_apply_quad_kernel, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, st, a, dy, dz, mean,
                           invstd, gamma, sums, Hp, Wp, H, W, C, n, slope, total / 4, g_cp);
    else
        hipLaunchKernelGGL(bn_lrelu_bwd_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, dy, dz, mean, invstd,
                           gamma, sums, Hp, Wp, H, W, C, n, slope, total, g_cp);
}

}  // namespace
