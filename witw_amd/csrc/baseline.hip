// cvig_baseline pieces that are not the conv itself (gfx950; small memory-bound kernels).
//
// The reference's SurfaceEncoder / OverheadEncoder (model/cvig_baseline.py:228-283) stack
// 7 x [Conv2d(k=4,s=2,p=0) -> LeakyReLU(0.2) -> BatchNorm2d]. A 4x4 stride-2 convolution is a
// 2x2 stride-1 convolution over the space-to-depth(2) image (channels (dy,dx,c)), which the
// NHWC MFMA conv kernel runs as a 3x3 filter whose first row/column of taps is zero; LeakyReLU
// and the (eval-mode) BatchNorm affine sit in that kernel's epilogue. Here: the space-to-depth
// re-layout (with the in-model x/255, -1+2x of :265-266 fused for the first layer), the GeM-like
// pooling (:276-282), the final f/sqrt(|f|) (:284), squared-Euclidean distance matrix and the
// exhaustive minibatch triplet loss (:286-315).
#include "common.h"
#include "bn_sums.h"
#include "loss_terms.h"
#include "sqdist_row.h"

namespace {

// x: NHWC [B,Hp,Wp,C] (or NCHW [B,C,Hp,Wp] if in_nchw) of which rows < H, cols < W are valid.
// y: NHWC [B,ceil(H/2),ceil(W/2),Cp], y[b,h2,w2,(dy*2+dx)*C+c] = f(x[b,2h2+dy,2w2+dx,c]); zero elsewhere.
__global__ void space_to_depth2_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int Hp, int Wp, int H, int W,
                                       int C, int Cp, int in_nchw, int normalize, size_t total,
                                       const float* __restrict__ scale, const float* __restrict__ shift) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int H2 = (H + 1) >> 1, W2 = (W + 1) >> 1;
    const int cc = idx % Cp;
    size_t t = idx / Cp;
    const int w2 = t % W2;
    t /= W2;
    const int h2 = t % H2;
    const int b = (int)(t / H2);
    float v = 0.f;
    if (cc < 4 * C) {
        const int q = cc / C, c = cc - q * C;
        const int h = 2 * h2 + (q >> 1), w = 2 * w2 + (q & 1);
        if (h < H && w < W) {
            v = in_nchw ? x[(((size_t)b * C + c) * Hp + h) * Wp + w] : x[(((size_t)b * Hp + h) * Wp + w) * C + c];
            if (normalize) {       // x = x / 255.; x = -1. + 2. * x   (model/cvig_baseline.py:265-266)
                v = v / 255.f;
                v = -1.f + 2.f * v;
            }
            if (scale != nullptr) v = v * scale[c] + shift[c];     // train-mode BatchNorm of the producer layer
        }
    }
    y[idx] = v;
}

// The same for an NHWC source with C % 4 == 0 and Cp == 4C (every block but the first): one thread per V channels of one quadrant,
// 16-byte loads, the same arithmetic per element, +0.0 outside the H x W valid region (the affine is NOT applied there). OUT = float
// stores V = 4 channels as they are; OUT = __bf16 stores V = 8 or 4 with one nearest-even rounding at the store.
template <typename OUT, int V>
__global__ void space_to_depth2_quad_kernel(const float* __restrict__ x, OUT* __restrict__ y, int Hp, int Wp, int H, int W, int C,
                                            size_t total, const float* __restrict__ scale, const float* __restrict__ shift) {
    typedef OUT out_v __attribute__((ext_vector_type(V)));
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int H2 = (H + 1) >> 1, W2 = (W + 1) >> 1, CV = C / V;
    const int cv = idx % CV;
    size_t t = idx / CV;
    const int q = t & 3;
    t >>= 2;
    const int w2 = t % W2;
    t /= W2;
    const int h2 = t % H2;
    const size_t b = t / H2;
    const int h = 2 * h2 + (q >> 1), w = 2 * w2 + (q & 1);
    out_v o;
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = (OUT)0.f;
    if (h < H && w < W) {
        const float* src = x + ((b * Hp + h) * Wp + w) * C + V * cv;
#pragma unroll
        for (int k = 0; k < V; k += 4) {
            f32x4 v = *reinterpret_cast<const f32x4*>(src + k);
            if (scale != nullptr) {
                const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + V * cv + k), sf = *reinterpret_cast<const f32x4*>(shift + V * cv + k);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = v[j] * sc[j] + sf[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) o[k + j] = (OUT)v[j];
        }
    }
    reinterpret_cast<out_v*>(y)[idx] = o;
}

// Mosaic space-to-depth: x NHWC [B,H,W,C] (all valid) -> y [ceil(B/g^2), g*H2, g*W2, 4C], H2 = ceil(H/2): image b sits in cell
// (b % g^2) of mosaic image b / g^2, cells row-major, each the space-to-depth(2) image of x[b]; zeros where no source exists.
// A k=4,s=2 layer over an H2 x W2 s2d map has (H2-1) x (W2-1) valid outputs, so no valid output's 2x2 window crosses a cell:
// the deep cvig_baseline layers (8x8 and 4x4 maps) run as g = 2 / g = 4 mosaics that fill the conv kernel's 16x16 tile.
// One thread per V channels of one output pixel's quadrant; OUT and V as in space_to_depth2_quad_kernel.
template <typename OUT, int V>
__global__ void s2d_mosaic_kernel(const float* __restrict__ x, OUT* __restrict__ y, int B, int H, int W, int C, int g, size_t total) {
    typedef OUT out_v __attribute__((ext_vector_type(V)));
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int H2 = (H + 1) >> 1, W2 = (W + 1) >> 1;
    const int CV = C / V;
    const int cv = idx % CV;
    size_t t = idx / CV;
    const int q = t & 3;
    t >>= 2;
    const int X = t % (g * W2);
    t /= (g * W2);
    const int Y = t % (g * H2);
    const int bm = (int)(t / (g * H2));
    const int cy = Y / H2, y2 = Y - cy * H2, cx = X / W2, x2 = X - cx * W2;
    const int b = (bm * g + cy) * g + cx;
    const int h = 2 * y2 + (q >> 1), w = 2 * x2 + (q & 1);
    out_v o;
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = (OUT)0.f;
    if (b < B && h < H && w < W) {
        const float* src = x + (((size_t)b * H + h) * W + w) * C + V * cv;
#pragma unroll
        for (int k = 0; k < V; k += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + k);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[k + j] = (OUT)v[j];
        }
    }
    reinterpret_cast<out_v*>(y)[idx] = o;
}

// Epilogue of a split-K taps4 convolution run over a g x g mosaic: ws [S][Bm, g*h, g*w, C] raw partial sums ->
// y [B, vh, vw, C] (valid outputs of every image, compact), y = affine(lrelu(sum_s ws[s] + bias)); the S partials are added in
// slice order (deterministic).
__global__ void splitk_finish_kernel(const float* __restrict__ ws, int S, size_t stride, const float* __restrict__ bias, int act,
                                     float slope, const float* __restrict__ post_scale, const float* __restrict__ post_shift,
                                     float* __restrict__ y, int B, int g, int h, int w, int vh, int vw, int C, size_t total4) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total4) return;
    const int C4 = C >> 2;
    const int c4 = idx % C4;
    size_t t = idx / C4;
    const int xx = t % vw;
    t /= vw;
    const int yy = t % vh;
    const int b = (int)(t / vh);
    const int bm = b / (g * g), cell = b - bm * g * g, cy = cell / g, cx = cell - cy * g;
    const size_t o = ((((size_t)bm * g * h + cy * h + yy) * (g * w)) + cx * w + xx) * C + 4 * c4;
    f32x4 a = *reinterpret_cast<const f32x4*>(ws + o);
    for (int s = 1; s < S; ++s) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(ws + (size_t)s * stride + o);
        a += v;
    }
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + 4 * c4);
    f32x4 ps = {1.f, 1.f, 1.f, 1.f}, pt = {0.f, 0.f, 0.f, 0.f};
    if (post_scale != nullptr) {
        ps = *reinterpret_cast<const f32x4*>(post_scale + 4 * c4);
        pt = *reinterpret_cast<const f32x4*>(post_shift + 4 * c4);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float v = a[e] + bv[e];
        if (act == 1) v = fmaxf(v, 0.f);
        else if (act == 2) v = v > 0.f ? v : v * slope;
        a[e] = v * ps[e] + pt[e];
    }
    reinterpret_cast<f32x4*>(y)[idx] = a;
}

// f[b, col0 + c] = (mean_{h<H,w<W} relu(x[b,h,w,c])^p)^(1/p); x NHWC [B,Hp,Wp,C]; one thread per (b,c).
constexpr int GEM_PH = 8;      // pixel phases per channel
__global__ __launch_bounds__(64 * GEM_PH) void gem_pool_kernel(const float* __restrict__ x, float* __restrict__ f, int B, int Hp, int Wp, int H,
                                                               int W, int C, int ldf, int col0, float p, const float* __restrict__ scale,
                                                               const float* __restrict__ shift) {
    // one workgroup per (image, 64 channels): a thread sums every GEM_PH-th pixel of its channel (a wave reads 256 contiguous bytes per
    // pixel), the phase sums are added in phase order through LDS. (One thread per (image, channel) walked the 13 x 13 map of block 5
    // serially behind a powf each: 107-124 us per call on 64 workgroups.)
    __shared__ float part[GEM_PH][64];
    const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + cl, b = blockIdx.x;
    float s = 0.f;
    if (c < C) {
        const float sc = scale != nullptr ? scale[c] : 1.f, sh = scale != nullptr ? shift[c] : 0.f;
        const int n = H * W;
        for (int q = ph; q < n; q += GEM_PH) {
            const int h = q / W, w = q - h * W;
            float v = x[(((size_t)b * Hp + h) * Wp + w) * C + c];
            if (scale != nullptr) v = v * sc + sh;
            s += powf(fmaxf(v, 0.f), p);
        }
    }
    part[ph][cl] = s;
    __syncthreads();
    if (ph != 0 || c >= C) return;
#pragma unroll
    for (int k = 1; k < GEM_PH; ++k) s += part[k][cl];
    f[(size_t)b * ldf + col0 + c] = powf(s / (float)(H * W), 1.f / p);
}

// f[b,:] /= |f[b,:]|^0.5   (model/cvig_baseline.py:284); one block per row.
__global__ __launch_bounds__(256) void embed_normalize_kernel(float* __restrict__ f, int n) {
    __shared__ float part[4];
    float* row = f + (size_t)blockIdx.x * n;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += row[i] * row[i];
    const float nrm = sqrtf(block_sum_256(s, part));
    const float den = powf(nrm, 0.5f);
    for (int i = threadIdx.x; i < n; i += 256) row[i] = row[i] / den;
}

// D[i][j] = sum_k (a[i][k] - b[j][k])^2 (optionally its square root); block = one i x 256 j.
__global__ __launch_bounds__(256) void pairwise_sqdist_kernel(const float* __restrict__ a, const float* __restrict__ bm,
                                                               float* __restrict__ D, int Na, int Nb, int n, int take_sqrt) {
    extern __shared__ float arow[];
    const int i = blockIdx.y;
    for (int k = threadIdx.x; k < n; k += 256) arow[k] = a[(size_t)i * n + k];
    __syncthreads();
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Nb) return;
    const float s = witw_sqdist_row(arow, bm + (size_t)j * n, n);      // shared with the pair re-scoring of baseline_retrieval.hip
    D[(size_t)i * Nb + j] = take_sqrt ? sqrtf(s) : s;
}

// part[i] = sum_{j != i} l(D_ii - D_ij) + l(D_ii - D_ji); D[i][j] = |e1_i - e2_j|^2
__global__ __launch_bounds__(256) void exhaustive_partials_kernel(const float* __restrict__ D, float* __restrict__ part, int B,
                                                                   BaselineTerm term) {
    __shared__ float sh[4];
    const int i = blockIdx.x;
    const float dii = D[(size_t)i * B + i];
    float s = 0.f;
    for (int j = threadIdx.x; j < B; j += 256) {
        if (j == i) continue;
        s += term.value(dii - D[(size_t)i * B + j]);
        s += term.value(dii - D[(size_t)j * B + i]);
    }
    const float tot = block_sum_256(s, sh);
    if (threadIdx.x == 0) part[i] = tot;
}

// ---------------------------------------------------------------------------------------------------------------
// Training-mode pieces (model/cvig_baseline.py:267-284 under .train(), autograd of :286-315): batch statistics of
// BatchNorm2d, its backward fused with the LeakyReLU backward, GeM / normalisation / loss backward, depth-to-space.
// The per-channel sums and the backward's element-wise pass are in bn_sums.h.

// BatchNorm2d training statistics: mean / biased var -> scale = gamma*invstd, shift = beta - mean*scale, and the
// running-stat update running = (1-m)*running + m*stat (unbiased variance), torch semantics. The sums are about pivot[c].
__global__ __launch_bounds__(BNF_CH * BNF_LANES) void bn_stats_finish_kernel(const float* __restrict__ part, int nparts, int C, float n, const float* __restrict__ pivot,
                                       const float* __restrict__ gamma,
                                       const float* __restrict__ beta, float eps, float momentum, float* __restrict__ mean,
                                       float* __restrict__ invstd, float* __restrict__ scale, float* __restrict__ shift,
                                       float* __restrict__ running_mean, float* __restrict__ running_var) {
    int c;
    float s0, s1;
    if (!bn_finish_sums(part, nparts, C, c, s0, s1)) return;
    const float dm = s0 / n;
    const float mu = pivot[c] + dm;
    const float var = fmaxf(s1 / n - dm * dm, 0.f);
    const float is = 1.f / sqrtf(var + eps);
    mean[c] = mu;
    invstd[c] = is;
    scale[c] = gamma[c] * is;
    shift[c] = beta[c] - mu * gamma[c] * is;
    if (running_mean != nullptr) {
        running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mu;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * (var * n / (n - 1.f));
    }
}

// sums[0][c] = sum dy, sums[1][c] = sum dy*xhat  (+ writes dgamma = sums[1], dbeta = sums[0])
__global__ __launch_bounds__(BNF_CH * BNF_LANES) void bn_bwd_finish_kernel(const float* __restrict__ part, int nparts, int C, float* __restrict__ sums,
                                     float* __restrict__ dgamma, float* __restrict__ dbeta) {
    int c;
    float s0, s1;
    if (!bn_finish_sums(part, nparts, C, c, s0, s1)) return;
    sums[c] = s0;
    sums[C + c] = s1;
    dbeta[c] = s0;
    dgamma[c] = s1;
}

// depth-to-space(2) of the s2d-layout gradient: dx[b,h,w,c] = g[b,h/2,w/2,((h&1)*2+(w&1))*C+c] (+ add[b,h,w,c]) on
// the valid region of a [B,Hp,Wp,C] tensor, 0 elsewhere.
__global__ void depth_to_space2_kernel(const float* __restrict__ g, const float* __restrict__ add, float* __restrict__ dx, int Hp,
                                       int Wp, int H, int W, int C, int Cp, size_t total) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = idx % C;
    size_t t = idx / C;
    const int w = t % Wp;
    t /= Wp;
    const int h = t % Hp;
    const size_t b = t / Hp;
    float v = 0.f;
    if (h < H && w < W) {
        const int H2 = (H + 1) >> 1, W2 = (W + 1) >> 1;
        v = g[((b * H2 + (h >> 1)) * W2 + (w >> 1)) * Cp + ((h & 1) * 2 + (w & 1)) * C + c];
        if (add != nullptr) v += add[idx];
    }
    dx[idx] = v;
}

// GeM backward: dy[b,h,w,c] (+)= df[b,col0+c] * m^(1/p-1) * relu(y)^(p-1) / N, y = a*scale+shift, m = f^p.
__global__ void gem_pool_bwd_kernel(const float* __restrict__ a, const float* __restrict__ scale, const float* __restrict__ shift,
                                    const float* __restrict__ f, const float* __restrict__ df, float* __restrict__ dy, int Hp,
                                    int Wp, int H, int W, int C, int ldf, int col0, float p, int accumulate, size_t total) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = idx % C;
    size_t t = idx / C;
    const int w = t % Wp;
    t /= Wp;
    const int h = t % Hp;
    const size_t b = t / Hp;
    float out = 0.f;
    if (h < H && w < W) {
        const float y = fmaxf(a[idx] * scale[c] + shift[c], 0.f);
        const float fv = f[b * ldf + col0 + c];              // = m^(1/p)
        if (y > 0.f && fv > 0.f) out = df[b * ldf + col0 + c] * powf(fv, 1.f - p) * powf(y, p - 1.f) / (float)(H * W);
    }
    dy[idx] = accumulate ? dy[idx] + out : out;
}

// f = g / |g|^(1/2)  ->  dg = df/|g|^(1/2) - 0.5 * (g.df) * g / |g|^(5/2); one block per row. f and df given, g = f*|g|^(1/2)
// is recovered from the saved norm.
__global__ __launch_bounds__(256) void embed_normalize_bwd_kernel(const float* __restrict__ g, const float* __restrict__ df,
                                                                   float* __restrict__ dg, int n) {
    __shared__ float part[4];
    const float* gr = g + (size_t)blockIdx.x * n;
    const float* dr = df + (size_t)blockIdx.x * n;
    float s0 = 0.f, s1 = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        s0 += gr[i] * gr[i];
        s1 += gr[i] * dr[i];
    }
    const float nn = block_sum_256(s0, part);     // |g|^2
    const float gd = block_sum_256(s1, part);
    const float nrm = sqrtf(nn);
    const float c0 = 1.f / sqrtf(nrm), c1 = 0.5f * gd / (nrm * nrm * sqrtf(nrm));
    for (int i = threadIdx.x; i < n; i += 256) dg[(size_t)blockIdx.x * n + i] = dr[i] * c0 - c1 * gr[i];
}

// G = dL/dD for the exhaustive loss; one block per row a (diagonal entry gathers the row and column terms).
__global__ __launch_bounds__(256) void exhaustive_bwd_kernel(const float* __restrict__ D, const float* __restrict__ gloss,
                                                              float* __restrict__ G, int B, BaselineTerm term) {
    __shared__ float sh[4];
    const int a = blockIdx.x;
    const float daa = D[(size_t)a * B + a];
    const float sc = term.scale(gloss[0], 2.f * B * (B - 1));
    float diag = 0.f;
    for (int j = threadIdx.x; j < B; j += 256) {
        if (j == a) continue;
        const float dab = D[(size_t)a * B + j];
        const float t1 = term.deriv(daa - dab);                       // anchor a in embed1, negative j
        const float t2 = term.deriv(D[(size_t)j * B + j] - dab);      // anchor j in embed2
        G[(size_t)a * B + j] = -(t1 + t2) * sc;
        diag += t1 + term.deriv(daa - D[(size_t)j * B + a]);
    }
    const float tot = block_sum_256(diag, sh);
    if (threadIdx.x == 0) G[(size_t)a * B + a] = tot * sc;
}

// D[a][b] = |e1_a - e2_b|^2: de1[a] = 2 * sum_b G[a][b] (e1_a - e2_b)   (side 0)
//                            de2[b] = 2 * sum_a G[a][b] (e2_b - e1_a)   (side 1); one block per output row.
__global__ __launch_bounds__(256) void sqdist_bwd_kernel(const float* __restrict__ e1, const float* __restrict__ e2,
                                                          const float* __restrict__ G, float* __restrict__ out, int B, int n,
                                                          int side) {
    const int r = blockIdx.x;
    const float* self = (side == 0 ? e1 : e2) + (size_t)r * n;
    const float* other = side == 0 ? e2 : e1;
    for (int k = threadIdx.x; k < n; k += 256) {
        float s = 0.f;
        const float sv = self[k];
        for (int q = 0; q < B; ++q) {
            const float gq = side == 0 ? G[(size_t)r * B + q] : G[(size_t)q * B + r];
            s += gq * (sv - other[(size_t)q * n + k]);
        }
        out[(size_t)r * n + k] = 2.f * s;
    }
}


// Conv2d(k=4, s=2) filter <-> the 3x3 filter over space-to-depth(2) channels the MFMA conv kernels take
// (model/cvig_baseline.py:236-252: channel (dy*2+dx)*ci + c of the space-to-depth image is pixel (2y+dy, 2x+dx), so tap (a+1, b+1),
// a, b in {0,1}, holds w[co][c][2a+dy][2b+dx]; tap row 0 and tap column 0 are zero). One launch each way instead of a zero fill and
// four strided copies per layer and step.
__global__ void conv4x4_to_k3_kernel(const float* __restrict__ w, float* __restrict__ k3, int ci, int cpad, size_t total) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int tap = idx % 9;
    size_t t = idx / 9;
    const int ch = t % cpad;
    const size_t co = t / cpad;
    const int kh = tap / 3, kw = tap % 3;
    float v = 0.f;
    if (kh >= 1 && kw >= 1 && ch < 4 * ci) {
        const int d = ch / ci, c = ch - d * ci;
        v = w[((co * ci + c) * 4 + 2 * (kh - 1) + (d >> 1)) * 4 + 2 * (kw - 1) + (d & 1)];
    }
    k3[idx] = v;
}

__global__ void k3_to_conv4x4_kernel(const float* __restrict__ k3, float* __restrict__ w, int ci, int cpad, size_t total) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int kx = idx & 3, ky = (idx >> 2) & 3;
    const size_t t = idx >> 4;
    const int c = t % ci;
    const size_t co = t / ci;
    const int ch = ((ky & 1) * 2 + (kx & 1)) * ci + c;
    w[idx] = k3[((co * cpad + ch) * 3 + (ky >> 1) + 1) * 3 + (kx >> 1) + 1];
}

// Both mosaic entry points: fp32 stores 4 channels per thread, bf16 stores 8 when C allows it
template <typename OUT>
int s2d_mosaic_launch(const char* what, const float* x, OUT* y, int B, int H, int W, int C, int g, void* stream) {
    WITW_CHECK_ARG(x && y, "%s: null pointer", what);
    WITW_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && (C & 3) == 0 && g >= 1 && g <= 64, "%s: bad shape", what);
    const int V = (sizeof(OUT) == 2 && (C & 7) == 0) ? 8 : 4;
    const size_t total = (size_t)cdiv(B, g * g) * (g * ((H + 1) / 2)) * (g * ((W + 1) / 2)) * 4 * (C / V);
    WITW_CHECK_ARG((total + 255) / 256 <= 0x7fffffffULL, "%s: tensor too large", what);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (V == 4) hipLaunchKernelGGL((s2d_mosaic_kernel<OUT, 4>), grid, dim3(256), 0, (hipStream_t)stream, x, y, B, H, W, C, g, total);
    else if constexpr (sizeof(OUT) == 2)
        hipLaunchKernelGGL((s2d_mosaic_kernel<OUT, 8>), grid, dim3(256), 0, (hipStream_t)stream, x, y, B, H, W, C, g, total);
    WITW_CHECK_LAUNCH(what);
    return WITW_OK;
}

}  // namespace

extern "C" {

int witw_space_to_depth2(const float* x, float* y, int B, int Hp, int Wp, int H, int W, int C, int Cpad, int in_nchw,
                         int normalize, const float* scale, const float* shift, void* stream) {
    WITW_CHECK_ARG(x && y, "space_to_depth2: null pointer");
    WITW_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && H <= Hp && W <= Wp && Cpad >= 4 * C, "space_to_depth2: bad shape");
    const size_t total = (size_t)B * ((H + 1) / 2) * ((W + 1) / 2) * Cpad;
    WITW_CHECK_ARG((total + 255) / 256 <= 0x7fffffffULL, "space_to_depth2: tensor too large");
    if (!in_nchw && !normalize && (C & 3) == 0 && Cpad == 4 * C)
        hipLaunchKernelGGL((space_to_depth2_quad_kernel<float, 4>), dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0,
                           (hipStream_t)stream, x, y, Hp, Wp, H, W, C, total / 4, scale, shift);
    else
        hipLaunchKernelGGL(space_to_depth2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, B,
                           Hp, Wp, H, W, C, Cpad, in_nchw, normalize, total, scale, shift);
    WITW_CHECK_LAUNCH("space_to_depth2");
    return WITW_OK;
}

// x fp32 NHWC [B,Hp,Wp,C] (C % 4 == 0) with valid region H x W, scale / shift fp32 [C] or both NULL -> y bf16 [B, ceil(H/2), ceil(W/2), 4C]
int witw_space_to_depth2_bf16(const float* x, void* y_bf16, int B, int Hp, int Wp, int H, int W, int C, const float* scale,
                              const float* shift, void* stream) {
    WITW_CHECK_ARG(x && y_bf16, "space_to_depth2_bf16: null pointer");
    WITW_CHECK_ARG(B > 0 && C > 0 && (C & 3) == 0 && H > 0 && W > 0 && H <= Hp && W <= Wp, "space_to_depth2_bf16: bad shape (C=%d must be a multiple of 4)", C);
    WITW_CHECK_ARG((scale == nullptr) == (shift == nullptr), "space_to_depth2_bf16: scale and shift go together");
    const int V = (C & 7) == 0 ? 8 : 4;
    const size_t total = (size_t)B * ((H + 1) / 2) * ((W + 1) / 2) * 4 * (C / V);
    WITW_CHECK_ARG((total + 255) / 256 <= 0x7fffffffULL, "space_to_depth2_bf16: tensor too large");
    const dim3 grid((unsigned)((total + 255) / 256));
    if (V == 8)
        hipLaunchKernelGGL((space_to_depth2_quad_kernel<__bf16, 8>), grid, dim3(256), 0, (hipStream_t)stream, x, (__bf16*)y_bf16, Hp, Wp, H, W, C,
                           total, scale, shift);
    else
        hipLaunchKernelGGL((space_to_depth2_quad_kernel<__bf16, 4>), grid, dim3(256), 0, (hipStream_t)stream, x, (__bf16*)y_bf16, Hp, Wp, H, W, C,
                           total, scale, shift);
    WITW_CHECK_LAUNCH("space_to_depth2_bf16");
    return WITW_OK;
}

int witw_space_to_depth2_mosaic(const float* x, float* y, int B, int H, int W, int C, int g, void* stream) {
    return s2d_mosaic_launch("space_to_depth2_mosaic", x, y, B, H, W, C, g, stream);
}

// witw_space_to_depth2_mosaic with a bf16 output: x fp32 NHWC [B,H,W,C] -> y bf16 [ceil(B/g^2), g*ceil(H/2), g*ceil(W/2), 4C], one
// nearest-even rounding, +0.0 where no source exists.
int witw_space_to_depth2_mosaic_bf16(const float* x, void* y_bf16, int B, int H, int W, int C, int g, void* stream) {
    return s2d_mosaic_launch("space_to_depth2_mosaic_bf16", x, (__bf16*)y_bf16, B, H, W, C, g, stream);
}

// ws: the [ksplit][Bm, g*h, g*w, C] partial sums witw_conv3x3_fwd_taps4_ex(ksplit > 1) wrote for B images laid out as g x g
// mosaics of h x w maps (g = 1: plain batch); y [B, vh, vw, C] = the (vh, vw) valid outputs of every image after bias, activation
// (0 none, 1 ReLU, 2 LeakyReLU) and the optional per-channel affine.
int witw_taps4_splitk_finish(const float* ws, int ksplit, const float* bias, int act, float lrelu_slope, const float* post_scale,
                             const float* post_shift, float* y, int B, int g, int h, int w, int vh, int vw, int C, void* stream) {
    WITW_CHECK_ARG(ws && bias && y, "taps4_splitk_finish: null pointer");
    WITW_CHECK_ARG(B > 0 && g >= 1 && h > 0 && w > 0 && vh > 0 && vw > 0 && vh <= h && vw <= w && C > 0 && (C & 3) == 0 && ksplit >= 1,
                   "taps4_splitk_finish: bad shape B=%d g=%d map %dx%d valid %dx%d C=%d ksplit=%d", B, g, h, w, vh, vw, C, ksplit);
    WITW_CHECK_ARG(act >= 0 && act <= 2, "taps4_splitk_finish: activation %d unknown", act);
    WITW_CHECK_ARG((post_scale == nullptr) == (post_shift == nullptr), "taps4_splitk_finish: post_scale and post_shift go together");
    const size_t stride = (size_t)cdiv(B, g * g) * (g * h) * (g * w) * C;
    const size_t total4 = (size_t)B * vh * vw * (C / 4);
    WITW_CHECK_ARG((total4 + 255) / 256 <= 0x7fffffffULL, "taps4_splitk_finish: tensor too large");
    hipLaunchKernelGGL(splitk_finish_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws, ksplit,
                       stride, bias, act, lrelu_slope, post_scale, post_shift, y, B, g, h, w, vh, vw, C, total4);
    WITW_CHECK_LAUNCH("taps4_splitk_finish");
    return WITW_OK;
}

int witw_gem_pool(const float* x, float* f, int B, int Hp, int Wp, int H, int W, int C, int ldf, int col0, float p,
                  const float* scale, const float* shift, void* stream) {
    WITW_CHECK_ARG(x && f, "gem_pool: null pointer");
    WITW_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && H <= Hp && W <= Wp && col0 >= 0 && col0 + C <= ldf, "gem_pool: bad shape");
    hipLaunchKernelGGL(gem_pool_kernel, dim3(B, cdiv(C, 64)), dim3(64 * GEM_PH), 0, (hipStream_t)stream, x, f, B, Hp, Wp, H, W, C, ldf,
                       col0, p, scale, shift);
    WITW_CHECK_LAUNCH("gem_pool");
    return WITW_OK;
}

int witw_embed_normalize(float* f, int B, int n, void* stream) {
    WITW_CHECK_ARG(f && B > 0 && n > 0, "embed_normalize: bad argument");
    hipLaunchKernelGGL(embed_normalize_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, f, n);
    WITW_CHECK_LAUNCH("embed_normalize");
    return WITW_OK;
}

int witw_pairwise_sqdist(const float* a, const float* b, float* D, int Na, int Nb, int n, int take_sqrt, void* stream) {
    WITW_CHECK_ARG(a && b && D, "pairwise_sqdist: null pointer");
    WITW_CHECK_ARG(Na > 0 && Nb > 0 && n > 0 && n <= 12288 && Na <= 65535, "pairwise_sqdist: bad shape Na=%d Nb=%d n=%d", Na, Nb, n);
    hipLaunchKernelGGL(pairwise_sqdist_kernel, dim3(cdiv(Nb, 256), Na), dim3(256), n * sizeof(float), (hipStream_t)stream, a, b, D,
                       Na, Nb, n, take_sqrt);
    WITW_CHECK_LAUNCH("pairwise_sqdist");
    return WITW_OK;
}

// exhaustive_minibatch_triplet_loss from D[i][j] = |embed1_i - embed2_j|^2; workspace: B floats.
int witw_exhaustive_triplet_loss(const float* D, int B, int soft_margin, float alpha, float margin, float* loss, float* workspace,
                                 void* stream) {
    WITW_CHECK_ARG(D && loss && workspace, "exhaustive_triplet_loss: null pointer");
    WITW_CHECK_ARG(B >= 2, "exhaustive_triplet_loss: batch %d < 2", B);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(exhaustive_partials_kernel, dim3(B), dim3(256), 0, st, D, workspace, B,
                       BaselineTerm{soft_margin, alpha, margin});
    hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(256), 0, st, workspace, loss, B, 2.f * B * (B - 1));
    WITW_CHECK_LAUNCH("exhaustive_triplet_loss");
    return WITW_OK;
}

// ---- training-mode entry points of cvig_baseline

long long witw_bn_workspace_floats(int B, int H, int W, int C) {
    const size_t npix = (size_t)B * H * W;
    const int rows = bl_rows(npix);
    long long nparts = (long long)((npix + rows - 1) / rows);
    if (nparts < 1024) nparts = 1024;          // the row-based form writes at most 1024 partials
    return nparts * 2 * C + 2 * C;
}

// Batch statistics of BatchNorm2d over the valid region of a [B,Hp,Wp,C] tensor -> mean, invstd, and the affine
// (scale, shift) with y = a*scale + shift; running stats updated in place when non-NULL (momentum, unbiased var).
int witw_bn_train_stats(const float* a, int B, int Hp, int Wp, int H, int W, int C, const float* gamma, const float* beta,
                        float eps, float momentum, float* mean, float* invstd, float* scale, float* shift, float* running_mean,
                        float* running_var, float* workspace, void* stream) {
    WITW_CHECK_ARG(a && gamma && beta && mean && invstd && scale && shift && workspace, "bn_train_stats: null pointer");
    WITW_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && H <= Hp && W <= Wp, "bn_train_stats: bad shape");
    WITW_CHECK_ARG((size_t)B * H * W > 1, "bn_train_stats: needs more than one value per channel");
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)B * H * W;
    const int nparts = bl_launch_sums(a, nullptr, nullptr, nullptr, a, workspace, B, Hp, Wp, H, W, C, st);      // pivot: a[0,0,0,c]
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3(cdiv(C, BNF_CH)), dim3(BNF_CH * BNF_LANES), 0, st, workspace, nparts, C, (float)npix, a, gamma, beta,
                       eps, momentum, mean, invstd, scale, shift, running_mean, running_var);
    WITW_CHECK_LAUNCH("bn_train_stats");
    return WITW_OK;
}

// Backward of y = BN_train(lrelu(z)) w.r.t. z, gamma, beta: a = lrelu(z) (saved), dy = gradient at y.
// dy_s2d_cp > 0: dy is still the space-to-depth image the next block's data-gradient conv wrote ([B, ceil(H/2), ceil(W/2), dy_s2d_cp],
// channel ((h&1)*2+(w&1))*C + c) and is read in place (no witw_depth_to_space2 pass); 0: dy is [B,Hp,Wp,C] like a.
int witw_bn_lrelu_bwd_ex(const float* a, const float* dy, float* dz, float* dgamma, float* dbeta, const float* mean,
                         const float* invstd, const float* gamma, int B, int Hp, int Wp, int H, int W, int C, float slope,
                         int dy_s2d_cp, float* workspace, void* stream) {
    WITW_CHECK_ARG(a && dy && dz && dgamma && dbeta && mean && invstd && gamma && workspace, "bn_lrelu_bwd: null pointer");
    WITW_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && H <= Hp && W <= Wp, "bn_lrelu_bwd: bad shape");
    WITW_CHECK_ARG(dy_s2d_cp == 0 || (dy_s2d_cp >= 4 * C && (dy_s2d_cp % 4) == 0), "bn_lrelu_bwd: space-to-depth channel stride %d for C=%d", dy_s2d_cp, C);
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)B * H * W;
    const int nparts = bl_launch_sums(a, dy, mean, invstd, nullptr, workspace, B, Hp, Wp, H, W, C, st, dy_s2d_cp);
    float* sums = workspace + (size_t)nparts * 2 * C;
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3(cdiv(C, BNF_CH)), dim3(BNF_CH * BNF_LANES), 0, st, workspace, nparts, C, sums, dgamma, dbeta);
    bl_launch_apply(a, dy, dz, mean, invstd, gamma, sums, (float)npix, B, Hp, Wp, H, W, C, slope, dy_s2d_cp, st);
    WITW_CHECK_LAUNCH("bn_lrelu_bwd");
    return WITW_OK;
}

int witw_bn_lrelu_bwd(const float* a, const float* dy, float* dz, float* dgamma, float* dbeta, const float* mean,
                      const float* invstd, const float* gamma, int B, int Hp, int Wp, int H, int W, int C, float slope,
                      float* workspace, void* stream) {
    return witw_bn_lrelu_bwd_ex(a, dy, dz, dgamma, dbeta, mean, invstd, gamma, B, Hp, Wp, H, W, C, slope, 0, workspace, stream);
}

int witw_depth_to_space2(const float* g, const float* add, float* dx, int B, int Hp, int Wp, int H, int W, int C, int Cpad,
                         void* stream) {
    WITW_CHECK_ARG(g && dx, "depth_to_space2: null pointer");
    WITW_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && H <= Hp && W <= Wp && Cpad >= 4 * C, "depth_to_space2: bad shape");
    const size_t total = (size_t)B * Hp * Wp * C;
    hipLaunchKernelGGL(depth_to_space2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, add, dx,
                       Hp, Wp, H, W, C, Cpad, total);
    WITW_CHECK_LAUNCH("depth_to_space2");
    return WITW_OK;
}

int witw_gem_pool_bwd(const float* a, const float* scale, const float* shift, const float* f, const float* df, float* dy, int B,
                      int Hp, int Wp, int H, int W, int C, int ldf, int col0, float p, int accumulate, void* stream) {
    WITW_CHECK_ARG(a && scale && shift && f && df && dy, "gem_pool_bwd: null pointer");
    WITW_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && H <= Hp && W <= Wp, "gem_pool_bwd: bad shape");
    const size_t total = (size_t)B * Hp * Wp * C;
    hipLaunchKernelGGL(gem_pool_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, scale, shift,
                       f, df, dy, Hp, Wp, H, W, C, ldf, col0, p, accumulate, total);
    WITW_CHECK_LAUNCH("gem_pool_bwd");
    return WITW_OK;
}

// g: the un-normalised concat feature [B,n]; df: gradient at f = g/|g|^(1/2); dg out.
int witw_embed_normalize_bwd(const float* g, const float* df, float* dg, int B, int n, void* stream) {
    WITW_CHECK_ARG(g && df && dg && B > 0 && n > 0, "embed_normalize_bwd: bad argument");
    hipLaunchKernelGGL(embed_normalize_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, g, df, dg, n);
    WITW_CHECK_LAUNCH("embed_normalize_bwd");
    return WITW_OK;
}

// backward of witw_pairwise_sqdist + witw_exhaustive_triplet_loss: grad_loss [1] -> de1, de2 [B,n]; workspace B*B floats.
int witw_exhaustive_triplet_loss_bwd(const float* e1, const float* e2, const float* D, const float* grad_loss, float* de1,
                                     float* de2, int B, int n, int soft_margin, float alpha, float margin, float* workspace,
                                     void* stream) {
    WITW_CHECK_ARG(e1 && e2 && D && grad_loss && de1 && de2 && workspace, "exhaustive_triplet_loss_bwd: null pointer");
    WITW_CHECK_ARG(B >= 2 && n > 0, "exhaustive_triplet_loss_bwd: bad shape");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(exhaustive_bwd_kernel, dim3(B), dim3(256), 0, st, D, grad_loss, workspace, B,
                       BaselineTerm{soft_margin, alpha, margin});
    hipLaunchKernelGGL(sqdist_bwd_kernel, dim3(B), dim3(256), 0, st, e1, e2, workspace, de1, B, n, 0);
    hipLaunchKernelGGL(sqdist_bwd_kernel, dim3(B), dim3(256), 0, st, e1, e2, workspace, de2, B, n, 1);
    WITW_CHECK_LAUNCH("exhaustive_triplet_loss_bwd");
    return WITW_OK;
}

// w [co][ci][4][4] (torch layout of Conv2d(ci, co, 4, 2)) -> k3 [co][cpad][3][3], cpad >= 4*ci (extra channels zero)
int witw_conv4x4_to_k3(const float* w, float* k3, int co, int ci, int cpad, void* stream) {
    WITW_CHECK_ARG(w && k3 && co > 0 && ci > 0 && cpad >= 4 * ci, "conv4x4_to_k3: bad arguments");
    const size_t total = (size_t)co * cpad * 9;
    hipLaunchKernelGGL(conv4x4_to_k3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, k3, ci, cpad, total);
    WITW_CHECK_LAUNCH("conv4x4_to_k3");
    return WITW_OK;
}

// the inverse gather (a weight gradient in the k3 layout -> the Conv2d parameter's layout)
int witw_k3_to_conv4x4(const float* k3, float* w, int co, int ci, int cpad, void* stream) {
    WITW_CHECK_ARG(w && k3 && co > 0 && ci > 0 && cpad >= 4 * ci, "k3_to_conv4x4: bad arguments");
    const size_t total = (size_t)co * ci * 16;
    hipLaunchKernelGGL(k3_to_conv4x4_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, k3, w, ci, cpad, total);
    WITW_CHECK_LAUNCH("k3_to_conv4x4");
    return WITW_OK;
}

}  // extern "C"
