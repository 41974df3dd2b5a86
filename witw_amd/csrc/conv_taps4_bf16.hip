// 2x2-tap convolution, NHWC bf16 operands / fp32 accumulate, implicit GEMM on v_mfma_f32_16x16x32_bf16 (gfx950): blocks 2-4 of
// cvig_baseline's encoders at inference (model/cvig_baseline.py:236-252, 267-275: Conv2d(k=4, s=2) over an activation = the taps
// {1,2}^2 of a 3x3 filter over its space-to-depth(2) image, witw_conv4x4_to_k3), bias -> LeakyReLU -> eval-mode BatchNorm affine in
// the epilogue, which writes the NEXT block's space-to-depth image directly (the layout of witw_conv3x3_fwd_taps4_ex with s2d != 0).
//
//   out[b, oy, ox, n] = sum_{ty,tx in {0,1}} sum_c x[b, oy+ty, ox+tx, c] * k3[n, c, 1+ty, 1+tx]       (x zero past H / W)
//
// Workgroup: 4 waves, 8 rows x 32 columns of outputs x 128 channels. Blocks 2 / 3 / 4 store 126 / 62 / 30 rows and columns at config 1's
// 512 x 512 inputs and 124 / 60 / 30 at its 500 x 500 ones, inside tiles covering 128 / 64 / 32: the 8 x 32 tile pads 3 / 6 / 12 % of the
// first and 6 / 12 / 12 % of the second, where a 64-column tile would pad block 4 by 53 %.
// K: a chunk of 16 channels x 4 taps is exactly two MFMAs' K = 32: step ty = tap row ty, lane l of a fragment holds 8 channels
// (group (l >> 4) & 1) of tap column l >> 5 for pixel / output channel l & 15 -- the k order of conv3x3_bf16_s16_kernel's tap
// pairs, with no ninth tap to share. Wave w: rows 2w, 2w+1 = 4 pixel tiles of 16 columns, times 8 channel tiles: 32 accumulators.
// Staging as in conv3x3_bf16.hip: the 9 x 33 halo tile goes global -> VGPR -> LDS (two planes of 8 channels, plane pitch a multiple
// of 16 slots: the conflict-free pitch of the s16 kernel), the 16 KB weight slab by LDS-DMA (the packed image is the LDS image), two
// stages, one barrier per chunk. The fragment reads are left to the compiler (DESIGN.md 4.11 says what that leaves).
//
// PLAIN form (training, blocks 2-4 under train_precision='bf16'): the same tile, staging and K loop, another store: fp32 [B,H,W,Cout] in
// the plain NHWC layout the BatchNorm kernels read, +0.0 outside the valid region, bias / LeakyReLU optional, and a tap base:
//   out[b, oy, ox, n] = sum_{ty,tx in {0,1}} sum_c x[b, oy+ty-off, ox+tx-off, c] * wpk[n, c, tap ty*2+tx]      off = 1 - tap_base
// tap_base = 1 is the forward above; tap_base = 0 with a transpose_flip-packed filter is its data gradient (x zero outside [0,H) x [0,W)).
#include "common.h"
#include "conv_launch.h"
#include "lds_frag.h"
#include <type_traits>

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int T4_TW = 32, T4_TH = 8, T4_TN = 128, T4_NW = 4;

struct Taps4BfArgs {
    const unsigned short* x;    // [B,H,W,Cin] NHWC bf16, Cin % 16 == 0
    const unsigned short* wpk;  // packed bf16: [n_tile][cin/16][tap = ty*2+tx][group][128][8]
    const float* bias;          // [Cout] fp32
    const float* post_scale;    // [Cout] fp32 or nullptr (then post_shift is nullptr too)
    const float* post_shift;
    void* y;                    // [B, s2d_h, s2d_w, 4*Cout] bf16 or fp32
    int B, H, W, Cin, Cout;
    int Ho, Wo;                 // computed outputs: 2*s2d_h x 2*s2d_w
    int s2d_h, s2d_w, valid_h, valid_w;
    int tiles_x, tiles_y;
    int n_tiles, sp_total, sp_per_xcd, xcd_map;
    float slope;
    int off, act;               // PLAIN only: halo shift 1 - tap_base; LeakyReLU on / off
};

template <bool OUT_F32, bool PLAIN = false>
__global__ __launch_bounds__(64 * T4_NW) void conv_taps4_bf16_kernel(Taps4BfArgs p) {
    constexpr int TW = T4_TW, TH = T4_TH, TN = T4_TN, NW = T4_NW, NTHREADS = 64 * NW;
    constexpr int IH = TH + 1, IW = TW + 1;
    constexpr int PL = (IH * IW + 15) / 16 * 16;      // plane pitch: a multiple of 16 slots (conv3x3_bf16_s16_kernel)
    constexpr int IN_S = 2 * PL;
    constexpr int IN_P = (IN_S + 63) / 64 * 64;
    constexpr int W_S = 4 * 2 * TN;                   // 16-B slots of one weight stage: 16 wave instructions of LDS-DMA
    constexpr int STAGE_S = IN_P + W_S;
    constexpr int NIN = (IN_S + NTHREADS - 1) / NTHREADS;
    constexpr int NWT_D = W_S / 64 / NW;
    constexpr unsigned OOR = 0x80000000u;
    constexpr int SLAB_P = 68;      // floats per slab row: 64 channels + 4
    static_assert(W_S % (64 * NW) == 0, "every wave moves the same number of weight pieces");
    static_assert(2 * STAGE_S * 16 >= NW * 32 * SLAB_P * 4, "the stages must hold one epilogue slab per wave");

    __shared__ u32x4 smem[2 * STAGE_S + 1];
    u32x4* const stageA = smem;
    u32x4* const stageB = smem + STAGE_S;
    u32x4* const dummy_slot = smem + 2 * STAGE_S;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave) & (NW - 1);
    const int l15 = lane & 15, kg = lane >> 4;
    const int sel = kg >> 1, grp = kg & 1;      // tap column / 8-channel group of this lane's k values

    // block -> (n tile, spatial tile): XCD-aware order, see conv3x3.hip (block i runs on XCD i % 8)
    int ntile, sp;
    if (p.xcd_map) {
        const int g = blockIdx.x >> 3;
        ntile = g % p.n_tiles;
        sp = (blockIdx.x & 7) * p.sp_per_xcd + g / p.n_tiles;
        if (sp >= p.sp_total) return;
    } else {
        ntile = blockIdx.x / p.sp_total;
        sp = blockIdx.x - ntile * p.sp_total;
    }
    const int tiles_img = p.tiles_x * p.tiles_y;
    const int b = sp / tiles_img;
    sp -= b * tiles_img;
    const int ty_ = sp / p.tiles_x;
    const int tx_ = sp - ty_ * p.tiles_x;
    const int oy0 = ty_ * TH, ox0 = tx_ * TW, n0 = ntile * TN;
    const int nkc = p.Cin >> 4;

    // ---- staging: input tile through registers (range-checked buffer loads: padding is a load policy), weight slab by LDS-DMA
    const size_t img_elems = (size_t)p.H * p.W * p.Cin;
    __amdgpu_buffer_rsrc_t in_rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + (size_t)b * img_elems), 0, (unsigned)(img_elems * 2), 0x00020000);
    const i32x4 w_rd = raw_rsrc(reinterpret_cast<const u32x4*>(p.wpk) + (size_t)ntile * nkc * W_S, (unsigned)nkc * W_S * 16u);
    unsigned gin[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
        const int s = tid + i * NTHREADS;
        const int pix = s >> 1, q = s & 1;
        const int r = pix / IW, c = pix - r * IW;
        int gr = oy0 + r, gc = ox0 + c;
        bool ok = pix < IH * IW && gr < p.H && gc < p.W;
        if constexpr (PLAIN) {      // tap_base = 0: the halo row / column lie before the tile, and before the image they are zeros
            gr -= p.off;
            gc -= p.off;
            ok = pix < IH * IW && gr >= 0 && gr < p.H && gc >= 0 && gc < p.W;
        }
        gin[i] = ok ? (unsigned)((((size_t)gr * p.W + gc) * p.Cin + q * 8) * 2) : OOR;
    }
    u32x4 rin[NIN];
    const unsigned lane16 = (unsigned)lane * 16u;
    auto stage_load = [&](int kc, u32x4* in_s) {
#pragma unroll
        for (int i = 0; i < NIN; ++i) rin[i] = __builtin_amdgcn_raw_buffer_load_b128(in_rs, gin[i], (unsigned)kc * 32u, 0);
        const unsigned in_lds = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_address(in_s));
#pragma unroll
        for (int d = 0; d < NWT_D; ++d) {
            const int j = wave_u + NW * d;
            dma16(w_rd, in_lds + (unsigned)(IN_P + j * 64) * 16u, lane16, (unsigned)kc * W_S * 16u + (unsigned)j * 1024u);
        }
    };
    auto stage_commit = [&](u32x4* in_s) {
#pragma unroll
        for (int i = 0; i < NIN; ++i) {
            const int s = tid + i * NTHREADS;
            u32x4* dst = (s >> 1) < IH * IW ? in_s + (s & 1) * PL + (s >> 1) : dummy_slot;
            *dst = rin[i];
        }
    };
    auto stage_wait = [&]() { __builtin_amdgcn_s_waitcnt(0x0F70); };      // vmcnt(0): this wave's LDS-DMA pieces have landed

    // ---- this wave's tiles: pixel tile a (0..3) = row 2*wave + (a >> 1), columns 16*(a & 1) ..+15; channel tile bt (0..7)
    const int a_lane = grp * PL + 2 * wave * IW + l15 + sel;
    const int w_lane = IN_P + sel * 2 * TN + grp * TN + l15;

    f32x4 acc[4][8];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int bt = 0; bt < 8; ++bt) acc[a][bt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // one K chunk: two K = 32 steps (tap rows) out of stage `in_s` while chunk kc + 1 moves into stage `in_n`
    auto chunk = [&](const u32x4* in_s, u32x4* in_n, int kc) {
        const int kn = (kc + 1 < nkc) ? kc + 1 : kc;      // behind the last chunk the other stage is refilled with it (never read)
        stage_load(kn, in_n);
#pragma unroll
        for (int ty = 0; ty < 2; ++ty) {
            u32x4 fa[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) fa[a] = in_s[a_lane + ((a >> 1) + ty) * IW + 16 * (a & 1)];
#pragma unroll
            for (int bt = 0; bt < 8; ++bt) {
                const u32x4 fb = in_s[w_lane + ty * 4 * TN + 16 * bt];
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    acc[a][bt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa[a]), __builtin_bit_cast(bf16x8, fb),
                                                                         acc[a][bt], 0, 0, 0);
            }
        }
        stage_commit(in_n);
        stage_wait();
        __syncthreads();
    };

    stage_load(0, stageA);
    stage_commit(stageA);
    stage_wait();
    __syncthreads();
    for (int kc = 0; kc < nkc; kc += 2) {
        chunk(stageA, stageB, kc);
        if (kc + 1 < nkc) chunk(stageB, stageA, kc + 1);
    }
    // every wave is behind the last chunk's barrier and nothing is in flight: the slabs below reuse the stages

    // ---- epilogue: bias -> LeakyReLU -> affine in fp32, one rounding at the store; register r of lane l of a tile = pixel
    // 4*(l >> 4) + r, channel l & 15. 32 pixels of a row x 64 channels at a time through a wave-private fp32 slab, 8 channels per lane out
    float* slab = reinterpret_cast<float*>(smem) + wave * (32 * SLAB_P);
    const bool has_post = p.post_scale != nullptr;
    const int prow = lane >> 3, pc8 = (lane & 7) * 8;
    const bool wide = (p.Cout & 7) == 0;
    typedef typename std::conditional<OUT_F32, float, __bf16>::type out_t;
    out_t* const yo = reinterpret_cast<out_t*>(p.y);
#pragma unroll
    for (int hn = 0; hn < 2; ++hn) {
        float bv[4], ps[4], pt[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ch = n0 + 64 * hn + 16 * j + l15;
            const bool in = ch < p.Cout;
            bv[j] = (in && (!PLAIN || p.bias != nullptr)) ? p.bias[ch] : 0.f;
            ps[j] = (in && has_post) ? p.post_scale[ch] : 1.f;
            pt[j] = (in && has_post) ? p.post_shift[ch] : 0.f;
        }
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = acc[2 * rr + i][4 * hn + j][r] + bv[j];
                        if (!PLAIN || p.act) v = v > 0.f ? v : v * p.slope;
                        if (has_post) v = v * ps[j] + pt[j];
                        slab[(16 * i + 4 * kg + r) * SLAB_P + 16 * j + l15] = v;
                    }
            const int yy = oy0 + 2 * wave + rr;
            const int nbase = n0 + 64 * hn + pc8;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int m = g * 8 + prow;
                f32x4 v0 = *reinterpret_cast<const f32x4*>(slab + m * SLAB_P + pc8);
                f32x4 v1 = *reinterpret_cast<const f32x4*>(slab + m * SLAB_P + pc8 + 4);
                const int xx = ox0 + m;
                if (!(yy < p.valid_h && xx < p.valid_w)) v0 = v1 = f32x4{0.f, 0.f, 0.f, 0.f};      // +0.0 outside the valid region
                if (yy < p.Ho && xx < p.Wo && nbase < p.Cout) {
                    const size_t o = PLAIN
                        ? (((size_t)b * p.Ho + yy) * p.Wo + xx) * p.Cout + nbase
                        : ((((size_t)b * p.s2d_h + (yy >> 1)) * p.s2d_w + (xx >> 1)) * 4 + (yy & 1) * 2 + (xx & 1)) * p.Cout + nbase;
                    if (wide) {
                        if constexpr (OUT_F32) {
                            __builtin_nontemporal_store(v0, reinterpret_cast<f32x4*>(yo + o));
                            __builtin_nontemporal_store(v1, reinterpret_cast<f32x4*>(yo + o + 4));
                        } else {
                            bf16x8 ob;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                ob[e] = (__bf16)v0[e];
                                ob[4 + e] = (__bf16)v1[e];
                            }
                            __builtin_nontemporal_store(ob, reinterpret_cast<bf16x8*>(yo + o));
                        }
                    } else {      // ragged Cout: one element at a time
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (nbase + e < p.Cout) yo[o + e] = (out_t)(e < 4 ? v0[e & 3] : v1[e & 3]);
                    }
                }
            }
        }
    }
}

// wpk[nt][kc][tap = ty*2+tx][g][n][0..7] (bf16, nearest-even) <- w[cout][cin][1+ty][1+tx] (fp32, torch KCRS); one thread per 16-B slot.
// transpose_flip: the data-gradient filter instead, as pack_weights_kernel of conv3x3.hip builds it: (Cout, Cin) describe the PACKED
// filter, the source is [Cin][Cout][3][3], tap (ty, tx) holds w[ci][co][2-ty][2-tx] (taps {0,1}^2 of the transposed, rotated filter)
__global__ void pack_weights_taps4_bf16_kernel(const float* __restrict__ w, unsigned short* __restrict__ wpk, int Cout, int Cin, int nkc,
                                               size_t total, int transpose_flip) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    size_t t = idx;
    const int n = t % T4_TN; t /= T4_TN;
    const int g = t % 2; t /= 2;
    const int tap = t % 4; t /= 4;
    const int kc = t % nkc; t /= nkc;
    const int co = (int)t * T4_TN + n;
    const int kh = transpose_flip ? 2 - (tap >> 1) : 1 + (tap >> 1), kw = transpose_flip ? 2 - (tap & 1) : 1 + (tap & 1);
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = kc * 16 + g * 8 + j;
        const size_t src = transpose_flip ? (size_t)ci * Cout + co : (size_t)co * Cin + ci;
        v[j] = (__bf16)((co < Cout && ci < Cin) ? w[(src * 3 + kh) * 3 + kw] : 0.f);
    }
    reinterpret_cast<bf16x8*>(wpk)[idx] = v;
}

// y[i] = bf16(x[i]), nearest-even: four elements per thread, the tail one at a time
__global__ void f32_to_bf16_kernel(const float* __restrict__ x, unsigned short* __restrict__ y, size_t n) {
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    const size_t i4 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 + 4 <= n) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + i4);
        bf16x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (__bf16)v[j];
        *reinterpret_cast<bf16x4*>(y + i4) = o;
    } else {
        __bf16* yb = reinterpret_cast<__bf16*>(y);
        for (size_t i = i4; i < n; ++i) yb[i] = (__bf16)x[i];
    }
}

template <bool OUT_F32, bool PLAIN = false>
int launch_taps4_bf(Taps4BfArgs a, hipStream_t st) {
    const long long grid = witw_conv_grid(a, T4_TH, T4_TN, PLAIN ? "conv3x3_bf16_fwd_taps4_plain" : "conv3x3_bf16_fwd_taps4");
    if (!grid) return WITW_ERR_INVALID;
    hipLaunchKernelGGL((conv_taps4_bf16_kernel<OUT_F32, PLAIN>), dim3((unsigned)grid), dim3(64 * T4_NW), 0, st, a);
    WITW_CHECK_LAUNCH("conv_taps4_bf16");
    if (PLAIN) witw_note_variant("conv_taps4_bf16_kernel<true,true>");
    else witw_note_variant("conv_taps4_bf16_kernel<%s>", OUT_F32 ? "true" : "false");
    return WITW_OK;
}

}  // namespace

extern "C" {

long long witw_conv3x3_bf16_packed_elems_taps4(int cout, int cin) {
    if (cout <= 0 || cin <= 0) return -1;
    return (long long)cdiv(cout, T4_TN) * cdiv(cin, 16) * 4 * 2 * T4_TN * 8;
}

int witw_conv3x3_bf16_pack_weights_taps4_ex(const float* w_kcrs, void* wpk_bf16, int cout, int cin, int transpose_flip, void* stream) {
    WITW_CHECK_ARG(w_kcrs && wpk_bf16, "bf16 pack_weights_taps4: null pointer");
    WITW_CHECK_ARG(cout > 0 && cin > 0, "bf16 pack_weights_taps4: bad shape cout=%d cin=%d", cout, cin);
    const int nkc = cdiv(cin, 16);
    const size_t total = (size_t)cdiv(cout, T4_TN) * nkc * 4 * 2 * T4_TN;
    WITW_CHECK_ARG((total + 255) / 256 <= 0x7fffffffull, "bf16 pack_weights_taps4: grid too large");
    hipLaunchKernelGGL(pack_weights_taps4_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_kcrs,
                       (unsigned short*)wpk_bf16, cout, cin, nkc, total, transpose_flip != 0);
    WITW_CHECK_LAUNCH("bf16 pack_weights_taps4");
    return WITW_OK;
}

int witw_conv3x3_bf16_pack_weights_taps4(const float* w_kcrs, void* wpk_bf16, int cout, int cin, void* stream) {
    return witw_conv3x3_bf16_pack_weights_taps4_ex(w_kcrs, wpk_bf16, cout, cin, 0, stream);
}

// x NHWC bf16 [B,H,W,Cin] (Cin % 16 == 0), wpk from witw_conv3x3_bf16_pack_weights_taps4, bias / post_scale / post_shift fp32 [Cout]
// -> y [B, ceil(valid_h/2), ceil(valid_w/2), 4*Cout], bf16 (out_f32 == 0) or fp32: the space-to-depth(2) image of
// lrelu(conv + bias) * post_scale + post_shift over the valid_h x valid_w region, channel ((row&1)*2 + (col&1))*Cout + c, +0.0 outside.
int witw_conv3x3_bf16_fwd_taps4(const void* x_bf16, const void* wpk_bf16, const float* bias, const float* post_scale,
                                const float* post_shift, void* y, int B, int H, int W, int Cin, int Cout, float lrelu_slope,
                                int valid_h, int valid_w, int out_f32, void* stream) {
    WITW_CHECK_ARG(x_bf16 && wpk_bf16 && bias && y, "conv3x3_bf16_fwd_taps4: null pointer");
    WITW_CHECK_ARG(B > 0 && H >= 2 && W >= 2 && Cout > 0, "conv3x3_bf16_fwd_taps4: bad shape B=%d H=%d W=%d Cout=%d", B, H, W, Cout);
    WITW_CHECK_ARG(Cin > 0 && (Cin % 16) == 0, "conv3x3_bf16_fwd_taps4: Cin=%d must be a positive multiple of 16", Cin);
    WITW_CHECK_ARG((post_scale == nullptr) == (post_shift == nullptr), "conv3x3_bf16_fwd_taps4: post_scale and post_shift go together");
    WITW_CHECK_ARG(valid_h > 0 && valid_w > 0 && valid_h <= H && valid_w <= W,
                   "conv3x3_bf16_fwd_taps4: valid region %dx%d outside the %dx%d map", valid_h, valid_w, H, W);
    WITW_CHECK_ARG((size_t)H * W * Cin * 2 < 0x80000000ull, "conv3x3_bf16_fwd_taps4: image too large for one buffer descriptor");
    WITW_CHECK_ARG((size_t)cdiv(Cout, T4_TN) * Cin * (4 * T4_TN * 2) < 0x80000000ull,
                   "conv3x3_bf16_fwd_taps4: packed filter too large for one buffer descriptor");
    Taps4BfArgs a;
    a.x = (const unsigned short*)x_bf16; a.wpk = (const unsigned short*)wpk_bf16; a.bias = bias;
    a.post_scale = post_scale; a.post_shift = post_shift; a.y = y;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
    a.valid_h = valid_h; a.valid_w = valid_w;
    a.s2d_h = (valid_h + 1) / 2; a.s2d_w = (valid_w + 1) / 2;
    a.Ho = 2 * a.s2d_h; a.Wo = 2 * a.s2d_w;
    a.tiles_x = cdiv(a.Wo, T4_TW);
    a.tiles_y = 0;
    a.slope = lrelu_slope;
    a.off = 0; a.act = 1;
    a.xcd_map = witw_conv_xcd_map();
    hipStream_t st = (hipStream_t)stream;
    return out_f32 ? launch_taps4_bf<true>(a, st) : launch_taps4_bf<false>(a, st);
}

// The PLAIN form: x NHWC bf16 [B,H,W,Cin] (Cin % 16 == 0), wpk from witw_conv3x3_bf16_pack_weights_taps4_ex, bias fp32 [Cout] or NULL
// -> y fp32 [B,H,W,Cout] = act(conv + bias) for rows < valid_h and columns < valid_w, +0.0 elsewhere; every element of y is written.
int witw_conv3x3_bf16_fwd_taps4_plain(const void* x_bf16, const void* wpk_bf16, const float* bias, float* y, int B, int H, int W, int Cin,
                                      int Cout, int lrelu, float lrelu_slope, int tap_base, int valid_h, int valid_w, void* stream) {
    WITW_CHECK_ARG(x_bf16 && wpk_bf16 && y, "conv3x3_bf16_fwd_taps4_plain: null pointer");
    WITW_CHECK_ARG(B > 0 && H > 0 && W > 0 && Cout > 0, "conv3x3_bf16_fwd_taps4_plain: bad shape B=%d H=%d W=%d Cout=%d", B, H, W, Cout);
    WITW_CHECK_ARG(Cin > 0 && (Cin % 16) == 0, "conv3x3_bf16_fwd_taps4_plain: Cin=%d must be a positive multiple of 16", Cin);
    WITW_CHECK_ARG(tap_base == 0 || tap_base == 1, "conv3x3_bf16_fwd_taps4_plain: tap_base=%d must be 0 or 1", tap_base);
    WITW_CHECK_ARG(valid_h > 0 && valid_w > 0 && valid_h <= H && valid_w <= W,
                   "conv3x3_bf16_fwd_taps4_plain: valid region %dx%d outside the %dx%d map", valid_h, valid_w, H, W);
    WITW_CHECK_ARG((size_t)H * W * Cin * 2 < 0x80000000ull, "conv3x3_bf16_fwd_taps4_plain: image too large for one buffer descriptor");
    WITW_CHECK_ARG((size_t)cdiv(Cout, T4_TN) * Cin * (4 * T4_TN * 2) < 0x80000000ull,
                   "conv3x3_bf16_fwd_taps4_plain: packed filter too large for one buffer descriptor");
    Taps4BfArgs a;
    a.x = (const unsigned short*)x_bf16; a.wpk = (const unsigned short*)wpk_bf16; a.bias = bias;
    a.post_scale = nullptr; a.post_shift = nullptr; a.y = y;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
    a.valid_h = valid_h; a.valid_w = valid_w;
    a.s2d_h = 0; a.s2d_w = 0;
    a.Ho = H; a.Wo = W;
    a.tiles_x = cdiv(a.Wo, T4_TW);
    a.tiles_y = 0;
    a.slope = lrelu_slope;
    a.off = 1 - tap_base; a.act = lrelu != 0;
    a.xcd_map = witw_conv_xcd_map();
    return launch_taps4_bf<true, true>(a, (hipStream_t)stream);
}

int witw_f32_to_bf16(const float* x, void* y_bf16, long long n, void* stream) {
    WITW_CHECK_ARG(x && y_bf16 && n > 0, "f32_to_bf16: null pointer or n <= 0");
    const size_t threads = ((size_t)n + 3) / 4;
    WITW_CHECK_ARG((threads + 255) / 256 <= 0x7fffffffULL, "f32_to_bf16: tensor too large");
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                       (unsigned short*)y_bf16, (size_t)n);
    WITW_CHECK_LAUNCH("f32_to_bf16");
    return WITW_OK;
}

}  // extern "C"
