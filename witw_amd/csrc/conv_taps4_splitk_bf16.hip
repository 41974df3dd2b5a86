// Split-K form of the bf16 2x2-tap convolution (conv_taps4_bf16.hip) for blocks 5-7 of cvig_baseline's encoders at inference
// (SurfaceEncoder(precision='bf16_all')): maps of 16 x 16 and below with K = 4 taps x 2048 channels, laid out as g x g mosaics of
// space-to-depth(2) cells (witw_space_to_depth2_mosaic_bf16, baseline.hip; g = 1 is the plain batch block 4 hands over). bf16 operands, fp32
// accumulation on v_mfma_f32_16x16x32_bf16 (gfx950), RAW fp32 partial sums of one K slice per workgroup into a workspace
//
//   ws[s, b, y, x, n] = sum_{c in slice s} sum_{ty,tx in {0,1}} x[b, y+ty, x+tx, c] * k3[n, c, 1+ty, 1+tx]      (x zero past H / W)
//
// which witw_taps4_splitk_finish (baseline.hip) reduces in slice order, finishes (bias -> LeakyReLU -> affine) and gathers.
//
// Workgroup: 4 waves, 16 rows x 16 columns x 128 channels: the mosaic sides of blocks 5 / 6 / 7 are 15 / 14 / 15 at 512 x 512 inputs,
// 15 / 14 / 14 at 500 x 500 and 11 / 15 / 16 at 382 x 382, where the 8 x 32 tile of conv_taps4_bf16_kernel would leave more than half
// its columns empty. Larger maps take cdiv(H,16) x cdiv(W,16) tiles per mosaic image. Wave w: rows 4w..4w+3 = 4 pixel tiles of 16
// columns, times 8 channel tiles: 32 accumulators, the per-wave shape of conv_taps4_bf16_kernel with one pixel tile per row.
// K order, fragments, packed filter image (PackedConvBf16Taps4, unchanged) and staging are that kernel's: the 17 x 17 halo tile goes
// global -> VGPR -> LDS (two planes of 8 channels, plane pitch a multiple of 16 slots), the 16 KB weight slab by LDS-DMA, two stages,
// one barrier per chunk; the fragment reads are left to the compiler.
// Split-K: blockIdx.y = slice s of the Cin/16 chunks, [kc0, kc1) with the first nkc % S slices one chunk longer: as even as possible,
// none empty (S <= nkc). The prefetch behind a slice's last chunk re-loads that chunk (never read): it stays inside the slice.
#include "common.h"
#include "conv_launch.h"
#include "lds_frag.h"
#include <algorithm>

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int SK_TW = 16, SK_TH = 16, SK_TN = 128, SK_NW = 4;

struct Taps4SkArgs {
    const unsigned short* x;    // [Bm,H,W,Cin] NHWC bf16, Cin % 16 == 0
    const unsigned short* wpk;  // packed bf16: [n_tile][cin/16][tap = ty*2+tx][group][128][8]
    float* ws;                  // [S][Bm,H,W,Cout] fp32 raw partial sums
    int B, H, W, Cin, Cout;
    int Ho, Wo;                 // = H, W: every position of the map is computed and stored
    int tiles_x, tiles_y;
    int n_tiles, sp_total, sp_per_xcd, xcd_map;
    int kc_base, kc_rem;        // slice s: kc_base + (s < kc_rem) chunks
    size_t split_stride;        // Bm*H*W*Cout
};

// Two waves per SIMD: within 256 registers the kernel needs no AGPR copies and no spill (200 VGPRs), and two workgroups per CU (2 x 52 KB
// of LDS) run one's MFMAs under the other's barrier and fragment reads. Without the bound the compiler spreads over 192 + 172 registers
// and one workgroup has the CU to itself.
__global__ __launch_bounds__(64 * SK_NW) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_taps4_splitk_bf16_kernel(Taps4SkArgs p) {
    constexpr int TW = SK_TW, TH = SK_TH, TN = SK_TN, NW = SK_NW, NTHREADS = 64 * NW;
    constexpr int IH = TH + 1, IW = TW + 1;
    constexpr int PL = (IH * IW + 15) / 16 * 16;      // plane pitch: a multiple of 16 slots (conv_taps4_bf16_kernel)
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

    // block -> (n tile, spatial tile): XCD-aware order, see conv3x3.hip (the grid's x extent is a multiple of 8 then, so block
    // (i, s) runs on XCD i % 8 for every slice s)
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
    const int slice = blockIdx.y;
    const int kc0 = slice * p.kc_base + min(slice, p.kc_rem);
    const int kc1 = kc0 + p.kc_base + (slice < p.kc_rem ? 1 : 0);      // <= nkc: the launcher checks S <= nkc

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
        const int gr = oy0 + r, gc = ox0 + c;
        const bool ok = pix < IH * IW && gr < p.H && gc < p.W;
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

    // ---- this wave's tiles: pixel tile a (0..3) = row 4*wave + a, columns 0..15; channel tile bt (0..7)
    const int a_lane = grp * PL + 4 * wave * IW + l15 + sel;
    const int w_lane = IN_P + sel * 2 * TN + grp * TN + l15;

    f32x4 acc[4][8];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int bt = 0; bt < 8; ++bt) acc[a][bt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // one K chunk: two K = 32 steps (tap rows) out of stage `in_s` while chunk kc + 1 moves into stage `in_n`
    auto chunk = [&](const u32x4* in_s, u32x4* in_n, int kc) {
        const int kn = (kc + 1 < kc1) ? kc + 1 : kc;      // behind the slice's last chunk the other stage is refilled with it (never read)
        stage_load(kn, in_n);
#pragma unroll
        for (int ty = 0; ty < 2; ++ty) {
            u32x4 fa[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) fa[a] = in_s[a_lane + (a + ty) * IW];
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

    stage_load(kc0, stageA);
    stage_commit(stageA);
    stage_wait();
    __syncthreads();
    for (int kc = kc0; kc < kc1; kc += 2) {
        chunk(stageA, stageB, kc);
        if (kc + 1 < kc1) chunk(stageB, stageA, kc + 1);
    }
    // every wave is behind the last chunk's barrier and nothing is in flight: the slabs below reuse the stages

    // ---- epilogue: the raw sums; register r of lane l of a tile = pixel 4*(l >> 4) + r, channel l & 15. Two rows of 16 pixels x 64
    // channels at a time through a wave-private fp32 slab, 8 channels per lane out. Every (y < H, x < W, n < Cout) of the tile is stored.
    float* slab = reinterpret_cast<float*>(smem) + wave * (32 * SLAB_P);
    const int prow = lane >> 3, pc8 = (lane & 7) * 8;
    const bool wide = (p.Cout & 7) == 0;
    float* const wo = p.ws + (size_t)slice * p.split_stride;
#pragma unroll
    for (int hn = 0; hn < 2; ++hn) {
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) slab[(16 * i + 4 * kg + r) * SLAB_P + 16 * j + l15] = acc[2 * rr + i][4 * hn + j][r];
            const int nbase = n0 + 64 * hn + pc8;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int m = g * 8 + prow;      // slab row: tile row m >> 4, column m & 15
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(slab + m * SLAB_P + pc8);
                const f32x4 v1 = *reinterpret_cast<const f32x4*>(slab + m * SLAB_P + pc8 + 4);
                const int yy = oy0 + 4 * wave + 2 * rr + (m >> 4);
                const int xx = ox0 + (m & 15);
                if (yy < p.H && xx < p.W && nbase < p.Cout) {
                    const size_t o = (((size_t)b * p.H + yy) * p.W + xx) * p.Cout + nbase;
                    if (wide) {
                        *reinterpret_cast<f32x4*>(wo + o) = v0;
                        *reinterpret_cast<f32x4*>(wo + o + 4) = v1;
                    } else {      // Cout % 8 == 4: one element at a time
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (nbase + e < p.Cout) wo[o + e] = e < 4 ? v0[e & 3] : v1[e & 3];
                    }
                }
            }
        }
    }
}

int forced_ksplit() {
    const char* e = getenv("WITW_CONV_KSPLIT");
    return e ? atoi(e) : 0;
}

}  // namespace

extern "C" {

// Split-K factor witw_conv3x3_bf16_fwd_taps4_splitk should run with (the principles of witw_conv3x3_taps4_ksplit): 1 when the plain
// launch already starts a workgroup per CU or K is short; otherwise enough slices for about two workgroups per CU (what the
// kernel's registers and LDS let a CU hold), each at least 8 chunks (128 input channels) long, and never more than 16: every slice
// writes and re-reads Bm*H*W*Cout fp32 (block 5 of 32 images: 14.7 MB per slice; S = 4 is its fastest, S = 16 is back at the unsplit
// time; docs/experiments.md has the sweep). WITW_CONV_KSPLIT forces S.
int witw_conv3x3_bf16_taps4_ksplit(int Bm, int H, int W, int Cin, int Cout) {
    if (Bm <= 0 || H <= 0 || W <= 0 || Cin <= 0 || (Cin % 16) != 0 || Cout <= 0) return -1;
    const int nkc = Cin >> 4;
    const long long wg = (long long)cdiv(Cout, SK_TN) * Bm * cdiv(H, SK_TH) * cdiv(W, SK_TW);
    const int forced = forced_ksplit();
    int S = 1;
    if (forced > 0) S = forced;
    else if (wg < 256 && nkc >= 16) S = (int)std::min<long long>(std::min(16, nkc / 8), (512 + wg - 1) / wg);
    return std::max(1, std::min(S, nkc));      // slices differ by at most one chunk: none is empty
}

// x NHWC bf16 [Bm,H,W,Cin] (Cin % 16 == 0; a g x g mosaic or the plain batch), wpk from witw_conv3x3_bf16_pack_weights_taps4 ->
// ws [ksplit][Bm,H,W,Cout] fp32: the RAW partial sums of each K slice over the taps {1,2}^2, x zero past H / W; no bias, no
// activation, no affine (witw_taps4_splitk_finish applies them). Every element of ws is written.
int witw_conv3x3_bf16_fwd_taps4_splitk(const void* x_bf16, const void* wpk_bf16, float* ws, int Bm, int H, int W, int Cin, int Cout,
                                       int ksplit, void* stream) {
    WITW_CHECK_ARG(x_bf16 && wpk_bf16 && ws, "conv3x3_bf16_fwd_taps4_splitk: null pointer");
    WITW_CHECK_ARG(Bm > 0 && H > 0 && W > 0 && Cout > 0, "conv3x3_bf16_fwd_taps4_splitk: bad shape Bm=%d H=%d W=%d Cout=%d", Bm, H, W, Cout);
    WITW_CHECK_ARG(Cin > 0 && (Cin % 16) == 0, "conv3x3_bf16_fwd_taps4_splitk: Cin=%d must be a positive multiple of 16", Cin);
    WITW_CHECK_ARG((Cout & 3) == 0, "conv3x3_bf16_fwd_taps4_splitk: Cout=%d must be a multiple of 4", Cout);
    WITW_CHECK_ARG(ksplit >= 1 && ksplit <= 65535 && ksplit <= (Cin >> 4), "conv3x3_bf16_fwd_taps4_splitk: ksplit=%d outside [1, Cin/16]",
                   ksplit);
    WITW_CHECK_ARG((size_t)H * W * Cin * 2 < 0x80000000ull, "conv3x3_bf16_fwd_taps4_splitk: image too large for one buffer descriptor");
    WITW_CHECK_ARG((size_t)cdiv(Cout, SK_TN) * Cin * (4 * SK_TN * 2) < 0x80000000ull,
                   "conv3x3_bf16_fwd_taps4_splitk: packed filter too large for one buffer descriptor");
    Taps4SkArgs a;
    a.x = (const unsigned short*)x_bf16; a.wpk = (const unsigned short*)wpk_bf16; a.ws = ws;
    a.B = Bm; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
    a.Ho = H; a.Wo = W;
    a.tiles_x = cdiv(W, SK_TW);
    a.tiles_y = 0;
    a.xcd_map = witw_conv_xcd_map();
    a.kc_base = (Cin >> 4) / ksplit; a.kc_rem = (Cin >> 4) % ksplit;
    a.split_stride = (size_t)Bm * H * W * Cout;
    const long long grid = witw_conv_grid(a, SK_TH, SK_TN, "conv3x3_bf16_fwd_taps4_splitk");
    if (!grid) return WITW_ERR_INVALID;
    hipLaunchKernelGGL(conv_taps4_splitk_bf16_kernel, dim3((unsigned)grid, (unsigned)ksplit), dim3(64 * SK_NW), 0, (hipStream_t)stream, a);
    WITW_CHECK_LAUNCH("conv_taps4_splitk_bf16");
    witw_note_variant("conv_taps4_splitk_bf16_kernel");
    return WITW_OK;
}

}  // extern "C"
