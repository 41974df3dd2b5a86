// 3x3 convolution, NHWC fp32, implicit GEMM on v_mfma_f32_32x32x2_f32 (gfx950).
//
// Replaces, for the FOV_DSM encoder of the reference (model/cvig_fov.py:256-294):
//   torch.nn.Conv2d(k=3, pad=1, stride (1,1)|(2,1)) [+ HorizCircPadding :212-231]
//   [+ AddDropout :234-245] [+ ReLU] [+ MaxPool2d(2,2)]
// as ONE kernel per conv layer: padding is a halo-load policy (zero rows, zero or
// wrapped columns), bias / dropout-scale / ReLU / 2x2 max-pool live in the epilogue.
//
// Tiling (per workgroup of NW = 4 or 8 waves; 8 = two waves per SIMD sharing one weight slab):
//   output tile  TH x TW = NW x 64 conv-output pixels  (2*NW MFMA M-tiles of 32 columns)
//   x TN output channels (64 or 128)                  (2 or 4 MFMA N-tiles of 32)
//   K loop over input channels in chunks of 8 (two "quads" of 4 channels); per chunk
//   the (TH-1)*SH+3 x 66 input halo tile and the 9x8xTN weight slab are staged in LDS
//   (double buffered, register-staged one chunk ahead of the MFMAs).
// LDS images are quad-planar ([quad][row][col] of float4 / [tap][quad][n] of float4)
// so every ds_read_b128 of a wave covers 2 x 512 contiguous bytes (conflict free) and
// yields the operands of 4 MFMA k-steps: MFMA step j takes channel j of quad 0 from
// lanes 0-31 and channel j of quad 1 from lanes 32-63 (A and B agree on that order).
#include "common.h"
#include "lds_frag.h"
#include <stdlib.h>
#include <algorithm>

namespace {

constexpr int TW_WIDE = 64;

// Source of every padded (out-of-image) halo slot: loading zeros from memory keeps the staging
// path free of selects, which the compiler would otherwise pin right behind each load (vmcnt(0)).
__device__ const f32x4 g_zero_f4[1] = {{0.f, 0.f, 0.f, 0.f}};

struct ConvArgs {
    const float* x;         // [B,H,W,Cin] NHWC, Cin % 8 == 0
    const float* wpk;       // packed: [n_tile][cin/8][tap][quad][TN][4]
    const float* bias;      // [n_tiles*TN] (zero padded)
    const float* dropmask;  // [B,Cout] scale (0 or 1/(1-p)) or nullptr
    const float* post_scale;  // nullptr, or per-channel scale/shift applied AFTER the activation (folded BatchNorm)
    const float* post_shift;
    float lrelu;            // negative slope when relu == 2 (LeakyReLU)
    unsigned char* pool_code;  // nullptr, or [B,Hy,Wy,Cout] argmax position (dy*2+dx) of the fused 2x2 max pool
    const float* gate;      // nullptr, or a tensor shaped like y: outputs where gate <= 0 are zeroed (ReLU backward)
    float* y;               // NHWC [B,Hy,Wy,Cout] or NCHW [B,Cout,Hy,Wy]
    int B, H, W, Cin, Cout;
    int Ho, Wo;             // conv output size (before pooling)
    int tiles_x, tiles_y;
    int n_tiles, sp_total, sp_per_xcd, xcd_map;   // workgroup -> tile mapping, see the kernel
    int circ, relu, out_nchw;
    int force_nw;           // 0 = choose, 4 / 8 = force the workgroup shape (tuning aid)
    int force_geo;          // -1 = choose, 0 / 1 = force the wide / narrow tile geometry
    int dil_h;              // 1: input rows are zero-interleaved (row 2i = physical row i): dgrad of a stride-(2,1) conv
    int tap_base;           // TAPS == 4 only: the 2x2 taps are (tap_base + {0,1}, tap_base + {0,1}) of the 3x3 window
    // TAPS == 4 only, split-K: ksplit > 1 launches grid.y = ksplit workgroups per tile, each reducing K-chunks
    // [blockIdx.y * kc_per_split, ...) and writing its RAW partial sums (no bias / activation / affine) to
    // y + blockIdx.y * split_stride; splitk_finish_kernel adds the partials in fixed order and applies the epilogue.
    int ksplit, kc_per_split;
    size_t split_stride;
    // TAPS == 4 only: s2d != 0 writes the output as the space-to-depth(2) image the next k=4,s=2 layer reads,
    // [B, s2d_h, s2d_w, 4*Cout] with channel ((y&1)*2 + (x&1))*Cout + c; outputs at y >= valid_h or x >= valid_w are
    // written as 0 (the conv grid is padded to the tile; the next layer's window must read zeros there).
    int s2d, s2d_h, s2d_w, valid_h, valid_w;
    // 1: Winograd F(2,3) along H (conv_wino_h2): wpk_wino is the filter of witw_conv3x3_pack_weights_wino, n_tiles counts
    // 64-channel tiles. Set by the launcher only for stride 1, no gate / dil_h / NCHW output / post affine, geometry 0.
    int wino;
    const float* wpk_wino;
    // Winograd form only: the launch starts wino_wgs workgroups, and workgroup w walks the run w, w + wino_wgs, ... of the
    // wino_items indices of the workgroup -> tile map (one index per workgroup when witw_conv3x3_wino_run is off)
    int wino_items, wino_wgs;
    // Winograd form only: a K chunk is staged by LDS-DMA (0: global -> registers -> LDS; same bits)
    int wino_dma;
#ifdef WITW_STAMPS
    unsigned long long* stamps;   // diagnostic build only (tools/conv_stamps.cpp)
#endif
};

// ---- Winograd F(2,3) along H (inference, stride 1, 3x3, geometry 0; a per-launch mode of conv3x3_nhwc_f32_kernel)
// For an output row pair (r, r+1) and one column tap kw, the 4 input rows d0..d3 = rows r-1..r+2 give
//   V0 = d0-d2, V1 = d1+d2, V2 = d2-d1, V3 = d1-d3             (in registers, after the raw ds_read_b128)
//   m_t += V_t . U_t  with  U0 = g0, U1 = ((g0+g1)+g2)/2, U2 = ((g0-g1)+g2)/2, U3 = g2   (packed once, pack_weights_wino_kernel)
//   y0 = (m0+m1)+m2, y1 = (m1-m2)-m3                               (epilogue)
// 4 products per (row pair, kw) instead of 6: 2/3 of the MFMAs of the direct form. Only H is transformed: W is the circularly
// padded axis, whose outputs must not depend on which of them share a tile. Accumulators per output double, so a wave covers
// half of what a direct wave covers: one row pair x 64 columns x 32 channels (acc[t][column half], 128 VGPRs); the workgroup
// tile is NW rows x 64 columns x 64 channels whatever TN names, the halo tile is staged exactly as in the direct form and the
// filter slab of a K chunk is [kw][t][quad][64] (12 slices instead of 9 of twice the width). Every output gets the same
// arithmetic in the same order (chunk -> kw -> channel) at NW = 4 and 8.
// DMA: a K chunk is staged by LDS-DMA (dma16, lds_frag.h), NIN + NWT pieces of 1 KB per wave, with no staging registers and no LDS
// write instructions; !DMA: global -> registers -> LDS (witw_conv3x3_wino_dma(0): A/B runs, the bitwise tests). A piece lands in
// 64 consecutive slots, so the DMA form's slot s is LDS slot s of the stage (plane s / (IH*IW), pixel s % (IH*IW)) where the
// register form's is (plane s & 1, pixel s >> 1). The input region of a stage is rounded up to whole pieces (IN_PAD) in both
// forms; the slots behind the tile take zeros from the buffer's range check.
template <int NW, bool POOL, bool DMA>
__device__ __forceinline__ void conv_wino_h2(const ConvArgs& p, f32x4* smem) {
    constexpr int TH = NW, TW = 64, IW = TW + 2, IH = TH + 2;
    constexpr int NTHREADS = 64 * NW;
    constexpr int WTN = 64;                    // output channels per workgroup
    constexpr int IN_F4 = 2 * IH * IW;
    constexpr int W_F4 = 12 * 2 * WTN;         // [kw][t][quad][n]
    constexpr int NIN = (IN_F4 + NTHREADS - 1) / NTHREADS;
    constexpr int NWT = W_F4 / NTHREADS;
    constexpr int IN_PAD = NIN * NTHREADS;     // input region of a stage: whole LDS-DMA pieces
    constexpr int STAGE_F4 = IN_PAD + W_F4;
    static_assert(NWT * NTHREADS == W_F4, "the filter slab splits evenly over the workgroup");

    // an opaque copy: nothing derived from it is shared with the direct form's code, whose registers would stay live over this form's
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int hq = lane >> 5;

    // item -> (n tile, image, spatial tile): the map of the direct form, taken over an item index instead of blockIdx.x. Workgroup
    // w walks items w, w + G, w + 2G, ... (G = p.wino_wgs, a multiple of 8 on the device: its run stays on one XCD's share of
    // the spatial tiles, and the n tiles of a spatial tile still run at the same time on that XCD's L2); the holes of the padded
    // XCD map (sp >= sp_total) are stepped over.
    const int tiles_img = p.tiles_x * p.tiles_y;
    auto item_sp = [&](int it, int& ntile) {
        if (p.xcd_map) {
            const int g = it >> 3;
            ntile = g % p.n_tiles;
            return (it & 7) * p.sp_per_xcd + g / p.n_tiles;
        }
        ntile = it / p.sp_total;
        return it - ntile * p.sp_total;
    };
    auto step_item = [&](int it) { return p.wino_items - it > p.wino_wgs ? it + p.wino_wgs : p.wino_items; };      // no overflow
    auto next_item = [&](int it) {      // first item of the run at or behind `it` that is a tile; p.wino_items when there is none
        int nt;
        while (it < p.wino_items && item_sp(it, nt) >= p.sp_total) it = step_item(it);
        return it;
    };
    int it = next_item(blockIdx.x);
    if (it >= p.wino_items) return;
    const int nkc = p.Cin >> 3;

    constexpr unsigned OOR = 0x80000000u;
    const size_t img_floats = (size_t)p.H * p.W * p.Cin;
    // the tile being accumulated (the epilogue's), and the source of the staging instructions: the same tile up to its last chunk,
    // whose "next chunk" is chunk 0 of the run's next item
    int ntile, b, oy0, ox0;
    __amdgpu_buffer_rsrc_t in_rs, w_rs;      // !DMA
    i32x4 in_rd, w_rd;                       // DMA: the same records as four SGPRs each
    unsigned gin[NIN];
    auto decode = [&](int item, int& nt_, int& b_, int& oy0_, int& ox0_) {
        int sp = item_sp(item, nt_);
        b_ = sp / tiles_img;
        sp -= b_ * tiles_img;
        const int ty = sp / p.tiles_x;
        oy0_ = ty * TH;
        ox0_ = (sp - ty * p.tiles_x) * TW;
    };
    // live = false: records of zero bytes, every staging load returns zeros without a memory access (behind a run's last item)
    auto stage_from = [&](int nt_, int b_, int oy0_, int ox0_, bool live) {
        const float* in_base = p.x + (size_t)b_ * img_floats;
        const f32x4* w_base = reinterpret_cast<const f32x4*>(p.wpk_wino) + (size_t)nt_ * nkc * W_F4;
        const unsigned in_bytes = live ? (unsigned)(img_floats * 4) : 0u, w_bytes = live ? (unsigned)nkc * W_F4 * 16u : 0u;
        if constexpr (DMA) {
            in_rd = raw_rsrc(in_base, in_bytes);
            w_rd = raw_rsrc(w_base, w_bytes);
        } else {
            in_rs = __builtin_amdgcn_make_buffer_rsrc((void*)in_base, 0, in_bytes, 0x00020000);
            w_rs = __builtin_amdgcn_make_buffer_rsrc((void*)w_base, 0, w_bytes, 0x00020000);
        }
        if (!live) return;
        // the slot's (row, column) is worked out anew for every item: kept in registers over the K loop it would not fit
        int t = tid;
        asm volatile("" : "+v"(t));
#pragma unroll
        for (int i = 0; i < NIN; ++i) {
            const int s = t + i * NTHREADS;
            const int q = DMA ? (s >= IH * IW) : (s & 1);
            const int pix = DMA ? s - q * (IH * IW) : s >> 1;
            const int r = pix / IW, c = pix - r * IW;
            const int gr = oy0_ - 1 + r;
            int gc = ox0_ - 1 + c;
            bool ok = (s < IN_F4) && gr >= 0 && gr < p.H;
            if (p.circ) {
                gc %= p.W;
                if (gc < 0) gc += p.W;
            } else {
                ok = ok && gc >= 0 && gc < p.W;
            }
            gin[i] = ok ? (unsigned)((((size_t)gr * p.W + gc) * p.Cin + q * 4) * 4) : OOR;
        }
    };
    decode(it, ntile, b, oy0, ox0);
    stage_from(ntile, b, oy0, ox0, true);
    const unsigned gwoff = (unsigned)tid * 16u;
    // staging of a K chunk, one instruction at a time (i < NIN: input tile, then the filter slab). DMA: piece i of this wave, slots
    // [i * NTHREADS + 64 * wave, + 64) of the stage's input region or of its filter slab
    const unsigned smem_lds = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_address(smem));
    const unsigned wave_lds = (unsigned)__builtin_amdgcn_readfirstlane(wave) * 1024u;
    auto dma_one = [&](int buf, int kc, int i) {
        const unsigned st = smem_lds + (unsigned)buf * (STAGE_F4 * 16u) + wave_lds;
        if (i < NIN) dma16(in_rd, st + (unsigned)i * (NTHREADS * 16u), gin[i], (unsigned)kc * 32u);
        else dma16(w_rd, st + (unsigned)(IN_PAD + (i - NIN) * NTHREADS) * 16u, gwoff,
                   (unsigned)kc * W_F4 * 16u + (unsigned)(i - NIN) * (NTHREADS * 16u));
    };
    // !DMA: global -> registers -> LDS
    f32x4 rin[NIN], rw[NWT];
    auto load_one = [&](int kc, int i) {
        if (i < NIN) rin[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(in_rs, gin[i], (unsigned)kc * 32u, 0));
        else rw[i - NIN] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                 w_rs, gwoff, (unsigned)kc * W_F4 * 16u + (unsigned)(i - NIN) * (NTHREADS * 16u), 0));
    };
    auto store_one = [&](int buf, int i) {
        f32x4* in_s = smem + buf * STAGE_F4;
        if (i < NIN) {
            const int s = tid + i * NTHREADS;
            f32x4* dst = (NIN * NTHREADS == IN_F4 || s < IN_F4) ? in_s + (s & 1) * (IH * IW) + (s >> 1) : smem + 2 * STAGE_F4;
            *dst = rin[i];
        } else {
            in_s[IN_PAD + tid + (i - NIN) * NTHREADS] = rw[i - NIN];
        }
    };

    // wave -> (row pair wm, channel half wn); step s = (kw = s >> 1, column half ct = s & 1), 6 steps per K chunk
    const int wm = wave >> 1, wn = wave & 1;
    const int abase = hq * (IH * IW) + 2 * wm * IW + l31;
    const int wbase = hq * WTN + wn * 32 + l31;
    f32x16 acc[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][ct][r] = 0.f;

    // fa: input rows d0..d3 of a step, transformed in place into V0..V3 late in the step before; fb: filter slices U0..U3 of a kw
    f32x4 fa[2][4], fb[2][4];
    auto read_a = [&](int set, const f32x4* in_s, int s, int i) { fa[set][i] = in_s[abase + i * IW + 32 * (s & 1) + (s >> 1)]; };
    auto read_b = [&](int set, const f32x4* w_s, int kw, int t) { fb[set][t] = w_s[(kw * 4 + t) * 2 * WTN + wbase]; };
    // the transform in 8 pairs of single v_add_f32 / v_sub_f32 (packed f32 VALU beside MFMAs costs more): pair k = channel k >> 1,
    // (V0, V3) then (V1, V2)
    auto transform2 = [&](int set, int k) {
        const int j = k >> 1;
        const float d0 = fa[set][0][j], d1 = fa[set][1][j], d2 = fa[set][2][j], d3 = fa[set][3][j];
        if ((k & 1) == 0) {
            fa[set][0][j] = d0 - d2;
            fa[set][3][j] = d1 - d3;
        } else {
            fa[set][1][j] = d1 + d2;
            fa[set][2][j] = d2 - d1;
        }
    };
    auto mfma_one = [&](int set, int bset, int ct, int i) {      // MFMA i of a step: channel i >> 2, product t = i & 3
        const int j = i >> 2, t = i & 3;
        acc[t][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][t][j], fb[bset][t][j], acc[t][ct], 0, 0, 0);
    };

    if constexpr (DMA) {
#pragma unroll
        for (int i = 0; i < NIN + NWT; ++i) dma_one(0, 0, i);
        wait_vmcnt<0>();
    } else {
#pragma unroll
        for (int i = 0; i < NIN + NWT; ++i) load_one(0, i);
#pragma unroll
        for (int i = 0; i < NIN + NWT; ++i) store_one(0, i);
    }
    __syncthreads();
    // filter slices before input rows, pinned: the transform's wait for the rows then leaves no read in flight at the loop's head,
    // where a read still pending from here would turn the first MFMA's counted wait into a full drain on every trip
#pragma unroll
    for (int i = 0; i < 4; ++i) read_b(0, smem + IN_PAD, 0, i);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) read_a(0, smem, 0, i);
#pragma unroll
    for (int k = 0; k < 8; ++k) transform2(0, k);

    // A step is 16 MFMAs on fragment set `set` and filter set `bset`. Behind MFMA i stands what mem(i) issues -- the next step's
    // fragment reads first, input rows 0..3 before filter slices, then a staging instruction where due, one instruction each --
    // and, from MFMA 8 on, one pair of the transform of those rows into set ^ 1: at least 4 MFMAs behind the last of their reads,
    // a whole step ahead of the MFMAs that take them. The order is pinned gap by gap (sched_barrier): left to itself the scheduler
    // sinks every v_add / v_sub to the MFMA it feeds and drags the raw rows' reads and full LDS drains there with it; named as
    // sched_group_barrier groups the greedy solver scatters reads and transforms over the step.
    auto step = [&](int set, int bset, int ct, auto&& mem, bool barrier_mid) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            mfma_one(set, bset, ct, i);
            mem(i);
            if (i >= 8) transform2(set ^ 1, i - 8);
            __builtin_amdgcn_sched_barrier(0);
            if (barrier_mid && i == 7) {
                if constexpr (DMA) wait_vmcnt<0>();      // this wave's pieces of the next chunk have landed; the barrier publishes them
                __syncthreads();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    static_assert(16 - 6 - (NIN + NWT) >= 0, "step too short to hide the staging instructions");

    // B slices: kw 0 and 2 in set 0, kw 1 in set 1 (kw 2 read in step 2, behind the last use of kw 0); the next chunk's kw 0
    // arrives in set 1 during step 5, behind the chunk's single barrier, and is moved to set 0. Next chunk: loads under step 0,
    // LDS writes under step 3. A transform waits for its four rows only, and in every step a younger LDS instruction follows the
    // row reads (filter slices in steps 0, 1, 2 and 5 -- hence kw 1 in two halves --, the staging writes in step 3), so the wait
    // is a counted one. Step 4 has none to offer: there the chunk's barrier, whose drain is the loop's only full one, stands
    // between the reads (MFMAs 0..3) and the transform (MFMAs 8..15). It still separates the last read of this stage (step 4)
    // from its next overwrite (step 3 of the next chunk), and the writes of the next stage (step 3) from their first read (step 5).
    // DMA: the next chunk's pieces go out under steps 0..2 instead (the other stage is free from the previous chunk's barrier on),
    // in the gaps that hold neither a fragment read nor a transform: all six in step 0's consecutive gaps, beside its reads, cost
    // 0.9 ms per step against the register path, spread over the bare gaps they win 1.4 ms. Each wave waits for its own pieces
    // (vmcnt) in front of the barrier of step 4, and step 3, which has no staging writes to offer, takes the second half of kw 2's
    // filter slices as its younger LDS instructions.
    // One K chunk on stage `cur`, staging chunk kn of the staging source into the other stage.
    auto chunk = [&](int cur, int kn) __attribute__((always_inline)) {
        const f32x4* in_s = smem + cur * STAGE_F4;
        const f32x4* w_s = in_s + IN_PAD;
        const f32x4* in_n = smem + (cur ^ 1) * STAGE_F4;
        // DMA pieces: the gaps of steps 0..2 that hold neither a fragment read nor a transform (6, 7; NW = 4: 6..9)
        constexpr int PER = (NIN + NWT + 2) / 3;
        auto dma_gap = [&](int s, int i) {
            const int j = s * PER + (i - 6);
            if (i >= 6 && i < 6 + PER && j < NIN + NWT) dma_one(cur ^ 1, kn, j);
        };
        step(0, 0, 0, [&](int i) {
            if (i < 4) read_a(1, in_s, 1, i);
            else if (i < 6) read_b(1, w_s, 1, i - 4);
            else if (DMA) dma_gap(0, i);
            else if (i < 6 + NIN + NWT) load_one(kn, i - 6);
        }, false);
        step(1, 0, 1, [&](int i) {
            if (i < 4) read_a(0, in_s, 2, i);
            else if (i < 6) read_b(1, w_s, 1, i - 2);
            else if (DMA) dma_gap(1, i);
        }, false);
        step(0, 1, 0, [&](int i) {
            if (i < 4) read_a(1, in_s, 3, i);
            else if (i < (DMA ? 6 : 8)) read_b(0, w_s, 2, i - 4);
            else if (DMA) dma_gap(2, i);
        }, false);
        step(1, 1, 1, [&](int i) {
            if (i < 4) read_a(0, in_s, 4, i);
            else if (DMA && i < 6) read_b(0, w_s, 2, i - 2);
            else if (!DMA && i < 4 + NIN + NWT) store_one(cur ^ 1, i - 4);
        }, false);
        step(0, 0, 0, [&](int i) {
            if (i < 4) read_a(1, in_s, 5, i);
        }, true);
        step(1, 0, 1, [&](int i) {
            if (i < 4) read_a(0, in_n, 0, i);
            else if (i < 8) read_b(1, in_n + IN_PAD, 0, i - 4);
        }, false);
#pragma unroll
        for (int t = 0; t < 4; ++t) fb[0][t] = fb[1][t];
    };

    // The run. The K loop is continuous over it: the stage parity carries on from item to item, and an item's last chunk stages
    // chunk 0 of the next item (its own addresses and filter base, computed here between the loop and that chunk) and reads its
    // first fragments in step 5, so only the run's first item pays the cold prologue above. Behind the run's last item the same
    // instructions load zeros from empty records. Between two items stands the epilogue, serial, and the accumulators are cleared.
    const int Hy = POOL ? (p.Ho >> 1) : p.Ho;
    const int Wy = POOL ? (p.Wo >> 1) : p.Wo;
    // wave-private 4 KB epilogue slabs (32 pixels x 32 channels) behind the stages and their dummy slot: the other stage holds the
    // next item's first chunk by then
    float* slab = reinterpret_cast<float*>(smem + 2 * STAGE_F4 + 1) + wave * (32 * 32);
    const int prow = lane >> 3, pc4 = (lane & 7) * 4;     // read-back role: pixel in a group of 8, channel quad
    int cur = 0;
    for (;;) {
        for (int kc = 1; kc < nkc; ++kc) {
            chunk(cur, kc);
            cur ^= 1;
        }
        const int it_n = next_item(step_item(it));
        const bool more = it_n < p.wino_items;
        int ntile_n = ntile, b_n = b, oy0_n = oy0, ox0_n = ox0;
        if (more) decode(it_n, ntile_n, b_n, oy0_n, ox0_n);
        stage_from(ntile_n, b_n, oy0_n, ox0_n, more);
        chunk(cur, 0);
        cur ^= 1;

        // ---- epilogue: output transform, bias, dropout scale, ReLU, optional 2x2 max pool (the wave's own row pair), 16-byte stores
        // through the wave's slab
        const int n0 = ntile * WTN;
        f32x16 yv[2][2];       // [output row of the pair][column half]
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float m0 = acc[0][ct][r], m1 = acc[1][ct][r], m2 = acc[2][ct][r], m3 = acc[3][ct][r];
                yv[0][ct][r] = (m0 + m1) + m2;
                yv[1][ct][r] = (m1 - m2) - m3;
            }
        const int nb = n0 + wn * 32;
        const int nch = nb + l31;
        const float bv = p.bias[nch];
        const float dm = (p.dropmask != nullptr && nch < p.Cout) ? p.dropmask[(size_t)b * p.Cout + nch] : 1.f;
        const int act = p.relu;
        auto fin = [&](float v) {
            v = (v + bv) * dm;
            if (act == 1) v = fmaxf(v, 0.f);
            else if (act == 2) v = v > 0.f ? v : v * p.lrelu;
            return v;
        };
        if constexpr (!POOL) {
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) slab[((r & 3) + 8 * (r >> 2) + 4 * hq) * 32 + l31] = fin(yv[k][ct][r]);
                    const int yy = oy0 + 2 * wm + k;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int m = g * 8 + prow;
                        const f32x4 v = *reinterpret_cast<const f32x4*>(slab + m * 32 + pc4);
                        const int xx = ox0 + 32 * ct + m;
                        if (yy < Hy && xx < Wy && nb + pc4 < p.Cout)
                            __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p.y + (((size_t)b * Hy + yy) * Wy + xx) * p.Cout + nb + pc4));
                    }
                }
        } else {
            const int yy = (oy0 + 2 * wm) >> 1;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int r = 4 * g + 2 * e;
                        const float a00 = yv[0][ct][r], a01 = yv[0][ct][r + 1], a10 = yv[1][ct][r], a11 = yv[1][ct][r + 1];
                        const float m = fmaxf(fmaxf(a00, a01), fmaxf(a10, a11));
                        const int pc = 16 * ct + 4 * g + 2 * hq + e;
                        slab[pc * 32 + l31] = fin(m);
                        const int xx = (ox0 >> 1) + pc;
                        if (p.pool_code != nullptr && yy < Hy && xx < Wy && nch < p.Cout) {
                            const int code = (a00 == m) ? 0 : (a01 == m) ? 1 : (a10 == m) ? 2 : 3;
                            p.pool_code[(((size_t)b * Hy + yy) * Wy + xx) * p.Cout + nch] = (unsigned char)code;
                        }
                    }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int pc = g * 8 + prow;
                const f32x4 v = *reinterpret_cast<const f32x4*>(slab + pc * 32 + pc4);
                const int xx = (ox0 >> 1) + pc;
                if (yy < Hy && xx < Wy && nb + pc4 < p.Cout)
                    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p.y + (((size_t)b * Hy + yy) * Wy + xx) * p.Cout + nb + pc4));
            }
        }
        if (!more) break;
        it = it_n;
        ntile = ntile_n;
        b = b_n;
        oy0 = oy0_n;
        ox0 = ox0_n;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][ct][r] = 0.f;
    }
}

// NW = waves per workgroup (4: 4x64-pixel tile, one wave per SIMD; 8: 8x64-pixel tile, two waves per SIMD
// sharing one weight slab: 40 % less staging and half the barriers per MFMA, used when the layer is tall
// and the grid large enough).
// GEO = shape of one MFMA M-tile (32 output pixels): 0 = 1 row x 32 columns, workgroup tile NW rows x 64 columns
// (wide maps); 1 = 2 rows x 16 columns, workgroup tile 4*NW rows x 16 columns (maps up to 32 columns wide, e.g. the
// fov-70 ground branch whose widths are 24 and 12 in the deep layers: a 64-column tile would idle 63-81 % of it).
// GEO = 2 (round 5) = geometry 0 for a ZERO-INTERLEAVED input (dil_h: the dgrad of a stride-(2,1) layer, model/cvig_fov.py:263-272): every
// odd logical input row is zero, so an M-tile on an even output row only meets data under tap row kh = 1 and one on an odd output
// row under kh = 0 and 2 -- the other (M-tile, tap) products multiply staged zeros. This instantiation issues neither those MFMAs nor
// their fragment reads: half the matrix work of the launch, the same sums bit for bit (a skipped product adds +-0). 8-wave 128-channel
// tile only (its M-tiles are whole rows of known parity: row 2 wm + (mt >> 1) of an 8-row tile).
// TAPS = 9: the full 3x3 window. TAPS = 4: a 2x2 sub-window of it (rows/columns tap_base + {0,1}): the cvig_baseline
// Conv2d(k=4, s=2, p=0) (model/cvig_baseline.py:236-252) is a 2x2 convolution over the space-to-depth(2) image, i.e. the
// 3x3 window whose first tap row and column are zero (dgrad: last row and column) — 4 of 9 taps carry all the work.
template <int TN, int SH, bool POOL, int NW, int GEO, int TAPS = 9>
__global__ __launch_bounds__(64 * NW) void conv3x3_nhwc_f32_kernel(ConvArgs p) {
    static_assert(TAPS == 9 || TAPS == 4, "3x3 window or a 2x2 sub-window");
    constexpr bool NARROW = GEO == 1;
    constexpr bool DIL = GEO == 2;              // zero-interleaved input rows: dead (M-tile, tap) products are not issued
    static_assert(!DIL || (TN == 128 && NW == 8 && SH == 1 && TAPS == 9 && !POOL), "the dilated form exists for the 8-wave 128-channel tile");
    constexpr int TH = NARROW ? 4 * NW : NW;
    constexpr int TW = NARROW ? 16 : 64;
    constexpr int IW = TW + 2;
    constexpr int NTHREADS = 64 * NW;
    constexpr int IH = (TH - 1) * SH + 3;
    constexpr int IN_F4 = 2 * IH * IW;          // float4 slots of one input stage
    constexpr int W_F4 = TAPS * 2 * TN;         // float4 slots of one weight stage
    constexpr int STAGE_F4 = IN_F4 + W_F4;
    constexpr int NIN = (IN_F4 + NTHREADS - 1) / NTHREADS;
    constexpr int NWT = (W_F4 + NTHREADS - 1) / NTHREADS;
    constexpr int WGM = (TN == 128) ? NW / 2 : NW;   // waves along M
    constexpr int WM = (2 * NW) / WGM;               // M-tiles per wave (2*NW per workgroup): 4 at TN=128, 2 at TN=64
    constexpr int WN = 2;                       // N-tiles per wave (64 channels)

    // +1: dummy slot that absorbs out-of-tile staging stores. The epilogue re-uses the buffer as NW wave-private 8 KB slabs:
    // with 4 taps and TN = 64 two stages are smaller than 8 slabs (58.6 KB < 64 KB), so the array is sized for both uses.
    // WINO: the classes that also run the Winograd F(2,3)-along-H form (conv_wino_h2) when the launcher sets p.wino
    constexpr bool WINO = SH == 1 && TAPS == 9 && GEO == 0 && (TN == 128 || POOL);
    // its two stages, the dummy slot and, behind them, a 4 KB epilogue slab per wave (both stages are live between two items of a run)
    // (the input region of a stage in whole 1 KB pieces per wave, as the LDS-DMA staging writes it)
    constexpr int WINO_IN_F4 = (2 * (NW + 2) * IW + NTHREADS - 1) / NTHREADS * NTHREADS;
    constexpr int WINO_F4 = WINO ? 2 * (WINO_IN_F4 + 12 * 2 * 64) + 1 + NW * 256 : 0;
    constexpr int DIRECT_F4 = (2 * STAGE_F4 + 1 > NW * 512) ? 2 * STAGE_F4 + 1 : NW * 512;
    constexpr int SMEM_F4 = DIRECT_F4 > WINO_F4 ? DIRECT_F4 : WINO_F4;
    __shared__ f32x4 smem[SMEM_F4];
    static_assert(SMEM_F4 * 16 >= NW * 32 * 64 * 4, "the buffer must hold one epilogue slab per wave");
    if constexpr (WINO) {
        // weighted as the unlikely side: the run loop around the K loop otherwise outweighs the direct form's blocks in the register
        // allocator's spill costs, and the direct epilogue spills (72 VGPRs in <128,1,false,8,0,9>)
        if (__builtin_expect(p.wino != 0, 0)) {
            if (p.wino_dma) conv_wino_h2<NW, POOL, true>(p, smem);
            else conv_wino_h2<NW, POOL, false>(p, smem);
            return;
        }
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int hq = lane >> 5;

    // ---- block -> (n tile, image, spatial tile). Workgroups go to the 8 XCDs round-robin (block i -> XCD i % 8), each
    // with its own L2. XCD x takes the contiguous range [x*sp_per_xcd, (x+1)*sp_per_xcd) of spatial tiles and runs
    // the n tiles of one spatial tile back to back: the halo tile is fetched over the fabric once instead of once per
    // n tile, vertically adjacent tiles share their halo rows in L2, and the (small) weight chunks of all n tiles stay
    // L2 resident. The grid is padded to 8 * sp_per_xcd * n_tiles; surplus workgroups leave here.
    int ntile, sp;
    if (p.xcd_map) {
        const int g = blockIdx.x >> 3;
        ntile = g % p.n_tiles;
        sp = (blockIdx.x & 7) * p.sp_per_xcd + g / p.n_tiles;
        if (sp >= p.sp_total) return;
    } else {        // n tile slowest: the workgroups in flight share one weight slab
        ntile = blockIdx.x / p.sp_total;
        sp = blockIdx.x - ntile * p.sp_total;
    }
    const int tiles_img = p.tiles_x * p.tiles_y;
    const int b = sp / tiles_img;
    sp -= b * tiles_img;
    const int ty = sp / p.tiles_x;
    const int tx = sp - ty * p.tiles_x;
    const int oy0 = ty * TH;
    const int ox0 = tx * TW;
    const int n0 = ntile * TN;
    int nkc = p.Cin >> 3;      // K-chunks (8 input channels each) this workgroup reduces
    int kc_lo = 0;             // ... starting at this one: split-K slices move the buffer bases, the loop stays 0 .. nkc
    if constexpr (TAPS == 4) {
        if (p.ksplit > 1) {
            kc_lo = (int)blockIdx.y * p.kc_per_split;
            nkc = min(nkc - kc_lo, p.kc_per_split);
        }
    }

    // ---- staging through buffer loads: one descriptor per image / per weight tile built from scalars, the
    // per-thread byte offset is fixed for the whole K loop and the K-chunk advance rides in the scalar
    // offset, so a load costs no VALU instruction next to the f32 MFMAs. Padded halo slots (rows outside the
    // image, zero-padded columns) carry an out-of-range offset and read 0.
    constexpr unsigned OOR = 0x80000000u;
    const int Hp = p.dil_h ? (p.H - 1) / 2 + 1 : p.H;          // physical rows of the input
    const size_t img_floats = (size_t)Hp * p.W * p.Cin;
    __amdgpu_buffer_rsrc_t in_rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.x + (size_t)b * img_floats + (size_t)kc_lo * 8), 0, (unsigned)(img_floats * 4) - (unsigned)kc_lo * 32u, 0x00020000);
    const unsigned wtile_bytes = (unsigned)nkc * W_F4 * 16u;
    __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(reinterpret_cast<const f32x4*>(p.wpk) + ((size_t)ntile * (p.Cin >> 3) + kc_lo) * W_F4), 0, wtile_bytes, 0x00020000);
    unsigned gin[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
        const int s = tid + i * NTHREADS;
        const int pix = s >> 1, q = s & 1;
        const int r = pix / IW, c = pix - r * IW;
        const int gr = oy0 * SH - 1 + r;
        int gc = ox0 - 1 + c;
        bool ok = (s < IN_F4) && gr >= 0 && gr < p.H;
        int grp = gr;                 // physical row
        if (p.dil_h) {
            ok = ok && (gr & 1) == 0;
            grp = gr >> 1;
        }
        if (p.circ) {
            gc %= p.W;
            if (gc < 0) gc += p.W;
        } else {
            ok = ok && gc >= 0 && gc < p.W;
        }
        gin[i] = ok ? (unsigned)((((size_t)grp * p.W + gc) * p.Cin + q * 4) * 4) : OOR;
    }
    const unsigned gwoff = (unsigned)tid * 16u;

    // Staging is branch-free so that the whole K-chunk body is ONE scheduling region; out-of-tile
    // slots are sent to the dummy LDS slot.
    f32x4 rin[NIN], rw[NWT];
    auto load_stage = [&](int kc) {
#pragma unroll
        for (int i = 0; i < NIN; ++i)
            rin[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(in_rs, gin[i], (unsigned)kc * 32u, 0));
        const unsigned wbase = (unsigned)kc * W_F4 * 16u;
#pragma unroll
        for (int i = 0; i < NWT; ++i)   // slots past the slab read past the tile (still inside wpk or range-checked to 0)
            rw[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w_rs, gwoff, wbase + (unsigned)i * (NTHREADS * 16u), 0));
    };
    auto store_stage = [&](int buf) {
        f32x4* in_s = smem + buf * STAGE_F4;
        f32x4* w_s = in_s + IN_F4;
#pragma unroll
        for (int i = 0; i < NIN; ++i) {
            const int s = tid + i * NTHREADS;
            f32x4* dst = (NIN * NTHREADS == IN_F4 || s < IN_F4) ? in_s + (s & 1) * (IH * IW) + (s >> 1) : smem + 2 * STAGE_F4;
            *dst = rin[i];
        }
#pragma unroll
        for (int i = 0; i < NWT; ++i) {
            const int s = tid + i * NTHREADS;
            f32x4* dst = (NWT * NTHREADS == W_F4 || s < W_F4) ? w_s + s : smem + 2 * STAGE_F4;
            *dst = rw[i];
        }
    };

    // ---- wave -> M-tiles / N-tiles
    const int wm = (TN == 128) ? (wave >> 1) : wave;
    const int wn = (TN == 128) ? (wave & 1) : 0;
    int trow[WM], tcol[WM];  // first tile row / column of each M-tile of this wave
#pragma unroll
    for (int mt = 0; mt < WM; ++mt) {
        if (NARROW) {                    // M-tile t covers tile rows 2t, 2t+1 and all 16 columns
            trow[mt] = 2 * ((TN == 128 ? 4 : 2) * wm + mt);
            tcol[mt] = 0;
        } else if (TN == 128) {
            trow[mt] = 2 * wm + (mt >> 1);
            tcol[mt] = 32 * (mt & 1);
        } else {
            trow[mt] = 2 * (wm >> 1) + mt;
            tcol[mt] = 32 * (wm & 1);
        }
    }
    // pixel m (0..31) of an M-tile -> (row, column) offset inside it
    auto m_row = [](int m) { return NARROW ? (m >> 4) : 0; };
    auto m_col = [](int m) { return NARROW ? (m & 15) : m; };
    int abase[WM];
#pragma unroll
    for (int mt = 0; mt < WM; ++mt)
        abase[mt] = hq * (IH * IW) + (trow[mt] + m_row(l31)) * SH * IW + tcol[mt] + m_col(l31) + (TAPS == 4 ? p.tap_base * (IW + 1) : 0);
    const int wbase = hq * TN + wn * 64 + l31;

    f32x16 acc[WM][WN];
#pragma unroll
    for (int mt = 0; mt < WM; ++mt)
#pragma unroll
        for (int nt = 0; nt < WN; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    // ---- main loop. Per K chunk: 9 taps x 4 k-steps x (WM x WN) MFMAs. The operand fragments of
    // tap t+1 are read from LDS BEFORE the MFMAs of tap t are issued (two register sets), the
    // next chunk's global loads are issued at the top of the chunk and written to the other LDS
    // buffer after tap 4, and the chunk's single barrier sits in front of tap 8 so that the
    // first fragments of the next chunk are fetched behind tap 8's MFMAs: the matrix pipe only
    // idles for the barrier skew.
    f32x4 fa[2][WM], fb[2][WN];
    // DIL: M-tile mt sits on output row 2 wm + (mt >> 1) of an 8-row tile at an even oy0: its input row under tap row kh is real
    // (even) iff (mt >> 1) + kh is odd
    auto live = [](int mt, int tap) { return !DIL || ((((mt >> 1) + tap / 3) & 1) == 1); };
    auto read_frags = [&](int set, const f32x4* in_s, const f32x4* w_s, int tap) {
        const int kh = (TAPS == 4) ? (tap >> 1) : tap / 3, kw = (TAPS == 4) ? (tap & 1) : tap - kh * 3;
#pragma unroll
        for (int mt = 0; mt < WM; ++mt)
            if (live(mt, tap)) fa[set][mt] = in_s[abase[mt] + kh * IW + kw];
#pragma unroll
        for (int nt = 0; nt < WN; ++nt) fb[set][nt] = w_s[tap * 2 * TN + wbase + nt * 32];
    };
    auto mfma_tap = [&](int set, int tap) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mt = 0; mt < WM; ++mt)
                if (live(mt, tap)) {
#pragma unroll
                    for (int nt = 0; nt < WN; ++nt)
                        acc[mt][nt] =
                            __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][mt][j], fb[set][nt][j], acc[mt][nt], 0, 0, 0);
                }
    };

#ifdef WITW_STAMPS
    unsigned long long t_stamp[6];
    int n_stamp = 0;
#define STAMP() do { if (n_stamp < 6) t_stamp[n_stamp++] = __builtin_amdgcn_s_memtime(); } while (0)
    const unsigned long long r_stamp0 = __builtin_amdgcn_s_memrealtime();
#else
#define STAMP() do { } while (0)
#endif
    STAMP();
    load_stage(0);
    store_stage(0);
    __syncthreads();
    read_frags(0, smem, smem + IN_F4, 0);
    STAMP();

    // Issue-order recipe for one tap (LLVM sched groups: 0x8 MFMA, 0x20 VMEM read, 0x100 DS read,
    // 0x200 DS write): every LDS / global instruction is issued alone between MFMAs so that it
    // hides in the shadow of a 64-cycle v_mfma_f32_32x32x2_f32 instead of stalling the pipe.
    constexpr int MPT = 4 * (DIL ? WM / 2 : WM) * WN;   // MFMAs per tap (DIL: half the M-tiles are live under any tap)
    constexpr int RPT = (DIL ? WM / 2 : WM) + WN;       // fragment reads per tap
#define SG_PLAIN_TAP()                                                  \
    do {                                                                \
        _Pragma("unroll") for (int i_ = 0; i_ < RPT; ++i_) {            \
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);          \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);          \
        }                                                               \
        _Pragma("unroll") for (int i_ = 0; i_ < MPT - 2 * RPT; ++i_)    \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);          \
    } while (0)
#define SG_HEAVY_TAP(MASK, NX)                                          \
    do {                                                                \
        _Pragma("unroll") for (int i_ = 0; i_ < RPT; ++i_) {            \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);          \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);          \
        }                                                               \
        _Pragma("unroll") for (int i_ = 0; i_ < (NX); ++i_) {           \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);          \
            __builtin_amdgcn_sched_group_barrier(MASK, 1, 0);           \
        }                                                               \
        _Pragma("unroll") for (int i_ = 0; i_ < MPT - RPT - (NX); ++i_) \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);          \
    } while (0)
    static_assert(MPT - RPT - (NIN + NWT) >= 0, "tap too short to hide the staging instructions");

    if constexpr (TAPS == 4) {
        // 4 taps per chunk: global loads of the next chunk ride under tap 0, its LDS writes under tap 2, the chunk's
        // barrier sits in front of tap 3, behind whose MFMAs the first fragments of the next chunk arrive. An even
        // tap count keeps the fragment sets aligned from chunk to chunk (no register copy).
        for (int kc = 0; kc < nkc; ++kc) {
            const int cur = kc & 1;
            const int kn = (kc + 1 < nkc) ? kc + 1 : kc;
            const f32x4* in_s = smem + cur * STAGE_F4;
            const f32x4* w_s = in_s + IN_F4;
            const f32x4* in_n = smem + (cur ^ 1) * STAGE_F4;
            read_frags(1, in_s, w_s, 1);
            load_stage(kn);
            mfma_tap(0, 0);
            SG_HEAVY_TAP(0x020, NIN + NWT);
            read_frags(0, in_s, w_s, 2);
            mfma_tap(1, 1);
            SG_PLAIN_TAP();
            read_frags(1, in_s, w_s, 3);
            store_stage(cur ^ 1);
            mfma_tap(0, 2);
            SG_HEAVY_TAP(0x200, NIN + NWT);
            __syncthreads();
            read_frags(0, in_n, in_n + IN_F4, 0);
            mfma_tap(1, 3);
            SG_PLAIN_TAP();
        }
    } else {
        for (int kc = 0; kc < nkc; ++kc) {
            const int cur = kc & 1;
            const int kn = (kc + 1 < nkc) ? kc + 1 : kc;   // last chunk restages itself (never read)
            const f32x4* in_s = smem + cur * STAGE_F4;
            const f32x4* w_s = in_s + IN_F4;
            const f32x4* in_n = smem + (cur ^ 1) * STAGE_F4;
            // tap 0 (+ global loads of the next chunk)
            read_frags(1, in_s, w_s, 1);
#ifndef WITW_DIAG_NOSTAGE
            load_stage(kn);
#endif
            mfma_tap(0, 0);
            SG_HEAVY_TAP(0x020, NIN + NWT);
#pragma unroll
            for (int tap = 1; tap < 4; ++tap) {
                read_frags((tap + 1) & 1, in_s, w_s, tap + 1);
                mfma_tap(tap & 1, tap);
                SG_PLAIN_TAP();
            }
            // tap 4 (+ LDS writes of the next chunk)
            read_frags(1, in_s, w_s, 5);
#ifndef WITW_DIAG_NOSTAGE
            store_stage(cur ^ 1);
#endif
            mfma_tap(0, 4);
            SG_HEAVY_TAP(0x200, NIN + NWT);
#pragma unroll
            for (int tap = 5; tap < 8; ++tap) {
                read_frags((tap + 1) & 1, in_s, w_s, tap + 1);
                mfma_tap(tap & 1, tap);
                SG_PLAIN_TAP();
            }
#ifndef WITW_DIAG_NOBARRIER
            __syncthreads();
#endif
            // tap 8, behind which the first fragments of the next chunk arrive
            read_frags(1, in_n, in_n + IN_F4, 0);
            mfma_tap(0, 8);
            SG_PLAIN_TAP();
#pragma unroll
            for (int mt = 0; mt < WM; ++mt) fa[0][mt] = fa[1][mt];
#pragma unroll
            for (int nt = 0; nt < WN; ++nt) fb[0][nt] = fb[1][nt];
        }
    }
#undef SG_PLAIN_TAP
#undef SG_HEAVY_TAP

    STAMP();
    // ---- epilogue: bias, dropout scale, ReLU, optional 2x2 max pool, store
    float bv[WN], dm[WN], ps[WN], pt[WN];
    int nch[WN];
    int act = p.relu;
    bool has_post = p.post_scale != nullptr;
    bool raw = false;          // split-K: the partial sums leave untouched (+0, *1, no activation), splitk_finish_kernel finishes
    if constexpr (TAPS == 4) {
        raw = p.ksplit > 1;
        if (raw) { act = 0; has_post = false; }
    }
#pragma unroll
    for (int nt = 0; nt < WN; ++nt) {
        nch[nt] = n0 + wn * 64 + nt * 32 + l31;
        bv[nt] = raw ? 0.f : p.bias[nch[nt]];
        dm[nt] = 1.f;
        if (p.dropmask != nullptr && nch[nt] < p.Cout) dm[nt] = p.dropmask[(size_t)b * p.Cout + nch[nt]];
        ps[nt] = 1.f;
        pt[nt] = 0.f;
        if (has_post && nch[nt] < p.Cout) {
            ps[nt] = p.post_scale[nch[nt]];
            pt[nt] = p.post_shift[nch[nt]];
        }
    }
    // conv + bias -> Dropout2d scale -> activation -> per-channel affine
    auto fin = [&](float v, int nt) {
        v = (v + bv[nt]) * dm[nt];
        if (act == 1) v = fmaxf(v, 0.f);
        else if (act == 2) v = v > 0.f ? v : v * p.lrelu;
        if (has_post) v = v * ps[nt] + pt[nt];
        return v;
    };
    const int Hy = POOL ? (p.Ho >> 1) : p.Ho;
    const int Wy = POOL ? (p.Wo >> 1) : p.Wo;

    auto emit = [&](float v, int nt, int yy, int xx) {
        v = fin(v, nt);
        if (yy < Hy && xx < Wy && nch[nt] < p.Cout) {
            size_t o;
            if (p.out_nchw)
                o = (((size_t)b * p.Cout + nch[nt]) * Hy + yy) * Wy + xx;
            else
                o = (((size_t)b * Hy + yy) * Wy + xx) * p.Cout + nch[nt];
            if (p.gate != nullptr && !(p.gate[o] > 0.f)) v = 0.f;
            p.y[o] = v;
        }
    };

    if (!POOL && !p.out_nchw && (p.Cout & 3) == 0) {
        // Wide NHWC store: one M-tile (32 pixels x this wave's 64 channels) at a time is transposed
        // through a wave-private 8 KB LDS slab (the staging buffers are dead: every useful fragment
        // read precedes the loop's last barrier) and leaves as 16-byte stores, 4 pixels x 256 B per
        // wave-instruction, instead of 4-byte stores straight from the accumulator layout.
        float* slab = reinterpret_cast<float*>(smem) + wave * (32 * 64);
        const int prow = lane >> 4, pc4 = (lane & 15) * 4;   // read-back role: pixel row in a group of 4, channel quad
#pragma unroll
        for (int mt = 0; mt < WM; ++mt) {
#pragma unroll
            for (int nt = 0; nt < WN; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = fin(acc[mt][nt][r], nt);
                    slab[((r & 3) + 8 * (r >> 2) + 4 * hq) * 64 + nt * 32 + l31] = v;
                }
            const int nbase = n0 + wn * 64 + pc4;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const int m = g * 4 + prow;
                const f32x4 v = *reinterpret_cast<const f32x4*>(slab + m * 64 + pc4);
                const int yy = oy0 + trow[mt] + m_row(m);
                const int xx = ox0 + tcol[mt] + m_col(m);
                bool ok = yy < Hy && xx < Wy && nbase < p.Cout;
                size_t o = (((size_t)b * Hy + yy) * Wy + xx) * p.Cout + nbase;
                f32x4 w = v;
                if constexpr (TAPS == 4) {
                    if (p.ksplit > 1) {
                        o += (size_t)blockIdx.y * p.split_stride;
                    } else if (p.s2d) {
                        ok = yy < 2 * p.s2d_h && xx < 2 * p.s2d_w && nbase < p.Cout;
                        o = ((((size_t)b * p.s2d_h + (yy >> 1)) * p.s2d_w + (xx >> 1)) * 4 + (yy & 1) * 2 + (xx & 1)) * p.Cout + nbase;
                        if (!(yy < p.valid_h && xx < p.valid_w)) w = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                }
                if (ok) {
                    if (p.gate != nullptr) {
                        const f32x4 gt = *reinterpret_cast<const f32x4*>(p.gate + o);
#pragma unroll
                        for (int e = 0; e < 4; ++e) w[e] = gt[e] > 0.f ? v[e] : 0.f;
                    }
                    __builtin_nontemporal_store(w, reinterpret_cast<f32x4*>(p.y + o));
                }
            }
        }
    } else if (!POOL) {
#pragma unroll
        for (int mt = 0; mt < WM; ++mt)
#pragma unroll
            for (int nt = 0; nt < WN; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = (r & 3) + 8 * (r >> 2) + 4 * hq;
                    emit(acc[mt][nt][r], nt, oy0 + trow[mt] + m_row(m), ox0 + tcol[mt] + m_col(m));
                }
    } else if (NARROW) {
        // Narrow geometry: both rows of a pooling window sit in ONE M-tile (registers r and r+8), its two columns in
        // registers r and r+1: 8 pooled pixels (1 row x 8 columns) per M-tile, all in-lane.
#pragma unroll
        for (int mt = 0; mt < WM; ++mt) {
            const int yy = (oy0 + trow[mt]) >> 1;
#pragma unroll
            for (int nt = 0; nt < WN; ++nt)
#pragma unroll
                for (int r = 0; r < 8; r += 2) {
                    const float a00 = acc[mt][nt][r], a01 = acc[mt][nt][r + 1];
                    const float a10 = acc[mt][nt][r + 8], a11 = acc[mt][nt][r + 9];
                    const float m = fmaxf(fmaxf(a00, a01), fmaxf(a10, a11));
                    const int xx = (ox0 >> 1) + (((r & 3) >> 1) | (hq << 1) | (((r >> 2) & 1) << 2));
                    emit(m, nt, yy, xx);
                    if (p.pool_code != nullptr && yy < Hy && xx < Wy && nch[nt] < p.Cout) {
                        const int code = (a00 == m) ? 0 : (a01 == m) ? 1 : (a10 == m) ? 2 : 3;
                        p.pool_code[(((size_t)b * Hy + yy) * Wy + xx) * p.Cout + nch[nt]] = (unsigned char)code;
                    }
                }
        }
    } else if ((p.Cout & 3) == 0 && p.gate == nullptr) {
        // Fused 2x2 max-pool, wide store: rows (2a, 2a+1) of one column half sit in M-tiles (mtA, mtB) of this
        // wave; the 16 pooled pixels x 64 channels of the pair go through the wave-private LDS slab and leave
        // as 16-byte stores (4 pooled pixels x 256 B per wave-instruction).
        float* slab = reinterpret_cast<float*>(smem) + wave * (32 * 64);
        const int prow = lane >> 4, pc4 = (lane & 15) * 4;
#pragma unroll
        for (int pr = 0; pr < WM / 2; ++pr) {
            const int mtA = (TN == 128) ? (pr & 1) : 0;       // TN==128: tiles {0,1}=row0 halves, {2,3}=row1
            const int mtB = (TN == 128) ? (2 + (pr & 1)) : 1;
            const int yy = (oy0 + trow[mtA]) >> 1;
            const int xb = (ox0 + tcol[mtA]) >> 1;
#pragma unroll
            for (int nt = 0; nt < WN; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const float a00 = acc[mtA][nt][4 * g + 2 * e], a01 = acc[mtA][nt][4 * g + 2 * e + 1];
                        const float a10 = acc[mtB][nt][4 * g + 2 * e], a11 = acc[mtB][nt][4 * g + 2 * e + 1];
                        const float m = fmaxf(fmaxf(a00, a01), fmaxf(a10, a11));
                        const int pc = 4 * g + 2 * hq + e;
                        slab[pc * 64 + nt * 32 + l31] = fin(m, nt);
                        if (p.pool_code != nullptr && yy < Hy && xb + pc < Wy && nch[nt] < p.Cout) {
                            // first position attaining the max, scan order (0,0),(0,1),(1,0),(1,1) as torch's max_pool2d
                            const int code = (a00 == m) ? 0 : (a01 == m) ? 1 : (a10 == m) ? 2 : 3;
                            p.pool_code[(((size_t)b * Hy + yy) * Wy + xb + pc) * p.Cout + nch[nt]] = (unsigned char)code;
                        }
                    }
            const int nbase = n0 + wn * 64 + pc4;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int pc = g * 4 + prow;
                const f32x4 v = *reinterpret_cast<const f32x4*>(slab + pc * 64 + pc4);
                if (yy < Hy && xb + pc < Wy && nbase < p.Cout)
                    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p.y + (((size_t)b * Hy + yy) * Wy + xb + pc) * p.Cout + nbase));
            }
        }
    } else {
        // rows (2a, 2a+1) of one column half sit in M-tiles (mtA, mtB) of this wave
#pragma unroll
        for (int pr = 0; pr < WM / 2; ++pr) {
            const int mtA = (TN == 128) ? (pr & 1) : 0;       // TN==128: tiles {0,1}=row0 halves, {2,3}=row1
            const int mtB = (TN == 128) ? (2 + (pr & 1)) : 1;
#pragma unroll
            for (int nt = 0; nt < WN; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const float a00 = acc[mtA][nt][4 * g + 2 * e], a01 = acc[mtA][nt][4 * g + 2 * e + 1];
                        const float a10 = acc[mtB][nt][4 * g + 2 * e], a11 = acc[mtB][nt][4 * g + 2 * e + 1];
                        const float v0 = fmaxf(a00, a01);
                        const float v1 = fmaxf(a10, a11);
                        const int yy = (oy0 + trow[mtA]) >> 1;
                        const int xx = ((ox0 + tcol[mtA]) >> 1) + 4 * g + 2 * hq + e;
                        emit(fmaxf(v0, v1), nt, yy, xx);
                        if (p.pool_code != nullptr && yy < Hy && xx < Wy && nch[nt] < p.Cout) {
                            // first position attaining the max, scan order (0,0),(0,1),(1,0),(1,1) as torch's max_pool2d
                            const float m = fmaxf(v0, v1);
                            const int code = (a00 == m) ? 0 : (a01 == m) ? 1 : (a10 == m) ? 2 : 3;
                            p.pool_code[(((size_t)b * Hy + yy) * Wy + xx) * p.Cout + nch[nt]] = (unsigned char)code;
                        }
                    }
        }
    }
#ifdef WITW_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP();
    if (lane == 0 && p.stamps != nullptr) {
        unsigned long long* o = p.stamps + ((size_t)blockIdx.x * NW + wave) * 8;
        for (int i = 0; i < n_stamp; ++i) o[i] = t_stamp[i];
        o[6] = __builtin_amdgcn_s_memrealtime() - r_stamp0;      // 100 MHz ticks over the same span as o[3] - o[0]
        o[7] = n_stamp;
    }
#endif
}

// One thread per packed float4: wpk[nt][kc][tap][q][n][0..3] <- w[cout][cin][kh][kw]
// (torch KCRS). transpose_flip!=0 builds the dgrad filter instead: roles of cin/cout
// swapped and taps rotated by 180 degrees (w'[ci][co][kh][kw] = w[co][ci][2-kh][2-kw]).
// taps = 9: all of the window; taps = 4: the 2x2 sub-window (tap_base + {0,1})^2 of the PACKED filter (TAPS = 4 kernels).
__global__ void pack_weights_kernel(const float* __restrict__ w, float* __restrict__ wpk, int Cout, int Cin,
                                    int n_tiles, int nkc, int TN, int transpose_flip, int src_cout, int src_cin, int taps,
                                    int tap_base) {
    const size_t total = (size_t)n_tiles * nkc * taps * 2 * TN;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    size_t t = idx;
    const int n = t % TN; t /= TN;
    const int q = t % 2; t /= 2;
    const int tap = t % taps; t /= taps;
    const int kc = t % nkc; t /= nkc;
    const int nt = (int)t;
    const int kh = (taps == 4) ? tap_base + (tap >> 1) : tap / 3, kw = (taps == 4) ? tap_base + (tap & 1) : tap % 3;
    const int co = nt * TN + n;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = kc * 8 + q * 4 + j;
        if (co < Cout && ci < Cin) {
            if (!transpose_flip)
                v[j] = w[(((size_t)co * src_cin + ci) * 3 + kh) * 3 + kw];
            else
                v[j] = w[(((size_t)ci * src_cin + co) * 3 + (2 - kh)) * 3 + (2 - kw)];
        }
    }
    reinterpret_cast<f32x4*>(wpk)[idx] = v;
}

// Winograd filter of conv_wino_h2, one thread per packed float4: wpk[nt][kc][kw][t][q][n][0..3] (64-channel tiles) from
// w[cout][cin][3][3] (torch KCRS), per column tap kw with g_kh = w[..][kh][kw]:
//   U0 = g0, U1 = ((g0+g1)+g2)*0.5, U2 = ((g0-g1)+g2)*0.5, U3 = g2   (exact x0.5; the library is built without contraction)
__global__ void pack_weights_wino_kernel(const float* __restrict__ w, float* __restrict__ wpk, int Cout, int Cin, int nkc,
                                         size_t total) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    size_t t = idx;
    const int n = t % 64; t /= 64;
    const int q = t % 2; t /= 2;
    const int tr = t % 4; t /= 4;
    const int kw = t % 3; t /= 3;
    const int kc = t % nkc; t /= nkc;
    const int co = (int)t * 64 + n;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = kc * 8 + q * 4 + j;
        if (co < Cout && ci < Cin) {
            const float* g = w + ((size_t)co * Cin + ci) * 9 + kw;
            const float g0 = g[0], g1 = g[3], g2 = g[6];
            v[j] = tr == 0 ? g0 : tr == 1 ? ((g0 + g1) + g2) * 0.5f : tr == 2 ? ((g0 - g1) + g2) * 0.5f : g2;
        }
    }
    reinterpret_cast<f32x4*>(wpk)[idx] = v;
}

// NCHW [B,C,H,W] -> NHWC8 [B,H,W,8], channels >= C zero filled (C <= 8).
__global__ void nchw_to_nhwc8_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int C, int H, int W) {
    const size_t npix = (size_t)B * H * W;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix) return;
    const size_t hw = (size_t)H * W;
    const size_t b = idx / hw, r = idx - b * hw;
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = (c < C) ? x[(b * C + c) * hw + r] : 0.f;
    f32x4* o = reinterpret_cast<f32x4*>(y + idx * 8);
    o[0] = f32x4{v[0], v[1], v[2], v[3]};
    o[1] = f32x4{v[4], v[5], v[6], v[7]};
}

// NCHW [B,C,H,W] -> NHWC [B,H,W,Cp] (Cp >= C, extra channels zero) and back; small tensors (embedding grads).
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int Cp, size_t hw, size_t total) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = idx % Cp;
    const size_t t = idx / Cp;
    const size_t b = t / hw, r = t - b * hw;
    y[idx] = (c < C) ? x[(b * C + c) * hw + r] : 0.f;
}

int env_int(const char* name, int dflt);
int wino_run();
int wino_dma();

template <int TN, int SH, bool POOL, int NW, int GEO, int TAPS = 9>
int launch_conv_nw(ConvArgs a, hipStream_t st) {
    a.tiles_y = cdiv(a.Ho, GEO == 1 ? 4 * NW : NW);
    a.tiles_x = cdiv(a.Wo, GEO == 1 ? 16 : 64);
    const long long sp_total = (long long)a.B * a.tiles_x * a.tiles_y;
    a.n_tiles = cdiv(a.Cout, a.wino ? 64 : TN);      // the Winograd form tiles 64 output channels per workgroup
    a.sp_per_xcd = (int)((sp_total + 7) / 8);
    // fewer spatial tiles than XCDs: the XCD-aware order would put every workgroup (all n tiles and K slices of a spatial tile) on
    // sp_total of the 8 XCDs -- cvig_baseline's last block, 2 mosaics x 4 n tiles x 32 K slices, ran on 64 of the 256 CUs
    if (sp_total < 8) a.xcd_map = 0;
    const long long grid = a.xcd_map ? 8LL * a.sp_per_xcd * a.n_tiles : sp_total * a.n_tiles;
    if (grid <= 0 || grid > 0x7fffffffLL || sp_total > 0x7fffffffLL) {
        witw_set_error("conv3x3: grid %lld out of range", grid);
        return WITW_ERR_INVALID;
    }
    a.sp_total = (int)sp_total;
    const unsigned gy = (TAPS == 4 && a.ksplit > 1) ? (unsigned)a.ksplit : 1u;
    // the Winograd form: at most one workgroup per CU, each walking a run of the map's indices (wino_run() off: one index each)
    a.wino_items = (int)grid;
    a.wino_wgs = (int)grid;
    if (a.wino && wino_run()) {
        const int forced = env_int("WITW_CONV_WINO_WGS", 0);      // test aid: runs of more than one item on small shapes
        a.wino_wgs = (int)std::min<long long>(grid, forced > 0 ? forced : witw_cu_count());
    }
    a.wino_dma = a.wino ? wino_dma() : 0;
    hipLaunchKernelGGL((conv3x3_nhwc_f32_kernel<TN, SH, POOL, NW, GEO, TAPS>), dim3(a.wino ? (unsigned)a.wino_wgs : (unsigned)grid, gy),
                       dim3(64 * NW), 0, st, a);
    WITW_CHECK_LAUNCH("conv3x3_nhwc_f32");
    witw_note_variant("conv3x3_nhwc_f32_kernel<%d,%d,%s,%d,%d,%d>", TN, SH, POOL ? "true" : "false", NW, GEO, TAPS);
    if (a.wino) witw_note_conv_form("wino_h2");
    return WITW_OK;
}

// 8-wave workgroups (8-row tiles) when no rows are wasted and the grid fills its rounds of one workgroup per CU (api.hip)
int choose_waves(int B, int Ho, int Wo, int Cout, int force_nw) {
    const int TN = (Cout >= 128) ? 128 : 64;
    const long long big = (long long)cdiv(Cout, TN) * B * cdiv(Wo, TW_WIDE) * cdiv(Ho, 8);
    if (force_nw == 4) return 4;
    return (force_nw == 8 || ((Ho % 8) == 0 && witw_fills_rounds(big))) ? 8 : 4;
}

// narrow geometry (2x16-pixel M-tiles, 16-column workgroup tiles) for maps of at most 32 columns
bool choose_narrow(int Wo, int force_geo) { return force_geo == 1 || (force_geo != 0 && Wo <= 32); }

int env_int(const char* name, int dflt) {
    const char* e = getenv(name);      // tuning / test aids: WITW_CONV_NW in {4,8}, WITW_CONV_GEO in {0,1}
    return e ? atoi(e) : dflt;
}

// 1 (default): the dgrad of a stride-(2,1) layer on the 8-wave 128-channel tile skips the products with zero-interleaved rows
// (GEO = 2); 0: it multiplies them like any other (WITW_CONV_DILSKIP=0 / witw_conv3x3_dil_skip(0): A/B runs, the bitwise test)
int g_dil_skip = -1;
int dil_skip() {
    if (g_dil_skip < 0) {
        const char* e = getenv("WITW_CONV_DILSKIP");
        g_dil_skip = e ? (atoi(e) != 0) : 1;
    }
    return g_dil_skip;
}

// 1 (default): a launch given a Winograd-packed filter runs the F(2,3)-along-H form where its class has one; 0: the direct form
// (WITW_CONV_WINO=0 / witw_conv3x3_wino(0): A/B runs)
int g_wino = -1;
int wino_on() {
    if (g_wino < 0) {
        const char* e = getenv("WITW_CONV_WINO");
        g_wino = e ? (atoi(e) != 0) : 1;
    }
    return g_wino;
}

// 1 (default): a Winograd launch starts one workgroup per CU and each walks a run of tiles with one continuous K loop; 0: one
// workgroup per tile (WITW_CONV_WINO_RUN=0 / witw_conv3x3_wino_run(0): A/B runs, the bitwise tests)
int g_wino_run = -1;
int wino_run() {
    if (g_wino_run < 0) {
        const char* e = getenv("WITW_CONV_WINO_RUN");
        g_wino_run = e ? (atoi(e) != 0) : 1;
    }
    return g_wino_run;
}

// 1 (default): a Winograd launch stages its K chunks by LDS-DMA; 0: through registers (WITW_CONV_WINO_DMA=0 /
// witw_conv3x3_wino_dma(0): A/B runs, the bitwise tests)
int g_wino_dma = -1;
int wino_dma() {
    if (g_wino_dma < 0) {
        const char* e = getenv("WITW_CONV_WINO_DMA");
        g_wino_dma = e ? (atoi(e) != 0) : 1;
    }
    return g_wino_dma;
}

template <int TN, int SH, bool POOL>
int launch_conv(ConvArgs a, hipStream_t st) {
    // the Winograd form: stride 1, 3x3, wide geometry, plain inference epilogue (no gate / dil_h / NCHW / affine), Cout % 4 == 0
    const bool wino = SH == 1 && (TN == 128 || POOL) && a.wpk_wino != nullptr && wino_on() && a.gate == nullptr && !a.dil_h &&
                      !a.out_nchw && a.post_scale == nullptr && (a.Cout & 3) == 0 && a.force_geo != 1 &&
                      !choose_narrow(a.Wo, a.force_geo);
    a.wino = wino ? 1 : 0;
    if (wino) return choose_waves(a.B, a.Ho, a.Wo, a.Cout, a.force_nw) == 8 ? launch_conv_nw<TN, SH, POOL, 8, 0>(a, st)
                                                                          : launch_conv_nw<TN, SH, POOL, 4, 0>(a, st);
#ifndef WITW_NO_NARROW
    if (choose_narrow(a.Wo, a.force_geo)) return launch_conv_nw<TN, SH, POOL, 4, 1>(a, st);
#endif
    if (choose_waves(a.B, a.Ho, a.Wo, a.Cout, a.force_nw) == 8) {
        if constexpr (TN == 128 && SH == 1 && !POOL) {
            if (a.dil_h && dil_skip()) return launch_conv_nw<TN, SH, POOL, 8, 2>(a, st);      // dead (M-tile, tap) products not issued
        }
        return launch_conv_nw<TN, SH, POOL, 8, 0>(a, st);
    }
    return launch_conv_nw<TN, SH, POOL, 4, 0>(a, st);
}

// 2x2 sub-window kernels (stride 1, no pool)
template <int TN>
int launch_conv_taps4(const ConvArgs& a, hipStream_t st) {
#ifndef WITW_NO_NARROW
    if (choose_narrow(a.Wo, a.force_geo)) return launch_conv_nw<TN, 1, false, 4, 1, 4>(a, st);
#endif
    if (choose_waves(a.B, a.Ho, a.Wo, a.Cout, a.force_nw) == 8) return launch_conv_nw<TN, 1, false, 8, 0, 4>(a, st);
    return launch_conv_nw<TN, 1, false, 4, 0, 4>(a, st);
}

}  // namespace

#ifdef WITW_STAMPS
unsigned long long* witw_conv_stamps_ptr = nullptr;
#endif

extern "C" {

int witw_conv3x3_tile_n(int cout) { return cout >= 128 ? 128 : 64; }

// waves per workgroup (4 or 8) the launcher picks for a layer: names the kernel instantiation
// conv3x3_nhwc_f32_kernel<tile_n, stride_h, pool, waves> that a profile will show
int witw_conv3x3_workgroup_waves(int B, int H, int W, int Cout, int stride_h) {
    if (B <= 0 || H <= 0 || W <= 0 || Cout <= 0 || (stride_h != 1 && stride_h != 2)) return -1;
    if (choose_narrow(W, env_int("WITW_CONV_GEO", -1))) return 4;
    return choose_waves(B, (H + 2 - 3) / stride_h + 1, W, Cout, env_int("WITW_CONV_NW", 0));
}

long long witw_conv3x3_packed_floats(int cout, int cin) {
    if (cout <= 0 || cin <= 0) return -1;
    const int TN = witw_conv3x3_tile_n(cout);
    const long long n_tiles = cdiv(cout, TN), nkc = cdiv(cin, 8);
    return n_tiles * nkc * 9 * 2 * TN * 4;
}

int witw_conv3x3_bias_floats(int cout) {
    const int TN = witw_conv3x3_tile_n(cout);
    return cdiv(cout, TN) * TN;
}

int witw_conv3x3_pack_weights(const float* w_kcrs, float* wpk, int cout, int cin, int transpose_flip, void* stream) {
    WITW_CHECK_ARG(w_kcrs && wpk, "pack_weights: null pointer");
    WITW_CHECK_ARG(cout > 0 && cin > 0, "pack_weights: bad shape cout=%d cin=%d", cout, cin);
    const int TN = witw_conv3x3_tile_n(cout);
    const int n_tiles = cdiv(cout, TN), nkc = cdiv(cin, 8);
    const size_t total = (size_t)n_tiles * nkc * 9 * 2 * TN;
    // in transpose_flip mode (cout,cin) describe the PACKED filter; the source tensor is [cin][cout][3][3]
    const int src_cin = transpose_flip ? cout : cin;
    hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       w_kcrs, wpk, cout, cin, n_tiles, nkc, TN, transpose_flip, cout, src_cin, 9, 0);
    WITW_CHECK_LAUNCH("pack_weights");
    return WITW_OK;
}

// ---- 2x2 sub-window form (cvig_baseline's Conv2d(k=4,s=2) over the space-to-depth image, model/cvig_baseline.py:236-252)
long long witw_conv3x3_packed_floats_taps4(int cout, int cin) {
    if (cout <= 0 || cin <= 0) return -1;
    const int TN = witw_conv3x3_tile_n(cout);
    return (long long)cdiv(cout, TN) * cdiv(cin, 8) * 4 * 2 * TN * 4;
}

// Packs 4 of the 9 taps of a [cout][cin][3][3] filter: rows/columns {1,2} (transpose_flip = 0: the forward filter whose
// first tap row/column are zero) or, with transpose_flip, rows/columns {0,1} of the transposed, 180-degree rotated filter
// (its dgrad filter, source tensor [cin][cout][3][3] as in witw_conv3x3_pack_weights).
int witw_conv3x3_pack_weights_taps4(const float* w_kcrs, float* wpk, int cout, int cin, int transpose_flip, void* stream) {
    WITW_CHECK_ARG(w_kcrs && wpk, "pack_weights_taps4: null pointer");
    WITW_CHECK_ARG(cout > 0 && cin > 0, "pack_weights_taps4: bad shape cout=%d cin=%d", cout, cin);
    const int TN = witw_conv3x3_tile_n(cout);
    const int n_tiles = cdiv(cout, TN), nkc = cdiv(cin, 8);
    const size_t total = (size_t)n_tiles * nkc * 4 * 2 * TN;
    const int src_cin = transpose_flip ? cout : cin;
    hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       w_kcrs, wpk, cout, cin, n_tiles, nkc, TN, transpose_flip, cout, src_cin, 4, transpose_flip ? 0 : 1);
    WITW_CHECK_LAUNCH("pack_weights_taps4");
    return WITW_OK;
}

// workgroups the taps4 launcher would start for this shape (ksplit = 1)
static long long taps4_workgroups(int B, int H, int W, int Cout) {
    const int TN = witw_conv3x3_tile_n(Cout);
    const long long nt = cdiv(Cout, TN);
    if (choose_narrow(W, env_int("WITW_CONV_GEO", -1))) return nt * B * cdiv(H, 16) * cdiv(W, 16);
    const int nw = choose_waves(B, H, W, Cout, env_int("WITW_CONV_NW", 0));
    return nt * B * cdiv(H, nw) * cdiv(W, 64);
}

// Split-K factor the taps4 conv should run with: 1 when the plain launch already fills the chip (>= 2 workgroups per CU) or K
// is short; otherwise enough K slices for ~4 workgroups per CU, each at least 32 K-chunks (256 input channels) long. The deep
// cvig_baseline layers (16x16 .. 4x4 maps, K = 4 taps x 2048) start 8 .. 128 workgroups on 256 CUs without it.
int witw_conv3x3_taps4_ksplit(int B, int H, int W, int Cin, int Cout) {
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return -1;
    const int forced = env_int("WITW_CONV_KSPLIT", 0);
    const int nkc = Cin >> 3;
    const long long wg = taps4_workgroups(B, H, W, Cout);
    int S = 1;
    if (forced > 0) S = forced;
    else if (wg < 512 && nkc >= 64) {
        S = (int)std::min<long long>(32, (1024 + wg - 1) / wg);
        // at least 32 chunks per slice -- 8 when the whole launch would not even reach one workgroup per CU otherwise (the 1 x 1 map of
        // cvig_baseline's last block: 8 tiles; 8 slices of 32 chunks ran 125 us on 64 CUs)
        S = std::min(S, wg * (nkc / 32) >= 256 ? nkc / 32 : nkc / 8);
    }
    S = std::max(1, std::min(S, nkc));
    const int per = cdiv(nkc, S);
    return cdiv(nkc, per);            // no empty slice
}

// y = act(conv over the 2x2 taps (tap_base + {0,1})^2 of the 3x3 window, zero padding 1) [* post_scale + post_shift],
// gate as in witw_conv3x3_fwd_ex. tap_base = 1 with a forward-packed filter, 0 with a transpose_flip-packed one.
//   ksplit > 1: split-K. y is a workspace of ksplit * B*H*W*Cout floats that receives the RAW partial sums of each K slice
//     ([ksplit][B,H,W,Cout]); bias / activation / affine are NOT applied (witw_taps4_splitk_finish does that), gate must be null.
//   s2d != 0 (ksplit == 1): y is the space-to-depth(2) image of the valid region, [B, ceil(valid_h/2), ceil(valid_w/2), 4*Cout]
//     with channel ((row&1)*2 + (col&1))*Cout + c and zeros outside the valid region: what the next k=4,s=2 layer reads.
int witw_conv3x3_fwd_taps4_ex(const float* x, const float* wpk4, const float* bias, const float* gate, const float* post_scale,
                              const float* post_shift, float* y, int B, int H, int W, int Cin, int Cout, int relu,
                              float lrelu_slope, int tap_base, int ksplit, int s2d, int valid_h, int valid_w, void* stream) {
    WITW_CHECK_ARG(x && wpk4 && bias && y, "conv3x3_fwd_taps4: null pointer");
    WITW_CHECK_ARG(B > 0 && H > 0 && W > 0 && Cout > 0, "conv3x3_fwd_taps4: bad shape B=%d H=%d W=%d Cout=%d", B, H, W, Cout);
    WITW_CHECK_ARG(Cin > 0 && (Cin % 8) == 0, "conv3x3_fwd_taps4: Cin=%d must be a positive multiple of 8", Cin);
    WITW_CHECK_ARG(relu >= 0 && relu <= 2, "conv3x3_fwd_taps4: activation %d unknown (0 none, 1 ReLU, 2 LeakyReLU)", relu);
    WITW_CHECK_ARG(tap_base == 0 || tap_base == 1, "conv3x3_fwd_taps4: tap_base=%d outside {0,1}", tap_base);
    WITW_CHECK_ARG((post_scale == nullptr) == (post_shift == nullptr), "conv3x3_fwd_taps4: post_scale and post_shift go together");
    WITW_CHECK_ARG(ksplit >= 1 && ksplit <= 65535 && ksplit <= (Cin >> 3), "conv3x3_fwd_taps4: ksplit=%d outside [1, Cin/8]", ksplit);
    WITW_CHECK_ARG(!(ksplit > 1 && (gate || s2d)), "conv3x3_fwd_taps4: split-K writes raw partial sums (no gate, no s2d output)");
    WITW_CHECK_ARG(!((ksplit > 1 || s2d) && (Cout & 3)), "conv3x3_fwd_taps4: split-K / s2d output need Cout %% 4 == 0, got %d", Cout);
    WITW_CHECK_ARG(!(s2d && gate), "conv3x3_fwd_taps4: s2d output with gate unsupported");
    WITW_CHECK_ARG(!s2d || (valid_h > 0 && valid_w > 0 && valid_h <= H && valid_w <= W),
                   "conv3x3_fwd_taps4: valid region %dx%d outside the %dx%d map", valid_h, valid_w, H, W);
    WITW_CHECK_ARG(!s2d || (2 * ((valid_h + 1) / 2) <= H && 2 * ((valid_w + 1) / 2) <= W),
                   "conv3x3_fwd_taps4: s2d output of an odd valid size needs one more computed row / column");
    ConvArgs a;
    a.x = x; a.wpk = wpk4; a.bias = bias; a.dropmask = nullptr; a.gate = gate; a.y = y;
    a.post_scale = post_scale; a.post_shift = post_shift; a.lrelu = lrelu_slope;
    a.pool_code = nullptr;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
    a.Ho = H; a.Wo = W;
    a.tiles_x = 0; a.tiles_y = 0;
    a.force_nw = env_int("WITW_CONV_NW", 0);
    a.force_geo = env_int("WITW_CONV_GEO", -1);
    a.xcd_map = env_int("WITW_CONV_XCD", 1) != 0;
    a.circ = 0; a.relu = relu; a.out_nchw = 0; a.dil_h = 0; a.tap_base = tap_base;
    a.ksplit = ksplit;
    a.wino = 0; a.wpk_wino = nullptr;
    a.kc_per_split = cdiv(Cin >> 3, ksplit);
    WITW_CHECK_ARG((long long)(ksplit - 1) * a.kc_per_split < (Cin >> 3), "conv3x3_fwd_taps4: ksplit=%d leaves an empty K slice", ksplit);
    a.split_stride = (size_t)B * H * W * Cout;
    a.s2d = s2d ? 1 : 0;
    a.valid_h = valid_h; a.valid_w = valid_w;
    a.s2d_h = (valid_h + 1) / 2; a.s2d_w = (valid_w + 1) / 2;
#ifdef WITW_STAMPS
    a.stamps = witw_conv_stamps_ptr;
#endif
    hipStream_t st = (hipStream_t)stream;
    return witw_conv3x3_tile_n(Cout) == 128 ? launch_conv_taps4<128>(a, st) : launch_conv_taps4<64>(a, st);
}

int witw_conv3x3_fwd_taps4(const float* x, const float* wpk4, const float* bias, const float* gate, const float* post_scale,
                           const float* post_shift, float* y, int B, int H, int W, int Cin, int Cout, int relu,
                           float lrelu_slope, int tap_base, void* stream) {
    return witw_conv3x3_fwd_taps4_ex(x, wpk4, bias, gate, post_scale, post_shift, y, B, H, W, Cin, Cout, relu, lrelu_slope,
                                     tap_base, 1, 0, 0, 0, stream);
}

int witw_nchw_to_nhwc8(const float* x, float* y, int B, int C, int H, int W, void* stream) {
    WITW_CHECK_ARG(x && y, "nchw_to_nhwc8: null pointer");
    WITW_CHECK_ARG(B > 0 && C > 0 && C <= 8 && H > 0 && W > 0, "nchw_to_nhwc8: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
    const size_t npix = (size_t)B * H * W;
    hipLaunchKernelGGL(nchw_to_nhwc8_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y,
                       B, C, H, W);
    WITW_CHECK_LAUNCH("nchw_to_nhwc8");
    return WITW_OK;
}

int witw_nchw_to_nhwc(const float* x, float* y, int B, int C, int H, int W, int Cpad, void* stream) {
    WITW_CHECK_ARG(x && y, "nchw_to_nhwc: null pointer");
    WITW_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && Cpad >= C, "nchw_to_nhwc: bad shape");
    const size_t total = (size_t)B * H * W * Cpad;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, C,
                       Cpad, (size_t)H * W, total);
    WITW_CHECK_LAUNCH("nchw_to_nhwc");
    return WITW_OK;
}

}  // extern "C"

namespace {

int conv3x3_fwd_any(const float* x, const float* wpk, const float* wpk_wino, const float* bias, const float* dropmask,
                    const float* gate, const float* post_scale, const float* post_shift, float* y, unsigned char* pool_code, int B,
                    int H, int W, int Cin, int Cout, int stride_h, int pad_circular, int relu, float lrelu_slope, int pool,
                    int out_nchw, int dilate_h, void* stream) {
    WITW_CHECK_ARG(x && wpk && bias && y, "conv3x3_fwd: null pointer");
    WITW_CHECK_ARG(B > 0 && H > 0 && W > 0 && Cout > 0, "conv3x3_fwd: bad shape B=%d H=%d W=%d Cout=%d", B, H, W, Cout);
    WITW_CHECK_ARG(Cin > 0 && (Cin % 8) == 0, "conv3x3_fwd: Cin=%d must be a positive multiple of 8", Cin);
    WITW_CHECK_ARG(stride_h == 1 || stride_h == 2, "conv3x3_fwd: stride_h=%d unsupported", stride_h);
    WITW_CHECK_ARG(!(pool && stride_h == 2), "conv3x3_fwd: pool with stride 2 unsupported");
    WITW_CHECK_ARG(!(pool && out_nchw), "conv3x3_fwd: pool with NCHW output unsupported");
    WITW_CHECK_ARG(!(pool && gate), "conv3x3_fwd: pool with gate unsupported");
    WITW_CHECK_ARG(!(dilate_h && stride_h == 2), "conv3x3_fwd: dilated input with stride 2 unsupported");
    WITW_CHECK_ARG(relu >= 0 && relu <= 2, "conv3x3_fwd: activation %d unknown (0 none, 1 ReLU, 2 LeakyReLU)", relu);
    WITW_CHECK_ARG((post_scale == nullptr) == (post_shift == nullptr), "conv3x3_fwd: post_scale and post_shift go together");
    WITW_CHECK_ARG(!(pool && relu == 2) && !(pool && post_scale), "conv3x3_fwd: pool needs a monotone epilogue (ReLU only)");
    ConvArgs a;
    a.x = x; a.wpk = wpk; a.bias = bias; a.dropmask = dropmask; a.gate = gate; a.y = y;
    a.post_scale = post_scale; a.post_shift = post_shift; a.lrelu = lrelu_slope;
    a.pool_code = pool ? pool_code : nullptr;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
    a.Ho = (H + 2 - 3) / stride_h + 1;
    a.Wo = W;
    a.tiles_x = 0;
    a.tiles_y = 0;   // set by the launcher for the chosen tile height
    a.force_nw = env_int("WITW_CONV_NW", 0);
    a.force_geo = env_int("WITW_CONV_GEO", -1);
    a.xcd_map = env_int("WITW_CONV_XCD", 1) != 0;      // 0: plain n-tile-major order (A/B timing)
    a.circ = pad_circular; a.relu = relu; a.out_nchw = out_nchw; a.dil_h = dilate_h; a.tap_base = 0;
    a.ksplit = 1; a.kc_per_split = 0; a.split_stride = 0; a.s2d = 0; a.s2d_h = a.s2d_w = a.valid_h = a.valid_w = 0;
    a.wino = 0; a.wpk_wino = wpk_wino;      // the launcher decides the form
#ifdef WITW_STAMPS
    a.stamps = witw_conv_stamps_ptr;
#endif
    hipStream_t st = (hipStream_t)stream;
    const int TN = witw_conv3x3_tile_n(Cout);
    if (TN == 128) {
        if (stride_h == 2) return launch_conv<128, 2, false>(a, st);
        return pool ? launch_conv<128, 1, true>(a, st) : launch_conv<128, 1, false>(a, st);
    }
    if (stride_h == 2) return launch_conv<64, 2, false>(a, st);
    return pool ? launch_conv<64, 1, true>(a, st) : launch_conv<64, 1, false>(a, st);
}

}  // namespace

extern "C" {

int witw_conv3x3_fwd_ex(const float* x, const float* wpk, const float* bias, const float* dropmask, const float* gate,
                        const float* post_scale, const float* post_shift, float* y, unsigned char* pool_code, int B, int H,
                        int W, int Cin, int Cout, int stride_h, int pad_circular, int relu, float lrelu_slope, int pool,
                        int out_nchw, int dilate_h, void* stream) {
    return conv3x3_fwd_any(x, wpk, nullptr, bias, dropmask, gate, post_scale, post_shift, y, pool_code, B, H, W, Cin, Cout,
                           stride_h, pad_circular, relu, lrelu_slope, pool, out_nchw, dilate_h, stream);
}

// witw_conv3x3_fwd_ex with both packings of the filter: the launch runs the Winograd F(2,3)-along-H form (wpk_wino) where its class
// and arguments allow it and witw_conv3x3_wino() is on, the direct form (wpk) otherwise; witw_last_conv_form() says which.
int witw_conv3x3_fwd_wino(const float* x, const float* wpk, const float* wpk_wino, const float* bias, const float* dropmask,
                          const float* gate, const float* post_scale, const float* post_shift, float* y, unsigned char* pool_code,
                          int B, int H, int W, int Cin, int Cout, int stride_h, int pad_circular, int relu, float lrelu_slope,
                          int pool, int out_nchw, int dilate_h, void* stream) {
    WITW_CHECK_ARG(wpk_wino, "conv3x3_fwd_wino: null Winograd filter");
    return conv3x3_fwd_any(x, wpk, wpk_wino, bias, dropmask, gate, post_scale, post_shift, y, pool_code, B, H, W, Cin, Cout,
                           stride_h, pad_circular, relu, lrelu_slope, pool, out_nchw, dilate_h, stream);
}

// 1 (default): launches given a Winograd-packed filter run the Winograd form where they can; 0: the direct form. enable < 0 only
// queries. Returns the previous setting.
int witw_conv3x3_wino(int enable) {
    const int prev = wino_on();
    if (enable >= 0) g_wino = enable != 0;
    return prev;
}

// 1 (default): a Winograd launch runs one workgroup per CU over runs of tiles; 0: one workgroup per tile (same bits). enable < 0
// only queries. Returns the previous setting.
int witw_conv3x3_wino_run(int enable) {
    const int prev = wino_run();
    if (enable >= 0) g_wino_run = enable != 0;
    return prev;
}

// 1 (default): a Winograd launch stages its K chunks by LDS-DMA; 0: through registers (same bits). enable < 0 only queries.
// Returns the previous setting.
int witw_conv3x3_wino_dma(int enable) {
    const int prev = wino_dma();
    if (enable >= 0) g_wino_dma = enable != 0;
    return prev;
}

long long witw_conv3x3_packed_floats_wino(int cout, int cin) {
    if (cout <= 0 || cin <= 0) return -1;
    return (long long)cdiv(cout, 64) * cdiv(cin, 8) * 12 * 2 * 64 * 4;
}

int witw_conv3x3_pack_weights_wino(const float* w_kcrs, float* wpk_wino, int cout, int cin, void* stream) {
    WITW_CHECK_ARG(w_kcrs && wpk_wino, "pack_weights_wino: null pointer");
    WITW_CHECK_ARG(cout > 0 && cin > 0, "pack_weights_wino: bad shape cout=%d cin=%d", cout, cin);
    const int n_tiles = cdiv(cout, 64), nkc = cdiv(cin, 8);
    const size_t total = (size_t)n_tiles * nkc * 12 * 2 * 64;
    hipLaunchKernelGGL(pack_weights_wino_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       w_kcrs, wpk_wino, cout, cin, nkc, total);
    WITW_CHECK_LAUNCH("pack_weights_wino");
    return WITW_OK;
}

// 1 (default): a zero-interleaved launch (dilate_h) on the 8-wave 128-channel tile does not issue the MFMAs whose input rows are
// the interleaved zeros (half of them; same bits); 0: it issues them all. enable < 0 only queries. Returns the previous setting.
int witw_conv3x3_dil_skip(int enable) {
    const int prev = dil_skip();
    if (enable >= 0) g_dil_skip = enable != 0;
    return prev;
}

int witw_conv3x3_fwd(const float* x, const float* wpk, const float* bias, const float* dropmask, float* y, int B, int H,
                     int W, int Cin, int Cout, int stride_h, int pad_circular, int relu, int pool, int out_nchw,
                     void* stream) {
    return witw_conv3x3_fwd_ex(x, wpk, bias, dropmask, nullptr, nullptr, nullptr, y, nullptr, B, H, W, Cin, Cout, stride_h,
                               pad_circular, relu ? 1 : 0, 0.f, pool, out_nchw, 0, stream);
}

}  // extern "C"
