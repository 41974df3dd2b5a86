/* libwitw_hip.so — C ABI of the MI355X (gfx950) hot path of IQTLabs/WITW.
 *
 * The reference exposes no FFI: its boundary is the Python surface of model/cvig_fov.py
 * (SURVEY.md §8b). Each entry point below replaces the stock-PyTorch op(s) behind one of those
 * Python functions; witw_amd/_lib.py binds them with ctypes and witw_amd/cvig_fov.py keeps the
 * reference's names on top (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller unless a
 *    comment says HOST; the library never allocates or frees;
 *  - fp32 everywhere (indices: int64 orientation, int32 ranks); tensors are contiguous;
 *  - every launcher is asynchronous on `stream` (a hipStream_t passed as void*, NULL = default
 *    stream), never synchronises, is re-entrant across streams;
 *  - return 0 on success, <0 on error (-1 invalid argument, -2 launch failure, -3 no gfx950
 *    device); the message is thread-local text from witw_last_error();
 *  - one process per GPU; the code object is gfx950 only.
 */
#ifndef WITW_HIP_H
#define WITW_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

const char* witw_last_error(void);
int witw_version(void);               /* major*10000 + minor*100 + patch */
int witw_device_check(int device);    /* 0 iff `device` is a gfx950 part */
/* name of the conv kernel instantiation the calling thread's last conv launcher picked, spelled as in rocprof kernel names
 * (e.g. "conv3x3_bf16_s16_kernel<false>"); "" before the first launch. Parity tests assert on it so that a change of the
 * launcher's thresholds cannot silently move a test onto another kernel. */
const char* witw_last_kernel_variant(void);
/* arithmetic form of the calling thread's last conv launch: "direct", or "wino_h2" when witw_conv3x3_fwd_wino ran the Winograd
 * F(2,3)-along-H form of conv3x3_nhwc_f32_kernel (same instantiation name); "" before the first launch. */
const char* witw_last_conv_form(void);

/* ---- FOV_DSM encoder: Conv2d(3x3,pad 1) [+HorizCircPadding] [+Dropout2d] [+ReLU] [+MaxPool2d(2)]
 *      reference: model/cvig_fov.py:212-231 (padding), :234-245 (dropout), :256-294 (layer stack).
 * Activations are NHWC with the channel count padded to a multiple of 8. */

/* output-channel tile the kernel will use for `cout` (64 or 128) */
int witw_conv3x3_tile_n(int cout);
/* waves per workgroup (4 or 8) chosen for a layer shape; with tile_n, stride and pool it names the kernel
 * instantiation conv3x3_nhwc_f32_kernel<tile_n,stride_h,pool,waves> seen in profiles */
int witw_conv3x3_workgroup_waves(int B, int H, int W, int Cout, int stride_h);
/* number of floats of the packed filter / of the zero-padded bias for a (cout, cin) layer */
long long witw_conv3x3_packed_floats(int cout, int cin);
int witw_conv3x3_bias_floats(int cout);
/* w_kcrs: torch layout [cout][cin][3][3]. transpose_flip=1 packs the data-gradient filter instead
 * (source layout [cin][cout][3][3], taps rotated 180 degrees). */
int witw_conv3x3_pack_weights(const float* w_kcrs, float* wpk, int cout, int cin, int transpose_flip, void* stream);
/* NCHW [B,C,H,W] (C<=8) -> NHWC8 [B,H,W,8], zero-filled channels; replaces the implicit layout of
 * the first Conv2d call (model/cvig_fov.py:293). */
int witw_nchw_to_nhwc8(const float* x, float* y, int B, int C, int H, int W, void* stream);
/* x [B,H,W,Cin] (Cin%8==0) -> y NHWC [B,Hy,Wy,Cout] (or NCHW [B,Cout,Hy,Wy] if out_nchw).
 * stride_h in {1,2} (stride_w = 1); pad_circular: wrap columns (HorizCircPadding) else zero pad;
 * dropmask: NULL or [B,Cout] Dropout2d scales applied before the ReLU; pool: fused MaxPool2d(2,2).
 * bias: witw_conv3x3_bias_floats(Cout) floats. */
int witw_conv3x3_fwd(const float* x, const float* wpk, const float* bias, const float* dropmask, float* y, int B, int H,
                     int W, int Cin, int Cout, int stride_h, int pad_circular, int relu, int pool, int out_nchw,
                     void* stream);

/* First layer fast path: Conv2d(C<=4 -> 64, 3x3, pad 1)+ReLU straight from the NCHW fp32 image (features[0..1],
 * model/cvig_fov.py:256-260): wf = witw_conv3x3_first_pack(w [64][C][3][3]) (a 2560-float buffer; round_bf16 = 1
 * writes the bf16 MFMA kernel's filter image instead and goes with out_bf16 = 1), y = NHWC [B,H,W,64] fp32, or bf16
 * with bf16-rounded operands on v_mfma_f32_32x32x16_bf16 when out_bf16 = 1 (this form takes C <= 8: cvig_semantic's 5-channel
 * first conv, model/cvig_semantic.py:301-303, at inference); out_bf16 = 2: fp32 arithmetic, split-fp16 output
 * [B,H,W,8,2,8] (hi / lo planes per 8 channels) for the fp16x3 path. */
int witw_conv3x3_first_pack(const float* w, float* wf, int C, int round_bf16, void* stream);
/* Layers 0 and 2 of the encoder fused, bf16 inference: x NCHW fp32 [B,C<=8,H,W] -> y NHWC bf16 [B,H/2,W/2,64] =
 * MaxPool2d(2)(ReLU(conv 64->64 (ReLU(conv C->64 (x))))) (features[0..4], model/cvig_fov.py:256-260), the 64-channel map between
 * the two convs never leaving the chip. wf0 / bias0: witw_conv3x3_first_pack(round_bf16 = 1) image and bias; wpk2 / bias2:
 * witw_conv3x3_bf16_pack_weights image (64 -> 64) and bias. Bit-identical to witw_conv3x3_first_fwd(out_bf16 = 1) followed by
 * witw_conv3x3_bf16_fwd(relu, pool). */
int witw_conv_first2_bf16_fwd(const float* x, const void* wf0, const float* bias0, const void* wpk2, const float* bias2, void* y,
                              int B, int C, int H, int W, int pad_circular, void* stream);
/* The training form (cvig_semantic trains layer 0, model/cvig_semantic.py:301-309, so the backward crosses both layers): the same
 * y, plus pool_code [B,H/2,W/2,64] (arg-max of each 2x2 window, dy*2+dx: the input of witw_maxpool2x2_bwd_bf16) and gate_bits
 * [B,H,W,8] bytes (bit c & 7 of byte c >> 3 = layer 0's output channel c at that pixel is > 0) instead of the two 64-channel
 * activations. Layer 2's own ReLU gate is y > 0. H and W even. */
int witw_conv_first2_bf16_fwd_train(const float* x, const void* wf0, const float* bias0, const void* wpk2, const float* bias2, void* y,
                                    unsigned char* pool_code, unsigned char* gate_bits, int B, int C, int H, int W, int pad_circular,
                                    void* stream);
/* Data gradient of a 64-input-channel stride-1 layer whose upstream ReLU gate is given as ONE BIT per output (gate_bits
 * [B,H,W,Cout/8] bytes as above) instead of a bf16 tensor: same bits as witw_conv3x3_bf16_fwd_ex(gate = the activation). Runs on the
 * weight-resident kernel only: witw_conv3x3_bf16_gatebits_ok tells whether a shape qualifies (1) or the tensor gate has to be kept (0). */
int witw_conv3x3_bf16_gatebits_ok(int B, int H, int W, int Cin, int Cout);
int witw_conv3x3_bf16_fwd_gatebits(const void* x_bf16, const void* wpk_bf16, const float* bias, const void* gate_bits, void* y, int B, int H,
                                   int W, int Cin, int Cout, int pad_circular, int relu, void* stream);
/* The first layer itself (described above witw_conv3x3_first_pack). Finite images only: the kernels multiply filter slots that hold
 * zero (a tap that does not exist, a channel >= C, a zero weight) with the pixel they meet, so a non-finite pixel makes the outputs
 * whose 3x3 window contains it unspecified among NaN and +-inf -- 0 * inf = NaN where the convolution in the reals gives +-inf -- and,
 * with relu, +0.0 (the ReLU of a NaN or of -inf). Every other output is unaffected. On finite data each form is tested bit for bit
 * against float64: tests/test_first_layer_gpu.py. */
int witw_conv3x3_first_fwd(const float* x, const float* wf, const float* bias, void* y, int B, int C, int H, int W,
                           int pad_circular, int relu, int out_bf16, void* stream);

/* Extended form used by the backward pass: `gate` (NULL or a tensor shaped like y) zeroes outputs where
 * gate <= 0 (ReLU backward), dilate_h=1 reads the input as zero-interleaved rows (row 2i = physical row i,
 * H is the dilated height) — the data gradient of a stride-(2,1) conv is then this same kernel on the
 * transpose_flip filter (autograd of torch.nn.Conv2d at model/cvig_fov.py:460). relu: 0 none, 1 ReLU,
 * 2 LeakyReLU(lrelu_slope); post_scale/post_shift (NULL or [Cout]): per-channel affine after the activation
 * (eval-mode BatchNorm2d of model/cvig_baseline.py:267-275).
 *
 * Epilogue contract of the unpooled launch, shared by witw_conv3x3_bf16_fwd_ex and witw_conv3x3_f16x3_fwd_ex (which have no
 * LeakyReLU / affine), as tested bit for bit by tests/test_conv_epilogue_gpu.py against tests/conv_epilogue_ref.py:
 *   - order: conv + bias -> Dropout2d scale (dropmask[b][c]) -> activation -> post affine -> gate;
 *   - the gate is a SELECT, open exactly where gate > 0 (for a split-fp16 gate: where its hi half is): +0.0, -0.0, negative values
 *     and NaN close it, the smallest positive subnormal and +inf open it;
 *   - a closed output is +0.0 (all bits zero), also where the value was negative, scaled by 0, infinite or NaN; an open output is
 *     the value, unchanged;
 *   - the gate is indexed like y: NCHW under out_nchw, NHWC otherwise. */
int witw_conv3x3_fwd_ex(const float* x, const float* wpk, const float* bias, const float* dropmask, const float* gate,
                        const float* post_scale, const float* post_shift, float* y, unsigned char* pool_code, int B, int H,
                        int W, int Cin, int Cout, int stride_h, int pad_circular, int relu, float lrelu_slope, int pool,
                        int out_nchw, int dilate_h, void* stream);
/* 1 (default): a zero-interleaved launch of witw_conv3x3_fwd_ex (dilate_h: the data gradient of a stride-(2,1) conv, model/cvig_fov.py:
 * 263-272 through autograd) on the 8-wave 128-channel tile skips the products whose input rows are the interleaved zeros -- half the
 * MFMAs, the same bits; 0: all products are issued. enable < 0 only queries; returns the previous setting. */
int witw_conv3x3_dil_skip(int enable);
/* Winograd F(2,3) along H (inference): the filter packed for it, [cdiv(cout,64)][cdiv(cin,8)][kw 3][t 4][quad 2][64][4] with
 * U0 = g0, U1 = ((g0+g1)+g2)/2, U2 = ((g0-g1)+g2)/2, U3 = g2 per column tap (g = the 3 taps of the column); its size in floats. */
long long witw_conv3x3_packed_floats_wino(int cout, int cin);
int witw_conv3x3_pack_weights_wino(const float* w_kcrs, float* wpk_wino, int cout, int cin, void* stream);
/* witw_conv3x3_fwd_ex with both packings of the filter: stride-1 launches with no gate / dilate_h / NCHW output / post affine,
 * Cout % 4 == 0 and the wide geometry, of the classes conv3x3_nhwc_f32_kernel<128,1,*,*,0,9> and <64,1,true,*,0,9>, run the
 * Winograd form (2/3 of the MFMAs; same instantiation name, witw_last_conv_form() == "wino_h2") while witw_conv3x3_wino is on;
 * every other launch runs the direct form on wpk. */
int witw_conv3x3_fwd_wino(const float* x, const float* wpk, const float* wpk_wino, const float* bias, const float* dropmask,
                          const float* gate, const float* post_scale, const float* post_shift, float* y, unsigned char* pool_code,
                          int B, int H, int W, int Cin, int Cout, int stride_h, int pad_circular, int relu, float lrelu_slope,
                          int pool, int out_nchw, int dilate_h, void* stream);
/* 1 (default, or WITW_CONV_WINO in the environment): witw_conv3x3_fwd_wino takes the Winograd form where it can; 0: always the
 * direct form (A/B runs). enable < 0 only queries; returns the previous setting. */
int witw_conv3x3_wino(int enable);
/* 1 (default, or WITW_CONV_WINO_RUN in the environment): a Winograd launch starts at most one workgroup per CU, and each walks a
 * run of tiles (every CU-count-th index of the workgroup -> tile map) with one continuous K loop; 0: one workgroup per tile. Same
 * bits either way (A/B runs). WITW_CONV_WINO_WGS=n in the environment forces the workgroup count (test aid). enable < 0 only
 * queries; returns the previous setting. */
int witw_conv3x3_wino_run(int enable);
/* 1 (default, or WITW_CONV_WINO_DMA in the environment): a Winograd launch stages the input tile and filter slab of a K chunk by
 * LDS-DMA (buffer loads that write the LDS directly); 0: through registers. Same bits either way (A/B runs). enable < 0 only
 * queries; returns the previous setting. */
int witw_conv3x3_wino_dma(int enable);
/* backward of the fused MaxPool2d(2,2): pool_code (written by the forward when non-NULL: first arg-max position
 * dy*2+dx in torch's scan order) routes dy [B,Hp,Wp,C] into dx [B,H,W,C] (H>=2Hp, W>=2Wp). */
int witw_maxpool2x2_bwd(const float* dy, const unsigned char* pool_code, float* dx, int B, int Hp, int Wp, int H, int W,
                        int C, void* stream);
/* NCHW [B,C,H,W] -> NHWC [B,H,W,Cpad] with zero-filled extra channels (embedding gradients). */
int witw_nchw_to_nhwc(const float* x, float* y, int B, int C, int H, int W, int Cpad, void* stream);
/* Weight / bias gradient of one conv layer. x: the layer's NHWC input [B,H,W,Cin], dz: gradient at its output
 * [B,Ho,W,Cout] NHWC (ReLU / dropout gates already applied). dw: torch layout [Cout][cin_real][3][3];
 * db: [Cout] or NULL; accumulate != 0 adds into dw/db. workspace: witw_conv3x3_wgrad_workspace_floats().
 *
 * Contract of every weight-gradient entry (witw_conv3x3_wgrad, _wgrad_taps4, _wgrad_bf16, _wgrad_bf16_nhwc, _wgrad_bf16_taps4, _wgrad_f16x3), as
 * tested by tests/test_wgrad_edges_gpu.py:
 *   accumulate: with accumulate != 0 each element of dw [Cout][cin_real][3][3] and of db (when not NULL) becomes
 *     old value + (the value accumulate == 0 would have stored): ONE fp32 add per element, bit for bit, no other arithmetic on
 *     the old value. Under _wgrad_taps4 the five taps outside {1,2}^2 are not touched at all (accumulate == 0 sets them to +0).
 *     Nothing outside dw's cin_real channels and db's Cout elements is written in either mode.
 *   workspace: its contents on entry are irrelevant (NaN included): every partial the reduction reads has been stored by the
 *     same call, also for K splits whose chunk range is empty. It needs the size of the matching *_workspace_floats() at the
 *     same arguments (and, for _wgrad_bf16_nhwc, the same witw_conv3x3_wgrad_bf16_mfma16 setting) and is scratch afterwards.
 *   refusals: a call that returns an error (Cin / Cout not a multiple of 4 -- 8 for the bf16 and fp16x3 entries --, cin_real
 *     outside (0, Cin], stride_h not 1 or 2, the f16x3 bias gradient at a Cout whose eighth does not divide 256) has launched
 *     nothing and written nothing. */
int witw_conv3x3_wgrad_splits(int B, int Ho, int Wo, int Cin, int Cout);
long long witw_conv3x3_wgrad_workspace_floats(int B, int H, int W, int Cin, int Cout, int stride_h);
int witw_conv3x3_wgrad(const float* x, const float* dz, float* dw, float* db, float* workspace, int B, int H, int W, int Cin,
                       int cin_real, int Cout, int stride_h, int pad_circular, int accumulate, void* stream);
/* torch.optim.Adam step (no weight decay / amsgrad), optimizer of model/cvig_fov.py:416-418. step counts from 1. */
int witw_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr, float beta1,
                   float beta2, float eps, int step, void* stream);
/* The same step for `count` parameter tensors in ceil(count / 48) launches: HOST arrays of device pointers, element counts and
 * 1-based step numbers (the loop over optimizer.param_groups of torch.optim.Adam.step, model/cvig_fov.py:463). */
int witw_adam_step_multi(float* const* param, const float* const* grad, float* const* exp_avg, float* const* exp_avg_sq,
                         const long long* n, const int* step, int count, float lr, float beta1, float beta2, float eps, void* stream);

/* ---- matching: correlation (:297-315) + crop_overhead (:318-343) + l2_distance (:346-363) fused.
 * ov [Bo,16,4,64], su [Bs,16,4,We] (NCHW embeddings). Outputs [Bo,Bs]; any of them may be NULL.
 * workspace: witw_match_workspace_floats(Bo,Bs) floats (window norms + surface norms). */
long long witw_match_workspace_floats(int Bo, int Bs);
int witw_match_fwd(const float* ov, const float* su, int Bo, int Bs, int We, long long* orientation, float* distance,
                   float* score, float* workspace, void* stream);
/* witw_match_fwd with an orientation prior: shift_mask [Bs] (device, may be NULL = witw_match_fwd) holds one 64-bit word per surface
 * embedding, bit k set = shift k may be chosen. orientation[o][s] = the FIRST maximum of the correlation over the allowed shifts of
 * s; distance and score are taken at that shift, as in witw_match_fwd. A word of 0 means "no prior" and behaves like all 64 bits
 * set, so no shift outside [0,64) can reach the window norms or the backward; an all-ones mask gives the bits of witw_match_fwd.
 * The mask never changes which kernel runs for a shape. witw_match_bwd takes orientation as a constant of the graph and is the
 * backward of this entry as it is. */
int witw_match_fwd_masked(const float* ov, const float* su, int Bo, int Bs, int We, long long* orientation, float* distance,
                          float* score, float* workspace, const unsigned long long* shift_mask, void* stream);
/* The match at a KNOWN orientation (an aligned protocol, a trusted heading): shift [Bs] (device int64) gives every surface embedding
 * its one shift, used as shift[s] & 63, and score[o][s] = sum_{ch,k<We} ov[o][ch][(k+shift[s])%64] * su[s][ch][k] is one
 * Bo x Bs x 64*We contraction -- 1/64 of the products of witw_match_fwd_masked under one-bit words. orientation[o][s] = shift[s] & 63;
 * distance and score are taken there and are BIT-IDENTICAL to witw_match_fwd_masked with shift_mask[s] = 1 << (shift[s] & 63) (the
 * same fp32 MFMA chain per pair, row outer, k inner). Any output may be NULL. workspace: witw_match_fixed_workspace_floats(Bo,Bs)
 * floats; it begins with the window norms [Bo,64] and surface norms [Bs] of a witw_match_fwd workspace, so witw_match_bwd,
 * witw_match_bwd_pairs and witw_match_pairs* take it as they take that one; the grouping of the surfaces by shift follows. Only
 * those first Bo * 64 + Bs floats are defined on return: the grouping table is sized for the worst case and written as far as the
 * shifts of this batch need, the entries behind that are left as they were. */
long long witw_match_fixed_workspace_floats(int Bo, int Bs);
int witw_match_fwd_fixed(const float* ov, const float* su, int Bo, int Bs, int We, const long long* shift /* [Bs], device */,
                         long long* orientation, float* distance, float* score, float* workspace, void* stream);
/* The same match through the row spectra (retrieval, BASELINE config 5: every gallery row against every query). The orientation
 * search is a circular cross-correlation along the 64 columns: with the 64-point DFT of every (channel,row) line of both sides it
 * costs 21k FLOP per pair instead of 524k. witw_match_spectrum: emb [B,64 lines,W] (overhead: W = 64; surface: W = We, zero-
 * padded) -> spec [B,32,128] (witw_match_spectrum_floats(B) floats; fp64 transform rounded once to fp32; the order of the two
 * 8-byte chunks inside each 16-byte slot depends on the side -- `role` -- and, for overheads, on bit 4 of the embedding's index, so
 * that the match kernel's LDS operand reads are free of bank conflicts: a spectrum is only meaningful to witw_match_fwd_dft, on the
 * side and at the row numbering (mod 32) it was computed for). witw_match_fwd_dft:
 * outputs as witw_match_fwd (first maximum wins); scores agree with the direct sum to fp32 rounding (1e-6 of |ov||su|), so
 * orientations can differ from witw_match_fwd only between shifts whose scores tie to that accuracy.
 * workspace: witw_match_dft_workspace_floats(Bo,Bs) floats. */
long long witw_match_spectrum_floats(long long n_embeddings);
int witw_match_spectrum(const float* emb, float* spec, int B, int W, int role /* 0 surface (query) side, 1 overhead (gallery) side */,
                        void* stream);
long long witw_match_dft_workspace_floats(int Bo, int Bs);
int witw_match_fwd_dft(const float* ov, const float* su, const float* spec_ov, const float* spec_su, int Bo, int Bs, int We,
                       long long* orientation, float* distance, float* score, float* workspace, void* stream);
/* the same, also writing gap [Bo,Bs] = best score - runner-up score over the 64 shifts (distance of the arg-max from a tie) */
int witw_match_fwd_dft_gap(const float* ov, const float* su, const float* spec_ov, const float* spec_su, int Bo, int Bs, int We,
                           long long* orientation, float* distance, float* score, float* gap, float* workspace, void* stream);
/* witw_match_fwd_dft / _gap under the orientation prior of witw_match_fwd_masked (model/cvig_fov.py:297-315 restricted per query;
 * retrieval loop :547-552): shift_mask [Bs] (device, NOT NULL here) holds one 64-bit word per surface embedding, bit k set = shift k
 * may be chosen, 0 = no prior = all 64 bits. orientation = the first maximum over the allowed shifts, distance / score at that
 * shift. gap may be NULL; otherwise gap = best score - second best ALLOWED score, +inf where the word allows a single shift. */
int witw_match_fwd_dft_masked(const float* ov, const float* su, const float* spec_ov, const float* spec_su, int Bo, int Bs, int We,
                              long long* orientation, float* distance, float* score, float* gap /* may be NULL */, float* workspace,
                              const unsigned long long* shift_mask, void* stream);
/* backward of witw_match_fwd (orientation is a constant of the graph): grad_distance [Bo,Bs] ->
 * grad_ov [Bo,16,4,64] and/or grad_su [Bs,16,4,We]; orientation/score/workspace as left by the forward. scratch: NULL,
 * or witw_match_bwd_scratch_floats(Bo,Bs,We) floats that let the surface gradient split the overheads over several
 * workgroups per surface (fixed-order sum; a batch of 128 surfaces alone leaves half the chip idle). */
long long witw_match_bwd_scratch_floats(int Bo, int Bs, int We);
int witw_match_bwd(const float* ov, const float* su, const long long* orientation, const float* score, const float* workspace,
                   const float* grad_distance, float* grad_ov, float* grad_su, float* scratch, int Bo, int Bs, int We,
                   void* stream);
/* compatibility entries with the reference's materialising semantics */
int witw_crop_overhead(const float* ov, const long long* orientation, float* out /*[Bo,Bs,16,4,We]*/, int Bo, int Bs,
                       int We, void* stream);
int witw_l2_distance(const float* cropped /*[Bo,Bs,n]*/, const float* su /*[Bs,n]*/, float* distance, int Bo, int Bs, int n,
                     void* stream);
/* ranks[q] = #{o : D[o][q] <= D[q+true_offset][q]} — the loop body of test(), model/cvig_fov.py:550-552 */
int witw_rank_count(const float* distance /*[Bo,Bs]*/, int* ranks /*[Bs]*/, int Bo, int Bs, int true_offset, void* stream);

/* k smallest distances of every query column of D[Bo][Bs], ordered by (distance, gallery index): values [Bs][k],
 * indices [Bs][k] (+row_offset: global row number of this shard's first row; -1 pads when Bo < k). 1 <= k <= 32. */
int witw_topk_smallest(const float* distance, float* values, long long* indices, int Bo, int Bs, int k, long long row_offset,
                       void* stream);
/* the same with the gallery rows split over workgroups (one workgroup column per 64 queries cannot fill the chip when the
 * gallery is long): workspace = witw_topk_workspace_bytes(Bo,Bs,k) bytes (NULL or 0 bytes: single pass). Same result. */
long long witw_topk_workspace_bytes(int Bo, int Bs, int k);
int witw_topk_smallest_ws(const float* distance, float* values, long long* indices, int Bo, int Bs, int k, long long row_offset,
                          void* workspace, void* stream);
/* the next k places of such a list: the k smallest among the rows that lie strictly behind (after_value[q], after_index[q]) in
 * the same order -- the bound is an entry of the list so far, usually its last: f32 [Bs] and int64 [Bs], the index a global row
 * number as row_offset produces them. A NaN after_value counts as +inf, as a NaN distance does; after_index -1 (the pad) has
 * nothing behind it: k pads. A list of any length is witw_topk_smallest_ws followed by calls of this entry, each bounded by the
 * last place of the one before. Workspace as for witw_topk_smallest_ws (witw_topk_workspace_bytes). 1 <= k <= 32. */
int witw_topk_smallest_after(const float* distance, float* values, long long* indices, int Bo, int Bs, int k, long long row_offset,
                             const float* after_value, const long long* after_index, void* workspace, void* stream);
/* sharded-gallery form: ranks[q] = #{o in this shard : D[o][q] <= threshold[q]} (threshold = true match's distance) */
int witw_rank_count_thresh(const float* distance, const float* threshold, int* ranks, int Bo, int Bs, void* stream);

/* Index-exact retrieval on top of the spectral pass (model/cvig_fov.py:547-552 ranks / top-k must not depend on which of two
 * equally accurate fp32 summation orders produced a distance). witw_match_pairs: a LIST of n_pairs (overhead row pair_o[i],
 * surface row pair_s[i]) pairs -> orientation / distance / score [n_pairs] (any may be NULL), bit-identical to the entries
 * witw_match_fwd writes for those pairs (same MFMA accumulation chain, one wave per pair); wn [Bo,64] / sn [Bs] = the norms
 * at the start of a witw_match_fwd / witw_match_fwd_dft workspace over the same ov / su (window norms, then surface norms).
 * witw_rank_count_band: D [Bo,Bs] known to +-eps: counts[q] = #{o : D[o][q] < threshold[q] - eps}; the (o,q) inside the band
 * |D - threshold| <= eps are appended to pair_o / pair_s (up to `capacity`), *n_pairs = how many there were in all. */
int witw_match_pairs(const float* ov, const float* su, const float* wn, const float* sn, const int* pair_o, const int* pair_s,
                     int n_pairs, int Bo, int Bs, int We, long long* orientation, float* distance, float* score, void* stream);
int witw_rank_count_band(const float* distance, const float* threshold, float eps, int* counts, int* pair_o, int* pair_s,
                         int* n_pairs, int capacity, int Bo, int Bs, void* stream);
/* witw_rank_count_band's list resolved without reading its length back to the host (model/cvig_fov.py:547-552: the rank is a
 * count of distances <= the true match's): re-scores the first min(*n_pairs_dev, capacity) pairs as witw_match_pairs does and
 * adds 1 to counts[pair_s[i]] for every pair with exact distance <= threshold[pair_s[i]]. */
int witw_match_pairs_count(const float* ov, const float* su, const float* wn, const float* sn, const int* pair_o, const int* pair_s,
                           const int* n_pairs_dev, int capacity, int Bo, int Bs, int We, const float* threshold, int* counts, void* stream);
/* witw_match_pairs / witw_match_pairs_count under shift masks (model/cvig_fov.py:547-552 with the orientation prior): shift_mask
 * [Bs] (device, NOT NULL here) is indexed by pair_s[i]; orientation / distance / score are bit-identical to the entries
 * witw_match_fwd_masked writes for those pairs. */
int witw_match_pairs_masked(const float* ov, const float* su, const float* wn, const float* sn, const int* pair_o, const int* pair_s,
                            int n_pairs, int Bo, int Bs, int We, long long* orientation, float* distance, float* score,
                            const unsigned long long* shift_mask, void* stream);
int witw_match_pairs_count_masked(const float* ov, const float* su, const float* wn, const float* sn, const int* pair_o,
                                  const int* pair_s, const int* n_pairs_dev, int capacity, int Bo, int Bs, int We,
                                  const float* threshold, int* counts, const unsigned long long* shift_mask, void* stream);
/* which kernel witw_match_pairs runs: 1 = v_fma_f32 chain on the vector pipe, one lane per shift (default, round 6); 0 = the
 * v_mfma_f32_32x32x2_f32 chain of rounds 4-5. Same bits (the f32 MFMA accumulates as a fused-multiply-add chain in k order).
 * impl < 0 only queries; returns the previous setting. */
int witw_match_pairs_impl(int impl);

/* ---- Orientation profiles: the match at EVERY shift, and ranked orientation hypotheses drawn from it.
 * witw_match_profile: score_all / distance_all [Bo,Bs,64] (either may be NULL, not both). score_all[o][s][k] is the correlation
 * of pair (o,s) at shift k; distance_all[o][s][k] = 2*(1 - score/(wn[o][k]*sn[s])), witw_match_fwd's epilogue expression. Per
 * pair the 64 scores carry THE BITS of the accumulation chain every forward form runs (row outer, k inner, k padded to even
 * with a zero multiplier): the first arg-max of score_all[o][s][:] is witw_match_fwd's orientation, and score_all / distance_all
 * at that shift are its score / distance bit for bit, whatever kernel form witw_match_fwd picks for the shape. workspace:
 * witw_match_workspace_floats(Bo,Bs) floats, filled as witw_match_fwd fills it (window norms, then surface norms);
 * witw_match_pairs* and witw_match_pairs_profile take it unchanged.
 * witw_match_pairs_profile: the same for a LIST of pairs (as witw_match_pairs: pair_o / pair_s int32 on the device, wn / sn
 * the norm blocks of a match workspace over the same ov / su); outputs [n_pairs,64], rows bit-identical to the rows
 * witw_match_profile writes for those pairs. The route at retrieval scale: the profiles of a query's k candidates.
 * witw_profile_hypotheses: score_all [n_pairs,64] -> shifts [n_pairs,n_hyp] (int64). Hypothesis 1 is the first maximum over the
 * allowed shifts -- witw_match_fwd_masked's rule, ties and NaNs included, so it is that entry's orientation. Hypothesis j+1
 * is the first maximum over the allowed shifts whose circular distance (on the ring of 64) to every earlier hypothesis is
 * > min_sep; once no shift is left the remaining entries are -1. Pair p reads the word shift_mask[p % n_words]: a dense
 * [Bo,Bs] profile passes the [Bs] words of witw_match_fwd_masked and n_words = Bs, a pair list passes gathered words and
 * n_words = n_pairs, one shared word n_words = 1; NULL, or a word of 0, allows all 64 shifts. 1 <= n_hyp <= 64,
 * 0 <= min_sep <= 31. Ranking is by the raw score, the quantity the reference's correlation maximises. */
int witw_match_profile(const float* ov, const float* su, int Bo, int Bs, int We, float* score_all, float* distance_all,
                       float* workspace, void* stream);
int witw_match_pairs_profile(const float* ov, const float* su, const float* wn, const float* sn, const int* pair_o,
                             const int* pair_s, int n_pairs, int Bo, int Bs, int We, float* score_all, float* distance_all,
                             void* stream);
int witw_profile_hypotheses(const float* score_all, int n_pairs, const unsigned long long* shift_mask, int n_words, int n_hyp,
                            int min_sep, long long* shifts, void* stream);

/* ---- Dropout2d masks (AddDropout, model/cvig_fov.py:234-245): out [n_layers][B][C] = 0 or 1/(1-p) per (sample, channel) from
 * Philox4x32-10 keyed on `seed`, counter (sample*C + channel, layers[i] | encoder << 16, step, rank) -- reproducible from those
 * numbers alone (the reference uses torch's global RNG stream). layers: HOST array of n_layers (<= 3) layer indices. */
int witw_dropout2d_scales(float* out, unsigned long long seed, unsigned encoder, unsigned step, unsigned rank, const int* layers,
                          int n_layers, int B, int C, float p, void* stream);

/* ---- triplet_loss, model/cvig_fov.py:366-382. workspace: 4*B floats, filled by fwd, read by bwd. */
int witw_triplet_loss_fwd(const float* distance /*[B,B]*/, int B, float alpha, float* loss /*[1]*/, float* workspace,
                          void* stream);
/* sharded global batch: un-normalised partial over the column slab D[Bo][Bs] (surfaces col0..col0+Bs of the global
 * batch), diag[Bo] = global diagonal; sum over ranks / (2*Bo*(Bo-1)) = the loss. workspace: Bo floats. */
int witw_triplet_loss_slab_fwd(const float* distance, const float* diag, int Bo, int Bs, int col0, float alpha, float* partial,
                               float* workspace, void* stream);
/* Backward of the sharded global-batch loss (the gradient of model/cvig_fov.py:366-382 restricted to one rank's column slab):
 * step 1 -> rowsig[Bo] = sum over THIS rank's surfaces of sigmoid(alpha*(d_ii - d_ij)) (the caller all-reduces it) and
 * colsig[Bs] = sum over all overheads of sigmoid(alpha*(d_cc - d_ij)), c = col0 + j (complete);
 * step 2 -> grad_distance[Bo,Bs] for the device scalar grad_loss of the global loss (normaliser 2*Bo*(Bo-1)). */
int witw_triplet_loss_slab_sig(const float* distance, const float* diag, int Bo, int Bs, int col0, float alpha, float* rowsig,
                               float* colsig, void* stream);
int witw_triplet_loss_slab_bwd(const float* distance, const float* diag, const float* rowsig, const float* colsig,
                               const float* grad_loss, float* grad_distance, int Bo, int Bs, int col0, float alpha, void* stream);
int witw_triplet_loss_bwd(const float* distance, const float* workspace, const float* grad_loss /*[1]*/,
                          float* grad_distance /*[B,B]*/, int B, float alpha, void* stream);

/* ---- batch-hard soft-margin triplet loss (Hermans et al. 2017; opt-in, not in the reference). With Dm = D whose diagonal is
 * +inf: rv/ri = row minima / argmins of Dm (overhead anchor -> hardest negative surface), cv/ci = column minima / argmins
 * (surface anchor -> hardest negative overhead); loss = (sum_i softplus(a(d_i - rv_i)) + sum_j softplus(a(d_j - cv_j))) / (2B),
 * softplus(x) = log(1+exp(x)). Selection as torch.min: a NaN is the minimum at the first NaN's index, else ties go to the lowest
 * index. Indices are int64 GLOBAL row / column numbers. Fixed-order reductions, no atomics: bitwise reproducible.
 * workspace: witw_batch_hard_workspace_bytes(Bo, Bs) bytes (-1 for a bad shape). */
long long witw_batch_hard_workspace_bytes(int Bo, int Bs);
/* full form on D[B,B] -> rv, ri, cv, ci [B] and the loss [1] */
int witw_batch_hard_fwd(const float* distance, int B, float alpha, float* rv, long long* ri, float* cv, long long* ci, float* loss,
                        void* workspace, void* stream);
/* slab form on the column slab D[Bo][Bs] of the global columns [col0, col0+Bs): rv/ri [Bo] = row minima over THESE columns only
 * (reduce them over the ranks with witw_batch_hard_merge_rows), cv/ci [Bs] = complete column minima */
int witw_batch_hard_slab_mine(const float* distance, int Bo, int Bs, int col0, float* rv, long long* ri, float* cv, long long* ci,
                              void* workspace, void* stream);
/* rv_parts / ri_parts [n_parts][B] (per-rank row minima, rank order) -> the global rv / ri [B]; an earlier part wins a tie */
int witw_batch_hard_merge_rows(const float* rv_parts, const long long* ri_parts, int n_parts, int B, float* rv, long long* ri,
                               void* stream);
/* un-normalised partial of the slab: row terms of the anchors col0..col0+Bs-1 (global rv [Bo]) + column terms of its columns;
 * the sum over the ranks / (2*Bo) is the loss */
int witw_batch_hard_slab_loss(const float* distance, const float* rv, const float* cv, int Bo, int Bs, int col0, float alpha,
                              float* partial, void* stream);
/* the gradient's pair list restricted to the slab's columns (B = global batch, diag [B] = global diagonal, rv/ri [B] global,
 * cv/ci [Bs]; Bs = B, col0 = 0 for the full form): 2*Bs + B entries (pair_o global row, pair_s local column, pair_w weight
 * including grad_loss [1]); entries for rows whose hardest negative lies in another slab are (-1, -1, 0) */
int witw_batch_hard_pairs(const float* diag, const float* rv, const long long* ri, const float* cv, const long long* ci,
                          const float* grad_loss, int B, int Bs, int col0, float alpha, int* pair_o, int* pair_s, float* pair_w,
                          void* stream);
/* dense dL/dD [B,B] of the full form for grad_loss [1] (at most 3B non-zeros) */
int witw_batch_hard_bwd(const float* distance, const float* rv, const long long* ri, const float* cv, const long long* ci,
                        const float* grad_loss, float* grad_distance, int B, float alpha, void* stream);
/* Backward of witw_match_fwd for a pair list instead of a dense grad_distance: grad_distance[o][s] = sum of pair_w over the
 * pairs (o, s). orientation / score / workspace as for witw_match_bwd. grad_ov [Bo,16,4,64] and grad_su [Bs,16,4,We] are written
 * in full (rows without pairs are zero). Pairs with an index outside [0,Bo) x [0,Bs) are ignored. Deterministic: the pairs are
 * sorted into per-row segments on the device (partners ascending, duplicates in list order) and each segment is summed in
 * order; no atomics. n_pairs <= 8192; scratch: witw_match_bwd_pairs_scratch_bytes(n_pairs, Bo, Bs) bytes (-1 if unsupported). */
long long witw_match_bwd_pairs_scratch_bytes(int n_pairs, int Bo, int Bs);
int witw_match_bwd_pairs(const float* ov, const float* su, const long long* orientation, const float* score, const float* workspace,
                         const int* pair_o, const int* pair_s, const float* pair_w, int n_pairs, int Bo, int Bs, int We,
                         float* grad_ov, float* grad_su, void* scratch, void* stream);

/* ---- bf16 inference path of the encoder (BASELINE config "cvig_semantic ... bf16 MFMA"): bf16 NHWC activations
 * (channels padded to 16) and packed bf16 filters, fp32 accumulate on v_mfma_f32_32x32x16_bf16, fp32 bias;
 * the last layer writes the fp32 NCHW embedding (out_nchw_f32). Pointers typed void* carry bf16 data. */
/* MFMA shape of the bf16 inference forward where both kernels apply (Cout >= 128, stride 1, >= 512 workgroups of 8 waves,
 * Cin % 32 == 0, bf16 NHWC out, no gate / Dropout2d scale / pool codes): 1 = v_mfma_f32_16x16x32_bf16 (default; two taps of a
 * 16-channel chunk per MFMA, the ninth tap of an even chunk shares its MFMA with the ninth tap of the next chunk), 0 =
 * v_mfma_f32_32x32x16_bf16. enable < 0 only queries; returns the previous setting. Results agree to one bf16 ulp. */
int witw_conv3x3_bf16_mfma16(int enable);
/* 1 (default): plain bf16 forwards with 64 input channels (layer 5 of the trunk, model/cvig_fov.py:261-262) and H % 8 == 0,
 * W % 32 == 0, Cout % 64 == 0, >= 4096 (8 x 32 tile, 64-channel block) units run on the kernel that keeps the filter block in
 * LDS (csrc/conv3x3_bf16_wres.hip); 0: on the tiled kernels. enable < 0 only queries; returns the previous setting. Bit-identical
 * to the 32x32x16 tiled kernel. */
int witw_conv3x3_bf16_wres(int enable);
long long witw_conv3x3_bf16_packed_elems(int cout, int cin);
int witw_conv3x3_bf16_pack_weights(const float* w_kcrs, void* wpk_bf16, int cout, int cin, void* stream);
/* transpose_flip != 0: the dgrad filter of the source tensor [cin][cout][3][3] (cout, cin describe the packed filter) */
int witw_conv3x3_bf16_pack_weights_ex(const float* w_kcrs, void* wpk_bf16, int cout, int cin, int transpose_flip, void* stream);
/* n filter images (and their biases) in one launch per 16 entries: what a bf16 training step re-packs after every Adam update
 * (csrc/pack_multi.hip). Entry i as witw_conv3x3_bf16_pack_weights_ex(w[i], wpk[i], cout[i], cin[i], transpose[i]); bias[i] NULL
 * or fp32 [cout[i]], copied to the first cout[i] floats of bias_dst[i]. Same bits as the one-at-a-time entry. */
int witw_conv3x3_bf16_pack_weights_multi(const void* const* w, void* const* wpk, const void* const* bias, void* const* bias_dst,
                                         const int* cout, const int* cin, const int* transpose, int n, void* stream);
int witw_nchw_f32_to_nhwc_bf16(const float* x, void* y_bf16, int B, int C, int H, int W, int Cpad, void* stream);
int witw_conv3x3_bf16_fwd(const void* x_bf16, const void* wpk_bf16, const float* bias, void* y, int B, int H, int W, int Cin,
                          int Cout, int stride_h, int pad_circular, int relu, int pool, int out_nchw_f32, void* stream);

/* ---- fp32-grade inference on the fp16 MFMA ("fp16x3"): every value is carried as hi = fp16(x), lo = fp16(x - hi) and a
 * product is hi*hi + lo*hi + hi*lo with fp32 accumulation (3 MFMAs of the 2.5 PF/s pipe per fp32-equivalent product; the
 * encoder stays within 2e-5 of fp64, like the fp32 MFMA path, inside the reference goldens' 1e-4). Activations are NHWC
 * "split-fp16": per pixel and 8 channels 16 B of hi then 16 B of lo ([B,H,W,C/8,2,8] fp16, 4 B per value). Same layer
 * arguments as witw_conv3x3_bf16_fwd; the last layer writes the fp32 NCHW embedding (out_nchw_f32). */
long long witw_conv3x3_f16x3_packed_elems(int cout, int cin);
int witw_conv3x3_f16x3_pack_weights(const float* w_kcrs, void* wpk_f16, int cout, int cin, void* stream);
int witw_nchw_f32_to_split_f16(const float* x, void* y_split, int B, int C, int H, int W, int Cpad, void* stream);
int witw_split_f16_to_f32(const void* x_split, float* y /*[pixels][C]*/, long long pixels, int C, void* stream);
int witw_conv3x3_f16x3_fwd(const void* x_split, const void* wpk_f16, const float* bias, void* y, int B, int H, int W, int Cin,
                           int Cout, int stride_h, int pad_circular, int relu, int pool, int out_nchw_f32, void* stream);
/* training forms, as witw_conv3x3_bf16_fwd_ex / witw_conv3x3_bf16_pack_weights_ex: Dropout2d scale, ReLU gate (a split-fp16
 * tensor shaped like y; the epilogue contract at witw_conv3x3_fwd_ex, the gate's sign read from its hi half; tests/
 * test_conv_epilogue_gpu.py), zero-interleaved rows; transpose_flip packs the dgrad filter of the source [cin][cout][3][3] */
int witw_conv3x3_f16x3_pack_weights_ex(const float* w_kcrs, void* wpk_f16, int cout, int cin, int transpose_flip, void* stream);
int witw_conv3x3_f16x3_fwd_ex(const void* x_split, const void* wpk_f16, const float* bias, const float* dropmask,
                              const void* gate_split, void* y, unsigned char* pool_code, int* overflow_flag, int B, int H, int W,
                              int Cin, int Cout, int stride_h, int pad_circular, int relu, int pool, int out_nchw_f32, int dilate_h,
                              void* stream);
/* pool_code (uint8 [B,Hy,Wy,Cout]) as in witw_conv3x3_bf16_fwd_ex; overflow_flag: NULL or a device int set to 1 when a
 * split-fp16 output leaves the fp16 range (|v| > 65504 or NaN cannot be carried as hi + lo). The max-pool backward on split tensors: */
int witw_maxpool2x2_bwd_split(const void* dy_split, const unsigned char* code, void* dx_split, int B, int Hp, int Wp, int H, int W,
                              int C, void* stream);

/* weight gradient of the fp16x3 training step (csrc/wgrad_f16x3.hip): operands in the batch-octet split layout
 * [ceil(B/8)][H][W][C][2][8] fp16 (witw_split_f16_to_octet from split-fp16 NHWC), products hi*hi + lo*hi + hi*lo on the fp16
 * MFMA; dz_split = the gradient as split-fp16 NHWC (bias gradient; NULL with db NULL); dw / db fp32. */
long long witw_octet_split_elems(int B, int H, int W, int C);
int witw_split_f16_to_octet(const void* x_split, void* y_oct, int B, int H, int W, int C, void* stream);
long long witw_conv3x3_wgrad_f16x3_workspace_floats(int B, int H, int W, int Cin, int Cout, int stride_h);
int witw_conv3x3_wgrad_f16x3(const void* x_oct, const void* dz_oct, const void* dz_split, float* dw, float* db, float* workspace,
                             int B, int H, int W, int Cin, int cin_real, int Cout, int stride_h, int pad_circular, int accumulate,
                             void* stream);

/* ---- bf16 (mixed-precision) TRAINING step of the encoder: the backward of the reference's training loop
 * (model/cvig_fov.py:447-460, autograd through torch.nn.Conv2d) with bf16 MFMA operands, fp32 accumulate, fp32
 * weight gradients / master weights / Adam.
 * witw_conv3x3_bf16_fwd_ex = witw_conv3x3_bf16_fwd plus: dropmask [B,Cout] fp32 (Dropout2d scale before the ReLU,
 * :287-288) or NULL; gate_bf16 = bf16 tensor shaped like y or NULL (outputs where gate <= 0 are zeroed: the ReLU
 * backward of a dgrad launch, which is this kernel on witw_conv3x3_bf16_pack_weights of the transposed, tap-rotated
 * filter); dilate_h = x holds (H-1)/2+1 physical rows standing for H zero-interleaved rows (dgrad of a stride-(2,1) layer);
 * pool_code = NULL or uint8 [B,Hy,Wy,Cout]: arg-max position (dy*2+dx) of the fused max-pool, consumed by
 * witw_maxpool2x2_bwd_bf16 (dy bf16 [B,Hp,Wp,C] -> dx bf16 [B,H,W,C]). Order of the epilogue and the gate: the contract stated
 * at witw_conv3x3_fwd_ex (open exactly where the bf16 gate is > 0, NaN closes it, a closed output is +0.0), tests/
 * test_conv_epilogue_gpu.py. */
int witw_conv3x3_bf16_fwd_ex(const void* x_bf16, const void* wpk_bf16, const float* bias, const float* dropmask,
                             const void* gate_bf16, void* y, unsigned char* pool_code, int B, int H, int W, int Cin, int Cout,
                             int stride_h, int pad_circular, int relu, int pool, int out_nchw_f32, int dilate_h, void* stream);
int witw_maxpool2x2_bwd_bf16(const void* dy_bf16, const unsigned char* code, void* dx_bf16, int B, int Hp, int Wp, int H, int W,
                             int C, void* stream);
/* Weight gradient on v_mfma_f32_32x32x16_bf16. Both operands in the batch-octet layout [ceil(B/8)][H][W][C][8 images]
 * (witw_nhwc_bf16_to_octet; witw_octet_elems = its element count): the 8 k values of an MFMA lane are 8 images at one
 * pixel, so a filter tap is a pixel offset and no transposition is needed. x_oct = the layer's input, dz_oct = the
 * gradient at its output; dw [Cout][cin_real][3][3] fp32, db [Cout] fp32 or NULL (summed inside the same kernel);
 * workspace of witw_conv3x3_wgrad_bf16_workspace_floats floats. */
long long witw_octet_elems(int B, int H, int W, int C);
int witw_nhwc_bf16_to_octet(const void* x_bf16, void* y_bf16, int B, int H, int W, int C, void* stream);
long long witw_conv3x3_wgrad_bf16_workspace_floats(int B, int H, int W, int Cin, int Cout, int stride_h);
int witw_conv3x3_wgrad_bf16(const void* x_oct, const void* dz_oct, float* dw, float* db, float* workspace, int B, int H, int W,
                            int Cin, int cin_real, int Cout, int stride_h, int pad_circular, int accumulate, void* stream);
/* Round 5: the same gradient straight from the NHWC bf16 tensors the forward / dgrad launches write (x [B][H][W][Cin], dz
 * [B][Ho][W][Cout]) -- no re-layout pass: the MFMA's k index is the pixel, the [pixel][channel] LDS image is transposed on the
 * way out by ds_read_b64_tr_b16 (replaces autograd through torch.nn.Conv2d in model/cvig_fov.py:447-460 like the entry above,
 * and is what the bf16 training step now calls). Workspace of witw_conv3x3_wgrad_bf16_nhwc_workspace_floats floats. */
long long witw_conv3x3_wgrad_bf16_nhwc_workspace_floats(int B, int H, int W, int Cin, int Cout, int stride_h);
/* 1: eligible layers (stride 1, Cin > 32, Cout > 64, W % 32 == 0) run it on v_mfma_f32_16x16x32_bf16; 0 (default; that form
 * measured 3-9 % slower): v_mfma_f32_32x32x16_bf16. enable < 0 only queries; returns the previous setting. Set it BEFORE sizing the
 * workspace. Same parity bar for both. */
int witw_conv3x3_wgrad_bf16_mfma16(int enable);
int witw_conv3x3_wgrad_bf16_nhwc(const void* x_nhwc, const void* dz_nhwc, float* dw, float* db, float* workspace, int B, int H, int W,
                                 int Cin, int cin_real, int Cout, int stride_h, int pad_circular, int accumulate, void* stream);

/* ---- 2x2 sub-window form of the 3x3 kernels: cvig_baseline's Conv2d(k=4,s=2,p=0) (model/cvig_baseline.py:236-252) is a
 * 2x2 convolution over the space-to-depth(2) image, i.e. a 3x3 window whose first tap row/column are zero (dgrad: last
 * row/column); these entries run only the 4 live taps (2.25x fewer MFMAs than witw_conv3x3_fwd_ex on the zero-filled
 * 3x3 filter, same results). pack: taps {1,2}^2 of w [cout][cin][3][3] (transpose_flip: taps {0,1}^2 of the dgrad
 * filter of the source [cin][cout][3][3]); fwd: tap_base = 1 with a forward-packed filter, 0 with a dgrad-packed one;
 * wgrad: taps {1,2}^2 of dw, exact zeros elsewhere (workspace as witw_conv3x3_wgrad, stride 1). */
long long witw_conv3x3_packed_floats_taps4(int cout, int cin);
int witw_conv3x3_pack_weights_taps4(const float* w_kcrs, float* wpk, int cout, int cin, int transpose_flip, void* stream);
int witw_conv3x3_fwd_taps4(const float* x, const float* wpk4, const float* bias, const float* gate, const float* post_scale,
                           const float* post_shift, float* y, int B, int H, int W, int Cin, int Cout, int relu,
                           float lrelu_slope, int tap_base, void* stream);
/* The same convolution with two options for the deep, small-map layers of the encoder (model/cvig_baseline.py:240-252, conv5-7:
 * 16x16 .. 4x4 maps with K = 4 taps x 2048 channels start far fewer workgroups than the chip has CUs):
 *  ksplit > 1  split-K: y is a workspace of ksplit*B*H*W*Cout floats receiving the RAW partial sums of each K slice
 *              ([ksplit][B,H,W,Cout]; no bias / activation / affine; gate must be NULL); witw_taps4_splitk_finish reduces them.
 *              witw_conv3x3_taps4_ksplit returns the factor the library would pick (1 = the plain launch fills the chip).
 *  s2d != 0    (ksplit == 1) y is written as the space-to-depth(2) image of the valid_h x valid_w region,
 *              [B, ceil(valid_h/2), ceil(valid_w/2), 4*Cout], zeros outside it: the layout the next k=4,s=2 layer reads
 *              (replaces a witw_space_to_depth2 pass over the activation). */
int witw_conv3x3_taps4_ksplit(int B, int H, int W, int Cin, int Cout);
int witw_conv3x3_fwd_taps4_ex(const float* x, const float* wpk4, const float* bias, const float* gate, const float* post_scale,
                              const float* post_shift, float* y, int B, int H, int W, int Cin, int Cout, int relu,
                              float lrelu_slope, int tap_base, int ksplit, int s2d, int valid_h, int valid_w, void* stream);
int witw_conv3x3_wgrad_taps4(const float* x, const float* dz, float* dw, float* db, float* workspace, int B, int H, int W,
                             int Cin, int cin_real, int Cout, int accumulate, void* stream);

/* ---- cvig_baseline (model/cvig_baseline.py). Conv2d(k=4,s=2,p=0) = the 3x3 kernel above on the
 * space-to-depth(2) image with a filter whose first tap row/column is zero. */
/* x NHWC [B,Hp,Wp,C] (NCHW if in_nchw) with valid region HxW -> NHWC [B,ceil(H/2),ceil(W/2),Cpad], channel
 * (dy*2+dx)*C+c; normalize=1 applies x/255, -1+2x (:265-266); scale/shift (NULL or [C]): per-channel affine of a
 * train-mode BatchNorm applied on the fly (also accepted by witw_gem_pool). */
/* The FIRST block of an encoder in one launch (model/cvig_baseline.py:236-240 conv1/bn1, :265-268 the in-model x/255, -1+2x,
 * LeakyReLU, eval-mode BatchNorm): x NCHW fp32 [B,C<=5,H,W] -> y [B, ceil(vh/2), ceil(vw/2), 256], the space-to-depth(2) image of
 * the vh x vw = ((H-4)/2+1) x ((W-4)/2+1) valid outputs (zeros elsewhere) that the second block reads. w: torch layout
 * [64][C][4][4]; scale / shift [64] (both or neither). Replaces witw_space_to_depth2(in_nchw, normalize) +
 * witw_conv3x3_fwd_taps4_ex(s2d = 1) for that block. */
int witw_conv4x4s2_first_fwd(const float* x, const float* w, const float* bias, const float* scale, const float* shift, float* y,
                             int B, int C, int H, int W, int normalize, float lrelu_slope, void* stream);
/* ---- cvig_baseline inference with bf16 operands on v_mfma_f32_16x16x32_bf16 (blocks 1-4 of the encoder, model/cvig_baseline.py:
 * 236-249, 265-275; blocks 5-7, the pooling and the normalisation stay on the fp32 entries).
 * witw_conv4x4s2_first_fwd_bf16: witw_conv4x4s2_first_fwd with y bf16 [B, ceil(vh/2), ceil(vw/2), 256]: the same fp32 arithmetic in
 * the same order, each output rounded once to nearest-even. */
int witw_conv4x4s2_first_fwd_bf16(const float* x, const float* w, const float* bias, const float* scale, const float* shift, void* y_bf16,
                                  int B, int C, int H, int W, int normalize, float lrelu_slope, void* stream);
/* The 2x2-tap convolution of blocks 2-4 (model/cvig_baseline.py:241-249, 267-275: Conv2d(k=4, s=2) -> LeakyReLU -> BatchNorm2d in
 * eval mode) on bf16 operands with fp32 accumulation. pack: taps {1,2}^2 of w [cout][cin][3][3] fp32 (what witw_conv4x4_to_k3
 * writes), rounded once to bf16 (nearest-even), into wpk of witw_conv3x3_bf16_packed_elems_taps4(cout, cin) bf16 elements (cin
 * padded to 16 with zeros); forward filters only. fwd: x NHWC bf16 [B,H,W,Cin] (Cin % 16 == 0, H, W >= 2), bias fp32 [Cout],
 * post_scale / post_shift fp32 [Cout] or both NULL ->
 *   y[b, r/2, c/2, ((r&1)*2 + (c&1))*Cout + n] = lrelu(sum_{ty,tx,ci} x[b,r+ty,c+tx,ci] * w[n,ci,1+ty,1+tx] + bias[n]) * post_scale[n]
 *                                                 + post_shift[n]      for r < valid_h, c < valid_w, +0.0 elsewhere
 * (x zero past H / W; 1 <= valid_h <= H, 1 <= valid_w <= W), y [B, ceil(valid_h/2), ceil(valid_w/2), 4*Cout]: the layout of
 * witw_conv3x3_fwd_taps4_ex with s2d != 0. The epilogue runs in fp32 in that entry's order; y is bf16 with ONE nearest-even
 * rounding per output (out_f32 == 0) or fp32 without any (out_f32 != 0). Any Cout >= 1 (a slower store unless Cout % 8 == 0). */
long long witw_conv3x3_bf16_packed_elems_taps4(int cout, int cin);
int witw_conv3x3_bf16_pack_weights_taps4(const float* w_kcrs, void* wpk_bf16, int cout, int cin, void* stream);
int witw_conv3x3_bf16_fwd_taps4(const void* x_bf16, const void* wpk_bf16, const float* bias, const float* post_scale,
                                const float* post_shift, void* y, int B, int H, int W, int Cin, int Cout, float lrelu_slope,
                                int valid_h, int valid_w, int out_f32, void* stream);
/* Blocks 5-7 of the same encoders on bf16 operands (SurfaceEncoder(precision='bf16_all')): the split-K form of the convolution above
 * over a g x g mosaic. x NHWC bf16 [Bm,H,W,Cin] (Cin % 16 == 0; the layout witw_space_to_depth2_mosaic_bf16 writes, or the plain batch),
 * wpk from witw_conv3x3_bf16_pack_weights_taps4 (unchanged), 1 <= ksplit <= Cin/16, Cout % 4 == 0 ->
 *   ws[s, b, r, c, n] = sum_{ty,tx} sum_{ci in slice s} x[b,r+ty,c+tx,ci] * w[n,ci,1+ty,1+tx]        for every r < H, c < W, n < Cout
 * (x zero past H / W), ws fp32 [ksplit][Bm,H,W,Cout]: RAW partial sums in fp32, no bias, no activation, no affine, and no element of
 * ws left unwritten. Slice s is a contiguous run of the Cin/16 chunks of 16 channels, the first (Cin/16) % ksplit slices one chunk
 * longer than the rest. witw_taps4_splitk_finish adds the slices in slice order (deterministic for a given ksplit), applies the
 * epilogue and gathers the valid outputs. witw_conv3x3_bf16_taps4_ksplit returns the factor the library would pick for the shape
 * (WITW_CONV_KSPLIT forces it), -1 on a bad shape. */
int witw_conv3x3_bf16_taps4_ksplit(int Bm, int H, int W, int Cin, int Cout);
int witw_conv3x3_bf16_fwd_taps4_splitk(const void* x_bf16, const void* wpk_bf16, float* ws, int Bm, int H, int W, int Cin, int Cout,
                                       int ksplit, void* stream);
/* witw_space_to_depth2_mosaic (below) with a bf16 output: x fp32 NHWC [B,H,W,C] (C % 4 == 0) -> y bf16 [ceil(B/g^2), g*ceil(H/2),
 * g*ceil(W/2), 4C], ONE nearest-even rounding per element, +0.0 where no source exists (16-byte stores where C % 8 == 0). */
int witw_space_to_depth2_mosaic_bf16(const float* x, void* y_bf16, int B, int H, int W, int C, int g, void* stream);
/* ---- cvig_baseline TRAINING with bf16 operands (blocks 2-4 under train_precision='bf16': forward, data gradient and weight gradient
 * of model/cvig_baseline.py:241-249, 267-275 on the bf16 MFMA with fp32 accumulation; BatchNorm, LeakyReLU gates, pooling, blocks 1 and
 * 5-7, the loss and Adam stay on the fp32 entries). Rounded (nearest-even, once): the filter, a block's input, a block's output gradient.
 * pack_weights_taps4_ex: witw_conv3x3_bf16_pack_weights_taps4 with transpose_flip as in witw_conv3x3_pack_weights_taps4: != 0 packs taps
 *   {0,1}^2 of the data-gradient filter, (cout, cin) describe the PACKED filter, the source is [cin][cout][3][3]:
 *   packed tap (ty, tx) of (co, ci) = bf16(w[ci][co][2-ty][2-tx]). transpose_flip == 0 is the entry without _ex.
 * fwd_taps4_plain: x NHWC bf16 [B,H,W,Cin] (Cin % 16 == 0), bias fp32 [Cout] or NULL, off = 1 - tap_base ->
 *   y[b,r,c,n] = act(sum_{ty,tx in {0,1}} sum_ci x[b,r+ty-off,c+tx-off,ci] * wpk[n,ci,tap (ty,tx)] + bias[n])   for r < valid_h, c < valid_w,
 *   +0.0 elsewhere (x zero outside [0,H) x [0,W)); act = LeakyReLU(lrelu_slope) when lrelu != 0, else none; y fp32 [B,H,W,Cout], every
 *   element written, never rounded: the layout witw_conv3x3_fwd_taps4 gives and witw_bn_train_stats / witw_bn_lrelu_bwd_ex read. tap_base = 1
 *   with a forward-packed filter is the block's forward, tap_base = 0 with a transpose_flip-packed one its data gradient. Any Cout >= 1.
 * space_to_depth2_bf16: witw_space_to_depth2 for an NHWC source with C % 4 == 0 and Cpad == 4C, bf16 out: y[b,h2,w2,(dy*2+dx)*C+c] =
 *   bf16(x[b,2h2+dy,2w2+dx,c] * scale[c] + shift[c]) inside the H x W valid region (fp32 multiply, then add, one rounding), +0.0 outside
 *   it whatever the shift; scale / shift both NULL: no affine. 16-byte stores where C % 8 == 0.
 * f32_to_bf16: y[i] = bf16(x[i]), i < n.
 * wgrad_bf16_taps4: x [B,H,W,Cin] (Cin % 8 == 0), dz [B,H,W,Cout] (Cout % 4 == 0), both NHWC bf16 ->
 *   dw[n, ci, 1+ty, 1+tx] (+)= sum_{b,r,c} dz[b,r,c,n] * x[b,r+ty,c+tx,ci]   (x zero past H / W; ci < cin_real; fp32 sums),
 *   db[n] (+)= sum_{b,r,c} dz[b,r,c,n] (db may be NULL); dw [Cout][cin_real][3][3] fp32, the five taps outside {1,2}^2 +0 (accumulate == 0)
 *   or untouched. The weight-gradient contract above holds (workspace of witw_conv3x3_wgrad_bf16_taps4_workspace_floats floats, fixed
 *   split order: bitwise reproducible). */
int witw_conv3x3_bf16_pack_weights_taps4_ex(const float* w_kcrs, void* wpk_bf16, int cout, int cin, int transpose_flip, void* stream);
int witw_conv3x3_bf16_fwd_taps4_plain(const void* x_bf16, const void* wpk_bf16, const float* bias, float* y, int B, int H, int W, int Cin,
                                      int Cout, int lrelu, float lrelu_slope, int tap_base, int valid_h, int valid_w, void* stream);
int witw_space_to_depth2_bf16(const float* x, void* y_bf16, int B, int Hp, int Wp, int H, int W, int C, const float* scale,
                              const float* shift, void* stream);
int witw_f32_to_bf16(const float* x, void* y_bf16, long long n, void* stream);
long long witw_conv3x3_wgrad_bf16_taps4_workspace_floats(int B, int H, int W, int Cin, int Cout);
int witw_conv3x3_wgrad_bf16_taps4(const void* x_nhwc, const void* dz_nhwc, float* dw, float* db, float* workspace, int B, int H, int W,
                                  int Cin, int cin_real, int Cout, int accumulate, void* stream);
int witw_space_to_depth2(const float* x, float* y, int B, int Hp, int Wp, int H, int W, int C, int Cpad, int in_nchw,
                         int normalize, const float* scale, const float* shift, void* stream);
/* Mosaic space-to-depth: x NHWC [B,H,W,C] (C % 4 == 0) -> y [ceil(B/g^2), g*ceil(H/2), g*ceil(W/2), 4C]: image b is cell b % g^2
 * (row-major) of mosaic image b / g^2. A k=4,s=2 layer over an n x n s2d map has (n-1)^2 valid outputs, so no valid window crosses
 * a cell: conv6 / conv7 (8x8, 4x4 maps) run as g = 2 / 4 mosaics that fill the kernel's 16x16 tile. */
int witw_space_to_depth2_mosaic(const float* x, float* y, int B, int H, int W, int C, int g, void* stream);
/* Reduce the split-K partial sums ws [ksplit][ceil(B/g^2), g*h, g*w, C] in slice order and apply bias, activation (0 none, 1 ReLU,
 * 2 LeakyReLU) and the optional per-channel affine: y [B,vh,vw,C] = the valid outputs of every image. */
int witw_taps4_splitk_finish(const float* ws, int ksplit, const float* bias, int act, float lrelu_slope, const float* post_scale,
                             const float* post_shift, float* y, int B, int g, int h, int w, int vh, int vw, int C, void* stream);
/* f[b,col0+c] = (mean relu(x)^p)^(1/p) over the valid HxW region (:276-282); f has row length ldf. */
int witw_gem_pool(const float* x, float* f, int B, int Hp, int Wp, int H, int W, int C, int ldf, int col0, float p,
                  const float* scale, const float* shift, void* stream);
/* f[b,:] /= sqrt(|f[b,:]|_2) in place (:284) */
int witw_embed_normalize(float* f, int B, int n, void* stream);
/* D[i][j] = |a_i - b_j|^2 (or its square root: Euclidean ranking distance of :457-458) */
int witw_pairwise_sqdist(const float* a, const float* b, float* D, int Na, int Nb, int n, int take_sqrt, void* stream);
/* Gallery retrieval on [rows, n] embeddings at GEMM cost (witw_amd/cvig_baseline.py: retrieve), 1 <= n <= 12288.
 * witw_row_sqnorm: out[i] = |x_i|^2, one wave per row.
 * witw_sqdist_gemm: D[i][j] = max(0, gn[i] + qn[j] - 2 g_i.q_j) (squared, no root) by a tiled fp32 MFMA GEMM; gn / qn = the
 * witw_row_sqnorm of g / q. Any Ng, Nq >= 1 (Ng is NOT bounded by 65,535). The product form cancels on near pairs: D is within
 * 3 gamma_(n+16) (max gn + max qn) of the value below (gamma_m = m u / (1 - m u), u = 2^-24), not its bits.
 * witw_sqdist_pairs: out[p] = the value witw_pairwise_sqdist(g, q, ..., take_sqrt) writes at [pair_g[p]][pair_q[p]], bit for
 * bit (the same difference-form sum in the same order), one thread per pair; indices must be inside the operands' rows; P may be 0. */
int witw_row_sqnorm(const float* x, float* out, int N, int n, void* stream);
int witw_sqdist_gemm(const float* g, const float* q, const float* gn, const float* qn, float* D, int Ng, int Nq, int n, void* stream);
int witw_sqdist_pairs(const float* g, const float* q, const int* pair_g, const int* pair_q, float* out, int P, int n, int take_sqrt,
                      void* stream);
/* exhaustive_minibatch_triplet_loss (:286-315) from D[i][j] = |embed1_i - embed2_j|^2; workspace B floats */
int witw_exhaustive_triplet_loss(const float* D, int B, int soft_margin, float alpha, float margin, float* loss,
                                 float* workspace, void* stream);

/* training mode of cvig_baseline (BatchNorm2d batch statistics, autograd of :267-315) */
long long witw_bn_workspace_floats(int B, int H, int W, int C);
/* batch mean / biased variance over the valid HxW region of a [B,Hp,Wp,C] tensor -> mean, invstd, and the affine
 * y = a*scale + shift; running_mean/var (may be NULL) are updated with `momentum` and the unbiased variance. */
int witw_bn_train_stats(const float* a, int B, int Hp, int Wp, int H, int W, int C, const float* gamma, const float* beta,
                        float eps, float momentum, float* mean, float* invstd, float* scale, float* shift, float* running_mean,
                        float* running_var, float* workspace, void* stream);
/* backward of y = BatchNorm_train(LeakyReLU(z)): a = LeakyReLU(z) as saved, dy at y -> dz (0 outside the valid region),
 * dgamma, dbeta. */
int witw_bn_lrelu_bwd(const float* a, const float* dy, float* dz, float* dgamma, float* dbeta, const float* mean,
                      const float* invstd, const float* gamma, int B, int Hp, int Wp, int H, int W, int C, float slope,
                      float* workspace, void* stream);
/* the same with dy still in the space-to-depth layout the next block's data-gradient conv wrote ([B, ceil(H/2), ceil(W/2), dy_s2d_cp],
 * channel ((h&1)*2+(w&1))*C + c), read in place: saves the witw_depth_to_space2 pass; dy_s2d_cp = 0: dy is [B,Hp,Wp,C] */
int witw_bn_lrelu_bwd_ex(const float* a, const float* dy, float* dz, float* dgamma, float* dbeta, const float* mean,
                         const float* invstd, const float* gamma, int B, int Hp, int Wp, int H, int W, int C, float slope,
                         int dy_s2d_cp, float* workspace, void* stream);
/* ---- the same BatchNorm2d cut where a collective fits (csrc/baseline_bn_sync.hip): statistics of a batch that is spread over N
 * ranks. Each direction is: partial sums on every rank -> the caller SUMS the [2*C] vectors and the counts over the ranks -> a second
 * entry uses the summed vector and the global count. With one rank the two run back to back, no collective. Tensors, valid region,
 * dy_s2d_cp and `workspace` (witw_bn_workspace_floats(B, H, W, C) floats, contents on entry irrelevant) are as in the entries above.
 * Every sum is taken in a fixed order without atomics: a repeated call gives the same bits. A refusal (non-zero return) launches
 * nothing and writes nothing; nothing is written outside the named outputs and the workspace.
 * bn_partial_stats: part[c] = S1 = sum (a - pivot[c]), part[C + c] = S2 = sum (a - pivot[c])^2 over the valid region (any number of
 *   values per channel, one included). pivot [C] is an INPUT and must hold the same values on every rank whose sums are added (the
 *   layer's running_mean as it stood before the step); the closer it is to the mean, the less of the variance is lost to cancellation.
 * bn_finalize_stats: part_sum [2*C] = the sums of every rank added, count = the values per channel behind them (global B*H*W):
 *   mean = pivot + S1/n, biased var = max(0, S2/n - (S1/n)^2), invstd = (var + eps)^-1/2, scale = gamma * invstd, shift = beta -
 *   mean * scale; running_mean / running_var (both NULL or neither) updated with `momentum` and the unbiased variance var * n / (n - 1).
 *   pivot may be running_mean itself. count <= 1 is REFUSED, as witw_bn_train_stats refuses one value per channel (torch raises there
 *   too): running_var has no unbiased update at n = 1, and nothing is written.
 * bn_lrelu_bwd_partial: part[c] = sum dy, part[C + c] = sum dy * xhat, xhat = (a - mean[c]) * invstd[c], over the valid region.
 * bn_lrelu_bwd_apply: sums [2*C] = those vectors of every rank added, count = the global values per channel (>= this tensor's own
 *   B*H*W, else refused) -> dz = lrelu'(a) * gamma * invstd * (dy - sums[c]/n - xhat * sums[C + c]/n) on the valid region, 0 outside
 *   it, every element of dz written: what witw_bn_lrelu_bwd_ex writes when count is its own B*H*W. dbeta = sums[0..C) and dgamma =
 *   sums[C..2C) are the GLOBAL parameter gradients, complete on every rank. */
int witw_bn_partial_stats(const float* a, int B, int Hp, int Wp, int H, int W, int C, const float* pivot, float* part,
                          float* workspace, void* stream);
int witw_bn_finalize_stats(const float* part_sum, const float* pivot, long long count, const float* gamma, const float* beta,
                           float eps, float momentum, float* mean, float* invstd, float* scale, float* shift, float* running_mean,
                           float* running_var, int C, void* stream);
int witw_bn_lrelu_bwd_partial(const float* a, const float* dy, const float* mean, const float* invstd, int B, int Hp, int Wp, int H,
                              int W, int C, int dy_s2d_cp, float* part, float* workspace, void* stream);
int witw_bn_lrelu_bwd_apply(const float* a, const float* dy, float* dz, const float* mean, const float* invstd, const float* gamma,
                            const float* sums, long long count, int B, int Hp, int Wp, int H, int W, int C, float slope,
                            int dy_s2d_cp, void* stream);
/* inverse of witw_space_to_depth2 for gradients: g [B,ceil(H/2),ceil(W/2),Cpad] -> dx [B,Hp,Wp,C] (+ add, may be NULL) */
int witw_depth_to_space2(const float* g, const float* add, float* dx, int B, int Hp, int Wp, int H, int W, int C, int Cpad,
                         void* stream);
int witw_gem_pool_bwd(const float* a, const float* scale, const float* shift, const float* f, const float* df, float* dy, int B,
                      int Hp, int Wp, int H, int W, int C, int ldf, int col0, float p, int accumulate, void* stream);
/* g: un-normalised feature [B,n], df: gradient at g/sqrt(|g|) -> dg */
int witw_embed_normalize_bwd(const float* g, const float* df, float* dg, int B, int n, void* stream);
/* backward of witw_pairwise_sqdist + witw_exhaustive_triplet_loss; workspace B*B floats */
int witw_exhaustive_triplet_loss_bwd(const float* e1, const float* e2, const float* D, const float* grad_loss, float* de1,
                                     float* de2, int B, int n, int soft_margin, float alpha, float margin, float* workspace,
                                     void* stream);
/* The same loss (:286-315) over the GLOBAL batch of B pairs when each of the ranks holds b of them (the reference gathers its
 * nn.DataParallel replicas' embeddings and takes the loss over all B, :339-343): this rank's COLUMN SLAB T [B,b],
 * T[g][c] = |x_g - y_c|^2 from witw_pairwise_sqdist(x, y), x [B,n] the all-gathered embeddings of one side, y [b,n] this rank's
 * of the other, column c being column col0 + c of the global matrix (col0 = rank * b). diag [B]: the global diagonal,
 * diag[col0 + c] = T[col0 + c][c] on the owning rank, all-gathered. l(x) = log(1 + exp(alpha x)) if soft_margin else
 * max(x + margin, 0) (:297-301), l' its derivative. B >= 2, 1 <= b <= B, 0 <= col0, col0 + b <= B; no pointer may be NULL.
 * Every sum has a fixed order, nothing is accumulated atomically: a call repeated gives the same bits.
 * _fwd: partial[0] = sum_c sum_{g != col0+c} l(diag[col0+c] - T[g][c]) + l(diag[g] - T[g][c]), un-normalised: the caller sums
 *       the ranks' partials and divides by 2B(B-1) (:313-315). workspace: B floats.
 * _sig: colsig[c] = sum_{g != col0+c} l'(diag[col0+c] - T[g][c]) (b floats, complete) and rowsig[g] = sum_{c: col0+c != g}
 *       l'(diag[g] - T[g][c]) (B floats, this slab's part: the caller sums it over the ranks).
 * _bwd: G [B,b] = dL/dT for grad_loss (device scalar) of the GLOBAL loss, sc = grad_loss / (2B(B-1)):
 *       G[g][c] = -(l'(diag[col0+c] - T[g][c]) + l'(diag[g] - T[g][c])) sc off the diagonal, G[col0+c][c] = (rowsig[col0+c] +
 *       colsig[c]) sc on it; rowsig = the SUMMED row sums. */
int witw_exhaustive_loss_slab_fwd(const float* T, const float* diag, int B, int b, int col0, int soft_margin, float alpha, float margin,
                                  float* partial, float* workspace, void* stream);
int witw_exhaustive_loss_slab_sig(const float* T, const float* diag, int B, int b, int col0, int soft_margin, float alpha, float margin,
                                  float* rowsig, float* colsig, void* stream);
int witw_exhaustive_loss_slab_bwd(const float* T, const float* diag, const float* rowsig, const float* colsig, const float* grad_loss,
                                  float* G, int B, int b, int col0, int soft_margin, float alpha, float margin, void* stream);
/* Backward of T = witw_pairwise_sqdist(x [B,n], y [b,n]) for any B, b >= 1, n <= 12288 (autograd of :307-308):
 * dx[g] = 2 sum_c G[g][c] (x_g - y_c) [B,n], dy[c] = 2 sum_g G[g][c] (y_c - x_g) [b,n]; dx or dy may be NULL (not both).
 * A workgroup keeps 8 (2 on a short side) output rows in registers against one read of the other side. */
int witw_sqdist_rect_bwd(const float* x, const float* y, const float* G, float* dx, float* dy, int B, int b, int n, void* stream);
/* Batch-hard form of the same loss on the same column slab (opt-in, not in the reference; Hermans et al. 2017): every anchor against
 * its hardest negative of the GLOBAL batch only. With Tm = T whose global diagonal is +inf: rv/ri [B] = minimum / argmin of every
 * global row of Tm, cv/ci [b] = of every column of the slab, mined by witw_batch_hard_slab_mine(T, B, b, col0) and, over the ranks,
 * witw_batch_hard_merge_rows (their selection rule; int64 global indices, constants for the gradient). d_k = the global diagonal,
 * l and l' as above (l'(x) = [x + margin > 0] for the hard margin; a NaN argument stays a NaN in l).
 *   loss = (sum_i l(d_i - rv[i]) + sum_j l(d_j - cv[j])) / 2B
 *   sc = grad_loss / 2B, w_r[i] = sc l'(d_i - rv[i]), w_c[j] = sc l'(d_j - cv[j]);  dL/dT = +w_r[i] + w_c[i] at (i, i),
 *   -w_r[i] at (i, ri[i]), -w_c[j] at (ci[j], j): at most 3B non-zeros, never built as a matrix.
 * B >= 2, 1 <= b, 0 <= col0, col0 + b <= B; no pointer may be NULL. Fixed-order sums, no atomics: a call repeated gives the same bits.
 * _slab_loss: partial[0] = sum over the slab's columns c, k = col0 + c, of l(T[k][c] - rv[k]) + l(T[k][c] - cv[c]) (the row terms of
 *       the anchors the slab owns, rv the GLOBAL row minima, + the column terms of its columns), un-normalised: the caller sums the
 *       ranks' partials and divides by 2B.
 * _pairs: the non-zeros of dL/dT that lie in the slab's columns, 2b + B entries laid out as witw_batch_hard_pairs lays them out:
 *       [0, b) the diagonal (col0 + j, j, +w_r[col0+j] + w_c[j]); [b, 2b) (ci[j], j, -w_c[j]); [2b, 2b + B) (i, ri[i] - col0, -w_r[i])
 *       when the slab holds column ri[i]. (-1, -1, 0) where it does not, or where the mined index is -1. pair_g = global row,
 *       pair_c = LOCAL column, pair_w includes grad_loss (device scalar); diag [B] = the global diagonal. */
int witw_baseline_hard_slab_loss(const float* T, const float* rv, const float* cv, int B, int b, int col0, int soft_margin, float alpha,
                                 float margin, float* partial, void* stream);
int witw_baseline_hard_pairs(const float* diag, const float* rv, const long long* ri, const float* cv, const long long* ci,
                             const float* grad_loss, int B, int b, int col0, int soft_margin, float alpha, float margin, int* pair_g,
                             int* pair_c, float* pair_w, void* stream);
/* Backward of T = witw_pairwise_sqdist(x [B,n], y [b,n]) for dL/dT given as a list of P >= 0 pairs (dL/dT[g][c] = the sum of pair_w
 * over the pairs (g, c); duplicates add up, an entry with g outside [0,B) or c outside [0,b) is skipped), any B, b >= 1,
 * 1 <= n <= 12288: a pair adds 2w (x_g - y_c) to dx[g] [B,n] and 2w (y_c - x_g) to dy[c] [b,n]. dx or dy may be NULL (not both);
 * every row of a non-NULL output is written, rows without a pair as zeros. A workgroup per output row and 256 columns scans the
 * list and sums its row's pairs in list order: no atomics, bitwise reproducible, and a row that is the partner of every pair is
 * one workgroup's P row reads. workspace: witw_sqdist_pairs_bwd_workspace_bytes(B, b, P) bytes (-1 for a bad shape; this form
 * needs none and answers 0, workspace may then be NULL). */
long long witw_sqdist_pairs_bwd_workspace_bytes(int B, int b, int P);
int witw_sqdist_pairs_bwd(const float* x, const float* y, const int* pair_g, const int* pair_c, const float* pair_w, int P, float* dx,
                          float* dy, int B, int b, int n, void* workspace, void* stream);

/* ---- data path: Resize (:100-134), ImageNormalization (:137-149; semantic: cvig_semantic.py:167-176),
 *      PolarTransform (:156-209). NCHW fp32. mean/stdv: HOST arrays of C floats (NULL = resize only). */
int witw_resize_bilinear_normalize(const float* x, float* y, int B, int C, int Hi, int Wi, int Ho, int Wo,
                                   const float* mean, const float* stdv, int n_div255, void* stream);
/* Resize (+ normalise) a batch of images of INDIVIDUAL sizes in one launch (the DataLoader hands over raw images of any size,
 * model/cvig_fov.py:393-403). desc: DEVICE array [B][5] of 64-bit words {device address of image b, H, W, start column, channels
 * stored per pixel}; kind 0 = float32 planar CHW sources, 1 = uint8 interleaved HWC (decoder output). y [B,C,Ho,Wo] = the image
 * resized to Ho x Wfull, columns start .. start+Wo-1 (mod Wfull) kept: the panorama crop of Resize (:118-128); Wfull == Wo and
 * start == 0 give the plain resize. Same arithmetic as witw_resize_bilinear_normalize. */
int witw_resize_bilinear_normalize_batched(const void* desc, float* y, int B, int C, int Ho, int Wo, int Wfull, int kind,
                                           const float* mean, const float* stdv, int n_div255, void* stream);
int witw_normalize(const float* x, float* y, int B, int C, int H, int W, const float* mean, const float* stdv, int n_div255,
                   void* stream);
/* taps: int32 [Ho*Wo][4] flat offsets into a size*size plane; wts: fp32 [Ho*Wo][4]; both DEVICE tables
 * built on the host in fp64 exactly as model/cvig_fov.py:163-181,197-201. */
int witw_polar_transform(const float* x, const int* taps, const float* wts, float* y, int B, int C, int size, int Ho, int Wo,
                         void* stream);
/* Overhead side of Compose[Resize, ImageNormalization, PolarTransform] (model/cvig_fov.py:393-397, classes :100-209) in ONE
 * launch: raw image -> bilinear size x size value -> (x/255 - mean)/std -> 4-tap polar gather -> y [B,C,Ho,Wo]; the size x size
 * image is never written; bit-identical to witw_resize_bilinear_normalize(_batched) followed by witw_polar_transform.
 * desc == NULL: src = fp32 [B,C,Hi,Wi]; else desc = the DEVICE table of witw_resize_bilinear_normalize_batched (kind 0 fp32
 * CHW, 1 uint8 HWC). wts: the weights of witw_polar_transform's table; taps: its taps as offsets (row * box width + column)
 * inside their tile's box. tiles: DEVICE int32 [n_tile][8] = {box x0, y0, width,
 * height, first output row, first output column, rows, columns}: a partition of the Ho x Wo outputs into tiles of at most 256
 * outputs, each with the bounding box (in the size x size plane) of all taps it reads, box width and height <= 64;
 * max_box = the largest box width*height (-1 otherwise: use the separate launches). */
int witw_polar_from_raw(const void* src, const void* desc, int kind, float* y, int B, int C, int Hi, int Wi, int size, int Ho,
                        int Wo, const int* taps, const float* wts, const int* tiles, int n_tile, int max_box, const float* mean,
                        const float* stdv, int n_div255, void* stream);
/* bilinear_interpolate (model/cvig_fov.py:156-183) on arbitrary coordinates: the same 4-tap gather with a caller-built
 * table; taps = flat offsets into a plane of plane_in elements, n_out samples per plane: y [B,C,n_out]. */
int witw_bilinear_gather(const float* x, const int* taps, const float* wts, float* y, int B, int C, long long plane_in,
                         long long n_out, void* stream);
/* SyncedRotation's overhead rotation (model/cvig_baseline.py:142: torchvision.transforms.functional.rotate on a float
 * CHW tensor = nearest-neighbour affine grid sample, zero fill, same size). x,y [B,C,H,W] fp32, y != x; theta DEVICE
 * fp32 [B][3][2]: per image the inverse rotation matrix divided by (W/2, H/2), row k = (x, y, 1) coefficient. */
int witw_rotate_nearest(const float* x, const float* theta, float* y, int B, int C, int H, int W, void* stream);
/* cvig_baseline's Compose[SyncedRotation, SurfaceResize] (model/cvig_baseline.py:324-328) for a BATCH straight from the decoder's
 * bytes, one launch per side. desc: the DEVICE table of witw_resize_bilinear_normalize_batched ([B][5] 64-bit words {address, H,
 * W, start, channels stored per pixel}; kind 0 = float32 planar CHW, 1 = uint8 interleaved HWC; the first C stored channels
 * are used, 1 <= C <= 8). y: fp32 [B,C,.,.] NCHW, values 0..255. A table row that does not fit the launch (see below) gives a
 * zero image; no row is read outside its own H x W x channels.
 * witw_baseline_rotate_batched: witw_rotate_nearest of every image (all H x W, theta as there: DEVICE fp32 [B][3][2]), bit for
 * bit what witw_rotate_nearest gives on the image converted to float CHW. y [B,C,H,W]. A row fits when its H, W are the launch's.
 * witw_baseline_roll_rows_batched: y[b][c][oy][ox] = image_b[c][oy / rep][(ox + start_b) mod W_b], y [B,C,Ho,Wo]: the left roll
 * of horizontal_shift (:97-113) and, at rep = 2, SurfaceResize('cvusa')'s repeat_interleave(2, -2) (:214) in one exact copy.
 * Ho must be a multiple of rep; a row fits when H_b == Ho / rep, W_b == Wo and 0 <= start_b < W_b. */
int witw_baseline_rotate_batched(const void* desc, const float* theta, float* y, int B, int C, int H, int W, int kind, void* stream);
int witw_baseline_roll_rows_batched(const void* desc, float* y, int B, int C, int Ho, int Wo, int rep, int kind, void* stream);

/* Conv2d(k=4, s=2) filter [co][ci][4][4] <-> the 3x3 filter over space-to-depth(2) channels [co][cpad][3][3] the taps4 kernels take
 * (model/cvig_baseline.py:236-252; tap row 0 / column 0 zero, channel (dy*2+dx)*ci + c); the second call is the inverse gather for
 * weight gradients. */
int witw_conv4x4_to_k3(const float* w, float* k3, int co, int ci, int cpad, void* stream);
int witw_k3_to_conv4x4(const float* k3, float* w, int co, int ci, int cpad, void* stream);

/* ---- JPEG back end on the device: what libjpeg does behind entropy decoding for the images the reference reads
 *      (skimage.io.imread -> PIL -> libjpeg-turbo, model/cvig_fov.py:88-89, in the DataLoader workers of :402). The entropy
 *      decoding stays on the host (witw_amd/csrc_host/jpeg_coef.cpp -> libwitw_jpeg.so: witw_jpeg_info, witw_jpeg_decode_coef;
 *      their _ex forms take progressive files too, all scans decoded into the same coefficient blocks, and -- flag bit 1, also on
 *      witw_jpeg_entropy_plan_ex -- 4:4:0 files: luma 1x2, an MCU of Y (top), Y (bottom), Cb, Cr).
 *      Byte-identical to Pillow's decode (JDCT_ISLOW, fancy upsampling).
 * witw_jpeg_idct: dequantisation + 'islow' integer inverse DCT. coef: DEVICE int16 [total_blocks][64] natural order; qt: DEVICE
 * uint16 [tables][64]; planes: DEVICE int64 [n_planes][6] = {first block, table index, byte offset of the output plane, blocks
 * wide, blocks high, blocks of all earlier planes}; out: the 8-bit component planes (bh*8 rows of bw*8 bytes). */
int witw_jpeg_idct(const void* coef, const void* qt, const void* planes, int n_planes, long long total_blocks, void* out, void* stream);
/* witw_jpeg_to_rgb: fancy chroma upsampling + YCbCr -> RGB. planes: the output above; images: DEVICE int64 [n_images][12] =
 * {H, W, components (1 | 3), mode (0 none, 1 h2v1, 2 h2v2 fancy, 3 / 4 the same replicated: chroma planes of <= 2 columns,
 * 5 h1v2 fancy (4:4:0: chroma at full width, half height; (3 nearest row + next nearest + {1 upper | 2 lower}) >> 2, edge rows repeated, planes of any size)), luma offset, luma stride, Cb offset, Cr offset, chroma stride, chroma
 * rows, chroma columns (real samples), output offset}; out: H x W x components interleaved bytes per image. */
int witw_jpeg_to_rgb(const void* planes, const void* images, int n_images, long long max_pixels, void* out, void* stream);
/* Entropy decoding ON THE DEVICE for files that carry restart markers (the reference decodes in its loader workers,
 * model/cvig_fov.py:88-89, :402): one GPU thread per restart interval. files: DEVICE int64 [n_files][4] = {address of the file bytes
 * (8-byte aligned, 24 readable bytes behind the end), address of the file's plan (host side: witw_jpeg_entropy_plan in
 * libwitw_jpeg.so -- header fields, Huffman tables, byte offset of every interval; a byte scan, no Huffman decoding; its layout, and that
 * of the info ints of witw_jpeg_info, is defined in witw_amd/csrc/jpeg_layout.h and nowhere else), address of the
 * file's coefficient area int16 [blocks][64] (zero-filled by the caller), file length}; the MCU geometry (blocks per MCU and where each
 * lies in its component's grid: 4:4:4, 4:2:2, 4:2:0, grey, and 4:4:0 = Y, Y below it, Cb, Cr) comes from the plan's per-component
 * (h, v); max_intervals: the largest interval count of a
 * file of the launch (grid sizing: one workgroup per 256 intervals of a file); errors: DEVICE int32 [n_files], zeroed by the
 * caller, 1 where a file's entropy-coded data is damaged, 2 for a bad plan. Coefficients bit-identical to the host decoder's
 * (witw_jpeg_decode_coef); witw_jpeg_idct / witw_jpeg_to_rgb take it from there. */
int witw_jpeg_huffman(const void* files, int n_files, int max_intervals, int* errors, void* stream);
/* The same for files WITHOUT restart markers (their plan holds ONE interval: the whole scan): a self-synchronising decode, one
 * workgroup of 512 threads per file (WITW_SELFSYNC_THREADS = 256 | 512 | 1024) -- the scan is unstuffed and cut into as many subsequences, every thread decodes its own from a
 * guessed state, then from its neighbour's exit state, round after round until no entry state changes (Huffman codes fall into step
 * after a few dozen symbols; thread 0 starts at the true state, so the fixed point is the true decoding); a prefix sum numbers the
 * blocks, a last pass writes the coefficients and a per-component prefix sum turns DC differences into DC values. files: DEVICE int64
 * [n_files][6] = {file bytes, plan, coefficient area (zero-filled), file length, scratch of file length + 32 bytes (8-byte aligned),
 * 0}; errors as above: 1 where the block count does not come out or where the writing pass meets, inside a block of the image, an
 * invalid code, a run past coefficient 63 or a symbol that reads behind the data. Coefficients bit-identical to the host decoder's. */
int witw_jpeg_huffman_selfsync(const void* files, int n_files, int* errors, void* stream);
/* The same with the threads per file chosen by the caller (256, 512 or 1024; jpeg.decode_packed_multi: 1024 when the launch holds a file
 * of 48 KB or more, else 512 -- larger files gain from shorter subsequences, smaller ones lose to the extra rounds). */
int witw_jpeg_huffman_selfsync_threads(const void* files, int n_files, int threads, int* errors, void* stream);
/* The scans of PROGRESSIVE files on the device (opt-in: jpeg.PROGRESSIVE_DEVICE; off, such files are Huffman-decoded by the loader
 * worker or left to Pillow as before): ONE STAGE of every file of the launch. A scan depends on exactly the earlier scans that coded
 * the same (component, coefficient) cells; the host's scan plan (witw_jpeg_scan_plan_ex in libwitw_jpeg.so: a byte scan, every check
 * that needs no Huffman decoding; layout 'JPW2' in witw_amd/csrc/jpeg_layout.h) gives each scan its stage = 0 where no earlier scan
 * coded one of its cells, else 1 + the largest stage among those that did (at most 14 stages; libjpeg's usual ten scans: three). The
 * caller launches stage 0, 1, ... up to the largest stage of the batch ON ONE STREAM: the order of the launches is the only
 * synchronisation between stages. files: DEVICE int64 [n_files][4] as witw_jpeg_huffman takes them = {file bytes (8-byte aligned, 24
 * readable bytes behind the end), scan plan (4-byte aligned), coefficient area int16 [blocks][64], zero-filled by the caller BEFORE
 * stage 0 and left alone between the stages, file length}; max_scans (1..64) / max_segments: the largest scan count of a file and
 * the largest segment count (restart intervals) of a scan in the launch -- grid sizing: a workgroup per (file, scan slot, 128
 * segments); a workgroup whose scan is of another stage, or past the file's last, leaves at once. One thread decodes one segment
 * (a file without restart markers: one thread per scan), coefficients are read and written as 16-bit cells only. errors: DEVICE int32
 * [n_files], zeroed by the caller before stage 0: 1 where the entropy-coded data of a scan is damaged (an invalid code, a DC size
 * above 15, a run past Se, a refinement symbol of size other than 1, bits taken from behind a segment's data: what
 * witw_jpeg_decode_coef_ex refuses with -3), 2 for a plan without the magic or with a scan record that cannot be walked. Every loop
 * bound and block index comes from the plan and is held under the plan's block count; nothing read from the entropy-coded data
 * indexes memory unchecked. After the last stage an unflagged file holds the coefficients witw_jpeg_decode_coef_ex writes, bit for
 * bit. Measured (profiles/jpeg_progressive_device.json): 128 files of 512 x 512 without restart markers, three stages,
 * 166 ms of device time against 1.16 ms for witw_jpeg_huffman_selfsync_threads on their sequential twins -- one thread walks a whole
 * scan; end to end slower than decoding the scans in the loader workers, hence opt-in. Files with restart markers were not measured. */
int witw_jpeg_progressive_stage(const void* files, int n_files, int stage, int max_scans, int max_segments, int* errors, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WITW_HIP_H */
