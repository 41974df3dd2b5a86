// The body of the spectral match kernel (see match_dft.hip, which includes this file once per kernel). The includer defines
//   WITW_DFT_KERNEL   the kernel's name
//   WITW_DFT_TPARAMS  its template parameters
//   WITW_DFT_CONSTS   the instantiation constants it does not take as template parameters
// so that match_dft_kernel<REC, GAP, VONLY> is compiled from the text it was compiled from before the shift masks existed (its
// gfx950 listing is the same instruction for instruction) and match_dft_masked_kernel<GAP, VONLY> from the same text with MASKED = true.
template <WITW_DFT_TPARAMS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void WITW_DFT_KERNEL(DftArgs p) {
    WITW_DFT_CONSTS
    __shared__ __attribute__((aligned(1024))) float smem[LDS_F];      // the read addresses XOR bits 4-7: stage bases stay 1 KB-aligned
    __shared__ float dt_s[NSLOT * 64];      // inverse-transform coefficients
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hk = lane >> 5;
    const int team = wave >> 1, par = wave & 1;

    // Persistent workgroups (one per CU: the LDS admits one anyway): workgroup b ranks tiles b, b + gridDim.x, ... Tile numbering
    // in 16 x 16 windows: consecutive tiles walk 16 overhead tiles of one surface tile, then the next surface tile, so the
    // resident workgroups share 16 + 16 tile spectra per slot (L2-resident while the slots advance together).
    const unsigned n_tiles = (unsigned)p.nbx * (unsigned)p.nby;      // < 2^31 (checked by the launcher): 32-bit tile arithmetic
    auto tile_origin = [&](unsigned tile, int& s0_, int& o0_) {
        const unsigned per_group = 16u * (unsigned)p.nbx;
        const int g = (int)(tile / per_group), within = (int)(tile - (unsigned)g * per_group);
        const int rows = min(16, p.nby - 16 * g);
        o0_ = (16 * g + within % rows) * 32;
        s0_ = (within / rows) * 32;
    };

    // ---- staging: LDS-DMA, 16 B per lane: one instruction brings two whole rows (lanes 0-31 row 2n, lanes 32-63 row 2n+1)
    // with no register transit and no ds_write; a lane fetches the 16-byte slot that belongs at its LDS position under the
    // swizzle. Wave w owns the rows of one kind: w&1 = slot parity, w>>1 = 0 surfaces / 1 overheads; 16 instructions per
    // step. Rows past the batch fall outside the descriptor (zeros); every slot a step reads exists (32 slots, 16 steps).
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int srp = wv & 1, is_ov = wv >> 1;
    const unsigned region = (is_ov ? A_F + srp * 32 * ROW_F : srp * 32 * ROW_F) * 4u;
    const unsigned lds0 = lds_address(smem);
    // lane -> (row 2n + hi, physical slot l32): logical slot = l32 ^ ((2n + hi) & 15) = (l32 ^ hi) ^ (2n & 15)
    const unsigned voff0 = (unsigned)hk * (SPEC * 4u) + (unsigned)(l31 ^ hk) * 16u;
    auto tile_rsrc = [&](int s0_, int o0_) {
        const int rows_here = is_ov ? min(32, p.Bo - o0_) : min(32, p.Bs - s0_);
        return raw_rsrc(is_ov ? p.spec_ov + (size_t)o0_ * SPEC : p.spec_su + (size_t)s0_ * SPEC, (unsigned)rows_here * SPEC * 4u);
    };
    i32x4 rs;
    auto dma_rows = [&](const i32x4& rs, int n, int step, int buf) {      // n = row pair, compile-time after unrolling
        const unsigned slot = (unsigned)(2 * step + srp);
        const unsigned soff = (unsigned)(2 * n) * (SPEC * 4u) + slot * 512u;
        const unsigned lds = lds0 + (unsigned)buf * (STAGE_F * 4u) + region + (unsigned)n * 1024u;
        dma16(rs, lds, voff0 ^ (unsigned)(((2 * n) & 15) << 4), soff);
    };

    // ---- operand roles. GEMM-1 row l31 = surface j, part (0: Re C, 1: Im C); row order j&3 + 4*part + 8*(j>>2)
    const int j = (l31 & 3) + 4 * (l31 >> 3), part = (l31 >> 2) & 1;
    //   K < 64 (lines x re of the overhead):  Re row reads P, Im row reads Q (sign below);  K >= 64 (x im): Re row reads Q, Im row reads P
    // byte offsets in a stage of k-group 0; k-group u is at offset ^ (u << 4) (the swizzle: slot u ^ (row & 15))
    // 8-byte chunk of a 16-byte slot: ds_read_b64 serves lanes 0-31 and 32-63 in one LDS cycle each when their 32 x 8 bytes fall on
    // 64 distinct banks. A surface's P and Q halves are 256 B apart (the same banks) and are read by the part-0 / part-1 lanes of
    // one instruction, so the surface spectra are STORED with the two chunks of every Q slot exchanged (match_spectrum_kernel,
    // role 0) and a lane reading Q takes chunk hk ^ 1: P readers sit on banks 4c+{0,1}, Q readers on 4c+{2,3}.
    // the odd wave takes the team's surfaces in the order j ^ 8: its accumulator r then belongs to surface r ^ 8, and in the
    // epilogue BOTH waves keep registers 0-7 (the E wave surfaces 0-7, the O wave 8-15) and send registers 8-15
    const int jr = j ^ (par << 3);
    const unsigned a_row = (unsigned)(par * 32 + team * 16 + jr) * 512u + ((unsigned)jr << 4);
    const unsigned a_off1 = a_row + (part ? 256u + 8u * (hk ^ 1) : 8u * hk);
    const unsigned a_off2 = a_row + (part ? 8u * hk : 256u + 8u * (hk ^ 1));
    // slot 0 (the even waves' first step) holds two REAL spectra, P = X_0 and Q = X_32: there the Im rows read what the Re rows
    // read, so that lanes 0-31 of the accumulators end up with C_0 + C_32 and lanes 32-63 (C = cb + sg * ca) with C_32 - C_0 --
    // the coefficient table of slot 0 turns them into (C_0 + (-1)^shift C_32) / 64
    const unsigned a_off1z = par ? a_off1 : a_row + 8u * hk;
    const unsigned a_off2z = par ? a_off2 : a_row + 256u + 8u * (hk ^ 1);
    // the Im rows' minus sign (K < 64: -Q) is applied once per step: ca collects K < 64, cb K >= 64, and accumulator register r
    // holds Re C in lanes 0-31 and Im C in lanes 32-63, so C = cb + sg * ca with sg = -1 in the upper half-wave
    const float sg = hk ? -1.f : 1.f;
    // overheads: one instruction reads one half of 32 different rows; rows r and r + 16 share the slot swizzle, so the spectra of
    // overheads with bit 4 of their index set are stored with the chunks of every slot exchanged (role 1) and read at hk ^ 1
    const unsigned b_off1 = (unsigned)(A_F + (par * 32 + l31) * ROW_F) * 4u + 8u * (hk ^ (l31 >> 4)) + ((unsigned)(l31 & 15) << 4);     // Q: + 256
    for (int t = tid; t < NSLOT * 64; t += 256) dt_s[t] = p.dtab[t];
    // (a global load of the step's coefficient would sit at the end of every step with its whole latency exposed: ~4.6k cycles per step)

    int s0, o0;
    tile_origin(blockIdx.x, s0, o0);
    rs = tile_rsrc(s0, o0);
#pragma unroll
    for (int n = 0; n < 16; ++n) dma_rows(rs, n, 0, 0);        // the first tile's first stage; a later one rides in the last step of the tile before it

    // the wave's 16 x 16 long-lived accumulation registers; zeroed here and again at the end of every epilogue (behind the norm
    // loads of the output phase, whose latency that hides)
    f32x16 acc2[16];
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc2[r][q] = 0.f;
    const int par_u = wv & 1;            // scalar copy of par: the epilogue's two roles are a uniform branch
    float fzero = 0.f;                   // (behind an empty asm: a register, not a folded constant)
    asm volatile("" : "+v"(fzero));

#if WITW_DFT_PHASES
    const unsigned long long ph_k0 = __builtin_amdgcn_s_memrealtime(), ph_c0 = __builtin_amdgcn_s_memtime();
    unsigned long long ph_s[2] = {0, 0}, ph_last = 0;      // [0] barrier -> end of the next GEMM 1 (GEMM 2 + GEMM 1), [1] the wait + barrier
    unsigned long long ph_steps = 0, ph_epi = 0, ph_t0 = 0, ph_t1 = 0, ph_e[6] = {0, 0, 0, 0, 0, 0}, ph_m[6];      // scalar: s_memrealtime sums over this workgroup's tiles
#endif
    int iter = 0;
#pragma clang loop unroll(disable)
    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, ++iter) {
    // the NEXT tile's origin and staging descriptor: its first stage is fetched by the staging DMA of this tile's last step (which
    // has no step of its own to fetch for) into stage 0, free by then -- before, a block of 16 DMA instructions per wave in the
    // epilogue (0.6 us per tile: outside the MFMAs' shadow a DMA instruction costs ~85 cycles of issue)
    int s0n = 0, o0n = 0;
    i32x4 rsn = raw_rsrc(p.spec_ov, 0u);      // no next tile: an empty descriptor (zeros)
    if (tile + gridDim.x < n_tiles) {
        tile_origin(tile + gridDim.x, s0n, o0n);
        rsn = tile_rsrc(s0n, o0n);
    }
    const bool rec = REC && p.stamps && blockIdx.x < 4 && iter == 1 && tid == 0;      // a steady-state tile of the first workgroups
    auto stamp = [&](int k) { if (rec) p.stamps[blockIdx.x * 64 + k] = __builtin_amdgcn_s_memrealtime(); };
    stamp(0);
#if WITW_DFT_PHASES
    ph_t0 = __builtin_amdgcn_s_memrealtime();
    ph_last = ph_t0;
#endif
    // vmcnt(0), said with the builtin: the staging DMA of the first stage has landed, AND the compiler's own counter bookkeeping
    // enters the step loop clean. As asm only, the norm loads of the previous tile's epilogue stayed "pending" for the compiler; in
    // the value-only instantiation their destination registers are the GEMM-1 accumulators, and it protected them with a
    // vmcnt(0) inside the step loop, right behind the first staging DMA of every step: 244 -> 256 ms on configuration 5
    __builtin_amdgcn_s_waitcnt(0x0F70);
    asm volatile("" ::: "memory");
    __syncthreads();
    stamp(1);

    // step i: 64 GEMM-1 MFMAs with the 16 DMA instructions of step i+1's rows issued two per MFMA group in the first 8 groups into
    // the other stage (free since the barrier of step i-1), barrier, then the 16 GEMM-2 MFMAs of step i behind the first operand
    // reads and the coefficient read of step i+1: the barrier sits BETWEEN the two GEMMs, so GEMM 2 (registers only) hides the LDS
    // latency of the next step's first reads and the drain of the last GEMM-1 MFMAs overlaps the barrier wait (round 5; before,
    // every step began with a barrier followed by the address arithmetic and the exposed latency of its first reads).
    // Operands as ds_read_b64: a lane holds k = 4u + 2hk and 4u + 2hk + 1 of its row, i.e. MFMA step 2u + e covers k = 4u + e
    // (lanes 0-31) and 4u + 2 + e (lanes 32-63) -- the same K permutation on both operands. Reads run two groups ahead; the
    // compiler would fuse neighbours into ds_read2_b64 (banked like ds_read_b32), hence the asm.
    constexpr int NQ = 3;      // register slots of the operand ring: reads run two k-groups ahead of the MFMAs (three: no gain)
    f32x2 qa1[NQ], qb1[NQ], qa2[NQ], qb2[NQ];
    unsigned xa1, xb1, xa2;
    const unsigned dt0 = lds_address(dt_s) + (unsigned)(par * 64 + lane) * 4u;      // + step * 512
    // read addresses of the 16 k-groups: base ^ (U << 4) (the slot swizzle), 48 registers that live across the step. They are
    // formed between the GEMM-2 MFMAs of the previous step (groups 0 and 1 at the step head): inside the groups the compiler
    // forms each address in the register the read is about to overwrite, which an MFMA in flight still names as its operand,
    // and the step ran 7 % slower (measured, same box).
    unsigned XA[16], XB[16], XC[16];
#define WITW_DFT_FETCH(U)                                              \
        {                                                              \
            qa1[(U) % NQ] = lds_read64<0>(XA[U]);                       \
            qb1[(U) % NQ] = lds_read64<0>(XB[U]);                       \
            qa2[(U) % NQ] = lds_read64<0>(XC[U]);                       \
            qb2[(U) % NQ] = lds_read64<256>(XB[U]);                     \
        }
#define WITW_DFT_ADDR(U)                                               \
        {                                                              \
            XA[U] = lds_xor<((U) << 4)>(xa1);                          \
            XB[U] = lds_xor<((U) << 4)>(xb1);                          \
            XC[U] = lds_xor<((U) << 4)>(xa2);                          \
        }
#define WITW_DFT_STEP_HEAD(STEP, SLOT0)                                \
        {                                                              \
            const unsigned sb = lds0 + (unsigned)((STEP) & 1) * (STAGE_F * 4u) + tile_zero; \
            xa1 = sb + ((SLOT0) ? a_off1z : a_off1); xb1 = sb + b_off1; xa2 = sb + ((SLOT0) ? a_off2z : a_off2); \
            WITW_DFT_ADDR(0)                                           \
            WITW_DFT_ADDR(1)                                           \
            WITW_DFT_FETCH(0)                                          \
            WITW_DFT_FETCH(1)                                          \
        }
    // tile_zero = 0 behind an empty asm: the 48 step-0 addresses below are the same for every tile, and the compiler would hoist
    // them out of the tile loop and keep them across the epilogue (42 registers; the GAP instantiation then spilled 59, reloaded
    // them behind the tile-top barrier and waited for the reloads -- i.e. for the staging DMA -- inside the step loop)
    unsigned tile_zero = 0;
    asm volatile("" : "+v"(tile_zero));
    WITW_DFT_STEP_HEAD(0, true)
#pragma unroll
    for (int u = 2; u < 16; ++u) {      // (again for every tile: 42 instructions, and the 48 registers are free during the epilogue)
        XA[u] = xa1 ^ (unsigned)(u << 4);
        XB[u] = xb1 ^ (unsigned)(u << 4);
        XC[u] = xa2 ^ (unsigned)(u << 4);
    }
#pragma clang loop unroll(disable)
    for (int i = 0; i < NSTEP; ++i) {
        const int bufn = (i + 1) & 1;
        const bool last_step = i + 1 == NSTEP;
        const int inext = last_step ? 0 : i + 1;      // the last step stages step 0 of the next tile
        i32x4 rsd;
#pragma unroll
        for (int e = 0; e < 4; ++e) rsd[e] = last_step ? rsn[e] : rs[e];
        f32x16 ca, cb;      // the first MFMA of each chain starts from C = 0
        float dval;
#define WITW_DFT_GROUP(U)                                                                                                      \
        {                                                                                                                      \
            constexpr int d = (U) % NQ;                                                                                        \
            constexpr int AH = 2;                                                                                              \
            if ((U) + AH < 16 && !(WITW_DFT_DIAG & 4)) WITW_DFT_FETCH((U) + AH < 16 ? (U) + AH : 0)                            \
            if ((U) + AH < 16) lds_wait<4 * AH>(qa1[d], qb1[d], qa2[d], qb2[d]);                                               \
            else if ((U) + 1 < 16) lds_wait<4 * (15 - (U) < AH ? 15 - (U) : AH)>(qa1[d], qb1[d], qa2[d], qb2[d]);              \
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(qa1[d]), "+v"(qb1[d]), "+v"(qa2[d]), "+v"(qb2[d]), "+v"(dval));     \
            if ((U) == 14) dval = lds_read32(dt0 + (unsigned)i * 512u);      /* the step's coefficient: waited for by group 15 */ \
            if ((U) == 0) mfma_v0(ca, qa1[d][0], qb1[d][0]); else mfma_v(ca, qa1[d][0], qb1[d][0]);                            \
            if (!(WITW_DFT_DIAG & 1) && (U) < 8) dma_rows(rsd, 2 * (U), inext, bufn);                                               \
            if ((U) == 0) mfma_v0(cb, qa2[d][0], qb2[d][0]); else mfma_v(cb, qa2[d][0], qb2[d][0]);                            \
            if (!(WITW_DFT_DIAG & 1) && (U) < 8) dma_rows(rsd, 2 * (U) + 1, inext, bufn);                                           \
            mfma_v(ca, qa1[d][1], qb1[d][1]);                                                                                  \
            mfma_v(cb, qa2[d][1], qb2[d][1]);                                                                                  \
        }
        WITW_DFT_GROUP(0) WITW_DFT_GROUP(1) WITW_DFT_GROUP(2) WITW_DFT_GROUP(3)
        WITW_DFT_GROUP(4) WITW_DFT_GROUP(5) WITW_DFT_GROUP(6) WITW_DFT_GROUP(7)
        WITW_DFT_GROUP(8) WITW_DFT_GROUP(9) WITW_DFT_GROUP(10) WITW_DFT_GROUP(11)
        WITW_DFT_GROUP(12) WITW_DFT_GROUP(13) WITW_DFT_GROUP(14) WITW_DFT_GROUP(15)
#undef WITW_DFT_GROUP
        stamp(2 + 3 * i);
#if WITW_DFT_PHASES
        const unsigned long long pa = __builtin_amdgcn_s_memrealtime();
#endif
        if (!(WITW_DFT_DIAG & 2)) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
#if WITW_DFT_PHASES
        const unsigned long long pb = __builtin_amdgcn_s_memrealtime();
        ph_s[0] += pa - ph_last; ph_s[1] += pb - pa; ph_last = pb;
#endif
        stamp(3 + 3 * i);
        if (i + 1 < NSTEP) WITW_DFT_STEP_HEAD(i + 1, false)
        mfma_settle(ca, cb);
        // C = cb + sg * ca into 16 DIFFERENT registers before the first GEMM-2 MFMA: left to the compiler every product went through
        // one register, and a VALU write to a register that the MFMA in flight names as its operand waits for that MFMA -- each
        // of the 16 GEMM-2 MFMAs then cost ~90 cycles instead of 64 (the same effect as the address registers above)
        float cc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) cc[r] = fmaf(ca[r], sg, cb[r]);
        asm volatile("" : "+v"(cc[0]), "+v"(cc[1]), "+v"(cc[2]), "+v"(cc[3]), "+v"(cc[4]), "+v"(cc[5]), "+v"(cc[6]), "+v"(cc[7]),
                          "+v"(cc[8]), "+v"(cc[9]), "+v"(cc[10]), "+v"(cc[11]), "+v"(cc[12]), "+v"(cc[13]), "+v"(cc[14]), "+v"(cc[15]));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc2[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(dval, cc[r], acc2[r], 0, 0, 0);      // [shift][overhead]
            if (r >= 2) {      // the next step's read addresses, in the shadow of this MFMA (groups 0 and 1: at the step head)
                XA[r] = xa1 ^ (unsigned)(r << 4);
                XB[r] = xb1 ^ (unsigned)(r << 4);
                XC[r] = xa2 ^ (unsigned)(r << 4);
            }
        }
        // the 16 operand registers stay live up to here: otherwise the address registers above are allocated on top of them. The
        // last accumulator is named as well: it ties this statement behind the last MFMA (an empty asm may move above the builtins)
        asm volatile("" : "+a"(acc2[15]) : "v"(cc[0]), "v"(cc[1]), "v"(cc[2]), "v"(cc[3]), "v"(cc[4]), "v"(cc[5]), "v"(cc[6]), "v"(cc[7]),
                           "v"(cc[8]), "v"(cc[9]), "v"(cc[10]), "v"(cc[11]), "v"(cc[12]), "v"(cc[13]), "v"(cc[14]), "v"(cc[15]), "v"(dval));
        stamp(4 + 3 * i);
    }
#undef WITW_DFT_STEP_HEAD
#undef WITW_DFT_FETCH
#undef WITW_DFT_ADDR

#if WITW_DFT_PHASES
    ph_t1 = __builtin_amdgcn_s_memrealtime();
    ph_steps += ph_t1 - ph_t0;
#endif
    // ---- the epilogue runs in the area of stage 1; stage 0 already holds the next tile's first stage (fetched by the last step)
    const int s0c = s0, o0c = o0;
    s0 = s0n; o0 = o0n; rs = rsn;      // the tile whose first stage is on its way
    if (WITW_DFT_DIAG & 8) {
        float t = 0.f;      // every accumulator stays live
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int q = 0; q < 16; ++q) t += acc2[r][q];
        if (t == 12345.f && p.score) p.score[tile] = t;
        continue;
    }
    // ---- epilogue. acc2[r][q] of lane (l31, hk) = E (even wave) or O (odd wave) of surface r of the team, overhead l31, shift
    // (q & 3) + 8 (q >> 2) + 4 hk (the odd wave: surface r ^ 8). Two rounds h: a wave sends registers 8 + 4h .. +3 (the partner's
    // surfaces) and receives the partner's tiles of its own surfaces, registers 4h .. +3; LDS [wave][surface of the round][register quad][lane] x 16 B (conflict-free both ways).
    float* xw = smem + STAGE_F + wv * 4096 + lane * 4;
    const float* xr = smem + STAGE_F + (wv ^ 1) * 4096 + lane * 4;
    float rv[8], rs[8];
    int rk[8];
    // value-only: the norms of the output phase depend on no result (window norm of shift 0) -- loaded here, a whole epilogue ahead
    float wn_e = 1.f, sn_e[4] = {1.f, 1.f, 1.f, 1.f};
    if (VONLY && p.distance) {
        const int og = o0c + l31;
        if (og < p.Bo) wn_e = p.wn[(size_t)og * 64];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int s = s0c + team * 16 + par * 8 + 4 * hk + jj;
            if (s < p.Bs) sn_e[jj] = p.sn[s];
        }
    }
    // MASKED: result 4h + rr of this wave belongs to surface s0c + team * 16 + par * 8 + 4h + rr -- wave-uniform, so the eight
    // mask words live in scalar registers: lanes 0-7 load one word each (0 = no prior and the surfaces past Bs of a ragged tile:
    // all ones), v_readlane spreads them
    int mlo[8], mhi[8];
    if (MASKED) {
        const int sm = s0c + (wv >> 1) * 16 + par_u * 8 + (lane & 7);
        unsigned long long mw = sm < p.Bs ? p.mask[sm] : 0ull;
        if (mw == 0ull) mw = ~0ull;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            mlo[e] = __builtin_amdgcn_readlane((int)(unsigned)mw, e);
            mhi[e] = __builtin_amdgcn_readlane((int)(unsigned)(mw >> 32), e);
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                const f32x4 t = {acc2[8 + 4 * h + rr][4 * qq], acc2[8 + 4 * h + rr][4 * qq + 1], acc2[8 + 4 * h + rr][4 * qq + 2], acc2[8 + 4 * h + rr][4 * qq + 3]};
                *reinterpret_cast<f32x4*>(xw + (rr * 4 + qq) * 256) = t;
            }
        // the sent registers are zeroed for the next tile here, in front of the barrier wait
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) mfma_zero(acc2[8 + 4 * h + rr], fzero);
        __syncthreads();
#if WITW_DFT_PHASES
        asm volatile("" ::: "memory");
        ph_m[2 * h] = __builtin_amdgcn_s_memrealtime();
#endif
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            f32x16 got;
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(xr + (rr * 4 + qq) * 256);
                got[4 * qq] = t[0]; got[4 * qq + 1] = t[1]; got[4 * qq + 2] = t[2]; got[4 * qq + 3] = t[3];
            }
            float v, s2 = 0.f;
            unsigned k;
            if (MASKED) {
                const unsigned lo = (unsigned)mlo[4 * h + rr] >> (4 * hk), hi = (unsigned)mhi[4 * h + rr] >> (4 * hk);
                if (par_u == 0) scan16_masked<GAP, VONLY>(acc2[4 * h + rr], got, lo, hi, v, k, s2);
                else scan16_masked<GAP, VONLY>(got, acc2[4 * h + rr], lo, hi, v, k, s2);
            }
            else if (par_u == 0) scan16<GAP, VONLY>(acc2[4 * h + rr], got, v, k, s2);      // kept: E, received: O
            else scan16<GAP, VONLY>(got, acc2[4 * h + rr], v, k, s2);
            // the other 16 shifts of the pair sit in lane ^ 32 (4 further on for the upper half-wave)
            float v0, v1;
            unsigned kl, ku0;
            half_swap(v, v0, v1);
            const float vc = fmaxf(v0, v1);
            int kc = 0;
            if (!VONLY) {
                half_swap(k, kl, ku0);
                const unsigned ku = ku0 == NOKEY ? NOKEY : ku0 + 4u;
                const unsigned kb = umin(v0 == vc ? kl : NOKEY, v1 == vc ? ku : NOKEY);
                kc = kb == NOKEY ? 0 : (int)((kb & 63u) + ((kb >> 31) << 5));      // no finite maximum (NaN scores): index 0
                // MASKED: ... the lowest allowed shift (scalar), so that every orientation written is one the word allows
                if (MASKED && kb == NOKEY) kc = mlo[4 * h + rr] ? __builtin_ctz((unsigned)mlo[4 * h + rr]) : 32 + __builtin_ctz((unsigned)mhi[4 * h + rr]);
            }
            rv[4 * h + rr] = vc;
            rk[4 * h + rr] = kc;
            if (GAP) {
                float s0, s1;
                half_swap(s2, s0, s1);
                rs[4 * h + rr] = fmaxf(fmaxf(s0, s1), fminf(v0, v1));
            }
        }
#if WITW_DFT_PHASES
        asm volatile("" :: "v"(rv[4 * h]), "v"(rv[4 * h + 1]), "v"(rv[4 * h + 2]), "v"(rv[4 * h + 3]), "v"(rk[4 * h + 3]) : "memory");
        ph_m[2 * h + 1] = __builtin_amdgcn_s_memrealtime();
#endif
        // this round's kept accumulators are dead: back to zero on the matrix pipe while the vector pipe goes on
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) mfma_zero(acc2[4 * h + rr], fzero);
        if (GAP) {
            // this instantiation sits at the register limit: a round's four results are written at once (two surfaces per
            // half-wave) instead of being carried to the end of the epilogue
            const int og = o0c + l31;
#pragma unroll
            for (int j2 = 0; j2 < 2; ++j2) {
                const float v = hk ? rv[4 * h + 2 + j2] : rv[4 * h + j2];
                const int kx = hk ? rk[4 * h + 2 + j2] : rk[4 * h + j2];
                const float g = hk ? rs[4 * h + 2 + j2] : rs[4 * h + j2];
                const int s = s0c + team * 16 + par * 8 + 4 * h + 2 * hk + j2;
                if (s < p.Bs && og < p.Bo) {
                    const size_t off = (size_t)og * p.Bs + s;
                    if (p.orientation) p.orientation[off] = kx;
                    if (p.score) p.score[off] = v;
                    if (p.distance) p.distance[off] = 2.f * (1.f - v / (p.wn[(size_t)og * 64 + kx] * p.sn[s]));
                    if (p.gap) p.gap[off] = v - g;
                }
            }
        }
        if (h == 0) __syncthreads();      // the partner has read round 0 before round 1 overwrites it
    }
    // ---- output: both half-waves hold the 8 results of overhead l31; the lower one writes surfaces 0-3, the upper one 4-7. The
    // window-norm loads are issued first, the accumulators are zeroed for the next tile behind them
    if (!GAP) {
        const int og = o0c + l31;
        float wnv[4], snv[4], vv[4];
        int kk[4];
        bool ok[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            vv[jj] = hk ? rv[4 + jj] : rv[jj];
            kk[jj] = hk ? rk[4 + jj] : rk[jj];
            const int s = s0c + team * 16 + par * 8 + 4 * hk + jj;
            ok[jj] = s < p.Bs && og < p.Bo;
            wnv[jj] = VONLY ? wn_e : (ok[jj] && p.distance) ? p.wn[(size_t)og * 64 + kk[jj]] : 1.f;
            snv[jj] = VONLY ? sn_e[jj] : (ok[jj] && p.distance) ? p.sn[s] : 1.f;
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int s = s0c + team * 16 + par * 8 + 4 * hk + jj;
            if (ok[jj]) {
                const size_t off = (size_t)og * p.Bs + s;
                if (p.orientation) p.orientation[off] = kk[jj];
                if (p.score) p.score[off] = vv[jj];
                if (p.distance) p.distance[off] = 2.f * (1.f - vv[jj] / (wnv[jj] * snv[jj]));
            }
        }
    }
    stamp(53);
#if WITW_DFT_PHASES
    asm volatile("" ::: "memory");
    {
        const unsigned long long te = __builtin_amdgcn_s_memrealtime();
        ph_epi += te - ph_t1;
        ph_e[0] += ph_m[0] - ph_t1; ph_e[1] += ph_m[1] - ph_m[0]; ph_e[2] += ph_m[2] - ph_m[1]; ph_e[3] += ph_m[3] - ph_m[2]; ph_e[4] += te - ph_m[3];
    }
#endif
    }   // tiles
#if WITW_DFT_PHASES
    if (p.stamps && blockIdx.x < 4 && tid == 0) {
        p.stamps[blockIdx.x * 64 + 0] = ph_steps;
        p.stamps[blockIdx.x * 64 + 1] = ph_epi;
        p.stamps[blockIdx.x * 64 + 2] = (unsigned long long)iter;
        for (int e = 0; e < 5; ++e) p.stamps[blockIdx.x * 64 + 3 + e] = ph_e[e];
        p.stamps[blockIdx.x * 64 + 10] = __builtin_amdgcn_s_memrealtime() - ph_k0;
        p.stamps[blockIdx.x * 64 + 11] = __builtin_amdgcn_s_memtime() - ph_c0;
        p.stamps[blockIdx.x * 64 + 8] = ph_s[0];
        p.stamps[blockIdx.x * 64 + 9] = ph_s[1];
    }
#endif
}
