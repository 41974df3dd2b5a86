// Orientation search + chord distance through the row spectra (gfx950, fp32 MFMA): the retrieval form of the fused match
// (BASELINE config C5; model/cvig_fov.py:297-363, called at :547-549 for every (gallery row, query) pair).
//
// score[o,s,shift] = sum_{ch,k} ov[o,ch,(k+shift)%64] * su[s,ch,k] is a circular cross-correlation along the 64 columns, summed
// over the 64 (channel,row) lines. With X_f = sum_k x[k] e^{-2 pi i f k/64} per line (su zero-padded to 64 columns):
//   C_f[o,s]   = sum_ch OV_f[o,ch] * conj(SU_f[s,ch])                                  f = 0..32
//   score[o,s,shift] = (1/64) [ C_0 + (-1)^shift C_32 + 2 sum_{f=1..31} (Re C_f cos(2 pi f shift/64) - Im C_f sin(..)) ]
// 2*2*128*33 + 2*2*32*33 = 21k FLOP per pair instead of 2*64*4096 = 524k of the direct form (match.hip), both on the fp32 MFMA
// (the algorithmic count; the kernel runs 32 slots: the real spectra at f = 0 and f = 32 share one, see NSLOT).
//
// Kernel: persistent workgroups (one per CU), a tile = 32 surfaces x 32 overheads, 4 waves = 2 surface teams x {even, odd}
// frequencies. Per frequency slot
//   GEMM 1 (32x32x2 f32 MFMA, K = 128 = 64 lines x {re,im}): rows = 16 surfaces x {Re C, Im C}, columns = 32 overheads. Rows are
//          ordered so that accumulator register r of lanes 0-31 holds Re C[surface r] and of lanes 32-63 Im C[surface r] of the
//          same (surface, overhead): exactly the A operand (32 overheads x K=2) of
//   GEMM 2 (one 32x32x2 MFMA per surface and slot): [32 overheads x (Re,Im)] x [(cos,-sin) x 32 shifts], accumulated over the
//          slots into 16 x f32x16 registers per wave (all 256 accumulation registers of the wave).
//          Round 5: the coefficients are the A operand and C the B operand, so the accumulator holds [32 shifts x 32 overheads]:
//          a lane owns ONE overhead and 16 of the 32 shifts in its 16 registers (the other 16 sit in lane ^ 32).
// Even frequencies give E[shift], odd ones O[shift] for shift < 32; score[shift] = E + O, score[shift+32] = E - O. The two
// waves of a team exchange HALF of their tiles register for register through LDS (the E wave finishes surfaces 0-7 of the
// team, the O wave 8-15: 16-byte writes and reads, no transposition), every lane scans its 16 shifts x {+, -} of a pair in
// registers, joins the other half-wave's result (first maximum wins, as torch.argmax) and writes
// orientation / score / distance like match.hip does.
#include "common.h"
#include "spectrum64_gen.h"

// WITW_DFT_DIAG (diagnostic builds, wrong results): 1 = no staging DMA inside the steps, 2 = no barrier / vmcnt wait per step,
// 4 = no operand reads inside the groups, 8 = the tile loop ends before the epilogue
#ifndef WITW_DFT_DIAG
#define WITW_DFT_DIAG 0
#endif
// WITW_DFT_PHASES=1 (diagnostic build): with WITW_DFT_STAMPS=2 in the environment the product instantiation sums s_memrealtime
// over the step loops and over the epilogues of a workgroup's tiles; printed to stderr
#ifndef WITW_DFT_PHASES
#define WITW_DFT_PHASES 0
#endif
namespace {

// Storage slots of a spectrum, [P(64 lines) | Q(64 lines)] each: slot t = 1..31 holds (Re, Im) of frequency t; the spectra at
// frequencies 0 and 32 are real, and slot 0 holds BOTH: P = X_0, Q = X_32 (round 5: 33 -> 32 slots, 17 -> 16 steps per tile, and
// no phantom 34th slot whose reads -- a neighbour's values times a zero coefficient -- let a NaN embedding reach the row before it)
constexpr int NSLOT = 32;
constexpr int SPEC = NSLOT * 128;      // floats per embedding spectrum (16 KB)
constexpr int NSTEP = 16;              // step i: even waves slot 2i, odd waves slot 2i+1
// LDS rows: 128 floats [P 64 | Q 64], unpadded (a 16-byte LDS-DMA writes 1 KB = two whole rows contiguously), with the 16-byte
// slots of each half XOR-swizzled by (row & 15): logical slot c of row r sits at slot c ^ (r & 15). ds_read_b64 of one k-group
// by 32 rows then touches every bank pair twice (rows r and r+16, and a surface's P and Q halves): 2-way, 4 LDS cycles.
constexpr int ROW_F = 128;
constexpr int A_F = 2 * 32 * ROW_F;    // [parity][32 surfaces]
constexpr int B_F = 2 * 32 * ROW_F;    // [parity][32 overheads]
constexpr int STAGE_F = A_F + B_F;     // 16384 floats
constexpr int LDS_F = 2 * STAGE_F;     // stage 0 | stage 1 / the epilogue exchange (4 waves x 16 KB per round)

__device__ __forceinline__ unsigned lds_address(const void* p) {
    return (unsigned)(unsigned long long)(__attribute__((address_space(3))) const void*)p;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ i32x4 raw_rsrc(const void* base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    i32x4 r;
    r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
    r[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)((a >> 32) & 0xffffu));
    r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
    r[3] = 0x00020000;
    return r;
}

// global -> LDS, 16 B per lane, 1 KB of contiguous LDS per wave instruction at lds_addr (M0); out-of-range lanes write 0
__device__ __forceinline__ void dma16(i32x4 rs, unsigned lds_addr, unsigned voff, unsigned soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                 :
                 : "s"(lds_addr), "v"(voff), "s"(rs), "s"(soff)
                 : "memory");
}

// One ds_read_b64 (the compiler would fuse neighbouring ones into ds_read2_b64, which is banked like ds_read_b32: 2-way on
// these rows). The results are ordered by lds_wait<N>() below, which also names them so that no MFMA moves above the wait.
template <int OFF>
__device__ __forceinline__ f32x2 lds_read64(unsigned addr) {
    f32x2 v;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
// operand address of k-group U: base ^ (U << 4) (the slot swizzle); formed in the GEMM-2 phase, see XA / XB / XC below
template <int IMM>
__device__ __forceinline__ unsigned lds_xor(unsigned addr) { return addr ^ (unsigned)IMM; }
// the step's inverse-transform coefficient, by hand as well (issued in group 14, covered by group 15's lgkmcnt(0)): a
// compiler-issued LDS read would be waited for with lgkmcnt(0) at its use, behind the next step's operand reads already in flight
__device__ __forceinline__ float lds_read32(unsigned addr) {
    float v;
    asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(addr));
    return v;
}
template <int N>
__device__ __forceinline__ void lds_wait(f32x2& a, f32x2& b, f32x2& c, f32x2& d) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N));
}

// GEMM-1 MFMA with its accumulator pinned to VGPRs. The wave owns 16 x 16 long-lived accumulation registers (all 256 AGPRs);
// left to the compiler the two short-lived GEMM-1 accumulators also go to AGPRs, 288 > 256, and one long-lived tile is shuttled
// through v_accvgpr moves every step: 79 instead of 69 cycles per MFMA in tools/mfma_rate.cpp's model of this loop. Inline asm
// is outside the compiler's hazard recogniser: the required wait states sit in mfma_settle() below.
__device__ __forceinline__ void mfma_v(f32x16& acc, float a, float b) {
    asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
// first MFMA of a chain: C = 0 as an inline constant instead of 16 zeroed registers
__device__ __forceinline__ void mfma_v0(f32x16& acc, float a, float b) {
    asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, 0" : "=v"(acc) : "v"(a), "v"(b));
}
// 16 accumulation registers back to zero for the next tile, as ONE instruction on the matrix pipe, which is idle during the
// epilogue (0 x 0 + 0), instead of 16 v_accvgpr_write on the vector pipe, which is the busy one there. asm: the builtin with
// constant operands is folded back into the 16 writes
__device__ __forceinline__ void mfma_zero(f32x16& acc, float zero) {
    asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %1, 0" : "=a"(acc) : "v"(zero));
}
// 16-pass XDL write -> VALU read of the result: 18 wait states (CDNA3 ISA, manually inserted wait states)
__device__ __forceinline__ void mfma_settle(f32x16& x, f32x16& y) {
    asm volatile("s_nop 15\n\ts_nop 3" : "+v"(x), "+v"(y));
}

// One pair's 16 shifts of a lane (register q = shift (q & 3) + 8 (q >> 2) + 4 hk; the 4 hk is added by the caller) x {E + O at
// that shift, E - O at shift + 32}: the largest value, its index in torch.argmax order (smallest index among equal values) and,
// GAP, the runner-up value. max(E + O, E - O) = E + |O| and a negative O puts it at shift + 32 (O = -0 cannot come out of an
// MFMA sum that started at +0), so the scan looks at 16 values instead of 32. The index travels as (sign bit of O | shift),
// ordered like the arg-max index under an unsigned minimum; no comparison of O, whose VCC result would cost two wait states
// before the v_cndmask that reads it (gfx950).
constexpr unsigned NOKEY = 0xffffffffu;
__device__ __forceinline__ unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }      // (min() resolves to the int overload)
// lo / hi = the lower / upper half-wave's x, in every lane: v_permlane32_swap exchanges the first operand's lanes 32-63 with the
// second one's lanes 0-31 (tools/debug/permlane_probe.cpp)
template <typename T>
__device__ __forceinline__ void half_swap(T x, T& lo, T& hi) {
    const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, x), false, false);
    const unsigned r0 = r[0], r1 = r[1];      // (a __builtin_bit_cast of the element expression r[1] itself reads element 0)
    lo = __builtin_bit_cast(T, r0);
    hi = __builtin_bit_cast(T, r1);
}
// VONLY: only the largest value is wanted (no orientation output and a full-width surface, whose window norm does not depend on
// the shift): the index search -- two thirds of the scan's instructions -- is left out
template <bool GAP, bool VONLY>
__device__ __forceinline__ void scan16(const f32x16& E, const f32x16& O, float& best, unsigned& key, float& second) {
    float m[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) m[q] = E[q] + fabsf(O[q]);
    float v = -INFINITY, s2 = -INFINITY;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        // GAP: the second largest of the 32 values rides along (E - |O| never is the largest of its pair)
        if (GAP) s2 = fmaxf(fmaxf(s2, fminf(m[q], v)), E[q] - fabsf(O[q]));
        v = fmaxf(v, m[q]);
    }
    unsigned k = NOKEY;
#pragma unroll
    for (int q = 0; q < (VONLY ? 0 : 16); ++q) {
        const unsigned c = (unsigned)((q & 3) + 8 * (q >> 2));
        const float oq = O[q];      // (a __builtin_bit_cast of the element expression O[q] itself reads element 0 for every q)
        const unsigned kq = (__builtin_bit_cast(unsigned, oq) & 0x80000000u) | c;      // v_and + v_or (as asm v_bfi_b32: more moves)
        k = umin(k, m[q] == v ? kq : NOKEY);
    }
    best = v;
    key = k;
    if (GAP) second = s2;
}

// MASKED (orientation prior, one 64-bit word per surface: bit k set = shift k may be chosen): a shift the word forbids enters
// with -inf, which breaks the pairing of shift c with c + 32 through E + |O| -- both candidates of a register are formed,
// a = E + O at shift c and b = E - O at shift c + 32, and the key's high bit is set exactly when b > a (a tie goes to a, the
// lower index). lo / hi: the surface's word (bits 0-31 / 32-63) shifted right by 4 hk, so that bit (q & 3) + 8 (q >> 2) of
// them is the lane's shift of register q; the test is re-derived from these two registers for every candidate (no per-register
// predicates are kept: the GAP instantiation sits at the register limit). GAP: the runner-up is the second largest ALLOWED
// value (-inf when one shift is allowed: the gap is then +inf). A lane none of whose 32 shifts is allowed (or whose allowed
// scores are all NaN) returns -inf and NOKEY.
// x where bit `c` of `word` is set, else -inf, as bit operations (v_bfe_i32 + one three-input bit op). The empty asm makes the
// word opaque behind x: without it the 32 tests of a scan depend on the mask word alone and are all formed ahead of the scan, 32
// live registers that the GAP instantiation does not have; as comparisons they would be 32 lane masks in scalar register pairs
__device__ __forceinline__ float allowed_or_ninf(float x, unsigned word, unsigned c) {
    asm("" : "+v"(word) : "v"(x));
    const unsigned sel = (unsigned)((int)(word << (31u - c)) >> 31);
    return __builtin_bit_cast(float, (__builtin_bit_cast(unsigned, x) & sel) | (0xff800000u & ~sel));
}
template <bool GAP, bool VONLY>
__device__ __forceinline__ void scan16_masked(const f32x16& E, const f32x16& O, unsigned lo, unsigned hi, float& best, unsigned& key,
                                              float& second) {
    float m[16];
    unsigned kq[16], hb = 0u;
    float v = -INFINITY, s2 = -INFINITY;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const unsigned c = (unsigned)((q & 3) + 8 * (q >> 2));
        const float a = allowed_or_ninf(E[q] + O[q], lo, c);
        const float b = allowed_or_ninf(E[q] - O[q], hi, c);
        m[q] = fmaxf(a, b);
        // b > a as the sign of a - b (+0 on a tie, -inf / +inf when one side is forbidden): no comparison, as in scan16.
        // GAP (at the register limit): the 16 signs are collected in ONE register, register q's ends up at bit 16 + q
        const float ab = a - b;
        const unsigned sign = __builtin_bit_cast(unsigned, ab) & 0x80000000u;
        if (GAP) hb = (hb >> 1) | sign;
        else if (!VONLY) kq[q] = sign | c;
        if (GAP) s2 = fmaxf(fmaxf(s2, fminf(m[q], v)), fminf(a, b));
        v = fmaxf(v, m[q]);
    }
    unsigned k = NOKEY;
#pragma unroll
    for (int q = 0; q < (VONLY ? 0 : 16); ++q) {
        const unsigned c = (unsigned)((q & 3) + 8 * (q >> 2));
        const unsigned kk = GAP ? (((hb << (15 - q)) & 0x80000000u) | c) : kq[q];
        k = umin(k, m[q] == v ? kk : NOKEY);
    }
    best = v;
    key = v > -INFINITY ? k : NOKEY;
    if (GAP) second = s2;
}

struct DftArgs {
    const float* spec_ov;    // [Bo][32][128]
    const float* spec_su;    // [Bs][32][128]
    const float* dtab;       // [32][64]: lane (hk, shift) -> inverse-transform coefficient of the slot's (Re | Im) at that shift
    const float* wn;         // [Bo,64] window norms per shift
    const float* sn;         // [Bs]    surface norms
    long long* orientation;  // [Bo,Bs] or null
    float* distance;         // [Bo,Bs] or null
    float* score;            // [Bo,Bs] or null
    float* gap;              // [Bo,Bs] or null (GAP instantiation): best score - runner-up score over the 64 shifts
    int Bo, Bs, nbx, nby;
    unsigned long long* stamps;      // null, or 64 slots per 4096th workgroup (WITW_DFT_STAMPS=1: in-kernel timeline)
    const unsigned long long* mask;  // [Bs] (MASKED instantiations): bit k of mask[s] set = shift k may be chosen for surface s (0 = no prior)
};

// REC: the diagnostic instantiation that records the in-kernel timeline (costs registers: the product launch uses REC = false)
// GAP: the shift scan also tracks the runner-up score and writes best - runner-up (narrow surfaces: the caller re-scores the
// pairs whose two best shifts tie to rounding, cvig_fov._dft_pass_narrow)
// MASKED: the shift search of surface s runs over the set bits of p.mask[s] (scan16_masked). Two kernels are compiled from one
// text (match_dft_kernel.h): match_dft_kernel<REC, GAP, VONLY>, the kernel it was before the masks existed, and
// match_dft_masked_kernel<GAP, VONLY> (witw_match_fwd_dft_masked)
#define WITW_DFT_KERNEL match_dft_kernel
#define WITW_DFT_TPARAMS bool REC, bool GAP, bool VONLY
#define WITW_DFT_CONSTS constexpr bool MASKED = false;
#include "match_dft_kernel.h"
#undef WITW_DFT_KERNEL
#undef WITW_DFT_TPARAMS
#undef WITW_DFT_CONSTS
#define WITW_DFT_KERNEL match_dft_masked_kernel
#define WITW_DFT_TPARAMS bool GAP, bool VONLY
#define WITW_DFT_CONSTS constexpr bool REC = false, MASKED = true;
#include "match_dft_kernel.h"
#undef WITW_DFT_KERNEL
#undef WITW_DFT_TPARAMS
#undef WITW_DFT_CONSTS

// spec[e][t][0..63] = Re X_t(line), [64..127] = Im X_t(line) (0 for t = 0, 32), X_t = sum_k x[line][k] e^{-2 pi i t k / 64}; fp64
// accumulation, rounded once to fp32. One workgroup per embedding [64 lines][W columns], W <= 64.
// role: whose spectrum this is, which fixes the order of the two 8-byte chunks (float pairs) inside each 16-byte slot so that the
// match kernel's ds_read_b64 are free of bank conflicts (see the operand roles there): 0 = surface (queries): the chunks of the
// Q half exchanged; 1 = overhead (gallery): both halves' chunks exchanged for embeddings whose index has bit 4 set.
__global__ __launch_bounds__(256) void match_spectrum_kernel(const float* __restrict__ emb, float* __restrict__ spec, int W, int role) {
    __shared__ float xs[64 * 65];
    __shared__ double cs[64], sn[64];
    const int tid = threadIdx.x, line = tid & 63, tq = tid >> 6;
    const float* x = emb + (size_t)blockIdx.x * 64 * W;
    for (int i = tid; i < 64 * W; i += 256) xs[(i / W) * 65 + (i % W)] = x[i];
    if (tid < 64) {
        cs[tid] = cospi((double)tid / 32.0);
        sn[tid] = sinpi((double)tid / 32.0);
    }
    __syncthreads();
    float* out = spec + (size_t)blockIdx.x * SPEC;
    for (int t = tq; t <= 32; t += 4) {      // frequencies 0..32; X_0 and X_32 are real and share storage slot 0 (P = X_0, Q = X_32)
        double pr = 0.0, pi = 0.0;
        for (int k = 0; k < W; ++k) {
            const int idx = (t * k) & 63;
            const double xv = (double)xs[line * 65 + k];
            pr += xv * cs[idx];
            pi -= xv * sn[idx];
        }
        const int swap_p = (role == 1 && (blockIdx.x & 16)) ? 2 : 0;      // float index ^ 2 = the other 8-byte chunk of the slot
        const int swap_q = (role == 0 || (blockIdx.x & 16)) ? 2 : 0;
        if (t == 32) out[64 + (line ^ swap_q)] = (float)pr;
        else {
            out[t * 128 + (line ^ swap_p)] = (float)pr;
            if (t != 0) out[t * 128 + 64 + (line ^ swap_q)] = (float)pi;
        }
    }
}

// The same spectra for full-width embeddings (W = 64: every gallery row, and the queries at fov 360) with the inner loop in
// registers (round 6). The kernel above reads three LDS words per (line, frequency, k) -- the sample, cos and sin as doubles -- and
// is bound by those reads: 125,000 gallery rows took 5 ms of the retrieval pass. Here a thread reads its line's samples (once per k from LDS), the 17 distinct twiddle magnitudes cos(2 pi m / 64), m = 0..16, are registers too, and because
// a wave's frequencies are fixed (wave 0 the even t, wave 1 the odd t) every (t, k) names its magnitude and sign when the body is
// generated: two v_fma_f64 per (line, t, k), one LDS word and one convert per (line, k). Same sums in the same k order, fp64, rounded once to fp32; products are fused here
// (the kernel above rounds the product, then the sum), so single values may differ in the last fp32 bit -- inside the rounding
// bound of the spectral scores that the index-exact re-scoring is built on (ops.SCORE_ROUNDING).
struct Twiddle64 { double c[17]; };      // cos(2 pi m / 64), m = 0..16: kernel arguments, i.e. scalar registers

// one workgroup = two waves per embedding: lane = line, wave = parity of the frequencies it sums; the body is generated
// (tools/gen_spectrum64.py -> spectrum64_gen.h): straight-line code, every twiddle a named scalar with its sign
__global__ __launch_bounds__(128) void match_spectrum64_kernel(const float* __restrict__ emb, float* __restrict__ spec, int role, Twiddle64 tw) {
    __shared__ float xs[64 * 65];
    const int tid = threadIdx.x, line = tid & 63;
    const int par = __builtin_amdgcn_readfirstlane(tid >> 6);
    const f32x4* x4 = reinterpret_cast<const f32x4*>(emb + (size_t)blockIdx.x * 4096);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int q = tid + i * 128;              // float4 index: row q >> 4, columns 4 (q & 15) ..
        const f32x4 v = x4[q];
        float* d = xs + (q >> 4) * 65 + 4 * (q & 15);
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
    const double c0 = tw.c[0], c1 = tw.c[1], c2 = tw.c[2], c3 = tw.c[3], c4 = tw.c[4], c5 = tw.c[5], c6 = tw.c[6], c7 = tw.c[7], c8 = tw.c[8],
                 c9 = tw.c[9], c10 = tw.c[10], c11 = tw.c[11], c12 = tw.c[12], c13 = tw.c[13], c14 = tw.c[14], c15 = tw.c[15], c16 = tw.c[16];
    __syncthreads();
    float* out = spec + (size_t)blockIdx.x * SPEC;
    const int swap_p = (role == 1 && (blockIdx.x & 16)) ? 2 : 0;      // as in match_spectrum_kernel
    const int swap_q = (role == 0 || (blockIdx.x & 16)) ? 2 : 0;
    const float* xrow = xs + line * 65;           // pitch 65: the wave's 64 lines read 64 different banks
#define WITW_SPEC_STORE(T, PR, PI)                                            \
    if ((T) == 32) out[64 + (line ^ swap_q)] = (float)(PR);                   \
    else {                                                                    \
        out[(T) * 128 + (line ^ swap_p)] = (float)(PR);                       \
        if ((T) != 0) out[(T) * 128 + 64 + (line ^ swap_q)] = (float)(PI);    \
    }
    if (par == 0) {
        WITW_SPECTRUM64_BODY_0(xrow);
        WITW_SPECTRUM64_STORE_0(WITW_SPEC_STORE);
    } else {
        WITW_SPECTRUM64_BODY_1(xrow);
        WITW_SPECTRUM64_STORE_1(WITW_SPEC_STORE);
    }
#undef WITW_SPEC_STORE
}

// dtab[t][hk*32 + shift]: coefficient of lanes 0-31 (hk = 0) / 32-63 (hk = 1) of slot t's C in score[shift], shift < 32. Slots
// 1..31: Re C_t / Im C_t. Slot 0: the kernel leaves C_0 + C_32 in lanes 0-31 and C_32 - C_0 in lanes 32-63, and
// (C_0 + (-1)^shift C_32) / 64 is the former at even shifts and minus the latter at odd ones
__global__ void match_dft_table_kernel(float* __restrict__ dtab) {
    const int t = blockIdx.x, lane = threadIdx.x, shift = lane & 31, hk = lane >> 5;
    double v;
    if (t == 0) v = hk ? ((shift & 1) ? -1.0 / 64.0 : 0.0) : ((shift & 1) ? 0.0 : 1.0 / 64.0);
    else {
        const double ang = (double)((t * shift) & 63) / 32.0;
        v = hk ? -sinpi(ang) / 32.0 : cospi(ang) / 32.0;
    }
    dtab[t * 64 + lane] = (float)v;
}

// the two norm kernels of match.hip's launch, restated here (file-local there)
__global__ __launch_bounds__(256) void dft_window_norm_kernel(const float* __restrict__ ov, float* __restrict__ wn, int We) {
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

__global__ __launch_bounds__(256) void dft_row_norm_kernel(const float* __restrict__ x, float* __restrict__ out, int n) {
    __shared__ float part[4];
    const float* base = x + (size_t)blockIdx.x * n;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = base[i];
        s += v * v;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = sqrtf((part[0] + part[1]) + (part[2] + part[3]));
}

}  // namespace

extern "C" {

// floats of one embedding's row spectrum (32 slots x [64 re | 64 im]; slot 0: [X_0 | X_32])
long long witw_match_spectrum_floats(long long n_embeddings) { return n_embeddings * (long long)SPEC; }

// emb [B,64 lines,W] (an overhead embedding [B,16,4,64], role 1, or a surface embedding [B,16,4,We], role 0) -> spec [B,32,128]
// in the chunk order the match kernel's operand reads expect of that side (an overhead's spectrum depends on its index & 16:
// spectra of a gallery must be computed at the row numbering they are matched at, multiples of 32 apart)
static int g_spectrum_regs = getenv("WITW_SPECTRUM_LDS") == nullptr;      // WITW_SPECTRUM_LDS=1: the LDS-table kernel at every width (A/B)

int witw_match_spectrum(const float* emb, float* spec, int B, int W, int role, void* stream) {
    WITW_CHECK_ARG(emb && spec, "match_spectrum: null pointer");
    WITW_CHECK_ARG(B > 0 && W >= 1 && W <= 64, "match_spectrum: bad shape B=%d W=%d", B, W);
    WITW_CHECK_ARG(role == 0 || role == 1, "match_spectrum: role %d (0 = surface / query side, 1 = overhead / gallery side)", role);
    if (W == 64 && g_spectrum_regs)
        {
        Twiddle64 tw;
        for (int m = 0; m <= 16; ++m) tw.c[m] = m == 16 ? 0.0 : cos(2.0 * 3.14159265358979323846 * m / 64.0);
        hipLaunchKernelGGL(match_spectrum64_kernel, dim3(B), dim3(128), 0, (hipStream_t)stream, emb, spec, role, tw);
    }
    else
        hipLaunchKernelGGL(match_spectrum_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, emb, spec, W, role);
    WITW_CHECK_LAUNCH("match_spectrum");
    return WITW_OK;
}

long long witw_match_dft_workspace_floats(int Bo, int Bs) { return (long long)Bo * 64 + Bs + NSLOT * 64; }

// Same outputs as witw_match_fwd (orientation / distance / score [Bo,Bs], any of them may be null) from the row spectra of the
// two sides (witw_match_spectrum of ov with W = 64 and of su with W = We); ov / su themselves are read for the norms only.
static int match_fwd_dft_launch(const float* ov, const float* su, const float* spec_ov, const float* spec_su, int Bo, int Bs, int We,
                                long long* orientation, float* distance, float* score, float* gap, float* workspace,
                                const unsigned long long* shift_mask, void* stream) {
    WITW_CHECK_ARG(ov && su && spec_ov && spec_su && workspace, "match_fwd_dft: null pointer");
    WITW_CHECK_ARG(Bo > 0 && Bs > 0, "match_fwd_dft: empty batch Bo=%d Bs=%d", Bo, Bs);
    WITW_CHECK_ARG(We >= 1 && We <= 64, "match_fwd_dft: surface embedding width %d outside [1,64]", We);
    hipStream_t st = (hipStream_t)stream;
    float* wn = workspace;
    float* sn = workspace + (size_t)Bo * 64;
    float* dtab = sn + Bs;
    hipLaunchKernelGGL(dft_window_norm_kernel, dim3(Bo), dim3(256), 0, st, ov, wn, We);
    hipLaunchKernelGGL(dft_row_norm_kernel, dim3(Bs), dim3(256), 0, st, su, sn, 64 * We);
    hipLaunchKernelGGL(match_dft_table_kernel, dim3(NSLOT), dim3(64), 0, st, dtab);
    DftArgs a;
    a.spec_ov = spec_ov; a.spec_su = spec_su; a.dtab = dtab; a.wn = wn; a.sn = sn;
    a.orientation = orientation; a.distance = distance; a.score = score; a.gap = gap;
    a.Bo = Bo; a.Bs = Bs; a.nbx = cdiv(Bs, 32); a.nby = cdiv(Bo, 32);
    const long long tiles = (long long)a.nbx * a.nby;
    WITW_CHECK_ARG(tiles < (1LL << 31), "match_fwd_dft: %lld tiles of 32 x 32 pairs (the kernel counts tiles in 32 bits)", tiles);
    const int n_cu = witw_cu_count();        // persistent workgroups, one per CU
    const unsigned grid = (unsigned)(tiles < n_cu ? tiles : n_cu);
    // WITW_DFT_STAMPS=1 (diagnostic, synchronous): the first workgroups record s_memrealtime around the phases of their second
    // tile; printed to stderr
    a.stamps = nullptr;
    a.mask = shift_mask;
    const int nrec = 4;
    if (!gap && !shift_mask && getenv("WITW_DFT_STAMPS") != nullptr && tiles >= 2LL * grid) {
        if (hipMalloc((void**)&a.stamps, (size_t)nrec * 64 * 8) != hipSuccess) a.stamps = nullptr;
        else (void)hipMemset(a.stamps, 0, (size_t)nrec * 64 * 8);
    }
    // value-only scan: no orientation wanted and the surface as wide as the overhead (fov 360: the window norm is the same sum for
    // every shift, in another order -- the distance then uses shift 0's, within an ulp of any other's)
    const bool vonly = !orientation && !gap && We == 64 && getenv("WITW_DFT_VONLY_OFF") == nullptr;
    // a mask was given: the masked instantiation of the same form (the diagnostic timeline has none)
    if (shift_mask) {
        if (gap) hipLaunchKernelGGL((match_dft_masked_kernel<true, false>), dim3(grid), dim3(256), 0, st, a);
        else if (vonly) hipLaunchKernelGGL((match_dft_masked_kernel<false, true>), dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((match_dft_masked_kernel<false, false>), dim3(grid), dim3(256), 0, st, a);
    }
    else if (gap) hipLaunchKernelGGL((match_dft_kernel<false, true, false>), dim3(grid), dim3(256), 0, st, a);
    else if (a.stamps && WITW_DFT_PHASES && getenv("WITW_DFT_STAMPS")[0] == '2') {
        if (vonly) hipLaunchKernelGGL((match_dft_kernel<false, false, true>), dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((match_dft_kernel<false, false, false>), dim3(grid), dim3(256), 0, st, a);
        (void)hipDeviceSynchronize();
        unsigned long long h[4 * 64];
        (void)hipMemcpy(h, a.stamps, sizeof(h), hipMemcpyDeviceToHost);
        for (int b = 0; b < 4; ++b)
            fprintf(stderr, "match_dft workgroup %d: %llu tiles, steps %.2f us per tile, epilogue %.2f us per tile (send 0 + barrier %.2f, scans 0 %.2f, "
                    "barrier + send 1 + barrier %.2f, scans 1 %.2f, output + zeroing %.2f)\n", b, h[b * 64 + 2],
                    h[b * 64] * 0.01 / (double)h[b * 64 + 2], h[b * 64 + 1] * 0.01 / (double)h[b * 64 + 2], h[b * 64 + 3] * 0.01 / (double)h[b * 64 + 2],
                    h[b * 64 + 4] * 0.01 / (double)h[b * 64 + 2], h[b * 64 + 5] * 0.01 / (double)h[b * 64 + 2], h[b * 64 + 6] * 0.01 / (double)h[b * 64 + 2],
                    h[b * 64 + 7] * 0.01 / (double)h[b * 64 + 2]);
        for (int b = 0; b < 4; ++b)
            fprintf(stderr, "match_dft workgroup %d: per step, previous barrier -> end of GEMM 1 %.3f us, vmcnt wait + barrier %.3f us; s_memtime ticks per us %.1f\n", b,
                    h[b * 64 + 8] * 0.01 / ((double)NSTEP * (double)h[b * 64 + 2]), h[b * 64 + 9] * 0.01 / ((double)NSTEP * (double)h[b * 64 + 2]),
                    (double)h[b * 64 + 11] / ((double)h[b * 64 + 10] * 0.01));
        (void)hipFree(a.stamps);
        a.stamps = nullptr;
    }
    else if (a.stamps) hipLaunchKernelGGL((match_dft_kernel<true, false, false>), dim3(grid), dim3(256), 0, st, a);
    else if (vonly) hipLaunchKernelGGL((match_dft_kernel<false, false, true>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((match_dft_kernel<false, false, false>), dim3(grid), dim3(256), 0, st, a);
    if (a.stamps) {
        (void)hipDeviceSynchronize();
        unsigned long long* h = (unsigned long long*)malloc((size_t)nrec * 64 * 8);
        (void)hipMemcpy(h, a.stamps, (size_t)nrec * 64 * 8, hipMemcpyDeviceToHost);
        for (int b = 0; b < nrec && b < 4; ++b) {
            const unsigned long long* t = h + (size_t)b * 64;
            fprintf(stderr, "match_dft workgroup %d, second tile: first-stage wait %.2f us; steps (gemm1, barrier, gemm2) us:", b, (t[1] - t[0]) * 0.01);
            for (int i = 0; i < NSTEP; ++i)
                fprintf(stderr, " [%.2f %.2f %.2f]", (t[2 + 3 * i] - (i ? t[1 + 3 * i] : t[1])) * 0.01, (t[3 + 3 * i] - t[2 + 3 * i]) * 0.01,
                        (t[4 + 3 * i] - t[3 + 3 * i]) * 0.01);
            fprintf(stderr, "; epilogue %.2f us; total %.2f us\n", (t[53] - t[1 + 3 * NSTEP]) * 0.01, (t[53] - t[0]) * 0.01);
        }
        free(h);
        (void)hipFree(a.stamps);
    }
    WITW_CHECK_LAUNCH("match_fwd_dft");
    return WITW_OK;
}

int witw_match_fwd_dft(const float* ov, const float* su, const float* spec_ov, const float* spec_su, int Bo, int Bs, int We,
                       long long* orientation, float* distance, float* score, float* workspace, void* stream) {
    return match_fwd_dft_launch(ov, su, spec_ov, spec_su, Bo, Bs, We, orientation, distance, score, nullptr, workspace, nullptr, stream);
}

// witw_match_fwd_dft that also writes gap [Bo,Bs] = best score - runner-up score of every pair (how far the chosen shift is
// from a tie): the caller re-scores the pairs whose gap is within rounding with witw_match_pairs.
int witw_match_fwd_dft_gap(const float* ov, const float* su, const float* spec_ov, const float* spec_su, int Bo, int Bs, int We,
                           long long* orientation, float* distance, float* score, float* gap, float* workspace, void* stream) {
    WITW_CHECK_ARG(gap, "match_fwd_dft_gap: null gap pointer");
    return match_fwd_dft_launch(ov, su, spec_ov, spec_su, Bo, Bs, We, orientation, distance, score, gap, workspace, nullptr, stream);
}

// witw_match_fwd_dft[_gap] (gap may be null) with the shift search of every surface s restricted to the set bits of shift_mask[s]
// ([Bs], device; a word of 0 = no prior = all 64 bits): the semantics of witw_match_fwd_masked. gap, when wanted, is the best
// score minus the second best ALLOWED score, +inf where the word allows one shift.
int witw_match_fwd_dft_masked(const float* ov, const float* su, const float* spec_ov, const float* spec_su, int Bo, int Bs, int We,
                              long long* orientation, float* distance, float* score, float* gap, float* workspace,
                              const unsigned long long* shift_mask, void* stream) {
    WITW_CHECK_ARG(shift_mask, "match_fwd_dft_masked: null shift_mask pointer");
    return match_fwd_dft_launch(ov, su, spec_ov, spec_su, Bo, Bs, We, orientation, distance, score, gap, workspace, shift_mask, stream);
}

}  // extern "C"
