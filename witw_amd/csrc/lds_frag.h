// Hand-issued memory primitives (gfx950) of the reduced-precision convolution kernels and of the spectral match (match_dft.hip,
// which takes the LDS-DMA part and reads its fragments with helpers of its own): LDS-DMA loads with a counted vmcnt wait, and LDS
// fragment reads with counted lgkmcnt waits. Every sequence below is inline assembly ON PURPOSE: it keeps the order it is written
// in, and the kernel, not the compiler, decides where the wave waits. The three convolution kernels that read fragments this way
// are correct only for the register allocations validated in build.py.
#pragma once
#include "common.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned lds_address(const void* p) {
    return (unsigned)(unsigned long long)(__attribute__((address_space(3))) const void*)p;
}

// ---- LDS-DMA (buffer_load ... lds)

// Raw buffer descriptor (base, stride 0, byte count, the flag word that __builtin_amdgcn_make_buffer_rsrc is given elsewhere in
// these kernels) as four SGPRs for the hand-issued LDS-DMA loads.
__device__ __forceinline__ i32x4 raw_rsrc(const void* base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    i32x4 r;
    r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
    r[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)((a >> 32) & 0xffffu));
    r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
    r[3] = 0x00020000;
    return r;
}

// One wave instruction of LDS-DMA: lane l moves 16 B from rs[voff_l + soff] to LDS byte address lds_addr + 16*l, 1 KB of
// contiguous LDS per instruction (out-of-range lanes store zeros: padding is a load policy).
//   * Why not the builtin: for the builtin form the compiler puts a vmcnt wait in front of every later ds_read (it cannot tell the
//     stage being read from the stage being filled), which serialises the pipeline; here the wave drains vmcnt itself
//     (wait_vmcnt, or s_waitcnt 0x0F70) once per K chunk before the barrier that publishes the data.
//   * m0 is written here and is NOT on the clobber list: it is a reserved register for LLVM's AMDGPU back end (clang warns "clobber
//     list contains reserved registers: m0 ... undefined behaviour" when it is listed), which keeps no value live in it across
//     instructions and re-sets it right before each of its own uses (LDS-DMA builtins, movrel, sendmsg).
__device__ __forceinline__ void dma16(i32x4 rs, unsigned lds_addr, unsigned voff, unsigned soff) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                 :
                 : "s"(lds_addr), "v"(voff), "s"(rs), "s"(soff)
                 : "memory");
#endif
}
// ... with the scalar offset as the literal 0 (no SGPR operand)
__device__ __forceinline__ void dma16(i32x4 rs, unsigned lds_addr, unsigned voff) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
                 :
                 : "s"(lds_addr), "v"(voff), "s"(rs)
                 : "memory");
#endif
}

// s_waitcnt vmcnt(N) only (expcnt / lgkmcnt left alone); N <= 63. Vector-memory operations retire in issue order, so N = the
// number of loads issued after the last one that must have landed.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | 0x0F70);
}

// ---- LDS fragment reads with counted waits
//
// Left to the scheduler each ds_read sinks to just in front of its MFMA and every MFMA waits on lgkmcnt(0), or refills are hoisted
// above the MFMAs that still read the old fragment and cost a second register set. asm volatile statements keep their order and
// LDS returns in order, so a consumer can wait with lgkmcnt(number of reads issued after the last one it needs); extra LDS
// operations of the compiler in the queue only make a wait stricter. lds_wait names the fragments it releases, so that the MFMAs
// reading them cannot be scheduled above it.
__device__ __forceinline__ u32x4 lds_read128(unsigned addr) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
    return v;
}
__device__ __forceinline__ u32x4 lds_read128(unsigned addr, int off) {      // off: a constant once the caller's loops are unrolled
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(off));
    return v;
}
typedef unsigned int u32x2_frag __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32x2_frag lds_read64(unsigned addr) {
    u32x2_frag v;
    asm volatile("ds_read_b64 %0, %1" : "=v"(v) : "v"(addr));
    return v;
}
// s_waitcnt lgkmcnt(0) over a whole array of fragments (everything this wave has in the LDS queue has landed)
template <typename T, int N>
__device__ __forceinline__ void lds_wait_all(T (&f)[N]) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("" : "+v"(f[i]));      // the consumers of f[i] stay behind the wait
}

// s_waitcnt lgkmcnt(n) that names the fragments it releases. n is a constant once the caller's loops are unrolled; the counter
// field has 4 bits: deeper queues wait at 15 (conservative).
#define WITW_LDS_WAIT(...)                                                        \
    switch (n) {                                                                  \
    case 0: asm volatile("s_waitcnt lgkmcnt(0)" : __VA_ARGS__); break;            \
    case 1: asm volatile("s_waitcnt lgkmcnt(1)" : __VA_ARGS__); break;            \
    case 2: asm volatile("s_waitcnt lgkmcnt(2)" : __VA_ARGS__); break;            \
    case 3: asm volatile("s_waitcnt lgkmcnt(3)" : __VA_ARGS__); break;            \
    case 4: asm volatile("s_waitcnt lgkmcnt(4)" : __VA_ARGS__); break;            \
    case 5: asm volatile("s_waitcnt lgkmcnt(5)" : __VA_ARGS__); break;            \
    case 6: asm volatile("s_waitcnt lgkmcnt(6)" : __VA_ARGS__); break;            \
    case 7: asm volatile("s_waitcnt lgkmcnt(7)" : __VA_ARGS__); break;            \
    case 8: asm volatile("s_waitcnt lgkmcnt(8)" : __VA_ARGS__); break;            \
    case 9: asm volatile("s_waitcnt lgkmcnt(9)" : __VA_ARGS__); break;            \
    case 10: asm volatile("s_waitcnt lgkmcnt(10)" : __VA_ARGS__); break;          \
    case 11: asm volatile("s_waitcnt lgkmcnt(11)" : __VA_ARGS__); break;          \
    case 12: asm volatile("s_waitcnt lgkmcnt(12)" : __VA_ARGS__); break;          \
    case 13: asm volatile("s_waitcnt lgkmcnt(13)" : __VA_ARGS__); break;          \
    case 14: asm volatile("s_waitcnt lgkmcnt(14)" : __VA_ARGS__); break;          \
    default: asm volatile("s_waitcnt lgkmcnt(15)" : __VA_ARGS__); break;          \
    }
__device__ __forceinline__ void lds_wait(int n, u32x4& a) { WITW_LDS_WAIT("+v"(a)) }
__device__ __forceinline__ void lds_wait(int n, u32x4& a, u32x4& b) { WITW_LDS_WAIT("+v"(a), "+v"(b)) }
__device__ __forceinline__ void lds_wait(int n, u32x4& a, u32x4& b0, u32x4& b1, u32x4& b2, u32x4& b3) {
    WITW_LDS_WAIT("+v"(a), "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3))
}
#undef WITW_LDS_WAIT

}  // namespace
