// Gallery retrieval for cvig_baseline embeddings (gfx950): Euclidean distances of [rows, n] embeddings at GEMM cost, plus the exact
// re-scoring of single pairs that makes the result index-exact (witw_amd/cvig_baseline.py: retrieve).
//
//   witw_row_sqnorm   |x_i|^2, one wave per row.
//   witw_sqdist_gemm  D[i][j] = max(0, gn[i] + qn[j] - 2 g_i.q_j): a tiled fp32 GEMM on v_mfma_f32_32x32x2_f32. Both operands are
//                     K-major ([rows, n]), so the gallery (A) and query (B) tiles are staged the same way. The product form loses the
//                     small distances of true pairs to cancellation: the host treats D as known to +-eps only (band_eps in
//                     cvig_baseline.py) and re-makes every decision inside that band on
//   witw_sqdist_pairs the difference form of pairwise_sqdist_kernel (baseline.hip) for a list of pairs, bit for bit: both call
//                     witw_sqdist_row (sqdist_row.h), the same expression in the same order.
//
// GEMM tile: 128 gallery rows x 128 queries per 256-thread workgroup, each of the 4 waves a 64 x 64 quadrant (2 x 2 MFMA tiles, 64
// accumulator registers). K runs in stages of KT = 32 floats through two LDS buffers: the global loads of stage s+1 are issued in
// front of the MFMAs of stage s and stored behind them, one barrier per stage. LDS rows are KT + 4 floats apart, which makes the
// 16-byte fragment reads conflict-free (36 r mod 64 takes 16 distinct multiples of 4 over each 16-lane group of ds_read_b128).
// The MFMA sums over k in any order, so lane half hk takes k = 16 hk + s of the stage in MFMA step s, for A and B alike: a lane's 16
// values of a tile row are four contiguous 16-byte reads instead of 16 strided dwords. 2 x 128 x 36 x 4 B x 2 stages = 72 KiB of
// LDS: two workgroups per CU. The tile index is linear in gridDim.x with the QUERY tile running fastest, so the workgroups resident
// together share few gallery tiles and all query tiles (the queries are the small side) and Ng is not bounded by gridDim.y.
#include "common.h"
#include "sqdist_row.h"

namespace {

constexpr int GT = 128;                 // tile rows of either operand
constexpr int KT = 32;                  // floats of K per stage
constexpr int LS = KT + 4;              // LDS row stride (floats)
constexpr int STAGE_F = 2 * GT * LS;    // floats per stage: the gallery tile, then the query tile
constexpr int GEMM_LDS_BYTES = 2 * STAGE_F * (int)sizeof(float);

// four consecutive floats of row `row` from column k on; zero past the operand's rows and past the row's end (never read there).
// VEC: n is a multiple of 4 and the base 16-byte aligned, so the four are one aligned load that is inside the row or outside it.
template <bool VEC>
__device__ __forceinline__ f32x4 load_k4(const float* __restrict__ base, int row, int nrows, int k, int n) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row >= nrows || k >= n) return v;
    const float* p = base + (size_t)row * n + k;
    if (VEC) return *reinterpret_cast<const f32x4*>(p);
    v[0] = p[0];
    if (k + 1 < n) v[1] = p[1];
    if (k + 2 < n) v[2] = p[2];
    if (k + 3 < n) v[3] = p[3];
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void sqdist_gemm_kernel(const float* __restrict__ g, const float* __restrict__ q,
                                                              const float* __restrict__ gn, const float* __restrict__ qn,
                                                              float* __restrict__ D, int Ng, int Nq, int n, int tiles_q) {
    extern __shared__ float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hk = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int tile_g = blockIdx.x / tiles_q, tile_q = blockIdx.x - tile_g * tiles_q;
    const int g0 = tile_g * GT, q0 = tile_q * GT;

    // staging: 8 threads cover the 128 bytes of one row's stage, 32 rows per pass, 4 passes per operand
    const int srow = tid >> 3, sk = (tid & 7) * 4;
    f32x4 rg[4], rq[4];
    auto load_stage = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rg[i] = load_k4<VEC>(g, g0 + srow + 32 * i, Ng, k0 + sk, n);
            rq[i] = load_k4<VEC>(q, q0 + srow + 32 * i, Nq, k0 + sk, n);
        }
    };
    auto store_stage = [&](int buf) {
        float* a_s = smem + buf * STAGE_F;
        float* b_s = a_s + GT * LS;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<f32x4*>(a_s + (srow + 32 * i) * LS + sk) = rg[i];
            *reinterpret_cast<f32x4*>(b_s + (srow + 32 * i) * LS + sk) = rq[i];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    const int a_off = (64 * wm + l31) * LS + 16 * hk;                 // this lane's row of the first gallery MFMA tile
    const int b_off = GT * LS + (64 * wn + l31) * LS + 16 * hk;       // ... and of the first query MFMA tile

    const int stages = (n + KT - 1) / KT;
    load_stage(0);
    store_stage(0);
    __syncthreads();
    for (int s = 0; s < stages; ++s) {
        const int cur = s & 1;
        const float* st = smem + cur * STAGE_F;
        if (s + 1 < stages) load_stage((s + 1) * KT);
#pragma unroll
        for (int j = 0; j < 4; ++j) {       // 4 MFMA k-steps per 16-byte fragment read
            f32x4 fa[2], fb[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                fa[t] = *reinterpret_cast<const f32x4*>(st + a_off + 32 * t * LS + 4 * j);
                fb[t] = *reinterpret_cast<const f32x4*>(st + b_off + 32 * t * LS + 4 * j);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mt][e], fb[nt][e], acc[mt][nt], 0, 0, 0);
        }
        if (s + 1 < stages) store_stage(cur ^ 1);      // read last in stage s-1: every wave is past that stage's barrier
        __syncthreads();
    }

    // epilogue: accumulator register r of lane (l31, hk) is row (r & 3) + 8 (r >> 2) + 4 hk, column l31 of its 32 x 32 tile
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int col = q0 + 64 * wn + 32 * nt + l31;
        if (col >= Nq) continue;
        const float qv = qn[col];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = g0 + 64 * wm + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hk;
                if (row < Ng) D[(size_t)row * Nq + col] = fmaxf((gn[row] + qv) - 2.f * acc[mt][nt][r], 0.f);
            }
    }
}

// out[i] = sum_k x[i][k]^2: one wave per row, lane l takes k = l, l + 64, ... (coalesced) into one running sum of at most
// ceil(n / 64) squares, then a butterfly (pairwise) sum over the 64 lanes: within gamma_(ceil(n/64) + 7) of the exact sum.
__global__ __launch_bounds__(256) void row_sqnorm_kernel(const float* __restrict__ x, float* __restrict__ out, int N, int n) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const float* xr = x + (size_t)row * n;
    float s = 0.f;
    for (int k = lane; k < n; k += 64) s += xr[k] * xr[k];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) out[row] = s;
}

// one thread per pair: the value pairwise_sqdist_kernel writes at [pair_g[p]][pair_q[p]]
__global__ __launch_bounds__(256) void sqdist_pairs_kernel(const float* __restrict__ g, const float* __restrict__ q,
                                                           const int* __restrict__ pair_g, const int* __restrict__ pair_q,
                                                           float* __restrict__ out, int P, int n, int take_sqrt) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float s = witw_sqdist_row(g + (size_t)pair_g[p] * n, q + (size_t)pair_q[p] * n, n);
    out[p] = take_sqrt ? sqrtf(s) : s;
}

}  // namespace

extern "C" {

int witw_row_sqnorm(const float* x, float* out, int N, int n, void* stream) {
    WITW_CHECK_ARG(x && out, "row_sqnorm: null pointer");
    WITW_CHECK_ARG(N > 0 && n > 0 && n <= 12288, "row_sqnorm: bad shape N=%d n=%d", N, n);
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3(cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, x, out, N, n);
    WITW_CHECK_LAUNCH("row_sqnorm");
    return WITW_OK;
}

int witw_sqdist_gemm(const float* g, const float* q, const float* gn, const float* qn, float* D, int Ng, int Nq, int n, void* stream) {
    WITW_CHECK_ARG(g && q && gn && qn && D, "sqdist_gemm: null pointer");
    WITW_CHECK_ARG(Ng > 0 && Nq > 0 && n > 0 && n <= 12288, "sqdist_gemm: bad shape Ng=%d Nq=%d n=%d", Ng, Nq, n);
    const long long tiles_q = cdiv(Nq, GT), tiles = (long long)cdiv(Ng, GT) * tiles_q;
    WITW_CHECK_ARG(tiles <= 0x7fffffffLL, "sqdist_gemm: %lld tiles exceed the grid", tiles);
    const bool vec = (n & 3) == 0 && (((uintptr_t)g | (uintptr_t)q) & 15) == 0;
    static bool lds_set = false;
    if (!lds_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(sqdist_gemm_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_BYTES);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(sqdist_gemm_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_BYTES);
        lds_set = true;
    }
    if (vec)
        hipLaunchKernelGGL(sqdist_gemm_kernel<true>, dim3((unsigned)tiles), dim3(256), GEMM_LDS_BYTES, (hipStream_t)stream, g, q, gn, qn, D,
                           Ng, Nq, n, (int)tiles_q);
    else
        hipLaunchKernelGGL(sqdist_gemm_kernel<false>, dim3((unsigned)tiles), dim3(256), GEMM_LDS_BYTES, (hipStream_t)stream, g, q, gn, qn, D,
                           Ng, Nq, n, (int)tiles_q);
    WITW_CHECK_LAUNCH("sqdist_gemm");
    return WITW_OK;
}

int witw_sqdist_pairs(const float* g, const float* q, const int* pair_g, const int* pair_q, float* out, int P, int n, int take_sqrt,
                      void* stream) {
    WITW_CHECK_ARG(P >= 0 && n > 0 && n <= 12288, "sqdist_pairs: bad shape P=%d n=%d", P, n);
    if (P == 0) return WITW_OK;
    WITW_CHECK_ARG(g && q && pair_g && pair_q && out, "sqdist_pairs: null pointer");
    hipLaunchKernelGGL(sqdist_pairs_kernel, dim3(cdiv(P, 256)), dim3(256), 0, (hipStream_t)stream, g, q, pair_g, pair_q, out, P, n,
                       take_sqrt);
    WITW_CHECK_LAUNCH("sqdist_pairs");
    return WITW_OK;
}

}  // extern "C"
