// Batch-hard soft-margin triplet loss (Hermans et al. 2017, "In Defense of the Triplet Loss") over the distance matrix of
// match, and the pair-list backward of match that its gradient needs (gfx950).
//
//   Dm = D with the diagonal set to +inf
//   rv[i], ri[i] = min / argmin of row i of Dm      (overhead anchor i -> hardest negative surface)
//   cv[j], ci[j] = min / argmin of column j of Dm   (surface anchor j -> hardest negative overhead)
//   loss = ( sum_i softplus(a(d_i - rv_i)) + sum_j softplus(a(d_j - cv_j)) ) / (2B),  softplus(x) = log(1+exp(x)) as written
//
// Selection rule (torch.min): a NaN is the minimum, at the first NaN's index; otherwise the smallest value, ties to the lowest
// index. The masked diagonal takes part as +inf at its own index, as in the masked_fill restatement.
// The mined indices are constants for the gradient, so dL/dD has at most 3B non-zeros:
//   +w_r[i] + w_c[i] at (i,i),  -w_r[i] at (i, ri[i]),  -w_c[j] at (ci[j], j),   w_r[i] = g a/(2B) sigmoid(a(d_i - rv_i)), w_c alike.
// match_bwd_pairs turns such a pair list into the embedding gradients without a dense [Bo,Bs] gradient matrix.
// Every reduction runs in a fixed order and nothing uses atomics: results are bitwise reproducible run to run.
#include "loss_kernels.h"

namespace {

constexpr int NO_INDEX = 0x7fffffff;      // "nothing seen yet": loses every comparison, written out as -1
constexpr int COL_ROWS = 64;              // rows per column-minimum partial (one workgroup = 64 columns x 64 rows)
constexpr int PAIRS_MAX = 8192;           // pair-list length one segment-building workgroup sorts in LDS (64 KB of keys)

// true iff (a, ia) is selected over (b, ib)
__device__ __forceinline__ bool better(float a, int ia, float b, int ib) {
    const bool an = a != a, bn = b != b;
    if (an != bn) return an;
    if (an) return ia < ib;
    if (a != b) return a < b;
    return ia < ib;
}

__device__ __forceinline__ long long out_index(int i) { return i == NO_INDEX ? -1ll : (long long)i; }

// Row minima of a column slab D[Bo][Bs] holding the global columns [col0, col0+Bs): one wave per row, lanes stride over the
// columns, then a 64-lane (value, index) butterfly (the rule is a total order, so every lane ends with the same pair).
__global__ __launch_bounds__(256) void hard_row_min_kernel(const float* __restrict__ D, float* __restrict__ rv,
                                                            long long* __restrict__ ri, int Bo, int Bs, int col0) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= Bo) return;      // wave-uniform
    const float* row = D + (size_t)i * Bs;
    float v = __builtin_inff();
    int ix = NO_INDEX;
    for (int j = lane; j < Bs; j += 64) {
        const int c = col0 + j;
        const float d = c == i ? __builtin_inff() : row[j];
        if (better(d, c, v, ix)) { v = d; ix = c; }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const float ov = __shfl_xor(v, m, 64);
        const int oi = __shfl_xor(ix, m, 64);
        if (better(ov, oi, v, ix)) { v = ov; ix = oi; }
    }
    if (lane == 0) {
        rv[i] = v;
        ri[i] = out_index(ix);
    }
}

// Column-minimum partials: workgroup (x, y) covers columns [64x, 64x+64) and rows [64y, 64y+64); lane = column (coalesced
// loads), wave w walks 16 rows in order, the four waves are merged in row order through LDS -> part[y][column].
__global__ __launch_bounds__(256) void hard_col_min_part_kernel(const float* __restrict__ D, float* __restrict__ pv,
                                                                 int* __restrict__ pi, int Bo, int Bs, int col0) {
    __shared__ float sv[4][64];
    __shared__ int si[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const int r0 = blockIdx.y * COL_ROWS + w * (COL_ROWS / 4);
    const int r1 = min(Bo, r0 + COL_ROWS / 4);
    float v = __builtin_inff();
    int ix = NO_INDEX;
    if (j < Bs) {
        const int c = col0 + j;
        for (int i = r0; i < r1; ++i) {
            const float d = i == c ? __builtin_inff() : D[(size_t)i * Bs + j];
            if (better(d, i, v, ix)) { v = d; ix = i; }
        }
    }
    sv[w][lane] = v;
    si[w][lane] = ix;
    __syncthreads();
    if (w == 0 && j < Bs) {
        for (int k = 1; k < 4; ++k)
            if (better(sv[k][lane], si[k][lane], v, ix)) { v = sv[k][lane]; ix = si[k][lane]; }
        pv[(size_t)blockIdx.y * Bs + j] = v;
        pi[(size_t)blockIdx.y * Bs + j] = ix;
    }
}

// The R row-chunk partials of every column merged in chunk order.
__global__ __launch_bounds__(256) void hard_col_min_merge_kernel(const float* __restrict__ pv, const int* __restrict__ pi,
                                                                  float* __restrict__ cv, long long* __restrict__ ci, int Bs, int R) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Bs) return;
    float v = __builtin_inff();
    int ix = NO_INDEX;
    for (int r = 0; r < R; ++r) {
        const float d = pv[(size_t)r * Bs + j];
        const int di = pi[(size_t)r * Bs + j];
        if (better(d, di, v, ix)) { v = d; ix = di; }
    }
    cv[j] = v;
    ci[j] = out_index(ix);
}

// Per-rank row minima [w][B] (global column indices, -1 = none) reduced in rank order.
__global__ __launch_bounds__(256) void hard_merge_rows_kernel(const float* __restrict__ pv, const long long* __restrict__ pi,
                                                               float* __restrict__ rv, long long* __restrict__ ri, int w, int B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    float v = __builtin_inff();
    int ix = NO_INDEX;
    for (int r = 0; r < w; ++r) {
        const long long li = pi[(size_t)r * B + i];
        if (li < 0) continue;
        const float d = pv[(size_t)r * B + i];
        if (better(d, (int)li, v, ix)) { v = d; ix = (int)li; }
    }
    rv[i] = v;
    ri[i] = out_index(ix);
}

// The loss and the gradient's pair list from the mined minima are hard_loss_kernel<FovTerm> and hard_pairs_kernel<FovTerm>
// (loss_kernels.h).

// Dense dL/dD of the full form (the stand-alone differentiable loss): the three kinds of non-zeros of the pair list, zero elsewhere.
__global__ __launch_bounds__(256) void hard_bwd_dense_kernel(const float* __restrict__ D, const float* __restrict__ rv,
                                                              const long long* __restrict__ ri, const float* __restrict__ cv,
                                                              const long long* __restrict__ ci, const float* __restrict__ gloss,
                                                              float* __restrict__ gD, int B, FovTerm term) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)B * B) return;
    const int i = (int)(idx / B), j = (int)(idx - (size_t)i * B);
    const float sc = term.scale(gloss[0], 2.f * B);
    const bool on_row = ri[i] == j, on_col = ci[j] == i;
    float g = 0.f;
    if (i == j || on_row) {
        const float wr = sc * term.deriv(D[(size_t)i * B + i] - rv[i]);
        if (i == j) g += wr;
        if (on_row) g -= wr;
    }
    if (i == j || on_col) {
        const float wc = sc * term.deriv(D[(size_t)j * B + j] - cv[j]);
        if (i == j) g += wc;
        if (on_col) g -= wc;
    }
    gD[idx] = g;
}

// ---- match_bwd_pairs: per-row segments of the pair list without atomics. Workgroup 0 sorts the keys (o, s, pair) and
// workgroup 1 the keys (s, o, pair) with a bitonic sort in LDS; each segment then lists its partners in ascending order
// (duplicate pairs in list order). Pairs with an index out of range (e.g. -1) sort behind every valid key and are dropped.
// Outputs: ord[2][n] pair numbers in segment order, seg_o[2][Bo] / seg_s[2][Bs] = (begin, end) of each row's segment.
__global__ __launch_bounds__(1024) void pairs_segments_kernel(const int* __restrict__ po, const int* __restrict__ ps, int n, int npad,
                                                              int Bo, int Bs, int* __restrict__ ord, int* __restrict__ seg_o,
                                                              int* __restrict__ seg_s) {
    extern __shared__ unsigned long long keys[];
    const bool by_s = blockIdx.x == 1;
    const int nrows = by_s ? Bs : Bo;
    int* seg = by_s ? seg_s : seg_o;
    int* order = ord + (by_s ? n : 0);
    const int tid = threadIdx.x;
    for (int r = tid; r < 2 * nrows; r += 1024) seg[r] = 0;
    for (int p = tid; p < npad; p += 1024) {
        unsigned long long k = ~0ull;
        if (p < n) {
            const int o = po[p], s = ps[p];
            if (o >= 0 && o < Bo && s >= 0 && s < Bs) {
                const unsigned long long a = (unsigned)(by_s ? s : o), b = (unsigned)(by_s ? o : s);
                k = (a << 34) | (b << 13) | (unsigned long long)p;
            }
        }
        keys[p] = k;
    }
    __syncthreads();
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npad; i += 1024) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned long long a = keys[i], b = keys[x];
                    if ((a > b) == ((i & k) == 0)) {
                        keys[i] = b;
                        keys[x] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int q = tid; q < n; q += 1024) {
        const unsigned long long k = keys[q];
        order[q] = k == ~0ull ? -1 : (int)(k & 8191ull);
        if (k == ~0ull) continue;
        const int row = (int)(k >> 34);
        if (q == 0 || (keys[q - 1] >> 34) != (unsigned long long)row) seg[2 * row] = q;
        if (q == n - 1 || keys[q + 1] == ~0ull || (keys[q + 1] >> 34) != (unsigned long long)row) seg[2 * row + 1] = q + 1;
    }
}

// grad_su: one workgroup per surface s sums its segment in order (the terms of match_bwd_su_kernel, csrc/match.hip). The
// per-pair scalars of 256 segment entries at a time are staged in LDS first, so that the loads of consecutive overhead rows in
// the inner loop do not wait on one another (a surface that is the hardest negative of many anchors has a long segment).
__global__ __launch_bounds__(256) void pairs_bwd_su_kernel(const float* __restrict__ ov, const float* __restrict__ su,
                                                            const long long* __restrict__ ori, const float* __restrict__ score,
                                                            const float* __restrict__ wn, const float* __restrict__ sn,
                                                            const int* __restrict__ po, const float* __restrict__ pw,
                                                            const int* __restrict__ ord, const int* __restrict__ seg,
                                                            float* __restrict__ gsu, int Bs, int We) {
    __shared__ float coef[256];
    __shared__ int rot[256];
    __shared__ int orow[256];
    __shared__ float part[4];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int E = 64 * We;
    const float sns = sn[s];
    int ch[16], kk[16];
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int e = tid + 256 * i;
        ch[i] = e / We;
        kk[i] = e - ch[i] * We;
        acc[i] = 0.f;
    }
    float self = 0.f;
    const int q0 = seg[2 * s], q1 = seg[2 * s + 1];
    for (int c0 = q0; c0 < q1; c0 += 256) {
        const int q = c0 + tid;
        __syncthreads();
        if (q < q1) {
            const int p = ord[q];
            const int o = po[p];
            const float g = pw[p];
            const size_t off = (size_t)o * Bs + s;
            const int t = (int)ori[off];
            const float w = wn[(size_t)o * 64 + t];
            coef[tid] = g * (-2.f / (w * sns));
            rot[tid] = t;
            orow[tid] = o;
            self += g * (2.f * score[off] / (w * sns * sns * sns));
        }
        __syncthreads();
        const int n = min(256, q1 - c0);
        for (int j = 0; j < n; ++j) {
            const float a = coef[j];
            const int t = rot[j];
            const float* row = ov + (size_t)orow[j] * 4096;
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (tid + 256 * i < E) acc[i] += a * row[ch[i] * 64 + ((kk[i] + t) & 63)];
        }
    }
    const float selfsum = block_sum_256(self, part);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int e = tid + 256 * i;
        if (e < E) gsu[(size_t)s * E + e] = acc[i] + su[(size_t)s * E + e] * selfsum;
    }
}

// grad_ov: one workgroup per overhead o sums its segment in order, scattered into the window columns (k + t) mod 64
// (the terms of match_bwd_ov_kernel, csrc/match.hip); per-pair scalars staged in LDS as above.
__global__ __launch_bounds__(256) void pairs_bwd_ov_kernel(const float* __restrict__ ov, const float* __restrict__ su,
                                                            const long long* __restrict__ ori, const float* __restrict__ score,
                                                            const float* __restrict__ wn, const float* __restrict__ sn,
                                                            const int* __restrict__ ps, const float* __restrict__ pw,
                                                            const int* __restrict__ ord, const int* __restrict__ seg,
                                                            float* __restrict__ gov, int Bs, int We) {
    __shared__ float coef[256];
    __shared__ float coef2[256];
    __shared__ int rot[256];
    __shared__ int srow[256];
    const int o = blockIdx.x, tid = threadIdx.x;
    const int w = tid & 63, cg = tid >> 6;   // element (ch = cg + 4*i, w)
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    float beta = 0.f;
    const int q0 = seg[2 * o], q1 = seg[2 * o + 1];
    for (int c0 = q0; c0 < q1; c0 += 256) {
        const int q = c0 + tid;
        __syncthreads();
        if (q < q1) {
            const int p = ord[q];
            const int s = ps[p];
            const float g = pw[p];
            const size_t off = (size_t)o * Bs + s;
            const int t = (int)ori[off];
            const float wv = wn[(size_t)o * 64 + t];
            const float sv = sn[s];
            coef[tid] = g * (-2.f / (wv * sv));
            coef2[tid] = g * (2.f * score[off] / (wv * wv * wv * sv));
            rot[tid] = t;
            srow[tid] = s;
        }
        __syncthreads();
        const int n = min(256, q1 - c0);
        for (int j = 0; j < n; ++j) {
            const int k = (w - rot[j]) & 63;
            if (k < We) {
                const float a = coef[j];
                beta += coef2[j];
                const float* base = su + (size_t)srow[j] * 64 * We + k;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] += a * base[(cg + 4 * i) * We];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const size_t e = (size_t)o * 4096 + (cg + 4 * i) * 64 + w;
        gov[e] = acc[i] + ov[e] * beta;
    }
}

int next_pow2(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

int launch_mine(const float* D, int Bo, int Bs, int col0, float* rv, long long* ri, float* cv, long long* ci, void* workspace,
                hipStream_t st) {
    const int R = cdiv(Bo, COL_ROWS);
    float* pv = (float*)workspace;
    int* pi = (int*)(pv + (size_t)R * Bs);
    hipLaunchKernelGGL(hard_row_min_kernel, dim3(cdiv(Bo, 4)), dim3(256), 0, st, D, rv, ri, Bo, Bs, col0);
    hipLaunchKernelGGL(hard_col_min_part_kernel, dim3(cdiv(Bs, 64), R), dim3(256), 0, st, D, pv, pi, Bo, Bs, col0);
    hipLaunchKernelGGL(hard_col_min_merge_kernel, dim3(cdiv(Bs, 256)), dim3(256), 0, st, pv, pi, cv, ci, Bs, R);
    return WITW_OK;
}

}  // namespace

extern "C" {

long long witw_batch_hard_workspace_bytes(int Bo, int Bs) {
    if (Bo < 2 || Bs < 1) return -1;
    return (long long)cdiv(Bo, COL_ROWS) * Bs * (sizeof(float) + sizeof(int));
}

int witw_batch_hard_fwd(const float* distance, int B, float alpha, float* rv, long long* ri, float* cv, long long* ci, float* loss,
                        void* workspace, void* stream) {
    WITW_CHECK_ARG(distance && rv && ri && cv && ci && loss && workspace, "batch_hard_fwd: null pointer");
    WITW_CHECK_ARG(B >= 2, "batch_hard_fwd: batch %d < 2 (every anchor needs a negative)", B);
    hipStream_t st = (hipStream_t)stream;
    launch_mine(distance, B, B, 0, rv, ri, cv, ci, workspace, st);
    hipLaunchKernelGGL(hard_loss_kernel<FovTerm>, dim3(1), dim3(256), 0, st, distance, rv, cv, loss, B, 0, FovTerm{alpha}, 2.f * B);
    WITW_CHECK_LAUNCH("batch_hard_fwd");
    return WITW_OK;
}

int witw_batch_hard_slab_mine(const float* distance, int Bo, int Bs, int col0, float* rv, long long* ri, float* cv, long long* ci,
                              void* workspace, void* stream) {
    WITW_CHECK_ARG(distance && rv && ri && cv && ci && workspace, "batch_hard_slab_mine: null pointer");
    WITW_CHECK_ARG(Bo >= 2, "batch_hard_slab_mine: batch %d < 2 (every anchor needs a negative)", Bo);
    WITW_CHECK_ARG(Bs >= 1 && col0 >= 0 && col0 + Bs <= Bo, "batch_hard_slab_mine: bad slab Bo=%d Bs=%d col0=%d", Bo, Bs, col0);
    launch_mine(distance, Bo, Bs, col0, rv, ri, cv, ci, workspace, (hipStream_t)stream);
    WITW_CHECK_LAUNCH("batch_hard_slab_mine");
    return WITW_OK;
}

int witw_batch_hard_merge_rows(const float* rv_parts, const long long* ri_parts, int n_parts, int B, float* rv, long long* ri,
                               void* stream) {
    WITW_CHECK_ARG(rv_parts && ri_parts && rv && ri, "batch_hard_merge_rows: null pointer");
    WITW_CHECK_ARG(B >= 2, "batch_hard_merge_rows: batch %d < 2", B);
    WITW_CHECK_ARG(n_parts >= 1, "batch_hard_merge_rows: shape mismatch, %d parts", n_parts);
    hipLaunchKernelGGL(hard_merge_rows_kernel, dim3(cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, rv_parts, ri_parts, rv, ri,
                       n_parts, B);
    WITW_CHECK_LAUNCH("batch_hard_merge_rows");
    return WITW_OK;
}

int witw_batch_hard_slab_loss(const float* distance, const float* rv, const float* cv, int Bo, int Bs, int col0, float alpha,
                              float* partial, void* stream) {
    WITW_CHECK_ARG(distance && rv && cv && partial, "batch_hard_slab_loss: null pointer");
    WITW_CHECK_ARG(Bo >= 2, "batch_hard_slab_loss: batch %d < 2", Bo);
    WITW_CHECK_ARG(Bs >= 1 && col0 >= 0 && col0 + Bs <= Bo, "batch_hard_slab_loss: bad slab Bo=%d Bs=%d col0=%d", Bo, Bs, col0);
    hipLaunchKernelGGL(hard_loss_kernel<FovTerm>, dim3(1), dim3(256), 0, (hipStream_t)stream, distance, rv, cv, partial, Bs, col0,
                       FovTerm{alpha}, 1.f);
    WITW_CHECK_LAUNCH("batch_hard_slab_loss");
    return WITW_OK;
}

int witw_batch_hard_pairs(const float* diag, const float* rv, const long long* ri, const float* cv, const long long* ci,
                          const float* grad_loss, int B, int Bs, int col0, float alpha, int* pair_o, int* pair_s, float* pair_w,
                          void* stream) {
    WITW_CHECK_ARG(diag && rv && ri && cv && ci && grad_loss && pair_o && pair_s && pair_w, "batch_hard_pairs: null pointer");
    WITW_CHECK_ARG(B >= 2, "batch_hard_pairs: batch %d < 2", B);
    WITW_CHECK_ARG(Bs >= 1 && col0 >= 0 && col0 + Bs <= B, "batch_hard_pairs: bad slab B=%d Bs=%d col0=%d", B, Bs, col0);
    hipLaunchKernelGGL(hard_pairs_kernel<FovTerm>, dim3(cdiv(2 * Bs + B, 256)), dim3(256), 0, (hipStream_t)stream, diag, rv, ri, cv, ci,
                       grad_loss, pair_o, pair_s, pair_w, B, Bs, col0, FovTerm{alpha});
    WITW_CHECK_LAUNCH("batch_hard_pairs");
    return WITW_OK;
}

int witw_batch_hard_bwd(const float* distance, const float* rv, const long long* ri, const float* cv, const long long* ci,
                        const float* grad_loss, float* grad_distance, int B, float alpha, void* stream) {
    WITW_CHECK_ARG(distance && rv && ri && cv && ci && grad_loss && grad_distance, "batch_hard_bwd: null pointer");
    WITW_CHECK_ARG(B >= 2, "batch_hard_bwd: batch %d < 2", B);
    const size_t total = (size_t)B * B;
    WITW_CHECK_ARG((total + 255) / 256 <= 0x7fffffffULL, "batch_hard_bwd: B=%d too large", B);
    hipLaunchKernelGGL(hard_bwd_dense_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, distance, rv,
                       ri, cv, ci, grad_loss, grad_distance, B, FovTerm{alpha});
    WITW_CHECK_LAUNCH("batch_hard_bwd");
    return WITW_OK;
}

long long witw_match_bwd_pairs_scratch_bytes(int n_pairs, int Bo, int Bs) {
    if (n_pairs < 1 || n_pairs > PAIRS_MAX || Bo < 1 || Bs < 1) return -1;
    return (long long)(2 * n_pairs + 2 * Bo + 2 * Bs) * sizeof(int);
}

int witw_match_bwd_pairs(const float* ov, const float* su, const long long* orientation, const float* score, const float* workspace,
                         const int* pair_o, const int* pair_s, const float* pair_w, int n_pairs, int Bo, int Bs, int We,
                         float* grad_ov, float* grad_su, void* scratch, void* stream) {
    WITW_CHECK_ARG(ov && su && orientation && score && workspace && pair_o && pair_s && pair_w && grad_ov && grad_su && scratch,
                   "match_bwd_pairs: null pointer");
    WITW_CHECK_ARG(Bo > 0 && Bs > 0 && We >= 1 && We <= 64 && Bo < (1 << 21) && Bs < (1 << 21),
                   "match_bwd_pairs: bad shape Bo=%d Bs=%d We=%d", Bo, Bs, We);
    WITW_CHECK_ARG(n_pairs >= 1 && n_pairs <= PAIRS_MAX, "match_bwd_pairs: %d pairs outside [1,%d]", n_pairs, PAIRS_MAX);
    hipStream_t st = (hipStream_t)stream;
    const float* wn = workspace;
    const float* sn = workspace + (size_t)Bo * 64;
    int* ord = (int*)scratch;
    int* seg_o = ord + 2 * n_pairs;
    int* seg_s = seg_o + 2 * Bo;
    const int npad = next_pow2(n_pairs);
    hipLaunchKernelGGL(pairs_segments_kernel, dim3(2), dim3(1024), npad * sizeof(unsigned long long), st, pair_o, pair_s, n_pairs,
                       npad, Bo, Bs, ord, seg_o, seg_s);
    hipLaunchKernelGGL(pairs_bwd_su_kernel, dim3(Bs), dim3(256), 0, st, ov, su, orientation, score, wn, sn, pair_o, pair_w,
                       ord + n_pairs, seg_s, grad_su, Bs, We);
    hipLaunchKernelGGL(pairs_bwd_ov_kernel, dim3(Bo), dim3(256), 0, st, ov, su, orientation, score, wn, sn, pair_s, pair_w, ord,
                       seg_o, grad_ov, Bs, We);
    WITW_CHECK_LAUNCH("match_bwd_pairs");
    return WITW_OK;
}

}  // extern "C"
