// cvig_baseline's exhaustive minibatch triplet loss (model/cvig_baseline.py:286-315) on a COLUMN SLAB of the global batch (gfx950):
// what one rank evaluates when the batch of B pairs is spread over the ranks, b pairs each (the reference gathers the
// nn.DataParallel replicas' embeddings and takes the loss over all B, :339-343).
//
//   x [B,n]  the all-gathered embeddings of one side, y [b,n] this rank's embeddings of the other side, col0 = rank * b
//   T [B,b]  T[g][c] = |x_g - y_c|^2 (witw_pairwise_sqdist); column c is column col0 + c of the global matrix
//   diag [B] diag[k] = T_k[k][k - col0_k] of the rank that owns column k, all-gathered
//   l = trip, l' = trip_d (exhaustive_terms.h: the dense kernels' own)
//
//   partial   = sum_c sum_{g != col0+c} l(diag[col0+c] - T[g][c]) + l(diag[g] - T[g][c])        (over the ranks: / 2B(B-1) = the loss)
//   colsig[c] = sum_{g != col0+c} l'(diag[col0+c] - T[g][c])                                   (complete on this rank)
//   rowsig[g] = sum_{c : col0+c != g} l'(diag[g] - T[g][c])                                    (summed over the ranks by the caller)
//   G[g][c]   = -(l'(diag[col0+c] - T[g][c]) + l'(diag[g] - T[g][c])) sc,  G[col0+c][c] = (rowsig[col0+c] + colsig[c]) sc
//   dx[g]     = 2 sum_c G[g][c] (x_g - y_c),   dy[c] = 2 sum_g G[g][c] (y_c - x_g)
//
// Every sum runs in a fixed order (a thread's strided or serial partial, the wave shuffle tree, four wave totals) and nothing
// is accumulated with atomics: the same call gives the same bits.
#include "common.h"
#include "exhaustive_terms.h"

namespace {

__device__ __forceinline__ float slab_block_sum(float v, float* sh) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// part[g] = row g's share of `partial`; one block per row of the slab
__global__ __launch_bounds__(256) void exhaustive_slab_partials_kernel(const float* __restrict__ T, const float* __restrict__ diag,
                                                                        float* __restrict__ part, int b, int col0, int soft,
                                                                        float alpha, float margin) {
    __shared__ float sh[4];
    const int g = blockIdx.x;
    const float dgg = diag[g];
    float s = 0.f;
    for (int c = threadIdx.x; c < b; c += 256) {
        if (col0 + c == g) continue;
        const float t = T[(size_t)g * b + c];
        s += trip(diag[col0 + c] - t, soft, alpha, margin);
        s += trip(dgg - t, soft, alpha, margin);
    }
    const float tot = slab_block_sum(s, sh);
    if (threadIdx.x == 0) part[g] = tot;
}

__global__ __launch_bounds__(256) void exhaustive_slab_sum_kernel(const float* __restrict__ part, float* __restrict__ out, int n) {
    __shared__ float sh[4];
    float s = 0.f;
    for (int t = threadIdx.x; t < n; t += 256) s += part[t];
    const float tot = slab_block_sum(s, sh);
    if (threadIdx.x == 0) out[0] = tot;
}

// blocks [0,B): rowsig[g] over this slab's columns; blocks [B,B+b): colsig[c] over all rows
__global__ __launch_bounds__(256) void exhaustive_slab_sig_kernel(const float* __restrict__ T, const float* __restrict__ diag,
                                                                   float* __restrict__ rowsig, float* __restrict__ colsig, int B, int b,
                                                                   int col0, int soft, float alpha, float margin) {
    __shared__ float sh[4];
    const bool is_col = blockIdx.x >= (unsigned)B;
    const int m = is_col ? blockIdx.x - B : blockIdx.x;
    const int own = is_col ? col0 + m : m;               // the global index whose diagonal entry is the positive distance
    const float dm = diag[own];
    const int cnt = is_col ? B : b;
    float s = 0.f;
    for (int t = threadIdx.x; t < cnt; t += 256) {
        if ((is_col ? t : col0 + t) == own) continue;
        const float d = is_col ? T[(size_t)t * b + m] : T[(size_t)m * b + t];
        s += trip_d(dm - d, soft, alpha, margin);
    }
    const float tot = slab_block_sum(s, sh);
    if (threadIdx.x == 0) (is_col ? colsig : rowsig)[m] = tot;
}

__global__ void exhaustive_slab_bwd_kernel(const float* __restrict__ T, const float* __restrict__ diag, const float* __restrict__ rowsig,
                                           const float* __restrict__ colsig, const float* __restrict__ gloss, float* __restrict__ G, int B,
                                           int b, int col0, int soft, float alpha, float margin) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * b) return;
    const int g = idx / b, c = idx - (size_t)g * b;
    const float sc = gloss[0] / (2.f * B * (B - 1));
    if (g == col0 + c) {
        G[idx] = (rowsig[g] + colsig[c]) * sc;
        return;
    }
    const float t = T[idx];
    G[idx] = -(trip_d(diag[col0 + c] - t, soft, alpha, margin) + trip_d(diag[g] - t, soft, alpha, margin)) * sc;
}

// out[r][k] = 2 sum_q Gm(r, q) (self[r][k] - other[q][k]), Gm(r, q) = G[r * g_row + q * g_other]: dx with (g_row, g_other) = (b, 1),
// dy with (1, b). A workgroup owns R output rows x 256 columns k: a lane keeps its R sums and its R self values in registers, so
// one read of other[q][k] (coalesced over the lanes) serves R rows -- others * n * ceil(rows / R) reads in all, where one block
// per output row (sqdist_bwd_kernel) makes others * n * rows; the R x RB_Q tile of G those rows share is staged through LDS and
// read back as R consecutive floats per q, the same address on every lane. The other side's rows are NOT staged: a lane only ever
// needs its own column of them, so the register reuse is all the reuse there is. q runs serially from 0: a fixed order.
constexpr int RB_Q = 64;

template <int R>
__global__ __launch_bounds__(256) void sqdist_rect_bwd_kernel(const float* __restrict__ self, const float* __restrict__ other,
                                                               const float* __restrict__ G, float* __restrict__ out, int rows,
                                                               int others, int n, int g_row, int g_other) {
    __shared__ __attribute__((aligned(16))) float sG[RB_Q][R];
    const int r0 = blockIdx.x * R;
    const int k = blockIdx.y * 256 + threadIdx.x;
    const bool live = k < n;
    float sv[R], acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        sv[r] = (live && r0 + r < rows) ? self[(size_t)(r0 + r) * n + k] : 0.f;
        acc[r] = 0.f;
    }
    for (int q0 = 0; q0 < others; q0 += RB_Q) {
        __syncthreads();                                  // the previous tile has been consumed
        for (int e = threadIdx.x; e < RB_Q * R; e += 256) {
            // consecutive lanes along the direction in which G is contiguous
            const int q = g_other == 1 ? e % RB_Q : e / R, r = g_other == 1 ? e / RB_Q : e % R;
            const bool in = q0 + q < others && r0 + r < rows;
            sG[q][r] = in ? G[(size_t)(r0 + r) * g_row + (size_t)(q0 + q) * g_other] : 0.f;       // rows past the end add nothing
        }
        __syncthreads();
        if (!live) continue;
        const int qn = min(RB_Q, others - q0);
#pragma unroll 4
        for (int q = 0; q < qn; ++q) {
            const float o = other[(size_t)(q0 + q) * n + k];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] += sG[q][r] * (sv[r] - o);
        }
    }
    if (!live) return;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (r0 + r < rows) out[(size_t)(r0 + r) * n + k] = 2.f * acc[r];
}

// 8 rows per workgroup once that still gives every CU a workgroup; below that 2, so that a short side (dy of a narrow slab) is not
// left to a handful of CUs
int launch_rect_bwd(const float* self, const float* other, const float* G, float* out, int rows, int others, int n, int g_row, int g_other,
                    hipStream_t st) {
    const int ks = cdiv(n, 256);
    if ((long long)cdiv(rows, 8) * ks >= 256) {
        hipLaunchKernelGGL(sqdist_rect_bwd_kernel<8>, dim3(cdiv(rows, 8), ks), dim3(256), 0, st, self, other, G, out, rows, others, n, g_row,
                           g_other);
        return 8;
    }
    hipLaunchKernelGGL(sqdist_rect_bwd_kernel<2>, dim3(cdiv(rows, 2), ks), dim3(256), 0, st, self, other, G, out, rows, others, n, g_row,
                       g_other);
    return 2;
}

bool slab_ok(int B, int b, int col0) { return B >= 2 && b >= 1 && b <= B && col0 >= 0 && col0 <= B - b; }

}  // namespace

extern "C" {

int witw_exhaustive_loss_slab_fwd(const float* T, const float* diag, int B, int b, int col0, int soft_margin, float alpha, float margin,
                                  float* partial, float* workspace, void* stream) {
    WITW_CHECK_ARG(T && diag && partial && workspace, "exhaustive_loss_slab_fwd: null pointer");
    WITW_CHECK_ARG(slab_ok(B, b, col0), "exhaustive_loss_slab_fwd: bad slab B=%d b=%d col0=%d", B, b, col0);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(exhaustive_slab_partials_kernel, dim3(B), dim3(256), 0, st, T, diag, workspace, b, col0, soft_margin, alpha, margin);
    hipLaunchKernelGGL(exhaustive_slab_sum_kernel, dim3(1), dim3(256), 0, st, workspace, partial, B);
    WITW_CHECK_LAUNCH("exhaustive_loss_slab_fwd");
    witw_note_variant("exhaustive_slab_partials_kernel");
    return WITW_OK;
}

int witw_exhaustive_loss_slab_sig(const float* T, const float* diag, int B, int b, int col0, int soft_margin, float alpha, float margin,
                                  float* rowsig, float* colsig, void* stream) {
    WITW_CHECK_ARG(T && diag && rowsig && colsig, "exhaustive_loss_slab_sig: null pointer");
    WITW_CHECK_ARG(slab_ok(B, b, col0), "exhaustive_loss_slab_sig: bad slab B=%d b=%d col0=%d", B, b, col0);
    hipLaunchKernelGGL(exhaustive_slab_sig_kernel, dim3(B + b), dim3(256), 0, (hipStream_t)stream, T, diag, rowsig, colsig, B, b, col0,
                       soft_margin, alpha, margin);
    WITW_CHECK_LAUNCH("exhaustive_loss_slab_sig");
    witw_note_variant("exhaustive_slab_sig_kernel");
    return WITW_OK;
}

int witw_exhaustive_loss_slab_bwd(const float* T, const float* diag, const float* rowsig, const float* colsig, const float* grad_loss,
                                  float* G, int B, int b, int col0, int soft_margin, float alpha, float margin, void* stream) {
    WITW_CHECK_ARG(T && diag && rowsig && colsig && grad_loss && G, "exhaustive_loss_slab_bwd: null pointer");
    WITW_CHECK_ARG(slab_ok(B, b, col0), "exhaustive_loss_slab_bwd: bad slab B=%d b=%d col0=%d", B, b, col0);
    const size_t total = (size_t)B * b;
    hipLaunchKernelGGL(exhaustive_slab_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, T, diag, rowsig,
                       colsig, grad_loss, G, B, b, col0, soft_margin, alpha, margin);
    WITW_CHECK_LAUNCH("exhaustive_loss_slab_bwd");
    witw_note_variant("exhaustive_slab_bwd_kernel");
    return WITW_OK;
}

int witw_sqdist_rect_bwd(const float* x, const float* y, const float* G, float* dx, float* dy, int B, int b, int n, void* stream) {
    WITW_CHECK_ARG(x && y && G, "sqdist_rect_bwd: null pointer");
    WITW_CHECK_ARG(dx || dy, "sqdist_rect_bwd: null pointer (dx and dy: at least one output)");
    WITW_CHECK_ARG(B >= 1 && b >= 1 && n >= 1 && n <= 12288, "sqdist_rect_bwd: bad shape B=%d b=%d n=%d", B, b, n);
    hipStream_t st = (hipStream_t)stream;
    int rx = 0, ry = 0;
    if (dx) rx = launch_rect_bwd(x, y, G, dx, B, b, n, b, 1, st);
    if (dy) ry = launch_rect_bwd(y, x, G, dy, b, B, n, 1, b, st);
    WITW_CHECK_LAUNCH("sqdist_rect_bwd");
    witw_note_variant("sqdist_rect_bwd_kernel<dx:%d,dy:%d>", rx, ry);
    return WITW_OK;
}

}  // extern "C"
