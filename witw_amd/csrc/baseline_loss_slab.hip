// cvig_baseline's exhaustive minibatch triplet loss (model/cvig_baseline.py:286-315) on a COLUMN SLAB of the global batch (gfx950):
// what one rank evaluates when the batch of B pairs is spread over the ranks, b pairs each (the reference gathers the
// nn.DataParallel replicas' embeddings and takes the loss over all B, :339-343).
//
//   x [B,n]  the all-gathered embeddings of one side, y [b,n] this rank's embeddings of the other side, col0 = rank * b
//   T [B,b]  T[g][c] = |x_g - y_c|^2 (witw_pairwise_sqdist); column c is column col0 + c of the global matrix
//   diag [B] diag[k] = T_k[k][k - col0_k] of the rank that owns column k, all-gathered
//   l, l' = BaselineTerm's value and derivative (loss_terms.h: the dense kernels' own); the kernels are loss_kernels.h's
//
//   partial   = sum_c sum_{g != col0+c} l(diag[col0+c] - T[g][c]) + l(diag[g] - T[g][c])        (over the ranks: / 2B(B-1) = the loss)
//   colsig[c] = sum_{g != col0+c} l'(diag[col0+c] - T[g][c])                                   (complete on this rank)
//   rowsig[g] = sum_{c : col0+c != g} l'(diag[g] - T[g][c])                                    (summed over the ranks by the caller)
//   G[g][c]   = -(l'(diag[col0+c] - T[g][c]) + l'(diag[g] - T[g][c])) sc,  G[col0+c][c] = (rowsig[col0+c] + colsig[c]) sc
//   dx[g]     = 2 sum_c G[g][c] (x_g - y_c),   dy[c] = 2 sum_g G[g][c] (y_c - x_g)
//
// Every sum runs in a fixed order (a thread's strided or serial partial, the wave shuffle tree, four wave totals) and nothing
// is accumulated with atomics: the same call gives the same bits.
#include "loss_kernels.h"

namespace {

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
    hipLaunchKernelGGL(slab_partials_kernel<BaselineTerm>, dim3(B), dim3(256), 0, st, T, diag, workspace, b, col0,
                       BaselineTerm{soft_margin, alpha, margin});
    hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(256), 0, st, workspace, partial, B, 1.f);
    WITW_CHECK_LAUNCH("exhaustive_loss_slab_fwd");
    witw_note_variant("exhaustive_slab_partials_kernel");
    return WITW_OK;
}

int witw_exhaustive_loss_slab_sig(const float* T, const float* diag, int B, int b, int col0, int soft_margin, float alpha, float margin,
                                  float* rowsig, float* colsig, void* stream) {
    WITW_CHECK_ARG(T && diag && rowsig && colsig, "exhaustive_loss_slab_sig: null pointer");
    WITW_CHECK_ARG(slab_ok(B, b, col0), "exhaustive_loss_slab_sig: bad slab B=%d b=%d col0=%d", B, b, col0);
    hipLaunchKernelGGL(slab_sig_kernel<BaselineTerm>, dim3(B + b), dim3(256), 0, (hipStream_t)stream, T, diag, rowsig, colsig, B, b, col0,
                       BaselineTerm{soft_margin, alpha, margin});
    WITW_CHECK_LAUNCH("exhaustive_loss_slab_sig");
    witw_note_variant("exhaustive_slab_sig_kernel");
    return WITW_OK;
}

int witw_exhaustive_loss_slab_bwd(const float* T, const float* diag, const float* rowsig, const float* colsig, const float* grad_loss,
                                  float* G, int B, int b, int col0, int soft_margin, float alpha, float margin, void* stream) {
    WITW_CHECK_ARG(T && diag && rowsig && colsig && grad_loss && G, "exhaustive_loss_slab_bwd: null pointer");
    WITW_CHECK_ARG(slab_ok(B, b, col0), "exhaustive_loss_slab_bwd: bad slab B=%d b=%d col0=%d", B, b, col0);
    const size_t total = (size_t)B * b;
    hipLaunchKernelGGL(slab_bwd_kernel<BaselineTerm>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, T, diag,
                       rowsig, colsig, grad_loss, G, B, b, col0, BaselineTerm{soft_margin, alpha, margin});
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
