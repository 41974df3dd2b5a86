// Batch-hard form of cvig_baseline's triplet loss on a COLUMN SLAB of the global batch, and the pair-list backward of the squared
// Euclidean distance that its gradient needs (gfx950). The mining is loss_hard.hip's (witw_batch_hard_slab_mine /
// witw_batch_hard_merge_rows on the slab T of witw_pairwise_sqdist); this file holds what is the baseline's own:
//
//   x [B,n]  the all-gathered embeddings of one side, y [b,n] this rank's of the other, T[g][c] = |x_g - y_c|^2, column c = global
//            column col0 + c, d_k = the global diagonal, Tm = T with the diagonal at +inf
//   rv[i], ri[i] = min / argmin of global row i of Tm, cv[j], ci[j] = min / argmin of column j (global indices, constants for the gradient)
//   l, l' = BaselineTerm's hard_value and derivative (loss_terms.h: the exhaustive kernels' own; a NaN argument stays a NaN in l);
//   the loss and pair-list kernels are hard_loss_kernel / hard_pairs_kernel of loss_kernels.h
//
//   partial = sum_c l(d_{col0+c} - rv[col0+c]) + l(d_{col0+c} - cv[c])                          (over the ranks: / 2B = the loss)
//   sc = grad_loss / 2B,  w_r[i] = sc l'(d_i - rv_i),  w_c[j] = sc l'(d_j - cv_j)
//   dL/dT = +w_r[i] + w_c[i] at (i,i),  -w_r[i] at (i, ri[i]),  -w_c[j] at (ci[j], j):  at most 3B non-zeros, kept as a pair list
//   a pair (g, c, w) adds 2w (x_g - y_c) to dx[g] and 2w (y_c - x_g) to dy[c]
//
// Every sum runs in a fixed order (a thread's strided partial, the wave shuffle tree, four wave totals; the pairs of an output row
// in list order) and nothing is accumulated with atomics: the same call gives the same bits.
#include "loss_kernels.h"

namespace {

// out[r][k] = 2 sum over the pairs of row r, in list order, of w (self[r][k] - other[q][k]). Workgroups [0, nx) own the rows of dx
// (self = x, r = pair_g, q = pair_c), the others the rows of dy (self = y, r = pair_c, q = pair_g); blockIdx.y picks 256 columns k.
// The list is scanned 256 entries at a time: a thread tests one entry, and the entries of this row are packed, order kept (wave
// ballots, four wave counts), into LDS; then every lane walks the packed partners for its own column k, the loads of consecutive
// partners independent of one another. A row that is the partner of every pair (a hub column: the hardest negative of all B rows)
// so costs its workgroup P coalesced row reads and no other workgroup anything; a row without pairs is written as zeros.
constexpr int PB_CHUNK = 256;

__global__ __launch_bounds__(256) void sqdist_pairs_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                const int* __restrict__ pg, const int* __restrict__ pc,
                                                                const float* __restrict__ pw, int P, float* __restrict__ dx,
                                                                float* __restrict__ dy, int nx, int B, int b, int n) {
    __shared__ int sq[PB_CHUNK];
    __shared__ float sw[PB_CHUNK];
    __shared__ int cnt[4];
    const bool is_dy = blockIdx.x >= (unsigned)nx;      // workgroup-uniform
    const int r = is_dy ? blockIdx.x - nx : blockIdx.x;
    const float* self = is_dy ? y : x;
    const float* other = is_dy ? x : y;
    float* out = is_dy ? dy : dx;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.y * 256 + tid;
    const bool live = k < n;
    const float sv = live ? self[(size_t)r * n + k] : 0.f;
    float acc = 0.f;
    for (int p0 = 0; p0 < P; p0 += PB_CHUNK) {
        const int p = p0 + tid;
        int q = -1;
        float w = 0.f;
        if (p < P) {
            const int g = pg[p], c = pc[p];
            if (g >= 0 && g < B && c >= 0 && c < b && (is_dy ? c : g) == r) {
                q = is_dy ? g : c;
                w = pw[p];
            }
        }
        const unsigned long long mask = __ballot(q >= 0);
        __syncthreads();                                  // the previous chunk has been consumed
        if (lane == 0) cnt[wave] = __popcll(mask);
        __syncthreads();
        int base = 0;
        for (int v = 0; v < wave; ++v) base += cnt[v];
        const int total = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
        if (total == 0) continue;                         // workgroup-uniform: the barriers above are the only ones passed
        if (q >= 0) {
            const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
            sq[pos] = q;
            sw[pos] = w;
        }
        __syncthreads();
        if (live) {
#pragma unroll 8
            for (int j = 0; j < total; ++j) acc += sw[j] * (sv - other[(size_t)sq[j] * n + k]);
        }
    }
    if (live) out[(size_t)r * n + k] = 2.f * acc;
}

bool slab_ok(int B, int b, int col0) { return b >= 1 && col0 >= 0 && col0 <= B - b; }

}  // namespace

extern "C" {

int witw_baseline_hard_slab_loss(const float* T, const float* rv, const float* cv, int B, int b, int col0, int soft_margin, float alpha,
                                 float margin, float* partial, void* stream) {
    WITW_CHECK_ARG(T && rv && cv && partial, "baseline_hard_slab_loss: null pointer");
    WITW_CHECK_ARG(B >= 2, "baseline_hard_slab_loss: batch %d < 2 (every anchor needs a negative)", B);
    WITW_CHECK_ARG(slab_ok(B, b, col0), "baseline_hard_slab_loss: bad slab B=%d b=%d col0=%d", B, b, col0);
    hipLaunchKernelGGL(hard_loss_kernel<BaselineTerm>, dim3(1), dim3(256), 0, (hipStream_t)stream, T, rv, cv, partial, b, col0,
                       BaselineTerm{soft_margin, alpha, margin}, 1.f);
    WITW_CHECK_LAUNCH("baseline_hard_slab_loss");
    witw_note_variant("baseline_hard_loss_kernel");
    return WITW_OK;
}

int witw_baseline_hard_pairs(const float* diag, const float* rv, const long long* ri, const float* cv, const long long* ci,
                             const float* grad_loss, int B, int b, int col0, int soft_margin, float alpha, float margin, int* pair_g,
                             int* pair_c, float* pair_w, void* stream) {
    WITW_CHECK_ARG(diag && rv && ri && cv && ci && grad_loss && pair_g && pair_c && pair_w, "baseline_hard_pairs: null pointer");
    WITW_CHECK_ARG(B >= 2, "baseline_hard_pairs: batch %d < 2 (every anchor needs a negative)", B);
    WITW_CHECK_ARG(slab_ok(B, b, col0), "baseline_hard_pairs: bad slab B=%d b=%d col0=%d", B, b, col0);
    hipLaunchKernelGGL(hard_pairs_kernel<BaselineTerm>, dim3(cdiv(2 * b + B, 256)), dim3(256), 0, (hipStream_t)stream, diag, rv, ri, cv,
                       ci, grad_loss, pair_g, pair_c, pair_w, B, b, col0, BaselineTerm{soft_margin, alpha, margin});
    WITW_CHECK_LAUNCH("baseline_hard_pairs");
    witw_note_variant("baseline_hard_pairs_kernel");
    return WITW_OK;
}

long long witw_sqdist_pairs_bwd_workspace_bytes(int B, int b, int P) {
    if (B < 1 || b < 1 || P < 0) return -1;
    return 0;      // a workgroup per output row scans the list itself: nothing is staged in memory
}

int witw_sqdist_pairs_bwd(const float* x, const float* y, const int* pair_g, const int* pair_c, const float* pair_w, int P, float* dx,
                          float* dy, int B, int b, int n, void* workspace, void* stream) {
    (void)workspace;
    WITW_CHECK_ARG(x && y, "sqdist_pairs_bwd: null pointer");
    WITW_CHECK_ARG(dx || dy, "sqdist_pairs_bwd: null pointer (dx and dy: at least one output)");
    WITW_CHECK_ARG(B >= 1 && b >= 1 && n >= 1 && n <= 12288, "sqdist_pairs_bwd: bad shape B=%d b=%d n=%d", B, b, n);
    WITW_CHECK_ARG(P >= 0, "sqdist_pairs_bwd: %d pairs", P);
    WITW_CHECK_ARG(P == 0 || (pair_g && pair_c && pair_w), "sqdist_pairs_bwd: null pointer (pair list of %d entries)", P);
    const int nx = dx ? B : 0;
    const long long rows = (long long)nx + (dy ? b : 0);
    WITW_CHECK_ARG(rows <= 0x7fffffffLL, "sqdist_pairs_bwd: B=%d b=%d too large", B, b);
    hipLaunchKernelGGL(sqdist_pairs_bwd_kernel, dim3((unsigned)rows, cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, y, pair_g,
                       pair_c, pair_w, P, dx, dy, nx, B, b, n);
    WITW_CHECK_LAUNCH("sqdist_pairs_bwd");
    witw_note_variant("sqdist_pairs_bwd_kernel<dx:%d,dy:%d>", dx ? 1 : 0, dy ? 1 : 0);
    return WITW_OK;
}

}  // extern "C"
