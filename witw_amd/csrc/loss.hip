// Soft-margin triplet loss over the B x B distance matrix (gfx950).
//
// Reference: triplet_loss, model/cvig_fov.py:366-382:
//   loss = ( sum_ij log(1+exp(a*(d_jj - d_ij))) + sum_ij log(1+exp(a*(d_ii - d_ij))) ) / (2B(B-1))
// (both sums over the FULL matrix, diagonal included; naive log(1+exp) kept).
// All reductions run in a fixed order (per-row / per-column partials, then one block) so the
// result is bitwise reproducible run to run. The dense kernels are below; the column-slab entries launch the kernels of
// loss_kernels.h with FovTerm.
#include "loss_kernels.h"

namespace {

// blocks [0,B): row i  -> ws[i]      = sum_j softplus(a*(d_ii - d_ij)), ws[2B+i] = sum_j sigmoid(.)
// blocks [B,2B): col j -> ws[B+j]    = sum_i softplus(a*(d_jj - d_ij)), ws[3B+j] = sum_i sigmoid(.)
__global__ __launch_bounds__(256) void triplet_partials_kernel(const float* __restrict__ D, float* __restrict__ ws, int B,
                                                                FovTerm term) {
    __shared__ float sh[4];
    const bool is_col = blockIdx.x >= (unsigned)B;
    const int m = is_col ? blockIdx.x - B : blockIdx.x;
    const float dm = D[(size_t)m * B + m];
    float sp = 0.f, sg = 0.f;
    for (int t = threadIdx.x; t < B; t += 256) {
        const float d = is_col ? D[(size_t)t * B + m] : D[(size_t)m * B + t];
        sp += term.value(dm - d);
        sg += term.deriv(dm - d);
    }
    const float tsp = block_sum_256(sp, sh);
    const float tsg = block_sum_256(sg, sh);
    if (threadIdx.x == 0) {
        ws[(is_col ? B : 0) + m] = tsp;
        ws[(is_col ? 3 * B : 2 * B) + m] = tsg;
    }
}

__global__ __launch_bounds__(256) void triplet_finish_kernel(const float* __restrict__ ws, float* __restrict__ loss, int B,
                                                              float norm) {
    __shared__ float sh[4];
    float a = 0.f, b = 0.f;
    for (int t = threadIdx.x; t < B; t += 256) {
        a += ws[B + t];   // surface -> overhead term (column partials), reference :377
        b += ws[t];       // overhead -> surface term (row partials), reference :378
    }
    const float ta = block_sum_256(a, sh);
    const float tb = block_sum_256(b, sh);
    if (threadIdx.x == 0) loss[0] = (ta + tb) / norm;
}

// dL/dD_ij = g*(a/norm) * ( -sig(a(d_jj-d_ij)) - sig(a(d_ii-d_ij)) + [i==j]*(colsig_j + rowsig_i) )
__global__ void triplet_bwd_kernel(const float* __restrict__ D, const float* __restrict__ ws,
                                   const float* __restrict__ gloss, float* __restrict__ gD, int B, FovTerm term,
                                   float norm) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * B) return;
    const int i = idx / B, j = idx - (size_t)i * B;
    const float d = D[idx];
    float g = -term.deriv(D[(size_t)j * B + j] - d) - term.deriv(D[(size_t)i * B + i] - d);
    if (i == j) g += ws[3 * B + j] + ws[2 * B + i];
    gD[idx] = g * term.scale(gloss[0], norm);
}

}  // namespace

extern "C" {

int witw_triplet_loss_fwd(const float* distance, int B, float alpha, float* loss, float* workspace, void* stream) {
    WITW_CHECK_ARG(distance && loss && workspace, "triplet_loss_fwd: null pointer");
    WITW_CHECK_ARG(B >= 2, "triplet_loss_fwd: batch %d < 2 (the reference divides by 2B(B-1))", B);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(triplet_partials_kernel, dim3(2 * B), dim3(256), 0, st, distance, workspace, B, FovTerm{alpha});
    hipLaunchKernelGGL(triplet_finish_kernel, dim3(1), dim3(256), 0, st, workspace, loss, B, 2.f * B * (B - 1));
    WITW_CHECK_LAUNCH("triplet_loss_fwd");
    return WITW_OK;
}

// Un-normalised partial of the loss over a column slab D[Bo][Bs] = distances of all Bo overheads to the
// surfaces [col0, col0+Bs) of the global batch; diag[Bo] = the global diagonal. The caller sums the partials of
// all ranks and divides by 2*Bo*(Bo-1). workspace: Bo floats.
int witw_triplet_loss_slab_fwd(const float* distance, const float* diag, int Bo, int Bs, int col0, float alpha, float* partial,
                               float* workspace, void* stream) {
    WITW_CHECK_ARG(distance && diag && partial && workspace, "triplet_loss_slab_fwd: null pointer");
    WITW_CHECK_ARG(Bo >= 2 && Bs >= 1 && col0 >= 0 && col0 + Bs <= Bo, "triplet_loss_slab_fwd: bad slab Bo=%d Bs=%d col0=%d", Bo, Bs,
                   col0);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(slab_partials_kernel<FovTerm>, dim3(Bo), dim3(256), 0, st, distance, diag, workspace, Bs, col0, FovTerm{alpha});
    hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(256), 0, st, workspace, partial, Bo, 1.f);
    WITW_CHECK_LAUNCH("triplet_loss_slab_fwd");
    return WITW_OK;
}

// Backward of the sharded loss, step 1: rowsig[Bo] (partial: this rank's surfaces only — all-reduce it over the
// ranks) and colsig[Bs] (complete) of the slab, see witw_triplet_loss_slab_fwd for the arguments.
int witw_triplet_loss_slab_sig(const float* distance, const float* diag, int Bo, int Bs, int col0, float alpha, float* rowsig,
                               float* colsig, void* stream) {
    WITW_CHECK_ARG(distance && diag && rowsig && colsig, "triplet_loss_slab_sig: null pointer");
    WITW_CHECK_ARG(Bo >= 2 && Bs >= 1 && col0 >= 0 && col0 + Bs <= Bo, "triplet_loss_slab_sig: bad slab Bo=%d Bs=%d col0=%d", Bo, Bs,
                   col0);
    hipLaunchKernelGGL(slab_sig_kernel<FovTerm>, dim3(Bo + Bs), dim3(256), 0, (hipStream_t)stream, distance, diag, rowsig, colsig, Bo,
                       Bs, col0, FovTerm{alpha});
    WITW_CHECK_LAUNCH("triplet_loss_slab_sig");
    return WITW_OK;
}

// Step 2: grad_distance[Bo,Bs] of the slab for grad_loss (device scalar) of the GLOBAL loss; rowsig = the summed row sums.
int witw_triplet_loss_slab_bwd(const float* distance, const float* diag, const float* rowsig, const float* colsig,
                               const float* grad_loss, float* grad_distance, int Bo, int Bs, int col0, float alpha, void* stream) {
    WITW_CHECK_ARG(distance && diag && rowsig && colsig && grad_loss && grad_distance, "triplet_loss_slab_bwd: null pointer");
    WITW_CHECK_ARG(Bo >= 2 && Bs >= 1 && col0 >= 0 && col0 + Bs <= Bo, "triplet_loss_slab_bwd: bad slab Bo=%d Bs=%d col0=%d", Bo, Bs,
                   col0);
    const size_t total = (size_t)Bo * Bs;
    hipLaunchKernelGGL(slab_bwd_kernel<FovTerm>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, distance, diag,
                       rowsig, colsig, grad_loss, grad_distance, Bo, Bs, col0, FovTerm{alpha});
    WITW_CHECK_LAUNCH("triplet_loss_slab_bwd");
    return WITW_OK;
}

int witw_triplet_loss_bwd(const float* distance, const float* workspace, const float* grad_loss, float* grad_distance, int B,
                          float alpha, void* stream) {
    WITW_CHECK_ARG(distance && workspace && grad_loss && grad_distance, "triplet_loss_bwd: null pointer");
    WITW_CHECK_ARG(B >= 2, "triplet_loss_bwd: batch %d < 2", B);
    const size_t total = (size_t)B * B;
    hipLaunchKernelGGL(triplet_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, distance,
                       workspace, grad_loss, grad_distance, B, FovTerm{alpha}, 2.f * B * (B - 1));
    WITW_CHECK_LAUNCH("triplet_loss_bwd");
    return WITW_OK;
}

}  // extern "C"
