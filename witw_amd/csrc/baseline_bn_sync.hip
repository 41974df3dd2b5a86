// cvig_baseline's training-mode BatchNorm2d cut at the seam where a collective fits (gfx950; HBM-bound reductions): on N ranks the
// statistics of the GLOBAL batch are the sum over the ranks of two numbers per channel, forward (sum (a - p), sum (a - p)^2 about a
// pivot p every rank shares) and backward (sum dy, sum dy * xhat). Each direction is partial sums -> [all-reduce of 2C floats, done
// by the caller] -> a pass that uses the summed vector and the global count. With one rank the same entries run back to back.
// The sums and the element-wise backward pass are the kernels of the one-call entries (bn_sums.h); what differs is the pivot, which
// is an input here (witw_bn_train_stats takes each channel's first value, which no two ranks share).
#include "common.h"
#include "bn_sums.h"

namespace {

// part [nparts][2][C] -> out [2][C]
__global__ __launch_bounds__(BNF_CH * BNF_LANES) void bn_part_finish_kernel(const float* __restrict__ part, int nparts, int C,
                                                                             float* __restrict__ out) {
    int c;
    float s0, s1;
    if (!bn_finish_sums(part, nparts, C, c, s0, s1)) return;
    out[c] = s0;
    out[C + c] = s1;
}

// sums [2][C] about pivot over n values per channel -> the statistics and the running-stat update of bn_stats_finish_kernel
// (baseline.hip), the same expressions. pivot may be running_mean itself: a thread reads its channel's pivot before it writes.
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ sums, const float* pivot, float n,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                          float momentum, float* __restrict__ mean, float* __restrict__ invstd,
                                                          float* __restrict__ scale, float* __restrict__ shift, float* running_mean,
                                                          float* __restrict__ running_var, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float dm = sums[c] / n;
    const float mu = pivot[c] + dm;
    const float var = fmaxf(sums[C + c] / n - dm * dm, 0.f);
    const float is = 1.f / sqrtf(var + eps);
    mean[c] = mu;
    invstd[c] = is;
    scale[c] = gamma[c] * is;
    shift[c] = beta[c] - mu * gamma[c] * is;
    if (running_mean != nullptr) {
        running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mu;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * (var * n / (n - 1.f));
    }
}

}  // namespace

extern "C" {

int witw_bn_partial_stats(const float* a, int B, int Hp, int Wp, int H, int W, int C, const float* pivot, float* part,
                          float* workspace, void* stream) {
    WITW_CHECK_ARG(a && pivot && part && workspace, "bn_partial_stats: null pointer");
    WITW_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && H <= Hp && W <= Wp, "bn_partial_stats: bad shape");
    hipStream_t st = (hipStream_t)stream;
    const int nparts = bl_launch_sums(a, nullptr, nullptr, nullptr, pivot, workspace, B, Hp, Wp, H, W, C, st);
    hipLaunchKernelGGL(bn_part_finish_kernel, dim3(cdiv(C, BNF_CH)), dim3(BNF_CH * BNF_LANES), 0, st, workspace, nparts, C, part);
    WITW_CHECK_LAUNCH("bn_partial_stats");
    return WITW_OK;
}

int witw_bn_finalize_stats(const float* part_sum, const float* pivot, long long count, const float* gamma, const float* beta,
                           float eps, float momentum, float* mean, float* invstd, float* scale, float* shift, float* running_mean,
                           float* running_var, int C, void* stream) {
    WITW_CHECK_ARG(part_sum && pivot && gamma && beta && mean && invstd && scale && shift, "bn_finalize_stats: null pointer");
    WITW_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "bn_finalize_stats: running_mean and running_var go together");
    WITW_CHECK_ARG(C > 0, "bn_finalize_stats: bad shape");
    WITW_CHECK_ARG(count > 1, "bn_finalize_stats: needs more than one value per channel, got count %lld", count);
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, part_sum, pivot, (float)count, gamma,
                       beta, eps, momentum, mean, invstd, scale, shift, running_mean, running_var, C);
    WITW_CHECK_LAUNCH("bn_finalize_stats");
    return WITW_OK;
}

int witw_bn_lrelu_bwd_partial(const float* a, const float* dy, const float* mean, const float* invstd, int B, int Hp, int Wp, int H,
                              int W, int C, int dy_s2d_cp, float* part, float* workspace, void* stream) {
    WITW_CHECK_ARG(a && dy && mean && invstd && part && workspace, "bn_lrelu_bwd_partial: null pointer");
    WITW_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && H <= Hp && W <= Wp, "bn_lrelu_bwd_partial: bad shape");
    WITW_CHECK_ARG(dy_s2d_cp == 0 || (dy_s2d_cp >= 4 * C && (dy_s2d_cp % 4) == 0),
                   "bn_lrelu_bwd_partial: space-to-depth channel stride %d for C=%d", dy_s2d_cp, C);
    hipStream_t st = (hipStream_t)stream;
    const int nparts = bl_launch_sums(a, dy, mean, invstd, nullptr, workspace, B, Hp, Wp, H, W, C, st, dy_s2d_cp);
    hipLaunchKernelGGL(bn_part_finish_kernel, dim3(cdiv(C, BNF_CH)), dim3(BNF_CH * BNF_LANES), 0, st, workspace, nparts, C, part);
    WITW_CHECK_LAUNCH("bn_lrelu_bwd_partial");
    return WITW_OK;
}

int witw_bn_lrelu_bwd_apply(const float* a, const float* dy, float* dz, const float* mean, const float* invstd, const float* gamma,
                            const float* sums, long long count, int B, int Hp, int Wp, int H, int W, int C, float slope,
                            int dy_s2d_cp, void* stream) {
    WITW_CHECK_ARG(a && dy && dz && mean && invstd && gamma && sums, "bn_lrelu_bwd_apply: null pointer");
    WITW_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && H <= Hp && W <= Wp, "bn_lrelu_bwd_apply: bad shape");
    WITW_CHECK_ARG(dy_s2d_cp == 0 || (dy_s2d_cp >= 4 * C && (dy_s2d_cp % 4) == 0),
                   "bn_lrelu_bwd_apply: space-to-depth channel stride %d for C=%d", dy_s2d_cp, C);
    WITW_CHECK_ARG(count >= (long long)B * H * W, "bn_lrelu_bwd_apply: count %lld is below this tensor's own %lld values per channel", count,
                   (long long)B * H * W);
    bl_launch_apply(a, dy, dz, mean, invstd, gamma, sums, (float)count, B, Hp, Wp, H, W, C, slope, dy_s2d_cp, (hipStream_t)stream);
    WITW_CHECK_LAUNCH("bn_lrelu_bwd_apply");
    return WITW_OK;
}

}  // extern "C"
