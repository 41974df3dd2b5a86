// Source pixel of SyncedRotation's nearest-neighbour rotation, shared by rotate_nearest_kernel (preprocess.hip) and
// rotate_batched_kernel (baseline_prep.hip): ONE expression, so that both kernels round every coordinate alike and the
// batched form is bit-identical to the per-sample one.
#pragma once
#include <hip/hip_runtime.h>

// th: the six floats of one image's theta (witw_rotate_nearest: the 2x3 inverse rotation matrix ALREADY divided by
// (0.5*W, 0.5*H) as torchvision's _gen_affine_grid does, laid out [k][j], k = x,y,1 row, j = output coordinate:
// gx = x*t00 + y*t10 + t20). Base grid = half-integer pixel centres (linspace(-W/2+.5, W/2-.5, W): step exactly 1);
// un-normalisation and rounding follow ATen's grid_sampler (align_corners=False, nearbyint, zero outside).
// -> whether output pixel (ox, oy) of an H x W image has a source pixel inside the image, and then that pixel (sx, sy).
__device__ __forceinline__ bool witw_rotate_source(const float* __restrict__ th, int ox, int oy, int H, int W, int& sx, int& sy) {
    const float xg = (float)ox + (0.5f - 0.5f * (float)W), yg = (float)oy + (0.5f - 0.5f * (float)H);
    const float gx = __fmaf_rn(yg, th[2], xg * th[0]) + th[4];
    const float gy = __fmaf_rn(yg, th[3], xg * th[1]) + th[5];
    const float fx = ((gx + 1.f) * (float)W - 1.f) / 2.f, fy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
    const float rx = nearbyintf(fx), ry = nearbyintf(fy);
    const bool ok = rx >= 0.f && rx <= (float)(W - 1) && ry >= 0.f && ry <= (float)(H - 1);
    sx = ok ? (int)rx : 0;
    sy = ok ? (int)ry : 0;
    return ok;
}
