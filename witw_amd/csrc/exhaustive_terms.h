// One term of exhaustive_minibatch_triplet_loss (model/cvig_baseline.py:286-315) and its derivative, x = d_positive - d_negative:
// the dense kernels (baseline.hip) and the column-slab kernels (baseline_loss_slab.hip) share ONE expression of each.
#pragma once
#include "common.h"

__device__ __forceinline__ float trip(float x, int soft, float alpha, float margin) {
    return soft ? logf(1.f + expf(alpha * x)) : fmaxf(x + margin, 0.f);
}

__device__ __forceinline__ float trip_d(float x, int soft, float alpha, float margin) {
    return soft ? alpha / (1.f + expf(-alpha * x)) : ((x + margin > 0.f) ? 1.f : 0.f);
}
