// sum_k (br[k] - arow[k])^2 as pairwise_sqdist_kernel (baseline.hip) and sqdist_pairs_kernel (baseline_retrieval.hip) both compute
// it: ONE expression, so the exact re-scoring of a pair is the matrix entry bit for bit by construction (the build runs with
// -ffp-contract=off: no product is fused into a sum in either caller).
#pragma once
#include "common.h"

// four running sums (k mod 4), added pairwise at the end: one running sum over n = 1536 squares drifts 16x further from the
// exact sum than torch's blocked sum does (its rounding grows with sqrt(n) x the sum so far), and is one dependent chain
__device__ __forceinline__ float witw_sqdist_row(const float* __restrict__ arow, const float* __restrict__ br, int n) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int k = 0;
    for (; k + 3 < n; k += 4) {
        const float d0 = br[k] - arow[k], d1 = br[k + 1] - arow[k + 1], d2 = br[k + 2] - arow[k + 2], d3 = br[k + 3] - arow[k + 3];
        s0 += d0 * d0;
        s1 += d1 * d1;
        s2 += d2 * d2;
        s3 += d3 * d3;
    }
    for (; k < n; ++k) {
        const float d = br[k] - arow[k];
        s0 += d * d;
    }
    return (s0 + s1) + (s2 + s3);
}
