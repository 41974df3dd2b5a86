// Batched device data path of cvig_baseline (gfx950; gather copies bound by HBM and L2): Compose[SyncedRotation, SurfaceResize]
// (model/cvig_baseline.py:130-144, :208-225, :324-328) for a whole batch straight from the decoder's bytes, over the descriptor
// table of witw_resize_bilinear_normalize_batched (preprocess.hip):
//   rotate_batched_kernel      SyncedRotation's overhead rotation: rotate_nearest_kernel per table row, the source pixel from the
//                              SAME helper (rotate_coord.h), so the same bits
//   roll_rows_batched_kernel   horizontal_shift (a left roll by `start` columns) + SurfaceResize('cvusa')'s repeat_interleave(2, -2):
//                              a pure copy, every source pixel read once and stored `rep` times
// Layout of both: blockIdx.y = image (so the descriptor is wave-uniform and fetched by scalar loads), consecutive lanes = consecutive
// pixels of a row: every plane store is 256 contiguous bytes per wave, and a lane fetches all C channels of its source pixel
// (adjacent bytes for uint8 HWC sources) before the first store. No LDS, a dozen registers: the occupancy is the 8 waves / SIMD cap.
// A table row that does not fit the launch (other size, start outside the row, fewer stored channels than C, null address) gives
// a zero image and is never dereferenced past its own H x W x cs.
#include "common.h"
#include "rotate_coord.h"

namespace {

struct ImgDesc {            // one row of the table, as in preprocess.hip
    unsigned long long ptr;
    long long H, W, start, cs;
};

constexpr int BP_THREADS = 256;

// all `n` channels of source pixel `src` (row * W + column) of image d, as floats (uint8 -> float is exact); zeros when !ok
template <int KIND, int CT>
__device__ __forceinline__ void fetch_pixel(const ImgDesc& d, bool ok, size_t src, size_t plane, int n, float (&v)[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        v[c] = 0.f;
        if (c < (CT > 0 ? CT : n) && ok) {
            if (KIND == 0)
                v[c] = reinterpret_cast<const float*>(d.ptr)[(size_t)c * plane + src];
            else
                v[c] = (float)reinterpret_cast<const unsigned char*>(d.ptr)[src * (size_t)d.cs + c];
        }
    }
}

template <int KIND, int CT>
__global__ __launch_bounds__(BP_THREADS) void rotate_batched_kernel(const ImgDesc* __restrict__ desc, const float* __restrict__ theta,
                                                                    float* __restrict__ y, int C, int H, int W) {
    const unsigned plane = (unsigned)H * (unsigned)W;
    const unsigned pix = blockIdx.x * (unsigned)BP_THREADS + threadIdx.x;
    if (pix >= plane) return;
    const int b = blockIdx.y;
    const int n = CT > 0 ? CT : C;
    const ImgDesc d = desc[b];
    const int oy = (int)(pix / (unsigned)W), ox = (int)(pix - (unsigned)oy * (unsigned)W);
    int sx, sy;
    bool ok = witw_rotate_source(theta + (size_t)b * 6, ox, oy, H, W, sx, sy);
    ok = ok && d.ptr != 0 && d.H == H && d.W == W && d.cs >= n;      // the table's own bounds: (sx, sy) lies inside H x W
    float v[8];
    fetch_pixel<KIND, CT>(d, ok, (size_t)sy * W + sx, plane, n, v);
    float* yb = y + (size_t)b * n * plane + pix;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (c < n) yb[(size_t)c * plane] = v[c];
}

// H = Ho / rep source rows; one thread per SOURCE pixel position (b, sy, ox), `rep` stores per channel
template <int KIND, int CT>
__global__ __launch_bounds__(BP_THREADS) void roll_rows_batched_kernel(const ImgDesc* __restrict__ desc, float* __restrict__ y, int C,
                                                                       int H, int Wo, int rep) {
    const unsigned plane = (unsigned)H * (unsigned)Wo;
    const unsigned pix = blockIdx.x * (unsigned)BP_THREADS + threadIdx.x;
    if (pix >= plane) return;
    const int b = blockIdx.y;
    const int n = CT > 0 ? CT : C;
    const ImgDesc d = desc[b];
    const int sy = (int)(pix / (unsigned)Wo), ox = (int)(pix - (unsigned)sy * (unsigned)Wo);
    const bool ok = d.ptr != 0 && d.H == H && d.W == Wo && d.start >= 0 && d.start < Wo && d.cs >= n;
    int cx = ok ? ox + (int)d.start : 0;      // (ox + start) mod W
    if (cx >= Wo) cx -= Wo;
    float v[8];
    fetch_pixel<KIND, CT>(d, ok, (size_t)sy * Wo + cx, plane, n, v);
    const size_t oplane = (size_t)plane * rep;
    float* yb = y + (size_t)b * n * oplane + (size_t)sy * rep * Wo + ox;
    for (int r = 0; r < rep; ++r) {
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (c < n) yb[(size_t)c * oplane + (size_t)r * Wo] = v[c];
    }
}

}  // namespace

extern "C" {

int witw_baseline_rotate_batched(const void* desc, const float* theta, float* y, int B, int C, int H, int W, int kind, void* stream) {
    WITW_CHECK_ARG(desc && theta && y, "baseline_rotate_batched: null pointer");
    WITW_CHECK_ARG(kind == 0 || kind == 1, "baseline_rotate_batched: source kind %d unknown (0 float32 CHW, 1 uint8 HWC)", kind);
    WITW_CHECK_ARG(C >= 1 && C <= 8, "baseline_rotate_batched: C=%d channels, 1..8 are supported", C);
    WITW_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W < 0x7fffffffLL,
                   "baseline_rotate_batched: bad shape B=%d H=%d W=%d", B, H, W);
    const dim3 grid((unsigned)(((long long)H * W + BP_THREADS - 1) / BP_THREADS), (unsigned)B);
#define WITW_BR(K, CT) hipLaunchKernelGGL((rotate_batched_kernel<K, CT>), grid, dim3(BP_THREADS), 0, (hipStream_t)stream, (const ImgDesc*)desc, theta, y, C, H, W)
    if (kind == 0) {
        if (C == 3) WITW_BR(0, 3); else WITW_BR(0, 0);
    } else {
        if (C == 3) WITW_BR(1, 3); else WITW_BR(1, 0);
    }
#undef WITW_BR
    WITW_CHECK_LAUNCH("baseline_rotate_batched");
    return WITW_OK;
}

int witw_baseline_roll_rows_batched(const void* desc, float* y, int B, int C, int Ho, int Wo, int rep, int kind, void* stream) {
    WITW_CHECK_ARG(desc && y, "baseline_roll_rows_batched: null pointer");
    WITW_CHECK_ARG(kind == 0 || kind == 1, "baseline_roll_rows_batched: source kind %d unknown (0 float32 CHW, 1 uint8 HWC)", kind);
    WITW_CHECK_ARG(C >= 1 && C <= 8, "baseline_roll_rows_batched: C=%d channels, 1..8 are supported", C);
    WITW_CHECK_ARG(rep >= 1, "baseline_roll_rows_batched: rep=%d, every source row is stored at least once", rep);
    WITW_CHECK_ARG(B > 0 && B <= 65535 && Ho > 0 && Wo > 0 && (long long)Ho * Wo < 0x7fffffffLL,
                   "baseline_roll_rows_batched: bad shape B=%d Ho=%d Wo=%d", B, Ho, Wo);
    WITW_CHECK_ARG(Ho % rep == 0, "baseline_roll_rows_batched: Ho=%d is not rep=%d times a source height", Ho, rep);
    const int H = Ho / rep;
    const dim3 grid((unsigned)(((long long)H * Wo + BP_THREADS - 1) / BP_THREADS), (unsigned)B);
#define WITW_BR(K, CT) hipLaunchKernelGGL((roll_rows_batched_kernel<K, CT>), grid, dim3(BP_THREADS), 0, (hipStream_t)stream, (const ImgDesc*)desc, y, C, H, Wo, rep)
    if (kind == 0) {
        if (C == 3) WITW_BR(0, 3); else WITW_BR(0, 0);
    } else {
        if (C == 3) WITW_BR(1, 3); else WITW_BR(1, 0);
    }
#undef WITW_BR
    WITW_CHECK_LAUNCH("baseline_roll_rows_batched");
    return WITW_OK;
}

}  // extern "C"
