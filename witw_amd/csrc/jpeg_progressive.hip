// The scans of PROGRESSIVE JPEG files on the device (gfx950; opt-in: witw_amd/jpeg.py PROGRESSIVE_DEVICE). A progressive file codes one
// set of coefficient blocks in several scans; a scan depends on exactly the earlier scans that coded the same (component, coefficient)
// cells, which the host's scan plan (csrc_host/jpeg_coef.cpp witw_jpeg_scan_plan_ex; layout 'JPW2' in jpeg_layout.h) turns into a STAGE
// per scan: libjpeg's usual ten scans are three stages (the DC scan and four first AC scans; four refinements; the last luma
// refinement). ONE LAUNCH PER STAGE covers every file of a batch side; the order of the launches on the stream is the only
// synchronisation between stages.
//   a workgroup per (file, scan): scans of another stage, and scan slots past the file's last, leave at once;
//   the workgroup builds the scan's tables in the LDS (a first DC scan: one per scan component; an AC scan: one; a DC refinement: none);
//   a thread per SEGMENT (scan, restart interval), looping when a scan has more segments than the launch has threads for it. A file
//   without restart markers keeps one thread per workgroup busy: like jpeg_huffman_kernel this is latency-bound per thread, and the
//   parallelism is files x scans.
// The per-segment procedures are prog_segment of jpeg_entropy.h (the same source runs on the host under the sanitizers); coefficient
// cells are read and written as 16-bit cells only: scans of one stage write different cells of the same block at the same time.
#include "common.h"
#include "jpeg_layout.h"
#include "jpeg_entropy.h"

namespace {

struct JpegFileDev {               // int64 x 4 per file, as jpeg_huffman_kernel takes them
    long long bytes;               // address of the file bytes (8-byte aligned, at least 24 readable bytes behind the end)
    long long plan;                // address of the scan plan (witw_jpeg_scan_plan_ex), 4-byte aligned
    long long coef;                // address of the file's coefficient area: int16 [blocks][64], ZERO-FILLED by the caller before stage 0
    long long n_bytes;             // file length
};

__constant__ unsigned char kProgZigZag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int PROG_T = 128;         // threads per workgroup: two waves build the tables; 18 KB of LDS, eight workgroups per CU
constexpr int PROG_TABLES = 4;      // a first DC scan names at most four components

// grid: x = file, y = scan slot, z = which PROG_T segments of the scan (a scan with more segments than PROG_T * gridDim.z loops)
__global__ __launch_bounds__(PROG_T) void jpeg_progressive_kernel(const JpegFileDev* __restrict__ files, int stage, int* __restrict__ errors) {
    __shared__ HuffLds tab[PROG_TABLES];
    __shared__ unsigned char zz[64];
    __shared__ ProgScan scan_s;      // prog_segment indexes the per-position geometry with a loop variable: from the LDS, not from registers
    const int tid = threadIdx.x;
    const int scan = blockIdx.y;
    const JpegFileDev f = files[blockIdx.x];
    const WITW_AS_GLOBAL int* plan = (const WITW_AS_GLOBAL int*)f.plan;
    // the magic first: nothing else of a plan that lacks it is read
    if (plan[WITW_JPEG_PLAN_MAGIC_AT] != WITW_JPEG_PLAN_PROG_MAGIC) {
        if (tid == 0 && scan == 0 && blockIdx.z == 0) errors[blockIdx.x] = 2;
        return;
    }
    const int n_scans = plan[WITW_JPEG_PLAN_PROG_SCANS], plan_bytes = plan[WITW_JPEG_PLAN_PROG_BYTES];
    if (n_scans < 1 || n_scans > WITW_JPEG_PLAN_PROG_MAX_SCANS || plan_bytes < WITW_JPEG_PLAN_PROG_FIXED) {
        if (tid == 0 && scan == 0 && blockIdx.z == 0) errors[blockIdx.x] = 2;
        return;
    }
    if (scan >= n_scans) return;
    if (plan[WITW_JPEG_PLAN_PROG_SCAN_AT / 4 + WITW_JPEG_PLAN_PROG_SCAN_INTS * scan + WITW_JPEG_PLAN_PROG_SCAN_STAGE] != stage) return;
    ProgScan S;
    if (!prog_scan_load(plan, scan, plan_bytes, S)) {      // (uniform: every value comes from the plan)
        if (tid == 0 && blockIdx.z == 0) errors[blockIdx.x] = 2;
        return;
    }
    if ((int)blockIdx.z * PROG_T >= S.segs) return;        // nothing of this scan for this workgroup: before any table is built
    // ---- the scan's tables, by build_huff_tables' method: symbols, canonical codes (one thread per table), look-ups (all threads)
    const int n_tab = S.Ss ? 1 : (S.Ah ? 0 : S.ns);
    const WITW_AS_GLOBAL unsigned char* tsrc = (const WITW_AS_GLOBAL unsigned char*)f.plan + S.tables;
    const int tstride = S.Ss ? WITW_JPEG_PLAN_AC_STRIDE : WITW_JPEG_PLAN_DC_STRIDE;
    const int tsyms = S.Ss ? 256 : 16;
    if (tid < 64) zz[tid] = kProgZigZag[tid];
    if (tid == 64) scan_s = S;
    for (int e = tid; e < n_tab * 256; e += PROG_T) {
        const int t = e >> 8, i = e & 255;
        tab[t].sym[i] = i < tsyms ? tsrc[tstride * t + WITW_JPEG_PLAN_TABLE_SYMS + i] : (unsigned char)0;
    }
    if (tid < n_tab) huff_assign_codes(tab[tid], tsrc + tstride * tid);
    __syncthreads();
    for (int e = tid; e < n_tab * (1 << HUFF_LOOK); e += PROG_T) {
        const int t = e >> HUFF_LOOK, i = e & ((1 << HUFF_LOOK) - 1);
        tab[t].look[i] = huff_look_entry(tab[t], i);
    }
    __syncthreads();
    // ---- a thread per segment
    const unsigned n_bytes = (unsigned)f.n_bytes;
    const unsigned end_all = witw_umin((unsigned)S.data_end, n_bytes);
    const unsigned units = (unsigned)S.cols * (unsigned)S.rows;
    const WITW_AS_GLOBAL unsigned* segs = (const WITW_AS_GLOBAL unsigned*)((const WITW_AS_GLOBAL unsigned char*)f.plan + S.segs_at);
    const WITW_AS_LDS HuffLds* tabs = (const WITW_AS_LDS HuffLds*)tab;
    const WITW_AS_LDS unsigned char* zzp = (const WITW_AS_LDS unsigned char*)zz;
    WITW_AS_GLOBAL short* coef = (WITW_AS_GLOBAL short*)f.coef;
    bool bad = false;
    for (int sg = (int)blockIdx.z * PROG_T + tid; sg < S.segs; sg += PROG_T * (int)gridDim.z) {
        const WITW_AS_GLOBAL unsigned* r = segs + WITW_JPEG_PLAN_PROG_SEG_INTS * sg;
        const unsigned i0 = witw_umin(r[WITW_JPEG_PLAN_PROG_SEG_BYTE], end_all);
        // (the RSTn marker in front of the next segment stops the reader before its first byte)
        unsigned i1 = sg + 1 < S.segs ? witw_umin(r[WITW_JPEG_PLAN_PROG_SEG_INTS + WITW_JPEG_PLAN_PROG_SEG_BYTE], end_all) : end_all;
        if (i1 < i0) i1 = i0;
        const unsigned u0 = witw_umin(r[WITW_JPEG_PLAN_PROG_SEG_UNIT], units);
        const unsigned u1 = u0 + witw_umin(r[WITW_JPEG_PLAN_PROG_SEG_UNITS], units - u0);
        BitReaderT<true, GlobalWords> b;
        b.start((GlobalWords)f.bytes, i0, i1);
        if (!prog_segment(b, (const WITW_AS_LDS ProgScan*)&scan_s, tabs, coef, zzp, u0, u1)) bad = true;
    }
    if (bad) errors[blockIdx.x] = 1;
}

}  // namespace

extern "C" {

// One stage of the progressive files of a batch side: see include/witw_hip.h.
int witw_jpeg_progressive_stage(const void* files, int n_files, int stage, int max_scans, int max_segments, int* errors, void* stream) {
    WITW_CHECK_ARG(files && errors, "jpeg_progressive_stage: null pointer");
    WITW_CHECK_ARG(n_files > 0 && max_segments > 0, "jpeg_progressive_stage: %d files, %d segments", n_files, max_segments);
    WITW_CHECK_ARG(max_scans > 0 && max_scans <= WITW_JPEG_PLAN_PROG_MAX_SCANS, "jpeg_progressive_stage: %d scans (1..%d)", max_scans,
                   (int)WITW_JPEG_PLAN_PROG_MAX_SCANS);
    WITW_CHECK_ARG(stage >= 0 && stage < WITW_JPEG_PLAN_PROG_MAX_STAGES, "jpeg_progressive_stage: stage %d (0..%d)", stage,
                   (int)WITW_JPEG_PLAN_PROG_MAX_STAGES - 1);
    int groups = (max_segments + PROG_T - 1) / PROG_T;      // per scan; at most 64 (a scan with more than 8,192 segments loops)
    if (groups > 64) groups = 64;
    hipLaunchKernelGGL(jpeg_progressive_kernel, dim3((unsigned)n_files, (unsigned)max_scans, (unsigned)groups), dim3(PROG_T), 0,
                       (hipStream_t)stream, (const JpegFileDev*)files, stage, errors);
    WITW_CHECK_LAUNCH("jpeg_progressive_stage");
    return WITW_OK;
}

}  // extern "C"
