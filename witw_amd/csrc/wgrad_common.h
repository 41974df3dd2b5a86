// Host side shared by the weight-gradient launchers (conv3x3_wgrad.hip, wgrad_bf16.hip, wgrad_f16x3.hip): the K-split count,
// the launch prologue (argument checks and split geometry, also what the *_workspace_floats entries size from) and the one
// split-K reduction behind every main kernel.
#pragma once
#include "common.h"

// K splits: enough of them that `tiles` output tiles make about `target_workgroups` workgroups, at most one per K chunk.
static inline int wgrad_splits(int target_workgroups, int tiles, int chunks) {
    int splits = cdiv(target_workgroups, tiles);
    if (splits > chunks) splits = chunks;
    return splits < 1 ? 1 : splits;
}

// How an entry cuts the work: a workgroup owns tile_ci x tile_co channels of all taps; one K chunk is `rows` output rows x `cols`
// output columns of one image (or image octet); `target` workgroups are aimed at.
struct WgradTiling {
    int target, tile_ci, tile_co, rows, cols;
};

struct WgradGeom {
    int Ho;
    int nseg, nrg;       // column segments per output row, row groups per image (octet)
    int chunks, splits;
    int cps;             // chunks per split
    int parts;           // weight partials in the workspace
    size_t n;            // floats of one weight partial of the full window: 9 * Cin * Cout
    float* bias_part;    // nullptr, or the bias partials [..][Cout] behind the weight partials (wgrad_prologue)
};

// Workspace: weight partials [parts][taps][Cin][Cout] from float 0, bias partials [..][Cout] from float parts * n.
static inline WgradGeom wgrad_geom(const WgradTiling& t, int images, int parts_per_split, int H, int W, int Cin, int Cout, int stride_h) {
    WgradGeom g;
    g.Ho = (H + 2 - 3) / stride_h + 1;
    g.nseg = cdiv(W, t.cols);
    g.nrg = cdiv(g.Ho, t.rows);
    g.chunks = images * g.nrg * g.nseg;
    g.splits = wgrad_splits(t.target, cdiv(Cin, t.tile_ci) * cdiv(Cout, t.tile_co), g.chunks);
    g.cps = cdiv(g.chunks, g.splits);
    g.parts = parts_per_split * g.splits;
    g.n = (size_t)9 * Cin * Cout;
    g.bias_part = nullptr;
    return g;
}

static inline long long wgrad_workspace_floats(const WgradGeom& g, long long bias_parts, int Cout) {
    return (long long)g.parts * (long long)g.n + bias_parts * Cout;
}

// The checks every entry makes (`name` goes into the messages; gran = channel granularity: 4 for fp32, 8 for the 16-bit forms),
// then the geometry. An entry's own conditions (descriptor sizes, ...) follow at the call site.
static inline int wgrad_prologue(WgradGeom& g, const char* name, int gran, const WgradTiling& t, int images, int parts_per_split,
                                 const void* x, const void* dz, const float* dw, const float* db, float* workspace, int B, int H, int W,
                                 int Cin, int cin_real, int Cout, int stride_h) {
    WITW_CHECK_ARG(x && dz && dw && workspace, "%s: null pointer", name);
    WITW_CHECK_ARG(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "%s: bad shape", name);
    WITW_CHECK_ARG((Cin % gran) == 0 && (Cout % gran) == 0, "%s: Cin=%d and Cout=%d must be multiples of %d", name, Cin, Cout, gran);
    WITW_CHECK_ARG(cin_real > 0 && cin_real <= Cin, "%s: cin_real=%d outside (0,%d]", name, cin_real, Cin);
    WITW_CHECK_ARG(stride_h == 1 || stride_h == 2, "%s: stride_h=%d unsupported", name, stride_h);
    g = wgrad_geom(t, images, parts_per_split, H, W, Cin, Cout, stride_h);
    g.bias_part = db ? workspace + (size_t)g.parts * g.n : nullptr;
    return WITW_OK;
}

// dW[co][ci][kh][kw] (+)= sum_k ws[k][tap][ci][co], k < parts; db[co] (+)= sum_k bias_part[k][co], k < bias_parts (db may be
// null). Fixed order, so bitwise reproducible: WGRAD_SERIAL adds k = 0, 1, ... from zero at every count; WGRAD_WIDE_AT_32 (the
// fp32 entries, where parts == bias_parts) switches at parts >= 32 to eight interleaved group sums added in group order
// (wgrad_reduce_wide_kernel). The two orders differ in the last bits, so an entry's choice is part of its results.
// taps = 4: the 2x2 sub-window, whose partials are [parts][4][Cin][Cout]. Defined in conv3x3_wgrad.hip.
enum WgradReduceForm { WGRAD_SERIAL, WGRAD_WIDE_AT_32 };
int witw_wgrad_reduce(const float* ws, const float* bias_part, float* dw, float* db, int Cin, int cin_real, int Cout, int taps, int parts,
                      int bias_parts, int accumulate, WgradReduceForm form, void* stream);
