// Launch prologue shared by the tiled NHWC 3x3 convolution kernels of the reduced-precision formats (conv3x3_bf16.hip,
// conv3x3_f16x3.hip): the same workgroup tile and the same block -> (n tile, spatial tile) order in all of them.
#pragma once
#include "common.h"
#include <stdlib.h>

// 1 (default): workgroups are numbered so that the spatial tiles of one XCD are contiguous (block i runs on XCD i % 8);
// WITW_CONV_XCD=0 turns that off. Read on every call.
static inline int witw_conv_xcd_map() {
    const char* e = getenv("WITW_CONV_XCD");
    return e ? atoi(e) != 0 : 1;
}

// Fills the tile counts of `a` (a.B, a.Ho, a.Cout, a.tiles_x, a.xcd_map set by the caller) for workgroup tiles of `th` output rows
// x `tn` channels and returns the grid, or sets "<what>: grid ... out of range" and returns 0.
template <class Args>
static inline long long witw_conv_grid(Args& a, int th, int tn, const char* what) {
    a.tiles_y = cdiv(a.Ho, th);
    const long long sp_total = (long long)a.B * a.tiles_x * a.tiles_y;
    a.n_tiles = cdiv(a.Cout, tn);
    a.sp_per_xcd = (int)((sp_total + 7) / 8);
    const long long grid = a.xcd_map ? 8LL * a.sp_per_xcd * a.n_tiles : sp_total * a.n_tiles;
    if (grid <= 0 || grid > 0x7fffffffLL || sp_total > 0x7fffffffLL) {
        witw_set_error("%s: grid %lld out of range", what, grid);
        return 0;
    }
    a.sp_total = (int)sp_total;
    return grid;
}
