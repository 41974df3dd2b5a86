// The two binary layouts the JPEG data path shares between the host parser (csrc_host/jpeg_coef.cpp), the device entropy decoders
// (csrc/jpeg.hip) and the Python side (witw_amd/jpeg.py, which repeats the names it uses; tests/test_jpeg.py holds them to this file).
// Constants only: plain C++ for host and device. Every value is written out as a number (`NAME = value`): the test reads them as text.
#pragma once

// ---- the entropy plan (witw_jpeg_entropy_plan_ex writes it, jpeg_huffman_kernel / jpeg_selfsync_kernel read it beside the FILE BYTES
// themselves -- they unstuff FF 00 on the fly). 32 int32 of header, the Huffman tables, the interval offsets:
//   int32[0] magic 'JPW1', [1] intervals, [2] MCUs per interval, [3] MCUs per row, [4] MCU rows, [5] components,
//   [6 + 7c ..] component c < 3: h, v, blocks wide, blocks high, first block (within the file's coefficient area), DC slot, AC slot,
//   [27] end of the entropy-coded data (byte offset in the file), [28..30] component of scan position k, [31] 0;
//   byte 128: DC tables of slots 0, 1 (16 counts + 16 symbols each), byte 192: AC tables of slots 0, 1 (16 counts + 256 symbols each);
//   byte 736: uint32 [intervals]: byte offset in the file of each interval's first entropy-coded byte.
// A file without restart markers gets a plan of ONE interval (the whole scan): the device decodes it with the self-synchronising
// kernel. Files with more than two DC or AC tables in use, or whose markers are out of sequence, return -2 / -3 and take the host
// path (witw_jpeg_decode_coef) as before.
enum {
    WITW_JPEG_PLAN_MAGIC = 0x3157504A,          // 'JPW1', the value of header int 0
    // header ints
    WITW_JPEG_PLAN_MAGIC_AT = 0,
    WITW_JPEG_PLAN_INTERVALS = 1,
    WITW_JPEG_PLAN_INTERVAL_MCUS = 2,           // MCUs per interval
    WITW_JPEG_PLAN_MCUX = 3,                    // MCUs per row
    WITW_JPEG_PLAN_MCUY = 4,                    // MCU rows
    WITW_JPEG_PLAN_NCOMP = 5,
    WITW_JPEG_PLAN_COMP = 6,                    // the record of component c starts at COMP + COMP_STRIDE * c ...
    WITW_JPEG_PLAN_COMP_STRIDE = 7,
    WITW_JPEG_PLAN_COMP_H = 0,                  // ... and holds these fields
    WITW_JPEG_PLAN_COMP_V = 1,
    WITW_JPEG_PLAN_COMP_BW = 2,                 // blocks wide
    WITW_JPEG_PLAN_COMP_BH = 3,                 // blocks high
    WITW_JPEG_PLAN_COMP_FIRST = 4,              // first block within the file's coefficient area
    WITW_JPEG_PLAN_COMP_DC = 5,                 // DC table slot
    WITW_JPEG_PLAN_COMP_AC = 6,                 // AC table slot
    WITW_JPEG_PLAN_DATA_END = 27,               // end of the entropy-coded data (byte offset in the file)
    WITW_JPEG_PLAN_SCAN_COMP = 28,              // + k: component of scan position k < 3
    WITW_JPEG_PLAN_HEADER_INTS = 32,
    // byte offsets
    WITW_JPEG_PLAN_DC = 128,                    // DC table of slot s at DC + DC_STRIDE * s: 16 counts, 16 symbols
    WITW_JPEG_PLAN_DC_STRIDE = 32,
    WITW_JPEG_PLAN_AC = 192,                    // AC table of slot s at AC + AC_STRIDE * s: 16 counts, 256 symbols
    WITW_JPEG_PLAN_AC_STRIDE = 272,
    WITW_JPEG_PLAN_TABLE_SYMS = 16,             // a table's symbols sit behind its 16 counts
    WITW_JPEG_PLAN_FIXED = 736                  // the interval offsets (uint32 each); a plan is FIXED + 4 * intervals bytes
};

// ---- the `info` ints of witw_jpeg_info / witw_jpeg_info_ex (columns COL_INFO .. of the packed descriptor of witw_amd/jpeg.py):
// H, W, ncomp, hmax, vmax, total blocks, then per component (4 slots): h, v, blocks wide, blocks high.
enum {
    WITW_JPEG_INFO_H = 0,
    WITW_JPEG_INFO_W = 1,
    WITW_JPEG_INFO_NCOMP = 2,
    WITW_JPEG_INFO_HMAX = 3,
    WITW_JPEG_INFO_VMAX = 4,
    WITW_JPEG_INFO_BLOCKS = 5,                  // coefficient blocks of the file, all components
    WITW_JPEG_INFO_COMP = 6,                    // the record of component c < 4 starts at COMP + COMP_STRIDE * c
    WITW_JPEG_INFO_COMP_STRIDE = 4,
    WITW_JPEG_INFO_COMP_H = 0,
    WITW_JPEG_INFO_COMP_V = 1,
    WITW_JPEG_INFO_COMP_BW = 2,
    WITW_JPEG_INFO_COMP_BH = 3,
    WITW_JPEG_INFO_INTS = 22
};
