// The binary layouts the JPEG data path shares between the host parser (csrc_host/jpeg_coef.cpp), the device entropy decoders
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

// ---- the scan plan of a PROGRESSIVE file (witw_jpeg_scan_plan_ex writes it, jpeg_progressive_kernel reads it beside the file bytes).
// A magic of its own; the frame part of the header (MCU grid, components, per component h, v, blocks wide, blocks high, first block)
// sits where the 'JPW1' header has it (WITW_JPEG_PLAN_MCUX .. WITW_JPEG_PLAN_COMP records; the two table-slot fields stay 0):
//   int32[0] magic 'JPW2', [1] scans, [2] segments of all scans, [3..26] as 'JPW1', [27] stages, [28] the largest segment count of a scan,
//   [29] coefficient blocks of the file (every block index is held under it), [30] the plan's size in bytes, [31] 0;
//   byte 128: PROG_MAX_SCANS scan records of PROG_SCAN_INTS int32 each (scans past the file's last: zero):
//     components in the scan, their indices (4 slots), Ss, Se, Ah, Al, the walk -- units per row and rows of units (an interleaved scan:
//     the MCU grid; a scan of one component: that component's own ceil(w_c / 8) x ceil(h_c / 8) blocks over its pitch `blocks wide`) --,
//     units per restart interval (0: none, one segment), stage, byte offset in the plan of the scan's Huffman tables (a first DC scan: one
//     DC table per scan component, PLAN_DC_STRIDE bytes each; an AC scan: one AC table of PLAN_AC_STRIDE bytes; a DC refinement: none,
//     0), byte offset in the plan of its segment records, their number, end of its entropy-coded data (byte offset in the file);
//   behind the scan records, scan by scan: the tables in force at that scan (16 counts + symbols, as in 'JPW1'), then a record of
//     PROG_SEG_INTS uint32 per segment = (scan, restart interval): byte offset in the file of its first entropy-coded byte, first unit,
//     units. A segment's data ends at the next marker.
// stage(scan) = 0 if no earlier scan coded any of its (component, coefficient) cells, else 1 + the largest stage among them: scans of
// one stage touch disjoint cells and are decoded in one launch. Files of more than PROG_MAX_SCANS scans get no plan.
enum {
    WITW_JPEG_PLAN_PROG_MAGIC = 0x3257504A,     // 'JPW2'
    WITW_JPEG_PLAN_PROG_SCANS = 1,
    WITW_JPEG_PLAN_PROG_SEGMENTS = 2,
    WITW_JPEG_PLAN_PROG_STAGES = 27,
    WITW_JPEG_PLAN_PROG_MAX_SEGMENTS = 28,      // the largest segment count of a scan
    WITW_JPEG_PLAN_PROG_BLOCKS = 29,
    WITW_JPEG_PLAN_PROG_BYTES = 30,
    WITW_JPEG_PLAN_PROG_MAX_SCANS = 64,
    WITW_JPEG_PLAN_PROG_MAX_STAGES = 14,        // Al <= 13
    WITW_JPEG_PLAN_PROG_SCAN_AT = 128,          // byte offset of scan record 0; record s at SCAN_AT + 4 * SCAN_INTS * s
    WITW_JPEG_PLAN_PROG_SCAN_INTS = 20,
    WITW_JPEG_PLAN_PROG_SCAN_NS = 0,            // the fields of a scan record
    WITW_JPEG_PLAN_PROG_SCAN_COMPS = 1,         // + k: component of scan position k < 4
    WITW_JPEG_PLAN_PROG_SCAN_SS = 5,
    WITW_JPEG_PLAN_PROG_SCAN_SE = 6,
    WITW_JPEG_PLAN_PROG_SCAN_AH = 7,
    WITW_JPEG_PLAN_PROG_SCAN_AL = 8,
    WITW_JPEG_PLAN_PROG_SCAN_COLS = 9,          // units per row of the walk
    WITW_JPEG_PLAN_PROG_SCAN_ROWS = 10,
    WITW_JPEG_PLAN_PROG_SCAN_RESTART = 11,      // units per restart interval (0: none)
    WITW_JPEG_PLAN_PROG_SCAN_STAGE = 12,
    WITW_JPEG_PLAN_PROG_SCAN_TABLES = 13,       // byte offset in the plan
    WITW_JPEG_PLAN_PROG_SCAN_SEGS_AT = 14,      // byte offset in the plan
    WITW_JPEG_PLAN_PROG_SCAN_SEGS = 15,
    WITW_JPEG_PLAN_PROG_SCAN_DATA_END = 16,     // byte offset in the file
    WITW_JPEG_PLAN_PROG_SEG_INTS = 3,
    WITW_JPEG_PLAN_PROG_SEG_BYTE = 0,           // the fields of a segment record
    WITW_JPEG_PLAN_PROG_SEG_UNIT = 1,
    WITW_JPEG_PLAN_PROG_SEG_UNITS = 2,
    WITW_JPEG_PLAN_PROG_FIXED = 5248            // SCAN_AT + 4 * SCAN_INTS * MAX_SCANS: tables and segment records start here
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
