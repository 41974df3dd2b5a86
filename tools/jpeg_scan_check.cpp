// Stand-alone driver for the DEVICE decoder of progressive files, run on the HOST: the scan plan (witw_jpeg_scan_plan_ex,
// witw_amd/csrc_host/jpeg_coef.cpp) and the per-segment procedures the kernel runs (prog_segment of witw_amd/csrc/jpeg_entropy.h, the
// same source, compiled here as plain C++), stage by stage as witw_jpeg_progressive_stage launches them, against the host decoder
// (witw_jpeg_decode_coef_ex). File bytes (+ the 24 bytes pack() leaves behind them), plan and coefficient area live in heap blocks of
// exactly their size: built with -fsanitize=address,undefined (tests/test_jpeg_scan_plan.py) every read or write outside them shows.
//   jpeg_scan_check FILE...   ->   one line per file:
//     "<info rc> <plan bytes, or the negative code, or - when not asked> <flag: 0 clean, 1 damaged data, 2 bad plan, - no plan>
//      <host decode rc or -> <= coefficients and tables equal the host decoder's | ! they differ | - nothing to compare> <file>"
//   exit status 0 unless a file cannot be read
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../witw_amd/csrc/jpeg_entropy.h"

extern "C" {
int witw_jpeg_info_ex(const uint8_t* data, size_t n, int32_t* info, int flags);
int witw_jpeg_decode_coef_ex(const uint8_t* data, size_t n, int16_t* coef, uint16_t* qt, int flags);
long long witw_jpeg_scan_plan_bytes_ex(const uint8_t* data, size_t n, int flags);
long long witw_jpeg_scan_plan_ex(const uint8_t* data, size_t n, uint8_t* plan, size_t plan_cap, uint16_t* qt, int flags);
}

static const unsigned char ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// what jpeg_progressive_kernel does for one (file, scan) of the stage at hand; segments LAST FIRST: their order must not matter
static int run_scan(const uint8_t* bytes, size_t n_bytes, const uint8_t* plan_bytes_p, int scan, short* coef) {
    const int32_t* plan = (const int32_t*)plan_bytes_p;
    ProgScan S;
    if (!prog_scan_load(plan, scan, plan[WITW_JPEG_PLAN_PROG_BYTES], S)) return 2;
    static HuffLds tab[4];
    const int n_tab = S.Ss ? 1 : (S.Ah ? 0 : S.ns);
    const uint8_t* tsrc = plan_bytes_p + S.tables;
    const int tstride = S.Ss ? WITW_JPEG_PLAN_AC_STRIDE : WITW_JPEG_PLAN_DC_STRIDE;
    const int tsyms = S.Ss ? 256 : 16;
    for (int t = 0; t < n_tab; ++t) {
        for (int i = 0; i < 256; ++i) tab[t].sym[i] = i < tsyms ? tsrc[tstride * t + WITW_JPEG_PLAN_TABLE_SYMS + i] : (unsigned char)0;
        huff_assign_codes(tab[t], tsrc + tstride * t);
        for (int i = 0; i < (1 << HUFF_LOOK); ++i) tab[t].look[i] = huff_look_entry(tab[t], i);
    }
    const unsigned nb = (unsigned)n_bytes;
    const unsigned end_all = witw_umin((unsigned)S.data_end, nb);
    const unsigned units = (unsigned)S.cols * (unsigned)S.rows;
    const uint32_t* segs = (const uint32_t*)(plan_bytes_p + S.segs_at);
    int flag = 0;
    for (int sg = S.segs - 1; sg >= 0; --sg) {
        const uint32_t* r = segs + WITW_JPEG_PLAN_PROG_SEG_INTS * sg;
        const unsigned i0 = witw_umin(r[WITW_JPEG_PLAN_PROG_SEG_BYTE], end_all);
        unsigned i1 = sg + 1 < S.segs ? witw_umin(r[WITW_JPEG_PLAN_PROG_SEG_INTS + WITW_JPEG_PLAN_PROG_SEG_BYTE], end_all) : end_all;
        if (i1 < i0) i1 = i0;
        const unsigned u0 = witw_umin(r[WITW_JPEG_PLAN_PROG_SEG_UNIT], units);
        const unsigned u1 = u0 + witw_umin(r[WITW_JPEG_PLAN_PROG_SEG_UNITS], units - u0);
        BitReaderT<true, GlobalWords> b;
        b.start((GlobalWords)bytes, i0, i1);
        if (!prog_segment(b, (const ProgScan*)&S, (const HuffLds*)tab, coef, ZIGZAG, u0, u1)) flag = 1;
    }
    return flag;
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        fseek(f, 0, SEEK_END);
        const long size = ftell(f);
        fseek(f, 0, SEEK_SET);
        if (size < 0) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        uint8_t* data = (uint8_t*)calloc((size_t)size + 24, 1);      // 8-byte aligned (malloc), 24 readable zero bytes behind the end
        if (fread(data, 1, (size_t)size, f) != (size_t)size) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        fclose(f);
        int32_t* info = (int32_t*)calloc(WITW_JPEG_INFO_INTS, sizeof(int32_t));
        const int rc = witw_jpeg_info_ex(data, (size_t)size, info, 1);
        const int blocks = info[WITW_JPEG_INFO_BLOCKS], ncomp = info[WITW_JPEG_INFO_NCOMP];
        // (a corrupted frame header may announce up to 65,535 x 65,535 samples: such a file is not decoded here)
        if (rc < 0 || blocks <= 0 || blocks > (1 << 20)) {
            printf("%d - - - - %s\n", rc, argv[a]);
            free(info); free(data);
            continue;
        }
        int16_t* host = (int16_t*)malloc((size_t)blocks * 64 * sizeof(int16_t));
        uint16_t* host_qt = (uint16_t*)calloc((size_t)ncomp * 64, sizeof(uint16_t));
        const int host_rc = witw_jpeg_decode_coef_ex(data, (size_t)size, host, host_qt, 1);
        const long long need = witw_jpeg_scan_plan_bytes_ex(data, (size_t)size, 1);
        // a file without a plan: the code witw_jpeg_scan_plan_ex gives it (a plan area as large as any plan of this file could be: the
        // fixed part, a table per scan, a segment record per two bytes)
        const size_t cap = need > 0 ? (size_t)need : (size_t)WITW_JPEG_PLAN_PROG_FIXED + 64 * 272 + 12 * ((size_t)size / 2 + 64);
        uint8_t* plan = (uint8_t*)malloc(cap);
        uint16_t* qt = (uint16_t*)calloc((size_t)ncomp * 64, sizeof(uint16_t));
        const long long wrote = witw_jpeg_scan_plan_ex(data, (size_t)size, plan, cap, qt, 1);
        if (need <= 0 || wrote != need) {
            printf("%d %lld - %d - %s\n", rc, wrote > 0 || need > 0 ? -100 : wrote, host_rc, argv[a]);      // (-100: the two entries disagree)
        } else {
            int16_t* coef = (int16_t*)calloc((size_t)blocks * 64, sizeof(int16_t));
            const int32_t* h = (const int32_t*)plan;
            int flag = h[WITW_JPEG_PLAN_MAGIC_AT] == WITW_JPEG_PLAN_PROG_MAGIC && h[WITW_JPEG_PLAN_PROG_BLOCKS] == blocks ? 0 : 2;
            // (every stage runs whatever an earlier one flagged, as the launches do)
            for (int stage = 0; flag != 2 && stage < h[WITW_JPEG_PLAN_PROG_STAGES]; ++stage)
                for (int s = h[WITW_JPEG_PLAN_PROG_SCANS] - 1; s >= 0; --s) {
                    if (h[WITW_JPEG_PLAN_PROG_SCAN_AT / 4 + WITW_JPEG_PLAN_PROG_SCAN_INTS * s + WITW_JPEG_PLAN_PROG_SCAN_STAGE] != stage) continue;
                    const int fl = run_scan(data, (size_t)size, plan, s, coef);
                    if (fl > flag) flag = fl;
                }
            const bool same = host_rc == 0 && !memcmp(coef, host, (size_t)blocks * 128) && !memcmp(qt, host_qt, (size_t)ncomp * 128);
            printf("%d %lld %d %d %s %s\n", rc, wrote, flag, host_rc, host_rc == 0 ? (same ? "=" : "!") : "-", argv[a]);
            free(coef);
        }
        free(qt); free(plan); free(host_qt); free(host); free(info); free(data);
    }
    return 0;
}
