// What the device entropy decoders share (csrc/jpeg.hip: jpeg_huffman_kernel, jpeg_selfsync_kernel; csrc/jpeg_progressive.hip:
// jpeg_progressive_kernel): the bit reader over the file's bytes, the decoding tables as they sit in the LDS, the Huffman look-up, and
// the per-segment procedures of a progressive scan. This is the code whose indices depend on the DATA, so it also compiles for the
// HOST (plain C++: the address spaces and the __device__ decoration are macros that are empty there): tools/jpeg_scan_check.cpp runs
// the very same procedures over heap blocks of exact size under the sanitizers (tests/test_jpeg_scan_plan_san.py).
#pragma once
#include "jpeg_layout.h"

// Addresses that arrive as integers (descriptor rows) carry no address space: dereferenced as plain pointers they become FLAT accesses,
// which count on the LDS counter as well as on the memory counter. The Huffman kernels name the space of everything they touch.
#if defined(__HIPCC__)
#define WITW_ENTROPY_FN __device__ __forceinline__
#define WITW_AS_GLOBAL __attribute__((address_space(1)))
#define WITW_AS_LDS __attribute__((address_space(3)))
#else
#define WITW_ENTROPY_FN inline
#define WITW_AS_GLOBAL
#define WITW_AS_LDS
#endif

namespace {

typedef const WITW_AS_GLOBAL unsigned long long* GlobalWords;
typedef const WITW_AS_LDS unsigned long long* LdsWords;      // a copy of the bytes in the LDS (jpeg_huffman_kernel)

constexpr int HUFF_LOOK = 11;       // bits of the first-step look-up: 4 KB per table. Codes longer than that are a fraction of a per cent of the
                                    // symbols of a photograph -- with 9 bits (2-3 %) one of a wave's 64 lanes needed the second step on most symbols
struct HuffLds {
    unsigned short look[1 << HUFF_LOOK];      // prefix -> (code length << 8) | symbol; 0: the code is longer than HUFF_LOOK bits
    int valoff[17];                // symbol index of the first code of a length minus that code
    unsigned lim[17];              // lim[L] = the first 16-bit left-aligned value ABOVE every code of length <= L (non-decreasing; a length
                                   // without codes repeats its predecessor's; lim[0] = 0): a code's length is 1 + the number of limits it reaches
    unsigned char sym[256];
};

WITW_ENTROPY_FN unsigned witw_umin(unsigned a, unsigned b) { return a < b ? a : b; }

template <bool STUFFED, typename WP = GlobalWords>
struct BitReaderT {                // STUFFED: over the file's bytes of one restart interval: FF 00 -> FF on the fly, any other FF xx ends the
                                   // data; !STUFFED: over an unstuffed copy (jpeg_selfsync_kernel), positions are plain bit indices
    WP words;
    unsigned pos, end;             // byte offsets from `words`
    unsigned long long cache;      // the aligned 8 bytes that hold byte `pos`
    unsigned long long ahead;      // ... and the 8 bytes behind them, requested when `cache` was taken (the stream is read in order:
                                   // the load's round trip runs under the decoding of the current word instead of in front of the next)
    unsigned cidx;                 // which 8-byte word `cache` is (0xffffffff: none)
    unsigned long long buf;        // bits, left-aligned
    int n;                         // valid bits in buf
    int starved;                   // zero bytes fed behind the end of the data

    WITW_ENTROPY_FN unsigned raw(unsigned p) {
        if ((p >> 3) != cidx) {
            const unsigned w = p >> 3;
            cache = (w == cidx + 1u) ? ahead : words[w];
            cidx = w;
            ahead = words[w + 1u];
        }
        return (unsigned)(cache >> (8 * (p & 7))) & 0xffu;
    }
    WITW_ENTROPY_FN unsigned window32() {      // the four bytes at `pos`, first byte lowest
        const unsigned w = pos >> 3;
        if (w != cidx) {
            cache = (w == cidx + 1u) ? ahead : words[w];
            cidx = w;
            ahead = words[w + 1u];
        }
        const unsigned s = (pos & 7u) * 8u;
        unsigned w32 = (unsigned)(cache >> s);
        if (s > 32u) w32 |= (unsigned)(ahead << (64u - s));
        return w32;
    }
    // Called with fewer than 32 valid bits, tops up to at least 32. In a wave of 64 readers every path ANY lane takes is paid by all, on
    // nearly every symbol, so the common step is short and branch-free: up to FOUR bytes at once.
    //   !STUFFED: always four (behind the end of the copy lie zero bytes; the position simply runs on);
    //   STUFFED: the bytes in front of the first FF of the four (all four when there is none), never past `end`; only an FF at the very
    //   position -- a stuffed FF 00 or a marker -- and the end of the data go byte by byte.
    WITW_ENTROPY_FN void fill() {
        if (!STUFFED) {
            buf |= (unsigned long long)__builtin_bswap32(window32()) << (32 - n);
            n += 32;
            pos += 4u;
            return;
        }
        if (pos < end) {
            const unsigned w32 = window32();
            const unsigned ff = ((~w32 - 0x01010101u) & w32) & 0x80808080u;      // bit 7 of every FF byte (exact for the lowest one)
            unsigned k = ff ? (unsigned)__builtin_ctz(ff) >> 3 : 4u;
            k = witw_umin(k, end - pos);
            if (k) {
                const unsigned v = __builtin_bswap32(w32) >> (32u - 8u * k);
                buf |= (unsigned long long)v << (64 - n - 8 * (int)k);
                n += 8 * (int)k;
                pos += k;
            }
        }
        while (n < 32) {
            unsigned b = 0;
            if (pos < end) {
                b = raw(pos);
                if (b == 0xffu) {
                    const unsigned b2 = pos + 1 < end ? raw(pos + 1) : 0xd9u;
                    if (b2 == 0u) pos += 2;                    // a stuffed FF
                    else { end = pos; b = 0; ++starved; }      // a marker (the next interval's RSTn, or EOI): the data ends here
                } else {
                    ++pos;
                }
            } else {
                ++starved;
            }
            buf |= (unsigned long long)b << (56 - n);
            n += 8;
        }
    }
    WITW_ENTROPY_FN int take(int k) {   // k in 0..16 (0: nothing, returns 0), caller has >= 32 valid bits
        const int v = (int)((buf >> 1) >> (63 - k));
        buf <<= k;
        n -= k;
        return v;
    }
    WITW_ENTROPY_FN int get(int k) {    // k in 1..16, caller has >= 32 valid bits
        const int v = (int)(buf >> (64 - k));
        buf <<= k;
        n -= k;
        return v;
    }
    WITW_ENTROPY_FN void start(WP base, unsigned byte_pos, unsigned byte_end) {
        words = base;
        pos = byte_pos; end = byte_end;
        cidx = 0xfffffff0u; cache = 0; ahead = 0; buf = 0; n = 0; starved = 0;
    }
    // !STUFFED: index of the next unread bit (zero bytes fed behind the end of the data count as read: the position keeps advancing)
    WITW_ENTROPY_FN unsigned bit_pos() const { return (pos + (unsigned)starved) * 8u - (unsigned)n; }
};

template <typename BR, typename HP>      // HP: pointer to a HuffLds (jpeg_huffman_kernel: typed as an LDS pointer -- a pointer the compiler cannot place becomes a flat access)
WITW_ENTROPY_FN int huff_decode(BR& b, HP hp) {      // caller has >= 32 valid bits; -1: invalid code
    auto& h = *hp;
    const unsigned e = h.look[(unsigned)(b.buf >> (64 - HUFF_LOOK))];
    if (e) {
        const int len = (int)(e >> 8);
        b.buf <<= len;
        b.n -= len;
        return (int)(e & 255u);
    }
    // longer than the look-up: the length by comparing against the limits of the remaining lengths, no loop
    const unsigned c16 = (unsigned)(b.buf >> 48);
    int len = HUFF_LOOK + 1, vo = h.valoff[HUFF_LOOK + 1];
#pragma unroll
    for (int L = HUFF_LOOK + 1; L < 16; ++L) {
        const bool above = c16 >= h.lim[L];
        len += above ? 1 : 0;
        vo = above ? h.valoff[L + 1] : vo;
    }
    if (c16 >= h.lim[16]) return -1;
    const int code = (int)(c16 >> (16 - len));
    b.buf <<= len;
    b.n -= len;
    return h.sym[(code + vo) & 255];
}

WITW_ENTROPY_FN int jpeg_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }
WITW_ENTROPY_FN int jpeg_extend0(int v, int s) { return v < ((1 << s) >> 1) ? v - (1 << s) + 1 : v; }      // the same, and 0 for s = 0 (v = 0)

// The two steps of build_huff_tables (csrc/jpeg.hip) for ONE table, as functions of their own: the canonical codes of the 16 lengths
// from the DHT counts, then entry i of the look-up. (A damaged plan whose counts over-subscribe a length gives limits above 0x10000 and
// look-ups that point anywhere in sym[]: every index is masked to the table, nothing else is indexed with them.)
template <typename H, typename CP>      // CP: pointer to the 16 counts
WITW_ENTROPY_FN void huff_assign_codes(H& h, CP counts) {
    int code = 0, k = 0;
    h.lim[0] = 0u;
    h.valoff[0] = 0;
    for (int len = 1; len <= 16; ++len) {
        h.valoff[len] = k - code;
        const int cnt = counts[len - 1];
        k += cnt;
        code += cnt;
        h.lim[len] = (unsigned)code << (16 - len);
        code <<= 1;
    }
}

template <typename H>
WITW_ENTROPY_FN unsigned short huff_look_entry(const H& h, int i) {
    const unsigned c16 = (unsigned)i << (16 - HUFF_LOOK);
    int len = 1;
#pragma unroll
    for (int L = 1; L < HUFF_LOOK; ++L) len += c16 >= h.lim[L] ? 1 : 0;
    unsigned short v = 0;
    if (c16 < h.lim[HUFF_LOOK]) v = (unsigned short)((len << 8) | h.sym[((int)(c16 >> (16 - len)) + h.valoff[len]) & 255]);
    return v;
}

// ---- progressive scans (T.81 annex G; the procedures are dc_first / ac_first / ac_refine / the DC-refinement line of decode_scan in
// csrc_host/jpeg_coef.cpp, the same checks count as damage). One SEGMENT = one restart interval of one scan: byte-aligned, DC predictors
// and EOBRUN start at zero, so segments decode independently; scans of one stage touch disjoint (component, coefficient) cells, so
// they decode concurrently too -- provided every coefficient is read and written as the 16-bit cell it is (`short` accesses only below).

struct ProgScan {                  // one scan record of the plan, with the geometry of its components (uniform over a workgroup)
    int ns, Ss, Se, Ah, Al;
    int cols, rows;                // the walk: units per row, rows of units
    int restart, stage, tables, segs_at, segs, data_end;
    int nh[4], nv[4], bw[4];       // per scan position: blocks of the component per unit (1 x 1 in a scan of one component), its pitch
    long long first[4];            // ... and its first block
    long long blocks;              // coefficient blocks of the file: no block index reaches it
};

// Scan record `s` of the plan -> S. False: the record does not describe a scan this decoder can walk (a damaged plan): nothing of it
// is used then. Everything that later bounds a loop or enters an index is range-checked HERE, against the plan's own block count.
template <typename IP>             // IP: pointer to the plan as int32
WITW_ENTROPY_FN bool prog_scan_load(IP plan, int s, int plan_bytes, ProgScan& S) {
    const IP r = plan + WITW_JPEG_PLAN_PROG_SCAN_AT / 4 + WITW_JPEG_PLAN_PROG_SCAN_INTS * s;
    S.ns = r[WITW_JPEG_PLAN_PROG_SCAN_NS];
    S.Ss = r[WITW_JPEG_PLAN_PROG_SCAN_SS]; S.Se = r[WITW_JPEG_PLAN_PROG_SCAN_SE];
    S.Ah = r[WITW_JPEG_PLAN_PROG_SCAN_AH]; S.Al = r[WITW_JPEG_PLAN_PROG_SCAN_AL];
    S.cols = r[WITW_JPEG_PLAN_PROG_SCAN_COLS]; S.rows = r[WITW_JPEG_PLAN_PROG_SCAN_ROWS];
    S.restart = r[WITW_JPEG_PLAN_PROG_SCAN_RESTART]; S.stage = r[WITW_JPEG_PLAN_PROG_SCAN_STAGE];
    S.tables = r[WITW_JPEG_PLAN_PROG_SCAN_TABLES]; S.segs_at = r[WITW_JPEG_PLAN_PROG_SCAN_SEGS_AT];
    S.segs = r[WITW_JPEG_PLAN_PROG_SCAN_SEGS]; S.data_end = r[WITW_JPEG_PLAN_PROG_SCAN_DATA_END];
    S.blocks = plan[WITW_JPEG_PLAN_PROG_BLOCKS];
    const int ncomp = plan[WITW_JPEG_PLAN_NCOMP];
    bool ok = S.ns >= 1 && S.ns <= 4 && ncomp >= 1 && ncomp <= 3 && S.Al >= 0 && S.Al <= 13 && S.Ah >= 0 && S.Ah <= 14 && S.blocks > 0;
    ok = ok && (S.Ss == 0 ? S.Se == 0 : (S.ns == 1 && S.Ss >= 1 && S.Ss <= S.Se && S.Se <= 63));
    ok = ok && S.cols >= 1 && S.rows >= 1 && (long long)S.cols * S.rows <= 0x7fffffffLL && S.segs >= 1 && S.data_end >= 0;
    const int n_tab = S.Ss ? 1 : (S.Ah ? 0 : S.ns);
    const int tab_bytes = S.Ss ? WITW_JPEG_PLAN_AC_STRIDE : WITW_JPEG_PLAN_DC_STRIDE * n_tab;
    ok = ok && (n_tab == 0 || (S.tables >= WITW_JPEG_PLAN_PROG_FIXED && (long long)S.tables + tab_bytes <= plan_bytes));
    ok = ok && S.segs_at >= WITW_JPEG_PLAN_PROG_FIXED && (S.segs_at & 3) == 0 &&
         (long long)S.segs_at + 4LL * WITW_JPEG_PLAN_PROG_SEG_INTS * S.segs <= plan_bytes;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        S.nh[k] = S.nv[k] = 1; S.bw[k] = 1; S.first[k] = 0;
        if (ok && k < S.ns) {
            const int c = r[WITW_JPEG_PLAN_PROG_SCAN_COMPS + k];
            if (c < 0 || c >= ncomp) { ok = false; continue; }
            const IP q = plan + WITW_JPEG_PLAN_COMP + WITW_JPEG_PLAN_COMP_STRIDE * c;
            const int ch = q[WITW_JPEG_PLAN_COMP_H], cv = q[WITW_JPEG_PLAN_COMP_V];
            const int cbw = q[WITW_JPEG_PLAN_COMP_BW], cbh = q[WITW_JPEG_PLAN_COMP_BH], cfirst = q[WITW_JPEG_PLAN_COMP_FIRST];
            S.nh[k] = S.ns > 1 ? ch : 1; S.nv[k] = S.ns > 1 ? cv : 1;
            S.bw[k] = cbw; S.first[k] = cfirst;
            // the walk stays inside the component's grid, the grid inside the file's blocks
            ok = ok && ch >= 1 && ch <= 2 && cv >= 1 && cv <= 2 && cbw >= 1 && cbh >= 1 && cfirst >= 0 &&
                 (long long)cfirst + (long long)cbw * cbh <= S.blocks &&
                 (long long)S.cols * S.nh[k] <= cbw && (long long)S.rows * S.nv[k] <= cbh;
        }
    }
    return ok;
}

// Units u0 .. u1 - 1 of scan *S from the reader's position (the start of a segment). S: pointer to the scan (the kernel keeps it in the
// LDS: the per-position geometry is indexed by a loop variable); tab: the scan's tables (a first DC scan: one per scan position; an AC
// scan: tab[0]); coef: the file's coefficient area; zz: the zig-zag order. False: damaged data -- an invalid code, a DC size above 15, a
// run past Se, a refinement symbol of size other than 1, or bits taken from behind the segment's data.
// Every store is to block index < S->blocks (prog_scan_load) at a coefficient k <= Se <= 63 tested just before; EOBRUN only counts.
// The reader is topped up at ONE place per loop (filling early takes the same bits; what counts as damage is what was consumed).
template <typename BR, typename SP, typename HP, typename CP, typename ZP>
WITW_ENTROPY_FN bool prog_segment(BR& b, SP S, HP tab, CP coef, ZP zz, unsigned u0, unsigned u1) {
    const int Ss = S->Ss, Se = S->Se, Ah = S->Ah, p1 = 1 << S->Al, ns = S->ns;
    const unsigned cols = (unsigned)S->cols;
    unsigned uy = u0 / cols, ux = u0 - uy * cols;
    bool bad = false;
    if (Ss == 0) {
        int p0 = 0, pr1 = 0, pr2 = 0, pr3 = 0;                  // the DC predictors of scan positions 0..3
        for (unsigned u = u0; u < u1 && !bad; ++u) {
            for (int k = 0; k < ns && !bad; ++k) {
                const int nh = S->nh[k], nv = S->nv[k], bw = S->bw[k];
                const long long first = S->first[k];
                int pred = k == 0 ? p0 : k == 1 ? pr1 : k == 2 ? pr2 : pr3;
                for (int j = 0; j < nh * nv && !bad; ++j) {
                    const int v = j / nh, hh = j - v * nh;
                    CP blk = coef + (first + (long long)(uy * (unsigned)nv + (unsigned)v) * bw + (ux * (unsigned)nh + (unsigned)hh)) * 64;
                    if (b.n < 32) b.fill();
                    if (Ah == 0) {
                        const int s = huff_decode(b, tab + k);
                        const bool inval = s < 0 || s > 15;
                        const int sz = inval ? 0 : s;
                        pred = (short)(pred + jpeg_extend0(b.take(sz), sz));      // (kept in 16 bits, as the host keeps it)
                        if (!inval) blk[0] = (short)(pred * p1);
                        bad = inval;
                    } else if (b.take(1)) {
                        blk[0] = (short)(blk[0] | p1);
                    }
                    if (b.starved * 8 > b.n) bad = true;
                }
                p0 = k == 0 ? pred : p0; pr1 = k == 1 ? pred : pr1; pr2 = k == 2 ? pred : pr2; pr3 = k == 3 ? pred : pr3;
            }
            if (++ux == cols) { ux = 0; ++uy; }
        }
        return !bad;
    }
    const long long first0 = S->first[0];
    const int bw0 = S->bw[0];
    int eobrun = 0;
    for (unsigned u = u0; u < u1 && !bad; ++u) {
        CP blk = coef + (first0 + (long long)uy * bw0 + ux) * 64;
        if (Ah == 0) {
            if (eobrun > 0) {
                --eobrun;                                       // the band of this block is empty
            } else {
                int k = Ss;
                while (k <= Se) {
                    if (b.n < 32) b.fill();
                    const int rs = huff_decode(b, tab);
                    const int r = (rs >> 4) & 15, sz = rs < 0 ? 0 : rs & 15;
                    const int at = k + r;
                    const int val = jpeg_extend0(b.take(sz), sz);
                    if (rs < 0 || (sz && at > Se)) {
                        bad = true;
                        k = 64;
                    } else if (sz) {
                        blk[zz[at]] = (short)(val * p1);        // at <= Se <= 63
                        k = at + 1;
                    } else if (r == 15) {
                        k += 16;
                    } else {                                    // EOBr: this block and 2^r - 1 + (r bits) more end here
                        eobrun = (1 << r) - 1 + b.take(r);
                        k = 64;
                    }
                }
            }
        } else {
            // ac_refine of the host as ONE loop over the band. r < 0: the next thing in the stream is a symbol; a symbol says: pass r
            // coefficients that are still zero (ZRL: 15, and the 16th), put `val` (+-(1 << Al); 0: ZRL) on the zero one behind them;
            // or EOBr: the rest of this block's band and the bands of eobrun - 1 more blocks hold correction bits only. Every
            // coefficient that is non-zero already takes a correction bit as it is passed (G.1.2.3).
            bool in_eob = eobrun > 0;
            int r = -1, val = 0;
            for (int k = Ss; k <= Se; ++k) {
                if (b.n < 32) b.fill();                         // a symbol (<= 16 bits), its sign bit or run bits (<= 14), one correction bit
                if (!in_eob && r < 0) {
                    const int rs = huff_decode(b, tab);
                    const int sz = rs < 0 ? 0 : rs & 15;
                    r = (rs >> 4) & 15;
                    if (rs < 0 || sz > 1) {                     // no code; a refinement symbol of a size other than 1
                        bad = true;
                        r = -1; val = 0;
                        k = 64;
                    } else if (sz) {
                        val = b.take(1) ? p1 : -p1;
                    } else if (r == 15) {
                        val = 0;
                    } else {
                        eobrun = (1 << r) + b.take(r);
                        in_eob = true;
                        r = -1; val = 0;
                    }
                }
                if (k <= Se) {                                  // k <= Se <= 63
                    CP cell = blk + zz[k];
                    const int c = *cell;
                    if (c) {
                        if (b.take(1) && !(c & p1)) *cell = (short)(c + (c >= 0 ? p1 : -p1));
                    } else if (!in_eob && --r < 0 && val) {
                        *cell = (short)val;
                    }
                }
            }
            if (!in_eob && r >= 0 && val) bad = true;           // a new coefficient whose run of zeros reaches past Se
            if (in_eob && !bad) --eobrun;
        }
        // bits taken from behind the segment's own data (zero bytes fed behind its end): damaged, checked block by block
        if (b.starved * 8 > b.n) bad = true;
        if (++ux == cols) { ux = 0; ++uy; }
    }
    return !bad;
}

}  // namespace
