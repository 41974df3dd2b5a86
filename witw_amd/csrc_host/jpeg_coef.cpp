// Host side of the on-device JPEG decode (the reference decodes on the host inside its DataLoader workers:
// skimage.io.imread -> PIL -> libjpeg, model/cvig_fov.py:88-89, :402): ENTROPY decoding only -- marker parsing, Huffman decoding,
// DC prediction, de-zigzag -- of baseline / extended-sequential 8-bit JFIF files into quantised DCT coefficient blocks. Everything
// behind it (dequantisation, the integer 'islow' inverse DCT, chroma upsampling, YCbCr -> RGB) runs on the GPU
// (csrc/jpeg.hip). Plain C ABI, no GPU runtime: DataLoader workers load this library, never libwitw_hip.so.
// Opt-in (the _ex entry points with flag bit 0): PROGRESSIVE files (SOF2) too -- every scan of the file is decoded here into the same
// coefficient blocks its sequential twin would hold (decode_progressive below), so the device back end does not know the difference.
// Opt-in (flag bit 1 of the _ex entry points): 4:4:0 files (h1v2: luma 1x2, chroma 1x1 -- a losslessly rotated 4:2:2 file). An MCU is
// 8 x 16 pixels: Y (top), Y (bottom), Cb, Cr. Every decoder below takes its MCU geometry from the components' (h, v), so only parse()
// knows the flag.
//
// Coefficient layout: component c holds bh[c] x bw[c] blocks (the MCU-padded block grid, raster order), each 64 int16 in NATURAL
// (row-major) order; components follow one another. Quantisation tables: 64 uint16 per component, natural order.
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#include "../csrc/jpeg_layout.h"      // the entropy plan and the `info` ints: every index below is one of its names

namespace {

const uint8_t ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int FAST = 10;          // look-ahead bits of the decoding tables

struct Huff {
    uint8_t look_len[1 << FAST];     // FAST-bit prefix -> code length (0: longer than FAST bits)
    uint8_t look_sym[1 << FAST];
    int32_t fast_ac[1 << FAST];      // AC tables: (value << 16) | (run << 8) | (code length + magnitude bits) when code AND magnitude
                                     // bits fit the look-ahead, else 0 (the usual two-step path)
    int32_t maxcode[18];             // largest code of each length (-1: none), [17] = sentinel
    int32_t valoff[17];              // symbol index of the first code of each length minus that code
    uint8_t sym[256];
    uint8_t counts[16];              // codes per length as the DHT segment gives them (witw_jpeg_entropy_plan hands them to the device)
    int nsym;
    bool present;
};

bool build_huff(Huff& h, const uint8_t* counts, const uint8_t* symbols, int nsym, bool ac) {
    memcpy(h.sym, symbols, nsym);
    memcpy(h.counts, counts, 16);
    h.nsym = nsym;
    memset(h.look_len, 0, sizeof(h.look_len));
    memset(h.fast_ac, 0, sizeof(h.fast_ac));
    h.present = false;
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        h.valoff[len] = k - code;
        // an over-subscribed length (more codes than the code space has left) is rejected BEFORE anything is written: with
        // code + count <= 2^len every look-up index below stays under 2^FAST and k stays under nsym <= 256
        if (code + counts[len - 1] > (1 << len) || k + counts[len - 1] > nsym) return false;
        for (int i = 0; i < counts[len - 1]; ++i, ++k, ++code) {
            if (len <= FAST) {
                const int first = code << (FAST - len), n = 1 << (FAST - len);
                for (int j = 0; j < n; ++j) {
                    h.look_len[first + j] = (uint8_t)len;
                    h.look_sym[first + j] = symbols[k];
                }
            }
        }
        h.maxcode[len] = counts[len - 1] ? code - 1 : -1;
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    if (k != nsym) return false;
    h.present = true;
    if (ac)
        for (int i = 0; i < (1 << FAST); ++i) {
            const int len = h.look_len[i];
            if (!len) continue;
            const int rs = h.look_sym[i], run = rs >> 4, mag = rs & 15;
            if (mag == 0 || len + mag > FAST) continue;
            int v = (i >> (FAST - len - mag)) & ((1 << mag) - 1);       // the magnitude bits behind the code
            if (v < (1 << (mag - 1))) v -= (1 << mag) - 1;
            h.fast_ac[i] = (int32_t)((uint32_t)v << 16) | (run << 8) | (len + mag);
        }
    return true;
}

// Bit reader over the UNSTUFFED entropy-coded bytes (FF 00 -> FF done once up front; 8 zero bytes behind the end)
struct Bits {
    const uint8_t* p;
    uint64_t buf;       // bits left-aligned
    int n;              // valid bits in buf
    void init(const uint8_t* a) { p = a; buf = 0; n = 0; }
    inline void fill() {      // tops up to at least 56 valid bits: one unaligned 8-byte load, whole bytes appended
        uint64_t w;
        memcpy(&w, p, 8);
        buf |= __builtin_bswap64(w) >> n;
        const int adv = (63 - n) >> 3;
        p += adv;
        n += adv << 3;
    }
    inline int peek(int k) const { return (int)(buf >> (64 - k)); }
    inline void skip(int k) { buf <<= k; n -= k; }
    inline int get(int k) { const int v = peek(k); skip(k); return v; }
};

inline int decode_sym(Bits& b, const Huff& h) {      // caller has >= 16 valid bits
    const int look = b.peek(FAST);
    int len = h.look_len[look];
    if (len) { b.skip(len); return h.look_sym[look]; }
    len = FAST + 1;
    int code = b.peek(len);
    while (code > h.maxcode[len]) { ++len; if (len > 16) return -1; code = b.peek(len); }
    b.skip(len);
    return h.sym[(code + h.valoff[len]) & 255];
}

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

struct Comp { int id, h, v, tq, td, ta, bw, bh; int64_t off; int pred; };

struct Parsed {
    int H, W, ncomp, hmax, vmax, mcux, mcuy, restart;
    Comp c[4];
    uint16_t qt[4][64];
    bool qt_present[4];
    Huff dc[4], ac[4];
    const uint8_t* scan;      // start of the entropy-coded segment
    int scan_ncomp, scan_comp[4];
    bool jfif, adobe;         // APP0 'JFIF' / APP14 'Adobe' seen (libjpeg picks the colour space from them, jdapimin.c)
    int adobe_transform;
    bool progressive;         // SOF2 (accepted only on request): `scan` is then the length field of the FIRST SOS segment
    int status;               // 0 ok, < 0 see witw_jpeg_* below
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

bool read_dqt(Parsed& P, const uint8_t* s, int sl) {
    int k = 0;
    while (k < sl) {
        const int pq = s[k] >> 4, tq = s[k] & 15;
        ++k;
        if (tq > 3 || pq > 1 || k + 64 * (pq + 1) > sl) return false;
        for (int j = 0; j < 64; ++j) {
            P.qt[tq][ZZ[j]] = (uint16_t)(pq ? be16(s + k + 2 * j) : s[k + j]);
        }
        P.qt_present[tq] = true;
        k += 64 * (pq + 1);
    }
    return true;
}

bool read_dht(Parsed& P, const uint8_t* s, int sl) {
    int k = 0;
    while (k < sl) {
        if (k + 17 > sl) return false;
        const int tc = s[k] >> 4, th = s[k] & 15;
        if (tc > 1 || th > 3) return false;
        int nsym = 0;
        for (int j = 0; j < 16; ++j) nsym += s[k + 1 + j];
        if (nsym > 256 || k + 17 + nsym > sl) return false;
        if (!build_huff(tc ? P.ac[th] : P.dc[th], s + k + 1, s + k + 17, nsym, tc != 0)) return false;
        k += 17 + nsym;
    }
    return true;
}

// accept_progressive: a SOF2 file that meets the constraints of a sequential one parses too (P.progressive); its scans are
// validated one by one as they are decoded (decode_progressive); accept_h1v2: three components sampled (1, 2), (1, 1), (1, 1) parse too
int parse(const uint8_t* d, size_t n, Parsed& P, bool accept_progressive = false, bool accept_h1v2 = false) {
    memset(&P, 0, sizeof(P));
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return -1;
    size_t i = 2;
    bool have_sof = false;
    while (i + 4 <= n) {
        if (d[i] != 0xFF) return -1;
        while (i < n && d[i] == 0xFF) ++i;      // fill bytes
        if (i >= n) return -1;
        const int m = d[i++];
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
        if (m == 0xD9) return -1;               // EOI before a scan
        if (i + 2 > n) return -1;
        const int len = be16(d + i);
        if (len < 2 || i + len > n) return -1;
        const uint8_t* s = d + i + 2;
        const int sl = len - 2;
        if (m == 0xDB) {
            if (!read_dqt(P, s, sl)) return -1;
        } else if (m == 0xC0 || m == 0xC1 || (m == 0xC2 && accept_progressive)) {
            if (sl < 6 || s[0] != 8) return -2;                   // 8-bit samples only
            P.H = be16(s + 1); P.W = be16(s + 3); P.ncomp = s[5];
            if (P.H <= 0 || P.W <= 0 || (P.ncomp != 1 && P.ncomp != 3) || sl < 6 + 3 * P.ncomp) return -2;
            for (int c = 0; c < P.ncomp; ++c) {
                P.c[c].id = s[6 + 3 * c];
                P.c[c].h = s[7 + 3 * c] >> 4; P.c[c].v = s[7 + 3 * c] & 15;
                P.c[c].tq = s[8 + 3 * c];
                if (P.c[c].h < 1 || P.c[c].h > 2 || P.c[c].v < 1 || P.c[c].v > 2 || P.c[c].tq > 3) return -2;
            }
            have_sof = true;
            P.progressive = m == 0xC2;
        } else if (m == 0xC2 || (m >= 0xC3 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC)) {
            return -2;                                              // progressive / lossless / arithmetic: host decoder
        } else if (m == 0xC4) {
            if (!read_dht(P, s, sl)) return -1;
        } else if (m == 0xE0) {                                     // jdmarker.c examine_app0
            if (sl >= 14 && !memcmp(s, "JFIF\0", 5)) P.jfif = true;
        } else if (m == 0xEE) {                                     // jdmarker.c examine_app14
            if (sl >= 12 && !memcmp(s, "Adobe", 5)) { P.adobe = true; P.adobe_transform = s[11]; }
        } else if (m == 0xDD) {
            if (sl < 2) return -1;
            P.restart = be16(s);
        } else if (m == 0xDA) {
            if (!have_sof || sl < 1) return -1;
            if (P.progressive) { P.scan = d + i; break; }          // the first of several scans: decode_progressive walks them
            const int ns = s[0];
            if (ns != P.ncomp || sl < 1 + 2 * ns + 3) return -2;   // one interleaved scan with every component
            for (int k = 0; k < ns; ++k) {
                int ci = -1;
                for (int c = 0; c < P.ncomp; ++c) if (P.c[c].id == s[1 + 2 * k]) ci = c;
                if (ci < 0) return -1;
                P.scan_comp[k] = ci;
                P.c[ci].td = s[2 + 2 * k] >> 4; P.c[ci].ta = s[2 + 2 * k] & 15;
                if (P.c[ci].td > 3 || P.c[ci].ta > 3) return -1;
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return -2;
            P.scan_ncomp = ns;
            P.scan = d + i + len;
            break;
        }
        i += len;
    }
    if (!P.scan) return -1;
    P.hmax = P.vmax = 1;
    for (int c = 0; c < P.ncomp; ++c) { if (P.c[c].h > P.hmax) P.hmax = P.c[c].h; if (P.c[c].v > P.vmax) P.vmax = P.c[c].v; }
    if (P.ncomp == 1) { P.c[0].h = P.c[0].v = 1; P.hmax = P.vmax = 1; }      // a single-component scan is never interleaved
    else if (P.c[1].h != 1 || P.c[1].v != 1 || P.c[2].h != 1 || P.c[2].v != 1 || P.c[0].h != P.hmax || P.c[0].v != P.vmax) return -2;
    // 4:4:0 (h1v2, e.g. a losslessly rotated 4:2:2 file) goes to the host decoder unless the caller asked for it (the device back end
    // upsamples h1v1, h2v1 and h2v2 and, for these callers, h1v2)
    if (P.hmax == 1 && P.vmax == 2 && !accept_h1v2) return -2;
    // colour space as libjpeg's default_decompress_parms (jdapimin.c) decides it for three components: JFIF => YCbCr; else an
    // Adobe marker's transform flag (0 = RGB, 1 = YCbCr); else the component ids ('R','G','B' = RGB). The device back end always
    // applies YCbCr -> RGB, so every other case (and an unknown transform, which libjpeg warns about) is the host decoder's.
    if (P.ncomp == 3 && !P.jfif) {
        if (P.adobe) { if (P.adobe_transform != 1) return -2; }
        else if (P.c[0].id == 'R' && P.c[1].id == 'G' && P.c[2].id == 'B') return -2;
    }
    P.mcux = (P.W + 8 * P.hmax - 1) / (8 * P.hmax);
    P.mcuy = (P.H + 8 * P.vmax - 1) / (8 * P.vmax);
    int64_t off = 0;
    for (int c = 0; c < P.ncomp; ++c) {
        P.c[c].bw = P.mcux * P.c[c].h; P.c[c].bh = P.mcuy * P.c[c].v;
        P.c[c].off = off;
        off += (int64_t)P.c[c].bw * P.c[c].bh;
        // (a progressive file names its tables scan by scan)
        if (!P.progressive && (!P.qt_present[P.c[c].tq] || !P.dc[P.c[c].td].present || !P.ac[P.c[c].ta].present)) return -1;
    }
    return 0;
}

// one Parsed per thread, on the HEAP (not in the TLS block): a sanitizer build red-zones it, so an overrun of the tables is seen
Parsed& parsed() {
    static thread_local Parsed* p = nullptr;
    if (!p) p = new Parsed;
    return *p;
}

// The entropy-coded bytes of ONE scan, unstuffed once: FF 00 -> FF, RSTn markers dropped (their byte positions kept), any other marker
// ends the data; zeros behind the end so that the bit reader may run ahead. One per thread, reused from file to file.
struct Unstuffed {
    // PAD zero bytes behind the data: a block of a corrupt stream can read at most 64 x (16 + 15 + 1) + 63 bits = 264 bytes past the
    // end before the per-block check of the decoders stops the decode
    static constexpr size_t PAD = 512;
    uint8_t* clean = nullptr;
    size_t clean_cap = 0;
    uint32_t* rst_pos = nullptr;      // position in `clean` | number of the RSTn marker << 29
    size_t rst_cap = 0;
    size_t w = 0, n_rst = 0;          // bytes in `clean`, restart markers seen

    // q: first entropy-coded byte, e: end of the file, max_rst: restart markers the scan can hold -> where the data ended (the FF of a
    // marker, or e when the file ends first)
    const uint8_t* load(const uint8_t* q, const uint8_t* e, size_t max_rst) {
        const size_t seg = (size_t)(e - q);
        if (clean_cap < seg + PAD) { delete[] clean; clean_cap = seg + PAD + seg / 4; clean = new uint8_t[clean_cap]; }
        if (rst_cap < max_rst) { delete[] rst_pos; rst_cap = max_rst + max_rst / 4; rst_pos = new uint32_t[rst_cap]; }
        w = n_rst = 0;
        const uint8_t* end = e;
        while (q < e) {
            const uint8_t* f = (const uint8_t*)memchr(q, 0xFF, (size_t)(e - q));
            if (!f) { memcpy(clean + w, q, (size_t)(e - q)); w += (size_t)(e - q); break; }
            memcpy(clean + w, q, (size_t)(f - q));
            w += (size_t)(f - q);
            if (f + 1 >= e) break;
            const int m = f[1];
            if (m == 0) { clean[w++] = 0xFF; q = f + 2; }
            else if (m >= 0xD0 && m <= 0xD7) { if (n_rst < rst_cap) rst_pos[n_rst++] = (uint32_t)w | ((uint32_t)(m - 0xD0) << 29); q = f + 2; }
            else if (m == 0xFF) { q = f + 1; }
            else { end = f; break; }                        // EOI or another marker: the entropy-coded data ends here
        }
        memset(clean + w, 0, PAD);     // the reader loads 8 bytes at a time and may run ahead by one block
        return end;
    }
};

Unstuffed& unstuffed() {
    static thread_local Unstuffed u;
    return u;
}

void fill_info(const Parsed& P, int32_t* info) {
    info[WITW_JPEG_INFO_H] = P.H; info[WITW_JPEG_INFO_W] = P.W; info[WITW_JPEG_INFO_NCOMP] = P.ncomp;
    info[WITW_JPEG_INFO_HMAX] = P.hmax; info[WITW_JPEG_INFO_VMAX] = P.vmax;
    int64_t total = 0;
    for (int c = 0; c < 4; ++c) {
        const bool on = c < P.ncomp;
        int32_t* q = info + WITW_JPEG_INFO_COMP + WITW_JPEG_INFO_COMP_STRIDE * c;
        q[WITW_JPEG_INFO_COMP_H] = on ? P.c[c].h : 0; q[WITW_JPEG_INFO_COMP_V] = on ? P.c[c].v : 0;
        q[WITW_JPEG_INFO_COMP_BW] = on ? P.c[c].bw : 0; q[WITW_JPEG_INFO_COMP_BH] = on ? P.c[c].bh : 0;
        if (on) total += (int64_t)P.c[c].bw * P.c[c].bh;
    }
    info[WITW_JPEG_INFO_BLOCKS] = (int32_t)total;
}

// the one interleaved scan of a sequential file (P: parse() == 0) -> 0 / -3
int decode_sequential(Parsed& P, const uint8_t* data, size_t n, int16_t* coef, uint16_t* qt) {
    int64_t total = 0;
    for (int c = 0; c < P.ncomp; ++c) {
        total += (int64_t)P.c[c].bw * P.c[c].bh;
        memcpy(qt + 64 * c, P.qt[P.c[c].tq], 128);
        P.c[c].pred = 0;
    }
    memset(coef, 0, (size_t)total * 128);
    Unstuffed& U = unstuffed();
    U.load(P.scan, data + n, P.restart ? (size_t)P.mcux * P.mcuy / P.restart + 2 : 1);
    const uint8_t* const clean = U.clean;
    const uint32_t* const rst_pos = U.rst_pos;
    const size_t w = U.w, n_rst = U.n_rst;
    Bits b;
    b.init(clean);
    int to_restart = P.restart, next_rst = 0;
    size_t rst_i = 0;
    const uint8_t* const limit = clean + w + 9;             // reading this far past the data means the stream was too short
    // an interval whose symbols took bits behind its own data (the next interval's, across the RSTn marker, or the zeros behind the
    // end) is damaged: libjpeg hits the marker there and decodes zeros (jdhuff.c, insufficient data); the device decoders flag it too
    auto overran = [&](size_t seg_end) { return (size_t)(b.p - clean) * 8 - (size_t)b.n > seg_end * 8; };
    for (int my = 0; my < P.mcuy; ++my)
        for (int mx = 0; mx < P.mcux; ++mx) {
            if (P.restart && to_restart == 0) {
                if (rst_i >= n_rst || (int)(rst_pos[rst_i] >> 29) != next_rst) return -3;
                if (overran(rst_pos[rst_i] & 0x1fffffffu)) return -3;
                b.init(clean + (rst_pos[rst_i] & 0x1fffffffu));
                ++rst_i;
                next_rst = (next_rst + 1) & 7;
                to_restart = P.restart;
                for (int c = 0; c < P.ncomp; ++c) P.c[c].pred = 0;
            }
            for (int k = 0; k < P.scan_ncomp; ++k) {
                Comp& C = P.c[P.scan_comp[k]];
                const Huff& hd = P.dc[C.td];
                const Huff& ha = P.ac[C.ta];
                for (int v = 0; v < C.v; ++v)
                    for (int h = 0; h < C.h; ++h) {
                        int16_t* blk = coef + (C.off + (int64_t)(my * C.v + v) * C.bw + (mx * C.h + h)) * 64;
                        b.fill();                           // >= 56 bits: a code (<= 16) + its magnitude bits (<= 15), twice over
                        int s = decode_sym(b, hd);
                        if (s < 0 || s > 15) return -3;
                        if (s) C.pred += extend(b.get(s), s);
                        blk[0] = (int16_t)C.pred;
                        for (int kk = 1; kk < 64;) {
                            if (b.n < 32) b.fill();
                            const int32_t fa = ha.fast_ac[b.peek(FAST)];
                            if (fa) {                       // code and value in one look-up
                                kk += (fa >> 8) & 15;
                                if (kk > 63) return -3;
                                b.skip(fa & 255);
                                blk[ZZ[kk++]] = (int16_t)(fa >> 16);
                                continue;
                            }
                            const int rs = decode_sym(b, ha);
                            if (rs < 0) return -3;
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;
                                kk += 16;
                                continue;
                            }
                            kk += r;
                            if (kk > 63) return -3;
                            blk[ZZ[kk]] = (int16_t)extend(b.get(s), s);
                            ++kk;
                        }
                        if (b.p > limit) return -3;
                    }
            }
            if (P.restart) --to_restart;
        }
    if (overran(w)) return -3;
    return 0;
}

// ---- progressive files (T.81 annex G; the procedures are those of libjpeg's jdphuff.c). The scans of a file refine one set of
// coefficient blocks: a DC scan (Ss = 0) codes the DC differences of one or several components down to bit Al, or (Ah > 0) one more
// bit of each; an AC scan codes the band Ss..Se of ONE component down to bit Al, with runs of blocks whose band is empty folded into
// one EOBn symbol (EOBRUN, up to 32,767 blocks), or (Ah > 0) one more bit of it: a correction bit for every coefficient that is
// non-zero already, new coefficients of +-(1 << Al) between them. A scan of one component walks THAT component's own block grid
// (ceil(w_c / 8) x ceil(h_c / 8), raster order), not the MCU-padded grid of the coefficient area.

inline int get_bit(Bits& b) { if (b.n < 1) b.fill(); return b.get(1); }

struct ScanHeader { int ns, comp[4], Ss, Se, Ah, Al; };

inline int dc_first(Bits& b, const Huff& hd, int16_t* blk, int Al, int& pred) {
    if (b.n < 32) b.fill();
    const int s = decode_sym(b, hd);
    if (s < 0 || s > 15) return -3;
    if (s) pred = (int16_t)(pred + extend(b.get(s), s));      // (kept in 16 bits: a hostile stream cannot overflow the sum)
    blk[0] = (int16_t)(pred * (1 << Al));
    return 0;
}

inline int ac_first(Bits& b, const Huff& ha, int16_t* blk, const ScanHeader& S, int& eobrun) {
    if (eobrun > 0) { --eobrun; return 0; }                       // the band of this block is empty
    for (int k = S.Ss; k <= S.Se;) {
        if (b.n < 32) b.fill();
        const int32_t fa = ha.fast_ac[b.peek(FAST)];
        if (fa) {                                                 // code and value in one look-up
            k += (fa >> 8) & 15;
            if (k > S.Se) return -3;
            b.skip(fa & 255);
            blk[ZZ[k++]] = (int16_t)((fa >> 16) * (1 << S.Al));
            continue;
        }
        const int rs = decode_sym(b, ha);
        if (rs < 0) return -3;
        const int r = rs >> 4, s = rs & 15;
        if (s) {
            k += r;
            if (k > S.Se) return -3;
            blk[ZZ[k++]] = (int16_t)(extend(b.get(s), s) * (1 << S.Al));
        } else if (r == 15) {
            k += 16;
        } else {                                                  // EOBr: this block and 2^r - 1 + (r bits) more end here
            eobrun = (1 << r) - 1;
            if (r) eobrun += b.get(r);
            break;
        }
    }
    return 0;
}

inline int ac_refine(Bits& b, const Huff& ha, int16_t* blk, const ScanHeader& S, int& eobrun) {
    const int p1 = 1 << S.Al, m1 = -p1;
    auto correct = [&](int16_t& c) { if (get_bit(b) && !(c & p1)) c = (int16_t)(c + (c >= 0 ? p1 : m1)); };
    int k = S.Ss;
    if (eobrun == 0) {
        while (k <= S.Se) {
            if (b.n < 32) b.fill();
            const int rs = decode_sym(b, ha);
            if (rs < 0) return -3;
            int r = rs >> 4, val = 0;
            if (rs & 15) {                                        // a new coefficient behind r zero ones: size 1, a sign bit
                if ((rs & 15) != 1) return -3;
                val = b.get(1) ? p1 : m1;
            } else if (r != 15) {                                 // EOBr: the rest of this block's band below, then 2^r - 1 + (r bits) blocks
                eobrun = 1 << r;
                if (r) eobrun += b.get(r);
                break;
            }
            // pass r coefficients that are still zero (ZRL: 16 of them); the non-zero ones on the way take a correction bit each
            for (; k <= S.Se; ++k) {
                int16_t& c = blk[ZZ[k]];
                if (c) correct(c);
                else if (--r < 0) break;
            }
            if (val) {
                if (k > S.Se) return -3;
                blk[ZZ[k]] = (int16_t)val;
            }
            ++k;
        }
    }
    if (eobrun > 0) {                                             // inside an EOB run: correction bits only
        for (; k <= S.Se; ++k)
            if (blk[ZZ[k]]) correct(blk[ZZ[k]]);
        --eobrun;
    }
    return 0;
}

// the entropy-coded data of one scan, loaded into U -> 0 / -3
int decode_scan(Parsed& P, const ScanHeader& S, const Unstuffed& U, int16_t* coef) {
    const uint8_t* const clean = U.clean;
    const bool interleaved = S.ns > 1;
    int cols = P.mcux, rows = P.mcuy;
    if (!interleaved) {                                           // the component's own blocks
        const Comp& C = P.c[S.comp[0]];
        cols = ((P.W * C.h + P.hmax - 1) / P.hmax + 7) / 8;
        rows = ((P.H * C.v + P.vmax - 1) / P.vmax + 7) / 8;
    }
    Bits b;
    b.init(clean);
    int to_restart = P.restart, next_rst = 0, eobrun = 0;
    size_t rst_i = 0;
    auto interval_end = [&]() { return rst_i < U.n_rst ? (size_t)(U.rst_pos[rst_i] & 0x1fffffffu) : U.w; };
    size_t seg_end = interval_end();
    for (int c = 0; c < P.ncomp; ++c) P.c[c].pred = 0;
    for (int my = 0; my < rows; ++my)
        for (int mx = 0; mx < cols; ++mx) {
            if (P.restart && to_restart == 0) {
                if (rst_i >= U.n_rst || (int)(U.rst_pos[rst_i] >> 29) != next_rst) return -3;
                b.init(clean + seg_end);
                ++rst_i;
                seg_end = interval_end();
                next_rst = (next_rst + 1) & 7;
                to_restart = P.restart;
                eobrun = 0;
                for (int c = 0; c < P.ncomp; ++c) P.c[c].pred = 0;
            }
            for (int k = 0; k < S.ns; ++k) {
                Comp& C = P.c[S.comp[k]];
                const int nh = interleaved ? C.h : 1, nv = interleaved ? C.v : 1;
                for (int v = 0; v < nv; ++v)
                    for (int h = 0; h < nh; ++h) {
                        int16_t* blk = coef + (C.off + (int64_t)(my * nv + v) * C.bw + (mx * nh + h)) * 64;
                        int rc = 0;
                        if (S.Ss == 0) {
                            if (S.Ah == 0) rc = dc_first(b, P.dc[C.td], blk, S.Al, C.pred);
                            else if (get_bit(b)) blk[0] |= (int16_t)(1 << S.Al);
                        } else {
                            rc = S.Ah == 0 ? ac_first(b, P.ac[C.ta], blk, S, eobrun) : ac_refine(b, P.ac[C.ta], blk, S, eobrun);
                        }
                        if (rc) return rc;
                        // bits taken from behind the interval's own data (the next interval's, or the zeros behind the end): damaged.
                        // Checked block by block, so that at most the block at the damage holds anything decoded from them
                        if ((size_t)(b.p - clean) * 8 - (size_t)b.n > seg_end * 8) return -3;
                    }
            }
            if (P.restart) --to_restart;
        }
    return 0;
}

// P: parse(accept_progressive) == 0 and P.progressive. Walks the marker segments from the first SOS to EOI: tables and the restart
// interval may change between scans; every scan is checked against what the earlier ones left (bits[c][k]: the bit position
// coefficient k of component c has been refined down to, -1 = not coded yet -- libjpeg's coef_bits, but an inconsistency is an error
// here where libjpeg warns and goes on). -> 0; -2 = the file ends before every coefficient has reached bit 0 (libjpeg smooths
// such a file between blocks: its pixels are not those of these coefficients); -3 = damaged
int decode_progressive(Parsed& P, const uint8_t* d, size_t n, int16_t* coef, uint16_t* qt) {
    int64_t total = 0;
    for (int c = 0; c < P.ncomp; ++c) {
        total += (int64_t)P.c[c].bw * P.c[c].bh;
        memcpy(qt + 64 * c, P.qt[P.c[c].tq], 128);
    }
    memset(coef, 0, (size_t)total * 128);
    int8_t bits[4][64];
    memset(bits, -1, sizeof(bits));
    bool latched[4] = {false, false, false, false};      // a component keeps the quantisation table in force at its first scan (jdinput.c)
    Unstuffed& U = unstuffed();
    size_t i = (size_t)(P.scan - d);                     // the length field of a marker segment
    for (int m = 0xDA; m != 0xD9;) {
        if (i + 2 > n) return -3;
        const int len = be16(d + i);
        if (len < 2 || i + len > n) return -3;
        const uint8_t* s = d + i + 2;
        const int sl = len - 2;
        i += len;
        if (m == 0xDB) {
            if (!read_dqt(P, s, sl)) return -3;
        } else if (m == 0xC4) {
            if (!read_dht(P, s, sl)) return -3;
        } else if (m == 0xDD) {
            if (sl < 2) return -3;
            P.restart = be16(s);
        } else if (m == 0xDA) {
            ScanHeader S;
            S.ns = sl ? s[0] : 0;
            if (S.ns < 1 || S.ns > P.ncomp || sl < 1 + 2 * S.ns + 3) return -3;
            S.Ss = s[1 + 2 * S.ns]; S.Se = s[2 + 2 * S.ns]; S.Ah = s[3 + 2 * S.ns] >> 4; S.Al = s[3 + 2 * S.ns] & 15;
            // T.81 G.1.1.1.1 / jdphuff.c start_pass_phuff_decoder: DC alone, an AC band of one component, one bit per refinement
            if (S.Ss == 0 ? S.Se != 0 : (S.Ss > S.Se || S.Se > 63 || S.ns != 1)) return -3;
            if (S.Al > 13 || (S.Ah && S.Ah != S.Al + 1)) return -3;
            for (int k = 0; k < S.ns; ++k) {
                int ci = -1;
                for (int c = 0; c < P.ncomp; ++c) if (P.c[c].id == s[1 + 2 * k]) ci = c;
                for (int j = 0; j < k; ++j) if (S.comp[j] == ci) ci = -1;
                if (ci < 0) return -3;
                S.comp[k] = ci;
                Comp& C = P.c[ci];
                C.td = s[2 + 2 * k] >> 4; C.ta = s[2 + 2 * k] & 15;
                if (C.td > 3 || C.ta > 3) return -3;
                if (S.Ss == 0 ? (S.Ah == 0 && !P.dc[C.td].present) : !P.ac[C.ta].present) return -3;
                if (S.Ss && bits[ci][0] < 0) return -3;                                   // AC before the component's DC
                for (int kk = S.Ss; kk <= S.Se; ++kk) {
                    if (bits[ci][kk] != (S.Ah ? S.Ah : -1)) return -3;                    // coded twice, or not down to Ah yet
                    bits[ci][kk] = (int8_t)S.Al;
                }
                if (!latched[ci]) {
                    if (!P.qt_present[C.tq]) return -3;
                    memcpy(qt + 64 * ci, P.qt[C.tq], 128);
                    latched[ci] = true;
                }
            }
            const Comp& C0 = P.c[S.comp[0]];
            const size_t units = S.ns > 1 ? (size_t)P.mcux * P.mcuy : (size_t)C0.bw * C0.bh;
            const uint8_t* end = U.load(d + i, d + n, P.restart ? units / P.restart + 2 : 1);
            const int rc = decode_scan(P, S, U, coef);
            if (rc) return rc;
            i = (size_t)(end - d);
        } else if (m >= 0xC0 && m <= 0xCF) {
            return -3;                                                                    // a second frame header, arithmetic conditioning
        }                                                                                 // (APPn, COM, ...: skipped)
        if (i + 2 > n || d[i] != 0xFF) return -3;                                         // no EOI: the file is cut short
        while (i < n && d[i] == 0xFF) ++i;
        if (i >= n) return -3;
        m = d[i++];
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m <= 0x01) return -3;               // no segment, and none of them belongs here
    }
    for (int c = 0; c < P.ncomp; ++c)
        for (int k = 0; k < 64; ++k)
            if (bits[c][k] != 0) return -2;
    return 0;
}

// ---- the scan plan of a progressive file (csrc/jpeg_layout.h, 'JPW2'): what the DEVICE needs to decode the scans itself
// (csrc/jpeg_progressive.hip). The walk of decode_progressive with every check that needs no Huffman decoding; where that one loads and
// decodes a scan's data, this one only looks for the markers in it. A byte scan: no Huffman decoding, no pass over coefficients.

struct PlanOut {                      // base == nullptr: count the bytes only
    uint8_t* base;
    size_t cap, at;
    bool put(const void* src, size_t len) {
        if (base) {
            if (at + len > cap) return false;
            memcpy(base + at, src, len);
        }
        at += len;
        return true;
    }
};

// P: parse(accept_progressive) == 0 and P.progressive -> the plan's size in bytes; -1 = plan_cap is too small; -2 = a file left to the
// host route (more than PROG_MAX_SCANS scans, a DC table of more than 16 symbols, scans that stop short of bit 0); -3 = a scan, a
// segment or the restart markers are not what decode_progressive accepts
long long scan_plan(Parsed& P, const uint8_t* d, size_t n, uint8_t* plan, size_t plan_cap, uint16_t* qt) {
    PlanOut out = {plan, plan_cap, (size_t)WITW_JPEG_PLAN_PROG_FIXED};
    if (plan) {
        if (plan_cap < (size_t)WITW_JPEG_PLAN_PROG_FIXED) return -1;
        memset(plan, 0, (size_t)WITW_JPEG_PLAN_PROG_FIXED);
    }
    int32_t* const h = reinterpret_cast<int32_t*>(plan);
    int64_t total = 0;
    for (int c = 0; c < P.ncomp; ++c) {
        total += (int64_t)P.c[c].bw * P.c[c].bh;
        if (qt) memcpy(qt + 64 * c, P.qt[P.c[c].tq], 128);
    }
    if (total > 0x7fffffff) return -2;
    int8_t bits[4][64], cell_stage[4][64];
    memset(bits, -1, sizeof(bits));
    memset(cell_stage, -1, sizeof(cell_stage));
    bool latched[4] = {false, false, false, false};
    int n_scans = 0, stages = 0;
    long long n_segments = 0, max_segments = 0;
    size_t i = (size_t)(P.scan - d);
    for (int m = 0xDA; m != 0xD9;) {
        if (i + 2 > n) return -3;
        const int len = be16(d + i);
        if (len < 2 || i + len > n) return -3;
        const uint8_t* s = d + i + 2;
        const int sl = len - 2;
        i += len;
        if (m == 0xDB) {
            if (!read_dqt(P, s, sl)) return -3;
        } else if (m == 0xC4) {
            if (!read_dht(P, s, sl)) return -3;
        } else if (m == 0xDD) {
            if (sl < 2) return -3;
            P.restart = be16(s);
        } else if (m == 0xDA) {
            ScanHeader S;
            S.ns = sl ? s[0] : 0;
            if (S.ns < 1 || S.ns > P.ncomp || sl < 1 + 2 * S.ns + 3) return -3;
            S.Ss = s[1 + 2 * S.ns]; S.Se = s[2 + 2 * S.ns]; S.Ah = s[3 + 2 * S.ns] >> 4; S.Al = s[3 + 2 * S.ns] & 15;
            if (S.Ss == 0 ? S.Se != 0 : (S.Ss > S.Se || S.Se > 63 || S.ns != 1)) return -3;
            if (S.Al > 13 || (S.Ah && S.Ah != S.Al + 1)) return -3;
            int stage = 0;
            for (int k = 0; k < S.ns; ++k) {
                int ci = -1;
                for (int c = 0; c < P.ncomp; ++c) if (P.c[c].id == s[1 + 2 * k]) ci = c;
                for (int j = 0; j < k; ++j) if (S.comp[j] == ci) ci = -1;
                if (ci < 0) return -3;
                S.comp[k] = ci;
                Comp& C = P.c[ci];
                C.td = s[2 + 2 * k] >> 4; C.ta = s[2 + 2 * k] & 15;
                if (C.td > 3 || C.ta > 3) return -3;
                if (S.Ss == 0 ? (S.Ah == 0 && !P.dc[C.td].present) : !P.ac[C.ta].present) return -3;
                if (S.Ss && bits[ci][0] < 0) return -3;
                for (int kk = S.Ss; kk <= S.Se; ++kk) {
                    if (bits[ci][kk] != (S.Ah ? S.Ah : -1)) return -3;
                    bits[ci][kk] = (int8_t)S.Al;
                    if (cell_stage[ci][kk] + 1 > stage) stage = cell_stage[ci][kk] + 1;
                }
                if (!latched[ci]) {
                    if (!P.qt_present[C.tq]) return -3;
                    if (qt) memcpy(qt + 64 * ci, P.qt[C.tq], 128);
                    latched[ci] = true;
                }
            }
            for (int k = 0; k < S.ns; ++k)
                for (int kk = S.Ss; kk <= S.Se; ++kk) cell_stage[S.comp[k]][kk] = (int8_t)stage;
            if (n_scans == WITW_JPEG_PLAN_PROG_MAX_SCANS) return -2;
            const Comp& C0 = P.c[S.comp[0]];
            long long cols = P.mcux, rows = P.mcuy;
            if (S.ns == 1) {
                cols = ((P.W * C0.h + P.hmax - 1) / P.hmax + 7) / 8;
                rows = ((P.H * C0.v + P.vmax - 1) / P.vmax + 7) / 8;
            }
            const long long units = cols * rows;
            if (units > 0x7fffffff) return -2;
            const long long n_int = P.restart > 0 ? (units + P.restart - 1) / P.restart : 1;
            int32_t rec[WITW_JPEG_PLAN_PROG_SCAN_INTS];
            memset(rec, 0, sizeof(rec));
            rec[WITW_JPEG_PLAN_PROG_SCAN_NS] = S.ns;
            for (int k = 0; k < S.ns; ++k) rec[WITW_JPEG_PLAN_PROG_SCAN_COMPS + k] = S.comp[k];
            rec[WITW_JPEG_PLAN_PROG_SCAN_SS] = S.Ss; rec[WITW_JPEG_PLAN_PROG_SCAN_SE] = S.Se;
            rec[WITW_JPEG_PLAN_PROG_SCAN_AH] = S.Ah; rec[WITW_JPEG_PLAN_PROG_SCAN_AL] = S.Al;
            rec[WITW_JPEG_PLAN_PROG_SCAN_COLS] = (int32_t)cols; rec[WITW_JPEG_PLAN_PROG_SCAN_ROWS] = (int32_t)rows;
            rec[WITW_JPEG_PLAN_PROG_SCAN_RESTART] = P.restart > 0 ? P.restart : 0;
            rec[WITW_JPEG_PLAN_PROG_SCAN_STAGE] = stage;
            rec[WITW_JPEG_PLAN_PROG_SCAN_SEGS] = (int32_t)n_int;
            // the tables in force now, only those the scan decodes with
            if (S.Ss == 0 ? S.Ah == 0 : true) rec[WITW_JPEG_PLAN_PROG_SCAN_TABLES] = (int32_t)out.at;
            if (S.Ss == 0 && S.Ah == 0) {
                for (int k = 0; k < S.ns; ++k) {
                    const Huff& hf = P.dc[P.c[S.comp[k]].td];
                    if (hf.nsym > 16) return -2;
                    uint8_t t[WITW_JPEG_PLAN_DC_STRIDE];
                    memset(t, 0, sizeof(t));
                    memcpy(t, hf.counts, 16);
                    memcpy(t + WITW_JPEG_PLAN_TABLE_SYMS, hf.sym, (size_t)hf.nsym);
                    if (!out.put(t, sizeof(t))) return -1;
                }
            } else if (S.Ss) {
                const Huff& hf = P.ac[C0.ta];
                uint8_t t[WITW_JPEG_PLAN_AC_STRIDE];
                memset(t, 0, sizeof(t));
                memcpy(t, hf.counts, 16);
                memcpy(t + WITW_JPEG_PLAN_TABLE_SYMS, hf.sym, (size_t)hf.nsym);
                if (!out.put(t, sizeof(t))) return -1;
            }
            rec[WITW_JPEG_PLAN_PROG_SCAN_SEGS_AT] = (int32_t)out.at;
            // the segments: the markers of the scan's data as Unstuffed::load reads them, RSTn in sequence and n_int - 1 of them
            const uint8_t* q = d + i;
            const uint8_t* const e = d + n;
            const uint8_t* end = e;
            long long found = 0;
            int next_rst = 0;
            auto segment = [&](size_t byte_at, long long k) {
                const long long first = P.restart > 0 ? k * P.restart : 0;
                const long long left = units - first;
                const uint32_t r[WITW_JPEG_PLAN_PROG_SEG_INTS] = {(uint32_t)byte_at, (uint32_t)first,
                                                                   (uint32_t)(P.restart > 0 && P.restart < left ? P.restart : left)};
                return out.put(r, sizeof(r));
            };
            if (!segment(i, 0)) return -1;
            while (q < e) {
                const uint8_t* f = (const uint8_t*)memchr(q, 0xFF, (size_t)(e - q));
                if (!f || f + 1 >= e) break;
                const int mk = f[1];
                if (mk == 0) { q = f + 2; continue; }
                if (mk == 0xFF) { q = f + 1; continue; }
                if (mk >= 0xD0 && mk <= 0xD7) {
                    if (mk - 0xD0 != next_rst || found + 1 >= n_int) return -3;
                    next_rst = (next_rst + 1) & 7;
                    ++found;
                    if (!segment((size_t)(f + 2 - d), found)) return -1;
                    q = f + 2;
                    continue;
                }
                end = f;
                break;
            }
            if (found != n_int - 1) return -3;
            rec[WITW_JPEG_PLAN_PROG_SCAN_DATA_END] = (int32_t)(end - d);
            if (plan) memcpy(plan + WITW_JPEG_PLAN_PROG_SCAN_AT + sizeof(rec) * (size_t)n_scans, rec, sizeof(rec));
            ++n_scans;
            n_segments += n_int;
            if (n_int > max_segments) max_segments = n_int;
            if (stage + 1 > stages) stages = stage + 1;
            i = (size_t)(end - d);
        } else if (m >= 0xC0 && m <= 0xCF) {
            return -3;
        }
        if (i + 2 > n || d[i] != 0xFF) return -3;
        while (i < n && d[i] == 0xFF) ++i;
        if (i >= n) return -3;
        m = d[i++];
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m <= 0x01) return -3;
    }
    for (int c = 0; c < P.ncomp; ++c)
        for (int k = 0; k < 64; ++k)
            if (bits[c][k] != 0) return -2;
    if (n_segments > 0x7fffffff || out.at > 0x7fffffff) return -2;
    if (plan) {
        h[WITW_JPEG_PLAN_MAGIC_AT] = WITW_JPEG_PLAN_PROG_MAGIC;
        h[WITW_JPEG_PLAN_PROG_SCANS] = n_scans; h[WITW_JPEG_PLAN_PROG_SEGMENTS] = (int32_t)n_segments;
        h[WITW_JPEG_PLAN_MCUX] = P.mcux; h[WITW_JPEG_PLAN_MCUY] = P.mcuy; h[WITW_JPEG_PLAN_NCOMP] = P.ncomp;
        for (int c = 0; c < P.ncomp; ++c) {
            int32_t* q = h + WITW_JPEG_PLAN_COMP + WITW_JPEG_PLAN_COMP_STRIDE * c;
            q[WITW_JPEG_PLAN_COMP_H] = P.c[c].h; q[WITW_JPEG_PLAN_COMP_V] = P.c[c].v;
            q[WITW_JPEG_PLAN_COMP_BW] = P.c[c].bw; q[WITW_JPEG_PLAN_COMP_BH] = P.c[c].bh; q[WITW_JPEG_PLAN_COMP_FIRST] = (int32_t)P.c[c].off;
        }
        h[WITW_JPEG_PLAN_PROG_STAGES] = stages; h[WITW_JPEG_PLAN_PROG_MAX_SEGMENTS] = (int32_t)max_segments;
        h[WITW_JPEG_PLAN_PROG_BLOCKS] = (int32_t)total; h[WITW_JPEG_PLAN_PROG_BYTES] = (int32_t)out.at;
    }
    return (long long)out.at;
}

}  // namespace

extern "C" {

// flags bit 0 = accept progressive files (SOF2) that meet the constraints below (8-bit, 1 or 3 components, the same samplings and
// colour spaces); bit 1 = accept 4:4:0 sampling (h1v2: luma (h, v) = (1, 2), both chroma (1, 1)) beside the samplings below -- a
// progressive 4:4:0 file needs both bits; every other bit is reserved (0). With flags == 0 the entries are their plain namesakes.
enum { WITW_JPEG_ACCEPT_PROGRESSIVE = 1, WITW_JPEG_ACCEPT_H1V2 = 2 };

// info: the WITW_JPEG_INFO_INTS ints of csrc/jpeg_layout.h (H, W, ncomp, hmax, vmax, total blocks, then per component (4 slots): h, v,
// blocks wide, blocks high).
// Returns 0; 1 = a progressive file this decoder takes (only the header has been looked at: witw_jpeg_decode_coef_ex says whether its
// scans are legal and complete); -1 = not a decodable JPEG stream; -2 = a JPEG this decoder leaves to the host library (progressive
// without bit 0, arithmetic, 12-bit, CMYK, non-interleaved scans, sampling other than 4:4:4 / 4:2:2 (h2v1) / 4:2:0 / grey (4:4:0: bit 1),
// RGB-colourspace files: Adobe transform 0 or component ids 'R','G','B' without a JFIF marker).
int witw_jpeg_info_ex(const uint8_t* data, size_t n, int32_t* info /* 22 */, int flags) {
    Parsed& P = parsed();
    const int rc = parse(data, n, P, (flags & WITW_JPEG_ACCEPT_PROGRESSIVE) != 0, (flags & WITW_JPEG_ACCEPT_H1V2) != 0);
    if (rc) return rc;
    fill_info(P, info);
    return P.progressive ? 1 : 0;
}

int witw_jpeg_info(const uint8_t* data, size_t n, int32_t* info /* 22 */) { return witw_jpeg_info_ex(data, n, info, 0); }

// coef: total blocks x 64 int16 (zero-filled here); qt: ncomp x 64 uint16. Returns 0 or a negative code as above; -3 = the
// entropy-coded data ended early or holds an invalid code (the blocks decoded so far are kept, the rest stay zero). A progressive
// file gives the blocks its sequential twin would; for it -3 also = a scan the earlier scans do not allow (Ss / Se / Ah / Al), and
// -2 = the file ends before every coefficient of every component has been refined down to bit 0 (the host library smooths such a
// file: leave it there).
int witw_jpeg_decode_coef_ex(const uint8_t* data, size_t n, int16_t* coef, uint16_t* qt, int flags) {
    Parsed& P = parsed();
    const int rc = parse(data, n, P, (flags & WITW_JPEG_ACCEPT_PROGRESSIVE) != 0, (flags & WITW_JPEG_ACCEPT_H1V2) != 0);
    if (rc) return rc;
    return P.progressive ? decode_progressive(P, data, n, coef, qt) : decode_sequential(P, data, n, coef, qt);
}

int witw_jpeg_decode_coef(const uint8_t* data, size_t n, int16_t* coef, uint16_t* qt) { return witw_jpeg_decode_coef_ex(data, n, coef, qt, 0); }

// ---- entropy decoding ON THE DEVICE for files that carry restart markers (csrc/jpeg.hip, jpeg_huffman_kernel: one GPU thread per
// restart interval). What is left for the host is a byte scan: the header, and the positions of the RSTn markers in the entropy-coded
// segment (memchr over ~80 KB per 512 x 512 image instead of decoding ~60 k Huffman symbols). The plan written here is what the
// kernel reads beside the FILE BYTES themselves; its layout is described, and named, in csrc/jpeg_layout.h.

// (flags: bit 1 as above; a progressive file has no ENTROPY plan whatever bit 0 says: its scans refine one another -- what the device
// needs for such a file is the scan plan, witw_jpeg_scan_plan_ex below)
long long witw_jpeg_entropy_plan_bytes_ex(const uint8_t* data, size_t n, int flags) {      // 0: not a file for this decoder
    Parsed& P = parsed();
    if (parse(data, n, P, false, (flags & WITW_JPEG_ACCEPT_H1V2) != 0)) return 0;
    if (P.restart <= 0) return WITW_JPEG_PLAN_FIXED + 4;      // no restart markers: ONE interval, decoded by the self-synchronising kernel
    const long long mcus = (long long)P.mcux * P.mcuy;
    return WITW_JPEG_PLAN_FIXED + 4 * ((mcus + P.restart - 1) / P.restart);
}

long long witw_jpeg_entropy_plan_bytes(const uint8_t* data, size_t n) { return witw_jpeg_entropy_plan_bytes_ex(data, n, 0); }

// plan: plan_cap bytes (witw_jpeg_entropy_plan_bytes); qt: ncomp x 64 uint16 (as witw_jpeg_decode_coef writes them).
// Returns the plan's size in bytes, or -1 / -2 as witw_jpeg_info, -2 also for files with more than two Huffman tables of a kind in
// use, -3 when the restart markers found do not number intervals - 1 in sequence.
long long witw_jpeg_entropy_plan_ex(const uint8_t* data, size_t n, uint8_t* plan, size_t plan_cap, uint16_t* qt, int flags) {
    Parsed& P = parsed();
    const int rc = parse(data, n, P, false, (flags & WITW_JPEG_ACCEPT_H1V2) != 0);
    if (rc) return rc;
    // no restart markers: the whole scan is ONE interval ([2] = every MCU of the image); the device finds its way into the middle of
    // it by self-synchronisation (csrc/jpeg.hip, jpeg_selfsync_kernel)
    const long long mcus = (long long)P.mcux * P.mcuy;
    if (P.restart <= 0) {
        if (mcus > 0x7fffffff) return -2;
        P.restart = (int)mcus;
    }
    const long long n_int = (mcus + P.restart - 1) / P.restart;
    const long long need = WITW_JPEG_PLAN_FIXED + 4 * n_int;
    if ((long long)plan_cap < need || n_int > 0x7fffffff) return -1;
    memset(plan, 0, (size_t)need);
    int32_t* h = reinterpret_cast<int32_t*>(plan);
    h[WITW_JPEG_PLAN_MAGIC_AT] = WITW_JPEG_PLAN_MAGIC;
    h[WITW_JPEG_PLAN_INTERVALS] = (int32_t)n_int; h[WITW_JPEG_PLAN_INTERVAL_MCUS] = P.restart;
    h[WITW_JPEG_PLAN_MCUX] = P.mcux; h[WITW_JPEG_PLAN_MCUY] = P.mcuy; h[WITW_JPEG_PLAN_NCOMP] = P.ncomp;
    int dc_slot[4] = {-1, -1, -1, -1}, ac_slot[4] = {-1, -1, -1, -1}, n_dc = 0, n_ac = 0;
    for (int c = 0; c < P.ncomp; ++c) {
        if (dc_slot[P.c[c].td] < 0) { if (n_dc == 2) return -2; dc_slot[P.c[c].td] = n_dc++; }
        if (ac_slot[P.c[c].ta] < 0) { if (n_ac == 2) return -2; ac_slot[P.c[c].ta] = n_ac++; }
        int32_t* q = h + WITW_JPEG_PLAN_COMP + WITW_JPEG_PLAN_COMP_STRIDE * c;
        q[WITW_JPEG_PLAN_COMP_H] = P.c[c].h; q[WITW_JPEG_PLAN_COMP_V] = P.c[c].v;
        q[WITW_JPEG_PLAN_COMP_BW] = P.c[c].bw; q[WITW_JPEG_PLAN_COMP_BH] = P.c[c].bh; q[WITW_JPEG_PLAN_COMP_FIRST] = (int32_t)P.c[c].off;
        q[WITW_JPEG_PLAN_COMP_DC] = dc_slot[P.c[c].td]; q[WITW_JPEG_PLAN_COMP_AC] = ac_slot[P.c[c].ta];
        memcpy(qt + 64 * c, P.qt[P.c[c].tq], 128);
    }
    for (int k = 0; k < P.scan_ncomp && k < 3; ++k) h[WITW_JPEG_PLAN_SCAN_COMP + k] = P.scan_comp[k];
    for (int t = 0; t < 4; ++t) {
        if (dc_slot[t] >= 0) {
            const Huff& hf = P.dc[t];
            if (hf.nsym > 16) return -2;                              // a DC table holds at most 12 categories (16 leaves room)
            uint8_t* d = plan + WITW_JPEG_PLAN_DC + WITW_JPEG_PLAN_DC_STRIDE * dc_slot[t];
            memcpy(d, hf.counts, 16);
            memcpy(d + WITW_JPEG_PLAN_TABLE_SYMS, hf.sym, (size_t)hf.nsym);
        }
        if (ac_slot[t] >= 0) {
            const Huff& hf = P.ac[t];
            uint8_t* d = plan + WITW_JPEG_PLAN_AC + WITW_JPEG_PLAN_AC_STRIDE * ac_slot[t];
            memcpy(d, hf.counts, 16);
            memcpy(d + WITW_JPEG_PLAN_TABLE_SYMS, hf.sym, (size_t)hf.nsym);
        }
    }
    uint32_t* off = reinterpret_cast<uint32_t*>(plan + WITW_JPEG_PLAN_FIXED);
    const uint8_t* q = P.scan;
    const uint8_t* e = data + n;
    long long found = 0;
    off[0] = (uint32_t)(P.scan - data);
    int next_rst = 0;
    const uint8_t* end = e;
    while (q < e) {
        const uint8_t* f = (const uint8_t*)memchr(q, 0xFF, (size_t)(e - q));
        if (!f || f + 1 >= e) break;
        const int m = f[1];
        if (m == 0) { q = f + 2; continue; }                           // a stuffed FF
        if (m == 0xFF) { q = f + 1; continue; }                        // fill byte
        if (m >= 0xD0 && m <= 0xD7) {
            if (m - 0xD0 != next_rst || found + 1 >= n_int) return -3;
            next_rst = (next_rst + 1) & 7;
            off[++found] = (uint32_t)(f + 2 - data);
            q = f + 2;
            continue;
        }
        end = f;                                                       // EOI or another marker: the entropy-coded data ends here
        break;
    }
    if (found != n_int - 1) return -3;
    h[WITW_JPEG_PLAN_DATA_END] = (int32_t)(end - data);
    return need;
}

long long witw_jpeg_entropy_plan(const uint8_t* data, size_t n, uint8_t* plan, size_t plan_cap, uint16_t* qt) {
    return witw_jpeg_entropy_plan_ex(data, n, plan, plan_cap, qt, 0);
}

// ---- the scans of a PROGRESSIVE file on the device (csrc/jpeg_progressive.hip: one launch per stage, a workgroup per scan, a thread
// per restart interval of it). The scan plan ('JPW2', csrc/jpeg_layout.h) is to such a file what the entropy plan is to a sequential
// one; the entropy-plan entries above keep refusing progressive files. flags: bit 1 as above; bit 0 is implied.

// the size of the file's scan plan in bytes; 0: no plan (not a progressive file this decoder takes, or one witw_jpeg_scan_plan_ex refuses)
long long witw_jpeg_scan_plan_bytes_ex(const uint8_t* data, size_t n, int flags) {
    Parsed& P = parsed();
    if (parse(data, n, P, true, (flags & WITW_JPEG_ACCEPT_H1V2) != 0) || !P.progressive) return 0;
    const long long need = scan_plan(P, data, n, nullptr, 0, nullptr);
    return need > 0 ? need : 0;
}

// plan: plan_cap bytes (witw_jpeg_scan_plan_bytes_ex), 4-byte aligned; qt: ncomp x 64 uint16 (as witw_jpeg_decode_coef_ex writes them).
// Returns the plan's size in bytes, or -1 / -2 as witw_jpeg_info_ex (-1 also: plan_cap too small; -2 also: a sequential file, a file
// of more than 64 scans, a DC table of more than 16 symbols, scans that stop short of bit 0 -- witw_jpeg_decode_coef_ex's -2), -3 when a
// segment length, a scan's Ss / Se / Ah / Al, the order of the scans, a missing table, the restart markers of a scan (RSTn out of
// sequence, or not one per interval) or a missing EOI is what witw_jpeg_decode_coef_ex refuses with -3. A file without a plan takes
// the host route. Every check that needs no Huffman decoding is made here; what shows only in the entropy-coded bits is the device's
// to flag.
long long witw_jpeg_scan_plan_ex(const uint8_t* data, size_t n, uint8_t* plan, size_t plan_cap, uint16_t* qt, int flags) {
    Parsed& P = parsed();
    const int rc = parse(data, n, P, true, (flags & WITW_JPEG_ACCEPT_H1V2) != 0);
    if (rc) return rc;
    if (!P.progressive || !plan || !qt) return -2;
    return scan_plan(P, data, n, plan, plan_cap, qt);
}

}  // extern "C"
