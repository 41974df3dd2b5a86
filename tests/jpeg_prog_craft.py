"""Test-only PROGRESSIVE JPEG writer (pure Python + numpy; beside tests/jpeg_craft.py, whose bit writer, tables and geometry it uses):
coefficient blocks in the layout jpeg.read_coef(...).coef returns, written under a scan script the test chooses -- Pillow only ever
writes libjpeg's default script. The coding procedures are T.81 annex G (G.1.2.1 DC, G.1.2.2 AC first, G.1.2.3 AC refinement), in the
order libjpeg's encoder (jcphuff.c) emits them; every scan gets Huffman tables made for it, defined in front of its SOS.

A script is a list of scans; a scan is a dict:
  comps   component indices of the scan (several: an interleaved DC scan)
  ss, se  spectral band (zig-zag positions), 0, 0 for a DC scan
  ah, al  successive approximation: ah = 0 a first scan down to bit al, else the refinement from bit ah to al = ah - 1
  slots   Huffman table slot (0..3) per scan component, default 0 for component 0 and 1 for the others
  dri     restart interval in MCUs, written as a DRI segment in front of the scan when it differs from the one in force (default 0)
  min_len lengthen every Huffman code of the scan to at least this many bits (the decoders' slow path: codes past the look-ahead)"""
import heapq

import numpy as np

from .jpeg_craft import SAMPLINGS, ZZ, _BitWriter, _codes, category, geometry, table_from_lengths, value_bits


def scan(comps, ss, se, ah, al, **kw):
    return dict(comps=tuple(comps), ss=ss, se=se, ah=ah, al=al, **kw)


def script_spectral(ncomp, bands=((1, 5), (6, 63))):
    """spectral selection only: DC of all components interleaved, then the AC bands of each component"""
    return [scan(range(ncomp), 0, 0, 0, 0)] + [scan([c], a, b, 0, 0) for (a, b) in bands for c in range(ncomp)]


def script_successive(ncomp, al=3, bands=((1, 63),)):
    """successive approximation: everything first down to bit `al`, then one refinement scan per bit; DC refinements interleaved"""
    s = [scan(range(ncomp), 0, 0, 0, al)] + [scan([c], a, b, 0, al) for (a, b) in bands for c in range(ncomp)]
    for bit in range(al, 0, -1):
        s += [scan([c], a, b, bit, bit - 1) for (a, b) in bands for c in range(ncomp)]
        s.append(scan(range(ncomp), 0, 0, bit, bit - 1))
    return s


def script_dc_separate(ncomp):
    """DC not interleaved: one DC scan (and one DC refinement) per component"""
    return [scan([c], 0, 0, 0, 1) for c in range(ncomp)] + [scan([c], 1, 63, 0, 0) for c in range(ncomp)] + \
        [scan([c], 0, 0, 1, 0) for c in range(ncomp)]


def block_rows(H, W, sampling, comps):
    """rows of the coefficient array of the blocks a scan of `comps` visits, in scan order, one list per MCU: several components
    walk the MCUs of the frame, ONE component walks its own ceil(w / 8) x ceil(h / 8) blocks (T.81 A.2.2, A.2.3)"""
    geo, _n, mx, my = geometry(H, W, sampling)
    hmax, vmax = max(g[0] for g in geo), max(g[1] for g in geo)
    offs = np.cumsum([0] + [bw * bh for _h, _v, bw, bh in geo])
    if len(comps) == 1:
        h, v, bw, _bh = geo[comps[0]]
        cols, rows = -(-(-(-W * h // hmax)) // 8), -(-(-(-H * v // vmax)) // 8)
        return [[(comps[0], int(offs[comps[0]] + r * bw + c))] for r in range(rows) for c in range(cols)]
    out = []
    for m in range(mx * my):
        mrow, mcol = divmod(m, mx)
        out.append([(c, int(offs[c] + (mrow * geo[c][1] + vv) * geo[c][2] + mcol * geo[c][0] + hh))
                    for c in comps for vv in range(geo[c][1]) for hh in range(geo[c][0])])
    return out


def padding_blocks(H, W, sampling):
    """bool [blocks]: blocks of the coefficient area that exist only as MCU padding (no single-component scan ever visits them)"""
    geo, n, _mx, _my = geometry(H, W, sampling)
    seen = np.zeros(n, dtype=bool)
    for c in range(len(geo)):
        for mcu in block_rows(H, W, sampling, (c,)):
            seen[mcu[0][1]] = True
    return ~seen


def huffman_table(freq, min_len=0):
    """{symbol: count} -> (counts[16], symbols): Huffman code lengths with one code point reserved (a pseudo-symbol of weight 0 takes
    the all-ones code, as libjpeg does it: T.81 forbids that code), lengthened to at least min_len bits on request"""
    syms = sorted(freq)
    heap = [(freq[s], i, (s,)) for i, s in enumerate(syms)] + [(0, -1, (None,))]
    depth = {s: 0 for s in syms + [None]}
    heapq.heapify(heap)
    tick = len(syms)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
        tick += 1
    assert max(depth.values()) <= 16, 'code longer than 16 bits: the test image is too large for this simple table builder'
    order = sorted(syms, key=lambda s: (depth[s], -freq[s]))      # the reserved point has the greatest depth: the last code stays unused
    return table_from_lengths(order, [max(depth[s], min_len) for s in order])


class _ScanCoder(object):
    """Codes the blocks of one scan into a list of items -- ('dc' | 'ac', slot, symbol), ('bits', value, count), ('rst', n) -- so that
    the symbol statistics are known before any bit is written (tables are made per scan)."""

    def __init__(self, sc, slots):
        self.sc, self.slots, self.items = sc, slots, []
        self.eobrun, self.pending = 0, []      # blocks of the running EOB run; their correction bits (refinement scans)

    def sym(self, kind, comp, s):
        self.items.append((kind, self.slots[comp], s))

    def bits(self, v, n):
        if n:
            self.items.append(('bits', int(v), int(n)))

    def flush_eobrun(self, comp):
        if self.eobrun:
            r = self.eobrun.bit_length() - 1
            self.sym('ac', comp, r << 4)
            self.bits(self.eobrun & ((1 << r) - 1), r)
            self.eobrun = 0
        for b in self.pending:
            self.bits(b, 1)
        self.pending = []

    def end_block_in_eobrun(self, comp, corr):
        self.eobrun += 1
        self.pending += corr
        if self.eobrun == 0x7fff:
            self.flush_eobrun(comp)

    def dc_first(self, comp, v, pred):
        v = int(v) >> self.sc['al']                      # the point transform of DC is an arithmetic shift (G.1.2.1)
        d = v - pred[comp]
        pred[comp] = v
        s = category(d)
        self.sym('dc', comp, s)
        self.bits(value_bits(d, s), s)

    def ac_first(self, comp, z):
        sc, r = self.sc, 0
        for k in range(sc['ss'], sc['se'] + 1):
            v = int(z[k])
            t = abs(v) >> sc['al']                       # AC: division towards zero
            if t == 0:
                r += 1
                continue
            self.flush_eobrun(comp)
            while r > 15:
                self.sym('ac', comp, 0xf0)
                r -= 16
            s = t.bit_length()
            self.sym('ac', comp, (r << 4) | s)
            self.bits(value_bits(t if v > 0 else -t, s), s)
            r = 0
        if r:
            self.end_block_in_eobrun(comp, [])

    def ac_refine(self, comp, z):
        sc = self.sc
        t = [abs(int(z[k])) >> sc['al'] for k in range(64)]
        last_new = max([k for k in range(sc['ss'], sc['se'] + 1) if t[k] == 1], default=-1)
        r, corr = 0, []                                  # zero-history run; correction bits passed since the last symbol
        for k in range(sc['ss'], sc['se'] + 1):
            if t[k] == 0:
                r += 1
                continue
            while r > 15 and k <= last_new:              # a ZRL only where a new coefficient follows; else the zeros fold into the EOB
                self.flush_eobrun(comp)
                self.sym('ac', comp, 0xf0)
                r -= 16
                for b in corr:
                    self.bits(b, 1)
                corr = []
            if t[k] > 1:                                 # non-zero before this scan: its next bit
                corr.append(t[k] & 1)
                continue
            self.flush_eobrun(comp)
            self.sym('ac', comp, (r << 4) | 1)
            self.bits(0 if z[k] < 0 else 1, 1)
            for b in corr:
                self.bits(b, 1)
            r, corr = 0, []
        if r or corr:
            self.end_block_in_eobrun(comp, corr)


def write(H, W, coef, qt, sampling, script, n_scans=None):
    """-> the bytes of a progressive JPEG: SOI, APP0 JFIF, DQT, SOF2, then per scan [DRI] DHT SOS and its entropy-coded data, EOI.
    coef: int16 [blocks, 64] (read_coef's layout); qt: uint16 [components, 64] natural order; n_scans: write only the first so many
    scans of the script (an INCOMPLETE file)."""
    geo, nblk, mx, my = geometry(H, W, sampling)
    ncomp = len(geo)
    coef = np.asarray(coef)
    qt = np.asarray(qt, dtype=np.int64).reshape(ncomp, 64)
    assert coef.shape == (nblk, 64), (coef.shape, nblk)
    zz = coef[:, ZZ].astype(np.int64)

    def seg(marker, body):
        return bytes([0xff, marker, (len(body) + 2) >> 8, (len(body) + 2) & 0xff]) + bytes(body)

    out = bytearray(b'\xff\xd8')
    out += seg(0xe0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for c in range(ncomp):
        q = qt[c][ZZ]
        assert q.min() >= 1 and q.max() <= 255
        out += seg(0xdb, bytes([c]) + bytes(int(x) for x in q))
    sof = bytearray([8, H >> 8, H & 0xff, W >> 8, W & 0xff, ncomp])
    for c, (h, v) in enumerate(SAMPLINGS[sampling]):
        sof += bytes([c + 1, (h << 4) | v, c])
    out += seg(0xc2, sof)
    dri_now = 0
    for sc in script[:n_scans]:
        comps = sc['comps']
        slots = dict(zip(comps, sc.get('slots', [0 if c == 0 else 1 for c in comps])))
        dri = sc.get('dri', 0)
        coder = _ScanCoder(sc, slots)
        pred = {c: 0 for c in comps}
        empty = ~zz[:, sc['ss']:sc['se'] + 1].any(axis=1)      # (large all-zero images: such a block only lengthens the EOB run)
        for m, mcu in enumerate(block_rows(H, W, sampling, comps)):
            if dri and m and m % dri == 0:
                coder.flush_eobrun(comps[0])
                coder.items.append(('rst', (m // dri - 1) & 7))
                pred = {c: 0 for c in comps}
            for c, row in mcu:
                if sc['ss'] == 0 and sc['ah'] == 0:
                    coder.dc_first(c, coef[row, 0], pred)
                elif sc['ss'] == 0:
                    coder.bits((int(coef[row, 0]) >> sc['al']) & 1, 1)
                elif empty[row]:
                    coder.end_block_in_eobrun(c, [])
                elif sc['ah'] == 0:
                    coder.ac_first(c, zz[row])
                else:
                    coder.ac_refine(c, zz[row])
        coder.flush_eobrun(comps[0])
        if dri != dri_now:
            out += seg(0xdd, bytes([dri >> 8, dri & 0xff]))
            dri_now = dri
        codes = {}
        for kind, tc in (('dc', 0), ('ac', 1)):
            for slot in sorted(set(it[1] for it in coder.items if it[0] == kind)):
                freq = {}
                for it in coder.items:
                    if it[0] == kind and it[1] == slot:
                        freq[it[2]] = freq.get(it[2], 0) + 1
                counts, symbols = huffman_table(freq, sc.get('min_len', 0))
                out += seg(0xc4, bytes([(tc << 4) | slot]) + bytes(counts) + bytes(symbols))
                codes[kind, slot] = _codes((counts, symbols))
        sos = bytearray([len(comps)])
        for c in comps:
            sos += bytes([c + 1, (slots[c] << 4) | slots[c]])
        out += seg(0xda, sos + bytes([sc['ss'], sc['se'], (sc['ah'] << 4) | sc['al']]))
        bw = _BitWriter()
        for it in coder.items:
            if it[0] == 'bits':
                bw.put(it[1], it[2])
            elif it[0] == 'rst':
                bw.pad()
                bw.out += bytes([0xff, 0xd0 + it[1]])
            else:
                bw.put(*codes[it[0], it[1]][it[2]])
        bw.pad()
        out += bw.out
    return bytes(out) + b'\xff\xd9'


def scans_of(data):
    """the scans of a progressive file (ours or Pillow's) as script entries, each with 'start' / 'end': the byte span of its
    entropy-coded data (the three bytes in front of 'start' are Ss, Se, Ah << 4 | Al)"""
    ids, scans, i = [], [], 2
    while data[i + 1] != 0xd9:
        ln = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == 0xc2:
            ids = [data[i + 10 + 3 * c] for c in range(data[i + 9])]
        if data[i + 1] == 0xda:
            ns, j = data[i + 4], i + 2 + ln
            k = j
            while not (data[k] == 0xff and data[k + 1] != 0 and not 0xd0 <= data[k + 1] <= 0xd7):
                k += 1
            scans.append(scan([ids.index(data[i + 5 + 2 * c]) for c in range(ns)], data[j - 3], data[j - 2], data[j - 1] >> 4,
                              data[j - 1] & 15, start=j, end=k))
            i = k
        else:
            i += 2 + ln
    return scans


def drop_last_scan(data):
    """the file without its last scan (tables in front of it included): SOI .. the end of the scan before, EOI"""
    return data[:scans_of(data)[-2]['end']] + b'\xff\xd9'
