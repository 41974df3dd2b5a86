"""Test-only baseline JPEG writer (pure Python + numpy): a file whose entropy-coded data says exactly what the test chose, down to
streams Pillow's encoder never produces -- DC / AC magnitude categories 12-15, 16-bit codes, blocks that end at coefficient 63 or on
a ZRL chain without EOB, fill bytes in front of RSTn / EOI -- and, through injection hooks, damaged ones.

Coefficients come in the layout jpeg.read_coef(...).coef returns: int16 [blocks, 64], natural order, the components one after another
(component c: its MCU-padded block grid, raster order), DC as an absolute value. The written coefficients are then an exact reference
for the entropy stage of any decoder (ITU-T T.81: F.1.2 for the coding, B.2 for the markers)."""
import io

import numpy as np

ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

SAMPLINGS = {          # name -> (h, v) per component as the SOF declares them
    'grey': [(1, 1)],
    'grey22': [(2, 2)],          # a single-component scan is never interleaved: one block per MCU whatever the SOF says (T.81 A.2.2)
    '444': [(1, 1), (1, 1), (1, 1)],
    '422': [(2, 1), (1, 1), (1, 1)],
    '420': [(2, 2), (1, 1), (1, 1)],
}

_STD = None


def standard_tables():
    """The Annex K tables (K.3) as Pillow's encoder writes them without optimisation: {'dc': [lum, chroma], 'ac': [lum, chroma]}, each
    (counts[16], symbols)."""
    global _STD
    if _STD is None:
        from PIL import Image
        bio = io.BytesIO()
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(bio, 'JPEG', quality=75, subsampling=0, optimize=False)
        d = bio.getvalue()
        tabs = {}
        i = 2
        while d[i + 1] != 0xda:
            ln = (d[i + 2] << 8) | d[i + 3]
            if d[i + 1] == 0xc4:
                s, k = d[i + 4:i + 2 + ln], 0
                while k < len(s):
                    counts = list(s[k + 1:k + 17])
                    tabs[s[k]] = (counts, list(s[k + 17:k + 17 + sum(counts)]))
                    k += 17 + sum(counts)
            i += 2 + ln
        _STD = {'dc': [tabs[0x00], tabs[0x01]], 'ac': [tabs[0x10], tabs[0x11]]}
    return _STD


def table_from_lengths(symbols, lengths):
    """Canonical table (counts, symbols) giving symbols[i] a code of lengths[i] bits (1..16); the code space must not be full (the
    all-ones code stays unused, T.81 C)."""
    order = sorted(range(len(symbols)), key=lambda i: lengths[i])
    counts = [0] * 16
    for i in order:
        counts[lengths[i] - 1] += 1
    assert sum(c * 2.0 ** -(L + 1) for L, c in enumerate(counts)) < 1.0, 'code space over-full'
    return counts, [symbols[i] for i in order]


def long_code_tables():
    """Tables with every magnitude category 0..15 and codes of up to 16 bits: DC categories 12-15 and the AC symbols of sizes 11-15
    get the longest codes, some of them 16 bits. {'dc': [t, t], 'ac': [t, t]}."""
    dc_sym = list(range(16))
    dc_len = [2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 12, 14, 16, 16]
    dc = table_from_lengths(dc_sym, dc_len)
    ac_sym = [0x00, 0xf0] + [(r << 4) | s for r in range(16) for s in range(1, 16)]
    ac_len = []
    for rs in ac_sym:
        r, s = rs >> 4, rs & 15
        ac_len.append(2 if rs == 0 else 9 if rs == 0xf0 else (16 if s >= 13 or r >= 13 else 14 if s >= 11 else 4 + min(s + r // 2, 8)))
    ac = table_from_lengths(ac_sym, ac_len)
    return {'dc': [dc, dc], 'ac': [ac, ac]}


def _codes(table):
    counts, symbols = table
    codes, code, k = {}, 0, 0
    for L in range(1, 17):
        for _ in range(counts[L - 1]):
            codes[symbols[k]] = (code, L)
            code += 1
            k += 1
        code <<= 1
    return codes


def geometry(H, W, sampling):
    """-> [(h, v, bw, bh)] per component as the decoders see them (read_coef's info), blocks in all, MCUs wide, MCUs high"""
    hv = SAMPLINGS[sampling]
    if len(hv) == 1:
        hv = [(1, 1)]
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    comps = [(h, v, mx * h, my * v) for h, v in hv]
    return comps, sum(bw * bh for _h, _v, bw, bh in comps), mx, my


def scan_rows(H, W, sampling):
    """row of the coefficient array (read_coef's layout) of every block in scan order (the block numbers of write(inject=...))"""
    comps, _nblk, mx, my = geometry(H, W, sampling)
    offs = np.cumsum([0] + [bw * bh for _h, _v, bw, bh in comps])
    rows = []
    for m in range(mx * my):
        mrow, mcol = divmod(m, mx)
        for c, (h, v, bw, _bh) in enumerate(comps):
            for vv in range(v):
                for hh in range(h):
                    rows.append(offs[c] + (mrow * v + vv) * bw + mcol * h + hh)
    return np.array(rows, dtype=np.int64)


def category(v):
    return int(abs(int(v))).bit_length()


def value_bits(v, s):
    """the s magnitude bits of v (T.81 F.1.2.1: negative values as v - 1 in s bits)"""
    return int(v) if v >= 0 else (int(v) - 1) & ((1 << s) - 1)


def ac(run, size, value):
    """an injection item: the AC symbol (run, size) with `value` in its magnitude bits -- also a run that goes past coefficient 63"""
    return ('sym', 'ac', (run << 4) | size, size, value_bits(value, size) if size else 0)


def dc(cat, bits=0):
    """an injection item: the DC symbol of category `cat` followed by `cat` raw bits"""
    return ('sym', 'dc', cat, cat, bits)


def raw_bits(s):
    """an injection item: the bits of the string s ('0' / '1'), stuffed like any other data"""
    return ('bits', s)


class _BitWriter(object):
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        if n == 0:
            return
        self.acc = (self.acc << n) | (int(v) & ((1 << n) - 1))
        self.n += n
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 0xff
            self.out.append(b)
            if b == 0xff:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def pad(self):      # to a byte boundary with 1-bits (T.81 F.1.2.3)
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def write(H, W, coef, qt, sampling='420', tables=None, dri=0, fill_rst=0, fill_eoi=0, inject=None, truncate=None, eoi=True):
    """-> the bytes of a baseline JPEG: SOI, APP0 JFIF, DQT, SOF0, DHT, [DRI], SOS, the entropy-coded data, [EOI].
    coef: int16 [blocks, 64] (read_coef's layout); qt: uint16 [components, 64] natural order (one table per component);
    tables: {'dc': [slot 0, slot 1], 'ac': [...]} of (counts, symbols), default the Annex K tables (component 0 slot 0, the others 1);
    dri: MCUs per restart interval (0: no restart markers); fill_rst / fill_eoi: FF fill bytes in front of every RSTn / the EOI;
    inject: {block number in scan order: {'pre': [items], 'post': [items], 'eob': bool}} -- items emitted in front of the block's DC
    symbol / behind its last coefficient, 'eob': False drops the block's EOB (dc(), ac(), raw_bits());
    truncate: keep this many bytes of the entropy-coded data; eoi: False drops the EOI marker."""
    comps, nblk, mx, my = geometry(H, W, sampling)
    ncomp = len(comps)
    coef = np.asarray(coef)
    qt = np.asarray(qt, dtype=np.int64).reshape(ncomp, 64)
    assert coef.shape == (nblk, 64), (coef.shape, nblk)
    tables = tables or standard_tables()
    slot = [0] + [1] * (ncomp - 1)
    dcc = [_codes(t) for t in tables['dc']]
    acc = [_codes(t) for t in tables['ac']]
    inject = inject or {}

    def seg(marker, body):
        return bytes([0xff, marker, (len(body) + 2) >> 8, (len(body) + 2) & 0xff]) + bytes(body)

    out = bytearray(b'\xff\xd8')
    out += seg(0xe0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for c in range(ncomp):
        q = qt[c][ZZ]
        assert q.min() >= 1 and q.max() <= 65535
        out += seg(0xdb, bytes([c]) + bytes(int(x) for x in q)) if q.max() <= 255 else \
            seg(0xdb, bytes([0x10 | c]) + b''.join(int(x).to_bytes(2, 'big') for x in q))
    sof = bytearray([8, H >> 8, H & 0xff, W >> 8, W & 0xff, ncomp])
    for c, (h, v) in enumerate(SAMPLINGS[sampling]):
        sof += bytes([c + 1, (h << 4) | v, c])
    out += seg(0xc0, sof)
    for kind, tc in (('dc', 0), ('ac', 1)):
        for s in range(2 if ncomp > 1 else 1):
            counts, symbols = tables[kind][s]
            out += seg(0xc4, bytes([(tc << 4) | s]) + bytes(counts) + bytes(symbols))
    if dri:
        out += seg(0xdd, bytes([dri >> 8, dri & 0xff]))
    sos = bytearray([ncomp])
    for c in range(ncomp):
        sos += bytes([c + 1, (slot[c] << 4) | slot[c]])
    out += seg(0xda, sos + bytes([0, 63, 0]))

    rows = scan_rows(H, W, sampling)
    bwr = _BitWriter()
    pred = [0] * ncomp
    b = 0
    n_mcu = mx * my

    def emit(items, c):
        for it in items:
            if it[0] == 'bits':
                for ch in it[1]:
                    bwr.put(int(ch), 1)
            else:
                _t, kind, sym, nbits, bits = it
                code, L = (dcc if kind == 'dc' else acc)[slot[c]][sym]
                bwr.put(code, L)
                bwr.put(bits, nbits)

    for m in range(n_mcu):
        if dri and m and m % dri == 0:
            bwr.pad()
            n_rst = (m // dri - 1) & 7
            bwr.out += b'\xff' * fill_rst + bytes([0xff, 0xd0 + n_rst])
            pred = [0] * ncomp
        for c, (h, v, _bw, _bh) in enumerate(comps):
            for _k in range(h * v):
                    blk = coef[rows[b]]
                    inj = inject.get(b, {})
                    emit(inj.get('pre', []), c)
                    z = blk[ZZ].astype(np.int64)
                    diff = int(z[0]) - pred[c]
                    pred[c] = int(z[0])
                    s = category(diff)
                    assert s <= 15, 'DC difference %d needs category %d' % (diff, s)
                    code, L = dcc[slot[c]][s]
                    bwr.put(code, L)
                    bwr.put(value_bits(diff, s), s)
                    nz = np.nonzero(z[1:])[0] + 1
                    k = 1
                    for at in nz:
                        run = int(at) - k
                        while run > 15:
                            code, L = acc[slot[c]][0xf0]
                            bwr.put(code, L)
                            run -= 16
                        vv_ = int(z[at])
                        s = category(vv_)
                        assert 1 <= s <= 15, 'AC value %d' % vv_
                        code, L = acc[slot[c]][(run << 4) | s]
                        bwr.put(code, L)
                        bwr.put(value_bits(vv_, s), s)
                        k = int(at) + 1
                    emit(inj.get('post', []), c)
                    if k < 64 and inj.get('eob', True):
                        code, L = acc[slot[c]][0x00]
                        bwr.put(code, L)
                    b += 1
    bwr.pad()
    data = bytes(bwr.out)
    if truncate is not None:
        data = data[:truncate]
    out += data
    if eoi:
        out += b'\xff' * fill_eoi + b'\xff\xd9'
    return bytes(out)


def scan_start(data):
    """byte offset of the first entropy-coded byte (behind the SOS segment)"""
    sos = data.find(b'\xff\xda')
    return sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])


def random_coef(g, H, W, sampling, density=0.15, amp=40, dc_amp=200, last=None):
    """Coefficients of an image: DC in [-dc_amp, dc_amp], a fraction `density` of the AC positions non-zero in [-amp, amp] (never
    0), AC position 63 non-zero in every block when last=True."""
    _comps, nblk, _mx, _my = geometry(H, W, sampling)
    c = np.zeros((nblk, 64), dtype=np.int16)
    c[:, 0] = g.integers(-dc_amp, dc_amp + 1, size=nblk)
    m = g.random((nblk, 63)) < density
    v = g.integers(1, amp + 1, size=(nblk, 63)) * np.where(g.random((nblk, 63)) < 0.5, -1, 1)
    c[:, 1:] = np.where(m, v, 0)
    if last:
        c[:, 63] = g.integers(1, amp + 1, size=nblk)
    return c


def flat_qt(ncomp, q=1):
    return np.full((ncomp, 64), q, dtype=np.uint16)


# Pixels are compared with Pillow only where the dequantised coefficients stay in an encoder's range: |c q| <= 2047 for every
# coefficient and sum |c q| <= 8192 over a block. Beyond it libjpeg-turbo's SIMD inverse DCT (16-bit lanes) and the C form
# (oracle/jpeg_oracle.py, csrc/jpeg.hip) may wrap differently; there the coefficients are compared only.
DEQUANT_BOUND, BLOCK_BOUND = 2047, 8192


def in_range(info, coef, qt):
    off = 0
    for c in range(int(info[2])):
        n = int(info[8 + 4 * c]) * int(info[9 + 4 * c])
        d = np.abs(coef[off:off + n].astype(np.int64) * qt[c].astype(np.int64))
        off += n
        if d.size and (d.max() > DEQUANT_BOUND or d.sum(axis=1).max() > BLOCK_BOUND):
            return False
    return True


def pillow(data):
    """Pillow's image of the file (what the reference's imread returns): uint8 HWC (grey: HW)"""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


# ---- the corpora of tests/test_jpeg_craft.py and tests/test_jpeg_damage_gpu.py

HUFF_STAGE = 10 * 1024      # csrc/jpeg.hip: LDS bytes per wave of 64 restart intervals (jpeg_huffman_kernel stages them when they fit)


def _dense(g, nblk, frac=0.9, v=1023):
    """blocks whose symbols are long runs of 1-bits (large positive values, the longest codes): FF bytes, stuffed, at every offset"""
    c = np.zeros((nblk, 64), dtype=np.int16)
    c[:, 0] = 1023
    c[:, 1:] = np.where(g.random((nblk, 63)) < frac, v, 0)
    return c


def valid_corpus(seed=3):
    """[(name, file bytes, written coefficients)]: every sampling x table set x DRI setting, and the edges the decoders' fast paths
    have: categories 12-15 and 16-bit codes, blocks ending at coefficient 63 or on a ZRL chain that lands on 64 (no EOB), FF fill
    bytes in front of RSTn / EOI, FF 00 straddling 8-byte words, a grey file declaring 2x2, > 16,384 restart intervals, waves on both
    sides of the LDS-staging limit, 96 and 97 blocks."""
    g = np.random.Generator(np.random.Philox(key=[seed, 90]))
    out = []
    for sampling in SAMPLINGS:
        ncomp = len(SAMPLINGS[sampling])
        for tname in ('std', 'long'):
            tabs = long_code_tables() if tname == 'long' else None
            for dri in (0, 3):
                for (H, W) in ((61, 43), (120, 136)):
                    if tname == 'long':          # categories 12-15 (DC differences stay within 15)
                        c = random_coef(g, H, W, sampling, density=0.2, amp=32767, dc_amp=16000)
                    else:
                        c = random_coef(g, H, W, sampling, density=0.2, amp=60, dc_amp=120)
                    qt = g.integers(1, 9, size=(ncomp, 64)).astype(np.uint16)
                    out.append(('%s_%s_dri%d_%dx%d' % (sampling, tname, dri, H, W),
                                write(H, W, c, qt, sampling, tables=tabs, dri=dri), c))
    # blocks that end at coefficient 63 (no EOB); ZRL chains that land on 64 (no EOB); fill bytes in front of RSTn and EOI
    for sampling, dri in (('420', 0), ('444', 2), ('grey', 0), ('grey', 5)):
        H, W = 104, 120
        ncomp = len(SAMPLINGS[sampling])
        c = random_coef(g, H, W, sampling, density=0.1, amp=20, dc_amp=100, last=True)
        inj, rows = {}, scan_rows(H, W, sampling)
        for b in range(1, c.shape[0], 3):            # every third block: coefficients up to zig-zag 15, then 3 ZRL = 64
            c[rows[b], ZZ[16:]] = 0
            c[rows[b], ZZ[15]] = 7
            inj[b] = {'post': [ac(15, 0, 0)] * 3, 'eob': False}
        out.append(('ends63_zrl64_fill_%s_dri%d' % (sampling, dri),
                    write(H, W, c, flat_qt(ncomp, 2), sampling, dri=dri, fill_rst=2, fill_eoi=3, inject=inj), c))
    # stuffing everywhere (long runs of 1-bits): self-sync sized, no DRI, and with DRI
    for dri in (0, 4):
        c = _dense(g, 300)
        out.append(('stuffed_grey_dri%d' % dri, write(8 * 15, 8 * 20, c, flat_qt(1, 1), 'grey', dri=dri, fill_eoi=1), c))
    # waves of 64 one-block intervals on both sides of the LDS staging limit (rows of 64 blocks: one wave each)
    rows = [_dense(g, 64, 0.95), random_coef(g, 8, 512, 'grey', density=0.05, amp=10), _dense(g, 64, 0.55), _dense(g, 64, 0.95)]
    c = np.concatenate(rows)
    out.append(('staging_grey_dri1', write(32, 512, c, flat_qt(1, 1), 'grey', dri=1), c))
    # more than 16,384 restart intervals (the second pass of jpeg_huffman_kernel's interval loop)
    c = random_coef(g, 1040, 1040, 'grey', density=0.01, amp=8, dc_amp=50)
    out.append(('many_intervals_grey_dri1', write(1040, 1040, c, flat_qt(1, 3), 'grey', dri=1), c))
    # 96 / 97 blocks without markers (either side of jpeg.SELFSYNC_MIN_BLOCKS), 96 in 4:2:0
    for (H, W, s) in ((8, 768, 'grey'), (8, 776, 'grey'), (64, 64, '420'), (16, 8 * 97, 'grey22')):
        c = random_coef(g, H, W, s, density=0.3, amp=50, dc_amp=300)
        out.append(('blocks_%s_%dx%d' % (s, H, W), write(H, W, c, flat_qt(len(SAMPLINGS[s]), 4), s), c))
    return out


def staging_sides(data):
    """(waves staged, waves not staged) of jpeg_huffman_kernel on this file: from its entropy plan, as the kernel decides"""
    from witw_amd import jpeg
    plan, _qt = jpeg.open_file(data).entropy_plan()
    hdr = plan[:128].view(np.int32)
    n_int, end = int(hdr[1]), min(int(hdr[27]), len(data))
    ioff = np.minimum(plan[736:736 + 4 * n_int].view(np.uint32).astype(np.int64), len(data))
    staged = unstaged = 0
    for iv0 in range(0, n_int, 64):
        r0 = int(ioff[iv0]) & ~7
        r1 = int(ioff[iv0 + 64]) if iv0 + 64 < n_int else end
        if r1 > r0 and r1 - r0 + 24 <= HUFF_STAGE:
            staged += 1
        else:
            unstaged += 1
    return staged, unstaged


def damage_corpus(seed=4):
    """[(name, file bytes)]: deterministic damage -- a run past coefficient 63 as a block's last symbol with no EOB (in a self-sync
    sized file, in an interval of a DRI file, in a file of <= 96 blocks), an invalid code (16 one-bits: FF 00 FF 00), a truncated
    scan, a truncated scan without EOI, a DC category of 16 -- and seeded random overwrites of entropy-coded bytes that keep markers
    and stuffing intact, of Pillow-written and of crafted files."""
    g = np.random.Generator(np.random.Philox(key=[seed, 91]))
    out = []
    shapes = (('selfsync', 120, 136, 0), ('dri', 120, 136, 2), ('small', 40, 48, 0))
    for kind, H, W, dri in shapes:
        for sampling in ('grey', '420'):
            ncomp = len(SAMPLINGS[sampling])
            c = random_coef(g, H, W, sampling, density=0.1, amp=30, dc_amp=100)
            qt = flat_qt(ncomp, 2)
            qt[:, 63] = 16
            nb = c.shape[0]
            for b in (nb // 2, nb - 1):
                cc = c.copy()
                cc[scan_rows(H, W, sampling)[b], 1:] = 0
                cc[scan_rows(H, W, sampling)[b], ZZ[60]] = 3                  # the block's last coefficient at zig-zag 60, then a run of 15: lands on 76
                out.append(('run63_%s_%s_b%d' % (kind, sampling, b),
                            write(H, W, cc, qt, sampling, dri=dri, inject={b: {'post': [ac(15, 7, 120)], 'eob': False}})))
            b = nb // 3
            out.append(('inval_%s_%s' % (kind, sampling), write(H, W, c, qt, sampling, dri=dri, inject={b: {'pre': [raw_bits('1' * 16)]}})))
            full = write(H, W, c, qt, sampling, dri=dri)
            n_ent = len(full) - scan_start(full) - 2
            out.append(('trunc_%s_%s' % (kind, sampling), write(H, W, c, qt, sampling, dri=dri, truncate=n_ent * 2 // 3)))
            out.append(('trunc_noeoi_%s_%s' % (kind, sampling), write(H, W, c, qt, sampling, dri=dri, truncate=n_ent - 5, eoi=False)))
    # DC category 16: a DC table of 16 symbols (the device plan holds 16) with 16 in place of 15
    tb = table_from_lengths(list(range(15)) + [16], [2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 12, 14, 16, 16])
    tabs = {'dc': [tb, tb], 'ac': long_code_tables()['ac']}
    for kind, H, W, dri in shapes:
        c = random_coef(g, H, W, 'grey', density=0.1, amp=30, dc_amp=100)
        out.append(('dc16_%s' % kind, write(H, W, c, flat_qt(1, 2), 'grey', tables=tabs, dri=dri, inject={c.shape[0] // 2: {'pre': [dc(16, 5)]}})))
    # random overwrites
    from PIL import Image
    for i in range(48):
        H, W = int(g.integers(40, 260)), int(g.integers(40, 260))
        if i % 3 == 2:
            s = ('grey', '444', '422', '420')[i % 4]
            raw = write(H, W, random_coef(g, H, W, s, density=0.15, amp=40, dc_amp=150),
                        flat_qt(len(SAMPLINGS[s]), int(g.integers(1, 6))), s, dri=int(g.integers(0, 4)) * (i % 2))
        else:
            a = g.integers(0, 256, size=(H // 8 + 2, W // 8 + 2, 3), dtype=np.uint8)
            a = np.asarray(Image.fromarray(a).resize((W, H), Image.BICUBIC))
            bio = io.BytesIO()
            kw = {'restart_marker_blocks': int(g.integers(1, 9))} if i % 2 else {}
            Image.fromarray(a).save(bio, 'JPEG', quality=int(g.integers(30, 96)), subsampling=int(g.integers(0, 3)), **kw)
            raw = bio.getvalue()
        raw = bytearray(raw)
        first = scan_start(bytes(raw))
        for _ in range(int(g.integers(1, 4))):
            pos = int(g.integers(first, len(raw) - 2))
            if raw[pos] != 0xff and raw[pos - 1] != 0xff:      # markers and stuffed bytes stay
                raw[pos] = int(g.integers(0, 255))
        out.append(('random_%d' % i, bytes(raw)))
    return out
