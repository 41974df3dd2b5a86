"""Test-only 4:4:0 (h1v2) JPEG files: luma sampled (1, 2), both chroma (1, 1) -- what a losslessly rotated 4:2:2 file holds. Pillow's
encoder cannot write this sampling, so the files come from the writers of tests/jpeg_craft.py (baseline) and tests/jpeg_prog_craft.py
(progressive), which take their geometry from jpeg_craft.SAMPLINGS. The entry '440' is in that dict only while one of the functions
here runs (registered()): the corpora of the other tests, which walk the dict, stay as they are.

Also here: the numpy restatement of libjpeg's h1v2 'fancy' upsampler (jdsample.c h1v2_fancy_upsample) and of the whole back end for such
a file, held to Pillow's bytes by tests/test_jpeg_440.py -- that test is what pins the arithmetic of the device kernel's mode 5."""
import contextlib
import io

import numpy as np

from oracle import jpeg_oracle as J

from . import jpeg_craft as JC
from . import jpeg_prog_craft as PC

NAME = '440'
HV = [(1, 2), (1, 1), (1, 1)]
H1V2 = 2               # flag bit 1 of the _ex entries of libwitw_jpeg.so
PROGRESSIVE = 1        # flag bit 0


@contextlib.contextmanager
def registered():
    """jpeg_craft.SAMPLINGS (the one dict jpeg_prog_craft shares) holds '440' inside the block only"""
    had = NAME in JC.SAMPLINGS
    JC.SAMPLINGS[NAME] = HV
    try:
        yield
    finally:
        if not had:
            del JC.SAMPLINGS[NAME]


def geometry(H, W):
    with registered():
        return JC.geometry(H, W, NAME)


def scan_rows(H, W):
    with registered():
        return JC.scan_rows(H, W, NAME)


def random_coef(g, H, W, **kw):
    with registered():
        return JC.random_coef(g, H, W, NAME, **kw)


def write(H, W, coef, qt, **kw):
    """a baseline 4:4:0 file (jpeg_craft.write's keywords: tables, dri, inject, truncate, ...)"""
    with registered():
        return JC.write(H, W, coef, qt, NAME, **kw)


def write_progressive(H, W, coef, qt, script):
    with registered():
        return PC.write(H, W, coef, qt, NAME, script)


def picture_coef(seed, H, W, quality=90):
    """(coef, qt) of a 4:4:0 file with photographic statistics: the TRANSPOSED coefficient blocks of the 4:2:2 file Pillow writes of
    the transposed picture -- what a lossless transposition (jpegtran -transpose) makes of that file. A photograph's coefficients
    stay inside the range in which Pillow's SIMD inverse DCT and the integer one agree (jpeg_craft.in_range)."""
    from PIL import Image
    from witw_amd import jpeg
    g = np.random.Generator(np.random.Philox(key=[44, seed]))
    small = g.integers(0, 256, size=(W // 8 + 2, H // 8 + 2, 3), dtype=np.uint8)
    img = np.asarray(Image.fromarray(small).resize((H + 16, W + 16), Image.BICUBIC))[8:8 + W, 8:8 + H]      # W rows x H columns
    a = np.clip(img.astype(np.int16) + g.integers(-20, 21, size=(W, H, 3)), 0, 255).astype(np.uint8)
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, 'JPEG', quality=quality, subsampling=1)
    return transposed(jpeg.read_coef(bio.getvalue()))


def transposed(src):
    """(coef, qt) of the 4:4:0 file a lossless transposition makes of the 4:2:2 file `src` (a JpegCoef): the block grid of every
    component transposed, and every block, and every quantisation table"""
    H, W = int(src.info[1]), int(src.info[0])
    comps, nblk, _mx, _my = geometry(H, W)
    out, off_s, off_d = np.zeros((nblk, 64), dtype=np.int16), 0, 0
    for c, (_h, _v, bw, bh) in enumerate(comps):
        sbw, sbh = int(src.info[8 + 4 * c]), int(src.info[9 + 4 * c])
        assert (sbw, sbh) == (bh, bw)
        s = src.coef[off_s:off_s + sbw * sbh].reshape(sbh, sbw, 8, 8)
        out[off_d:off_d + bw * bh] = s.transpose(1, 0, 3, 2).reshape(-1, 64)
        off_s += sbw * sbh
        off_d += bw * bh
    return out, src.qt.reshape(-1, 8, 8).transpose(0, 2, 1).reshape(-1, 64).copy()


def upsample_h1v2(p):
    """p uint8 [h, w] (real samples only) -> [2h, w] (jdsample.c h1v2_fancy_upsample: 3/4 nearest + 1/4 next nearest row, bias 1 for the
    upper and 2 for the lower output row; the row above the first / below the last real row is that row again: jdmainct.c context
    rows). libjpeg picks it for every h1v2 component under fancy upsampling, whatever the plane's size: no replicating variant."""
    a = p.astype(np.int64)
    up = np.concatenate((a[:1], a[:-1]), 0)
    dn = np.concatenate((a[1:], a[-1:]), 0)
    out = np.empty((2 * a.shape[0], a.shape[1]), dtype=np.int64)
    out[0::2] = (3 * a + up + 1) >> 2
    out[1::2] = (3 * a + dn + 2) >> 2
    return out.astype(np.uint8)


def decode(info, coef, qt):
    """the back end for a 4:4:0 file: oracle.jpeg_oracle's dequantisation + inverse DCT and colour conversion around upsample_h1v2
    -> uint8 [H, W, 3]"""
    H, W, ncomp, hmax, vmax = (int(v) for v in info[:5])
    assert (ncomp, hmax, vmax) == (3, 1, 2)
    planes, off = [], 0
    for c in range(3):
        bw, bh = int(info[8 + 4 * c]), int(info[9 + 4 * c])
        planes.append(J.plane(coef[off:off + bw * bh], qt[c], bh, bw))
        off += bw * bh
    ch = -(-H // 2)
    return J.ycc_to_rgb(planes[0][:H, :W], *(upsample_h1v2(p[:ch, :W])[:H] for p in planes[1:]))


def info_of(H, W):
    """the 22 ints witw_jpeg_info_ex gives for a 4:4:0 file of H x W"""
    comps, nblk, _mx, _my = geometry(H, W)
    info = np.zeros(22, dtype=np.int32)
    info[:6] = (H, W, 3, 1, 2, nblk)
    for c, (h, v, bw, bh) in enumerate(comps):
        info[6 + 4 * c:10 + 4 * c] = (h, v, bw, bh)
    return info


def pixel_coef(g, H, W):
    """random coefficients inside the range in which the file's pixels are comparable with Pillow's (jpeg_craft.in_range)"""
    return random_coef(g, H, W, density=0.12, amp=30, dc_amp=120)


SIZES = ((8, 8), (8, 16), (9, 17), (16, 8), (40, 48), (41, 23))      # H x W
DRIS = (0, 1, 2, 5)


def corpus(seed=5):
    """[(name, H, W, file bytes, written coefficients, qt)]: SIZES x DRIS x {standard, long-code} tables. Standard-table files hold
    coefficients whose pixels compare with Pillow's; long-code files hold magnitudes up to category 15 (coefficients only)."""
    g = np.random.Generator(np.random.Philox(key=[seed, 440]))
    out = []
    for (H, W) in SIZES:
        for dri in DRIS:
            for tname in ('std', 'long'):
                if tname == 'long':
                    c = random_coef(g, H, W, density=0.2, amp=32767, dc_amp=16000)
                    qt = JC.flat_qt(3, 1)
                    tabs = JC.long_code_tables()
                else:
                    c = pixel_coef(g, H, W)
                    qt = g.integers(1, 5, size=(3, 64)).astype(np.uint16)
                    tabs = None
                out.append(('%dx%d_dri%d_%s' % (H, W, dri, tname), H, W, write(H, W, c, qt, tables=tabs, dri=dri), c, qt))
    return out
