"""Test-only: the progressive files the scan-plan tests share (tests/test_jpeg_scan_plan.py on the CPU, tests/test_jpeg_scan_gpu.py on
the device) -- the clean corpus, the damaged streams of one small file, and a reader of the scan plan that takes every offset from
witw_amd/csrc/jpeg_layout.h (read as text, as tests/test_jpeg.py reads it). Each list is built once per process."""
import functools
import os
import re

import numpy as np

from witw_amd import jpeg

from . import jpeg_prog_craft as PC
from .test_jpeg_progressive import crafted_cases, flat_blocks_file, picture, save, source, with_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((8, 8), (17, 9), (40, 56), (64, 64))
SAMPLINGS = ('grey', '444', '422', '420')


@functools.lru_cache(maxsize=None)
def layout():
    """every `WITW_JPEG_NAME = value` of the layout header -> {NAME: value}"""
    with open(os.path.join(ROOT, 'witw_amd', 'csrc', 'jpeg_layout.h')) as f:
        text = re.sub(r'//[^\n]*', '', f.read())
    return {n[len('WITW_JPEG_'):]: int(v, 0) for n, v in re.findall(r'\b(WITW_JPEG_\w+)\s*=\s*(0[xX][0-9a-fA-F]+|\d+)\b', text)}


def plan_scans(plan):
    """the scan records of a scan plan (uint8 array) -> list of dicts: comps, ss, se, ah, al, cols, rows, restart, stage, segs, and
    segments = [(byte offset, first unit, units)]"""
    L = layout()
    h = plan[:128].view(np.int32)
    assert int(h[0]) == L['PLAN_PROG_MAGIC'] and int(h[L['PLAN_PROG_BYTES']]) == plan.size
    out = []
    for s in range(int(h[L['PLAN_PROG_SCANS']])):
        at = L['PLAN_PROG_SCAN_AT'] + 4 * L['PLAN_PROG_SCAN_INTS'] * s
        r = plan[at:at + 4 * L['PLAN_PROG_SCAN_INTS']].view(np.int32)
        g = lambda name: int(r[L['PLAN_PROG_SCAN_' + name]])      # noqa: E731
        n_seg = g('SEGS')
        seg = plan[g('SEGS_AT'):g('SEGS_AT') + 4 * L['PLAN_PROG_SEG_INTS'] * n_seg].view(np.uint32).reshape(n_seg, L['PLAN_PROG_SEG_INTS'])
        out.append(dict(comps=tuple(int(r[L['PLAN_PROG_SCAN_COMPS'] + k]) for k in range(g('NS'))), ss=g('SS'), se=g('SE'), ah=g('AH'),
                        al=g('AL'), cols=g('COLS'), rows=g('ROWS'), restart=g('RESTART'), stage=g('STAGE'), segs=n_seg,
                        data_end=g('DATA_END'), segments=[tuple(int(x) for x in row) for row in seg]))
    return out


def scan_plan(data):
    """the file's scan plan (uint8 array) or None"""
    f = jpeg.open_file(data, progressive='device')
    pl = f.scan_plan() if f is not None else None
    return None if pl is None else pl[0]


def greatest_eob_runs():
    """tests/test_jpeg_progressive.py test_eob_runs_of_the_greatest_length_and_across_restarts: 33,124 blocks with a handful of AC
    coefficients, EOB runs of 32,767 carried over block rows, without and with restart markers cutting them"""
    g = np.random.Generator(np.random.Philox(key=[31, 1456]))
    coef = np.zeros((182 * 182, 64), dtype=np.int16)
    coef[:, 0] = g.integers(-100, 101, size=coef.shape[0])
    coef[[5, 20000, 33000, 33123], 1] = (3, -2, 1, 5)
    coef[33001, 9] = -1
    qt = np.full((1, 64), 2, dtype=np.uint16)
    return [('eob_greatest_dri%d' % dri, PC.write(1456, 1456, coef, qt, 'grey', with_options(PC.script_successive(1, al=1), dri=dri)))
            for dri in (0, 40000 // 3)]


@functools.lru_cache(maxsize=None)
def clean_corpus():
    """[(name, bytes)]: Pillow's progressive files for every sampling and size, every crafted scan script (spectral splits, successive
    approximation with al = 3, DC in separate scans, restart intervals, a table lengthened with min_len = 12: codes past the 11-bit
    look-up), one EOB run over more than 1,024 blocks, the greatest-length EOB runs across restarts, an AC band split at every position"""
    out = []
    for sampling in SAMPLINGS:
        for (h, w) in SIZES:
            out.append(('twin_%s_%dx%d' % (sampling, h, w), save(picture(h * 100 + w, h, w, grey=sampling == 'grey'), sampling, 95, progressive=True)))
    for name, sampling, size, script, kw in crafted_cases():
        _seq, src = source(sampling, size[0], size[1], **kw)
        out.append((name, PC.write(size[0], size[1], src.coef, src.qt, sampling, script)))
        if name == 'codes_past_the_look_ahead':
            assert script[0]['min_len'] == 12
    out.append(('flat', flat_blocks_file()[2]))
    out += greatest_eob_runs()
    _seq, src = source('grey', 17, 9, quality=98)
    for k in range(1, 63):
        out.append(('band_split_%02d' % k, PC.write(17, 9, src.coef, src.qt, 'grey', PC.script_successive(1, al=1, bands=((1, k), (k + 1, 63))))))
    return out


@functools.lru_cache(maxsize=None)
def segments_400():
    """grey 160 x 160 with a restart marker behind every block: 400 segments in every scan, more than a workgroup has threads"""
    _seq, src = source('grey', 160, 160, quality=85, seed=160)
    return PC.write(160, 160, src.coef, src.qt, 'grey', with_options(PC.script_successive(1, al=1), dri=1))


@functools.lru_cache(maxsize=None)
def small_file():
    """the 17 x 9 4:2:0 file whose truncations and corruptions the damage tests use (that of tests/test_jpeg_progressive_san.py)"""
    return save(picture(1709, 17, 9), '420', 90, progressive=True)


def truncations():
    small = small_file()
    return [('cut_%04d' % n, small[:n]) for n in range(len(small))]


@functools.lru_cache(maxsize=None)
def corruptions():
    """2,000 single-byte corruptions of small_file()"""
    small = small_file()
    g = np.random.Generator(np.random.Philox(key=[31, 2000]))
    out = []
    for k in range(2000):
        b = bytearray(small)
        b[int(g.integers(0, len(b)))] = int(g.integers(0, 256))
        out.append(('flip_%04d' % k, bytes(b)))
    return out


def host_decode(data):
    """witw_jpeg_decode_coef_ex under the progressive flag -> (rc of witw_jpeg_info_ex, rc of the decode or None, coef or None)"""
    lib = jpeg.host_lib()
    d = np.frombuffer(data, dtype=np.uint8)
    info = np.zeros(22, dtype=np.int32)
    rc = lib.witw_jpeg_info_ex(d.ctypes.data, d.size, info.ctypes.data, 1)
    if rc < 0:
        return rc, None, None
    coef = np.zeros((int(info[5]), 64), dtype=np.int16)
    qt = np.zeros((int(info[2]), 64), dtype=np.uint16)
    return rc, int(lib.witw_jpeg_decode_coef_ex(d.ctypes.data, d.size, coef.ctypes.data, qt.ctypes.data, 1)), coef
