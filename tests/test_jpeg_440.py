"""4:4:0 (h1v2) JPEG files, CPU side (opt-in: jpeg.SAMPLING_440 / WITW_JPEG_440, open_file / read_coef(h1v2=), flag bit 1 of the _ex
entries of libwitw_jpeg.so): with nothing set such a file is Pillow's as before; with the opt-in the host decoder returns the
coefficients the file was written from (tests/jpeg_440_craft.py: Pillow cannot write the sampling), the entropy plan describes the
1 x 2 MCU to the device decoders, a progressive twin gives the same blocks when both opt-ins are on, and the numpy restatement of
libjpeg's h1v2 upsampler behind the oracle's inverse DCT equals Pillow byte for byte -- which is what pins upsampling mode 5 of
csrc/jpeg.hip. tests/test_jpeg_440_gpu.py takes the same files through the device."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from witw_amd import jpeg

from . import jpeg_440_craft as C4
from . import jpeg_craft as JC
from . import jpeg_prog_craft as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, 'tests', 'golden', 'jpeg', '440')
FIXTURES = ('s440_q90', 's440_rst')
CORPUS = C4.corpus()


def fixture(name):
    return open(os.path.join(HERE, name + '.jpg'), 'rb').read()


def expected():
    return np.load(os.path.join(HERE, 'expected_440.npz'))


def decode_ex(data, flags):
    """the C entry points themselves -> (witw_jpeg_info_ex, witw_jpeg_decode_coef_ex or None, coef, qt, info)"""
    lib = jpeg.host_lib()
    d = np.frombuffer(data, dtype=np.uint8)
    info = np.zeros(22, dtype=np.int32)
    rc = lib.witw_jpeg_info_ex(d.ctypes.data, d.size, info.ctypes.data, flags)
    if rc < 0:
        return rc, None, None, None, info
    coef = np.full((int(info[5]), 64), 0x5555, dtype=np.int16)
    qt = np.zeros((int(info[2]), 64), dtype=np.uint16)
    return rc, lib.witw_jpeg_decode_coef_ex(d.ctypes.data, d.size, coef.ctypes.data, qt.ctypes.data, flags), coef, qt, info


def plan_ex(data, flags):
    """-> (witw_jpeg_entropy_plan_bytes_ex, witw_jpeg_entropy_plan_ex, plan)"""
    lib = jpeg.host_lib()
    d = np.frombuffer(data, dtype=np.uint8)
    n = int(lib.witw_jpeg_entropy_plan_bytes_ex(d.ctypes.data, d.size, flags))
    plan, qt = np.zeros(max(n, 4096), np.uint8), np.zeros((3, 64), np.uint16)
    return n, int(lib.witw_jpeg_entropy_plan_ex(d.ctypes.data, d.size, plan.ctypes.data, ctypes.c_size_t(plan.size), qt.ctypes.data, flags)), plan


# ---- the default ----------------------------------------------------------------------------------------------------------------------

def test_default_is_unchanged():
    assert jpeg.SAMPLING_440 is False or os.environ.get('WITW_JPEG_440')
    lib = jpeg.host_lib()
    for name in FIXTURES:
        data = fixture(name)
        if not os.environ.get('WITW_JPEG_440'):
            assert jpeg.open_file(data) is None and jpeg.read_coef(data) is None
        assert jpeg.open_file(data, h1v2=False) is None and jpeg.read_coef(data, h1v2=False) is None
        assert jpeg.open_file(data, progressive=True, h1v2=False) is None
        d = np.frombuffer(data, dtype=np.uint8)
        info = np.zeros(22, dtype=np.int32)
        coef, qt = np.zeros((72, 64), np.int16), np.zeros((3, 64), np.uint16)
        assert lib.witw_jpeg_info(d.ctypes.data, d.size, info.ctypes.data) == -2
        assert lib.witw_jpeg_decode_coef(d.ctypes.data, d.size, coef.ctypes.data, qt.ctypes.data) == -2
        assert lib.witw_jpeg_entropy_plan_bytes(d.ctypes.data, d.size) == 0
        plan = np.zeros(4096, np.uint8)
        assert lib.witw_jpeg_entropy_plan(d.ctypes.data, d.size, plan.ctypes.data, ctypes.c_size_t(plan.size), qt.ctypes.data) == -2
        for flags in (0, 1):                             # bit 1 clear
            assert decode_ex(data, flags)[0] == -2
            assert lib.witw_jpeg_decode_coef_ex(d.ctypes.data, d.size, coef.ctypes.data, qt.ctypes.data, flags) == -2
            assert plan_ex(data, flags)[:2] == (0, -2)
    # the other samplings through the entries with bit 1 set: as through the plain ones
    g = np.random.Generator(np.random.Philox(key=[5, 441]))
    for sampling in ('grey', '444', '422', '420'):
        c = JC.random_coef(g, 41, 23, sampling)
        data = JC.write(41, 23, c, JC.flat_qt(len(JC.SAMPLINGS[sampling]), 2), sampling, dri=3)
        ref = jpeg.read_coef(data)
        rc_info, rc, coef, qt, info = decode_ex(data, C4.H1V2)
        assert (rc_info, rc) == (0, 0)
        np.testing.assert_array_equal(coef, ref.coef)
        np.testing.assert_array_equal(info, ref.info)
        n, rc, plan = plan_ex(data, C4.H1V2)
        ref_plan, _qt = jpeg.open_file(data).entropy_plan()
        assert n == rc == ref_plan.size
        np.testing.assert_array_equal(plan[:n], ref_plan)
    assert C4.NAME not in JC.SAMPLINGS                    # the helper leaves the writers' table as the other tests see it


# ---- the host decoder -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', [c[0] for c in CORPUS])
def test_host_decoder_returns_the_written_coefficients(name):
    """8x8 .. 41x23 (one MCU; a padded lower luma block; odd sizes; several MCU rows and columns), DRI 0 / 1 / 2 / 5, standard and
    long-code tables: every block, MCU padding included, through the C entry and through read_coef"""
    _n, H, W, data, coef, qt = next(c for c in CORPUS if c[0] == name)
    rc_info, rc, got, got_qt, info = decode_ex(data, C4.H1V2)
    assert (rc_info, rc) == (0, 0)
    np.testing.assert_array_equal(info, C4.info_of(H, W))
    np.testing.assert_array_equal(got_qt, qt)
    bad = np.nonzero((got != coef).any(axis=1))[0]
    assert bad.size == 0, '%d of %d blocks differ, first %s' % (bad.size, coef.shape[0], bad[:5])
    r = jpeg.read_coef(data, h1v2=True)
    np.testing.assert_array_equal(r.coef, coef)
    assert r.shape == (H, W, 3)
    assert decode_ex(data, C4.H1V2 | C4.PROGRESSIVE)[:2] == (0, 0)


@pytest.mark.parametrize('name', [c[0] for c in CORPUS if c[0].startswith(('9x17_', '41x23_', '8x16_dri0'))])
def test_entropy_plan_gives_the_device_decoders_the_1x2_mcu(name):
    """the plan's per-component (h, v, blocks wide, blocks high, first block) and scan order are all the device decoders know of the
    geometry: a plain-Python rendering of their algorithm (tests/test_jpeg.py) decodes the file from the plan alone"""
    from .test_jpeg import _decode_from_plan
    _n, H, W, data, coef, qt = next(c for c in CORPUS if c[0] == name)
    f = jpeg.open_file(data, h1v2=True)
    plan, plan_qt = f.entropy_plan()
    np.testing.assert_array_equal(plan_qt, qt)
    hdr = plan[:128].view(np.int32)
    comps, nblk, mx, my = C4.geometry(H, W)
    dri = int(name.split('_')[1][3:])
    assert list(hdr[1:6]) == [-(-mx * my // dri) if dri else 1, dri or mx * my, mx, my, 3]
    first = np.cumsum([0] + [bw * bh for _h, _v, bw, bh in comps])
    for c, (h, v, bw, bh) in enumerate(comps):
        assert list(hdr[6 + 7 * c:11 + 7 * c]) == [h, v, bw, bh, first[c]]
    assert list(hdr[28:31]) == [0, 1, 2] and (hdr[6], hdr[7]) == (1, 2)
    np.testing.assert_array_equal(_decode_from_plan(np.frombuffer(data, dtype=np.uint8), plan, nblk), coef)


@pytest.mark.parametrize('size', C4.SIZES)
def test_progressive_twin_gives_the_sequential_files_coefficients(size):
    """both opt-ins on: interleaved DC scans walk the 1 x 2 MCUs, the single-component scans the component's own block grid (for luma
    ceil(H / 8) rows: the lower block of the last MCU row may be padding no AC scan visits); with either opt-in off the file is Pillow's"""
    H, W = size
    coef, qt = C4.picture_coef(H * 100 + W, H, W)
    seq = C4.write(H, W, coef, qt)
    for script in (PC.script_spectral(3), PC.script_successive(3, al=2, bands=((1, 9), (10, 63))),
                   [dict(s, dri=(0, 2, 5)[i % 3]) for i, s in enumerate(PC.script_successive(3, al=1))]):
        prog = C4.write_progressive(H, W, coef, qt, script)
        np.testing.assert_array_equal(JC.pillow(prog), JC.pillow(seq))              # a legal stream that means the same picture
        assert jpeg.read_coef(prog) is None and jpeg.read_coef(prog, progressive=True) is None and jpeg.read_coef(prog, h1v2=True) is None
        assert decode_ex(prog, C4.PROGRESSIVE)[0] == -2 and decode_ex(prog, C4.H1V2)[0] == -2
        p, s = jpeg.read_coef(prog, progressive=True, h1v2=True), jpeg.read_coef(seq, h1v2=True)
        np.testing.assert_array_equal(p.info, s.info)
        np.testing.assert_array_equal(p.qt, s.qt)
        np.testing.assert_array_equal(p.coef, s.coef)
        np.testing.assert_array_equal(s.coef, coef)
        f = jpeg.open_file(prog, progressive=True, h1v2=True)
        assert f.progressive and f.entropy_plan() is None
        assert plan_ex(prog, C4.H1V2 | C4.PROGRESSIVE)[:2] == (0, -2)


# ---- the upsampler's arithmetic ---------------------------------------------------------------------------------------------------------

def test_fixtures_are_what_this_pillow_decodes():
    exp = expected()
    for name in FIXTURES:
        np.testing.assert_array_equal(JC.pillow(fixture(name)), exp[name])
        r = jpeg.read_coef(fixture(name), h1v2=True)
        np.testing.assert_array_equal(r.coef, exp[name + '_coef'])
        np.testing.assert_array_equal(r.qt, exp[name + '_qt'])
        np.testing.assert_array_equal(C4.decode(r.info, r.coef, r.qt), exp[name])
    np.testing.assert_array_equal(exp['s440_q90'], exp['s440_rst'])


def test_h1v2_upsampling_restatement_equals_pillow_on_the_corpus():
    """dequantise -> inverse DCT -> h1v2 upsample -> colour (jpeg_440_craft.decode: the oracle's stages around upsample_h1v2) against
    Image.open on every file of the corpus whose dequantised coefficients stay in an encoder's range (jpeg_craft.in_range: beyond it
    Pillow's SIMD inverse DCT wraps differently from the integer form, whatever the sampling) -- all standard-table files are"""
    compared = 0
    for name, H, W, data, coef, qt in CORPUS:
        r = jpeg.read_coef(data, h1v2=True)
        if not JC.in_range(r.info, r.coef, r.qt):
            assert name.endswith('_long')
            continue
        np.testing.assert_array_equal(C4.decode(r.info, r.coef, r.qt), JC.pillow(data), err_msg=name)
        compared += 1
    assert compared == len(C4.SIZES) * len(C4.DRIS)


@pytest.mark.parametrize('size', [(1, 1), (1, 8), (2, 8), (2, 2), (3, 5), (4, 1), (5, 2), (9, 8), (17, 3), (25, 40), (41, 9), (57, 16), (16, 33)])
def test_h1v2_upsampling_degenerate_planes(size):
    """chroma planes of one and two rows (H <= 4), of one and two columns (where libjpeg replicates for the HORIZONTAL modes: here it
    filters all the same), odd heights 8k + 1 (the last chroma row stands for one luma row) and 16k + 9 (the last MCU row's lower luma
    block is padding): photographic coefficients, and flat random ones in range"""
    H, W = size
    g = np.random.Generator(np.random.Philox(key=[H, W]))
    for coef, qt in (C4.picture_coef(H * 1000 + W, H, W, quality=92), (C4.pixel_coef(g, H, W), JC.flat_qt(3, 3))):
        data = C4.write(H, W, coef, qt)
        r = jpeg.read_coef(data, h1v2=True)
        assert JC.in_range(r.info, r.coef, r.qt)
        np.testing.assert_array_equal(C4.decode(r.info, r.coef, r.qt), JC.pillow(data))


def test_decode_tables_number_the_new_mode():
    """(hmax, vmax) = (1, 2) -> mode 5 at every width (no replicating variant); chroma rows = ceil(H / 2), columns = W; other samplings
    keep their modes; anything else still raises"""
    rows = []
    for (H, W, hv) in ((40, 48, (1, 2)), (9, 1, (1, 2)), (3, 2, (1, 2)), (40, 48, (2, 1)), (40, 2, (2, 1)), (40, 48, (2, 2)), (40, 48, (1, 1))):
        with C4.registered():
            name = {(1, 2): '440', (2, 1): '422', (2, 2): '420', (1, 1): '444'}[hv]
            comps, nblk, _mx, _my = JC.geometry(H, W, name)
        d = np.zeros(jpeg.DESC_COLS, dtype=np.int64)
        d[2:8] = (H, W, 3, hv[0], hv[1], nblk)
        for c, (h, v, bw, bh) in enumerate(comps):
            d[8 + 4 * c:12 + 4 * c] = (h, v, bw, bh)
        d[0], d[1] = 128 * sum(int(r[7]) for r in rows), 1 << 20
        rows.append(d)
    _planes, images, _blk, _pb, _ob, _qb = jpeg.decode_tables(np.stack(rows))
    assert list(images[:, 3]) == [5, 5, 5, 1, 3, 2, 0]
    assert [tuple(r) for r in images[:3, 9:11]] == [(20, 48), (5, 1), (2, 2)]
    bad = rows[0].copy()
    bad[5], bad[6] = 2, 4
    with pytest.raises(ValueError):
        jpeg.decode_tables(bad[None])


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def _patch_sof(data, comp, hv, marker=b'\xff\xc0'):
    b = bytearray(data)
    i = b.index(marker)
    b[i + 4 + 6 + 3 * comp + 1] = hv
    return bytes(b)


def _refused(data):
    return jpeg.open_file(data, h1v2=True) is None and jpeg.read_coef(data, h1v2=True) is None and \
        decode_ex(data, C4.H1V2)[0] == -2 and decode_ex(data, C4.H1V2 | C4.PROGRESSIVE)[0] == -2 and plan_ex(data, C4.H1V2)[:2] == (0, -2)


def test_other_samplings_and_colour_spaces_stay_refused_with_the_opt_in():
    from PIL import Image
    a = (np.arange(48 * 40 * 3, dtype=np.uint32).reshape(48, 40, 3) * 7 % 256).astype(np.uint8)

    def pil(**kw):
        bio = io.BytesIO()
        Image.fromarray(a).save(bio, 'JPEG', quality=90, **kw)
        return bio.getvalue()
    s422 = pil(subsampling=1)
    assert jpeg.open_file(s422, h1v2=True) is not None
    assert _refused(_patch_sof(_patch_sof(s422, 0, 0x21), 1, 0x12))            # luma 2x1 with a chroma 1x2
    assert _refused(_patch_sof(_patch_sof(s422, 0, 0x12), 2, 0x12))            # luma 1x2 with a chroma 1x2
    assert _refused(_patch_sof(s422, 0, 0x14)) and _refused(_patch_sof(s422, 0, 0x13))      # 1x4, 1x3
    # 4:1:1 (luma 4x1). What Pillow writes for subsampling='4:1:1' is luma 2x2 -- 4:2:0 under another name, taken as ever -- so
    # the real thing is made by declaring it in the frame header
    s411 = pil(subsampling='4:1:1')
    assert s411[s411.index(b'\xff\xc0') + 11] == 0x22 and jpeg.open_file(s411, h1v2=True) is not None
    assert _refused(_patch_sof(s422, 0, 0x41))
    ok = fixture('s440_q90')
    assert jpeg.open_file(ok, h1v2=True) is not None
    # RGB colour space: no JFIF marker and the component ids 'R', 'G', 'B'; an Adobe marker with transform 0 (RGB) or 2 (YCCK)
    i = ok.index(b'\xff\xe0')
    ln = int.from_bytes(ok[i + 2:i + 4], 'big')
    bare = ok[:i] + ok[i + 2 + ln:]
    assert jpeg.open_file(bare, h1v2=True) is not None
    b = bytearray(bare)
    j, k = b.index(b'\xff\xc0'), b.index(b'\xff\xda')
    for c, ch in enumerate(b'RGB'):
        b[j + 4 + 6 + 3 * c] = ch
        b[k + 5 + 2 * c] = ch
    assert _refused(bytes(b))
    for transform, ours in ((1, True), (0, False), (2, False)):
        f = ok[:i] + b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00' + bytes([transform]) + ok[i + 2 + ln:]
        assert (jpeg.open_file(f, h1v2=True) is not None) == ours and (ours or _refused(f))
    rgb = pil(subsampling=0, keep_rgb=True)
    assert _refused(rgb) and _refused(_patch_sof(rgb, 0, 0x12))
    # CMYK (four components) with a 1x2 first component
    bio = io.BytesIO()
    Image.fromarray(np.dstack([a, a[:, :, :1]]), 'CMYK').save(bio, 'JPEG', quality=90)
    cmyk = bio.getvalue()
    assert cmyk[cmyk.index(b'\xff\xc0') + 9] == 4 and _refused(cmyk) and _refused(_patch_sof(cmyk, 0, 0x12))
    # a progressive 4:4:0 file needs both bits; 12-bit samples stay refused
    b = bytearray(ok)
    b[b.index(b'\xff\xc0') + 4] = 12
    assert _refused(bytes(b))


# ---- damage ---------------------------------------------------------------------------------------------------------------------------

def _second_luma_damage(sampling, H, W, dri, mcu, kind):
    """a file of `sampling` ('440': MCU = Y, Y below, Cb, Cr; '422': Y, Y right, Cb, Cr) whose block 1 of MCU `mcu` -- the second luma
    block -- is damaged: 'cut' = the data ends inside it: that block holds 63 coefficients of 1000 (26 bits each under the standard
    table: 200 bytes), every other block a DC value alone, and the data is cut 30 bytes behind the point from which the file differs
    from its twin without those coefficients; 'inval' = 16 one-bits, no code of the table, in front of it"""
    with C4.registered():
        nblk = JC.geometry(H, W, sampling)[1]
        rows = JC.scan_rows(H, W, sampling)
        coef = np.zeros((nblk, 64), dtype=np.int16)
        coef[:, 0] = 5
        b = 4 * mcu + 1
        if kind == 'inval':
            return JC.write(H, W, coef, JC.flat_qt(3, 1), sampling, dri=dri, inject={b: {'pre': [JC.raw_bits('1' * 16)]}}), rows, b
        twin = JC.write(H, W, coef, JC.flat_qt(3, 1), sampling, dri=dri)
        coef[rows[b], 1:] = 1000
        full = JC.write(H, W, coef, JC.flat_qt(3, 1), sampling, dri=dri)
        s = JC.scan_start(full)
        differ = next(i for i in range(s, len(full)) if full[i] != twin[i])
        return JC.write(H, W, coef, JC.flat_qt(3, 1), sampling, dri=dri, truncate=differ - s + 30), rows, b


@pytest.mark.parametrize('kind', ['cut', 'inval'])
@pytest.mark.parametrize('shape', [(8, 16, 0, 0), (40, 48, 0, 7), (40, 48, 2, 7), (41, 23, 1, 4)])
def test_damage_in_the_second_luma_block_is_the_code_of_the_422_case(shape, kind):
    H, W, dri, mcu = shape
    d440, rows, b = _second_luma_damage('440', H, W, dri, mcu, kind)
    d422, _r, _b = _second_luma_damage('422', W, H, dri, mcu, kind)        # the transposed geometry: as many MCUs
    rc_info, rc, coef, _qt, _info = decode_ex(d440, C4.H1V2)
    assert (rc_info, rc) == (0, -3)
    assert decode_ex(d422, C4.H1V2)[:2] == (rc_info, rc) and decode_ex(d422, 0)[:2] == (rc_info, rc)
    assert jpeg.read_coef(d440, h1v2=True) is None
    # the decode stopped inside that very block: the first luma block of the MCU is whole, nothing behind the damaged block is written
    assert coef[rows[b - 1], 0] == 5 and not coef[rows[b - 1], 1:].any()
    assert not coef[rows[b + 1:]].any()
    if kind == 'cut':
        assert coef[rows[b], 1] == 1000 and not (coef[rows[b], 1:] == 1000).all()


def test_pack_hands_a_damaged_440_file_to_pillow(monkeypatch):
    """the host-coefficient route (DEVICE_ENTROPY off): decode_into fails inside pack(), Pillow's pixels ride in the file's span"""
    monkeypatch.setattr(jpeg, 'DEVICE_ENTROPY', False)
    bad, _rows, _b = _second_luma_damage('440', 40, 48, 2, 7, 'inval')
    good = fixture('s440_rst')
    buf, desc, _k = jpeg.pack([jpeg.open_file(bad, h1v2=True), jpeg.open_file(good, h1v2=True)])
    d = desc.numpy()
    assert list(d[:, 24]) == [1, 0] and list(d[:, 26]) == [0, 0] and (int(d[0, 2]), int(d[0, 3]), int(d[0, 25])) == (40, 48, 3)
    np.testing.assert_array_equal(buf.numpy()[d[0, 0]:d[0, 0] + 40 * 48 * 3].reshape(40, 48, 3), JC.pillow(bad))
    np.testing.assert_array_equal(buf.numpy()[d[1, 0]:d[1, 0] + 72 * 128].view(np.int16).reshape(-1, 64), expected()['s440_rst_coef'])


# ---- the flag's way through Python ---------------------------------------------------------------------------------------------------

def test_module_flag_is_the_default_of_the_keyword(monkeypatch):
    data = fixture('s440_q90')
    monkeypatch.setattr(jpeg, 'SAMPLING_440', True)
    assert jpeg.open_file(data) is not None and jpeg.read_coef(data) is not None and jpeg.open_file(data, h1v2=False) is None
    assert jpeg.open_file(data).flags == jpeg.ACCEPT_H1V2 == C4.H1V2


def test_environment_variable_sets_the_module_flag():
    import sys
    code = 'from witw_amd import jpeg; print(int(jpeg.SAMPLING_440), int(jpeg.PROGRESSIVE))'
    for value, want in (('1', '1 0'), ('on', '1 0'), ('TRUE', '1 0'), ('0', '0 0'), ('', '0 0')):
        env = dict(os.environ, WITW_JPEG_440=value, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        env.pop('WITW_JPEG_PROGRESSIVE', None)
        p = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, cwd=ROOT)
        assert p.stdout.strip().splitlines()[-1:] == [want], (value, p.stdout, p.stderr[-500:])


@pytest.mark.parametrize('device_entropy', ['all', 'restart', False])
def test_pack_takes_a_440_file_through_the_branches_of_a_422_file(monkeypatch, device_entropy):
    monkeypatch.setattr(jpeg, 'DEVICE_ENTROPY', device_entropy)
    monkeypatch.setattr(jpeg, 'SAMPLING_440', True)
    plain, rst = fixture('s440_q90'), fixture('s440_rst')
    coef, qt = C4.picture_coef(90, 40, 48, quality=90)
    with C4.registered():
        t_coef = JC.random_coef(np.random.Generator(np.random.Philox(key=[1, 2])), 48, 40, '422')
        s422 = JC.write(48, 40, t_coef, JC.flat_qt(3, 2), '422'), JC.write(48, 40, t_coef, JC.flat_qt(3, 2), '422', dri=2)
    prog = C4.write_progressive(40, 48, coef, qt, PC.script_spectral(3))
    items = [jpeg.open_file(x) for x in (plain, rst) + s422] + [jpeg.open_file(prog, progressive=True)]
    assert all(i is not None for i in items)
    buf, desc, kind = jpeg.pack(items)
    d = desc.numpy()
    want = {'all': [1, 1], 'restart': [0, 1], False: [0, 0]}[device_entropy]
    assert kind == jpeg.KIND_JPEG and not d[:, 24].any() and list(d[:, 26]) == want + want + [0]
    assert list(d[0, 2:8]) == [40, 48, 3, 1, 2, 72] and list(d[2, 2:8]) == [48, 40, 3, 2, 1, 72]
    b = buf.numpy()
    for i, data in ((0, plain), (1, rst)):
        if d[i, 26]:
            assert bytes(b[d[i, 0]:d[i, 0] + len(data)]) == data and d[i, 28] == len(data)
            assert b[d[i, 27]:d[i, 27] + 4].view(np.int32)[0] == 0x3157504A and d[i, 29] == (1 if i == 0 else 9)
        else:
            np.testing.assert_array_equal(b[d[i, 0]:d[i, 0] + 72 * 128].view(np.int16).reshape(-1, 64), coef)
        np.testing.assert_array_equal(b[d[i, 1]:d[i, 1] + 3 * 128].view(np.uint16).reshape(3, 64), qt)
    np.testing.assert_array_equal(b[d[4, 0]:d[4, 0] + 72 * 128].view(np.int16).reshape(-1, 64), coef)
    _planes, images, _blk, _pb, _ob, _qb = jpeg.decode_tables(d[d[:, 26] == 0]) if (d[:, 26] == 0).any() else (0, np.zeros((0, 12)), 0, 0, 0, 0)
    assert set(images[:, 3]) <= {1, 5}


def _pairs_csv(tmp_path, n=1):
    from PIL import Image
    rows = []
    for i in range(n):
        Image.fromarray(C4.decode(C4.info_of(40, 48), *C4.picture_coef(7 + i, 40, 48))).save(str(tmp_path / ('ov_%d.jpg' % i)), quality=88)
        with open(str(tmp_path / ('su_%d.jpg' % i)), 'wb') as f:
            f.write(C4.write(24 + 8 * i, 40, *C4.picture_coef(70 + i, 24 + 8 * i, 40), dri=(0, 3)[i % 2]))
        rows.append('ov_%d.jpg,su_%d.jpg' % (i, i))
    (tmp_path / 'pairs.csv').write_text('\n'.join(rows) + '\n')
    return str(tmp_path / 'pairs.csv')


def test_dataset_keyword_and_module_flag(tmp_path, monkeypatch):
    import inspect
    from witw_amd import cvig_baseline, cvig_fov, cvig_semantic
    for m in (cvig_fov, cvig_semantic, cvig_baseline):
        assert 'jpeg_440' in inspect.signature(m.ImagePairDataset.__init__).parameters, m.__name__
    csv = _pairs_csv(tmp_path)
    off = cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg')[0]
    assert isinstance(off['surface'], np.ndarray) and isinstance(off['overhead'], jpeg.JpegFile)
    on = cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg', jpeg_440=True)[0]
    assert isinstance(on['surface'], jpeg.JpegFile) and list(on['surface'].info[3:5]) == [1, 2]
    np.testing.assert_array_equal(off['surface'], JC.pillow(open(str(tmp_path / 'su_0.jpg'), 'rb').read()))
    monkeypatch.setattr(jpeg, 'SAMPLING_440', True)
    assert isinstance(cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg')[0]['surface'], jpeg.JpegFile)
    assert isinstance(cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg', jpeg_440=False)[0]['surface'], np.ndarray)
    ds = cvig_semantic.ImagePairDataset.__new__(cvig_semantic.ImagePairDataset)
    cvig_fov.ImagePairDataset.__init__(ds, 'cvusa', csv, raw='jpeg', jpeg_progressive=True, jpeg_440=True)
    assert ds.jpeg_440 is True and ds.jpeg_progressive is True


@pytest.mark.parametrize('how', ['keyword', 'environment'])
def test_flag_reaches_spawned_loader_workers(tmp_path, monkeypatch, how):
    """a spawned worker imports witw_amd.jpeg afresh: it sees the keyword (pickled with the dataset) or WITW_JPEG_440 (inherited)"""
    import torch
    from witw_amd import cvig_fov
    csv = _pairs_csv(tmp_path)
    if how == 'environment':
        monkeypatch.setenv('WITW_JPEG_440', '1')
    ds = cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg', jpeg_440=True if how == 'keyword' else None)
    loader = torch.utils.data.DataLoader(ds, batch_size=1, num_workers=1, multiprocessing_context='spawn', collate_fn=cvig_fov.collate_packed)
    batch = next(iter(loader))
    d = batch['surface_desc'].numpy()
    assert batch['surface_kind'] == jpeg.KIND_JPEG and d[0, 24] == 0 and list(d[0, 2:7]) == [24, 40, 3, 1, 2]


# ---- the host decoder as a stand-alone program under the sanitizers -----------------------------------------------------------------------

def test_host_decoder_with_the_440_geometry_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tools/jpeg_440_check.cpp + csrc_host/jpeg_coef.cpp, flags 3, file bytes / coefficients / tables / plan in heap blocks of exactly
    their size: the committed fixtures, a progressive twin, every truncation of the restart-marker fixture and 1,000 single-byte
    corruptions of it run through without a report. Nothing is loaded into Python."""
    gxx = shutil.which('g++')
    if not gxx:
        pytest.skip('no g++ on this box')
    exe = str(tmp_path / 'jpeg_440_check')
    build = subprocess.run([gxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                            '-static-libasan', '-static-libubsan', '-o', exe,
                            os.path.join(ROOT, 'witw_amd', 'csrc_host', 'jpeg_coef.cpp'), os.path.join(ROOT, 'tools', 'jpeg_440_check.cpp')],
                           capture_output=True, text=True)
    if build.returncode != 0:
        if 'asan' in build.stderr or 'ubsan' in build.stderr or 'sanitize' in build.stderr:
            pytest.skip('this compiler cannot link the sanitizer runtimes')
        raise AssertionError(build.stderr[-3000:])
    clean, damaged = [os.path.join(HERE, n + '.jpg') for n in FIXTURES], []

    def put(group, name, data):
        path = str(tmp_path / name)
        with open(path, 'wb') as f:
            f.write(data)
        group.append(path)

    exp = expected()
    put(clean, 'prog.jpg', C4.write_progressive(40, 48, exp['s440_q90_coef'], exp['s440_q90_qt'], PC.script_successive(3, al=2)))
    for name, _H, _W, data, _c, _q in CORPUS:
        if name.startswith(('9x17', '41x23')):
            put(clean, name + '.jpg', data)
    small = fixture('s440_rst')
    for n in range(len(small)):
        put(damaged, 'cut_%04d.jpg' % n, small[:n])
    g = np.random.Generator(np.random.Philox(key=[44, 1000]))
    for k in range(1000):
        b = bytearray(small)
        b[int(g.integers(0, len(b)))] = int(g.integers(0, 256))
        put(damaged, 'flip_%04d.jpg' % k, bytes(b))
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    p = subprocess.run([exe] + clean + damaged, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and 'Sanitizer' not in p.stderr and 'runtime error' not in p.stderr, (p.returncode, p.stderr[-3000:])
    lines = p.stdout.splitlines()
    assert len(lines) == len(clean) + len(damaged)
    assert all(ln.split()[:2] in (['0', '0'], ['1', '0']) for ln in lines[:len(clean)]), lines[:len(clean)]
    assert [ln.split()[2] != '-' for ln in lines[:3]] == [True, True, False]      # a plan for the sequential files, none for the progressive one
    cuts = lines[len(clean):len(clean) + len(small) - 2]      # (without its EOI marker alone the sequential file is whole)
    assert all(ln.split()[0] == '-1' or ln.split()[1] == '-3' for ln in cuts), [ln for ln in cuts if ln.split()[1] not in ('-', '-3')][:5]
    assert all(ln.split()[0] in ('-2', '-1', '0', '1') for ln in lines[len(clean):])
