"""The host entropy decoder (csrc_host/jpeg_coef.cpp) on crafted baseline streams (tests/jpeg_craft.py): files whose coefficients the
test chose, down to what Pillow's encoder never writes (categories 12-15, 16-bit codes, blocks ending at coefficient 63 or on a ZRL
chain without EOB, fill bytes, > 16,384 restart intervals), and damaged ones. The written coefficients are the reference for the
entropy stage; Pillow (libjpeg, what the reference's imread uses) for the pixels. tests/test_jpeg_damage_gpu.py holds the device
decoders to the same files."""
import numpy as np
import pytest

from oracle import jpeg_oracle as J
from witw_amd import jpeg

from . import jpeg_craft as JC

pillow = JC.pillow


VALID = JC.valid_corpus()


@pytest.mark.parametrize('name', [n for n, _d, _c in VALID])
def test_crafted_file_decodes_to_the_written_coefficients(name):
    _n, data, coef = next(v for v in VALID if v[0] == name)
    r = jpeg.read_coef(data)
    assert r is not None
    np.testing.assert_array_equal(r.coef, coef)
    assert jpeg.open_file(data).entropy_plan() is not None          # the device path takes it
    if JC.in_range(r.info, r.coef, r.qt):
        np.testing.assert_array_equal(J.decode(r.info, r.coef, r.qt), pillow(data))


def test_valid_corpus_reaches_the_edges():
    names = [n for n, _d, _c in VALID]
    for s in JC.SAMPLINGS:
        for t in ('std', 'long'):
            for dri in (0, 3):
                assert any(n.startswith('%s_%s_dri%d' % (s, t, dri)) for n in names)
    long_files = [c for n, _d, c in VALID if '_long_' in n]
    cats = set(np.unique(np.abs(np.concatenate(long_files).astype(np.int64))).tolist())
    assert any(2 ** 11 <= v for v in cats) and any(2 ** 14 <= v for v in cats)        # AC categories 12 .. 15
    counts = JC.long_code_tables()['ac'][0][0]
    assert counts[15] > 0 and JC.long_code_tables()['dc'][0][0][15] > 0                   # 16-bit codes
    stuffed = next(d for n, d, _c in VALID if n == 'stuffed_grey_dri0')
    pos = [i for i in range(JC.scan_start(stuffed), len(stuffed) - 1) if stuffed[i] == 0xff and stuffed[i + 1] == 0]
    assert len(pos) > 1000 and set(p % 8 for p in pos) == set(range(8))                 # FF 00 at every offset of an 8-byte word
    fill = next(d for n, d, _c in VALID if n == 'ends63_zrl64_fill_444_dri2')
    assert b'\xff\xff\xff\xd0' in fill and fill.endswith(b'\xff\xff\xff\xff\xd9')
    staged, unstaged = JC.staging_sides(next(d for n, d, _c in VALID if n == 'staging_grey_dri1'))
    assert staged >= 1 and unstaged >= 1
    many = next(d for n, d, _c in VALID if n == 'many_intervals_grey_dri1')
    plan, _qt = jpeg.open_file(many).entropy_plan()
    assert int(plan[4:8].view(np.int32)[0]) > 16384
    blocks = {n: c.shape[0] for n, _d, c in VALID if n.startswith('blocks_')}
    assert sorted(blocks.values()) == [96, 96, 97, 194]
    assert jpeg.SELFSYNC_MIN_BLOCKS == 96


def _run_past_63(H=24, W=40, q63=16, value=120):
    g = np.random.Generator(np.random.Philox(key=[7, 63]))
    c = JC.random_coef(g, H, W, 'grey', density=0.1, amp=5, dc_amp=20)
    qt = JC.flat_qt(1, 2)
    qt[0, 63] = q63
    b = 4
    c[b, 1:] = 0
    c[b, JC.ZZ[60]] = 3            # last coefficient at zig-zag 60; then (15, size 7): position 76, the block's last symbol, no EOB
    data = JC.write(H, W, c, qt, 'grey', inject={b: {'post': [JC.ac(15, 7, value)], 'eob': False}})
    return data, c, qt, b


def test_damage_kinds_are_refused_by_the_host_decoder():
    g = np.random.Generator(np.random.Philox(key=[7, 64]))
    H, W = 40, 48
    c = JC.random_coef(g, H, W, '420', density=0.1, amp=30, dc_amp=100)
    qt = JC.flat_qt(3, 2)
    assert jpeg.read_coef(JC.write(H, W, c, qt, '420')) is not None
    assert jpeg.read_coef(_run_past_63()[0]) is None                                    # a run past coefficient 63
    inval = JC.write(H, W, c, qt, '420', inject={5: {'pre': [JC.raw_bits('1' * 16)]}})
    assert b'\xff\x00\xff\x00' in inval[JC.scan_start(inval):]                           # 16 one-bits: no code of the Annex K tables
    assert jpeg.read_coef(inval) is None
    full = JC.write(H, W, c, qt, '420')
    n = len(full) - JC.scan_start(full) - 2
    assert jpeg.read_coef(JC.write(H, W, c, qt, '420', truncate=n // 2)) is None         # a truncated scan
    assert jpeg.read_coef(JC.write(H, W, c, qt, '420', truncate=n - 3, eoi=False)) is None
    # DC category 16: the table is accepted (16 symbols fit the device plan), the symbol is not
    tb = JC.table_from_lengths(list(range(15)) + [16], [2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 12, 14, 16, 16])
    cg = JC.random_coef(g, H, W, 'grey', density=0.1, amp=30, dc_amp=100)
    dc16 = JC.write(H, W, cg, JC.flat_qt(1, 2), 'grey', tables={'dc': [tb, tb], 'ac': JC.long_code_tables()['ac']},
                    inject={10: {'pre': [JC.dc(16, 5)]}})
    assert jpeg.open_file(dc16).entropy_plan() is not None and jpeg.read_coef(dc16) is None
    # ... and with more than 16 DC symbols the parser keeps the file off the device path
    tb17 = JC.table_from_lengths(list(range(17)), [2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 12, 14, 16, 16, 16])
    dc17 = JC.write(H, W, cg, JC.flat_qt(1, 2), 'grey', tables={'dc': [tb17, tb17], 'ac': JC.long_code_tables()['ac']},
                    inject={10: {'pre': [JC.dc(16, 5)]}})
    assert jpeg.open_file(dc17).entropy_plan() is None and jpeg.read_coef(dc17) is None


def test_run_past_63_is_not_the_picture_of_the_stream_without_that_symbol():
    """libjpeg stores a coefficient whose run goes past 63 at coefficient 63 (its natural-order table has overflow entries): a decoder
    that drops the symbol without flagging the file returns pixels that are not the reference's"""
    data, c, qt, b = _run_past_63()
    info = jpeg.open_file(data).info
    ref = pillow(data)
    assert (J.decode(info, c, qt) != ref).sum() >= 32
    c63 = c.copy()
    c63[b, 63] = 120
    assert JC.in_range(info, c63, qt)
    np.testing.assert_array_equal(J.decode(info, c63, qt), ref)


def test_damage_corpus_holds_each_kind_and_pillow_reads_what_the_host_accepts():
    """the corpus of tests/test_jpeg_damage_gpu.py: every deterministic case is refused by the host decoder; wherever the host decoder
    accepts a damaged file its coefficients give Pillow's pixels (dequantised values in range) -- among them restart intervals whose
    symbols ran on into the next interval's bits, where libjpeg hits the RSTn marker and decodes zeros"""
    from PIL import ImageFile
    D = JC.damage_corpus()
    for name, data in D:
        if not name.startswith('random_'):
            assert jpeg.read_coef(data) is None, name
        it = jpeg.open_file(data)
        assert it is not None and (it.entropy_plan() is not None or name.startswith('trunc_dri')), name
    old = ImageFile.LOAD_TRUNCATED_IMAGES
    ImageFile.LOAD_TRUNCATED_IMAGES = True
    try:
        compared = 0
        for name, data in D:
            r = jpeg.read_coef(data)
            if r is not None and JC.in_range(r.info, r.coef, r.qt):
                np.testing.assert_array_equal(J.decode(r.info, r.coef, r.qt), pillow(data), err_msg=name)
                compared += 1
        assert compared >= 10
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = old
