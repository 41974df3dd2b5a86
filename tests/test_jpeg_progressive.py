"""Progressive JPEG files on the host-coefficient route (opt-in: jpeg.PROGRESSIVE / WITW_JPEG_PROGRESSIVE; csrc_host/jpeg_coef.cpp
witw_jpeg_info_ex / witw_jpeg_decode_coef_ex): the coefficient blocks of a progressive file are EXACTLY those of its sequential
twin -- on Pillow's files (libjpeg's default script) and on files written here under other scan scripts (tests/jpeg_prog_craft.py),
each of which Pillow must decode to the sequential file's pixels; incomplete, illegal and truncated files are refused; with the
flag off nothing changes. CPU only: tests/test_jpeg_progressive_gpu.py takes such files through the device back end."""
import ctypes
import io
import os

import numpy as np
import pytest

from witw_amd import jpeg

from . import jpeg_prog_craft as PC

SUBSAMPLING = {'grey': None, '444': 0, '422': 1, '420': 2}      # sampling name (tests/jpeg_craft.py) -> Pillow's save option


def picture(seed, h, w, grey=False):
    """photographic statistics (smooth + noise), as tests/golden/gen_jpeg_fixtures.py draws them"""
    from PIL import Image
    g = np.random.Generator(np.random.Philox(key=[31, seed]))
    small = g.integers(0, 256, size=(h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
    img = np.asarray(Image.fromarray(small).resize((w + 16, h + 16), Image.BICUBIC))[8:8 + h, 8:8 + w]
    a = np.clip(img.astype(np.int16) + g.integers(-20, 21, size=(h, w, 3)), 0, 255).astype(np.uint8)
    return a[:, :, 1] if grey else a


def save(a, sampling, quality, **kw):
    from PIL import Image
    bio = io.BytesIO()
    if SUBSAMPLING[sampling] is not None:
        kw['subsampling'] = SUBSAMPLING[sampling]
    Image.fromarray(a).save(bio, 'JPEG', quality=quality, **kw)
    return bio.getvalue()


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def decode_ex(data, flags=1):
    """the C entry points themselves -> (witw_jpeg_info_ex, witw_jpeg_decode_coef_ex or None, coef, qt)"""
    lib = jpeg.host_lib()
    d = np.frombuffer(data, dtype=np.uint8)
    info = np.zeros(22, dtype=np.int32)
    rc = lib.witw_jpeg_info_ex(d.ctypes.data, d.size, info.ctypes.data, flags)
    if rc < 0:
        return rc, None, None, None
    coef = np.full((int(info[5]), 64), 0x5555, dtype=np.int16)
    qt = np.zeros((int(info[2]), 64), dtype=np.uint16)
    return rc, lib.witw_jpeg_decode_coef_ex(d.ctypes.data, d.size, coef.ctypes.data, qt.ctypes.data, flags), coef, qt


def assert_twin(prog, seq_data):
    """the progressive file decodes to the sequential file's coefficients and tables, padding blocks included"""
    s = jpeg.read_coef(seq_data)
    p = jpeg.read_coef(prog, progressive=True)
    assert s is not None and p is not None
    np.testing.assert_array_equal(p.info, s.info)
    np.testing.assert_array_equal(p.qt, s.qt)
    np.testing.assert_array_equal(p.coef, s.coef)
    f = jpeg.open_file(prog, progressive=True)
    assert f.progressive and f.entropy_plan() is None and not jpeg.open_file(seq_data, progressive=True).progressive
    assert jpeg.read_coef(prog) is None and jpeg.open_file(prog) is None      # off by default


@pytest.mark.parametrize('quality', [50, 95])
@pytest.mark.parametrize('size', [(8, 8), (17, 9), (40, 56), (64, 64)])
@pytest.mark.parametrize('sampling', ['grey', '444', '422', '420'])
def test_progressive_file_gives_its_sequential_twins_coefficients(sampling, size, quality):
    """(40 x 56 at 4:2:0 leaves a column of MCU-padding blocks in Y, 17 x 9 a column and a row: only the interleaved DC scans reach them)"""
    a = picture(size[0] * 100 + size[1], size[0], size[1], grey=sampling == 'grey')
    prog, seq = save(a, sampling, quality, progressive=True), save(a, sampling, quality)
    assert b'\xff\xc2' in prog and len(PC.scans_of(prog)) >= 6
    assert_twin(prog, seq)
    np.testing.assert_array_equal(pillow(prog), pillow(seq))


@pytest.mark.parametrize('kw', [{'restart_marker_blocks': 3}, {'restart_marker_rows': 1}])
def test_progressive_twin_with_restart_markers(kw):
    """restart intervals count MCUs of the scan at hand: whole MCUs in the interleaved DC scans, single blocks of the component's own
    grid in the others; predictors and EOB runs start afresh behind every marker"""
    a = picture(7, 40, 56)
    try:
        prog, seq = save(a, '420', 85, progressive=True, **kw), save(a, '420', 85, **kw)
    except TypeError:
        pytest.skip('this Pillow does not write restart markers')
    if b'\xff\xdd' not in prog:
        pytest.skip('this Pillow does not write restart markers')
    assert any(b'\xff\xd0' in prog[s['start']:s['end']] for s in PC.scans_of(prog))
    assert_twin(prog, seq)


def source(sampling, h, w, quality=90, seed=1):
    """a sequential file and its coefficients: what the crafted progressive files are written from"""
    seq = save(picture(seed, h, w, grey=sampling == 'grey'), sampling, quality)
    return seq, jpeg.read_coef(seq)


def with_options(script, **kw):
    return [dict(s, **kw) for s in script]


def crafted_cases():
    cases = []
    for sampling in ('grey', '420', '444', '422'):
        n = 1 if sampling == 'grey' else 3
        cases += [('spectral_%s' % sampling, sampling, (40, 56), PC.script_spectral(n), {}),
                  ('successive_al3_%s' % sampling, sampling, (40, 56), PC.script_successive(n, al=3), {})]
    cases += [
        # every refinement construct at once: two bands, Al = 2, so correction bits fall inside zero runs, ZRLs and EOB runs
        ('successive_al2_bands_420', '420', (33, 49), PC.script_successive(3, al=2, bands=((1, 9), (10, 63))), {'quality': 97}),
        ('successive_low_quality', '444', (64, 64), PC.script_successive(3, al=1), {'quality': 15}),      # long EOB runs
        ('dc_separate_444', '444', (24, 40), PC.script_dc_separate(3), {}),
        ('dc_separate_420_padded', '420', (17, 9), PC.script_dc_separate(3), {}),      # padding blocks get no DC at all
        ('restart_in_every_scan', '420', (40, 56), with_options(PC.script_successive(3, al=2), dri=5), {}),
        ('restart_interval_changes', '422', (40, 56), [dict(s, dri=(0, 2, 7)[i % 3]) for i, s in enumerate(PC.script_successive(3, al=1))], {}),
        ('one_table_slot_redefined_per_scan', '444', (24, 40), with_options(PC.script_successive(3, al=1), slots=[0, 0, 0]), {}),
        ('slots_2_and_3', '420', (24, 40), [dict(s, slots=[(2, 3, 1)[c] for c in s['comps']]) for s in PC.script_spectral(3)], {}),
        ('codes_past_the_look_ahead', '420', (40, 56), with_options(PC.script_successive(3, al=2), min_len=12), {'quality': 95}),
    ]
    return cases


@pytest.mark.parametrize('name,sampling,size,script,kw', crafted_cases(), ids=[c[0] for c in crafted_cases()])
def test_crafted_scan_scripts(name, sampling, size, script, kw):
    """files written here under scripts Pillow never writes: Pillow reads each as the sequential file's pixels (so the stream is a
    legal one), and the decoder returns the coefficients the file was written from"""
    seq, src = source(sampling, size[0], size[1], **kw)
    prog = PC.write(size[0], size[1], src.coef, src.qt, sampling, script)
    np.testing.assert_array_equal(pillow(prog), pillow(seq))
    got = jpeg.read_coef(prog, progressive=True)
    assert got is not None
    np.testing.assert_array_equal(got.qt, src.qt)
    want = src.coef.copy()
    if name.startswith('dc_separate'):
        want[PC.padding_blocks(size[0], size[1], sampling), 0] = 0      # no single-component scan visits an MCU-padding block
        assert name != 'dc_separate_420_padded' or (want != src.coef).any()
    np.testing.assert_array_equal(got.coef, want)


def test_ac_band_split_at_every_position():
    seq, src = source('grey', 17, 9, quality=98)
    ref = pillow(seq)
    for k in range(1, 63):
        prog = PC.write(17, 9, src.coef, src.qt, 'grey', PC.script_successive(1, al=1, bands=((1, k), (k + 1, 63))))
        np.testing.assert_array_equal(pillow(prog), ref, err_msg=str(k))
        np.testing.assert_array_equal(jpeg.read_coef(prog, progressive=True).coef, src.coef, err_msg=str(k))


def flat_blocks_file():
    """264 x 264 grey, every 8 x 8 block flat: 1,089 blocks without one AC coefficient"""
    g = np.random.Generator(np.random.Philox(key=[31, 264]))
    a = g.integers(0, 256, size=(33, 33), dtype=np.uint8).repeat(8, 0).repeat(8, 1)
    seq = save(a, 'grey', 90)
    src = jpeg.read_coef(seq)
    assert not src.coef[:, 1:].any()
    return seq, src, PC.write(264, 264, src.coef, src.qt, 'grey', PC.script_successive(1, al=2))


def test_one_eob_run_over_more_than_1024_blocks():
    seq, src, prog = flat_blocks_file()
    ac = [s for s in PC.scans_of(prog) if s['ss']]
    assert len(ac) == 3 and all(s['end'] - s['start'] <= 4 for s in ac)      # EOB10 + 10 bits: the whole scan
    np.testing.assert_array_equal(pillow(prog), pillow(seq))
    np.testing.assert_array_equal(jpeg.read_coef(prog, progressive=True).coef, src.coef)


def test_eob_runs_of_the_greatest_length_and_across_restarts():
    """33,124 blocks with a handful of AC coefficients: EOB runs of 32,767 (the most one symbol can say) carried over block rows, a
    refinement scan whose runs carry correction bits, and the same with restart markers cutting the runs"""
    H = W = 1456
    g = np.random.Generator(np.random.Philox(key=[31, 1456]))
    coef = np.zeros((182 * 182, 64), dtype=np.int16)
    coef[:, 0] = g.integers(-100, 101, size=coef.shape[0])
    coef[[5, 20000, 33000, 33123], 1] = (3, -2, 1, 5)
    coef[33001, 9] = -1
    qt = np.full((1, 64), 2, dtype=np.uint16)
    for dri in (0, 40000 // 3):
        prog = PC.write(H, W, coef, qt, 'grey', with_options(PC.script_successive(1, al=1), dri=dri))
        if not dri:
            first_ac = [s for s in PC.scans_of(prog) if s['ss']][0]
            assert first_ac['end'] - first_ac['start'] < 40
        got = jpeg.read_coef(prog, progressive=True)
        np.testing.assert_array_equal(got.coef, coef)
    from PIL import Image
    assert Image.open(io.BytesIO(prog)).size == (W, H) and pillow(prog).shape == (H, W)      # (a legal stream for libjpeg too)


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_incomplete_file_is_left_to_the_host_decoder():
    """a file whose scans stop short of bit 0: libjpeg smooths it between blocks, its pixels are not those of the coefficients"""
    seq, src = source('420', 40, 56)
    script = PC.script_successive(3, al=2)
    whole = PC.write(40, 56, src.coef, src.qt, '420', script)
    assert decode_ex(whole)[:2] == (1, 0)
    for data in (PC.drop_last_scan(whole), PC.write(40, 56, src.coef, src.qt, '420', script, n_scans=len(script) - 3),
                 PC.write(40, 56, src.coef, src.qt, '420', script, n_scans=1)):
        assert pillow(data).shape == (40, 56, 3)                      # Pillow reads it
        rc_info, rc, _c, _q = decode_ex(data)
        assert (rc_info, rc) == (1, -2)
        assert jpeg.read_coef(data, progressive=True) is None
    # Pillow's own file without its last scan
    prog = save(picture(3, 40, 56), '420', 80, progressive=True)
    assert decode_ex(PC.drop_last_scan(prog))[:2] == (1, -2)


def patched(data, scan_index, ss=None, se=None, ahal=None):
    b, j = bytearray(data), PC.scans_of(data)[scan_index]['start']
    for off, v in ((3, ss), (2, se), (1, ahal)):
        if v is not None:
            b[j - off] = v
    return bytes(b)


def test_illegal_scan_parameters_are_refused():
    seq, src = source('444', 24, 40)
    S = PC.script_successive(3, al=2)      # scans: 0 DC first; 1-3 AC first; 4-6 AC refine 2->1; 7 DC refine; 8-10 AC refine; 11 DC refine
    good = PC.write(24, 40, src.coef, src.qt, '444', S)
    assert decode_ex(good)[:2] == (1, 0)
    ac = PC.scan
    bad = {
        'Ss > Se': patched(good, 1, ss=9, se=5),
        'Se > 63': patched(good, 1, se=64),
        'DC mixed with AC': patched(good, 0, se=5),
        'AC scan of three components': patched(good, 0, ss=1, se=63),
        'Al > 13': patched(good, 1, ahal=0x0e),
        'refinement of more than one bit': patched(good, 4, ahal=0x20),
        'Ah is not the Al before': patched(good, 4, ahal=0x32),
        'refinement of a band never coded': PC.write(24, 40, src.coef, src.qt, '444', S[:1] + S[4:5]),
        'AC before the DC of the component': PC.write(24, 40, src.coef, src.qt, '444', [ac([0], 1, 63, 0, 0)] + PC.script_spectral(3)),
        'band coded twice': PC.write(24, 40, src.coef, src.qt, '444', S[:2] + S[1:2] + S[2:]),
        'overlapping bands': PC.write(24, 40, src.coef, src.qt, '444', PC.script_spectral(3, bands=((1, 10), (8, 63)))),
    }
    for what, data in bad.items():
        rc_info, rc, _c, _q = decode_ex(data)
        assert (rc_info, rc) == (1, -3), what
        assert jpeg.read_coef(data, progressive=True) is None, what


def test_truncation_inside_every_kind_of_scan_is_refused():
    """Pillow's script holds all four kinds of scan. A file cut inside scan j: -3; coefficients only later scans bring are still zero,
    and so is the band of scan j in the last block it would have reached (the decode stops within a block of the damage)"""
    H, W = 64, 64
    prog = save(picture(5, H, W), '420', 90, progressive=True)
    scans = PC.scans_of(prog)
    kinds = set((s['ss'] == 0, s['ah'] == 0) for s in scans)
    assert len(kinds) == 4
    nblk = [64, 16, 16]
    first = np.cumsum([0] + nblk)
    for j, s in enumerate(scans):
        assert s['end'] - s['start'] >= 8
        for frac in (0.25, 0.5, 0.75):
            cut = s['start'] + int((s['end'] - s['start']) * frac)
            for tail in (b'', b'\xff\xd9'):
                rc_info, rc, coef, _q = decode_ex(prog[:cut] + tail)
                assert (rc_info, rc) == (1, -3), (j, frac, tail)
                assert not (coef == 0x5555).any()                                  # the whole area was zero-filled first
                for later in scans[j + 1:]:
                    if later['ah'] == 0:
                        for c in later['comps']:
                            assert not coef[first[c]:first[c + 1]][:, PC.ZZ[later['ss']:later['se'] + 1]].any(), (j, frac)
                if s['ah'] == 0:
                    last = PC.block_rows(H, W, '420', s['comps'])[-1][-1][1]
                    assert not coef[last, PC.ZZ[s['ss']:s['se'] + 1]].any(), (j, frac)


# ---- defaults, pack(), the flag's way into loader workers -------------------------------------------------------------------------

def test_off_by_default():
    prog = save(picture(2, 40, 56), '420', 85, progressive=True)
    assert jpeg.PROGRESSIVE is False or os.environ.get('WITW_JPEG_PROGRESSIVE')
    lib = jpeg.host_lib()
    d = np.frombuffer(prog, dtype=np.uint8)
    info = np.zeros(22, dtype=np.int32)
    assert lib.witw_jpeg_info(d.ctypes.data, d.size, info.ctypes.data) == -2
    assert decode_ex(prog, flags=0)[0] == -2                               # flags == 0: witw_jpeg_info
    coef, qt = np.zeros((96, 64), np.int16), np.zeros((3, 64), np.uint16)
    assert lib.witw_jpeg_decode_coef(d.ctypes.data, d.size, coef.ctypes.data, qt.ctypes.data) == -2
    assert lib.witw_jpeg_decode_coef_ex(d.ctypes.data, d.size, coef.ctypes.data, qt.ctypes.data, 0) == -2
    plan = np.zeros(4096, np.uint8)
    assert lib.witw_jpeg_entropy_plan_bytes(d.ctypes.data, d.size) == 0
    assert lib.witw_jpeg_entropy_plan(d.ctypes.data, d.size, plan.ctypes.data, ctypes.c_size_t(plan.size), qt.ctypes.data) == -2
    assert jpeg.open_file(prog, progressive=False) is None and jpeg.read_coef(prog, progressive=False) is None
    # a sequential file through the _ex entries: as through the plain ones
    seq = save(picture(2, 40, 56), '420', 85)
    rc_info, rc, coef, qt = decode_ex(seq)
    assert (rc_info, rc) == (0, 0)
    np.testing.assert_array_equal(coef, jpeg.read_coef(seq).coef)
    # progressive files this decoder does not take, flag or no flag: 4:4:0 sampling, RGB colour space
    b = bytearray(prog)
    b[b.index(b'\xff\xc2') + 4 + 6 + 1] = 0x12
    assert decode_ex(bytes(b))[0] == -2
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(picture(2, 40, 56)).save(bio, 'JPEG', quality=85, subsampling=0, keep_rgb=True, progressive=True)
    assert decode_ex(bio.getvalue())[0] == -2


def test_module_flag_is_the_default_of_the_keyword(monkeypatch):
    prog = save(picture(2, 40, 56), '420', 85, progressive=True)
    monkeypatch.setattr(jpeg, 'PROGRESSIVE', True)
    assert jpeg.open_file(prog).progressive and jpeg.read_coef(prog) is not None and jpeg.open_file(prog, progressive=False) is None


@pytest.mark.parametrize('device_entropy', ['all', 'restart', False])
def test_pack_sends_a_progressive_file_down_the_host_coefficient_route(monkeypatch, device_entropy):
    monkeypatch.setattr(jpeg, 'DEVICE_ENTROPY', device_entropy)
    monkeypatch.setattr(jpeg, 'PROGRESSIVE', True)
    a = picture(2, 40, 56)
    prog, seq = save(a, '420', 85, progressive=True), save(a, '420', 85, restart_marker_blocks=2)
    buf, desc, kind = jpeg.pack([jpeg.open_file(prog), jpeg.open_file(seq)])
    d = desc.numpy()
    assert kind == jpeg.KIND_JPEG and list(d[:, 24]) == [0, 0]                # neither is raw
    assert list(d[:, 26]) == [0, 1 if device_entropy else 0]                 # the progressive one: coefficient blocks from the host
    c = jpeg.read_coef(seq)
    np.testing.assert_array_equal(buf.numpy()[d[0, 0]:d[0, 0] + c.coef.size * 2].view(np.int16).reshape(-1, 64), c.coef)
    np.testing.assert_array_equal(buf.numpy()[d[0, 1]:d[0, 1] + c.qt.size * 2].view(np.uint16).reshape(-1, 64), c.qt)
    np.testing.assert_array_equal(d[0, 2:24], c.info)


def test_pack_hands_an_incomplete_progressive_file_to_pillow(monkeypatch):
    """the existing fallback: decode_into fails, Pillow's pixels ride in the file's span as a raw image"""
    seq, src = source('420', 40, 56)
    part = PC.write(40, 56, src.coef, src.qt, '420', PC.script_successive(3, al=2), n_scans=7)
    f = jpeg.open_file(part, progressive=True)
    assert f is not None and f.progressive
    buf, desc, _k = jpeg.pack([f, jpeg.open_file(seq)])
    d = desc.numpy()
    assert list(d[:, 24]) == [1, 0] and (int(d[0, 2]), int(d[0, 3]), int(d[0, 25])) == (40, 56, 3)
    np.testing.assert_array_equal(buf.numpy()[d[0, 0]:d[0, 0] + 40 * 56 * 3].reshape(40, 56, 3), pillow(part))


def _pairs_csv(tmp_path):
    from PIL import Image
    Image.fromarray(picture(8, 40, 56)).save(str(tmp_path / 'ov.jpg'), quality=88, progressive=True)
    Image.fromarray(picture(9, 24, 40)).save(str(tmp_path / 'su.jpg'), quality=88)
    (tmp_path / 'pairs.csv').write_text('ov.jpg,su.jpg\n')
    return str(tmp_path / 'pairs.csv')


def test_dataset_keyword_and_module_flag(tmp_path, monkeypatch):
    from witw_amd import cvig_fov
    csv = _pairs_csv(tmp_path)
    off = cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg')[0]
    assert isinstance(off['overhead'], np.ndarray) and isinstance(off['surface'], jpeg.JpegFile)
    on = cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg', jpeg_progressive=True)[0]
    assert on['overhead'].progressive and not on['surface'].progressive
    monkeypatch.setattr(jpeg, 'PROGRESSIVE', True)
    assert cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg')[0]['overhead'].progressive
    assert isinstance(cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg', jpeg_progressive=False)[0]['overhead'], np.ndarray)


def test_every_drivers_dataset_takes_the_keyword():
    """cvig_fov.train() / test() build `m.ImagePairDataset(..., jpeg_progressive=...)` for the module m they are run for"""
    import inspect
    from witw_amd import cvig_baseline, cvig_fov, cvig_semantic
    for m in (cvig_fov, cvig_semantic, cvig_baseline):
        assert 'jpeg_progressive' in inspect.signature(m.ImagePairDataset.__init__).parameters, m.__name__


@pytest.mark.parametrize('how', ['keyword', 'environment'])
def test_flag_reaches_spawned_loader_workers(tmp_path, monkeypatch, how):
    """a spawned worker imports witw_amd.jpeg afresh: it sees the keyword (pickled with the dataset) or WITW_JPEG_PROGRESSIVE
    (inherited), never the parent's module attribute; a forked worker inherits all three"""
    import torch
    from witw_amd import cvig_fov
    csv = _pairs_csv(tmp_path)
    if how == 'environment':
        monkeypatch.setenv('WITW_JPEG_PROGRESSIVE', '1')
    ds = cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg', jpeg_progressive=True if how == 'keyword' else None)
    loader = torch.utils.data.DataLoader(ds, batch_size=1, num_workers=1, multiprocessing_context='spawn', collate_fn=cvig_fov.collate_packed)
    batch = next(iter(loader))
    d = batch['overhead_desc'].numpy()
    assert batch['overhead_kind'] == jpeg.KIND_JPEG and list(d[0, 24:27]) == [0, 0, 0] and list(d[0, 2:5]) == [40, 56, 3]
