"""Progressive files on the DEVICE route (opt-in: jpeg.PROGRESSIVE_DEVICE / WITW_JPEG_PROGRESSIVE_DEVICE), the part that needs no GPU:
the scan plan (csrc_host/jpeg_coef.cpp witw_jpeg_scan_plan_ex) and the HOST BUILD of the per-segment procedures the kernel runs
(csrc/jpeg_entropy.h prog_segment, driven by tools/jpeg_scan_check.cpp stage by stage, segments last first) against the host decoder
-- exact, on the clean corpus; under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program on the clean corpus, every
truncation and 2,000 corruptions of one small file; the plan's stages and refusals; and pack()'s routing.
tests/test_jpeg_scan_gpu.py takes the same files through the kernel."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from witw_amd import jpeg

from . import jpeg_prog_craft as PC
from . import jpeg_scan_corpus as SC
from .test_jpeg_progressive import picture, save, source

ROOT = SC.ROOT
SOURCES = [os.path.join(ROOT, 'witw_amd', 'csrc_host', 'jpeg_coef.cpp'), os.path.join(ROOT, 'tools', 'jpeg_scan_check.cpp')]


def _write(tmp_path, files):
    paths = []
    for name, data in files:
        paths.append(str(tmp_path / (name + '.jpg')))
        with open(paths[-1], 'wb') as f:
            f.write(data)
    return paths


def _run(exe, paths, env=None):
    """-> the program's lines as (info rc, plan, flag, host rc, equal) string tuples, in file order"""
    lines = []
    for i in range(0, len(paths), 500):
        p = subprocess.run([exe] + paths[i:i + 500], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and 'Sanitizer' not in p.stderr and 'runtime error' not in p.stderr, (p.returncode, p.stderr[-3000:])
        lines += [tuple(ln.split()[:5]) for ln in p.stdout.splitlines()]
    assert len(lines) == len(paths)
    return lines


def _assert_clean(lines, names):
    """every file has a plan, no flag, and the host decoder's coefficients and tables"""
    bad = [(n, ln) for n, ln in zip(names, lines) if not (ln[0] == '1' and int(ln[1]) > 0 and ln[2:] == ('0', '0', '='))]
    assert not bad, bad[:5]


def test_clean_corpus_host_build_of_the_segment_body_equals_the_host_decoder(tmp_path):
    """(a) fails before the feature: libwitw_jpeg.so has no witw_jpeg_scan_plan_ex"""
    gxx = shutil.which('g++')
    if not gxx:
        pytest.skip('no g++ on this box')
    exe = str(tmp_path / 'jpeg_scan_check')
    subprocess.run([gxx, '-O2', '-std=c++17', '-o', exe] + SOURCES, check=True, capture_output=True)
    corpus = SC.clean_corpus() + [('segments_400', SC.segments_400())]
    _assert_clean(_run(exe, _write(tmp_path, corpus)), [n for n, _d in corpus])


def test_segment_body_and_plan_writer_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """(b) the same program with the sanitizer runtimes linked statically: file (+ 24 bytes), plan and coefficient area are heap blocks
    of exactly their size. No report on any file; a damaged file has no plan, or is flagged, or holds the coefficients of a host decode
    that returned 0 (so: flagged wherever the host decoder says -3)."""
    gxx = shutil.which('g++')
    if not gxx:
        pytest.skip('no g++ on this box')
    exe = str(tmp_path / 'jpeg_scan_check_san')
    build = subprocess.run([gxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                            '-static-libasan', '-static-libubsan', '-o', exe] + SOURCES, capture_output=True, text=True)
    if build.returncode != 0:
        if 'asan' in build.stderr or 'ubsan' in build.stderr or 'sanitize' in build.stderr:
            pytest.skip('this compiler cannot link the sanitizer runtimes')
        raise AssertionError(build.stderr[-3000:])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    clean = SC.clean_corpus()
    damaged = SC.truncations() + SC.corruptions()
    assert len(damaged) == len(SC.small_file()) + 2000
    lines = _run(exe, _write(tmp_path, clean + damaged), env)
    _assert_clean(lines[:len(clean)], [n for n, _d in clean])
    planned = flagged = 0
    for (name, _d), ln in zip(damaged, lines[len(clean):]):
        if ln[1] == '-' or int(ln[1]) <= 0:
            continue                                       # no plan: the file takes the host route
        planned += 1
        flagged += ln[2] != '0'
        assert ln[2] != '0' or ln[3:] == ('0', '='), (name, ln)
    assert planned >= 200 and flagged >= 50, (planned, flagged)      # neither alternative is met vacuously


# ---- (c) the plan -----------------------------------------------------------------------------------------------------------------

def _shares_a_cell(a, b):
    return bool(set(a['comps']) & set(b['comps'])) and a['ss'] <= b['se'] and b['ss'] <= a['se']


def test_stages_of_the_standard_script_and_of_every_clean_file():
    prog = save(picture(5, 64, 64), '420', 90, progressive=True)
    scans = SC.plan_scans(SC.scan_plan(prog))
    assert len(scans) == 10
    assert {st: sum(1 for s in scans if s['stage'] == st) for st in set(s['stage'] for s in scans)} == {0: 5, 1: 4, 2: 1}
    L = SC.layout()
    for name, data in SC.clean_corpus():
        plan = SC.scan_plan(data)
        assert plan is not None, name
        scans = SC.plan_scans(plan)
        h = plan[:128].view(np.int32)
        assert int(h[L['PLAN_PROG_STAGES']]) == 1 + max(s['stage'] for s in scans) <= L['PLAN_PROG_MAX_STAGES']
        assert int(h[L['PLAN_PROG_MAX_SEGMENTS']]) == max(s['segs'] for s in scans) and int(h[L['PLAN_PROG_SEGMENTS']]) == sum(s['segs'] for s in scans)
        in_file = PC.scans_of(data)
        assert [(s['comps'], s['ss'], s['se'], s['ah'], s['al']) for s in scans] == \
            [(tuple(s['comps']), s['ss'], s['se'], s['ah'], s['al']) for s in in_file], name
        for j, s in enumerate(scans):
            # the stage rule: 0 when no earlier scan coded one of its cells, else 1 + the largest stage among those that did
            earlier = [e['stage'] for e in scans[:j] if _shares_a_cell(e, s)]
            assert s['stage'] == (1 + max(earlier) if earlier else 0), (name, j)
            # the segments tile the walk; the first starts behind the SOS header, the scan's data ends where scans_of finds its end
            units = s['cols'] * s['rows']
            assert [u for _b, u, _n in s['segments']] == list(range(0, units, s['restart'] or units)), (name, j)
            assert sum(n for _b, _u, n in s['segments']) == units and s['segments'][0][0] == in_file[j]['start']
            assert s['data_end'] == in_file[j]['end']


def test_plan_of_the_restart_file_has_a_segment_per_block():
    scans = SC.plan_scans(SC.scan_plan(SC.segments_400()))
    assert all(s['segs'] == 400 and s['restart'] == 1 for s in scans)


def _grey_one_coefficient_bands(extra):
    _seq, src = source('grey', 17, 9, quality=98)
    script = [PC.scan([0], 0, 0, 0, 0)] + [PC.scan([0], k, k, 0, 1 if extra else 0) for k in range(1, 64)]
    if extra:
        script.append(PC.scan([0], 1, 63, 1, 0))
    return PC.write(17, 9, src.coef, src.qt, 'grey', script), src


def _plan_rc(data, flags=1):
    lib = jpeg.host_lib()
    d = np.frombuffer(data, dtype=np.uint8)
    plan, qt = np.zeros(1 << 16, np.uint8), np.zeros((3, 64), np.uint16)
    return (int(lib.witw_jpeg_scan_plan_bytes_ex(d.ctypes.data, d.size, flags)),
            int(lib.witw_jpeg_scan_plan_ex(d.ctypes.data, d.size, plan.ctypes.data, ctypes.c_size_t(plan.size), qt.ctypes.data, flags)))


def test_a_file_of_65_scans_gets_no_plan_one_of_64_does():
    ok, src = _grey_one_coefficient_bands(False)
    assert len(PC.scans_of(ok)) == 64 and SC.host_decode(ok)[1] == 0
    assert len(SC.plan_scans(SC.scan_plan(ok))) == 64
    many, _src = _grey_one_coefficient_bands(True)
    assert len(PC.scans_of(many)) == 65
    rc, hrc, coef = SC.host_decode(many)
    assert (rc, hrc) == (1, 0)                                 # a legal, complete file: the host route decodes it
    np.testing.assert_array_equal(coef, src.coef)
    assert _plan_rc(many) == (0, -2) and SC.scan_plan(many) is None


def test_incomplete_and_sequential_files_get_no_plan():
    seq, src = source('420', 40, 56)
    part = PC.write(40, 56, src.coef, src.qt, '420', PC.script_successive(3, al=2), n_scans=7)
    assert SC.host_decode(part)[:2] == (1, -2)
    assert _plan_rc(part) == (0, -2) and SC.scan_plan(part) is None
    assert _plan_rc(seq) == (0, -2)
    f = jpeg.open_file(seq, progressive='device')
    assert f is not None and not f.progressive and not f.device_scans and f.scan_plan() is None and f.entropy_plan() is not None
    # and the entropy-plan entries still refuse a progressive file
    whole = PC.write(40, 56, src.coef, src.qt, '420', PC.script_successive(3, al=2))
    g = jpeg.open_file(whole, progressive='device')
    assert g.progressive and g.device_scans and g.entropy_plan() is None and g.scan_plan() is not None
    d = np.frombuffer(whole, dtype=np.uint8)
    assert jpeg.host_lib().witw_jpeg_entropy_plan_bytes_ex(d.ctypes.data, d.size, 1) == 0
    assert _plan_rc(b'\xff\xd8\xff\xd9') == (0, -1)


def _patched(data, scan_index, ss=None, se=None, ahal=None):
    b, j = bytearray(data), PC.scans_of(data)[scan_index]['start']
    for off, v in ((3, ss), (2, se), (1, ahal)):
        if v is not None:
            b[j - off] = v
    return bytes(b)


def test_illegal_scan_parameters_get_no_plan():
    """the cases of tests/test_jpeg_progressive.py test_illegal_scan_parameters_are_refused: -3, as witw_jpeg_decode_coef_ex says"""
    seq, src = source('444', 24, 40)
    S = PC.script_successive(3, al=2)
    good = PC.write(24, 40, src.coef, src.qt, '444', S)
    assert _plan_rc(good)[0] > 0 and _plan_rc(good)[0] == _plan_rc(good)[1]
    bad = {
        'Ss > Se': _patched(good, 1, ss=9, se=5),
        'Se > 63': _patched(good, 1, se=64),
        'DC mixed with AC': _patched(good, 0, se=5),
        'AC scan of three components': _patched(good, 0, ss=1, se=63),
        'Al > 13': _patched(good, 1, ahal=0x0e),
        'refinement of more than one bit': _patched(good, 4, ahal=0x20),
        'Ah is not the Al before': _patched(good, 4, ahal=0x32),
        'refinement of a band never coded': PC.write(24, 40, src.coef, src.qt, '444', S[:1] + S[4:5]),
        'AC before the DC of the component': PC.write(24, 40, src.coef, src.qt, '444', [PC.scan([0], 1, 63, 0, 0)] + PC.script_spectral(3)),
        'band coded twice': PC.write(24, 40, src.coef, src.qt, '444', S[:2] + S[1:2] + S[2:]),
        'overlapping bands': PC.write(24, 40, src.coef, src.qt, '444', PC.script_spectral(3, bands=((1, 10), (8, 63)))),
    }
    for what, data in bad.items():
        assert SC.host_decode(data)[:2] == (1, -3), what
        assert _plan_rc(data) == (0, -3), what
        assert SC.scan_plan(data) is None, what


def test_restart_markers_out_of_sequence_or_missing_get_no_plan():
    _seq, src = source('420', 40, 56)
    good = PC.write(40, 56, src.coef, src.qt, '420', SC.with_options(PC.script_successive(3, al=1), dri=5))
    assert _plan_rc(good)[1] > 0
    b = bytearray(good)
    at = good.index(b'\xff\xd1', PC.scans_of(good)[1]['start'])
    b[at + 1] = 0xd3                                           # RST1 -> RST3
    assert _plan_rc(bytes(b)) == (0, -3) and SC.host_decode(bytes(b))[1] == -3
    assert _plan_rc(good[:at] + good[at + 2:]) == (0, -3)      # a marker dropped
    assert _plan_rc(good[:-2]) == (0, -3)                      # no EOI


# ---- (d) routing ------------------------------------------------------------------------------------------------------------------

def _pair():
    a = picture(2, 40, 56)
    return save(a, '420', 85, progressive=True), save(a, '420', 85, restart_marker_blocks=2)


def test_off_by_default_and_pack_is_unchanged_with_the_flag_off(monkeypatch):
    prog, seq = _pair()
    assert jpeg.PROGRESSIVE_DEVICE is False or os.environ.get('WITW_JPEG_PROGRESSIVE_DEVICE')
    monkeypatch.setattr(jpeg, 'PROGRESSIVE_DEVICE', False)
    monkeypatch.setattr(jpeg, 'PROGRESSIVE', False)
    assert jpeg.open_file(prog) is None
    monkeypatch.setattr(jpeg, 'PROGRESSIVE', True)
    monkeypatch.setattr(jpeg, 'DEVICE_ENTROPY', 'all')
    f = jpeg.open_file(prog)
    assert f.progressive and not f.device_scans
    buf, desc, _k = jpeg.pack([f, jpeg.open_file(seq)])
    # today's bytes: the host-coefficient entry a JpegCoef of the same file makes, and the sequential file beside it on the device route
    want, wdesc, _k = jpeg.pack([jpeg.read_coef(prog), jpeg.open_file(seq)])
    assert _same_block(buf, desc, want, wdesc)
    assert list(desc.numpy()[:, jpeg.COL_ON_DEVICE]) == [0, 1]
    # progressive=True pins the host route under the module flag too
    monkeypatch.setattr(jpeg, 'PROGRESSIVE_DEVICE', True)
    buf2, desc2, _k = jpeg.pack([jpeg.open_file(prog, progressive=True), jpeg.open_file(seq)])
    assert _same_block(buf2, desc2, want, wdesc)


def _same_block(buf, desc, want, wdesc):
    """the same descriptor and, byte for byte, the same entries, tables and plans (the padding between them is never written)"""
    d, a, b = desc.numpy(), buf.numpy(), want.numpy()
    if a.size != b.size or not np.array_equal(d, wdesc.numpy()):
        return False
    for r in d:
        ncomp, on_dev = int(r[jpeg.COL_INFO + jpeg.INFO_NCOMP]), int(r[jpeg.COL_ON_DEVICE])
        spans = [(int(r[jpeg.COL_OFFSET]), int(r[jpeg.COL_FILE_LEN]) + 24 if on_dev else int(r[jpeg.COL_INFO + jpeg.INFO_BLOCKS]) * 128),
                 (int(r[jpeg.COL_QT]), ncomp * 128)]
        if on_dev:                                             # (a sequential file's entropy plan: PLAN_FIXED + 4 bytes per interval)
            assert on_dev == 1
            spans.append((int(r[jpeg.COL_PLAN]), SC.layout()['PLAN_FIXED'] + 4 * int(r[jpeg.COL_INTERVALS])))
        if any(not np.array_equal(a[o:o + n], b[o:o + n]) for o, n in spans):
            return False
    return True


@pytest.mark.parametrize('device_entropy', ['all', 'restart', False])
def test_pack_sends_a_planned_progressive_file_to_the_device(monkeypatch, device_entropy):
    monkeypatch.setattr(jpeg, 'DEVICE_ENTROPY', device_entropy)
    monkeypatch.setattr(jpeg, 'PROGRESSIVE_DEVICE', True)
    prog, seq = _pair()
    f = jpeg.open_file(prog)                                   # the module flag: implies taking progressive files
    assert f is not None and f.progressive and f.device_scans and isinstance(jpeg.PROGRESSIVE, bool)
    buf, desc, kind = jpeg.pack([f, jpeg.open_file(seq)])
    d, b = desc.numpy(), buf.numpy()
    assert kind == jpeg.KIND_JPEG and d.shape[1] == jpeg.DESC_COLS == 30 and list(d[:, jpeg.COL_RAW]) == [0, 0]
    c = jpeg.read_coef(seq)
    np.testing.assert_array_equal(d[0, jpeg.COL_INFO:jpeg.COL_RAW], c.info)
    np.testing.assert_array_equal(b[d[0, jpeg.COL_QT]:d[0, jpeg.COL_QT] + c.qt.size * 2].view(np.uint16).reshape(-1, 64), c.qt)
    if not device_entropy:
        assert list(d[:, jpeg.COL_ON_DEVICE]) == [0, 0]       # the host route, as before
        np.testing.assert_array_equal(b[d[0, 0]:d[0, 0] + c.coef.size * 2].view(np.int16).reshape(-1, 64), c.coef)
        return
    assert list(d[:, jpeg.COL_ON_DEVICE]) == [2, 1]
    plan, _qt = f.scan_plan()
    n = len(prog)
    assert d[0, jpeg.COL_FILE_LEN] == n and d[0, jpeg.COL_OFFSET] % 128 == 0 and d[0, jpeg.COL_PLAN] % 16 == 0
    assert bytes(b[d[0, 0]:d[0, 0] + n]) == prog and not b[d[0, 0] + n:d[0, 0] + n + 24].any()
    np.testing.assert_array_equal(b[d[0, jpeg.COL_PLAN]:d[0, jpeg.COL_PLAN] + plan.size], plan)
    scans = SC.plan_scans(plan)
    sizes = int(d[0, jpeg.COL_INTERVALS])
    assert (sizes & 0xffffffff, (sizes >> 32) & 0xff, sizes >> 40) == (max(s['segs'] for s in scans), 10, 3)
    assert d[1, jpeg.COL_INTERVALS] == jpeg.plan_intervals(jpeg.open_file(seq).entropy_plan()[0])      # other entries: untouched


def test_a_file_without_a_plan_takes_the_host_route_under_the_flag(monkeypatch):
    monkeypatch.setattr(jpeg, 'DEVICE_ENTROPY', 'all')
    many, src = _grey_one_coefficient_bands(True)
    f = jpeg.open_file(many, progressive='device')
    assert f.device_scans and f.scan_plan() is None
    buf, desc, _k = jpeg.pack([f])
    d = desc.numpy()
    assert list(d[0, [jpeg.COL_RAW, jpeg.COL_ON_DEVICE]]) == [0, 0]
    np.testing.assert_array_equal(buf.numpy()[d[0, 0]:d[0, 0] + src.coef.size * 2].view(np.int16).reshape(-1, 64), src.coef)
    # an incomplete one: host decode refuses it, Pillow's pixels ride in its span
    _seq, s2 = source('420', 40, 56)
    part = PC.write(40, 56, s2.coef, s2.qt, '420', PC.script_successive(3, al=2), n_scans=7)
    _b, desc, _k = jpeg.pack([jpeg.open_file(part, progressive='device')])
    assert list(desc.numpy()[0, [jpeg.COL_RAW, jpeg.COL_ON_DEVICE]]) == [1, 0]


def test_new_plan_names_of_jpeg_py_are_those_of_the_header():
    L = SC.layout()
    names = ['PLAN_PROG_MAGIC', 'PLAN_PROG_SCANS', 'PLAN_PROG_SEGMENTS', 'PLAN_PROG_STAGES', 'PLAN_PROG_MAX_SEGMENTS', 'PLAN_PROG_BLOCKS',
             'PLAN_PROG_BYTES', 'PLAN_PROG_MAX_SCANS', 'PLAN_PROG_MAX_STAGES']
    for n in names:
        assert getattr(jpeg, n) == L[n], n
    assert L['PLAN_PROG_MAGIC'] != L['PLAN_MAGIC'] and L['PLAN_PROG_MAX_SCANS'] == 64
    assert L['PLAN_PROG_FIXED'] == L['PLAN_PROG_SCAN_AT'] + 4 * L['PLAN_PROG_SCAN_INTS'] * L['PLAN_PROG_MAX_SCANS']
    assert jpeg.COL_INTERVALS + 1 == jpeg.DESC_COLS


def test_environment_variable_sets_the_module_flag():
    code = 'from witw_amd import jpeg; print(jpeg.PROGRESSIVE_DEVICE, jpeg.PROGRESSIVE)'
    for value, want in (('1', 'True False'), ('on', 'True False'), ('', 'False False')):
        env = dict(os.environ, WITW_JPEG_PROGRESSIVE_DEVICE=value, PYTHONPATH=ROOT)
        env.pop('WITW_JPEG_PROGRESSIVE', None)
        assert subprocess.check_output([sys.executable, '-c', code], env=env, text=True).split('\n')[-2] == want


def _pairs_csv(tmp_path):
    from PIL import Image
    Image.fromarray(picture(8, 40, 56)).save(str(tmp_path / 'ov.jpg'), quality=88, progressive=True)
    Image.fromarray(picture(9, 24, 40)).save(str(tmp_path / 'su.jpg'), quality=88)
    (tmp_path / 'pairs.csv').write_text('ov.jpg,su.jpg\n')
    return str(tmp_path / 'pairs.csv')


def test_dataset_keyword(tmp_path, monkeypatch):
    from witw_amd import cvig_fov
    csv = _pairs_csv(tmp_path)
    on = cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg', jpeg_progressive='device')[0]
    assert on['overhead'].progressive and on['overhead'].device_scans and not on['surface'].device_scans
    assert not cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg', jpeg_progressive=True)[0]['overhead'].device_scans
    monkeypatch.setattr(jpeg, 'PROGRESSIVE_DEVICE', True)
    assert cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg')[0]['overhead'].device_scans


def test_keyword_reaches_a_spawned_loader_worker(tmp_path):
    """a spawned worker imports witw_amd.jpeg afresh: the keyword travels pickled with the dataset"""
    import torch
    from witw_amd import cvig_fov
    csv = _pairs_csv(tmp_path)
    ds = cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg', jpeg_progressive='device')
    loader = torch.utils.data.DataLoader(ds, batch_size=1, num_workers=1, multiprocessing_context='spawn', collate_fn=cvig_fov.collate_packed)
    batch = next(iter(loader))
    d = batch['overhead_desc'].numpy()
    assert batch['overhead_kind'] == jpeg.KIND_JPEG and list(d[0, 24:27]) == [0, 0, 2] and list(d[0, 2:5]) == [40, 56, 3]
