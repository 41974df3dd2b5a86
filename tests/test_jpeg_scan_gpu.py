"""Progressive files decoded ON THE DEVICE (csrc/jpeg_progressive.hip through witw_jpeg_progressive_stage; opt-in,
jpeg.PROGRESSIVE_DEVICE): the clean corpus of tests/test_jpeg_scan_plan.py on the bare kernel, bit for bit the host decoder's
coefficients; a mixed batch and the data path through jpeg.decode / GpuPreprocess, byte for byte Pillow's; damaged streams -- only ones
the host build of the same code has run clean under the sanitizers -- flagged or decoded as the host decodes them.
Order: (e) clean corpus, (f) mixed batch, (g) damage -- run only when (e) and (f) passed --, (h) data path."""
import numpy as np
import pytest
import torch

from witw_amd import jpeg

from . import jpeg_prog_craft as PC
from . import jpeg_scan_corpus as SC
from .test_jpeg_progressive import picture, pillow, save, source

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
PASSED = set()


def _launch(files):
    """the stage launches over `files` (bytes, each with a scan plan), straight through the C ABI -> (coef int16 [blocks, 64] per file,
    error flag per file, stages launched)"""
    from witw_amd import _lib, ops
    items = [jpeg.open_file(f, progressive='device') for f in files]
    plans = [it.scan_plan()[0] for it in items]
    blocks = np.array([int(it.info[jpeg.INFO_BLOCKS]) for it in items], dtype=np.int64)
    first = np.cumsum(blocks) - blocks
    coef = torch.zeros((int(blocks.sum()), 64), dtype=torch.int16, device=DEV)
    keep, rows = [], []
    for it, plan, f0 in zip(items, plans, first):
        raw = np.zeros((it.data.size + 24 + 7) // 8 * 8, dtype=np.uint8)       # 24 readable bytes behind the end, as pack() leaves
        raw[:it.data.size] = it.data
        rb, pb = torch.from_numpy(raw).to(DEV), torch.from_numpy(plan.copy()).to(DEV)
        keep += [rb, pb]
        rows.append((rb.data_ptr(), pb.data_ptr(), coef.data_ptr() + int(f0) * 128, it.data.size))
    errors = torch.zeros((len(items),), dtype=torch.int32, device=DEV)
    files_t = torch.tensor(rows, dtype=torch.int64, device=DEV)
    sizes = [jpeg.prog_launch_sizes(p) for p in plans]
    segs, scans, stages = max(s & 0xffffffff for s in sizes), max((s >> 32) & 0xff for s in sizes), max(s >> 40 for s in sizes)
    lib = _lib.load()
    for stage in range(stages):
        _lib.check(lib.witw_jpeg_progressive_stage(files_t.data_ptr(), len(items), stage, scans, segs, errors.data_ptr(), ops._stream()),
                   'witw_jpeg_progressive_stage')
    torch.cuda.synchronize()
    got = coef.cpu().numpy()
    return [got[f0:f0 + nb] for f0, nb in zip(first, blocks)], errors.cpu().numpy(), stages


def _assert_host_coefficients(named):
    got, err, stages = _launch([d for _n, d in named])
    for (name, data), c, e in zip(named, got, err):
        rc, hrc, want = SC.host_decode(data)
        assert (rc, hrc) == (1, 0), name
        assert e == 0, (name, int(e))
        bad = np.nonzero((c != want).any(axis=1))[0]
        assert bad.size == 0, '%s: %d of %d blocks differ, first %s' % (name, bad.size, want.shape[0], bad[:5])
    return stages


def test_clean_corpus_on_the_kernel_equals_the_host_decoder():
    """(e) every file of the CPU corpus in ONE set of launches; 400 segments per scan (more than a workgroup: the loop over segments
    and the grid's third dimension); a batch of files of 1, 3 and 4 stages"""
    _assert_host_coefficients(SC.clean_corpus())
    big = SC.segments_400()
    assert all(s['segs'] == 400 for s in SC.plan_scans(SC.scan_plan(big)))
    _assert_host_coefficients([('segments_400', big)])
    _seq, src = source('420', 40, 56)
    mixed = [('one_stage', PC.write(40, 56, src.coef, src.qt, '420', PC.script_spectral(3))),
             ('three_stages', save(picture(5, 64, 64), '420', 90, progressive=True)),
             ('four_stages', PC.write(40, 56, src.coef, src.qt, '420', PC.script_successive(3, al=3)))]
    assert [1 + max(s['stage'] for s in SC.plan_scans(SC.scan_plan(d))) for _n, d in mixed] == [1, 3, 4]
    assert _assert_host_coefficients(mixed) == 4
    PASSED.add('e')


def _grey_65_scans():
    _seq, src = source('grey', 17, 9, quality=98)
    script = [PC.scan([0], 0, 0, 0, 0)] + [PC.scan([0], k, k, 0, 1) for k in range(1, 64)] + [PC.scan([0], 1, 63, 1, 0)]
    return PC.write(17, 9, src.coef, src.qt, 'grey', script)


def test_mixed_batch_through_decode_equals_pillow(monkeypatch):
    """(f) progressive files on the device route, sequential files with and without restart markers, a raw array and a file of 65
    scans (host route) in one batch"""
    monkeypatch.setattr(jpeg, 'PROGRESSIVE_DEVICE', True)
    assert jpeg.DEVICE_ENTROPY == 'all'
    del jpeg._ERRORS[:]
    g = np.random.Generator(np.random.Philox(key=[33, 1]))
    seq, src = source('420', 33, 49, quality=97)
    raws = [save(picture(1, 40, 56), '420', 90, progressive=True), save(picture(2, 17, 9, grey=True), 'grey', 85, progressive=True),
            save(picture(3, 64, 64), '444', 75, progressive=True), save(picture(4, 97, 131), '422', 80),
            save(picture(6, 40, 56), '420', 85, restart_marker_blocks=2),
            g.integers(0, 256, size=(7, 9, 3), dtype=np.uint8),
            _grey_65_scans(),
            PC.write(33, 49, src.coef, src.qt, '420', SC.with_options(PC.script_successive(3, al=2, bands=((1, 9), (10, 63))), dri=3))]
    items = [r if isinstance(r, np.ndarray) else jpeg.open_file(r) for r in raws]
    _buf, desc, _k = jpeg.pack(items)
    d = desc.numpy()
    assert list(d[:, jpeg.COL_RAW]) == [0, 0, 0, 0, 0, 1, 0, 0]
    assert list(d[:, jpeg.COL_ON_DEVICE]) == [2, 2, 2, 1, 1, 0, 0, 2]
    out = jpeg.decode(items, DEV)
    for k, (o, r) in enumerate(zip(out, raws)):
        ref = r if isinstance(r, np.ndarray) else pillow(r)
        np.testing.assert_array_equal(o.cpu().numpy(), ref if ref.ndim == 3 else ref[:, :, None], err_msg=str(k))
    np.testing.assert_array_equal(out[7].cpu().numpy(), pillow(seq))
    assert jpeg.entropy_errors() == 0
    PASSED.add('f')


def _damaged_streams():
    """truncations of the small file at 16 cut points, four evenly spaced inside a scan of each of the four kinds, and the first 64
    of its corruptions that still have a scan plan -- all of them among the streams the sanitizer run of the CPU test covers"""
    small = SC.small_file()
    kinds = {}
    for s in PC.scans_of(small):
        kinds.setdefault((s['ss'] == 0, s['ah'] == 0), s)
    assert len(kinds) == 4
    cuts = [small[:s['start'] + (s['end'] - s['start']) * (j + 1) // 5] for s in kinds.values() for j in range(4)]
    all_cuts = set(d for _n, d in SC.truncations())
    assert len(cuts) == 16 and all(c in all_cuts for c in cuts)
    flips = [d for _n, d in SC.corruptions() if SC.scan_plan(d) is not None][:64]
    assert len(flips) == 64
    return cuts, flips


def test_damaged_streams_are_flagged_or_decoded_as_the_host_decodes_them(monkeypatch):
    """(g) through jpeg.decode with the host block present: Pillow's reading of every file. On the bare kernel: flagged wherever the
    host decoder returns -3, and an unflagged file has the host decoder's coefficients. (A prefix of a file has no EOI, so no
    truncation has a scan plan: the sixteen cuts take the host route and Pillow; the bare kernel sees the 64 corruptions, 29 of
    which the host decoder refuses.)"""
    if not {'e', 'f'} <= PASSED:
        pytest.fail('not run: the clean-corpus and mixed-batch tests of this module have to pass first')
    from .test_jpeg_damage_gpu import pipeline_check
    monkeypatch.setattr(jpeg, 'PROGRESSIVE_DEVICE', True)
    cuts, flips = _damaged_streams()
    planned = [d for d in cuts + flips if SC.scan_plan(d) is not None]
    got, err, _stages = _launch(planned)
    refused = 0
    for k, (data, c, e) in enumerate(zip(planned, got, err)):
        _rc, hrc, want = SC.host_decode(data)
        if hrc != 0:
            refused += 1
            assert e != 0, 'stream %d is refused by the host decoder (%d) but not flagged' % (k, hrc)
        if e == 0:
            np.testing.assert_array_equal(c, want, err_msg='stream %d unflagged' % k)
    assert refused >= 8, refused                               # the invariant is not met vacuously
    _repaired, n_ok, n_refused = pipeline_check(cuts + flips, monkeypatch)
    assert n_ok + n_refused == 80 and n_ok >= 60


def test_data_path_on_the_device_route_equals_host_decode(tmp_path):
    """(h) ImagePairDataset(raw='jpeg', jpeg_progressive='device') through one loader worker and GpuPreprocess: the twin of
    tests/test_jpeg_progressive_gpu.py test_data_path_with_progressive_files_equals_host_decode"""
    import os
    from PIL import Image
    from witw_amd import cvig_fov
    root, rows = str(tmp_path), []
    for i, ((hs, ws), (ho, wo)) in enumerate([((48, 80), (64, 64)), ((100, 133), (120, 90))]):
        for tag, (h, w) in (('su', (hs, ws)), ('ov', (ho, wo))):
            Image.fromarray(picture(40 + i, h, w)).save(os.path.join(root, '%s_%d.jpg' % (tag, i)), quality=88, progressive=(tag == 'ov' or i == 1))
        rows.append('ov_%d.jpg,su_%d.jpg' % (i, i))
    csv = os.path.join(root, 'pairs.csv')
    open(csv, 'w').write('\n'.join(rows) + '\n')
    prep = cvig_fov.GpuPreprocess('cvusa', fov=360, random_orientation=False)
    ref = prep(cvig_fov.collate_packed([cvig_fov.ImagePairDataset('cvusa', csv, raw=True)[i] for i in range(2)]))
    ds = cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg', jpeg_progressive='device')
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, num_workers=1, collate_fn=cvig_fov.collate_packed)
    batches = list(loader)
    assert int(batches[0]['overhead_desc'][:, 24].sum()) == 0 and int(batches[0]['surface_desc'][:, 24].sum()) == 0
    assert list(batches[0]['overhead_desc'][:, 26].numpy()) == [2, 2] and list(batches[0]['surface_desc'][:, 26].numpy()) == [1, 2]
    del jpeg._ERRORS[:]
    got = prep(batches[0])
    assert torch.equal(got['surface'], ref['surface']) and torch.equal(got['polar'], ref['polar'])
    assert jpeg.entropy_errors() == 0
