"""4:4:0 (h1v2) files through the device (opt-in jpeg.SAMPLING_440): the entropy decoders of csrc/jpeg.hip on the 1 x 2 MCU (Y, Y below
it, Cb, Cr -- taken from the plan like every other geometry) give the host decoder's coefficients, and upsampling mode 5 behind them
gives Pillow's bytes -- single files on every DEVICE_ENTROPY route, mixed batches, damaged files, the data path. The arithmetic of
the mode is pinned on the CPU (tests/test_jpeg_440.py)."""
import io

import numpy as np
import pytest
import torch

from witw_amd import jpeg

from . import jpeg_440_craft as C4
from . import jpeg_craft as JC
from . import jpeg_prog_craft as PC
from .test_jpeg_440 import CORPUS, _second_luma_damage, fixture
from .test_jpeg_damage_gpu import _image_of, _kernels, _launch, _pillow_or_none, pipeline_check

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SINGLE = [c for c in CORPUS if c[0].split('_')[0] in ('8x16', '9x17', '41x23', '40x48') and c[0].split('_')[1] in ('dri0', 'dri2')]
_BIG = []


def big():
    """(file bytes without restart markers, with a marker every 3 MCUs, coefficients): 120 x 136, 8 x 17 MCUs, 544 blocks -- more than
    jpeg.SELFSYNC_MIN_BLOCKS, so the marker-less one is the self-synchronising kernel's on the data path; more than 256 intervals
    with dri=1 would need a second workgroup, 46 here"""
    if not _BIG:
        g = np.random.Generator(np.random.Philox(key=[44, 120]))
        c, qt = C4.pixel_coef(g, 120, 136), g.integers(1, 5, size=(3, 64)).astype(np.uint16)
        _BIG.extend([C4.write(120, 136, c, qt), C4.write(120, 136, c, qt, dri=3), c])
    return _BIG


def test_device_entropy_decoders_give_the_host_coefficients(monkeypatch):
    """every file of the single-file set (long-code tables with categories 12-15 included) and the 544-block pair, on every kernel that
    may meet it: the interval kernel, the self-synchronising kernel at 256 / 512 / 1024 threads"""
    monkeypatch.setattr(jpeg, 'SAMPLING_440', True)
    files = [(n, d, c) for n, _H, _W, d, c, _q in SINGLE] + [('big', big()[0], big()[2]), ('big_rst', big()[1], big()[2])]
    groups = {}
    for i, (_n, d, _c) in enumerate(files):
        for k in _kernels(d):
            groups.setdefault(k, []).append(i)
    assert set(groups) == {'huffman', 256, 512, 1024}
    for k, idx in groups.items():
        got, err = _launch([files[i][1] for i in idx], k)
        for j, i in enumerate(idx):
            name, data, c = files[i]
            assert err[j] == 0, (k, name, int(err[j]))
            host = jpeg.read_coef(data)
            np.testing.assert_array_equal(host.coef, c)
            bad = np.nonzero((got[j] != host.coef).any(axis=1))[0]
            assert bad.size == 0, '%s on %s: %d of %d blocks differ, first %s' % (k, name, bad.size, c.shape[0], bad[:5])


@pytest.mark.parametrize('device_entropy', ['all', 'restart', False])
def test_single_files_equal_pillow(monkeypatch, device_entropy):
    monkeypatch.setattr(jpeg, 'SAMPLING_440', True)
    monkeypatch.setattr(jpeg, 'DEVICE_ENTROPY', device_entropy)
    del jpeg._ERRORS[:]
    files = [(n, d) for n, _H, _W, d, _c, _q in SINGLE if n.endswith('_std')] + [('big', big()[0]), ('big_rst', big()[1])] + \
        [(n, fixture(n)) for n in ('s440_q90', 's440_rst')]
    assert len(files) == 12
    for name, data in files:
        item = jpeg.open_file(data)
        _b, desc, _k = jpeg.pack([item])
        rst = int(item.entropy_plan()[0][4:8].view(np.int32)[0]) > 1             # more than one restart interval
        assert int(desc[0, 24]) == 0 and int(desc[0, 26]) == (1 if device_entropy == 'all' or (device_entropy and rst) else 0), name
        out = jpeg.decode([item], DEV)[0].cpu().numpy()
        np.testing.assert_array_equal(out, JC.pillow(data), err_msg=name)
    assert jpeg.entropy_errors() == 0


def _mixed_batch():
    """[(what, bytes or uint8 array)]: 4:4:4, 4:2:2, 4:2:0, grey (Pillow's), 4:4:0 without and with restart markers, a 544-block 4:4:0
    file, a progressive 4:4:0 file, and a file the decoder leaves to Pillow under every setting (RGB colour space)"""
    from PIL import Image
    from .test_jpeg_progressive import picture, save
    exp_c = C4.picture_coef(90, 40, 48, quality=90)
    bio = io.BytesIO()
    Image.fromarray(picture(6, 33, 47)).save(bio, 'JPEG', quality=90, subsampling=0, keep_rgb=True)
    return [('444', save(picture(1, 24, 40), '444', 92)), ('422', save(picture(2, 97, 131), '422', 80, restart_marker_blocks=2)),
            ('420', save(picture(3, 40, 56), '420', 90)), ('grey', save(picture(4, 17, 9, grey=True), 'grey', 85)),
            ('440', fixture('s440_q90')), ('440_rst', fixture('s440_rst')), ('440_big', big()[0]),
            ('440_prog', C4.write_progressive(40, 48, exp_c[0], exp_c[1], PC.script_successive(3, al=2))),
            ('pillow', bio.getvalue())]


def _items(batch):
    out = []
    for _what, data in batch:
        f = jpeg.open_file(data)
        if f is None:
            f = JC.pillow(data)
            f = f[:, :, None] if f.ndim == 2 else f
        out.append(f)
    return out


def _refs(batch):
    return [r if r.ndim == 3 else r[:, :, None] for r in (JC.pillow(d) for _w, d in batch)]


def test_mixed_batch_equals_pillow(monkeypatch):
    monkeypatch.setattr(jpeg, 'SAMPLING_440', True)
    monkeypatch.setattr(jpeg, 'PROGRESSIVE', True)
    assert jpeg.DEVICE_ENTROPY == 'all'
    del jpeg._ERRORS[:]
    batch, refs = _mixed_batch(), _refs(_mixed_batch())
    items = _items(batch)
    assert [isinstance(i, jpeg.JpegFile) for i in items] == [True] * 8 + [False]
    assert [list(i.info[3:5]) for i in items[4:8]] == [[1, 2]] * 4 and items[7].progressive
    buf, desc, _k = jpeg.pack(items)
    d = desc.numpy()
    # the device path ran for the 4:4:0 entries: none is raw (24), the sequential ones are entropy-decoded on the device (26), the
    # progressive one brings the host's coefficient blocks, and all four go through upsampling mode 5
    assert list(d[:, 24]) == [0] * 8 + [1] and list(d[:, 26]) == [1] * 7 + [0, 0]
    assert list(jpeg.decode_tables(d[4:8])[1][:, 3]) == [5, 5, 5, 5]
    dbuf = buf.to(DEV)
    keep, table = jpeg.decode_packed(dbuf, desc, host_buf=buf)
    torch.cuda.synchronize()
    for i, ref in enumerate(refs):
        np.testing.assert_array_equal(_image_of([dbuf] + keep, table, i), ref, err_msg='decode_packed: ' + batch[i][0])
    # the same batch as two parts of one side (quarter batches): one set of launches over both
    order = [8, 4, 0, 7, 5], [6, 1, 2, 3]
    parts = []
    for idx in order:
        b, ds, _k = jpeg.pack([items[i] for i in idx])
        parts.append((b.to(DEV), ds, b))
    keep, table, _f = jpeg.decode_packed_multi(parts)
    torch.cuda.synchronize()
    for j, i in enumerate(order[0] + order[1]):
        np.testing.assert_array_equal(_image_of([p[0] for p in parts] + keep, table, j), refs[i], err_msg='decode_packed_multi: ' + batch[i][0])
    assert jpeg.entropy_errors() == 0


def test_opt_in_off_gives_the_same_images_with_the_440_files_as_raw_bytes(monkeypatch):
    monkeypatch.setattr(jpeg, 'SAMPLING_440', False)
    monkeypatch.setattr(jpeg, 'PROGRESSIVE', True)
    batch, refs = _mixed_batch(), _refs(_mixed_batch())
    items = _items(batch)
    assert [isinstance(i, jpeg.JpegFile) for i in items] == [True] * 4 + [False] * 5
    buf, desc, _k = jpeg.pack(items)
    assert list(desc[:, 24].numpy()) == [0] * 4 + [1] * 5
    out = jpeg.decode(items, DEV)
    monkeypatch.setattr(jpeg, 'SAMPLING_440', True)
    on = jpeg.decode(_items(batch), DEV)
    for i, ref in enumerate(refs):
        np.testing.assert_array_equal(out[i].cpu().numpy(), ref, err_msg=batch[i][0])
        assert torch.equal(out[i], on[i]), batch[i][0]


def test_damaged_440_files_are_flagged_and_come_back_as_pillow_reads_them(monkeypatch):
    """the existing error-flag path (CHECK_ERRORS): an invalid code and a cut inside the second luma block of an MCU -- in a file of the
    one-thread route, in an interval of a restart-marker file, in a self-sync sized file -- are flagged by the device decoder and
    re-decoded by Pillow from the host block; the sound files of the batch equal Pillow"""
    monkeypatch.setattr(jpeg, 'SAMPLING_440', True)
    raws = [_second_luma_damage('440', H, W, dri, mcu, kind)[0]
            for (H, W, dri, mcu) in ((40, 48, 0, 7), (40, 48, 2, 7), (120, 136, 0, 70), (120, 136, 3, 70)) for kind in ('cut', 'inval')]
    assert all(jpeg.read_coef(r) is None for r in raws)
    # (a cut also takes the later RSTn markers away: such a file gets no plan and is Pillow's inside pack(), as a 4:2:2 file's would be)
    planned = [r for r in raws if jpeg.open_file(r).entropy_plan() is not None]
    assert len(planned) == 6
    sound = [fixture('s440_q90'), fixture('s440_rst'), big()[0], big()[1]]
    repaired, n_ok, n_refused = pipeline_check(raws[:4] + sound[:2] + raws[4:] + sound[2:], monkeypatch)
    assert n_ok + n_refused == 12 and n_ok >= 8
    # decode_packed: every damaged file that travelled as file bytes and that Pillow reads was flagged and re-decoded
    assert repaired == sum(_pillow_or_none(r) is not None for r in planned) >= 4


def test_data_path_with_440_surfaces_equals_host_decode(tmp_path):
    """ImagePairDataset(raw='jpeg', jpeg_440=True) through two loader workers: no surface travels as pixels, and the 'surface' /
    'polar' tensors are those of Pillow's decode (raw=True), bit for bit"""
    import os
    from PIL import Image
    from witw_amd import cvig_fov
    from .test_jpeg_progressive import picture
    root, rows = str(tmp_path), []
    for i, (hs, ws) in enumerate([(48, 80), (100, 133), (41, 23), (64, 96)]):
        Image.fromarray(picture(40 + i, 64 + 8 * i, 64)).save(os.path.join(root, 'ov_%d.jpg' % i), quality=88)
        with open(os.path.join(root, 'su_%d.jpg' % i), 'wb') as f:
            f.write(C4.write(hs, ws, *C4.picture_coef(50 + i, hs, ws, quality=88), dri=(0, 4)[i % 2]))
        rows.append('ov_%d.jpg,su_%d.jpg' % (i, i))
    csv = os.path.join(root, 'pairs.csv')
    open(csv, 'w').write('\n'.join(rows) + '\n')
    prep = cvig_fov.GpuPreprocess('cvusa', fov=360, random_orientation=False)
    ref = prep(cvig_fov.collate_packed([cvig_fov.ImagePairDataset('cvusa', csv, raw=True)[i] for i in range(4)]))
    off = cvig_fov.collate_packed([cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg')[i] for i in range(4)])
    assert off['surface_kind'] == 1 and off['overhead_kind'] == jpeg.KIND_JPEG      # opt-in off: every surface is Pillow's pixels (kind 1)
    ds = cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg', jpeg_440=True)
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, num_workers=2, collate_fn=cvig_fov.collate_packed)
    batches = list(loader)
    d = batches[0]['surface_desc'].numpy()
    assert int(d[:, 24].sum()) == 0 and list(d[:, 26]) == [1, 1, 1, 1] and [list(r) for r in d[:, 5:7]] == [[1, 2]] * 4
    got = prep(batches[0])
    assert torch.equal(got['surface'], ref['surface']) and torch.equal(got['polar'], ref['polar'])
