"""Progressive files through the device back end (csrc/jpeg.hip behind the host's progressive entropy decoder, jpeg.PROGRESSIVE on):
one batch of progressive, sequential and raw entries, every image byte for byte Pillow's. Damaged streams stay on the CPU
(tests/test_jpeg_progressive.py); what is left of them reaches the GPU as Pillow's pixels."""
import numpy as np
import pytest
import torch

from witw_amd import jpeg

from . import jpeg_prog_craft as PC
from .test_jpeg_progressive import flat_blocks_file, picture, pillow, save, source

pytestmark = pytest.mark.gpu


def test_progressive_files_in_a_mixed_batch_equal_pillow(monkeypatch):
    monkeypatch.setattr(jpeg, 'PROGRESSIVE', True)
    assert jpeg.DEVICE_ENTROPY == 'all'
    del jpeg._ERRORS[:]
    g = np.random.Generator(np.random.Philox(key=[32, 1]))
    seq, src = source('420', 33, 49, quality=97)
    raws = [save(picture(1, 40, 56), '420', 90, progressive=True), save(picture(2, 17, 9, grey=True), 'grey', 85, progressive=True),
            save(picture(3, 64, 64), '444', 75, progressive=True), save(picture(4, 97, 131), '422', 80),
            g.integers(0, 256, size=(7, 9, 3), dtype=np.uint8),
            flat_blocks_file()[2],                                                                   # successive approximation, one long EOB run
            PC.write(33, 49, src.coef, src.qt, '420', PC.script_successive(3, al=2, bands=((1, 9), (10, 63))))]
    items = [r if isinstance(r, np.ndarray) else jpeg.open_file(r) for r in raws]
    assert [isinstance(i, jpeg.JpegFile) and i.progressive for i in items] == [True, True, True, False, False, True, True]
    buf, desc, _k = jpeg.pack(items)
    d = desc.numpy()
    assert list(d[:, 24]) == [0, 0, 0, 0, 1, 0, 0]                  # raw: the array alone
    assert list(d[:, 26]) == [0, 0, 0, 1, 0, 0, 0]                  # entropy-decoded on the device: the sequential file alone
    out = jpeg.decode(items, torch.device('cuda:0'))
    for k, (o, r) in enumerate(zip(out, raws)):
        ref = r if isinstance(r, np.ndarray) else pillow(r)
        np.testing.assert_array_equal(o.cpu().numpy(), ref if ref.ndim == 3 else ref[:, :, None], err_msg=str(k))
    np.testing.assert_array_equal(out[6].cpu().numpy(), pillow(seq))
    assert jpeg.entropy_errors() == 0


def test_data_path_with_progressive_files_equals_host_decode(tmp_path):
    """ImagePairDataset(raw='jpeg', jpeg_progressive=True) through loader workers: no file of the batch travels as pixels, and the
    'surface' / 'polar' tensors are those of Pillow's decode (raw=True), bit for bit"""
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
    ds = cvig_fov.ImagePairDataset('cvusa', csv, raw='jpeg', jpeg_progressive=True)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, num_workers=1, collate_fn=cvig_fov.collate_packed)
    batches = list(loader)
    assert int(batches[0]['overhead_desc'][:, 24].sum()) == 0 and int(batches[0]['surface_desc'][:, 24].sum()) == 0
    assert list(batches[0]['overhead_desc'][:, 26].numpy()) == [0, 0] and list(batches[0]['surface_desc'][:, 26].numpy()) == [1, 0]
    got = prep(batches[0])
    assert torch.equal(got['surface'], ref['surface']) and torch.equal(got['polar'], ref['polar'])
