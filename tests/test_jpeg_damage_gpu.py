"""The device entropy decoders (csrc/jpeg.hip: jpeg_huffman_kernel, one thread per restart interval; jpeg_selfsync_kernel, one
workgroup per marker-less file) on crafted streams (tests/jpeg_craft.py) and on damaged ones. Valid files: the written coefficients
bit for bit, no flag. Damaged files: whatever the host decoder refuses is flagged, and an unflagged file has the host decoder's
coefficients -- so the pipeline, which hands flagged files to Pillow, returns Pillow's image of every file."""
import numpy as np
import pytest
import torch

from witw_amd import jpeg

from . import jpeg_craft as JC

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
THREADS = (256, 512, 1024)


def _launch(files, kernel):
    """entropy-decode `files` (bytes, each with an entropy plan) with kernel 'huffman' or a self-sync thread count ->
    (coef int16 [blocks, 64] per file, error flag per file)"""
    from witw_amd import _lib, ops
    items = [jpeg.open_file(f) for f in files]
    plans = [it.entropy_plan() for it in items]
    blocks = np.array([int(it.info[5]) for it in items], dtype=np.int64)
    first = np.cumsum(blocks) - blocks
    coef = torch.zeros((int(blocks.sum()), 64), dtype=torch.int16, device=DEV)
    keep, rows = [], []
    for it, (plan, _qt), f0 in zip(items, plans, first):
        raw = np.zeros((it.data.size + 24 + 7) // 8 * 8, dtype=np.uint8)       # 24 readable bytes behind the end, as pack() leaves
        raw[:it.data.size] = it.data
        rb, pb = torch.from_numpy(raw).to(DEV), torch.from_numpy(np.concatenate([plan, np.zeros(16, np.uint8)])).to(DEV)
        sc = torch.empty(((it.data.size + 32 + 7) // 8 * 8,), dtype=torch.uint8, device=DEV)
        keep += [rb, pb, sc]
        rows.append((rb.data_ptr(), pb.data_ptr(), coef.data_ptr() + int(f0) * 128, it.data.size, sc.data_ptr(), 0))
    errors = torch.zeros((len(items),), dtype=torch.int32, device=DEV)
    lib = _lib.load()
    if kernel == 'huffman':
        files_t = torch.tensor([r[:4] for r in rows], dtype=torch.int64, device=DEV)
        n_int = max(int(p[0][4:8].view(np.int32)[0]) for p in plans)
        _lib.check(lib.witw_jpeg_huffman(files_t.data_ptr(), len(items), n_int, errors.data_ptr(), ops._stream()), 'witw_jpeg_huffman')
    else:
        files_t = torch.tensor(rows, dtype=torch.int64, device=DEV)
        _lib.check(lib.witw_jpeg_huffman_selfsync_threads(files_t.data_ptr(), len(items), kernel, errors.data_ptr(), ops._stream()),
                   'witw_jpeg_huffman_selfsync_threads')
    torch.cuda.synchronize()
    got = coef.cpu().numpy()
    return [got[f0:f0 + nb] for f0, nb in zip(first, blocks)], errors.cpu().numpy()


def _n_int(data):
    return int(jpeg.open_file(data).entropy_plan()[0][4:8].view(np.int32)[0])


def _kernels(data):
    """the launches that may decode this file: the interval kernel for DRI files and marker-less ones of <= SELFSYNC_MIN_BLOCKS blocks
    (decode_packed_multi's choice), the self-sync kernel at every thread count for marker-less files"""
    n_int, blocks = _n_int(data), int(jpeg.open_file(data).info[5])
    ks = ['huffman'] if n_int > 1 or blocks <= jpeg.SELFSYNC_MIN_BLOCKS else []
    return ks + (list(THREADS) if n_int == 1 else [])


def _by_kernel(files):
    groups = {}
    for i, f in enumerate(files):
        for k in _kernels(f):
            groups.setdefault(k, []).append(i)
    return groups


def test_valid_crafted_corpus_decodes_to_the_written_coefficients():
    """A: every sampling, table set and DRI setting, categories 12-15, 16-bit codes, blocks ending at 63 / on a ZRL chain at 64,
    fill bytes, FF 00 at every word offset, > 16,384 intervals, both sides of the LDS staging limit, 96 / 97 blocks"""
    V = JC.valid_corpus()
    files = [d for _n, d, _c in V]
    groups = _by_kernel(files)
    assert set(groups) == {'huffman', 256, 512, 1024}
    for k, idx in groups.items():
        got, err = _launch([files[i] for i in idx], k)
        for j, i in enumerate(idx):
            name, _d, c = V[i]
            assert err[j] == 0, (k, name, int(err[j]))
            bad = np.nonzero((got[j] != c).any(axis=1))[0]
            assert bad.size == 0, '%s on %s: %d of %d blocks differ, first %s' % (k, name, bad.size, c.shape[0], bad[:5])


def test_damaged_files_are_flagged_or_decoded_as_the_host_decodes_them():
    """B: whatever the host decoder refuses is flagged; an unflagged file has the host decoder's coefficients -- on every kernel and
    thread count. The regression: a run past coefficient 63 as a block's last symbol with no EOB, which the self-sync kernel's
    writing pass ended quietly (same block count: no flag)."""
    D = [(n, d) for n, d in JC.damage_corpus() if jpeg.open_file(d).entropy_plan() is not None]
    files = [d for _n, d in D]
    host = [jpeg.read_coef(d) for d in files]
    regress = [i for i, (n, _d) in enumerate(D) if n.startswith('run63_')]
    assert {D[i][0].split('_')[1] for i in regress} == {'selfsync', 'dri', 'small'}
    for k, idx in _by_kernel(files).items():
        got, err = _launch([files[i] for i in idx], k)
        rejected = 0
        for j, i in enumerate(idx):
            name = D[i][0]
            if host[i] is None:
                rejected += 1
                assert err[j] != 0, '%s: %s is refused by the host decoder but not flagged' % (k, name)
            if err[j] == 0:
                np.testing.assert_array_equal(got[j], host[i].coef, err_msg='%s: %s unflagged' % (k, name))
        assert rejected >= 8, (k, rejected)           # the invariant is not met vacuously
        assert any(i in regress for i in idx)


def _pillow_or_none(data):
    try:
        return JC.pillow(data)
    except OSError:
        return None


def _image_of(keep, table, i):
    H, W, C = int(table[i, 1]), int(table[i, 2]), int(table[i, 4])
    src = next(t for t in keep if t.dtype == torch.uint8 and t.data_ptr() <= int(table[i, 0]) < t.data_ptr() + max(1, t.numel()))
    o = int(table[i, 0]) - src.data_ptr()
    return src.reshape(-1)[o:o + H * W * C].reshape(H, W, C).cpu().numpy()


def _expected(data):
    """Pillow's image; for a file the host decoder accepts with dequantised values out of an encoder's range, the C-form decode of
    its coefficients (libjpeg-turbo's SIMD inverse DCT wraps differently there, JC.in_range)"""
    from oracle import jpeg_oracle as J
    r = jpeg.read_coef(data)
    ref = JC.pillow(data)
    if r is not None and not JC.in_range(r.info, r.coef, r.qt):
        ref = J.decode(r.info, r.coef, r.qt)
    return ref if ref.ndim == 3 else ref[:, :, None]


def pipeline_check(raws, monkeypatch):
    """decode_packed(host_buf=...) and jpeg.decode() on `raws` against _expected; files Pillow refuses in batches of their own,
    each of which must raise"""
    from PIL import ImageFile
    monkeypatch.setattr(jpeg, 'DEVICE_ENTROPY', 'all')
    monkeypatch.setattr(ImageFile, 'LOAD_TRUNCATED_IMAGES', True)
    ok = [r for r in raws if _pillow_or_none(r) is not None]
    refused = [r for r in raws if _pillow_or_none(r) is None]
    refs = [_expected(r) for r in ok]
    items = [jpeg.open_file(r) for r in ok]
    assert all(isinstance(it, jpeg.JpegFile) for it in items)
    buf, desc, _k = jpeg.pack(items)
    before = jpeg.REPAIRED[0]
    dbuf = buf.to(DEV)
    keep, table = jpeg.decode_packed(dbuf, desc, host_buf=buf)
    torch.cuda.synchronize()
    repaired = jpeg.REPAIRED[0] - before
    for i, ref in enumerate(refs):
        np.testing.assert_array_equal(_image_of([dbuf] + keep, table, i), ref, err_msg='decode_packed, file %d' % i)
    out = jpeg.decode([jpeg.open_file(r) for r in ok], DEV)
    for i, ref in enumerate(refs):
        np.testing.assert_array_equal(out[i].cpu().numpy(), ref, err_msg='jpeg.decode, file %d' % i)
    for r in refused:
        with pytest.raises(OSError):
            jpeg.decode([jpeg.open_file(r)], DEV)
    return repaired, len(ok), len(refused)


def test_damage_corpus_through_the_pipeline_gives_pillows_images(monkeypatch):
    """C: every file of B through decode_packed(host_buf=...) and jpeg.decode(): Pillow's bytes"""
    raws = [d for _n, d in JC.damage_corpus()]
    repaired, n_ok, _n_refused = pipeline_check(raws, monkeypatch)
    assert repaired >= 20 and n_ok >= 60


def test_a_part_off_the_128_byte_grid_is_refused(monkeypatch):
    """E: decode_packed_multi with a part whose device block sits 64 bytes off the 128-byte grid of the lowest part"""
    from witw_amd import _lib
    monkeypatch.setattr(jpeg, 'DEVICE_ENTROPY', 'all')
    g = np.random.Generator(np.random.Philox(key=[19, 3]))
    c = JC.random_coef(g, 40, 48, '420', density=0.1, amp=20, dc_amp=100)
    data = JC.write(40, 48, c, JC.flat_qt(3, 3), '420')
    buf_a, desc_a, _k = jpeg.pack([jpeg.open_file(data)])
    buf_b, desc_b, _k = jpeg.pack([jpeg.open_file(data)])
    a = buf_a.to(DEV)
    big = torch.zeros((buf_b.numel() + 256,), dtype=torch.uint8, device=DEV)
    big[64:64 + buf_b.numel()] = buf_b.to(DEV)
    b = big[64:64 + buf_b.numel()]
    assert (b.data_ptr() - a.data_ptr()) % 128 != 0
    with pytest.raises(_lib.WitwError):
        jpeg.decode_packed_multi([(a, desc_a, buf_a), (b, desc_b, buf_b)])
    torch.cuda.synchronize()
