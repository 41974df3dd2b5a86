"""cvig_baseline's packed data path on the GPU: the two batched kernels of csrc/baseline_prep.hip against the per-sample ops they
replace (bit for bit), their memory contract, GpuPreprocess's packed / staged route against its per-sample route for every input
form, and the drivers under data_path='packed'."""
import os

import numpy as np
import pytest
import torch

from oracle import cvig_baseline_oracle as OB
from tests.mem_arena import Arena, ArenaTorch
from witw_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLES = [0, 90, 37.3, 180, 301.0, -17.5]
PERM = [3, 0, 5, 1, 4, 2]            # table row i describes image PERM[i]: not the order of the addresses


def _images(seed, n, hw, kind, cs):
    """n images of hw: kind 1 = uint8 HWC arrays with cs stored channels, kind 0 = float32 CHW tensors (values with fractions)"""
    g = np.random.Generator(np.random.Philox(key=[seed, 7]))
    if kind == 1:
        return [g.integers(0, 256, size=hw + (cs,), dtype=np.uint8) for _ in range(n)]
    return [torch.from_numpy((g.random((cs,) + hw, dtype=np.float32) * np.float32(255.)).astype(np.float32)) for _ in range(n)]


def _chw(a):
    """the image as ops.rotate_nearest / torch.roll take it: float32 CHW, first three channels"""
    if isinstance(a, np.ndarray):
        return torch.from_numpy(a[:, :, :3].astype(np.float32).transpose(2, 0, 1).copy())
    return a[:3].clone()


def _table(images, order=None, starts=None, place=None):
    """images in ONE packed block at the 16-byte aligned offsets cvig_fov._pack_side gives -> (block on the device, table, kind)"""
    from witw_amd import cvig_fov
    buf, desc, kind = cvig_fov._pack_side(images)
    assert all(int(o) % 16 == 0 for o in desc[:, 0])
    dbuf = buf.cuda() if place is None else place(buf.cuda())
    order = list(range(len(images))) if order is None else order
    rows = [(dbuf.data_ptr() + int(desc[j, 0]), int(desc[j, 1]), int(desc[j, 2]), 0 if starts is None else starts[i], int(desc[j, 3]))
            for i, j in enumerate(order)]
    table = torch.tensor(rows, dtype=torch.int64).cuda()
    return dbuf, (table if place is None else place(table)), kind


@pytest.mark.parametrize('hw', [(37, 53), (64, 64), (96, 128)])
@pytest.mark.parametrize('kind,cs', [(1, 3), (1, 4), (0, 3), (0, 5)])
def test_rotate_batched_is_rotate_nearest_bit_for_bit(hw, kind, cs):
    from witw_amd import baseline_data as bd
    from witw_amd import cvig_baseline as cb
    from witw_amd import ops
    images = _images(11 + cs, 6, hw, kind, cs)
    _keep, table, k = _table(images, PERM)
    assert k == kind
    got = bd.rotate_batched(table, ANGLES, 6, 3, hw, kind=kind)
    x = torch.stack([_chw(images[j]) for j in PERM])
    want = ops.rotate_nearest(x.cuda(), ANGLES)
    assert got.shape == (6, 3) + hw and torch.equal(got, want)
    assert torch.equal(got[0].cpu(), x[0])                                   # 0 degrees: the identity
    # the theta computed ahead (GpuPreprocess.stage) is the same launch
    theta = ops.rotation_theta(ANGLES, *hw).reshape(6, 6).cuda()
    assert torch.equal(bd.rotate_batched(table, None, 6, 3, hw, kind=kind, theta=theta), want)
    if hw[0] == hw[1]:                                                       # 90 degrees on a square: an exact quarter turn
        assert torch.equal(got[1].cpu(), cb.quantized_rotation(x[1], 3))


def test_rotate_batched_against_the_oracle():
    """the inputs and the cap of test_rotate_nearest_matches_torchvision_restatement (tests/test_drivers2_gpu.py): at most 1e-3 of
    the pixels sit within float rounding of a .5 boundary and take a neighbouring source"""
    from witw_amd import baseline_data as bd
    x = torch.from_numpy(synth.images_u8(70, 1, (3, 3, 96, 128)))
    angles = [0.0, 90.0, 37.3]
    images = [np.ascontiguousarray(x[i].permute(1, 2, 0).numpy().astype(np.uint8)) for i in range(3)]
    _keep, table, kind = _table(images)
    got = bd.rotate_batched(table, angles, 3, 3, (96, 128), kind=kind).cpu()
    for i, a in enumerate(angles):
        diff = (got[i] != OB.rotate(x[i], a)).any(dim=0).float().mean().item()
        print('angle %g: fraction of differing pixels %.3g' % (a, diff))
        assert diff <= 1e-3, (a, diff)


@pytest.mark.parametrize('rep', [1, 2])
@pytest.mark.parametrize('kind', [0, 1])
def test_roll_rows_batched_is_roll_and_repeat_interleave(rep, kind):
    from witw_amd import baseline_data as bd
    for hw, starts in (((32, 360), [0, 1, 90, 359]), ((37, 53), [52, 0])):
        n = len(starts)
        images = [_images(21 + i, 1, hw, kind, 3 + (i % 2) * (1 if kind else 2))[0] for i in range(n)]      # 3 and 4 (5) stored channels
        order = list(range(n))[::-1]
        _keep, table, k = _table(images, order, starts)
        got = bd.roll_rows_batched(table, n, 3, (rep * hw[0], hw[1]), rep=rep, kind=k)
        want = torch.stack([torch.roll(_chw(images[j]), -s, -1).repeat_interleave(rep, -2) for j, s in zip(order, starts)])
        assert got.shape == want.shape and torch.equal(got.cpu(), want), (hw, rep, kind)


@pytest.mark.parametrize('skew', [0, 16])
def test_memory_contract_of_both_kernels(monkeypatch, skew):
    """outputs inside guard bands and pre-filled with a NaN canary: no byte outside the payload is written and every output
    element is stored (the zero corners of a 45-degree rotation too), at a 256-byte and at a 16-byte aligned address; a table row
    whose image is SMALLER than the launch (a valid small image) gives a zero image instead of reads past its end"""
    from witw_amd import baseline_data as bd
    from witw_amd import ops
    arena = Arena('cuda', skew_bytes=skew)
    monkeypatch.setattr(bd, 'torch', ArenaTorch(arena))
    hw = (37, 53)
    for kind in (1, 0):
        images = _images(31, 3, hw, kind, 3) + _images(32, 1, (20, 30), kind, 3)
        _keep, table, k = _table(images, [2, 0, 1], place=arena.place)
        y = bd.rotate_batched(table, [45., 45., 200.], 3, 3, hw, kind=k)
        arena.check(y)
        assert torch.equal(y, ops.rotate_nearest(torch.stack([_chw(images[j]) for j in (2, 0, 1)]).cuda(), [45., 45., 200.]))
        assert float(y[0, :, 0, 0].abs().sum()) == 0.                       # a corner the rotation leaves empty
        _keep, table, k = _table(images, [0, 3, 1], place=arena.place)       # row 1: the 20 x 30 image
        y = bd.rotate_batched(table, [10., 10., 10.], 3, 3, hw, kind=k)
        arena.check(y)
        assert float(y[1].abs().sum()) == 0. and float(y[0].abs().sum()) > 0. and float(y[2].abs().sum()) > 0.
        for rep in (1, 2):
            _keep, table, k = _table(images, [1, 2, 0], [52, 0, 7], place=arena.place)
            y = bd.roll_rows_batched(table, 3, 3, (rep * hw[0], hw[1]), rep=rep, kind=k)
            arena.check(y)
            want = torch.stack([torch.roll(_chw(images[j]), -s, -1).repeat_interleave(rep, -2) for j, s in zip([1, 2, 0], [52, 0, 7])])
            assert torch.equal(y.cpu(), want)
            _keep, table, k = _table(images, [1, 3, 0], [5, 5, 5], place=arena.place)
            y = bd.roll_rows_batched(table, 3, 3, (rep * hw[0], hw[1]), rep=rep, kind=k)
            arena.check(y)
            assert float(y[1].abs().sum()) == 0. and float(y[0].abs().sum()) > 0.
        # a start outside the row: zeros as well, not a read past the row
        _keep, table, k = _table(images[:3], None, [0, 53, -1], place=arena.place)
        y = bd.roll_rows_batched(table, 3, 3, hw, rep=1, kind=k)
        arena.check(y)
        assert float(y[1].abs().sum()) == 0. and float(y[2].abs().sum()) == 0. and torch.equal(y[0].cpu(), _chw(images[0]))


# ----------------------------------------------------------------------------- GpuPreprocess: packed / staged route == per-sample route
SIZES = {'cvusa': ([(40, 120)] * 3, [(48, 48)] * 3), 'witw': ([(30, 50), (61, 47), (40, 40)], [(48, 48)] * 3)}


def _u8_samples(dataset, seed=41):
    g = np.random.Generator(np.random.Philox(key=[seed, 3]))
    su, ov = SIZES[dataset]
    return [{'surface': g.integers(0, 256, size=s + (3,), dtype=np.uint8), 'overhead': g.integers(0, 256, size=o + (3,), dtype=np.uint8)}
            for s, o in zip(su, ov)]


def _as_tensors(samples):
    return {'surface': [_chw(s['surface']) for s in samples], 'overhead': [_chw(s['overhead']) for s in samples]}


def _same(a, b):
    return a['surface'].shape == b['surface'].shape and torch.equal(a['surface'], b['surface']) and torch.equal(a['overhead'], b['overhead'])


@pytest.mark.parametrize('dataset', ['cvusa', 'witw'])
def test_gpu_preprocess_packed_route_equals_per_sample_route(dataset):
    from witw_amd import cvig_baseline as cb
    from witw_amd import cvig_fov
    from witw_amd import ring as ring_mod
    samples = _u8_samples(dataset)
    prep = cb.GpuPreprocess(dataset)
    torch.manual_seed(5)
    want = prep(_as_tensors(samples))                                         # the per-sample route: lists of float tensors
    assert want['surface'].shape == ((3, 3, 80, 120) if dataset == 'cvusa' else (3, 3, 500, 500)) and want['overhead'].shape == (3, 3, 48, 48)
    torch.manual_seed(5)
    drawn = [torch.rand(()).item() * 360. for _ in range(3)]

    def run(batch, p=prep, **kw):
        torch.manual_seed(5)
        return p(batch, **kw)

    assert _same(run(cb.collate_packed(samples)), want)                       # uint8 arrays through collate_packed
    assert _same(run(cvig_fov.collate_raw(samples)), want)                    # raw lists of uint8 arrays
    assert _same(run([cb.collate_packed(samples[:2]), cb.collate_packed(samples[2:])]), want)      # a list of two parts
    torch.manual_seed(5)
    st = prep.stage(cb.collate_packed(samples))                               # staged ahead, preprocessed later
    assert isinstance(st, cvig_fov.StagedBatch) and st.n == 3 and st.angles == drawn
    torch.manual_seed(77)
    assert _same(prep(st), want)
    tensors = _as_tensors(samples)                                            # float tensors: packed (kind 0), staged from resident ones
    packed_f32 = cb.collate_packed([{'surface': s, 'overhead': o} for s, o in zip(tensors['surface'], tensors['overhead'])])
    assert packed_f32['surface_kind'] == 0 and _same(run(packed_f32), want)
    torch.manual_seed(5)
    assert _same(prep(prep.stage({'surface': [t.cuda() for t in tensors['surface']], 'overhead': [t.cuda() for t in tensors['overhead']]})), want)
    ring = ring_mod.PinnedRing(slots=2, slot_bytes=1 << 20)                   # a PinnedRing-backed batch
    try:
        batch = cb.collate_packed(samples, ring=ring)
        assert 'ring' in batch
        assert _same(run(batch, cb.GpuPreprocess(dataset, ring=ring)), want)
    finally:
        ring.close()
    # angles= on both routes; another seed must not matter then
    inj = [10., 200., 359.]
    torch.manual_seed(1)
    a = prep(_as_tensors(samples), angles=inj)
    torch.manual_seed(2)
    b = prep(cb.collate_packed(samples), angles=inj)
    assert _same(a, b) and not torch.equal(a['overhead'], want['overhead'])
    if dataset == 'cvusa':
        assert torch.equal(a['surface'][1], torch.roll(_chw(samples[1]['surface']), -round(200. * 120 / 360.), -1).repeat_interleave(2, -2).cuda())


def _write_jpegs(root, dataset, extra_surface=None):
    """the sizes of SIZES as JPEG files + the data set's CSV; extra_surface: one more pair whose surface is that file"""
    from PIL import Image
    g = np.random.Generator(np.random.Philox(key=[43, 3]))
    su, ov = SIZES[dataset]
    pairs = []
    for i, (s, o) in enumerate(zip(su, ov)):
        for tag, (h, w) in (('su', s), ('ov', o)):
            a = g.integers(0, 256, size=(h // 4 + 1, w // 4 + 1, 3), dtype=np.uint8).repeat(4, 0).repeat(4, 1)[:h, :w]
            Image.fromarray(a).save(os.path.join(root, '%s_%d.jpg' % (tag, i)), quality=88)
        pairs.append(('su_%d.jpg' % i, 'ov_%d.jpg' % i))
    if extra_surface:
        pairs.append((extra_surface, 'ov_0.jpg'))
    csv = os.path.join(root, 'pairs.csv')
    with open(csv, 'w') as f:
        if dataset == 'cvusa':
            f.write(''.join('%s,%s\n' % (o, s) for s, o in pairs))
        else:
            f.write(','.join('c%d' % i for i in range(17)) + '\n' + ''.join(','.join(['x'] * 15 + [s, o]) + '\n' for s, o in pairs))
    return csv


@pytest.mark.parametrize('dataset', ['cvusa', 'witw'])
def test_gpu_preprocess_jpeg_files(tmp_path, dataset):
    """raw='jpeg': the files are entropy-decoded by the dataset, finished on the device and preprocessed in two launches -- the bits
    of the reference route on Pillow's float tensors; one committed fixture as a witw surface"""
    from witw_amd import cvig_baseline as cb
    from witw_amd import cvig_fov
    extra = os.path.join(ROOT, 'tests', 'golden', 'jpeg', 's420_q90.jpg') if dataset == 'witw' else None
    csv = _write_jpegs(str(tmp_path), dataset, extra)
    ref_set, jpeg_set = cb.ImagePairDataset(dataset, csv), cb.ImagePairDataset(dataset, csv, raw='jpeg')
    n = len(ref_set)
    assert n == (4 if extra else 3)
    prep = cb.GpuPreprocess(dataset)
    torch.manual_seed(8)
    want = prep(cvig_fov.collate_raw([ref_set[i] for i in range(n)]))
    batch = cb.collate_packed([jpeg_set[i] for i in range(n)])
    torch.manual_seed(8)
    got = prep(batch)
    assert _same(got, want)
    torch.manual_seed(8)
    assert _same(prep(cvig_fov.collate_raw([jpeg_set[i] for i in range(n)])), want)      # raw lists of JpegFile objects


def test_gpu_preprocess_refuses_what_it_cannot_batch():
    from witw_amd import _lib
    from witw_amd import cvig_baseline as cb
    samples = _u8_samples('cvusa')
    odd = [dict(s) for s in samples]
    odd[2]['overhead'] = np.zeros((50, 48, 3), dtype=np.uint8)
    with pytest.raises(_lib.WitwError, match=r'overhead images .* 48x48 and 50x48'):
        cb.GpuPreprocess('cvusa')(cb.collate_packed(odd))
    odd = [dict(s) for s in samples]
    odd[1]['surface'] = np.zeros((40, 100, 3), dtype=np.uint8)
    with pytest.raises(_lib.WitwError, match=r'surface images .* 40x120 and 40x100'):
        cb.GpuPreprocess('cvusa')(cb.collate_packed(odd))
    cb.GpuPreprocess('witw')(cb.collate_packed(odd))                          # witw surfaces may differ
    gray = [dict(s) for s in samples]
    gray[0]['surface'] = np.zeros((40, 120, 1), dtype=np.uint8)
    with pytest.raises(_lib.WitwError, match='1 channels'):
        cb.GpuPreprocess('cvusa')(cb.collate_packed(gray))
    with pytest.raises(_lib.WitwError, match='2 angles'):
        cb.GpuPreprocess('cvusa')(cb.collate_packed(samples), angles=[1., 2.])
    prep = cb.GpuPreprocess('cvusa')
    with pytest.raises(_lib.WitwError, match='staged with'):                  # a staged batch has its angles already
        prep(prep.stage(cb.collate_packed(samples)), angles=[1., 2., 3.])
    assert cb.GpuPreprocess('cvusa').stage(cb.collate_packed([])).n == 0      # a rank's empty share


# ----------------------------------------------------------------------------- drivers
def _write_driver_dataset(root, n):
    from PIL import Image
    rows = []
    for i in range(n):
        Image.fromarray(synth.images_u8(72, i, (400, 400, 3)).astype(np.uint8)).save(os.path.join(root, 'ov_%d.jpg' % i), quality=90)
        Image.fromarray(synth.images_u8(73, i, (200, 800, 3)).astype(np.uint8)).save(os.path.join(root, 'su_%d.jpg' % i), quality=90)
        rows.append('ov_%d.jpg,su_%d.jpg' % (i, i))
    with open(os.path.join(root, 'pairs.csv'), 'w') as f:
        f.write('\n'.join(rows) + '\n')
    return os.path.join(root, 'pairs.csv')


def test_drivers_on_the_packed_data_path(tmp_path, monkeypatch, capsys):
    from witw_amd import cvig_baseline as cb
    csv = _write_driver_dataset(str(tmp_path), 5)
    monkeypatch.chdir(tmp_path)
    for workers in (0, 2):                                                    # 2: the workers build their batches in the pinned ring
        best = cb.train(dataset='cvusa', val_quantity=2, batch_size=3, num_workers=workers, num_epochs=1, csv_path=csv, data_path='packed')
        assert best is not None and np.isfinite(best), (workers, best)
    assert os.path.exists(os.path.join('weights', 'surface_best.pth'))
    torch.manual_seed(12)
    packed = cb.test(dataset='cvusa', batch_size=4, num_workers=0, csv_path=csv, data_path='packed')
    torch.manual_seed(12)
    reference = cb.test(dataset='cvusa', batch_size=4, num_workers=0, csv_path=csv)
    out = capsys.readouterr().out
    assert packed == reference and out.count('Locations: 5') == 2, (packed, reference)
    monkeypatch.setattr(cb.Globals, 'data_path', 'packed')                    # None = the Global
    torch.manual_seed(12)
    assert cb.test(dataset='cvusa', batch_size=4, num_workers=0, csv_path=csv) == reference


def test_cli_data_path(monkeypatch):
    from witw_amd import cvig_baseline as cb
    seen = {}
    monkeypatch.setattr(cb, 'train', lambda **kw: seen.update(train=kw))
    monkeypatch.setattr(cb, 'test', lambda **kw: seen.update(test=kw))
    cb.main(['--data-path', 'packed'])
    cb.main(['--mode', 'test', '--data-path', 'packed'])
    assert seen['train']['data_path'] == 'packed' and seen['test']['data_path'] == 'packed'
    cb.main([])
    assert 'data_path' not in seen['train']              # no flag: the drivers take Globals.data_path
    with pytest.raises(SystemExit):
        cb.main(['--data-path', 'zip'])
