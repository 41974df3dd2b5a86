"""Blocks 5-7 of cvig_baseline's bf16 inference path (SurfaceEncoder(precision='bf16_all')) on the GPU against
tests/baseline_bf16_all_ref.py (float64, rounded where the product rounds).

    witw_conv3x3_bf16_fwd_taps4_splitk + witw_taps4_splitk_finish   exact cases (A.CASE_SPLITS: workspace and output equal float64 through an
                                                                    integer view, instantiation asserted), split-K invariance, the
                                                                    workspace fully written, N(0,1) data at the workload's K
    witw_space_to_depth2_mosaic_bf16                                bit for bit the fp32 entry's output rounded to bf16
    SurfaceEncoder(precision='bf16_all')                            1e-2 of the reference embedding's norm, launch record, batch
                                                                    independence, weight-version cache, refusals, test() driver, CLI
    memory contract                                                 both new wrappers between guard bands (tests/mem_arena.py)

Tile of conv_taps4_splitk_bf16_kernel: 16 rows x 16 columns x 128 output channels, K chunks of 16 input channels: A.CASES names the
shapes. tests/test_baseline_bf16_all_ref.py proves on the CPU that the exact cases tell nine wrong kernels from the right one."""
import os

import numpy as np
import pytest
import torch

from witw_amd import synth
from tests import baseline_bf16_all_ref as A
from tests import baseline_bf16_ref as R
from tests.mem_arena import Arena, ArenaTorch

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
KERNEL = 'conv_taps4_splitk_bf16_kernel'


def _f32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _bf16(a):
    """values that ARE bf16 numbers -> a bfloat16 tensor"""
    R.bf16_bits(a)
    return _f32(a).to(torch.bfloat16)


def _bits(t):
    t = t.contiguous().cpu()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()]).numpy().view({4: np.uint32, 2: np.uint16}[t.element_size()])


def _bits_t(t):
    return t.contiguous().view(torch.int32)


class _RecordingTorch(object):
    """stand-in for `torch` inside baseline_bf16: every device `empty` is filled with NaN and kept"""

    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, **kw):
        t = torch.empty(*size, **kw)
        t.fill_(float('nan'))
        self.made.append(t)
        return t


def _run_case(c, S, monkeypatch):
    """-> (workspace, y) of one wrapper call; the workspace is caught at its allocation, pre-filled with NaN"""
    from witw_amd import baseline_bf16 as bb
    from witw_amd import ops
    x, k3, bias, scale, shift = c.data()
    pk = bb.PackedConvBf16Taps4(_f32(k3), _f32(bias))
    xb, sc, sh = _bf16(x), _f32(scale), _f32(shift)
    rec = _RecordingTorch()
    log, check = [], bb._lib.check
    with monkeypatch.context() as m:
        m.setattr(bb, 'torch', rec)
        m.setattr(bb._lib, 'check', lambda rc, what='': (check(rc, what), log.append((what, ops.last_kernel_variant())))[0])
        y = bb.conv_taps4_splitk_bf16(xb, pk, c.n_images, c.g, c.valid, lrelu_slope=c.slope, post_scale=sc, post_shift=sh, ksplit=S)
    assert [w for w, _v in log] == ['witw_conv3x3_bf16_fwd_taps4_splitk', 'witw_taps4_splitk_finish'] and log[0][1] == KERNEL
    ws, y_made = rec.made
    assert y_made.data_ptr() == y.data_ptr()
    return ws, y


@pytest.mark.parametrize('c,S', A.CASE_SPLITS, ids=A.CASE_SPLIT_IDS)
def test_exact_cases_equal_float64(c, S, monkeypatch):
    """workspace -> finish -> y, each bit for bit; no NaN of the pre-filled workspace survives: every element of [S,Bm,H,W,Cout] is stored"""
    ws, y = _run_case(c, S, monkeypatch)
    want_ws, want = c.partials(S), c.expected(S)
    assert tuple(ws.shape) == want_ws.shape and ws.dtype == torch.float32
    assert not bool(torch.isnan(ws).any()), int(torch.isnan(ws).sum())
    got, exp = _bits(ws), R.f32_bits(want_ws + 0.)          # + 0.: the sums hold no -0.0 and neither may the reference
    assert np.array_equal(got, exp), (c.name, S, int((got != exp).sum()), got.size)
    assert y.dtype == torch.float32 and tuple(y.shape) == want.shape
    got, exp = _bits(y), R.f32_bits(want)
    assert np.array_equal(got, exp), (c.name, S, int((got != exp).sum()), got.size)


def test_split_k_invariance_and_library_choice(monkeypatch):
    """exact data: every slicing of Cin = 64 gives the same bits; ksplit=None is the library's S passed explicitly"""
    from witw_amd import _lib
    from witw_amd import baseline_bf16 as bb
    c = A.case('k64')
    ys = [_run_case(c, S, monkeypatch)[1] for S in (1, 2, 3, 4)]
    for y in ys[1:]:
        assert torch.equal(_bits_t(y), _bits_t(ys[0]))
    r = np.random.RandomState(3)
    x = _bf16(R.bf16_round(r.normal(size=(c.Bm, c.g * c.h, c.g * c.w, 256))))
    pk = bb.PackedConvBf16Taps4(_f32(r.normal(size=(24, 256, 3, 3))), _f32(r.normal(size=24)))
    S = _lib.load().witw_conv3x3_bf16_taps4_ksplit(c.Bm, c.g * c.h, c.g * c.w, 256, 24)
    assert 1 <= S <= 16
    auto = bb.conv_taps4_splitk_bf16(x, pk, c.n_images, c.g, c.valid)
    assert torch.equal(_bits_t(auto), _bits_t(bb.conv_taps4_splitk_bf16(x, pk, c.n_images, c.g, c.valid, ksplit=S)))
    if S > 1:       # N(0,1) data: another slicing rounds differently, so the comparison above can tell
        assert not torch.equal(_bits_t(auto), _bits_t(bb.conv_taps4_splitk_bf16(x, pk, c.n_images, c.g, c.valid, ksplit=1)))


@pytest.mark.parametrize('B,H,W,C,g', A.RELAYOUT_SHAPES)
def test_relayout_bf16_is_the_fp32_entry_rounded(B, H, W, C, g):
    from witw_amd import baseline_bf16 as bb
    from witw_amd import ops
    y = _f32(A.relayout_data(B, H, W, C))
    m32 = ops.space_to_depth2_mosaic(y, g)
    m16 = bb.space_to_depth2_mosaic_bf16(y, g)
    assert m16.dtype == torch.bfloat16 and m16.shape == m32.shape
    want = R.bf16_bits(R.bf16_round(m32.cpu().numpy().astype(np.float64)) + 0.)
    assert np.array_equal(_bits(m16), want)
    assert np.array_equal(_bits(m16), R.bf16_bits(A.s2d_mosaic(A.relayout_data(B, H, W, C), g) + 0.))      # and the float64 restatement


@pytest.mark.parametrize('n_images,g,h,w,valid', [(1, 1, 15, 15, (14, 14)), (4, 2, 7, 7, (6, 6))], ids=['15x15_g1', '14x14_g2'])
def test_random_operands_at_the_workloads_k(n_images, g, h, w, valid):
    """N(0,1) bf16 operands, Cin = 2048, Cout = 128, library-chosen S, against float64 on the same rounded operands. The fp32 output is
    held to the distance test_baseline_bf16_gpu.test_random_operands_within_one_bf16_ulp holds its fp32 store to: 2^-7 of the larger
    magnitude plus 1e-5 of the largest output."""
    from witw_amd import baseline_bf16 as bb
    r = np.random.RandomState(31)
    Cin, Cout = 2048, 128
    x = R.bf16_round(r.normal(size=(1, g * h, g * w, Cin)))
    k3 = R.bf16_round(r.normal(size=(Cout, Cin, 3, 3)))
    bias, scale, shift = (np.float32(t).astype(np.float64) for t in (r.normal(size=Cout), r.normal(1, 0.3, size=Cout), r.normal(size=Cout)))
    ref = torch.from_numpy(A.finish(A.splitk_partials(x, k3, 1), bias, 0.2, scale, shift, n_images, g, valid)).float()
    pk = bb.PackedConvBf16Taps4(_f32(k3), _f32(bias))
    got = bb.conv_taps4_splitk_bf16(_bf16(x), pk, n_images, g, valid, lrelu_slope=0.2, post_scale=_f32(scale), post_shift=_f32(shift)).cpu()
    S = bb._lib.load().witw_conv3x3_bf16_taps4_ksplit(1, g * h, g * w, Cin, Cout)
    print('S = %d: worst |got - ref| %.3g, largest output %.3g' % (S, float((got - ref).abs().max()), float(ref.abs().max())))
    bad = (got - ref).abs() > 2.0 ** -7 * torch.maximum(ref.abs(), got.abs()) + 1e-5 * float(ref.abs().max())
    assert not bool(bad.any()), int(bad.sum())


# ----------------------------------------------------------------------------- encoder
def _load(enc, params):
    with torch.no_grad():
        for i, q in enumerate(params, 1):
            conv, bn = getattr(enc, 'conv%d' % i), getattr(enc, 'bn%d' % i)
            conv.weight.copy_(torch.from_numpy(q['w']))
            conv.bias.copy_(torch.from_numpy(q['b']))
            bn.weight.copy_(torch.from_numpy(q['gamma']))
            bn.bias.copy_(torch.from_numpy(q['beta']))
            bn.running_mean.copy_(torch.from_numpy(q['mean']))
            bn.running_var.copy_(torch.from_numpy(q['var']))
    return enc.eval()


def _encoder(precision, params):
    from witw_amd import cvig_baseline as cb
    return _load(cb.SurfaceEncoder(precision=precision).to(DEV), params)


def _record(monkeypatch, fn):
    """-> (result, [(C entry, instantiation it registered)]) of the launches inside fn()"""
    from witw_amd import _lib, ops
    log, check = [], _lib.check
    with monkeypatch.context() as m:
        m.setattr(_lib, 'check', lambda rc, what='': (check(rc, what), log.append((what, ops.last_kernel_variant())))[0])
        out = fn()
    return out, log


@pytest.fixture(scope='module')
def enc_case():
    params = R.make_params(41)
    xs = {(2, 382, 382): synth.images_u8(81, 0, (2, 3, 382, 382)).astype(np.float32), (1, 383, 397): synth.images_u8(82, 0, (1, 3, 383, 397)).astype(np.float32)}
    refs = {k: A.encoder_forward_all(v, params) for k, v in xs.items()}
    return params, xs, refs


@pytest.mark.parametrize('shape', [(2, 382, 382), (1, 383, 397)], ids=['2x382x382', '1x383x397'])
def test_encoder_embedding_and_launch_record(enc_case, shape, monkeypatch):
    params, xs, refs = enc_case
    x = torch.from_numpy(xs[shape]).to(DEV)
    e32, _log32 = _record(monkeypatch, lambda: _encoder('fp32', params)(x))
    e16, log16 = _record(monkeypatch, lambda: _encoder('bf16', params)(x))
    eall, log = _record(monkeypatch, lambda: _encoder('bf16_all', params)(x))
    ref = refs[shape]
    got = eall.double().cpu().numpy()
    n = np.linalg.norm(ref, axis=1)
    dev = np.linalg.norm(got - ref, axis=1) / n
    d32 = np.linalg.norm(got - e32.double().cpu().numpy(), axis=1) / n
    d16 = np.linalg.norm(got - e16.double().cpu().numpy(), axis=1) / n
    print('bf16_all encoder %s: %.3e of the norm from the bf16_all reference, %.3e from the fp32 encoder, %.3e from the bf16 encoder'
          % (shape, dev.max(), d32.max(), d16.max()))
    assert dev.max() <= 1e-2
    names = [w for w, _v in log]
    assert [v for w, v in log if w == 'witw_conv4x4s2_first_fwd_bf16'] == ['conv4x4s2_first_kernel<3,true>']
    assert [v for w, v in log if w == 'witw_conv3x3_bf16_fwd_taps4'] == ['conv_taps4_bf16_kernel<false>'] * 3          # block 4 stores bf16 too
    assert [v for w, v in log if w == 'witw_conv3x3_bf16_fwd_taps4_splitk'] == [KERNEL] * 3
    assert names.count('witw_taps4_splitk_finish') == 3
    assert 'witw_conv3x3_fwd_taps4_ex' not in names and 'witw_space_to_depth2_mosaic' not in names
    assert names.count('witw_space_to_depth2_mosaic_bf16') == 2
    # 'bf16' is what it was: block 4 stores fp32, blocks 5-7 run the fp32 split-K launches
    assert [v for w, v in log16 if w == 'witw_conv3x3_bf16_fwd_taps4'] == ['conv_taps4_bf16_kernel<false>'] * 2 + ['conv_taps4_bf16_kernel<true>']
    n16 = [w for w, _v in log16]
    assert n16.count('witw_conv3x3_fwd_taps4_ex') == 3 and 'witw_conv3x3_bf16_fwd_taps4_splitk' not in n16
    assert n16.count('witw_space_to_depth2_mosaic') == 2 and 'witw_space_to_depth2_mosaic_bf16' not in n16


def _block_shapes(B, H, W):
    """(Bm, mosaic H, mosaic W) of the inputs of blocks 5-7 for a batch of B images of H x W"""
    vh, vw, g, out = H, W, 1, []
    for i in range(1, 8):
        vh, vw = (vh - 4) // 2 + 1, (vw - 4) // 2 + 1
        if i >= 4 and i < 7:
            nh, nw = (vh + 1) // 2, (vw + 1) // 2
            g = 1 if i == 4 else max(1, min(16 // nh, 16 // nw))
            out.append((-(-B // (g * g)), g * nh, g * nw))
    return out


def test_encoder_is_batch_independent(enc_case):
    """image 0 of B = 1 and of B = 3: equal bits. The split-K factor decides the order of the sum, so the library must answer the same S
    for both batch sizes at each of the three block shapes (it does: few workgroups either way, S at its cap)."""
    from witw_amd import _lib
    params, xs, _refs = enc_case
    lib = _lib.load()
    for s1, s3 in zip(_block_shapes(1, 383, 397), _block_shapes(3, 383, 397)):
        assert lib.witw_conv3x3_bf16_taps4_ksplit(*s1, 2048, 512) == lib.witw_conv3x3_bf16_taps4_ksplit(*s3, 2048, 512), (s1, s3)
    enc = _encoder('bf16_all', params)
    x1 = torch.from_numpy(xs[(1, 383, 397)]).to(DEV)
    x3 = torch.cat([x1, torch.from_numpy(synth.images_u8(83, 0, (2, 3, 383, 397)).astype(np.float32)).to(DEV)])
    e1, e3 = enc(x1), enc(x3)
    assert torch.equal(_bits_t(e1[0]), _bits_t(e3[0]))
    assert torch.equal(_bits_t(enc(x3[2:3].contiguous())[0]), _bits_t(e3[2]))


def test_weight_version_cache(enc_case):
    """an in-place change of conv6.weight, then a C-ABI Adam step on conv5 / conv7 (which torch's version counters cannot see): the next
    forward uses the new filters -- the same bits as a fresh encoder with those weights. No fp32 image of any block is ever packed."""
    from witw_amd import cvig_fov
    params, xs, _refs = enc_case
    x = torch.from_numpy(xs[(1, 383, 397)]).to(DEV)
    enc = _encoder('bf16_all', params)
    e0 = enc(x).clone()
    assert all(enc._packed[i][1] is None for i in range(1, 8)) and all(('bf16', i) in enc._packed for i in range(2, 8))

    def fresh():
        f = _encoder('bf16_all', params)
        f.load_state_dict(enc.state_dict())
        return f.eval()(x)
    with torch.no_grad():
        enc.conv6.weight.mul_(1.5)
    e1 = enc(x).clone()
    assert (e1 - e0).abs().max().item() > 1e-4 and torch.equal(_bits_t(e1), _bits_t(fresh()))
    opt = cvig_fov.Adam([enc.conv5.weight, enc.conv7.weight], lr=1e-2)
    for p in (enc.conv5.weight, enc.conv7.weight):
        p.grad = torch.ones_like(p)
    opt.step()
    e2 = enc(x).clone()
    assert (e2 - e1).abs().max().item() > 1e-4 and torch.equal(_bits_t(e2), _bits_t(fresh()))


def test_bf16_all_refuses_training_wide_inputs_and_unknown_precisions():
    from witw_amd import _lib
    from witw_amd import cvig_baseline as cb
    x = torch.zeros((1, 3, 382, 382), device=DEV)
    with pytest.raises(_lib.WitwError, match='fp32 is the only training arithmetic'):
        cb.SurfaceEncoder(precision='bf16_all').to(DEV).train()(x)
    with pytest.raises(_lib.WitwError, match='fused first block'):
        cb.SurfaceEncoder(orientation=True, bands=4, precision='bf16_all').to(DEV).eval()(torch.zeros((1, 6, 382, 382), device=DEV))
    with pytest.raises(_lib.WitwError, match="'fp32', 'bf16' or 'bf16_all'"):
        cb.SurfaceEncoder(precision='bf16_5to7')


def test_wrappers_refuse_wrong_tensors(monkeypatch):
    from witw_amd import _lib, ops
    from witw_amd import baseline_bf16 as bb
    pk = bb.PackedConvBf16Taps4(torch.zeros((8, 16, 3, 3), device=DEV), torch.zeros(8, device=DEV))
    pk6 = bb.PackedConvBf16Taps4(torch.zeros((6, 16, 3, 3), device=DEV), torch.zeros(6, device=DEV))
    pk32 = ops.PackedConv(torch.zeros((8, 16, 3, 3), device=DEV), torch.zeros(8, device=DEV), taps4=True)
    x = torch.zeros((2, 4, 6, 16), dtype=torch.bfloat16, device=DEV)           # a 2 x 2 mosaic of 5..8 cells of 2 x 3
    y = torch.zeros((3, 5, 7, 8), device=DEV)
    with monkeypatch.context() as m:       # every refusal comes before anything is allocated
        m.setattr(bb, 'torch', _NoAllocTorch())
        for bad in (x.cpu(), x.float(), x[..., :8], x.permute(0, 2, 1, 3), x[0]):
            with pytest.raises(_lib.WitwError):
                bb.conv_taps4_splitk_bf16(bad, pk, 5, 2, (1, 2))
        for n_images, g in ((4, 2), (9, 2), (5, 1), (5, 4), (5, 0)):
            with pytest.raises(_lib.WitwError, match='mosaic'):
                bb.conv_taps4_splitk_bf16(x, pk, n_images, g, (1, 2))
        with pytest.raises(_lib.WitwError, match='PackedConvBf16Taps4'):
            bb.conv_taps4_splitk_bf16(x, pk32, 5, 2, (1, 2))
        with pytest.raises(_lib.WitwError, match='channels'):
            bb.conv_taps4_splitk_bf16(torch.zeros((2, 4, 6, 32), dtype=torch.bfloat16, device=DEV), pk, 5, 2, (1, 2))
        with pytest.raises(_lib.WitwError, match='multiple of 4'):
            bb.conv_taps4_splitk_bf16(x, pk6, 5, 2, (1, 2))
        with pytest.raises(_lib.WitwError):
            bb.conv_taps4_splitk_bf16(x, pk, 5, 2, (1, 2), post_scale=torch.ones(8, device=DEV))
        for bad_valid in ((3, 2), (1, 0), (2, 4)):
            with pytest.raises(_lib.WitwError, match='valid region'):
                bb.conv_taps4_splitk_bf16(x, pk, 5, 2, bad_valid)
        for bad_s in (0, 2, -1):
            with pytest.raises(_lib.WitwError, match='ksplit'):
                bb.conv_taps4_splitk_bf16(x, pk, 5, 2, (1, 2), ksplit=bad_s)
        for bad in (y.cpu(), y.bfloat16(), y[..., :4], y[0], torch.zeros((3, 5, 7, 6), device=DEV)):
            with pytest.raises(_lib.WitwError):
                bb.space_to_depth2_mosaic_bf16(bad, 2)
        for bad_g in (0, 65):
            with pytest.raises(_lib.WitwError):
                bb.space_to_depth2_mosaic_bf16(y, bad_g)
    assert bb.conv_taps4_splitk_bf16(x, pk, 5, 2, (1, 2)).shape == (5, 1, 2, 8)          # the same arguments, all right: it runs
    lib = _lib.load()
    for args in ((0, 15, 15, 2048, 512), (1, 15, 15, 2040, 512), (1, 15, 15, 2048, 0)):
        assert lib.witw_conv3x3_bf16_taps4_ksplit(*args) == -1


class _NoAllocTorch(object):
    """stand-in for `torch` inside baseline_bf16 while a refusal is expected: an allocation is a failure"""

    def __getattr__(self, name):
        if name in ('empty', 'zeros', 'empty_like', 'zeros_like'):
            raise AssertionError('allocated before refusing')
        return getattr(torch, name)


# ----------------------------------------------------------------------------- driver
def _write_baseline_dataset(root, n):
    from PIL import Image
    rows = []
    for i in range(n):
        Image.fromarray(synth.images_u8(72, i, (400, 400, 3)).astype(np.uint8)).save(os.path.join(root, 'ov_%d.png' % i))
        Image.fromarray(synth.images_u8(73, i, (200, 800, 3)).astype(np.uint8)).save(os.path.join(root, 'su_%d.png' % i))
        rows.append('ov_%d.png,su_%d.png' % (i, i))
    with open(os.path.join(root, 'pairs.csv'), 'w') as f:
        f.write('\n'.join(rows) + '\n')
    return os.path.join(root, 'pairs.csv')


def test_test_driver_on_bf16_all(tmp_path, monkeypatch, capsys):
    """test(precision='bf16_all') runs to the recall table over encoders of that precision"""
    from witw_amd import cvig_baseline as cb
    csv = _write_baseline_dataset(str(tmp_path), 4)
    monkeypatch.chdir(tmp_path)
    os.makedirs('weights')
    torch.manual_seed(7)
    su, ov = cb.SurfaceEncoder(), cb.OverheadEncoder()
    for e in (su, ov):
        for i in range(1, 8):
            getattr(e, 'bn%d' % i).running_var.uniform_(0.05, 0.3)
    torch.save(su.state_dict(), 'weights/surface_best.pth')
    torch.save(ov.state_dict(), 'weights/overhead_best.pth')
    seen = []
    real = cb.ranks
    monkeypatch.setattr(cb, 'ranks', lambda o, s: (seen.append((o.clone(), s.clone())), real(o, s))[1])
    turn = cb.SyncedRotation.__call__
    monkeypatch.setattr(cb.SyncedRotation, '__call__', lambda self, data, angle=None: turn(self, data, 0.))      # the driver's only random step
    (table, log) = _record(monkeypatch, lambda: cb.test(dataset='cvusa', batch_size=4, num_workers=0, csv_path=csv, precision='bf16_all'))
    out = capsys.readouterr().out
    assert 'Top  1:' in out and 'Locations: 4' in out and 0 <= table['top_1'] <= 100
    names = [w for w, _v in log]
    assert names.count('witw_conv3x3_bf16_fwd_taps4_splitk') >= 6 and 'witw_conv3x3_fwd_taps4_ex' not in names      # two encoders, one batch
    ds = cb.ImagePairDataset('cvusa', csv)
    prep = cb.GpuPreprocess('cvusa')
    su16, ov16 = cb.SurfaceEncoder(precision='bf16_all').to(DEV).eval(), cb.OverheadEncoder(precision='bf16_all').to(DEV).eval()
    su16.load_state_dict(su.state_dict())
    ov16.load_state_dict(ov.state_dict())
    data = prep({'surface': [ds[i]['surface'] for i in range(4)], 'overhead': [ds[i]['overhead'] for i in range(4)]})
    (o, s), = seen
    assert torch.equal(_bits_t(s), _bits_t(su16(data['surface']))) and torch.equal(_bits_t(o), _bits_t(ov16(data['overhead'])))


def test_cli_accepts_bf16_all_in_test_mode_only(monkeypatch):
    from witw_amd import cvig_baseline as cb
    calls = []
    monkeypatch.setattr(cb._fov, 'init_distributed', lambda: None)
    monkeypatch.setattr(cb, 'test', lambda **kw: calls.append(kw))
    monkeypatch.setattr(cb, 'train', lambda **kw: calls.append(kw))
    cb.main(['--mode', 'test', '--precision', 'bf16_all'])
    assert calls == [dict(dataset='cvusa', match_method=None, precision='bf16_all')]
    with pytest.raises(SystemExit):
        cb.main(['--mode', 'train', '--precision', 'bf16_all'])
    assert len(calls) == 1


# ----------------------------------------------------------------------------- memory contract
@pytest.mark.parametrize('skew', [0, 16])
@pytest.mark.parametrize('name', ['ragged_17x18', 'mosaic_g5', 'cout12'])
def test_memory_contract_of_the_wrappers(name, skew, monkeypatch):
    """conv_taps4_splitk_bf16 and space_to_depth2_mosaic_bf16 between guard bands (tests/mem_arena.py): inputs inside NaN bands, every
    device allocation of the wrappers (workspace included) inside bands with a canary payload. No band is touched, every element of the
    workspace and of the outputs is stored, the inputs are unchanged and the values are those of ordinary allocations, bit for bit."""
    from witw_amd import baseline_bf16 as bb
    c = A.case(name)
    S = c.ksplits[-1]
    x, k3, bias, scale, shift = c.data()
    pk = bb.PackedConvBf16Taps4(_f32(k3), _f32(bias))
    inputs = dict(x=_bf16(x))
    if scale is not None:
        inputs.update(scale=_f32(scale), shift=_f32(shift))

    def call(p):
        y = bb.conv_taps4_splitk_bf16(p['x'], pk, c.n_images, c.g, c.valid, lrelu_slope=c.slope, post_scale=p.get('scale'), post_shift=p.get('shift'),
                                      ksplit=S)
        g = max(1, min(16 // ((c.valid[0] + 1) // 2), 16 // ((c.valid[1] + 1) // 2), 5))
        return y, bb.space_to_depth2_mosaic_bf16(y, g)
    plain = [t.clone() for t in call(inputs)]
    arena = Arena(DEV, skew_bytes=skew)
    with monkeypatch.context() as m:
        m.setattr(bb, 'torch', ArenaTorch(arena))
        placed = {k: arena.place(t, k) for k, t in inputs.items()}
        got = call(placed)
        made = [a.tensor for a in arena.live if a.kind == 'empty']
    assert len(made) == 3 and tuple(made[0].shape) == (S, c.Bm, c.g * c.h, c.g * c.w, c.Cout)      # workspace, y, mosaic
    arena.check(made)
    for a, b in zip(got, plain):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for k, t in inputs.items():
        assert torch.equal(placed[k].view(torch.uint8), t.view(torch.uint8)), k
