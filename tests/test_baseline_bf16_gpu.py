"""cvig_baseline's bf16 inference path on the GPU against tests/baseline_bf16_ref.py (float64, rounded where the product rounds).

    witw_conv3x3_bf16_fwd_taps4 / _pack_weights_taps4    exact cases (ref.CASES: equality through an integer view, instantiation
                                                         asserted), nearest-even at the pack and at the store, N(0,1) data to 1 bf16 ulp
    witw_conv4x4s2_first_fwd_bf16                        bit for bit the fp32 entry's output rounded to bf16
    SurfaceEncoder(precision='bf16')                     1e-2 of the reference embedding's norm, launch record, batch independence,
                                                         weight-version cache, the test() driver
    memory contract                                      every new wrapper between guard bands (tests/mem_arena.py)

Tile of conv_taps4_bf16_kernel: 8 rows x 32 columns x 128 output channels, K chunks of 16 input channels: ref.CASES names the shapes.
tests/test_baseline_bf16_ref.py proves on the CPU that the exact cases tell twelve wrong kernels from the right one."""
import os

import numpy as np
import pytest
import torch

from witw_amd import synth
from tests import baseline_bf16_ref as R
from tests.mem_arena import Arena, ArenaTorch
from tests.test_large_grid_parity_gpu import _assert_bf16_ulp

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
NAME = {False: 'conv_taps4_bf16_kernel<false>', True: 'conv_taps4_bf16_kernel<true>'}


def _f32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _bf16(a):
    """values that ARE bf16 numbers -> a bfloat16 tensor"""
    R.bf16_bits(a)
    return _f32(a).to(torch.bfloat16)


def _bits(t):
    t = t.contiguous().cpu()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()]).numpy().view({4: np.uint32, 2: np.uint16}[t.element_size()])


def _run(x, k3, bias, scale, shift, slope, valid, out_f32):
    from witw_amd import baseline_bf16 as bb
    from witw_amd import ops
    pk = bb.PackedConvBf16Taps4(_f32(k3), _f32(bias))
    y = bb.conv_taps4_s2d_bf16(_bf16(x), pk, valid, lrelu_slope=slope, post_scale=_f32(scale), post_shift=_f32(shift), out_f32=out_f32)
    assert ops.last_kernel_variant() == NAME[out_f32]
    return y


@pytest.mark.parametrize('c', R.CASES, ids=[c.name for c in R.CASES])
def test_exact_cases_equal_float64(c):
    x, k3, bias, scale, shift = c.data()
    # every partial sum of any order is an integer of magnitude <= NZ + 2 = 8: exact in fp32 and, through the epilogue, in bf16
    assert R.l1_bound(x, k3, bias) <= c.NZ + 2
    pre = R.preact(x, k3, bias)[:, :c.valid[0], :c.valid[1]]
    assert (pre > 0).mean() >= 0.25 and (pre < 0).mean() >= 0.25, ((pre > 0).mean(), (pre < 0).mean())
    want = c.expected()
    assert np.array_equal(R.bf16_round(want), want)          # also the fp32-out cases hold bf16 numbers only
    y = _run(x, k3, bias, scale, shift, c.slope, c.valid, c.out_f32)
    assert y.dtype == (torch.float32 if c.out_f32 else torch.bfloat16) and tuple(y.shape) == want.shape
    got, exp = _bits(y), R.out_bits(want, c.out_f32)
    assert np.array_equal(got, exp), (c.name, int((got != exp).sum()), got.size)


def test_pack_image_is_nearest_even():
    """all slots of the documented image, filters carrying factors below, on and above a bf16 tie; ragged Cout and Cin (zero fill)"""
    from witw_amd import baseline_bf16 as bb
    _x, k3 = R.rounding_case()[:2]
    r = np.random.RandomState(5)
    for w in (k3, k3[:, :40], np.concatenate([k3] * 4)[:136, :24] * r.choice([1., 3., 0.375], size=(136, 24, 1, 1))):
        pk = bb.PackedConvBf16Taps4(_f32(w), _f32(np.zeros(w.shape[0])))
        want = R.pack_taps4(w)
        assert pk.wpk.numel() == want.size and pk.cin_pad == want.shape[1] * 16
        assert np.array_equal(_bits(pk.wpk).reshape(want.shape), R.bf16_bits(want))


@pytest.mark.parametrize('out_f32', [False, True])
def test_store_rounds_once_to_nearest_even(out_f32):
    x, k3, bias, scale, shift, slope, valid = R.rounding_case()
    want = R.conv_taps4(x, k3, bias, slope, scale, shift, valid, out_f32)
    if not out_f32:      # the case means something: ties are there, and half-up or truncated filters would answer differently
        assert not np.array_equal(want, R.conv_taps4(x, k3, bias, slope, scale, shift, valid, False, 'double_round'))
        assert not np.array_equal(want, R.conv_taps4(x, k3, bias, slope, scale, shift, valid, False, 'trunc_filters'))
    y = _run(x, k3, bias, scale, shift, slope, valid, out_f32)
    got, exp = _bits(y), R.out_bits(want, out_f32)
    assert np.array_equal(got, exp), (int((got != exp).sum()), got.size)


@pytest.mark.parametrize('affine', [False, True])
@pytest.mark.parametrize('C', [3, 5])
def test_first_block_bf16_is_the_fp32_entry_rounded(C, affine):
    from witw_amd import ops
    r = np.random.RandomState(20 + C)
    x = _f32(r.randint(0, 256, size=(2, C, 383, 390)))
    w, b = _f32(r.normal(0, 0.02, (64, C, 4, 4))), _f32(r.normal(0, 0.02, 64))
    sc, sh = (_f32(r.normal(1, 0.3, 64)), _f32(r.normal(0, 0.3, 64))) if affine else (None, None)
    y32 = ops.conv4x4s2_first(x, w, b, sc, sh)
    assert ops.last_kernel_variant() == 'conv4x4s2_first_kernel<%d>' % C
    y16 = ops.conv4x4s2_first(x, w, b, sc, sh, out_bf16=True)
    assert ops.last_kernel_variant() == 'conv4x4s2_first_kernel<%d,true>' % C
    assert y16.dtype == torch.bfloat16 and y16.shape == y32.shape
    want = R.bf16_bits(R.bf16_round(y32.cpu().numpy().astype(np.float64)))
    assert np.array_equal(_bits(y16), want)


@pytest.mark.parametrize('B,H,W,Cin,Cout,valid,out_f32', [(2, 19, 37, 48, 136, (18, 36), False), (1, 12, 35, 256, 128, (11, 33), False),
                                                          (1, 12, 35, 256, 128, (11, 33), True), (1, 9, 33, 1024, 24, (8, 32), False)])
def test_random_operands_within_one_bf16_ulp(B, H, W, Cin, Cout, valid, out_f32):
    """N(0,1) bf16 operands against float64 on the same rounded operands, by the project's form of 'one bf16 ulp'
    (test_large_grid_parity_gpu._assert_bf16_ulp): 2^-7 of the larger magnitude plus 1e-5 of the largest output next to zero, and
    more than 97 % of the bf16 outputs EQUAL to the rounded reference. The fp32 store is held to the same distance from the unrounded
    reference (nothing is rounded there, so no equality share)."""
    r = np.random.RandomState(31)
    x = R.bf16_round(r.normal(size=(B, H, W, Cin)))
    k3 = R.bf16_round(r.normal(size=(Cout, Cin, 3, 3)))
    bias, scale, shift = r.normal(size=Cout), r.normal(1, 0.3, size=Cout), r.normal(size=Cout)
    bias, scale, shift = (np.float32(t).astype(np.float64) for t in (bias, scale, shift))
    ref = torch.from_numpy(R.conv_taps4(x, k3, bias, 0.2, scale, shift, valid, out_f32=True)).float()      # before any store rounding
    got = _run(x, k3, bias, scale, shift, 0.2, valid, out_f32).float().cpu()
    if out_f32:
        bad = (got - ref).abs() > 2.0 ** -7 * torch.maximum(ref.abs(), got.abs()) + 1e-5 * float(ref.abs().max())
        print('fp32 store: worst |got - ref| %.3g, largest output %.3g' % (float((got - ref).abs().max()), float(ref.abs().max())))
        assert not bool(bad.any()), int(bad.sum())
    else:
        r16 = ref.bfloat16().float()
        print('bf16 store: %.4f of the outputs equal the rounded reference, worst |got - r16| %.3g, largest output %.3g'
              % (float((got == r16).float().mean()), float((got - r16).abs().max()), float(r16.abs().max())))
        _assert_bf16_ulp(got, ref)


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
    return _load(cb.SurfaceEncoder(**({} if precision is None else {'precision': precision})).to(DEV), params)


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
    refs = {k: R.encoder_forward(v, params) for k, v in xs.items()}
    return params, xs, refs


@pytest.mark.parametrize('shape', [(2, 382, 382), (1, 383, 397)], ids=['2x382x382', '1x383x397'])
def test_encoder_embedding_and_launch_record(enc_case, shape, monkeypatch):
    params, xs, refs = enc_case
    x = torch.from_numpy(xs[shape]).to(DEV)
    e32, log32 = _record(monkeypatch, lambda: _encoder('fp32', params)(x))
    e16, log16 = _record(monkeypatch, lambda: _encoder('bf16', params)(x))
    ref = refs[shape]
    got = e16.double().cpu().numpy()
    dev = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
    d32 = np.linalg.norm(got - e32.double().cpu().numpy(), axis=1) / np.linalg.norm(ref, axis=1)
    print('bf16 encoder %s: %.3e of the norm from the bf16 reference, %.3e from the fp32 encoder' % (shape, dev.max(), d32.max()))
    assert dev.max() <= 1e-2
    assert [v for w, v in log16 if w == 'witw_conv4x4s2_first_fwd_bf16'] == ['conv4x4s2_first_kernel<3,true>']
    assert [v for w, v in log16 if w == 'witw_conv3x3_bf16_fwd_taps4'] == [NAME[False], NAME[False], NAME[True]]      # blocks 2, 3, 4
    assert not [w for w, _v in log32 if 'bf16' in w]
    splitk16 = [v for w, v in log16 if w == 'witw_conv3x3_fwd_taps4_ex']
    splitk32 = [v for w, v in log32 if w == 'witw_conv3x3_fwd_taps4_ex']
    assert len(splitk16) == 3 and splitk16 == splitk32[-3:]          # blocks 5-7 run what they run in fp32
    none = _encoder(None, params)(x)
    assert torch.equal(_bits_t(none), _bits_t(e32))                   # precision='fp32' is the encoder built without the argument


def _bits_t(t):
    return t.contiguous().view(torch.int32)


def test_encoder_is_batch_independent(enc_case):
    params, xs, _refs = enc_case
    enc = _encoder('bf16', params)
    x1 = torch.from_numpy(xs[(1, 383, 397)]).to(DEV)
    x3 = torch.cat([x1, torch.from_numpy(synth.images_u8(83, 0, (2, 3, 383, 397)).astype(np.float32)).to(DEV)])
    e1, e3 = enc(x1), enc(x3)
    assert torch.equal(_bits_t(e1[0]), _bits_t(e3[0]))
    assert torch.equal(_bits_t(enc(x3[2:3].contiguous())[0]), _bits_t(e3[2]))


def test_weight_version_cache(enc_case):
    """an in-place weight change, then a C-ABI Adam step (which torch's version counters cannot see): the next bf16 forward uses
    the new filters -- the same bits as a fresh encoder with those weights"""
    from witw_amd import cvig_fov
    params, xs, _refs = enc_case
    x = torch.from_numpy(xs[(1, 383, 397)]).to(DEV)
    enc = _encoder('bf16', params)
    e0 = enc(x).clone()

    def fresh():
        f = _encoder('bf16', params)
        f.load_state_dict(enc.state_dict())
        return f.eval()(x)
    with torch.no_grad():
        enc.conv3.weight.mul_(1.5)
    e1 = enc(x).clone()
    assert (e1 - e0).abs().max().item() > 1e-4 and torch.equal(_bits_t(e1), _bits_t(fresh()))
    opt = cvig_fov.Adam([enc.conv2.weight, enc.conv4.weight], lr=1e-2)
    for p in (enc.conv2.weight, enc.conv4.weight):
        p.grad = torch.ones_like(p)
    opt.step()
    e2 = enc(x).clone()
    assert (e2 - e1).abs().max().item() > 1e-4 and torch.equal(_bits_t(e2), _bits_t(fresh()))


def test_bf16_refuses_training_and_wide_inputs(enc_case):
    from witw_amd import _lib
    from witw_amd import cvig_baseline as cb
    x = torch.zeros((1, 3, 382, 382), device=DEV)
    with pytest.raises(_lib.WitwError, match='fp32 is the only training arithmetic'):
        cb.SurfaceEncoder(precision='bf16').to(DEV).train()(x)
    with pytest.raises(_lib.WitwError, match='fused first block'):
        cb.SurfaceEncoder(orientation=True, bands=4, precision='bf16').to(DEV).eval()(torch.zeros((1, 6, 382, 382), device=DEV))


def test_wrappers_refuse_wrong_tensors():
    from witw_amd import _lib, ops
    from witw_amd import baseline_bf16 as bb
    pk = bb.PackedConvBf16Taps4(torch.zeros((8, 16, 3, 3), device=DEV), torch.zeros(8, device=DEV))
    x = torch.zeros((1, 4, 4, 16), dtype=torch.bfloat16, device=DEV)
    for bad in (x.cpu(), x.float(), x[..., :8], x.permute(0, 2, 1, 3)[:, :, :3]):
        with pytest.raises(_lib.WitwError):
            bb.conv_taps4_s2d_bf16(bad, pk, (3, 3))
    with pytest.raises(_lib.WitwError):
        bb.conv_taps4_s2d_bf16(x, pk, (3, 3), post_scale=torch.ones(8, device=DEV))
    for bad_valid in ((5, 3), (3, 0), (-1, 3)):
        with pytest.raises(_lib.WitwError, match='valid region'):
            bb.conv_taps4_s2d_bf16(x, pk, bad_valid)
    with pytest.raises(_lib.WitwError):
        bb.PackedConvBf16Taps4(torch.zeros((8, 16, 3, 3)), torch.zeros(8))
    with pytest.raises(_lib.WitwError):
        ops.conv4x4s2_first(torch.zeros((1, 3, 8, 8)), torch.zeros((64, 3, 4, 4), device=DEV), torch.zeros(64, device=DEV), out_bf16=True)


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


def test_test_driver_on_bf16(tmp_path, monkeypatch, capsys):
    """test(precision='bf16') runs to the recall table; the embeddings it ranks are those of direct bf16 encoder calls"""
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
    table = cb.test(dataset='cvusa', batch_size=3, num_workers=0, csv_path=csv, precision='bf16')
    out = capsys.readouterr().out
    assert 'Top  1:' in out and 'Locations: 4' in out and 0 <= table['top_1'] <= 100
    ds = cb.ImagePairDataset('cvusa', csv)
    prep = cb.GpuPreprocess('cvusa')
    su16, ov16 = cb.SurfaceEncoder(precision='bf16').to(DEV).eval(), cb.OverheadEncoder(precision='bf16').to(DEV).eval()
    su16.load_state_dict(su.state_dict())
    ov16.load_state_dict(ov.state_dict())
    want_s, want_o = [], []
    for idx in ([0, 1, 2], [3]):          # the driver's batches
        data = prep({'surface': [ds[i]['surface'] for i in idx], 'overhead': [ds[i]['overhead'] for i in idx]})
        want_s.append(su16(data['surface']))
        want_o.append(ov16(data['overhead']))
    (o, s), = seen
    assert torch.equal(_bits_t(s), _bits_t(torch.cat(want_s))) and torch.equal(_bits_t(o), _bits_t(torch.cat(want_o)))


# ----------------------------------------------------------------------------- memory contract
@pytest.mark.parametrize('skew', [0, 16])
@pytest.mark.parametrize('name', ['tile+1', 'odd_valid', 'small'])
def test_memory_contract_of_the_wrappers(name, skew, monkeypatch):
    """PackedConvBf16Taps4, conv_taps4_s2d_bf16 and conv4x4s2_first(out_bf16=True) between guard bands (tests/mem_arena.py): inputs
    inside NaN bands, every device allocation of the wrapper inside bands with a canary payload. No band is touched, every output
    element is stored, the inputs are unchanged and the values are those of ordinary allocations, bit for bit."""
    from witw_amd import baseline_bf16 as bb
    from witw_amd import ops
    c = [k for k in R.CASES if k.name == name][0]
    x, k3, bias, scale, shift = c.data()
    r = np.random.RandomState(3)
    img = _f32(r.randint(0, 256, size=(2, 3, 37, 70)))
    w1, b1 = _f32(r.normal(0, 0.02, (64, 3, 4, 4))), _f32(r.normal(0, 0.02, 64))
    inputs = dict(x=_bf16(x), k3=_f32(k3), bias=_f32(bias), img=img, w1=w1, b1=b1)
    if scale is not None:
        inputs.update(scale=_f32(scale), shift=_f32(shift))

    def call(p):
        pk = bb.PackedConvBf16Taps4(p['k3'], p['bias'])
        y = bb.conv_taps4_s2d_bf16(p['x'], pk, c.valid, lrelu_slope=c.slope, post_scale=p.get('scale'), post_shift=p.get('shift'), out_f32=c.out_f32)
        f = ops.conv4x4s2_first(p['img'], p['w1'], p['b1'], None, None, out_bf16=True)
        return pk.wpk, y, f
    plain = [t.clone() for t in call(inputs)]
    arena = Arena(DEV, skew_bytes=skew)
    with monkeypatch.context() as m:
        m.setattr(bb, 'torch', ArenaTorch(arena))
        m.setattr(ops, 'torch', ArenaTorch(arena))
        placed = {k: arena.place(t, k) for k, t in inputs.items()}
        got = call(placed)
    arena.check(got)
    for a, b in zip(got, plain):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for k, t in inputs.items():
        assert torch.equal(placed[k].view(torch.uint8), t.view(torch.uint8)), k
