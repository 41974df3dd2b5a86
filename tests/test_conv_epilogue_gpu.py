"""The unpooled conv3x3 launch -- every forward layer without a pool and, on the transposed, tap-rotated filter, every data gradient --
bit for bit against tests/conv_epilogue_ref.py in all three precisions, each case on a named kernel instantiation.

The data makes every kernel exact whatever its summation order (operands in {-1, 0, 1} or +-1 .. +-3, integer bias, scales that are
powers of two or 1.25), so every comparison of the table's cases is an equality through an integer view: bias -> Dropout2d scale ->
activation -> affine -> gate, the gate a select that is open exactly where gate > 0 and leaves +0.0 where it is closed, the dilated
rows on the even rows, the filter transposed AND rotated. tests/test_conv_epilogue_ref.py proves on the CPU that each of those mistakes
would change the expected bits of every case it applies to; the table in tests/conv_epilogue_ref.py names the store each case reaches.

One block per precision at the end runs Gaussian data under the bounds the suite already holds these kernels to
(tests/test_large_grid_parity_gpu.py, tests/test_f16x3_gpu.py)."""
import numpy as np
import pytest
import torch

from tests import conv_epilogue_ref as R
from tests import pool_ref as P
from tests.test_large_grid_parity_gpu import _assert_bf16_ulp
from tests.test_pool_codes_gpu import _bits, _nhwc, _want_split, _waves

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def _cu():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def _f32(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)


def _packed(ops, prec, w, b, flip, **kw):
    cls = {'f32': ops.PackedConv, 'bf16': ops.PackedConvBf16, 'f16': ops.PackedConvF16x3}[prec]
    return cls(_f32(w), None if b is None else _f32(b), transpose_flip=flip, **kw)


def _input(ops, prec, a_nchw):
    """activations in the launch's input layout (exact: small integers)"""
    if prec == 'f16':
        return ops.nchw_to_split_f16(_f32(a_nchw), a_nchw.shape[1])
    x = _f32(_nhwc(a_nchw))
    return x.bfloat16() if prec == 'bf16' else x


def _gate_host(prec, g_nchw, nchw):
    """the gate in the output's layout and the gate's own format, as numpy: fp32 values, or the int16 bit patterns of bf16 [..,C] /
    split-fp16 [..,C/8,2,8] (subnormals, -0.0, infinities and NaN as they are)"""
    if prec == 'f32':
        return np.array(g_nchw if nchw else _nhwc(g_nchw), dtype=np.float32)
    return R.bf16_bits(_nhwc(g_nchw)) if prec == 'bf16' else R.split_bits(_nhwc(g_nchw))


def _gate_dev(c, d, B, host):
    """host (the gate of the images the reference describes) -> the device gate of the whole batch; the other images of a large batch
    repeat those gates"""
    g = torch.from_numpy(host).to(DEV)
    if d.sel is not None:
        src = torch.arange(B) % len(d.sel)
        src[list(d.sel)] = torch.arange(len(d.sel))
        g = g[src.to(DEV)].contiguous()
    return g if c.prec == 'f32' else g.view(torch.bfloat16 if c.prec == 'bf16' else torch.float16)


def _launch(ops, c, d, pk, x, gate):
    kw = dict(stride_h=c.launch_sh, circular=c.circ, relu=c.act == 'relu', drop_scale=None if d.drop is None else _f32(d.drop),
              gate=gate, dilate_h=c.dilated, out_h=c.out_h)
    if c.prec == 'f32':
        post = {} if d.post_scale is None else dict(post_scale=_f32(d.post_scale), post_shift=_f32(d.post_shift))
        with _waves(c.nw):
            y = ops.conv3x3_fwd(x, pk, out_nchw=c.store == 'nchw', lrelu_slope=R.SLOPE if c.act == 'lrelu' else None, **post, **kw)
    elif c.prec == 'bf16':
        y = ops.conv3x3_bf16_fwd(x, pk, out_nchw_f32=c.store == 'nchw', **kw)
    else:
        y = ops.conv3x3_f16x3_fwd(x, pk, out_nchw_f32=c.store == 'nchw', **kw)
    torch.cuda.synchronize()
    return y, ops.last_kernel_variant(), ops.last_conv_form()


def _switches(ops, c):
    """set what the case's flags ask for -> a function that restores it"""
    from witw_amd import _lib
    lib = _lib.load()
    undo = []
    if c.prec == 'f32':
        prev = lib.witw_conv3x3_dil_skip(0 if 'dilskip0' in c.flags else 1)
        undo.append(lambda: lib.witw_conv3x3_dil_skip(prev))
    if c.prec == 'bf16':
        prev16 = ops.bf16_mfma16('mfma16off' not in c.flags)
        undo.append(lambda: ops.bf16_mfma16(prev16))
        prevw = ops.bf16_wres(True)
        undo.append(lambda: ops.bf16_wres(prevw))
    return lambda: [f() for f in undo]


def _run(ops, c, data_of=None, x=None, gate_edit=None, **pack_kw):
    """-> (the launch's output, the reference's Data). data_of: the case whose operands and answers are used (default: c's own);
    x: another input than the reference's; gate_edit(host gate) -> host gate: what a test changes in the gate before it is uploaded"""
    B = c.batch(_cu())
    d = R.case_data(data_of or c, _cu())
    pk = _packed(ops, c.prec, d.w, d.b, c.site != 'fwd', **pack_kw)
    gate = None
    if c.gate:
        host = _gate_host(c.prec, d.gate, c.store == 'nchw')
        gate = _gate_dev(c, d, B, host if gate_edit is None else gate_edit(host))
    restore = _switches(ops, c)
    try:
        y, variant, form = _launch(ops, c, d, pk, _input(ops, c.prec, d.x if x is None else x), gate)
    finally:
        restore()
    assert variant == c.variant(), (variant, c.variant())
    if c.prec == 'f32':
        assert form == 'direct'
    return y, d


def _check(ops, c, y, d):
    if d.sel is not None:
        y = y[list(d.sel)].contiguous()
    want = d.want if c.store == 'nchw' else _nhwc(d.want)
    if c.store == 'nchw' or c.prec == 'f32':
        assert y.dtype == torch.float32
        np.testing.assert_array_equal(_bits(y), R.f32_bits(want))
    elif c.prec == 'bf16':
        assert y.dtype == torch.bfloat16
        np.testing.assert_array_equal(_bits(y), R.bf16_bits(want))
    else:
        split = R.split_bits(want)
        np.testing.assert_array_equal(_bits(y), split)                                      # hi and lo themselves
        np.testing.assert_array_equal(ops.split_f16_to_f32(y).cpu().numpy(), want.astype(np.float32))      # hi + lo, as values
        if not split[..., 1, :].any() and not np.signbit(want).any():
            np.testing.assert_array_equal(split, _want_split(d.want))                       # the encoder against the pool-code tests'
    if c.prec == 'f16':
        assert not ops.f16x3_overflowed(DEV)


SKIP = [c for c in R.CASES if c.variant().endswith(',8,2,9>')]
TWINS = [c._replace(flags=('dilskip0',)) for c in SKIP]
MAIN = [c for c in R.CASES if c not in SKIP and c not in TWINS]      # those eight: test_fp32_dilated_skip_equals_its_twin


@pytest.mark.parametrize('c', MAIN, ids=[c.id for c in MAIN])
def test_unpooled_epilogue_bits(c):
    from witw_amd import ops
    y, d = _run(ops, c)
    _check(ops, c, y, d)


# ================================================================================ fp32: the zero-row-skipping form and its twin
@pytest.mark.parametrize('c', SKIP, ids=[c.id for c in SKIP])
def test_fp32_dilated_skip_equals_its_twin(c):
    """<128,1,false,8,2,9> does not issue the products with the interleaved zero rows; under witw_conv3x3_dil_skip(0) the same launch
    runs on <128,1,false,8,0,9>: the same bits on the same data, and each the reference's on its own case of the table"""
    from witw_amd import ops
    twin = c._replace(flags=('dilskip0',))
    assert len(SKIP) == 4 and twin in R.CASES and twin.variant() == 'conv3x3_nhwc_f32_kernel<128,1,false,8,0,9>'
    y, d = _run(ops, c)
    _check(ops, c, y, d)
    yt, _d = _run(ops, twin, data_of=c)
    assert torch.equal(y.view(torch.int32), yt.view(torch.int32))
    yt, dt = _run(ops, twin)
    _check(ops, twin, yt, dt)


# ================================================================================ fp32: a Winograd-packed filter under a training epilogue
WINO = [c for c in R.CASES if c.prec == 'f32' and c.site == 'fwd' and c.sh == 1 and c.cout >= 128 and c.W > 32
        and (c.gate or c.post or c.store != 'slab')]


@pytest.mark.parametrize('c', WINO, ids=[c.id for c in WINO])
def test_fp32_wino_packed_filter_runs_direct_form(c):
    """a gate, the post affine, an NCHW output or Cout % 4 != 0 keep a launch off the Winograd form: 'direct', and the plain packing's bits"""
    from witw_amd import ops
    assert ops.conv_wino()
    y, d = _run(ops, c)
    yw, dw = _run(ops, c, wino=True)           # asserts the same instantiation and last_conv_form() == 'direct'
    assert torch.equal(y.view(torch.int32), yw.view(torch.int32))
    _check(ops, c, yw, dw)


def test_fp32_wino_packed_filter_dilated_runs_direct_form_and_plain_takes_wino():
    from witw_amd import ops
    x, w, b = P.exact_operands(77, 2, 8, 128, 4, 64)
    pk, pkw = _packed(ops, 'f32', w, b, False), _packed(ops, 'f32', w, b, False, wino=True)
    xd = _input(ops, 'f32', x)
    with _waves(8):
        out = {}
        for name, p in (('plain', pk), ('wino', pkw)):
            out[name] = ops.conv3x3_fwd(xd, p, relu=False, dilate_h=True, out_h=8)
            assert ops.last_conv_form() == 'direct' and ops.last_kernel_variant() == 'conv3x3_nhwc_f32_kernel<128,1,false,8,2,9>'
        assert torch.equal(out['plain'].view(torch.int32), out['wino'].view(torch.int32))
        xi = np.zeros((2, 8, 8, 64))
        xi[:, :, ::2] = x
        np.testing.assert_array_equal(_bits(out['wino']), R.f32_bits(_nhwc(R.conv(xi, w, b, 1, False))))
        # and the same filter does take the Winograd form where nothing keeps it off: the cases above test the launcher, not the packing
        ops.conv3x3_fwd(_input(ops, 'f32', xi), pkw, relu=True)
        assert ops.last_conv_form() == 'wino_h2'


# ================================================================================ fp32: values that are not finite under a closed gate
def _first(pred):
    return next(c for c in R.CASES if pred(c))


# one case per (channel tile, geometry, store): slab (the gated dgrad), generic and NCHW (gated forwards), each narrow and wide (the
# 64-channel tile on 4 waves, the 128-channel tile on 8)
INF = [_first(lambda c, tn=tn, narrow=narrow, store=store: c.prec == 'f32' and c.gate and c.store == store and c.H * c.W > 1
              and (c.cout >= 128) == (tn == 128) and (c.W <= 32) == narrow and (narrow or c.nw == (4 if tn == 64 else 8))
              and (store != 'slab' or c.site == 'dgrad'))
       for tn in (64, 128) for narrow in (False, True) for store in ('slab', 'generic', 'nchw')]


@pytest.mark.parametrize('c', INF, ids=[c.id for c in INF])
def test_fp32_closed_gate_hides_infinities(c):
    """+-inf in the input makes the conv value +-inf or NaN (inf * 0, inf - inf) over whole neighbourhoods; a closed gate still leaves
    the bits of +0.0 (a product with 0 would leave NaN), an open one the reference's value"""
    from witw_amd import ops
    d = R.case_data(c)
    assert c.act != 'relu'                                  # max(NaN, 0) is not what this test is about
    g = np.random.Generator(np.random.Philox(key=[5, 5]))
    x = np.array(d.x)
    x.reshape(-1)[g.permutation(x.size)[:4]] = [np.inf, -np.inf, np.inf, -np.inf]      # each one poisons its 3 x 3 neighbourhood in every channel
    z = R.dgrad(x, d.w, (c.H, c.W), c.sh, c.circ) if c.site == 'dgrad' else R.conv(x, d.w, d.b, c.sh, c.circ)
    want = R.gate_select(R.epilogue(z, d.drop, c.act, R.SLOPE, d.post_scale, d.post_shift), d.gate)
    opened = d.gate > 0
    assert (~np.isfinite(want[opened])).any() and np.isnan(want).any() and np.isfinite(want[opened]).any()
    y, _d = _run(ops, c, x=x)
    if c.store != 'nchw':
        want, opened = _nhwc(want), _nhwc(opened)
    got, ref, nan = _bits(y), R.f32_bits(want), np.isnan(want)
    assert not got[~opened].any()
    assert np.isnan(y.cpu().numpy()[nan]).all()
    np.testing.assert_array_equal(got[~nan], ref[~nan])


# ================================================================================ bf16 / split-fp16: a NaN gate is closed, as in fp32
# one case per kernel that reads a 16-bit gate: the 4-wave 64- and 128-channel tiles, an 8-wave tile, and for bf16 the 16x16x32
# training form and the weight-resident kernel
NAN16 = [_first(lambda c: 's16' in c.flags), _first(lambda c: 'wres' in c.flags)] + [
    _first(lambda c, prec=prec, tn=tn, big=big: c.prec == prec and c.gate and c.big == big and not set(c.flags) & {'s16', 'wres'}
           and (c.cout >= 128) == (tn == 128) and c.H * c.W > 1)
    for prec in ('bf16', 'f16') for tn, big in ((64, False), (128, False), (128, True))]


@pytest.mark.parametrize('c', NAN16, ids=[c.id for c in NAN16])
def test_16bit_nan_gate_is_closed(c):
    """every ordinary positive gate value becomes a NaN, of either sign and with a payload, in the bf16 gate / the hi half of the
    split-fp16 gate: `gate > 0` is false, the output there is +0.0; +inf, next to it in the integer order, stays open"""
    from witw_amd import ops
    d = R.case_data(c, _cu())
    kind = _nhwc(d.gate_kind)
    nans = np.array([0x7fc1, -0x40 + 3] if c.prec == 'bf16' else [0x7e01, -0x200 + 3], dtype=np.int16)      # sign 0 / sign 1

    def edit(host):
        hi = host if c.prec == 'bf16' else host[..., 0, :]
        k = kind.reshape(hi.shape)
        hi[k == 0] = nans[np.arange(int((k == 0).sum())) & 1]
        assert np.isnan(hi.view(np.float16).astype(np.float32) if c.prec == 'f16' else
                        (hi.view(np.uint16).astype(np.uint32) << 16).view(np.float32))[k == 0].all()
        return host

    want = np.array(_nhwc(d.want))
    assert ((kind == 0) & (want != 0)).any() and ((kind == 7) & (want != 0)).any()
    want[kind == 0] = 0.0
    y, _d = _run(ops, c, gate_edit=edit)
    if d.sel is not None:
        y = y[list(d.sel)].contiguous()
    np.testing.assert_array_equal(_bits(y), R.bf16_bits(want) if c.prec == 'bf16' else R.split_bits(want))


# ================================================================================ Gaussian data under the suite's existing bounds
def _gauss(seed, shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).numpy()


@pytest.mark.parametrize('hw', [(9, 70), (5, 12)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('kind', ['s1', 's2', 'dilated-dgrad'])
@pytest.mark.parametrize('prec', ['f32', 'bf16', 'f16'])
def test_gaussian_within_existing_bounds(prec, kind, hw):
    """fp32: 3e-5 of the output scale; split-fp16: 5e-6 * max(1, scale); bf16: _assert_bf16_ulp, on bf16-rounded operands"""
    from witw_amd import ops
    (H, W), B, cin, cout, circ = hw, 2, 48, 64, hw[1] > 32
    dg = kind == 'dilated-dgrad'
    sh = 1 if kind == 's1' else 2
    x = _gauss(1, (B, cin, (H - 1) // 2 + 1 if dg else H, W))
    w = _gauss(2, (cin, cout, 3, 3) if dg else (cout, cin, 3, 3), 0.05)
    b = None if dg else _gauss(3, (cout,), 0.1)
    if prec == 'bf16':
        x, w = (torch.from_numpy(t).bfloat16().float().numpy() for t in (x, w))
    ref = R.dgrad(x, w, (H, W), 2, circ) if dg else R.forward(x, w, b, sh, circ, act='relu')
    pk = _packed(ops, prec, w, b, dg)
    kw = dict(stride_h=1 if dg else sh, circular=circ, relu=not dg, dilate_h=dg, out_h=H if dg else None)
    fn = {'f32': ops.conv3x3_fwd, 'bf16': ops.conv3x3_bf16_fwd, 'f16': ops.conv3x3_f16x3_fwd}[prec]
    y = fn(_input(ops, prec, x), pk, **kw)
    assert ops.last_kernel_variant() == {'f32': 'conv3x3_nhwc_f32_kernel<64,%d,false,4,%d,9>' % (kw['stride_h'], int(W <= 32)),
                                         'bf16': 'conv3x3_nhwc_bf16_kernel<64,%d,false,4>' % kw['stride_h'],
                                         'f16': 'conv3x3_nhwc_f16x3_kernel<64,%d,false,4>' % kw['stride_h']}[prec]
    scale = float(np.abs(ref).max())
    if prec == 'f32':
        np.testing.assert_allclose(y.cpu().numpy(), _nhwc(ref), rtol=0, atol=3e-5 * scale)
    elif prec == 'f16':
        assert not ops.f16x3_overflowed(DEV)
        np.testing.assert_allclose(ops.split_f16_to_f32(y).cpu().numpy(), _nhwc(ref), rtol=0, atol=5e-6 * max(1.0, scale))
    else:
        _assert_bf16_ulp(y.float().cpu(), torch.from_numpy(_nhwc(ref)).float())
