"""Max-pool arg-max codes and the routing of the pooled gradient, bit for bit, at every place that computes them.

The training backward of the three encoders never stores the unpooled activation: the fused conv + ReLU + max-pool forward writes one
byte per pooled output (dy * 2 + dx of the first maximum in scan order, as torch.max_pool2d picks it) and maxpool2x2_bwd /
maxpool2x2_bwd_bf16 / maxpool2x2_bwd_split place the gradient with it. A wrong byte moves a gradient to a neighbouring pixel; the loss
still falls and a norm-relative tolerance does not notice. The byte is computed independently, each time with its own register-to-pixel
mapping, at every `pool_code` store of csrc/ -- each is named below next to the case that reaches it, and the case asserts the kernel
instantiation, so that a change of launcher thresholds cannot move it elsewhere unnoticed:

    csrc/conv3x3.hip        conv_wino_h2<NW, POOL>                      (a) fp32 'wino'      NW = 4 (the launcher's choice) and 8
                            narrow geometry (GEO = 1)                   (a) fp32 'narrow'    TN 64 / 128, always 4 waves
                            wide, through the LDS slab (Cout % 4 == 0)  (a) fp32 'slab'      TN 64 / 128, 4 and 8 waves
                            wide, generic (ragged Cout)                 (a) fp32 'generic'   TN 64 / 128, 4 and 8 waves
    csrc/conv3x3_bf16.hip   conv3x3_nhwc_bf16_kernel (32x32x16)         (a) bf16 tiled       TN 64 / 128
                            conv3x3_bf16_s16_kernel<true, TRAIN>        (a) bf16 16x16x32    the grid must fill the chip: B = 116
    csrc/conv3x3_f16x3.hip  conv3x3_nhwc_f16x3_kernel                   (a) split-fp16       TN 64 / 128
    csrc/conv_first2_bf16.hip conv_first2_bf16_kernel<CW, false, TRAIN> (a) first two layers CW = 4 and 8

The data (tests/pool_ref.py) makes every kernel exact whatever its summation order -- operands in {-1, 0, 1}, integer bias, |z| <= 128 --
and tests/test_pool_ref.py holds every case below to a minimum of positive windows, of ties at the maximum and of each code. So all
comparisons here are equalities: the pooled output and the routed gradient through an integer view, the codes wherever the window's
maximum is > 0 (where it is <= 0 the ReLU gates the gradient and any code in 0..3 serves).

(b) runs the three scatter kernels alone on arbitrary codes and on gradients that hold -0.0, infinities, NaNs with a payload and
subnormals: a scatter moves bits, and every position it does not write is +0.0."""
import contextlib
import os

import numpy as np
import pytest
import torch

from tests import pool_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


@contextlib.contextmanager
def _waves(nw):
    """force the fp32 conv's workgroup shape (WITW_CONV_NW = 4 / 8), or with None leave the choice to the launcher; restored after"""
    old = os.environ.get('WITW_CONV_NW')
    if nw is None:
        os.environ.pop('WITW_CONV_NW', None)
    else:
        os.environ['WITW_CONV_NW'] = str(nw)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop('WITW_CONV_NW', None)
        else:
            os.environ['WITW_CONV_NW'] = old


def _nhwc(a):
    return np.ascontiguousarray(np.asarray(a).transpose(0, 2, 3, 1))


def _f32(a_nchw):
    """float64 NCHW -> fp32 NHWC on the device (exact: small integers)"""
    return torch.from_numpy(_nhwc(a_nchw).astype(np.float32)).to(DEV)


def _f32_nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _bits(t):
    """a device tensor's bit patterns, as a numpy integer array of the same shape"""
    t = t.contiguous().cpu()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()]).numpy()


def _want_f32(a_nchw):
    return _nhwc(a_nchw).astype(np.float32).view(np.int32)


def _want_bf16(a_nchw):
    return torch.from_numpy(_nhwc(a_nchw).astype(np.float32)).bfloat16().view(torch.int16).numpy()


def _want_split(a_nchw):
    """split-fp16 [B,H,W,C/8,2,8] of values that are fp16 numbers: hi = the value, lo = +0.0"""
    v = _nhwc(a_nchw).astype(np.float16)
    assert np.array_equal(v.astype(np.float64), _nhwc(a_nchw))
    B, H, W, C = v.shape
    out = np.zeros((B, H, W, C // 8, 2, 8), dtype=np.int16)
    out[:, :, :, :, 0, :] = v.view(np.int16).reshape(B, H, W, C // 8, 8)
    return out


def _check_codes(ref, code):
    """every code in 0..3, and the reference's wherever the window's maximum is > 0"""
    assert code.dtype == torch.uint8 and tuple(code.shape) == tuple(_nhwc(ref.code).shape)
    got = code.cpu().numpy().transpose(0, 3, 1, 2)
    assert int(got.max()) <= 3
    pos = ref.m > 0
    np.testing.assert_array_equal(got[pos], ref.code[pos])


def _gated(ref, y_pos):
    """gy where the kernel's own pooled output is > 0 and +0.0 elsewhere (a select: gy * 0 would be -0.0 under a negative gy), fp32 NHWC"""
    gy = _f32(ref.gy)
    return torch.where(y_pos, gy, torch.zeros_like(gy)).contiguous()


# ================================================================================ (a) fp32: csrc/conv3x3.hip
def _fp32_forward(ops, x, pk, circ, nw):
    with _waves(nw):
        y, code = ops.conv3x3_fwd(x, pk, circular=circ, relu=True, pool=True, want_pool_code=True)
        torch.cuda.synchronize()
        return y, code, ops.last_kernel_variant(), ops.last_conv_form()


def _check_fp32(ops, ref, y, code, H, W):
    np.testing.assert_array_equal(_bits(y), _want_f32(ref.pooled))
    _check_codes(ref, code)
    dz = ops.maxpool2x2_bwd(_gated(ref, y > 0), code, (H, W))
    np.testing.assert_array_equal(_bits(dz), _want_f32(ref.dz))


@pytest.mark.parametrize('circ', R.PADS)
@pytest.mark.parametrize('case', R.FP32_CASES, ids=lambda c: '%s-%dx%d-%d-%d' % c)
def test_fp32_codes_values_and_routing(case, circ):
    from witw_amd import ops
    site, H, W, cin, cout = case
    ref = R.conv_case(2, H, W, cin, cout, circ)
    x, w, b = _f32(ref.x), _f32_nchw(ref.w), _f32_nchw(ref.b)
    pk = ops.PackedConv(w, b)
    tn = 128 if cout >= 128 else 64
    name = 'conv3x3_nhwc_f32_kernel<%d,1,true,%d,%d,9>'
    if site == 'narrow':
        # conv3x3.hip, `else if (NARROW)`: both rows of a window in one M-tile; maps of at most 32 columns, 4 waves whatever is asked
        assert W <= 32
        for nw in (None, 8):
            y, code, variant, form = _fp32_forward(ops, x, pk, circ, nw)
            assert (variant, form) == (name % (tn, 4, 1), 'direct')
            _check_fp32(ops, ref, y, code, H, W)
        return
    assert W > 32
    if site == 'wino':
        # conv3x3.hip, conv_wino_h2<NW, POOL>: the store near the top of the file, reached by a Winograd-packed filter; the launcher's
        # own choice for these grids is 4 waves, 8 is the other instantiation of the same epilogue
        pk_w = ops.PackedConv(w, b, wino=True)
        direct = {}
        for nw, waves in ((None, 4), (8, 8)):
            yd, cd, variant, form = _fp32_forward(ops, x, pk, circ, nw)
            assert (variant, form) == (name % (tn, waves, 0), 'direct')
            yw, cw, variant, form = _fp32_forward(ops, x, pk_w, circ, nw)
            assert (variant, form) == (name % (tn, waves, 0), 'wino_h2')
            _check_fp32(ops, ref, yw, cw, H, W)
            assert torch.equal(cw, cd) and torch.equal(yw.view(torch.int32), yd.view(torch.int32))
            direct[waves] = (yd, cd)
        _check_fp32(ops, ref, direct[4][0], direct[4][1], H, W)
        return
    # conv3x3.hip, wide geometry: `else if ((p.Cout & 3) == 0 && p.gate == nullptr)` through the LDS slab ('slab'), or the last `else`
    # with its per-element stores ('generic': a Cout that is no multiple of 4)
    assert (cout % 4 == 0) == (site == 'slab')
    codes = {}
    for nw in (4, 8):
        y, code, variant, form = _fp32_forward(ops, x, pk, circ, nw)
        assert (variant, form) == (name % (tn, nw, 0), 'direct')
        _check_fp32(ops, ref, y, code, H, W)
        codes[nw] = code
    assert torch.equal(codes[4], codes[8])


# ================================================================================ (a) bf16: csrc/conv3x3_bf16.hip
def _bf16_x(a_nchw):
    return _f32(a_nchw).bfloat16()


def _check_bf16(ops, ref, y, code, H, W, sel=None):
    """sel: the images of the batch that ref describes (None: all)"""
    ys, cs = (y, code) if sel is None else (y[sel].contiguous(), code[sel].contiguous())
    np.testing.assert_array_equal(_bits(ys), _want_bf16(ref.pooled))
    _check_codes(ref, cs)
    dz = ops.maxpool2x2_bwd_bf16(_gated(ref, ys.float() > 0).bfloat16(), cs, (H, W))
    np.testing.assert_array_equal(_bits(dz), _want_bf16(ref.dz))


@pytest.mark.parametrize('circ', R.PADS)
@pytest.mark.parametrize('case', R.LOW_CASES, ids=lambda c: '%dx%d-%d-%d' % c)
def test_bf16_tiled_kernel_codes_values_and_routing(case, circ):
    """conv3x3_bf16.hip, conv3x3_nhwc_bf16_kernel's `else if ((p.Cout & 7) == 0)` pool epilogue (the 32x32x16 MFMA)"""
    from witw_amd import ops
    H, W, cin, cout = case
    ref = R.conv_case(2, H, W, cin, cout, circ)
    pk = ops.PackedConvBf16(_f32_nchw(ref.w), _f32_nchw(ref.b))
    prev = ops.bf16_mfma16(False)
    try:
        y, code = ops.conv3x3_bf16_fwd(_bf16_x(ref.x), pk, circular=circ, relu=True, pool=True, want_pool_code=True)
        assert ops.last_kernel_variant() == 'conv3x3_nhwc_bf16_kernel<%d,1,true,4>' % (128 if cout >= 128 else 64)
    finally:
        ops.bf16_mfma16(prev)
    _check_bf16(ops, ref, y, code, H, W)


@pytest.mark.parametrize('circ', R.PADS)
def test_bf16_16x16x32_train_kernel_codes_values_and_routing(circ):
    """conv3x3_bf16.hip, conv3x3_bf16_s16_kernel<true, TRAIN>'s store: only a grid that fills the chip selects the kernel (R.S16_CASE:
    the smallest such batch of 16 x 64 maps); four images of the batch are compared"""
    from witw_amd import ops
    B, H, W, cin, cout = R.S16_CASE
    sel = R.pick(B)
    ref = R.conv_case(B, H, W, cin, cout, circ, tuple(sel))
    pk = ops.PackedConvBf16(_f32_nchw(ref.w), _f32_nchw(ref.b))
    prev = ops.bf16_mfma16(True)
    try:
        y, code = ops.conv3x3_bf16_fwd(_bf16_x(ref.x), pk, circular=circ, relu=True, pool=True, want_pool_code=True)
        assert ops.last_kernel_variant() == 'conv3x3_bf16_s16_kernel<true,true>', ops.last_kernel_variant()
    finally:
        ops.bf16_mfma16(prev)
    _check_bf16(ops, ref, y, code, H, W, sel)
    assert int(code.max()) <= 3


# ================================================================================ (a) split-fp16: csrc/conv3x3_f16x3.hip
@pytest.mark.parametrize('circ', R.PADS)
@pytest.mark.parametrize('case', R.LOW_CASES, ids=lambda c: '%dx%d-%d-%d' % c)
def test_split_fp16_codes_values_and_routing(case, circ):
    """conv3x3_f16x3.hip, conv3x3_nhwc_f16x3_kernel's `else if ((p.Cout & 7) == 0)` pool epilogue, and maxpool2x2_bwd_split"""
    from witw_amd import ops
    H, W, cin, cout = case
    ref = R.conv_case(2, H, W, cin, cout, circ)
    pk = ops.PackedConvF16x3(_f32_nchw(ref.w), _f32_nchw(ref.b))
    xs = ops.nchw_to_split_f16(_f32_nchw(ref.x), cin)
    y, code = ops.conv3x3_f16x3_fwd(xs, pk, circular=circ, relu=True, pool=True, want_pool_code=True)
    assert ops.last_kernel_variant() == 'conv3x3_nhwc_f16x3_kernel<%d,1,true,4>' % (128 if cout >= 128 else 64)
    assert not ops.f16x3_overflowed(DEV)
    np.testing.assert_array_equal(_bits(y), _want_split(ref.pooled))
    _check_codes(ref, code)
    gated = _gated(ref, ops.split_f16_to_f32(y) > 0)                                   # fp32 NHWC
    dy = ops.nchw_to_split_f16(gated.permute(0, 3, 1, 2).contiguous(), cout)
    np.testing.assert_array_equal(_bits(dy), _want_split(np.where(ref.m > 0, ref.gy, 0.0)))
    dz = ops.maxpool2x2_bwd_split(dy, code, (H, W))
    np.testing.assert_array_equal(_bits(dz), _want_split(ref.dz))


# ================================================================================ (a) the fused first two layers: csrc/conv_first2_bf16.hip
@pytest.mark.parametrize('circ', R.PADS)
@pytest.mark.parametrize('shape', R.FIRST2_SHAPES, ids=lambda s: '%dx%dx%dx%d' % s)
def test_first_two_layers_training_form_codes_and_values(shape, circ):
    """conv_first2_bf16.hip, the TRAIN instantiations' code store (through the wave's byte slab), against the float64 composition of
    both layers; the gate bits stay with tests/test_bf16_gpu.py"""
    from witw_amd import ops
    B, C, H, W = shape
    ref = R.first2_case(B, C, H, W, circ)
    pf = ops.PackedFirstConv(_f32_nchw(ref.w0), _f32_nchw(ref.b0), bf16=True)
    p2 = ops.PackedConvBf16(_f32_nchw(ref.w2), _f32_nchw(ref.b2))
    y, code, _bits_unused = ops.conv_first2_bf16_train(_f32_nchw(ref.x), pf, p2, circular=circ)
    assert ops.last_kernel_variant() == 'conv_first2_bf16_kernel<%d,train>' % (4 if C <= 4 else 8)
    _check_bf16(ops, ref, y, code, H, W)


# ================================================================================ (b) the scatter kernels alone
SCATTER_SHAPES = [((2, 3, 5), (6, 10)), ((2, 3, 5), (7, 11)), ((1, 1, 1), (3, 2)), ((3, 4, 33), (9, 67))]      # (B, Hp, Wp) -> (H, W)

SCATTER_IDS = ['%dx%dx%d-%dx%d' % (s[0] + s[1]) for s in SCATTER_SHAPES]

# -0.0, +-inf, NaNs with a payload (either sign), the smallest and another subnormal of either sign, +0.0
SPECIAL32 = [0x80000000, 0x7f800000, 0xff800000, 0x7fc12345, 0xffc00abc, 0x00000001, 0x807fffff, 0x00000400, 0x00000000]
SPECIAL16 = {'bf16': [0x8000, 0x7f80, 0xff80, 0x7fc5, 0xffd3, 0x0001, 0x807f, 0x0010, 0x0000],
             'f16': [0x8000, 0x7c00, 0xfc00, 0x7e05, 0xfe13, 0x0001, 0x83ff, 0x0010, 0x0000]}


def _scatter_operands(seed, shape, finite, special, dtype):
    """bit patterns [B,Hp,Wp,...]: a third special values, the rest ordinary finite numbers; codes uniform over 0..3"""
    g = np.random.Generator(np.random.Philox(key=[seed, int(np.prod(shape))]))
    bits = np.where(g.random(shape) < 1.0 / 3, np.asarray(special, dtype=np.uint32)[g.integers(0, len(special), shape)], finite(g, shape))
    return bits.astype(dtype), g


def _finite32(g, shape):
    return g.standard_normal(shape, dtype=np.float32).view(np.uint32)


def _finite_bf16(g, shape):
    return g.standard_normal(shape, dtype=np.float32).view(np.uint32) >> 16


def _finite_f16(g, shape):
    return g.standard_normal(shape, dtype=np.float32).astype(np.float16).view(np.uint16).astype(np.uint32)


@pytest.mark.parametrize('C', [1, 5, 64, 72])
@pytest.mark.parametrize('shape', SCATTER_SHAPES, ids=SCATTER_IDS)
def test_scatter_fp32_moves_bits(shape, C):
    from witw_amd import ops
    (B, Hp, Wp), (H, W) = shape
    dy, g = _scatter_operands(61, (B, Hp, Wp, C), _finite32, SPECIAL32, np.uint32)
    code = g.integers(0, 4, (B, Hp, Wp, C)).astype(np.uint8)
    dx = ops.maxpool2x2_bwd(torch.from_numpy(dy.view(np.int32)).to(DEV).view(torch.float32), torch.from_numpy(code).to(DEV), (H, W))
    assert dx.dtype == torch.float32 and tuple(dx.shape) == (B, H, W, C)
    np.testing.assert_array_equal(_bits(dx), R.scatter_ref(dy.view(np.int32), code, H, W))


@pytest.mark.parametrize('C', [8, 64, 72])
@pytest.mark.parametrize('shape', SCATTER_SHAPES, ids=SCATTER_IDS)
def test_scatter_bf16_moves_bits(shape, C):
    from witw_amd import ops
    (B, Hp, Wp), (H, W) = shape
    dy, g = _scatter_operands(62, (B, Hp, Wp, C), _finite_bf16, SPECIAL16['bf16'], np.uint16)
    code = g.integers(0, 4, (B, Hp, Wp, C)).astype(np.uint8)
    dx = ops.maxpool2x2_bwd_bf16(torch.from_numpy(dy.view(np.int16)).to(DEV).view(torch.bfloat16), torch.from_numpy(code).to(DEV), (H, W))
    assert dx.dtype == torch.bfloat16 and tuple(dx.shape) == (B, H, W, C)
    np.testing.assert_array_equal(_bits(dx), R.scatter_ref(dy.view(np.int16), code, H, W))


@pytest.mark.parametrize('C', [8, 64, 72])
@pytest.mark.parametrize('shape', SCATTER_SHAPES, ids=SCATTER_IDS)
def test_scatter_split_fp16_moves_bits(shape, C):
    """both planes of a channel follow the channel's code: dy [B,Hp,Wp,C/8,2,8], code [B,Hp,Wp,C]"""
    from witw_amd import ops
    (B, Hp, Wp), (H, W) = shape
    dy, g = _scatter_operands(63, (B, Hp, Wp, C // 8, 2, 8), _finite_f16, SPECIAL16['f16'], np.uint16)
    code = g.integers(0, 4, (B, Hp, Wp, C)).astype(np.uint8)
    dx = ops.maxpool2x2_bwd_split(torch.from_numpy(dy.view(np.int16)).to(DEV).view(torch.float16), torch.from_numpy(code).to(DEV), (H, W))
    assert dx.dtype == torch.float16 and tuple(dx.shape) == (B, H, W, C // 8, 2, 8)
    got = _bits(dx)
    for plane in range(2):
        src = np.ascontiguousarray(dy[:, :, :, :, plane, :]).reshape(B, Hp, Wp, C).view(np.int16)
        np.testing.assert_array_equal(got[:, :, :, :, plane, :].reshape(B, H, W, C), R.scatter_ref(src, code, H, W))


def test_scatter_shape_checks_raise():
    """an output smaller than twice the pooled map, and for the 16-bit forms a channel count that is no multiple of 8"""
    from witw_amd import _lib, ops
    code = torch.zeros((1, 2, 3, 8), dtype=torch.uint8, device=DEV)
    f32 = torch.zeros((1, 2, 3, 8), dtype=torch.float32, device=DEV)
    split = torch.zeros((1, 2, 3, 1, 2, 8), dtype=torch.float16, device=DEV)
    for hw in ((3, 6), (4, 5)):          # H < 2 Hp; W < 2 Wp
        with pytest.raises(_lib.WitwError):
            ops.maxpool2x2_bwd(f32, code, hw)
        with pytest.raises(_lib.WitwError):
            ops.maxpool2x2_bwd_bf16(f32.bfloat16(), code, hw)
        with pytest.raises(_lib.WitwError):
            ops.maxpool2x2_bwd_split(split, code, hw)
    for C in (4, 12):
        c = torch.zeros((1, 2, 3, C), dtype=torch.uint8, device=DEV)
        with pytest.raises(_lib.WitwError):
            ops.maxpool2x2_bwd_bf16(torch.zeros((1, 2, 3, C), dtype=torch.bfloat16, device=DEV), c, (4, 6))
    # the split layout cannot spell such a count, so the library's own check is asked directly
    lib = _lib.load()
    out = torch.zeros((1, 4, 6, 2, 2, 8), dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.WitwError):
        _lib.check(lib.witw_maxpool2x2_bwd_split(split.data_ptr(), code.data_ptr(), out.data_ptr(), 1, 2, 3, 4, 6, 12,
                                                 torch.cuda.current_stream().cuda_stream), 'witw_maxpool2x2_bwd_split')
    torch.cuda.synchronize()
