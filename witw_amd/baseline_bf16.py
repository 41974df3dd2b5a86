"""Host-side wrappers of csrc/conv_taps4_bf16.hip: the bf16 filter packing and the 2x2-tap convolution of blocks 2-4 of cvig_baseline's
encoders at inference (SurfaceEncoder(precision='bf16')). With ops.conv4x4s2_first(out_bf16=True) they are the bf16 part of that
forward and live here, not in ops.py; their memory-contract cases are in tests/test_baseline_bf16_gpu.py. No CPU fallback.
precision='bf16_all' adds blocks 5-7: conv_taps4_splitk_bf16 (csrc/conv_taps4_splitk_bf16.hip) and space_to_depth2_mosaic_bf16 (the
bf16 store of csrc/baseline.hip's mosaic kernel); memory-contract cases in tests/test_baseline_bf16_all_gpu.py.
train_precision='bf16' (training: forward, data gradient and weight gradient of blocks 2-4) adds the transpose_flip packing,
conv_taps4_plain_bf16, space_to_depth2_bf16 (csrc/baseline.hip), to_bf16 and conv3x3_wgrad_bf16_taps4
(tests/test_baseline_bf16_train_gpu.py)."""
import torch

from . import _lib
from .ops import _Packed, _dev_f32, _p, _post_affine, _prof_begin, _prof_end, _stream, _wgrad_setup


class PackedConvBf16Taps4(_Packed):
    """bf16 packing of the taps {1,2}^2 of one [cout][cin][3][3] filter (ops.conv4x4_to_k3 of a Conv2d(k=4, s=2)) for conv_taps4_s2d_bf16
    + the fp32 bias. transpose_flip (training only, conv_taps4_plain_bf16 with tap_base = 0): the taps {0,1}^2 of the data-gradient filter
    w_t[ci][co][kh][kw] = w[co][ci][2-kh][2-kw] instead, no bias."""
    CPAD, DTYPE = 16, torch.bfloat16
    taps4 = True

    def __init__(self, weight, bias, reuse=None, transpose_flip=False):
        lib = _lib.load()
        self.tap_base = 0 if transpose_flip else 1
        if reuse is not None and getattr(reuse, 'tap_base', 1) != self.tap_base:
            reuse = None
        w, reuse = self._filter_buffer(weight, bool(transpose_flip), reuse, lib.witw_conv3x3_bf16_packed_elems_taps4)
        if tuple(w.shape[2:]) != (3, 3):
            raise _lib.WitwError('PackedConvBf16Taps4: expects a [cout, cin, 3, 3] filter, got %s' % (tuple(w.shape),))
        if transpose_flip:
            _lib.check(lib.witw_conv3x3_bf16_pack_weights_taps4_ex(w.data_ptr(), self.wpk.data_ptr(), self.cout, self.cin, 1, _stream()),
                       'witw_conv3x3_bf16_pack_weights_taps4_ex')
        else:
            _lib.check(lib.witw_conv3x3_bf16_pack_weights_taps4(w.data_ptr(), self.wpk.data_ptr(), self.cout, self.cin, _stream()),
                       'witw_conv3x3_bf16_pack_weights_taps4')
        self._bias_buffer(reuse, None if transpose_flip else bias)


def _bf16_nhwc(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous() and t.dim() == 4):
        raise _lib.WitwError('%s must be a contiguous bfloat16 NHWC GPU tensor (no CPU fallback)' % name)
    return t


def _fwd_packed(name, packed):
    if not isinstance(packed, PackedConvBf16Taps4) or packed.tap_base != 1:
        raise _lib.WitwError('%s: a forward-packed PackedConvBf16Taps4 filter is required' % name)


def _channels(name, channels, packed):
    if channels != packed.cin_pad:
        raise _lib.WitwError('%s: input has %d channels, packed weights expect %d' % (name, channels, packed.cin_pad))


def _valid_region(name, vh, vw, H, W, what='map'):
    """(vh, vw) as ints inside the H x W map, checked before anything is allocated"""
    vh, vw = int(vh), int(vw)
    if not (1 <= vh <= H and 1 <= vw <= W):
        raise _lib.WitwError('%s: valid region %dx%d outside the %dx%d %s' % (name, vh, vw, H, W, what))
    return vh, vw


def conv_taps4_s2d_bf16(x_nhwc, packed, valid_hw, lrelu_slope=0.2, post_scale=None, post_shift=None, out_f32=False):
    """conv_taps4_s2d on bf16 operands with fp32 accumulation (witw_conv3x3_bf16_fwd_taps4): x bf16 [B,H,W,Cin_pad], packed a
    PackedConvBf16Taps4 -> [B, ceil(vh/2), ceil(vw/2), 4*Cout], bf16 (one nearest-even rounding behind the fp32 epilogue bias ->
    LeakyReLU -> affine) or fp32 with out_f32 (no rounding), +0.0 outside the (vh, vw) valid outputs."""
    lib = _lib.load()
    x_nhwc = _bf16_nhwc(x_nhwc, 'conv_taps4_s2d_bf16: x')
    B, H, W, C = x_nhwc.shape
    _fwd_packed('conv_taps4_s2d_bf16', packed)
    _channels('conv_taps4_s2d_bf16', C, packed)
    post_scale, post_shift = _post_affine('conv_taps4_s2d_bf16', post_scale, post_shift, packed.cout)
    vh, vw = _valid_region('conv_taps4_s2d_bf16', *valid_hw, H, W)      # before anything is allocated: the library's error, not torch's
    y = torch.empty((B, (vh + 1) // 2, (vw + 1) // 2, 4 * packed.cout), dtype=torch.float32 if out_f32 else torch.bfloat16, device=x_nhwc.device)
    prof = _prof_begin()
    _lib.check(lib.witw_conv3x3_bf16_fwd_taps4(x_nhwc.data_ptr(), packed.wpk.data_ptr(), packed.bias.data_ptr(), _p(post_scale), _p(post_shift),
                                               y.data_ptr(), B, H, W, C, packed.cout, float(lrelu_slope), int(vh), int(vw), int(bool(out_f32)),
                                               _stream()), 'witw_conv3x3_bf16_fwd_taps4')
    if prof is not None:
        _prof_end(prof, ('bf16_taps4', 128, 1, False), 2.0 * packed.cin * packed.cout * 4 * vh * vw * B, kernel=True)
    return y


def conv_taps4_splitk_bf16(x_mosaic_bf16, packed, n_images, g, valid_hw, lrelu_slope=0.2, post_scale=None, post_shift=None, ksplit=None):
    """ops.conv_taps4_splitk on bf16 operands with fp32 accumulation (blocks 5-7 of SurfaceEncoder(precision='bf16_all')): x bf16
    [ceil(n/g^2), g*h, g*w, Cin_pad], a g x g mosaic (g = 1: the plain batch), packed a PackedConvBf16Taps4 -> y fp32
    [n_images, vh, vw, Cout] = affine(lrelu(conv + bias)) of the valid outputs, never rounded. witw_conv3x3_bf16_fwd_taps4_splitk writes
    the raw fp32 sums of ksplit K slices (None: the library's choice) into a workspace, witw_taps4_splitk_finish adds them in slice order."""
    lib = _lib.load()
    x = x_mosaic_bf16
    _bf16_nhwc(x, 'conv_taps4_splitk_bf16: x')
    _fwd_packed('conv_taps4_splitk_bf16', packed)
    Bm, H, W, C = x.shape
    n_images, g = int(n_images), int(g)
    if g < 1 or n_images < 1 or H % g or W % g or Bm != (n_images + g * g - 1) // (g * g):
        raise _lib.WitwError('conv_taps4_splitk_bf16: %s is not a %dx%d mosaic of %d images' % (tuple(x.shape), g, g, n_images))
    _channels('conv_taps4_splitk_bf16', C, packed)
    if packed.cout % 4:
        raise _lib.WitwError('conv_taps4_splitk_bf16: Cout=%d must be a multiple of 4' % packed.cout)
    post_scale, post_shift = _post_affine('conv_taps4_splitk_bf16', post_scale, post_shift, packed.cout)
    h, w = H // g, W // g
    vh, vw = _valid_region('conv_taps4_splitk_bf16', *valid_hw, h, w, 'cell')
    S = lib.witw_conv3x3_bf16_taps4_ksplit(Bm, H, W, C, packed.cout) if ksplit is None else int(ksplit)
    if not 1 <= S <= C // 16:
        raise _lib.WitwError('conv_taps4_splitk_bf16: ksplit=%d outside [1, Cin/16 = %d]' % (S, C // 16))
    ws = torch.empty((S, Bm, H, W, packed.cout), dtype=torch.float32, device=x.device)
    y = torch.empty((n_images, vh, vw, packed.cout), dtype=torch.float32, device=x.device)
    prof = _prof_begin()
    _lib.check(lib.witw_conv3x3_bf16_fwd_taps4_splitk(x.data_ptr(), packed.wpk.data_ptr(), ws.data_ptr(), Bm, H, W, C, packed.cout, S,
                                                      _stream()), 'witw_conv3x3_bf16_fwd_taps4_splitk')
    if prof is not None:
        _prof_end(prof, ('bf16_taps4_splitk', 128, 1, False), 2.0 * packed.cin * packed.cout * 4 * vh * vw * n_images, kernel=True)
    act = 2 if lrelu_slope is not None else 0
    _lib.check(lib.witw_taps4_splitk_finish(ws.data_ptr(), S, packed.bias.data_ptr(), act, float(lrelu_slope or 0.), _p(post_scale),
                                            _p(post_shift), y.data_ptr(), n_images, g, h, w, vh, vw, packed.cout, _stream()),
               'witw_taps4_splitk_finish')
    return y


def space_to_depth2_mosaic_bf16(y_f32, g=1):
    """ops.space_to_depth2_mosaic with one nearest-even rounding at a bf16 store: y fp32 [B,H,W,C] -> bf16
    [ceil(B/g^2), g*ceil(H/2), g*ceil(W/2), 4C], +0.0 where no source exists."""
    lib = _lib.load()
    y = y_f32
    if not (isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float32 and y.is_contiguous() and y.dim() == 4):
        raise _lib.WitwError('space_to_depth2_mosaic_bf16: y must be a contiguous float32 NHWC GPU tensor (no CPU fallback)')
    B, H, W, C = y.shape
    g = int(g)
    if C % 4 or not 1 <= g <= 64:
        raise _lib.WitwError('space_to_depth2_mosaic_bf16: C=%d must be a multiple of 4 and 1 <= g=%d <= 64' % (C, g))
    out = torch.empty(((B + g * g - 1) // (g * g), g * ((H + 1) // 2), g * ((W + 1) // 2), 4 * C), dtype=torch.bfloat16, device=y.device)
    _lib.check(lib.witw_space_to_depth2_mosaic_bf16(y.data_ptr(), out.data_ptr(), B, H, W, C, g, _stream()), 'witw_space_to_depth2_mosaic_bf16')
    return out


# ----------------------------------------------------------------------------- training (train_precision='bf16')
def conv_taps4_plain_bf16(x_nhwc, packed, valid_hw=None, lrelu_slope=None):
    """ops.conv3x3_fwd with a taps4 filter on bf16 operands with fp32 accumulation (witw_conv3x3_bf16_fwd_taps4_plain): x bf16
    [B,H,W,Cin_pad], packed a PackedConvBf16Taps4 -> fp32 [B,H,W,Cout] in the plain layout, never rounded, +0.0 outside the (vh, vw)
    valid outputs (None: all of H x W). A forward-packed filter (tap_base 1) adds its bias, then LeakyReLU when lrelu_slope is given:
    a block's forward; a transpose_flip-packed one (tap_base 0) has neither: the block's data gradient."""
    lib = _lib.load()
    x = _bf16_nhwc(x_nhwc, 'conv_taps4_plain_bf16: x')
    if not isinstance(packed, PackedConvBf16Taps4):
        raise _lib.WitwError('conv_taps4_plain_bf16: a PackedConvBf16Taps4 filter is required')
    B, H, W, C = x.shape
    if C != packed.cin_pad:
        raise _lib.WitwError('conv_taps4_plain_bf16: input has %d channels, packed weights expect %d' % (C, packed.cin_pad))
    if packed.tap_base == 0 and lrelu_slope is not None:
        raise _lib.WitwError('conv_taps4_plain_bf16: a data-gradient filter takes no activation')
    vh, vw = _valid_region('conv_taps4_plain_bf16', *((H, W) if valid_hw is None else valid_hw), H, W)
    y = torch.empty((B, H, W, packed.cout), dtype=torch.float32, device=x.device)
    prof = _prof_begin()
    _lib.check(lib.witw_conv3x3_bf16_fwd_taps4_plain(x.data_ptr(), packed.wpk.data_ptr(), packed.bias.data_ptr() if packed.tap_base else None,
                                                     y.data_ptr(), B, H, W, C, packed.cout, int(lrelu_slope is not None),
                                                     float(lrelu_slope or 0.), packed.tap_base, vh, vw, _stream()),
               'witw_conv3x3_bf16_fwd_taps4_plain')
    if prof is not None:
        _prof_end(prof, ('bf16_taps4_plain', 128, 1, False), 2.0 * packed.cin * packed.cout * 4 * vh * vw * B, kernel=True)
    return y


def space_to_depth2_bf16(x_nhwc, valid_hw=None, scale=None, shift=None):
    """ops.space_to_depth2 of an NHWC activation with one nearest-even rounding at a bf16 store: x fp32 [B,Hp,Wp,C] (C % 4 == 0) -> bf16
    [B, ceil(vh/2), ceil(vw/2), 4C], the train-mode BatchNorm affine (scale, shift: [C]) applied on the fly, +0.0 outside the valid region."""
    lib = _lib.load()
    x = _dev_f32(x_nhwc, 'x')
    if x.dim() != 4 or x.shape[3] % 4:
        raise _lib.WitwError('space_to_depth2_bf16: x must be NHWC with C %% 4 == 0, got %s' % (tuple(x.shape),))
    B, Hp, Wp, C = x.shape
    H, W = _valid_region('space_to_depth2_bf16', *((Hp, Wp) if valid_hw is None else valid_hw), Hp, Wp)
    if (scale is None) != (shift is None):
        raise _lib.WitwError('space_to_depth2_bf16: scale and shift come together')
    if scale is not None:
        scale, shift = _dev_f32(scale, 'scale'), _dev_f32(shift, 'shift')
        if scale.numel() != C or shift.numel() != C:
            raise _lib.WitwError('space_to_depth2_bf16: scale / shift must have C entries')
    y = torch.empty((B, (H + 1) // 2, (W + 1) // 2, 4 * C), dtype=torch.bfloat16, device=x.device)
    _lib.check(lib.witw_space_to_depth2_bf16(x.data_ptr(), y.data_ptr(), B, Hp, Wp, H, W, C, _p(scale), _p(shift), _stream()),
               'witw_space_to_depth2_bf16')
    return y


def to_bf16(x):
    """fp32 -> bf16 of the same shape, one nearest-even rounding per element (witw_f32_to_bf16): a block's output gradient dz."""
    lib = _lib.load()
    x = _dev_f32(x, 'x')
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    if x.numel():
        _lib.check(lib.witw_f32_to_bf16(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), 'witw_f32_to_bf16')
    return y


def conv3x3_wgrad_bf16_taps4(x_nhwc, dz_nhwc, cin_real, want_bias=True, out=None, accumulate=False):
    """ops.conv3x3_wgrad(taps4=True) on bf16 operands with fp32 accumulation (witw_conv3x3_wgrad_bf16_taps4): x bf16 [B,H,W,Cin], dz bf16
    [B,H,W,Cout] -> (dW [Cout,cin_real,3,3] fp32 with taps {1,2}^2 computed and exact zeros elsewhere, db [Cout] fp32 or None).
    out = (dW, db): write into (accumulate: add to) these contiguous fp32 tensors."""
    lib = _lib.load()
    x, dz = _bf16_nhwc(x_nhwc, 'conv3x3_wgrad_bf16_taps4: x'), _bf16_nhwc(dz_nhwc, 'conv3x3_wgrad_bf16_taps4: dz')
    B, H, W, Cin = x.shape
    Cout = dz.shape[3]
    if accumulate and out is None:
        raise _lib.WitwError('conv3x3_wgrad_bf16_taps4: accumulate needs out')
    _, dw, db = _wgrad_setup('conv3x3_wgrad_bf16_taps4', B, H, W, Cout, cin_real, 1, dz.shape[:3], x.device, want_bias, out)
    n_ws = lib.witw_conv3x3_wgrad_bf16_taps4_workspace_floats(B, H, W, Cin, Cout)
    ws = torch.empty(n_ws, dtype=torch.float32, device=x.device)
    prof = _prof_begin()
    _lib.check(lib.witw_conv3x3_wgrad_bf16_taps4(x.data_ptr(), dz.data_ptr(), dw.data_ptr(), _p(db), ws.data_ptr(), B, H, W, Cin, cin_real,
                                                 Cout, int(bool(accumulate)), _stream()), 'witw_conv3x3_wgrad_bf16_taps4')
    if prof is not None:
        _prof_end(prof, ('wgrad_bf16_taps4', 1), 2.0 * cin_real * Cout * 4 * H * W * B, kernel=True)
    return dw, db
