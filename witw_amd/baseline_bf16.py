"""Host-side wrappers of csrc/conv_taps4_bf16.hip: the bf16 filter packing and the 2x2-tap convolution of blocks 2-4 of cvig_baseline's
encoders at inference (SurfaceEncoder(precision='bf16')). With ops.conv4x4s2_first(out_bf16=True) they are the bf16 part of that
forward and live here, not in ops.py; their memory-contract cases are in tests/test_baseline_bf16_gpu.py. No CPU fallback.
precision='bf16_all' adds the wrappers of csrc/conv_taps4_splitk_bf16.hip for blocks 5-7: conv_taps4_splitk_bf16 and
space_to_depth2_mosaic_bf16 (memory-contract cases in tests/test_baseline_bf16_all_gpu.py)."""
import torch

from . import _lib
from .ops import _Packed, _dev_f32, _p, _prof_begin, _prof_end, _stream


class PackedConvBf16Taps4(_Packed):
    """bf16 packing of the taps {1,2}^2 of one [cout][cin][3][3] filter (ops.conv4x4_to_k3 of a Conv2d(k=4, s=2)) for conv_taps4_s2d_bf16
    + the fp32 bias. Forward filters only: cvig_baseline's bf16 arithmetic is inference."""
    CPAD, DTYPE = 16, torch.bfloat16
    taps4 = True

    def __init__(self, weight, bias, reuse=None):
        lib = _lib.load()
        w, reuse = self._filter_buffer(weight, False, reuse, lib.witw_conv3x3_bf16_packed_elems_taps4)
        if tuple(w.shape[2:]) != (3, 3):
            raise _lib.WitwError('PackedConvBf16Taps4: expects a [cout, cin, 3, 3] filter, got %s' % (tuple(w.shape),))
        _lib.check(lib.witw_conv3x3_bf16_pack_weights_taps4(w.data_ptr(), self.wpk.data_ptr(), self.cout, self.cin, _stream()),
                   'witw_conv3x3_bf16_pack_weights_taps4')
        self._bias_buffer(reuse, bias)


def conv_taps4_s2d_bf16(x_nhwc, packed, valid_hw, lrelu_slope=0.2, post_scale=None, post_shift=None, out_f32=False):
    """conv_taps4_s2d on bf16 operands with fp32 accumulation (witw_conv3x3_bf16_fwd_taps4): x bf16 [B,H,W,Cin_pad], packed a
    PackedConvBf16Taps4 -> [B, ceil(vh/2), ceil(vw/2), 4*Cout], bf16 (one nearest-even rounding behind the fp32 epilogue bias ->
    LeakyReLU -> affine) or fp32 with out_f32 (no rounding), +0.0 outside the (vh, vw) valid outputs."""
    lib = _lib.load()
    if not (isinstance(x_nhwc, torch.Tensor) and x_nhwc.is_cuda and x_nhwc.dtype == torch.bfloat16 and x_nhwc.is_contiguous() and x_nhwc.dim() == 4):
        raise _lib.WitwError('conv_taps4_s2d_bf16: x must be a contiguous bfloat16 NHWC GPU tensor (no CPU fallback)')
    if not isinstance(packed, PackedConvBf16Taps4):
        raise _lib.WitwError('conv_taps4_s2d_bf16: a PackedConvBf16Taps4 filter is required')
    B, H, W, C = x_nhwc.shape
    if C != packed.cin_pad:
        raise _lib.WitwError('conv_taps4_s2d_bf16: input has %d channels, packed weights expect %d' % (C, packed.cin_pad))
    if (post_scale is None) != (post_shift is None):
        raise _lib.WitwError('conv_taps4_s2d_bf16: post_scale and post_shift come together')
    if post_scale is not None:
        post_scale, post_shift = _dev_f32(post_scale, 'post_scale'), _dev_f32(post_shift, 'post_shift')
        if post_scale.numel() != packed.cout or post_shift.numel() != packed.cout:
            raise _lib.WitwError('post_scale/post_shift must have Cout entries')
    vh, vw = (int(v) for v in valid_hw)
    if not (1 <= vh <= H and 1 <= vw <= W):      # before anything is allocated: the library's error, not torch's
        raise _lib.WitwError('conv_taps4_s2d_bf16: valid region %dx%d outside the %dx%d map' % (vh, vw, H, W))
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
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and x.dim() == 4):
        raise _lib.WitwError('conv_taps4_splitk_bf16: x must be a contiguous bfloat16 NHWC GPU tensor (no CPU fallback)')
    if not isinstance(packed, PackedConvBf16Taps4):
        raise _lib.WitwError('conv_taps4_splitk_bf16: a PackedConvBf16Taps4 filter is required')
    Bm, H, W, C = x.shape
    n_images, g = int(n_images), int(g)
    if g < 1 or n_images < 1 or H % g or W % g or Bm != (n_images + g * g - 1) // (g * g):
        raise _lib.WitwError('conv_taps4_splitk_bf16: %s is not a %dx%d mosaic of %d images' % (tuple(x.shape), g, g, n_images))
    if C != packed.cin_pad:
        raise _lib.WitwError('conv_taps4_splitk_bf16: input has %d channels, packed weights expect %d' % (C, packed.cin_pad))
    if packed.cout % 4:
        raise _lib.WitwError('conv_taps4_splitk_bf16: Cout=%d must be a multiple of 4' % packed.cout)
    if (post_scale is None) != (post_shift is None):
        raise _lib.WitwError('conv_taps4_splitk_bf16: post_scale and post_shift come together')
    if post_scale is not None:
        post_scale, post_shift = _dev_f32(post_scale, 'post_scale'), _dev_f32(post_shift, 'post_shift')
        if post_scale.numel() != packed.cout or post_shift.numel() != packed.cout:
            raise _lib.WitwError('post_scale/post_shift must have Cout entries')
    h, w = H // g, W // g
    vh, vw = (int(v) for v in valid_hw)
    if not (1 <= vh <= h and 1 <= vw <= w):
        raise _lib.WitwError('conv_taps4_splitk_bf16: valid region %dx%d outside the %dx%d cell' % (vh, vw, h, w))
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
