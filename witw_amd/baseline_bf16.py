"""Host-side wrappers of csrc/conv_taps4_bf16.hip: the bf16 filter packing and the 2x2-tap convolution of blocks 2-4 of cvig_baseline's
encoders at inference (SurfaceEncoder(precision='bf16')). With ops.conv4x4s2_first(out_bf16=True) they are the bf16 part of that
forward and live here, not in ops.py; their memory-contract cases are in tests/test_baseline_bf16_gpu.py. No CPU fallback."""
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
