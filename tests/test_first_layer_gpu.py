"""The first-layer kernels of the image entry path, bit for bit against float64 (tests/first_layer_ref.py) on data where every kernel
is exact whatever its summation order; tests/test_first_layer_ref.py proves on the CPU that the data tells eleven wrong kernels from
the right one. Every case asserts ops.last_kernel_variant(), runs under both paddings with the ReLU on and off, and is an equality
through an integer view (one pytest id of test_first_layer_equals_float64 runs both ReLU settings of its operands: the counts below are
twice the ids). B = 2 unless said; shapes (H, W): S = (1,1) (3,12) (8,64) (9,65) (13,99) (5,130).

    kernel                                       C           shapes                         data             cases
    conv3x3_first_kernel, fp32 store             1 2 3 4     S                              ints, dyadic     4 x 6 x 2 x 2 pads x 2 relu = 192
    conv3x3_first_kernel, split-fp16 store       1 3 4       (3,12) (9,65) (13,99)          dyadic           3 x 3 x 1 x 4 = 36
    conv3x3_first_persist_kernel                 1 2 3 4     (9,66) (8,130), B below        ints, dyadic     4 x 2 x 2 x 4 = 64
    conv3x3_first_kernel at the persistent B     3           (9,65)                         dyadic           4
    conv3x3_first_bf16_kernel<4>                 1 2 3 4     S                              ints, round16    192
    conv3x3_first_bf16_kernel<8>                 5 6 7 8     S                              ints, round16    192
    conv_first2_bf16_kernel<4/8,infer>           pool_ref.FIRST2_SHAPES                     ints             3 x 2 pads = 6
    conv_first2_bf16_kernel<4/8,train> gate bits pool_ref.FIRST2_SHAPES                     ints             6
    pack_first_kernel / pack_first_bf16_kernel   1 .. 4 / 1 .. 8: all 2560 floats of the fp32 image, the 384 (C <= 4) or 640 documented
                                                 16-byte slots of the bf16 image                             4 + 8
    one +inf pixel                               each of the five forward kernels / stores                   5

The persistent kernel is taken from 4 tiles per compute unit on and W >= 66. Its B is the smallest with B * tiles >= 4 * CUs and
(B * tiles) % (2 * CUs) != 0 (first_layer_ref.persist_batch: 257 images of (9,66) and 342 of (8,130) on 256 CUs), so its 2 * CUs
workgroups walk unequal runs of tiles and the fetch past the last tile is taken; all images are compared. (9,65) at the batch of
(9,66) has the tiles, not the width: it must stay on conv3x3_first_kernel.

Not reachable: the `out_bf16 == 1` branch of conv3x3_first_kernel (the bf16 rounding on load and the bf16 store inside the fp32
kernel). witw_conv3x3_first_fwd sends every out_bf16 = 1 launch to conv3x3_first_bf16_kernel<4 / 8>, so no case can run it.

Non-finite pixels (contract at witw_conv3x3_first_fwd, include/witw_hip.h): the fp32 kernels multiply a tap that does not exist by a
zero weight and every kernel multiplies zero filter elements, so a +inf pixel gives NaN where float64 gives +-inf. Observed on
gfx950, ReLU off, one +inf pixel, the 9 x 64 outputs around it as NaN / +inf / -inf: conv3x3_first_kernel 423 / 74 / 79 (fp32 store,
ints) and 310 / 125 / 141 (split store, dyadic, by hi), conv3x3_first_persist_kernel 439 / 63 / 74, conv3x3_first_bf16_kernel<4>
401 / 80 / 95, <8> 478 / 58 / 40: none finite, NaN wherever one of the channel's weights over the window is zero. The kernels are left
as they are. Asserted: outputs whose window does not hold the pixel are bit-equal to the reference, those whose window does are
non-finite (ReLU off: the ReLU turns NaN and -inf into +0.0)."""
import numpy as np
import pytest
import torch

from tests import first_layer_ref as R
from tests import pool_ref as P

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
IDS = [k.id for k in R.KEYS]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _bits(t):
    t = t.contiguous().cpu()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()]).numpy()


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _launch(ops, k, d, on, x=None):
    pk = ops.PackedFirstConv(_dev(d.w), _dev(d.b), bf16=k.row == 'bf16')
    y = ops.conv3x3_first_fwd(_dev(d.x) if x is None else x, pk, circular=k.circ, relu=on, split_f16=k.row == 'split')
    assert ops.last_kernel_variant() == k.variant(), (k.id, ops.last_kernel_variant())
    return y


@pytest.mark.parametrize('k', R.KEYS, ids=IDS)
def test_first_layer_equals_float64(k):
    from witw_amd import ops
    cu = _cu()
    d = R.data(k, cu)
    B = k.batch(cu)
    assert d.x.shape[0] == B and d.sel is None
    if k.big:
        tiles = k.tiles if k.row == 'persist' else 4
        assert B * tiles >= 4 * cu and (B * tiles) % (2 * cu) != 0 and B * k.tiles >= 4 * cu
    x = _dev(d.x)
    for on in R.RELUS:
        y = _launch(ops, k, d, on, x)
        want = R.expected(k, d, on)
        got = _bits(y)
        assert got.shape == want.shape
        assert np.array_equal(got, want), (k.id, on, int((got != want).sum()), got.size)


@pytest.mark.parametrize('circ', P.PADS)
@pytest.mark.parametrize('shape', P.FIRST2_SHAPES, ids=lambda s: '%dx%dx%dx%d' % s)
def test_first_two_layers_inference_form_and_gate_bits(shape, circ):
    """conv_first2_bf16_kernel<CW,infer>: the pooled output of both layers, rounded once to bf16; <CW,train>: bit c & 7 of byte
    c >> 3 = (float64 layer-0 value of channel c > 0)"""
    from witw_amd import ops
    B, C, H, W = shape
    c = P.first2_case(B, C, H, W, circ)
    want_y, want_bits = R.first2_answers(shape, circ)
    pf = ops.PackedFirstConv(_dev(c.w0), _dev(c.b0), bf16=True)
    p2 = ops.PackedConvBf16(_dev(c.w2), _dev(c.b2))
    y = ops.conv_first2_bf16(_dev(c.x), pf, p2, circular=circ)
    assert ops.last_kernel_variant() == 'conv_first2_bf16_kernel<%d,infer>' % (4 if C <= 4 else 8)
    assert np.array_equal(_bits(y), want_y)
    _y, _code, bits = ops.conv_first2_bf16_train(_dev(c.x), pf, p2, circular=circ)
    assert ops.last_kernel_variant() == 'conv_first2_bf16_kernel<%d,train>' % (4 if C <= 4 else 8)
    got = bits.cpu().numpy()
    assert got.shape == want_bits.shape and np.array_equal(got, want_bits), int((got != want_bits).sum())


@pytest.mark.parametrize('C', [1, 2, 3, 4])
def test_fp32_filter_image(C):
    """pack_first_kernel: wf[i][h][n][0..3] = w[n][0..3][tap 2i + h], zeros for tap 9 and channels >= C: all 2560 floats"""
    from witw_amd import ops
    w = R.pack_probe(C)
    pk = ops.PackedFirstConv(_dev(w), _dev(np.zeros(64)))
    assert np.array_equal(_bits(pk.wf).reshape(5, 2, 64, 4), R.E.f32_bits(R.pack_f32(w)))


@pytest.mark.parametrize('C', [1, 2, 3, 4, 5, 6, 7, 8])
def test_bf16_filter_image(C):
    """pack_first_bf16_kernel: the 384 (C <= 4: two taps of four channels) or 640 (one tap of eight channels) documented 16-byte slots;
    a slot the C <= 4 form does not write is not looked at. The probe's values are bf16 numbers; the rounding is round16's business."""
    from witw_amd import ops
    w = R.pack_probe(C)
    pk = ops.PackedFirstConv(_dev(w), _dev(np.zeros(64)), bf16=True)
    want = R.E.bf16_bits(R.pack_bf16(w))
    got = pk.wf.cpu().view(torch.int16).numpy()[:want.size].reshape(want.shape)
    assert want.size == (384 if C <= 4 else 640) * 8 and np.array_equal(got, want)


NONFINITE = [R.Key('f32', 3, 9, 65, 'ints', True), R.Key('split', 3, 9, 65, 'dyadic', True), R.Key('persist', 3, 9, 66, 'ints', True),
             R.Key('bf16', 3, 9, 65, 'ints', True), R.Key('bf16', 5, 9, 65, 'ints', True)]


@pytest.mark.parametrize('k', NONFINITE, ids=[k.id for k in NONFINITE])
def test_one_infinite_pixel(k):
    """a single +inf pixel in image 0, on the image's first column under circular padding (its window wraps): outside the pixel's
    3 x 3 neighbourhood the output keeps its bits, inside it every channel is NaN or +-inf (ReLU off)"""
    from witw_amd import ops
    d = R.data(k, _cu())
    ph, pc = 4, 0
    x = np.array(d.x)
    x[0, 1, ph, pc] = np.inf
    want = R.expected(k, d, False)
    y = _launch(ops, k, d, False, _dev(x))
    got = _bits(y)
    hit = np.zeros(d.x.shape[:1] + (k.H, k.W), dtype=bool)
    for dh in (-1, 0, 1):
        for dw in (-1, 0, 1):
            hit[0, ph + dh, (pc + dw) % k.W] = True
    assert hit.sum() == 9 and np.array_equal(got[~hit], want[~hit])
    v = (y.float() if k.row != 'split' else y[..., 0, :].reshape(y.shape[:3] + (64,)).float()).cpu().numpy()[hit]
    assert v.shape == (9, 64) and not np.isfinite(v).any()
    print('%s: of 9 x 64 outputs around a +inf pixel %d NaN, %d +inf, %d -inf' % (k.variant(), int(np.isnan(v).sum()), int(np.isposinf(v).sum()),
                                                                                   int(np.isneginf(v).sum())))
    # under the ReLU the neighbourhood is unspecified (NaN and -inf become +0.0); everything else keeps its bits
    got = _bits(_launch(ops, k, d, True, _dev(x)))
    assert np.array_equal(got[~hit], R.expected(k, d, True)[~hit])
