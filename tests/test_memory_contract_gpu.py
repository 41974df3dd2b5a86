"""Memory contract of every kernel-launching entry of witw_amd.ops: what a launch may touch besides the values it returns.

One table of cases (CASES); each case builds its inputs through `place`, calls one ops entry and returns what it returned. Every
case runs twice on ordinary torch allocations and once inside a tests/mem_arena.Arena (ops.torch replaced by ArenaTorch, so
outputs and workspaces are interior views between guard bands, inputs sit between NaN bands):

  P1 containment   no band of any output, workspace or input is touched
  P2 coverage      every element of every returned `empty` tensor was stored (a canary NaN / 0xA5 pattern is left otherwise)
  P3 placement     the arena result equals the plain result: bitwise where two plain calls agree bitwise, else within the
                   tolerance the entry's own parity test applies (the case names it)
  P4 finiteness    finite inputs between NaN bands give what the plain call gives finite, finite

Cases marked skew run once more with every placed input and preallocated output 16 bytes past a 256-byte boundary
(test_alignment_16_bytes): the kernels' widest accesses are 16 bytes, so that is the alignment the entries are held to.
ISOLATION holds the per-sample entries: every batch entry but one is NaN, the clean one's output must not change by a bit.

The device JPEG entries (witw_amd/jpeg.py) are out of scope: they have their own descriptor format and their own crafted-stream
and damage tests (tests/test_jpeg_gpu.py, tests/test_jpeg_damage_gpu.py).
"""
import collections

import numpy as np
import pytest
import torch

from tests.mem_arena import ALT_BAND_BYTE, Arena, ArenaError, ArenaTorch
from witw_amd import synth

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
Case = collections.namedtuple('Case', 'id family entries fn skew variant tol canon')
CASES = []
ISOLATION = []
SKEW_FAMILIES = ('conv_f32', 'conv_f32_wino', 'conv_f32_dgrad', 'first_layer', 'first2_bf16', 'conv_bf16', 'conv_f16x3', 'match', 'loss', 'adam')


def case(family, entries, id, skew=False, variant=None, tol=None, canon=None):
    """register fn(place) under `id`; entries: the ops names the case is the contract case of; variant: the expected
    ops.last_kernel_variant() (or a prefix ending in '*'); tol: (relative-norm bound, where it comes from) for entries whose two
    plain calls differ bitwise; canon: maps the flattened outputs to what is compared (an unordered list -> its sorted form)"""
    def deco(fn):
        assert id not in [c.id for c in CASES], id
        CASES.append(Case(id, family, tuple(entries.split()), fn, skew or family in SKEW_FAMILIES, variant, tol, canon))
        return fn
    return deco


def _g(*key):
    return np.random.Generator(np.random.Philox(key=([int(k) for k in key] + [0])[:2]))


def _n(g, shape, scale=1.0):
    return torch.from_numpy((g.standard_normal(shape, dtype=np.float32) * np.float32(scale)).astype(np.float32))


def _big(seed, shape, dtype=torch.float32):
    """large operands: drawn on the device (same values for the same seed)"""
    return torch.randn(shape, generator=torch.Generator(DEV).manual_seed(seed), device=DEV).to(dtype)


def _ops():
    from witw_amd import ops
    return ops


# ============================================================================ fp32 conv forward
F32_CASES = [
    # B, H, W, Cin, Cout, stride_h, circ, relu, pool, nchw, extras
    (1, 12, 99, 16, 64, 1, False, True, True, False, 'code'),      # ragged width, floor pooling (+ the pool codes)
    (1, 12, 99, 16, 64, 1, True, False, False, False, ''),
    (1, 4, 12, 24, 200, 1, True, True, False, False, ''),          # Cout not a tile multiple
    (1, 4, 12, 24, 200, 1, False, True, False, False, 'drop gate'),
    (1, 16, 24, 64, 256, 2, True, True, False, False, ''),         # stride (2,1)
    (2, 4, 64, 64, 16, 1, True, False, False, True, ''),           # NCHW out
    (1, 5, 130, 8, 64, 1, True, True, False, False, ''),           # two column tiles, odd height
    (1, 5, 130, 8, 64, 1, False, True, False, False, ''),
]


def _f32_case(c):
    B, H, W, Cin, Cout, sh, circ, relu, pool, nchw, extras = c

    def fn(p):
        ops = _ops()
        g = _g(1, H * W + Cout)
        x = p(_n(g, (B, H, W, Cin)))
        pk = ops.PackedConv(p(_n(g, (Cout, Cin, 3, 3), (2.0 / (9 * Cin)) ** 0.5)), p(_n(g, (Cout,), 0.1)))
        kw = {}
        if 'drop' in extras:
            kw['drop_scale'] = p(torch.from_numpy(synth.dropout_scales(5, 0, B, Cout)))
        if 'gate' in extras:
            kw['gate'] = p(_n(g, (B, H, W, Cout)))
        return ops.conv3x3_fwd(x, pk, stride_h=sh, circular=circ, relu=relu, pool=pool, out_nchw=nchw,
                               want_pool_code='code' in extras, **kw)
    return fn


for _c in F32_CASES:
    case('conv_f32', 'conv3x3_fwd PackedConv', 'conv3x3_fwd-%dx%dx%dx%d-%d-s%d-c%d%s' % (_c[:6] + (_c[6], '-' + _c[10].replace(' ', '-') if _c[10] else '')),
         skew=True)(_f32_case(_c))

WINO_CLASSES = [(64, 128, False), (128, 128, True), (64, 64, True)]        # tests/test_conv_wino_gpu.py CLASSES


def _wino_case(cin, cout, pool):
    def fn(p):
        ops = _ops()
        g = _g(2, cin + cout)
        x = p(_n(g, (2, 13, 72, cin)))
        pk = ops.PackedConv(p(_n(g, (cout, cin, 3, 3), (2.0 / (9 * cin)) ** 0.5)), p(_n(g, (cout,), 0.1)), wino=True)
        y = ops.conv3x3_fwd(x, pk, circular=True, relu=True, pool=pool)
        assert ops.last_conv_form() == ('wino_h2' if ops.conv_wino() else 'direct')
        return y
    return fn


for _cin, _cout, _pool in WINO_CLASSES:
    case('conv_f32_wino', 'conv3x3_fwd PackedConv', 'conv3x3_fwd-wino-%d-%d-p%d' % (_cin, _cout, _pool), skew=True)(_wino_case(_cin, _cout, _pool))


@case('conv_f32_dgrad', 'conv3x3_fwd PackedConv', 'conv3x3_fwd-dgrad-dilate-out_h7', skew=True)
def _f32_dgrad(p):
    ops = _ops()
    g = _g(3)
    B, W, cin, cout = 2, 24, 16, 64                 # dz [B,4,W,16] stands for 7 rows (odd height under stride 2)
    dz = p(_n(g, (B, 4, W, cin)))
    pkt = ops.PackedConv(p(_n(g, (cin, cout, 3, 3), 0.1)), None, transpose_flip=True)
    gate = p(_n(g, (B, 7, W, cout)))
    scale = p(torch.from_numpy(synth.dropout_scales(6, 0, B, cout)))
    return ops.conv3x3_fwd(dz, pkt, stride_h=1, circular=True, relu=False, drop_scale=scale, gate=gate, dilate_h=True, out_h=7)


# ============================================================================ first layer, fused first two layers
def _first_case(B, C, H, W, bf16):
    def fn(p):
        ops = _ops()
        g = _g(4, C * 1000 + W)
        x = p(_n(g, (B, C, H, W)))
        pk = ops.PackedFirstConv(p(_n(g, (64, C, 3, 3), (2.0 / (9 * C)) ** 0.5)), p(_n(g, (64,), 0.1)), bf16=bf16)
        return ops.conv3x3_first_fwd(x, pk, circular=(C == 3))
    return fn


for _s in ((1, 3, 13, 99), (1, 1, 9, 40)):
    for _bf in (False, True):
        case('first_layer', 'conv3x3_first_fwd PackedFirstConv', 'conv3x3_first_fwd-%dx%dx%dx%d-bf16_%d' % (_s + (_bf,)), skew=True)(_first_case(*_s, bf16=_bf))


@case('first_layer', 'conv3x3_first_fwd', 'conv3x3_first_fwd-split_f16')
def _first_split(p):
    ops = _ops()
    g = _g(4, 77)
    pk = ops.PackedFirstConv(p(_n(g, (64, 3, 3, 3), 0.3)), p(_n(g, (64,), 0.1)))
    return ops.conv3x3_first_fwd(p(_n(g, (1, 3, 13, 99))), pk, circular=True, split_f16=True)


def _first2_case(B, C, H, W, train):
    def fn(p):
        ops = _ops()
        g = _g(5, C * 1000 + W)
        x = p(_n(g, (B, C, H, W)))
        pf = ops.PackedFirstConv(p(_n(g, (64, C, 3, 3), (2.0 / (9 * C)) ** 0.5)), p(_n(g, (64,), 0.1)), bf16=True)
        p2 = ops.PackedConvBf16(p(_n(g, (64, 64, 3, 3), 0.05)), p(_n(g, (64,), 0.1)))
        if train:
            out = ops.conv_first2_bf16_train(x, pf, p2, circular=True)
            assert ops.last_kernel_variant() == 'conv_first2_bf16_kernel<%d,train>' % (4 if C <= 4 else 8)
            return out
        return ops.conv_first2_bf16(x, pf, p2, circular=True)
    return fn


for _s, _t in (((1, 5, 9, 33), False), ((2, 3, 20, 70), False), ((1, 5, 10, 34), True), ((2, 3, 20, 70), True)):
    case('first2_bf16', 'conv_first2_bf16_train' if _t else 'conv_first2_bf16', 'conv_first2_bf16%s-%dx%dx%dx%d' % (('_train' if _t else '',) + _s),
         skew=True)(_first2_case(*_s, train=_t))


# ============================================================================ bf16 / fp16x3 conv forward and dgrad
def _bf16_fwd_case(c):
    B, H, W, Cin, Cout, sh, circ, relu, pool = c

    def fn(p):
        ops = _ops()
        g = _g(7, Cin + Cout)
        x = p(_n(g, (B, H, W, Cin)).bfloat16())
        pk = ops.PackedConvBf16(p(_n(g, (Cout, Cin, 3, 3), (2.0 / (9 * Cin)) ** 0.5)), p(_n(g, (Cout,), 0.1)))
        return ops.conv3x3_bf16_fwd(x, pk, stride_h=sh, circular=circ, relu=relu, pool=pool, out_nchw_f32=(Cout == 16),
                                    want_pool_code=pool)
    return fn


for _c in [(1, 12, 99, 16, 64, 1, True, True, True), (2, 16, 24, 32, 256, 2, True, True, False), (2, 4, 64, 64, 16, 1, True, False, False)]:
    case('conv_bf16', 'conv3x3_bf16_fwd PackedConvBf16', 'conv3x3_bf16_fwd-%dx%dx%dx%d-%d-s%d' % _c[:6], skew=True)(_bf16_fwd_case(_c))


def _bf16_dgrad_case(c):
    B, H, W, Cin, Cout, sh, circ = c            # tests/test_bf16_train_gpu.py DGRAD_CASES

    def fn(p):
        ops = _ops()
        g = _g(8, H * W)
        Ho = (H + 2 - 3) // sh + 1
        pt = ops.PackedConvBf16(p(_n(g, (Cout, Cin, 3, 3), 0.05)), None, transpose_flip=True)
        cpad = (Cout + 15) // 16 * 16
        gy = torch.zeros((B, Ho, W, cpad), dtype=torch.bfloat16)
        gy[..., :Cout] = _n(g, (B, Ho, W, Cout)).bfloat16()
        return ops.conv3x3_bf16_fwd(p(gy), pt, stride_h=1, circular=circ, relu=False,
                                    drop_scale=p(torch.from_numpy(synth.dropout_scales(8, 0, B, Cin))),
                                    gate=p(_n(g, (B, H, W, Cin)).bfloat16()), dilate_h=(sh == 2), out_h=H if sh == 2 else None)
    return fn


for _c in [(2, 8, 12, 256, 64, 2, True), (3, 7, 24, 64, 64, 2, False), (2, 4, 64, 64, 16, 1, False)]:
    case('conv_bf16', 'conv3x3_bf16_fwd PackedConvBf16', 'conv3x3_bf16_fwd-dgrad-%dx%dx%dx%d-%d-s%d' % _c[:6], skew=True)(_bf16_dgrad_case(_c))


@case('conv_bf16', 'conv3x3_bf16_fwd', 'conv3x3_bf16_fwd-weight-resident', skew=True, variant='conv3x3_bf16_wres_kernel*')
def _bf16_wres(p):
    """the smallest shape witw_bf16_wres_applies accepts: B * (H/8) * (W/16) * (Cout/64) = 32 * 256 units"""
    ops = _ops()
    assert ops.bf16_wres()
    x = p(_big(11, (2, 128, 512, 64), torch.bfloat16))
    pk = ops.PackedConvBf16(p(_big(12, (512, 64, 3, 3)) * 0.06), p(_big(13, (512,)) * 0.1))
    return ops.conv3x3_bf16_fwd(x, pk, circular=True, relu=True)


@case('conv_bf16', 'conv3x3_bf16_dgrad_gatebits', 'conv3x3_bf16_dgrad_gatebits', skew=True, variant='conv3x3_bf16_wres_kernel<gate_bits>')
def _bf16_gatebits(p):
    ops = _ops()
    B, H, W = 16, 128, 512                          # the smallest batch the weight-resident kernel takes at 64 -> 64 (tests/test_bf16_gpu.py)
    assert ops.gatebits_dgrad_ok(B, H, W, 64, 64)
    dz = p(_big(14, (B, H, W, 64), torch.bfloat16))
    bits = p(torch.randint(0, 256, (B, H, W, 8), generator=torch.Generator(DEV).manual_seed(15), device=DEV, dtype=torch.int32).to(torch.uint8))
    pt = ops.PackedConvBf16(p(_big(16, (64, 64, 3, 3)) * 0.06), None, transpose_flip=True)
    return ops.conv3x3_bf16_dgrad_gatebits(dz, pt, bits, circular=True)


def _f16x3_fwd_case(c):
    B, H, W, Cin, Cout, sh, circ, relu, pool = c

    def fn(p):
        ops = _ops()
        g = _g(9, Cin + Cout)
        xs = p(ops.nchw_to_split_f16(_n(g, (B, Cin, H, W)).to(DEV), Cin))
        pk = ops.PackedConvF16x3(p(_n(g, (Cout, Cin, 3, 3), (2.0 / (9 * Cin)) ** 0.5)), p(_n(g, (Cout,), 0.1)))
        return ops.conv3x3_f16x3_fwd(xs, pk, stride_h=sh, circular=circ, relu=relu, pool=pool, out_nchw_f32=(Cout == 16),
                                     want_pool_code=pool)
    return fn


for _c in [(1, 12, 99, 8, 64, 1, True, True, True), (2, 16, 24, 32, 256, 2, True, True, False), (2, 4, 64, 64, 16, 1, True, False, False),
           (1, 9, 130, 24, 136, 1, False, True, False)]:
    case('conv_f16x3', 'conv3x3_f16x3_fwd PackedConvF16x3', 'conv3x3_f16x3_fwd-%dx%dx%dx%d-%d-s%d' % _c[:6], skew=True)(_f16x3_fwd_case(_c))


@case('conv_f16x3', 'conv3x3_f16x3_fwd PackedConvF16x3', 'conv3x3_f16x3_fwd-dgrad', skew=True)
def _f16x3_dgrad(p):
    ops = _ops()
    g = _g(10)
    B, H, W, Cin, Cout = 3, 7, 24, 64, 64           # DGRAD_CASES row 3: odd height under stride 2
    pt = ops.PackedConvF16x3(p(_n(g, (Cout, Cin, 3, 3), 0.05)), None, transpose_flip=True)
    gy = p(ops.nchw_to_split_f16(_n(g, (B, Cout, 4, W)).to(DEV), Cout))
    gate = p(ops.nchw_to_split_f16(_n(g, (B, Cin, H, W)).to(DEV), Cin))
    return ops.conv3x3_f16x3_fwd(gy, pt, stride_h=1, circular=False, relu=False, gate=gate,
                                 drop_scale=p(torch.from_numpy(synth.dropout_scales(8, 0, B, Cin))), dilate_h=True, out_h=H)


# ============================================================================ weight gradients
def _wgrad_f32_case(B, H, W, Cin, Cout, sh, circ, out):
    def fn(p):
        ops = _ops()
        g = _g(20, H * W + Cout)
        Ho = (H + 2 - 3) // sh + 1
        x, dz = p(_n(g, (B, H, W, Cin))), p(_n(g, (B, Ho, W, Cout)))
        if out:     # the .grad views of a GradBucket: preallocated, between bands too
            return ops.conv3x3_wgrad(x, dz, Cin, stride_h=sh, circular=circ, out=(p(torch.zeros(Cout, Cin, 3, 3)), p(torch.zeros(Cout))))
        return ops.conv3x3_wgrad(x, dz, Cin, stride_h=sh, circular=circ)
    return fn


for _c in [(1, 5, 130, 8, 72, 1, True, False), (2, 7, 24, 64, 64, 2, False, False), (2, 7, 24, 64, 64, 2, False, True)]:
    case('wgrad', 'conv3x3_wgrad', 'conv3x3_wgrad-%dx%dx%dx%d-%d-s%d-c%d-out%d' % _c)(_wgrad_f32_case(*_c))


@case('wgrad', 'conv3x3_wgrad', 'conv3x3_wgrad-taps4')
def _wgrad_taps4(p):
    ops = _ops()
    g = _g(21)
    return ops.conv3x3_wgrad(p(_n(g, (2, 9, 30, 64))), p(_n(g, (2, 9, 30, 64))), 64, taps4=True)


WGRAD_LOW = [(5, 19, 37, 40, 24, 1, True), (3, 7, 20, 16, 256, 2, True), (10, 6, 12, 64, 16, 1, True)]


def _wgrad_bf16_case(c, layout, out=False):
    B, H, W, Cin, Cout, sh, circ = c

    def fn(p):
        ops = _ops()
        g = _g(22, H * W + Cout)
        Ho = (H + 2 - 3) // sh + 1
        x, dz = p(_n(g, (B, H, W, Cin)).bfloat16()), p(_n(g, (B, Ho, W, Cout)).bfloat16())
        kw = {'out': (p(torch.zeros(Cout, Cin, 3, 3)), p(torch.zeros(Cout)))} if out else {}
        return ops.conv3x3_wgrad_bf16(x, dz, Cin, stride_h=sh, circular=circ, layout=layout, **kw)
    return fn


def _wgrad_f16x3_case(c):
    B, H, W, Cin, Cout, sh, circ = c

    def fn(p):
        ops = _ops()
        g = _g(23, H * W + Cout)
        Ho = (H + 2 - 3) // sh + 1
        xs = p(ops.nchw_to_split_f16(_n(g, (B, Cin, H, W)).to(DEV), Cin))
        gs = p(ops.nchw_to_split_f16(_n(g, (B, Cout, Ho, W)).to(DEV), Cout))
        # the launcher computes the bias gradient only where Cout / 8 divides 256 and says so otherwise
        return ops.conv3x3_wgrad_f16x3(xs, gs, Cin, stride_h=sh, circular=circ, want_bias=256 % (Cout // 8) == 0)
    return fn


for _c in WGRAD_LOW:
    for _l in ('nhwc', 'octet'):
        case('wgrad', 'conv3x3_wgrad_bf16', 'conv3x3_wgrad_bf16-%s-%dx%dx%dx%d-%d-s%d' % ((_l,) + _c[:6]))(_wgrad_bf16_case(_c, _l))
    case('wgrad', 'conv3x3_wgrad_f16x3', 'conv3x3_wgrad_f16x3-%dx%dx%dx%d-%d-s%d' % _c[:6])(_wgrad_f16x3_case(_c))
case('wgrad', 'conv3x3_wgrad_bf16', 'conv3x3_wgrad_bf16-nhwc-out')(_wgrad_bf16_case(WGRAD_LOW[0], 'nhwc', out=True))


# ============================================================================ pooling backward
def _pool_code(g, shape):
    return torch.from_numpy(g.integers(0, 4, shape).astype(np.uint8))


@case('pool_bwd', 'maxpool2x2_bwd', 'maxpool2x2_bwd-2x10x70')
def _pool_bwd(p):
    g = _g(30)
    return _ops().maxpool2x2_bwd(p(_n(g, (2, 5, 35, 64))), p(_pool_code(g, (2, 5, 35, 64))), (10, 70))


@case('pool_bwd', 'maxpool2x2_bwd_bf16', 'maxpool2x2_bwd_bf16-2x10x70')
def _pool_bwd_bf16(p):
    g = _g(31)
    return _ops().maxpool2x2_bwd_bf16(p(_n(g, (2, 5, 35, 64)).bfloat16()), p(_pool_code(g, (2, 5, 35, 64))), (10, 70))


@case('pool_bwd', 'maxpool2x2_bwd_split', 'maxpool2x2_bwd_split-2x10x70')
def _pool_bwd_split(p):
    ops = _ops()
    g = _g(32)
    dy = p(ops.nchw_to_split_f16(_n(g, (2, 64, 5, 35)).to(DEV), 64))
    return ops.maxpool2x2_bwd_split(dy, p(_pool_code(g, (2, 5, 35, 64))), (10, 70))


# ============================================================================ layout converters (odd shapes of test_nchw_f32_to_nhwc_bf16_is_exact)
ODD = [(3, 5, 33, 70), (1, 1, 5, 3)]


def _layout(name, entries, build):
    for s in ODD:
        case('layout', entries, '%s-%dx%dx%dx%d' % ((name,) + s))(lambda p, s=s: build(_ops(), p, _g(40, s[1] * 100 + s[3]), s))


_layout('nchw_to_nhwc8', 'nchw_to_nhwc8', lambda ops, p, g, s: ops.nchw_to_nhwc8(p(_n(g, s))))
_layout('nchw_to_nhwc', 'nchw_to_nhwc', lambda ops, p, g, s: ops.nchw_to_nhwc(p(_n(g, s)), 24))
_layout('nchw_to_nhwc_bf16', 'nchw_to_nhwc_bf16', lambda ops, p, g, s: ops.nchw_to_nhwc_bf16(p(_n(g, s)), 16))
_layout('nchw_to_split_f16', 'nchw_to_split_f16', lambda ops, p, g, s: ops.nchw_to_split_f16(p(_n(g, s)), 8))
_layout('split_f16_to_f32', 'split_f16_to_f32', lambda ops, p, g, s: ops.split_f16_to_f32(p(ops.nchw_to_split_f16(_n(g, s).to(DEV), 8))))
_layout('nhwc_bf16_to_octet', 'nhwc_bf16_to_octet', lambda ops, p, g, s: ops.nhwc_bf16_to_octet(p(_n(g, (s[0], s[2], s[3], 16)).bfloat16())))
_layout('split_f16_to_octet', 'split_f16_to_octet', lambda ops, p, g, s: ops.split_f16_to_octet(p(ops.nchw_to_split_f16(_n(g, s).to(DEV), 8))))
_layout('space_to_depth2', 'space_to_depth2', lambda ops, p, g, s: ops.space_to_depth2(p(_n(g, (s[0], s[2], s[3], s[1])))))
_layout('space_to_depth2-quad', 'space_to_depth2',
        lambda ops, p, g, s: ops.space_to_depth2(p(_n(g, (s[0], s[2], s[3], 8))), valid_hw=(s[2] - 1, s[3] - 1), cpad=32, scale=p(_n(g, (8,))), shift=p(_n(g, (8,)))))
_layout('space_to_depth2-nchw', 'space_to_depth2', lambda ops, p, g, s: ops.space_to_depth2(p(_n(g, s).abs() * 50), in_nchw=True, normalize=True))
_layout('space_to_depth2_mosaic', 'space_to_depth2_mosaic', lambda ops, p, g, s: ops.space_to_depth2_mosaic(p(_n(g, (s[0], s[2], s[3], 8))), 2))
_layout('depth_to_space2', 'depth_to_space2',
        lambda ops, p, g, s: ops.depth_to_space2(p(_n(g, (s[0], (s[2] + 1) // 2, (s[3] + 1) // 2, 4 * 8))), torch.empty((s[0], s[2] + 1, s[3], 8)), (s[2], s[3])))
_layout('conv4x4_to_k3', 'conv4x4_to_k3', lambda ops, p, g, s: ops.conv4x4_to_k3(p(_n(g, (s[3], s[1], 4, 4))), (4 * s[1] + 7) // 8 * 8))
_layout('k3_to_conv4x4', 'k3_to_conv4x4', lambda ops, p, g, s: ops.k3_to_conv4x4(p(_n(g, (s[3], (4 * s[1] + 7) // 8 * 8, 3, 3))), s[1]))


# ============================================================================ matching
def _emb(Bo, Bs, We, seed=50):
    return (torch.from_numpy(synth.embeddings(seed, 1, (Bo, 16, 4, 64))), torch.from_numpy(synth.embeddings(seed, 2, (Bs, 16, 4, We))))


def _words(Bs, seed):
    """shift masks: a few allowed shifts per query, one query without a prior (0), one with bit 63"""
    w = torch.from_numpy(_g(51, seed).integers(1, 2 ** 62, (Bs,)).astype(np.int64))
    w[0] = 0
    if Bs > 1:
        w[1] = -(2 ** 63) | 5
    return w


def _fixed(p, we):
    """the workspace of match_fwd_fixed is defined over its norms, [Bo,64] + [Bs] floats; what follows is the launch's own grouping
    table, sized for the worst case and written only as far as this batch's shifts need (ops.match_fwd_fixed, include/witw_hip.h)"""
    ori, dist, score, ws = _ops().match_fwd_fixed(*[p(t) for t in _emb(37, 29, we)], shift=p(_words(29, we) >> 3),
                                                  want_score=True, want_workspace=True)
    return ori, dist, score, ws[:37 * 64 + 29]


for _we in (33, 64, 12):
    case('match', 'match_fwd', 'match_fwd-37x29-We%d' % _we, skew=True)(
        lambda p, we=_we: _ops().match_fwd(*[p(t) for t in _emb(37, 29, we)]))
    case('match', 'match_fwd', 'match_fwd-masked-37x29-We%d' % _we, skew=True)(
        lambda p, we=_we: _ops().match_fwd(*[p(t) for t in _emb(37, 29, we)], shift_mask=p(_words(29, we))))
    case('match', 'match_fwd', 'match_fwd-score-ws-37x29-We%d' % _we, skew=True)(
        lambda p, we=_we: _ops().match_fwd(*[p(t) for t in _emb(37, 29, we)], want_score=True, want_workspace=True))
    case('match', 'match_fwd_fixed', 'match_fwd_fixed-37x29-We%d' % _we, skew=True)(lambda p, we=_we: _fixed(p, we))


def _match_saved(ops, p, Bo, Bs, We):
    ov, su = [p(t) for t in _emb(Bo, Bs, We)]
    ori, dist, score, ws = ops.match_fwd(ov, su, want_score=True, want_workspace=True)
    return ov, su, p(ori), p(dist), p(score), p(ws)


@case('match', 'match_bwd', 'match_bwd-37x29-We33', skew=True,
      tol=(1e-6, 'tests/test_batch_hard_gpu.py::test_match_bwd_pairs_equals_dense_match_bwd: 1e-6 of the norm'))
def _match_bwd(p):
    ops = _ops()
    ov, su, ori, _d, score, ws = _match_saved(ops, p, 37, 29, 33)
    return ops.match_bwd(ov, su, ori, score, ws, p(_n(_g(52), (37, 29))))


@case('match', 'match_bwd_pairs', 'match_bwd_pairs-40x24-We12', skew=True)
def _match_bwd_pairs(p):
    ops = _ops()
    Bo, Bs = 40, 24
    ov, su, ori, _d, score, ws = _match_saved(ops, p, Bo, Bs, 12)
    g = torch.Generator().manual_seed(300)
    n = 3 * Bo
    po = torch.randint(0, Bo, (n,), generator=g, dtype=torch.int32)
    ps = torch.randint(0, Bs, (n,), generator=g, dtype=torch.int32)
    po[:6], ps[6:12] = 3, 2
    po[15], ps[16] = -1, -1                      # ignored entries
    return ops.match_bwd_pairs(ov, su, ori, score, ws, p(po), p(ps), p(torch.randn((n,), generator=g)))


for _side, _w in ((True, 64), (False, 33), (False, 64), (False, 12)):
    case('match', 'match_spectrum', 'match_spectrum-%s-We%d' % ('ov' if _side else 'su', _w), skew=True)(
        lambda p, side=_side, w=_w: _ops().match_spectrum(p(_emb(37, 29, w)[0 if side else 1]), overhead=side))

for _bo in (40, 33):
    for _we in (33, 64, 12):
        case('match', 'match_fwd_dft match_spectrum', 'match_fwd_dft-%dx5-We%d' % (_bo, _we), skew=True)(
            lambda p, bo=_bo, we=_we: _ops().match_fwd_dft(*[p(t) for t in _emb(bo, 5, we)], want_score=True))
        case('match', 'match_fwd_dft', 'match_fwd_dft-gap-%dx5-We%d' % (_bo, _we), skew=True)(
            lambda p, bo=_bo, we=_we: _ops().match_fwd_dft(*[p(t) for t in _emb(bo, 5, we)], want_gap=True))
        case('match', 'match_fwd_dft', 'match_fwd_dft-masked-%dx5-We%d' % (_bo, _we), skew=True)(
            lambda p, bo=_bo, we=_we: _ops().match_fwd_dft(*[p(t) for t in _emb(bo, 5, we)], want_gap=True, shift_mask=p(_words(5, we))))
    case('match', 'match_fwd_dft', 'match_fwd_dft-values-only-%dx5' % _bo, skew=True)(
        lambda p, bo=_bo: _ops().match_fwd_dft(*[p(t) for t in _emb(bo, 5, 64)], want_orientation=False, want_workspace=True))


def _pairs(Bo, Bs, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, Bo, (n,), generator=g, dtype=torch.int32), torch.randint(0, Bs, (n,), generator=g, dtype=torch.int32))


def _match_pairs_case(masked):
    def fn(p):
        ops = _ops()
        Bo, Bs = 37, 29
        ov, su, _o, _d, _s, ws = _match_saved(ops, p, Bo, Bs, 33)
        po, ps = _pairs(Bo, Bs, 50, 53)
        return ops.match_pairs(ov, su, p(ws[:Bo * 64].clone()), p(ws[Bo * 64:Bo * 64 + Bs].clone()), p(po), p(ps),
                               shift_mask=p(_words(Bs, 3)) if masked else None)
    return fn


case('match', 'match_pairs', 'match_pairs', skew=True)(_match_pairs_case(False))
case('match', 'match_pairs', 'match_pairs-masked', skew=True)(_match_pairs_case(True))


def _dist(Bo, Bs, seed=54):
    return torch.from_numpy(_g(seed, Bo * Bs).random((Bo, Bs), dtype=np.float32) * 4)


case('match', 'rank_count', 'rank_count-37x29', skew=True)(lambda p: _ops().rank_count(p(_dist(37, 29)), 3))
case('match', 'rank_count_thresh', 'rank_count_thresh-37x29', skew=True)(
    lambda p: _ops().rank_count_thresh(p(_dist(37, 29)), p(_dist(1, 29, 55).reshape(29))))


def _sorted_pairs(outs):
    """rank_count_band appends its (row, query) pairs in the order the workgroups finish: compare them as a set"""
    counts, po, ps = outs
    return [counts, torch.sort(po.long() * (1 << 32) + ps.long()).values]


case('match', 'rank_count_band', 'rank_count_band-37x29', skew=True, canon=_sorted_pairs)(
    lambda p: _ops().rank_count_band(p(_dist(37, 29)), p(_dist(1, 29, 55).reshape(29)), 0.2))


def _resolved_case(masked):
    def fn(p):
        ops = _ops()
        Bo, Bs = 37, 29
        ov, su, _o, dist, _s, ws = _match_saved(ops, p, Bo, Bs, 33)
        thr = p(dist[3].clone())              # one gallery row's distances as the thresholds: that row always counts
        return ops.rank_count_resolved(dist, thr, 1e-3, ov, su, p(ws[:Bo * 64].clone()), p(ws[Bo * 64:Bo * 64 + Bs].clone()),
                                       shift_mask=p(torch.zeros(Bs, dtype=torch.int64)) if masked else None)
    return fn


case('match', 'rank_count_resolved', 'rank_count_resolved', skew=True)(_resolved_case(False))
case('match', 'rank_count_resolved', 'rank_count_resolved-masked', skew=True)(_resolved_case(True))
for _rows, _k in ((37, 5), (37, 32), (40, 32), (7, 32), (3, 5)):        # the last two: fewer gallery rows than k
    case('match', 'topk_smallest', 'topk_smallest-%dx29-k%d' % (_rows, _k), skew=True)(
        lambda p, rows=_rows, k=_k: _ops().topk_smallest(p(_dist(rows, 29)), k, row_offset=1000))


@case('match', 'crop_overhead', 'crop_overhead-5x7-We33')
def _crop(p):
    ov = p(_emb(5, 7, 33)[0])
    return _ops().crop_overhead(ov, p(torch.from_numpy(_g(56).integers(0, 64, (5, 7)).astype(np.int64))), 33)


@case('match', 'l2_distance', 'l2_distance-5x7-We33')
def _l2(p):
    g = _g(57)
    return _ops().l2_distance(p(_n(g, (5, 7, 16, 4, 33))), p(_n(g, (7, 16, 4, 33))))


# ============================================================================ losses
@case('loss', 'triplet_loss_fwd', 'triplet_loss_fwd-37', skew=True)
def _tl_fwd(p):
    return _ops().triplet_loss_fwd(p(_dist(37, 37)), 10.)


@case('loss', 'triplet_loss_bwd', 'triplet_loss_bwd-37', skew=True)
def _tl_bwd(p):
    ops = _ops()
    D = p(_dist(37, 37))
    _loss, ws = ops.triplet_loss_fwd(D, 10.)
    return ops.triplet_loss_bwd(D, p(ws), p(torch.ones(1)), 10.)


def _slab(p, r):
    """slab r of a 2-slab split of B = 37 (19 + 18 columns)"""
    D = _dist(37, 37)
    col0, b = (0, 19) if r == 0 else (19, 18)
    return p(D[:, col0:col0 + b].contiguous()), p(D.diagonal().contiguous()), col0


for _r in (0, 1):
    @case('loss', 'triplet_loss_slab_fwd', 'triplet_loss_slab_fwd-37-slab%d' % _r, skew=True)
    def _tl_slab_fwd(p, r=_r):
        slab, diag, col0 = _slab(p, r)
        return _ops().triplet_loss_slab_fwd(slab, diag, col0, 10.)

    @case('loss', 'triplet_loss_slab_sig', 'triplet_loss_slab_sig-37-slab%d' % _r, skew=True)
    def _tl_slab_sig(p, r=_r):
        slab, diag, col0 = _slab(p, r)
        return _ops().triplet_loss_slab_sig(slab, diag, col0, 10.)

    @case('loss', 'triplet_loss_slab_bwd', 'triplet_loss_slab_bwd-37-slab%d' % _r, skew=True)
    def _tl_slab_bwd(p, r=_r):
        ops = _ops()
        slab, diag, col0 = _slab(p, r)
        rowsig, colsig = ops.triplet_loss_slab_sig(slab, diag, col0, 10.)
        return ops.triplet_loss_slab_bwd(slab, diag, p(rowsig), p(colsig), p(torch.ones(1)), col0, 10.)


def _bh_matrix(B, seed):
    """tests/test_batch_hard_gpu.py _matrix: ties, +-inf entries"""
    g = torch.Generator().manual_seed(seed)
    D = torch.rand((B, B), generator=g) * 4
    if B >= 3:
        D[:, B - 1] = D[:, 1]
        D[B - 2, :] = D[0, :]
        D[1, 1] = float('-inf')
        D[2, 1] = float('inf')
    return D


for _B in (2, 3, 37):
    case('loss', 'batch_hard_fwd', 'batch_hard_fwd-%d' % _B, skew=True)(lambda p, B=_B: _ops().batch_hard_fwd(p(_bh_matrix(B, 100 + B)), 10.))

    @case('loss', 'batch_hard_bwd', 'batch_hard_bwd-%d' % _B, skew=True)
    def _bh_bwd(p, B=_B):
        ops = _ops()
        D = p(_bh_matrix(B, 100 + B))
        _l, rv, ri, cv, ci = ops.batch_hard_fwd(D, 10.)
        return ops.batch_hard_bwd(D, p(rv), p(ri), p(cv), p(ci), p(torch.tensor([0.7])), 10.)

    @case('loss', 'batch_hard_pairs', 'batch_hard_pairs-%d' % _B, skew=True)
    def _bh_pairs(p, B=_B):
        ops = _ops()
        D = p(_bh_matrix(B, 100 + B))
        _l, rv, ri, cv, ci = ops.batch_hard_fwd(D, 10.)
        return ops.batch_hard_pairs(p(D.diagonal().contiguous()), p(rv), p(ri), p(cv), p(ci), p(torch.tensor([0.7])), 0, 10.)


@case('loss', 'batch_hard_slab_mine', 'batch_hard_slab_mine-37x5', skew=True)
def _bh_mine(p):
    return _ops().batch_hard_slab_mine(p(_bh_matrix(37, 44)[:, 10:15].contiguous()), 10)


@case('loss', 'batch_hard_merge_rows', 'batch_hard_merge_rows-7x37', skew=True)
def _bh_merge(p):
    g = torch.Generator().manual_seed(45)
    return _ops().batch_hard_merge_rows(p(torch.rand((7, 37), generator=g)), p(torch.randint(0, 37, (7, 37), generator=g)))


@case('loss', 'batch_hard_slab_loss', 'batch_hard_slab_loss-37x5', skew=True)
def _bh_slab_loss(p):
    D = _bh_matrix(37, 44)
    g = torch.Generator().manual_seed(46)
    return _ops().batch_hard_slab_loss(p(D[:, 10:15].contiguous()), p(torch.rand((37,), generator=g)), p(torch.rand((5,), generator=g)), 10, 10.)


@case('loss', 'pairwise_sqdist', 'pairwise_sqdist-37x29x70')
def _sqdist(p):
    g = _g(60)
    return _ops().pairwise_sqdist(p(_n(g, (37, 70))), p(_n(g, (29, 70))), take_sqrt=True)


for _soft in (False, True):
    case('loss', 'exhaustive_triplet_loss', 'exhaustive_triplet_loss-37-soft%d' % _soft)(
        lambda p, soft=_soft: _ops().exhaustive_triplet_loss(p(_dist(37, 37)), soft_margin=soft))

    @case('loss', 'exhaustive_triplet_loss_bwd', 'exhaustive_triplet_loss_bwd-37-soft%d' % _soft)
    def _ex_bwd(p, soft=_soft):
        ops = _ops()
        g = _g(61)
        e1, e2 = p(_n(g, (37, 70))), p(_n(g, (37, 70)))
        D = p(ops.pairwise_sqdist(e1, e2))
        return ops.exhaustive_triplet_loss_bwd(e1, e2, D, p(torch.ones(1)), soft_margin=soft)


case('loss', 'dropout2d_scales', 'dropout2d_scales-3x5x37')(lambda p: _ops().dropout2d_scales(7, 1, 11, 0, [17, 19, 21], 5, 37, 0.2, DEV))


# ============================================================================ preprocessing
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _img(seed, shape):
    return torch.from_numpy(synth.images_u8(seed, 1, shape))


case('preprocess', 'resize_bilinear', 'resize_bilinear-up-normalise')(lambda p: _ops().resize_bilinear(p(_img(70, (2, 3, 37, 53))), (128, 99), MEAN, STD))
case('preprocess', 'resize_bilinear', 'resize_bilinear-down')(lambda p: _ops().resize_bilinear(p(_img(71, (1, 3, 37, 53))), (9, 7)))
case('preprocess', 'resize_bilinear', 'resize_bilinear-1x1')(lambda p: _ops().resize_bilinear(p(_img(72, (1, 1, 1, 1))), (3, 5)))
case('preprocess', 'normalize', 'normalize-2x3x37x53')(lambda p: _ops().normalize(p(_img(73, (2, 3, 37, 53))), MEAN, STD))


def _desc(p, images):
    """resize_batched / polar_from_raw descriptor rows over placed fp32 CHW images; the images are returned to keep them alive"""
    keep = [p(t) for t in images]
    rows = [(t.data_ptr(), t.shape[1], t.shape[2], 0, t.shape[0]) for t in keep]
    return keep, p(torch.tensor(rows, dtype=torch.int64))


@case('preprocess', 'resize_batched', 'resize_batched-3-images')
def _resize_batched(p):
    keep, desc = _desc(p, [_img(74, (3, 37, 53)), _img(75, (3, 20, 91)), _img(76, (3, 64, 40))])
    return _ops().resize_batched(desc, 3, 3, (32, 99), mean=MEAN, std=STD), keep


case('preprocess', 'polar_transform', 'polar_transform-37')(lambda p: _ops().polar_transform(p(_n(_g(77), (2, 3, 37, 37))), 16, 50))
case('preprocess', 'polar_from_raw', 'polar_from_raw-tensor')(
    lambda p: _ops().polar_from_raw(p(_img(78, (2, 3, 37, 53))), mean=MEAN, std=STD, size=128, h_s=64, w_s=256))


@case('preprocess', 'polar_from_raw', 'polar_from_raw-desc')
def _polar_desc(p):
    keep, desc = _desc(p, [_img(79, (3, 37, 53)), _img(80, (3, 150, 91))])
    return _ops().polar_from_raw(desc=desc, kind=0, batch=2, channels=3, mean=MEAN, std=STD, size=128, h_s=64, w_s=256), keep


@case('preprocess', 'bilinear_interpolate', 'bilinear_interpolate-37x53')
def _bilin(p):
    g = _g(81)
    return _ops().bilinear_interpolate(p(_n(g, (3, 37, 53))), g.random((11, 13)) * 60 - 4, g.random((11, 13)) * 44 - 4)


case('preprocess', 'rotate_nearest', 'rotate_nearest-3x37x53')(
    lambda p: _ops().rotate_nearest(p(_n(_g(82), (3, 2, 37, 53))), [33.3, 90.0, 301.0]))


# ============================================================================ baseline model
def _taps4(p, g, Cin, Cout):
    k3 = _n(g, (Cout, Cin, 3, 3), 0.05)
    k3[:, :, 0, :] = 0
    k3[:, :, :, 0] = 0
    return _ops().PackedConv(p(k3), p(_n(g, (Cout,), 0.1)), taps4=True), p(1 + _n(g, (Cout,), 0.1)), p(_n(g, (Cout,), 0.1))


@case('baseline', 'conv4x4s2_first', 'conv4x4s2_first-4x1x65x130', variant='conv4x4s2_first_kernel<1>')
def _c44(p):
    g = _g(90)
    return _ops().conv4x4s2_first(p(_img(90, (4, 1, 65, 130))), p(_n(g, (64, 1, 4, 4), 0.1)), p(_n(g, (64,), 0.1)), p(1 + _n(g, (64,), 0.1)),
                                  p(_n(g, (64,), 0.1)))


@case('baseline', 'conv_taps4_s2d', 'conv_taps4_s2d-2x9x30')
def _t4s2d(p):
    g = _g(91)
    pk, sc, sh = _taps4(p, g, 64, 64)
    return _ops().conv_taps4_s2d(p(_n(g, (2, 9, 30, 64))), pk, (8, 29), lrelu_slope=0.2, post_scale=sc, post_shift=sh)


@case('baseline', 'conv3x3_fwd', 'conv3x3_fwd-taps4-2x9x30')
def _t4fwd(p):
    g = _g(92)
    pk, sc, sh = _taps4(p, g, 64, 64)
    return _ops().conv3x3_fwd(p(_n(g, (2, 9, 30, 64))), pk, relu=False, lrelu_slope=0.2, post_scale=sc, post_shift=sh)


def _splitk_case(B, gm, h, Cin, Cout, ksplit):
    def fn(p):
        g = _g(93, Cin + h)
        pk, sc, sh = _taps4(p, g, Cin, Cout)
        Bm = (B + gm * gm - 1) // (gm * gm)
        return _ops().conv_taps4_splitk(p(_n(g, (Bm, gm * h, gm * h, Cin))), pk, B, gm, (h - 1, h - 1), lrelu_slope=0.2, post_scale=sc,
                                        post_shift=sh, ksplit=ksplit)
    return fn


for _c in [(5, 2, 8, 256, 128, 3), (3, 1, 12, 64, 64, 8), (3, 1, 12, 64, 64, 1)]:        # uneven K slices over a mosaic; all 8 chunks; one slice
    case('baseline', 'conv_taps4_splitk', 'conv_taps4_splitk-%dx%dx%d-%d-%d-k%s' % _c)(_splitk_case(*_c))


@case('baseline', 'gem_pool', 'gem_pool-3x7x9-into-columns')
def _gem(p):
    g = _g(94)
    out = p(torch.zeros(3, 160))                    # the embedding: this launch owns columns 64 .. 127 of 160
    return _ops().gem_pool(p(_n(g, (3, 7, 9, 64)).abs() + 0.1), (5, 9), out, 64, 3., p(1 + _n(g, (64,), 0.1)), p(_n(g, (64,), 0.01).abs()))


@case('baseline', 'gem_pool_bwd', 'gem_pool_bwd-3x7x9')
def _gem_bwd(p):
    ops = _ops()
    g = _g(95)
    a, sc, sh = p(_n(g, (3, 7, 9, 64)).abs() + 0.1), p(1 + _n(g, (64,), 0.1)), p(_n(g, (64,), 0.01).abs())
    f = ops.gem_pool(a, (5, 9), torch.zeros((3, 160), device=DEV), 64, 3., sc, sh)
    df = p(_n(g, (3, 160)))
    fresh = ops.gem_pool_bwd(a, sc, sh, p(f), df, (5, 9), 64, 3.)
    acc = ops.gem_pool_bwd(a, sc, sh, p(f), df, (5, 9), 64, 3., out=p(_n(g, (3, 7, 9, 64))))     # accumulating form, preallocated
    return fresh, acc


case('baseline', 'embed_normalize_', 'embed_normalize_-3x161')(lambda p: _ops().embed_normalize_(p(_n(_g(96), (3, 161)))))
case('baseline', 'embed_normalize_bwd', 'embed_normalize_bwd-3x161')(
    lambda p: _ops().embed_normalize_bwd(p(_n(_g(97), (3, 161))), p(_n(_g(98), (3, 161)))))


def _bn_case(B, Hp, Wp, H, W, C, s2d):
    def fn(p):
        ops = _ops()
        g = _g(99, C + Hp)
        a = p(torch.nn.functional.leaky_relu(_n(g, (B, Hp, Wp, C)), 0.2))
        gamma, beta = p(1 + _n(g, (C,), 0.1)), p(_n(g, (C,), 0.1))
        rm, rvar = p(torch.zeros(C)), p(torch.ones(C))
        stats = ops.bn_train_stats(a, (H, W), gamma, beta, rm, rvar)
        dy = _n(g, (B, Hp, Wp, C))
        dy[:, H:] = 0
        dy[:, :, W:] = 0
        dy = p(ops.space_to_depth2(dy.to(DEV), valid_hw=(H, W), cpad=4 * C)) if s2d else p(dy)
        return stats, rm, rvar, ops.bn_lrelu_bwd(a, dy, (H, W), p(stats[0]), p(stats[1]), gamma, 0.2, dy_s2d=s2d)
    return fn


for _c in [(3, 10, 12, 9, 11, 64, False), (2, 8, 8, 7, 7, 128, True), (2, 6, 10, 6, 9, 6, False)]:
    case('baseline', 'bn_train_stats bn_lrelu_bwd', 'bn_train_stats+bn_lrelu_bwd-%dx%dx%d-%dx%d-%d-s2d%d' % _c)(_bn_case(*_c))


# ============================================================================ optimiser
def _adam_case(n):
    def fn(p):
        g = _g(110, n)
        t = [p(_n(g, (n,))), p(_n(g, (n,))), p(_n(g, (n,), 0.1)), p(_n(g, (n,)).abs() * 0.01)]
        _ops().adam_step(t[0], t[1], t[2], t[3], 3)
        return t
    return fn


for _nn in (1, 255, 257, 4099):
    case('adam', 'adam_step', 'adam_step-%d' % _nn, skew=True)(_adam_case(_nn))


@case('adam', 'adam_step_multi', 'adam_step_multi-1-255-257-4099', skew=True)
def _adam_multi(p):
    g = _g(111)
    sizes = (1, 255, 257, 4099)
    groups = [[p(_n(g, (n,))) for n in sizes], [p(_n(g, (n,))) for n in sizes], [p(_n(g, (n,), 0.1)) for n in sizes],
              [p(_n(g, (n,)).abs() * 0.01) for n in sizes]]
    _ops().adam_step_multi(groups[0], groups[1], groups[2], groups[3], [3, 1, 7, 2])
    return groups


# ============================================================================ the runner
def _plain_place(t):
    return t.detach().to(DEV).contiguous()


def _flat(r, acc=None):
    acc = [] if acc is None else acc
    if isinstance(r, torch.Tensor):
        acc.append(r)
    elif isinstance(r, (tuple, list)):
        for x in r:
            _flat(x, acc)
    elif r is not None and isinstance(getattr(r, 'data', None), torch.Tensor):
        acc.append(r.data)
    return acc


def _bits(t):
    return t.detach().reshape(-1).contiguous().view(torch.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _in_arena(c, monkeypatch, skew, int_fill=0xA5):
    from witw_amd import ops
    arena = Arena(DEV, skew_bytes=skew, int_fill=int_fill)
    with monkeypatch.context() as m:
        m.setattr(ops, 'torch', ArenaTorch(arena))
        got = c.fn(arena.place)
        variant = ops.last_kernel_variant()
    return arena, got, variant


def _run_contract(c, monkeypatch, skew=0):
    canon = c.canon or (lambda outs: outs)
    a = canon(_flat(c.fn(_plain_place)))
    b = canon(_flat(c.fn(_plain_place)))
    torch.cuda.synchronize()
    assert len(a) == len(b) and a, 'the case returns no tensor'
    repeatable = all(_same_bits(x, y) for x, y in zip(a, b))
    arena, got, variant = _in_arena(c, monkeypatch, skew)
    try:
        arena.check(got)                                                                        # P1, P2
    except ArenaError as e:
        # an integer output may hold the canary's value by right (a gate byte 0xA5): stored iff a run with the other fill leaves
        # none of those elements at the OTHER fill. Everything else is a finding.
        soft = [f for f in e.findings if f['kind'] == 'uncovered' and f['dtype'] == torch.uint8]
        if len(soft) != len(e.findings):
            raise
        arena2, got2, _v = _in_arena(c, monkeypatch, skew, int_fill=ALT_BAND_BYTE)
        flat2 = _flat(got2)
        arena2.live = []
        torch.cuda.synchronize()
        for f in soft:
            never = f['mask'] & (flat2[f['ret']] == ALT_BAND_BYTE)
            assert not bool(never.any()), '%s\n(%d of them hold the fill byte under either fill: never written)' % (f['text'], int(never.sum()))
    got = canon(_flat(got))
    if c.variant is not None:
        assert variant.startswith(c.variant[:-1]) if c.variant.endswith('*') else variant == c.variant, variant
    assert len(got) == len(a)
    for k, (x, y) in enumerate(zip(got, a)):                                                    # P4, then P3
        if y.is_floating_point() and bool(torch.isfinite(y.float()).all()):
            bad = ~torch.isfinite(x.float())
            assert not bool(bad.any()), 'output %d: %d non-finite element(s) from finite inputs between NaN bands, first at %s' % (
                k, int(bad.sum()), tuple(bad.nonzero()[0].tolist()))
    for k, (x, y) in enumerate(zip(got, a)):
        if repeatable:
            assert _same_bits(x, y), 'output %d %s changes with where its operands are placed: %d element(s) differ' % (
                k, tuple(y.shape), int((x != y).sum()) if x.shape == y.shape else -1)
        else:
            assert c.tol is not None, 'two plain calls differ bitwise and the case names no tolerance'
            if y.is_floating_point():
                assert float((x.double() - y.double()).norm()) <= c.tol[0] * float(y.double().norm()), (k, c.tol)
            else:
                assert torch.equal(x, y)


@pytest.mark.parametrize('c', CASES, ids=[c.id for c in CASES])
def test_memory_contract(c, monkeypatch):
    _run_contract(c, monkeypatch)


SKEWED = [c for c in CASES if c.skew]


@pytest.mark.parametrize('c', SKEWED, ids=[c.id for c in SKEWED])
def test_alignment_16_bytes(c, monkeypatch):
    """Outcome (i) for every conv forward, match, top-k, rank-count, loss and Adam entry: correct with every operand 16 bytes
    past a 256-byte boundary. The kernels' widest global accesses (float4 / 8 x bf16 loads and stores, LDS-DMA and buffer loads of
    16 bytes per lane) need the 16-byte alignment a contiguous tensor of whole pixels / embedding rows keeps; none assumes more."""
    _run_contract(c, monkeypatch, skew=16)


# ============================================================================ batch isolation
def isolation(id, variant=None):
    def deco(fn):
        ISOLATION.append((id, fn, variant))
        return fn
    return deco


def _nan_but(x, keep, dim=0):
    y = torch.full_like(x, float('nan'))
    idx = [slice(None)] * x.dim()
    idx[dim] = keep
    y[tuple(idx)] = x[tuple(idx)]
    return y


def _iso_conv(id, build, keep=1):
    """build(ops, x) -> output with the batch in dim 0; x: the clean batch on the device"""
    @isolation(id)
    def fn():
        ops = _ops()
        x, run = build(ops)
        clean = run(x)
        v_clean = ops.last_kernel_variant()
        dirty = run(_nan_but(x, keep))
        assert ops.last_kernel_variant() == v_clean
        return [(clean[keep], dirty[keep])]
    return fn


def _iso_f32(ops):
    g = _g(120)
    pk = ops.PackedConv(_n(g, (200, 24, 3, 3), 0.07).to(DEV), _n(g, (200,), 0.1).to(DEV))
    return _n(g, (3, 4, 12, 24)).to(DEV), lambda x: ops.conv3x3_fwd(x, pk, circular=True)


def _iso_f32_pool(ops):
    g = _g(121)
    pk = ops.PackedConv(_n(g, (64, 16, 3, 3), 0.08).to(DEV), _n(g, (64,), 0.1).to(DEV))
    return _n(g, (3, 12, 99, 16)).to(DEV), lambda x: ops.conv3x3_fwd(x, pk, circular=False, pool=True)


def _iso_wino(ops):
    g = _g(122)
    pk = ops.PackedConv(_n(g, (128, 64, 3, 3), 0.04).to(DEV), _n(g, (128,), 0.1).to(DEV), wino=True)
    return _n(g, (3, 13, 72, 64)).to(DEV), lambda x: ops.conv3x3_fwd(x, pk, circular=True)


def _iso_first(ops, bf16=False):
    g = _g(123)
    pk = ops.PackedFirstConv(_n(g, (64, 3, 3, 3), 0.3).to(DEV), _n(g, (64,), 0.1).to(DEV), bf16=bf16)
    return _n(g, (3, 3, 13, 99)).to(DEV), lambda x: ops.conv3x3_first_fwd(x, pk, circular=True)


def _iso_first2(ops):
    g = _g(124)
    pf = ops.PackedFirstConv(_n(g, (64, 3, 3, 3), 0.3).to(DEV), _n(g, (64,), 0.1).to(DEV), bf16=True)
    p2 = ops.PackedConvBf16(_n(g, (64, 64, 3, 3), 0.05).to(DEV), _n(g, (64,), 0.1).to(DEV))
    return _n(g, (3, 3, 20, 70)).to(DEV), lambda x: ops.conv_first2_bf16(x, pf, p2, circular=True)


def _iso_bf16(ops):
    g = _g(125)
    pk = ops.PackedConvBf16(_n(g, (64, 16, 3, 3), 0.08).to(DEV), _n(g, (64,), 0.1).to(DEV))
    return _n(g, (3, 12, 99, 16)).bfloat16().to(DEV), lambda x: ops.conv3x3_bf16_fwd(x, pk, circular=True, pool=True)


def _iso_f16x3(ops):
    g = _g(126)
    pk = ops.PackedConvF16x3(_n(g, (136, 24, 3, 3), 0.07).to(DEV), _n(g, (136,), 0.1).to(DEV))
    # a NaN has no hi + lo split: poison the split tensor itself
    def run(x):
        y = ops.conv3x3_f16x3_fwd(x, pk, circular=False)
        ops.f16x3_overflowed(DEV)           # the poisoned images raise the range flag by right: leave it clear for the next test
        return y
    return ops.nchw_to_split_f16(_n(g, (3, 24, 9, 130)).to(DEV), 24), run


_iso_conv('conv3x3_fwd-3x4x12x24-200', _iso_f32)
_iso_conv('conv3x3_fwd-pool-3x12x99x16-64', _iso_f32_pool)
_iso_conv('conv3x3_fwd-wino-3x13x72x64-128', _iso_wino)
_iso_conv('conv3x3_first_fwd-3x3x13x99', _iso_first)
_iso_conv('conv3x3_first_fwd-bf16-3x3x13x99', lambda ops: _iso_first(ops, True))
_iso_conv('conv_first2_bf16-3x3x20x70', _iso_first2)
_iso_conv('conv3x3_bf16_fwd-3x12x99x16-64', _iso_bf16)
_iso_conv('conv3x3_f16x3_fwd-3x9x130x24-136', _iso_f16x3)
_iso_conv('rotate_nearest-3x2x37x53', lambda ops: (_n(_g(127), (3, 2, 37, 53)).to(DEV), lambda x: ops.rotate_nearest(x, [33.3, 90.0, 301.0])))
_iso_conv('polar_from_raw-3x3x37x53', lambda ops: (_img(128, (3, 3, 37, 53)).to(DEV),
                                                  lambda x: ops.polar_from_raw(x, mean=MEAN, std=STD, size=128, h_s=64, w_s=256)))


@isolation('resize_batched-3-images')
def _iso_resize_batched():
    ops = _ops()
    imgs = [_img(129, (3, 37, 53)).to(DEV), _img(130, (3, 20, 91)).to(DEV), _img(131, (3, 64, 40)).to(DEV)]

    def run(images):
        desc = torch.tensor([(t.data_ptr(), t.shape[1], t.shape[2], 0, t.shape[0]) for t in images], dtype=torch.int64).to(DEV)
        return ops.resize_batched(desc, 3, 3, (32, 99), mean=MEAN, std=STD)
    clean = run(imgs)
    dirty = run([t if i == 1 else torch.full_like(t, float('nan')) for i, t in enumerate(imgs)])
    return [(clean[1], dirty[1])]


def _iso_match(dft, masked):
    def fn():
        ops = _ops()
        Bo, Bs, o, s = 37, 5, 20, 3
        ov, su = [t.to(DEV) for t in _emb(Bo, Bs, 33, seed=132)]
        kw = {'shift_mask': _words(Bs, 9).to(DEV)} if masked else {}
        f = ops.match_fwd_dft if dft else ops.match_fwd
        ori, dist = f(ov, su, **kw)[:2]
        ori2, dist2 = f(_nan_but(ov, o), _nan_but(su, s), **kw)[:2]
        # pair (o, s) depends on gallery row o and query s only
        return [(dist[o, s], dist2[o, s]), (ori[o, s], ori2[o, s])]
    return fn


for _d in (False, True):
    for _m in (False, True):
        isolation('match_fwd%s%s-37x5-We33' % ('_dft' if _d else '', '-masked' if _m else ''))(_iso_match(_d, _m))


@pytest.mark.parametrize('entry', ISOLATION, ids=[e[0] for e in ISOLATION])
def test_batch_isolation(entry):
    """Every batch entry but one is NaN: the clean entry's output is finite and bit-identical to the launch with all entries clean
    (same batch size and grid, so the same kernel instantiation). Generalises
    tests/test_conv_gpu.py::test_first_layer_missing_planes_read_zeros_not_the_next_image."""
    _id, fn, _variant = entry
    pairs = fn()
    torch.cuda.synchronize()
    for clean, dirty in pairs:
        if clean.is_floating_point():
            assert bool(torch.isfinite(clean.float()).all())
            assert bool(torch.isfinite(dirty.float()).all()), 'a poisoned neighbour reaches the clean entry'
        assert _same_bits(clean, dirty), 'the clean entry changes with its neighbours: %d element(s)' % int((clean != dirty).sum())
