"""cvig_baseline's bf16 TRAINING path (SurfaceEncoder(train_precision='bf16')) on the GPU against tests/baseline_bf16_train_ref.py
(float64, rounded where the product rounds: filter, block input, block output gradient).

    exact operands (ternary, every |sum| <= 8)   the plain-output conv at tap_base 1 and 0, the transposed pack, the bf16 space-to-depth,
                                                 the 4-tap weight gradient: the WHOLE output buffer bit for bit
    N(0,1) operands at K = 4 x 1024             |err| <= (K + S + 2) 2^-24 sum |x||w| per output, against float64 on the rounded operands
    memory contract                              every new wrapper between guard bands, the split-K workspace pre-filled with NaN
    encoder step                                 embedding, 28 gradients, running statistics, re-pack after Adam, reproducible bits
    surface                                      the knob trains, refuses what it must, train() runs two epochs"""
import functools
import os

import numpy as np
import pytest
import torch

from witw_amd import synth
from tests import baseline_bf16_ref as R0
from tests import baseline_bf16_train_ref as R
from tests.mem_arena import Arena, ArenaTorch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _bf16(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    assert torch.equal(t.to(torch.bfloat16).float(), t), 'not bf16 values'
    return t.to(torch.bfloat16).to(DEV)


def _same_bits_f32(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    w = R0.f32_bits(want + 0.)                    # + 0.: a float64 -0 of the reference is the kernel's +0
    g = np.ascontiguousarray(got + np.float32(0.)).view(np.uint32)
    bad = np.argwhere(g != w)
    assert not len(bad), '%s: %d of %d elements differ, first at %s: got %r want %r' % (
        what, len(bad), g.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _ternary_filter(r, cout, cin, nz):
    """[cout][cin][2][2] with nz entries of +-1 per output channel"""
    live = np.zeros((cout, cin * 4))
    for n in range(cout):
        idx = r.choice(cin * 4, size=min(nz, cin * 4), replace=False)
        live[n, idx] = r.choice([-1., 1.], size=len(idx))
    return live.reshape(cout, cin, 2, 2)


SHAPES = [(2, 2), (9, 33), (17, 40)]          # the 8 x 32 tile: below it, one row and one column past it, several tiles


# ----------------------------------------------------------------------------- the plain-output convolution
@pytest.mark.parametrize('cin', [16, 48])
@pytest.mark.parametrize('tap_base', [1, 0])
def test_plain_conv_exact(tap_base, cin):
    """witw_conv3x3_bf16_fwd_taps4_plain: forward (tap_base 1: bias + LeakyReLU(0.5)) and data gradient (tap_base 0, transpose_flip
    filter: neither) over Cout 8 / 12 / 136, three map sizes, B 1 / 3, valid region equal to and below the map"""
    from witw_amd import baseline_bf16 as bb
    r = np.random.RandomState(100 * tap_base + cin)
    for cout in (8, 12, 136):
        for (H, W) in SHAPES:
            for B in (1, 3):
                x = r.randint(-1, 2, size=(B, H, W, cin)).astype(np.float64)
                k3 = r.randint(-1, 2, size=(cout, cin, 3, 3)).astype(np.float64) if tap_base else \
                    r.randint(-1, 2, size=(cin, cout, 3, 3)).astype(np.float64)          # the dead taps must not matter
                if tap_base:
                    k3[:, :, 1:3, 1:3] = _ternary_filter(r, cout, cin, 6)
                    bias = r.randint(-2, 3, size=cout).astype(np.float64)
                    w4 = R.fwd_filter(k3)
                    pk = bb.PackedConvBf16Taps4(_f32(k3), _f32(bias))
                else:
                    # source [cin][cout][3][3]: its taps {1,2}^2, rotated, are the packed taps {0,1}^2 of (cout, cin)
                    k3[:, :, 1:3, 1:3] = _ternary_filter(r, cout, cin, 8).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]
                    bias = None
                    w4 = R.dgrad_filter(k3)
                    pk = bb.PackedConvBf16Taps4(_f32(k3), None, transpose_flip=True)
                    assert (np.abs(w4).sum((1, 2, 3)) <= 8).all() and pk.cout == cout and pk.cin == cin
                for valid in ((H, W), (max(1, H - 1), max(1, W - 2))):
                    slope = 0.5 if tap_base else None
                    got = bb.conv_taps4_plain_bf16(_bf16(x), pk, valid, lrelu_slope=slope)
                    want = R.conv_plain(x, w4, bias, tap_base, valid, slope)
                    _same_bits_f32(got, want, 'tap_base %d cin %d cout %d %dx%d B %d valid %s' % (tap_base, cin, cout, H, W, B, valid))


@pytest.mark.parametrize('cout,cin', [(8, 16), (12, 48), (136, 16)])
def test_transposed_pack_equals_the_fp32_pack_rounded(cout, cin):
    """witw_conv3x3_bf16_pack_weights_taps4_ex(transpose_flip=1) read back through convolutions of one-hot inputs, against the fp32
    witw_conv3x3_pack_weights_taps4(transpose_flip=1) image read back the same way and rounded element by element"""
    from witw_amd import baseline_bf16 as bb
    from witw_amd import ops
    r = np.random.RandomState(7)
    src = r.normal(0., 1., (cin, cout, 3, 3)).astype(np.float32)        # source [cin][cout][3][3] -> packed (cout, cin)
    pk16 = bb.PackedConvBf16Taps4(_f32(src), None, transpose_flip=True)
    pk32 = ops.PackedConv(_f32(src), None, transpose_flip=True, taps4=True)
    # input channel ci hot at pixel (1,1) of image ci: out[ci, 1-ty+.., ..] reads tap (ty, tx) at output pixel (2-ty, 2-tx) - (1,1) + ...
    x = np.zeros((cin, 3, 3, pk32.cin_pad))
    x16 = np.zeros((cin, 3, 3, pk16.cin_pad))
    for ci in range(cin):
        x[ci, 1, 1, ci] = x16[ci, 1, 1, ci] = 1.
    y32 = ops.conv3x3_fwd(_f32(x), pk32, relu=False).cpu().numpy().astype(np.float64)      # [cin,3,3,cout]: products with 1 and 0 only
    y16 = bb.conv_taps4_plain_bf16(_bf16(x16), pk16)
    _same_bits_f32(y16, R0.bf16_round(y32), 'pack (%d,%d)' % (cout, cin))
    want = R.conv_plain(x16[..., :cin], R.dgrad_filter(src), None, 0)
    _same_bits_f32(y16, want, 'pack vs float64 (%d,%d)' % (cout, cin))
    assert np.count_nonzero(want) == 4 * cin * cout


# ----------------------------------------------------------------------------- bf16 space-to-depth, cast
@pytest.mark.parametrize('C', [8, 12])
@pytest.mark.parametrize('valid', [(7, 9), (6, 10), (8, 11)])
def test_space_to_depth_bf16_exact(C, valid):
    """values k/8, scale a power of two, integer shift: every value a bf16 number; the shift is non-zero everywhere, so a mask that let
    the affine out of the valid region would show"""
    from witw_amd import baseline_bf16 as bb
    r = np.random.RandomState(C)
    a = r.randint(-16, 17, size=(3, 8, 11, C)) / 8.
    scale = r.choice([0.5, 1., 2.], size=C) * r.choice([-1., 1.], size=C)
    shift = r.choice([-3., -1., 1., 2.], size=C)
    got = bb.space_to_depth2_bf16(_f32(a), valid, _f32(scale), _f32(shift))
    want = R.space_to_depth2(a, valid, scale, shift)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == want.shape
    assert np.array_equal(got.view(torch.int16).cpu().numpy().view(np.uint16), R0.bf16_bits(want + 0.))
    got = bb.space_to_depth2_bf16(_f32(a), valid)
    assert np.array_equal(got.view(torch.int16).cpu().numpy().view(np.uint16), R0.bf16_bits(R.space_to_depth2(a, valid) + 0.))


def test_space_to_depth_bf16_and_cast_round_to_nearest_even():
    from witw_amd import baseline_bf16 as bb
    f = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 - 2.0 ** -16, 1 + 2.0 ** -8 + 2.0 ** -16, 1 + 3 * 2.0 ** -8 - 2.0 ** -16,
                  1 + 3 * 2.0 ** -8 + 2.0 ** -16, -1 - 2.0 ** -8, -1 - 3 * 2.0 ** -8])
    a = np.resize(f, (2, 5, 7, 8)) * np.resize(np.array([1., 2., 0.5, 4., 3.]), (2, 5, 7, 8))
    got = bb.space_to_depth2_bf16(_f32(a), (5, 7))
    assert np.array_equal(got.view(torch.int16).cpu().numpy().view(np.uint16), R0.bf16_bits(R.space_to_depth2(a, (5, 7))))
    flat = np.resize(a.reshape(-1), 4 * 67 + 3)           # a tail that is no multiple of four
    got = bb.to_bf16(_f32(flat))
    assert np.array_equal(got.view(torch.int16).cpu().numpy().view(np.uint16), R0.bf16_bits(R0.bf16_round(flat)))


# ----------------------------------------------------------------------------- the weight gradient
def _wgrad_case(r, B, H, W, cin, cout):
    h = r.randint(-1, 2, size=(B, H, W, cin)).astype(np.float64)
    dz = np.zeros((B, H, W, cout))
    for n in range(cout):                       # at most 8 non-zero pixels per channel: every sum has at most 8 terms
        k = min(8, B * H * W)
        idx = r.choice(B * H * W, size=k, replace=False)
        idx[0] = B * H * W - 1                  # the last pixel of the last image: its window leaves the map
        dz.reshape(-1, cout)[idx, n] = r.choice([-1., 1.], size=k)
    return h, dz


def _splits(lib, B, H, W, cin, cout):
    return lib.witw_conv3x3_wgrad_bf16_taps4_workspace_floats(B, H, W, cin, cout) // (9 * cin * cout + cout)


@pytest.mark.parametrize('cin', [16, 48])
@pytest.mark.parametrize('cout', [8, 12, 136])
def test_wgrad_taps4_exact(cin, cout):
    """witw_conv3x3_wgrad_bf16_taps4 over B = 1 / 3 and the three map sizes, accumulate 0 (the five dead taps come back +0) and 1 (they
    and everything else keep what they held)"""
    from witw_amd import baseline_bf16 as bb
    r = np.random.RandomState(cin + cout)
    for (B, H, W) in [(3, 2, 2), (1, 9, 33), (3, 9, 33), (3, 17, 40)]:
        h, dz = _wgrad_case(r, B, H, W, cin, cout)
        dk3, db = R.wgrad_taps4(h, dz)
        what = 'cin %d cout %d B %d %dx%d' % (cin, cout, B, H, W)
        dw_g, db_g = bb.conv3x3_wgrad_bf16_taps4(_bf16(h), _bf16(dz), cin)
        _same_bits_f32(dw_g, dk3, what + ' dw')
        _same_bits_f32(db_g, db, what + ' db')
        dw0 = r.randint(-2, 3, size=dk3.shape).astype(np.float64)
        db0 = r.randint(-2, 3, size=db.shape).astype(np.float64)
        out = (_f32(dw0), _f32(db0))
        bb.conv3x3_wgrad_bf16_taps4(_bf16(h), _bf16(dz), cin, out=out, accumulate=True)
        _same_bits_f32(out[0], dw0 + dk3, what + ' dw accumulate')
        _same_bits_f32(out[1], db0 + db, what + ' db accumulate')


@pytest.mark.parametrize('cin,cout,shape,full', [
    (16, 8, (3, 40, 272), True),        # 3 x 5 x 17 = 255 K chunks of 8 rows x 16 columns: one split each
    (16, 8, (2, 64, 256), True),        # 256: the last count with one chunk per split
    (16, 8, (3, 16, 688), False),       # 258: two chunks per split, the splits behind the 129th are empty and write zero partials
    (16, 136, (3, 8, 672), True),       # two channel tiles halve the splits: 126 chunks ...
    (16, 136, (3, 8, 688), False),      # ... and 129
])
def test_wgrad_taps4_exact_across_the_split_boundaries(cin, cout, shape, full):
    from witw_amd import _lib
    from witw_amd import baseline_bf16 as bb
    B, H, W = shape
    chunks = B * ((H + 7) // 8) * ((W + 15) // 16)
    S = _splits(_lib.load(), B, H, W, cin, cout)
    assert (S == chunks) if full else (1 <= S < chunks), (S, chunks)
    r = np.random.RandomState(H + W)
    h, dz = _wgrad_case(r, B, H, W, cin, cout)
    dk3, db = R.wgrad_taps4(h, dz)
    for acc in (0, 1):
        dw0 = r.randint(-2, 3, size=dk3.shape).astype(np.float64) * acc
        db0 = r.randint(-2, 3, size=db.shape).astype(np.float64) * acc
        out = (_f32(dw0 + 0.25 * (1 - acc)), _f32(db0 + 0.25 * (1 - acc)))      # accumulate 0 overwrites whatever was there
        bb.conv3x3_wgrad_bf16_taps4(_bf16(h), _bf16(dz), cin, out=out, accumulate=bool(acc))
        _same_bits_f32(out[0], dw0 + dk3, 'dw %s accumulate %d' % (shape, acc))
        _same_bits_f32(out[1], db0 + db, 'db %s accumulate %d' % (shape, acc))


def test_wgrad_taps4_equals_the_nine_tap_entry_at_the_live_taps():
    """the 9-tap NHWC entry (zero padding, stride 1) holds the same sums at taps {1,2}^2: exact operands, so bit for bit"""
    from witw_amd import baseline_bf16 as bb
    from witw_amd import ops
    r = np.random.RandomState(5)
    h, dz = _wgrad_case(r, 3, 17, 40, 48, 136)
    dw4, db4 = bb.conv3x3_wgrad_bf16_taps4(_bf16(h), _bf16(dz), 48)
    dw9, db9 = ops.conv3x3_wgrad_bf16(_bf16(h), _bf16(dz), 48)
    assert torch.equal(dw4[:, :, 1:, 1:], dw9[:, :, 1:, 1:]) and torch.equal(db4, db9)
    assert not dw4[:, :, 0, :].any() and not dw4[:, :, :, 0].any()


# ----------------------------------------------------------------------------- N(0,1) operands: the derived accumulation bound
def test_plain_conv_normal_operands_within_the_fp32_sum_bound():
    """K = 4 x 1024 products per output, float64 on the ROUNDED operands: only the accumulation differs. A length-K fp32 sum in any
    order is within gamma_K sum |x_i||w_i|; (K + S + 2) 2^-24 with S = 1 slice covers it and the bias addition."""
    from witw_amd import baseline_bf16 as bb
    r = np.random.RandomState(21)
    for tap_base in (1, 0):
        cin, cout, B, H, W = 1024, 24, 1, 9, 33
        x = R0.bf16_round(r.normal(0., 1., (B, H, W, cin)))
        k3 = r.normal(0., 1., (cout, cin, 3, 3) if tap_base else (cin, cout, 3, 3))
        w4 = R.fwd_filter(k3) if tap_base else R.dgrad_filter(k3)
        bias = r.normal(0., 1., cout).astype(np.float32).astype(np.float64) if tap_base else None
        pk = bb.PackedConvBf16Taps4(_f32(k3), _f32(bias) if tap_base else None, transpose_flip=not tap_base)
        got = bb.conv_taps4_plain_bf16(_bf16(x), pk).cpu().numpy().astype(np.float64)
        want = R.conv_plain(x, w4, bias, tap_base)
        l1 = R.conv_plain(np.abs(x), np.abs(w4), None if bias is None else np.abs(bias), tap_base)
        bound = (4 * cin + 1 + 2) * 2.0 ** -24 * l1
        err = np.abs(got - want)
        print('plain conv tap_base %d: worst err / bound = %.3f' % (tap_base, float((err / bound).max())))
        assert (err <= bound).all()


def test_wgrad_normal_operands_within_the_fp32_sum_bound():
    """K = 4096 pixels per weight, S splits and their serial reduction: |err| <= (K + S + 2) 2^-24 sum |dz||h|"""
    from witw_amd import _lib
    from witw_amd import baseline_bf16 as bb
    r = np.random.RandomState(22)
    B, H, W, cin, cout = 1, 64, 64, 48, 24
    h = R0.bf16_round(r.normal(0., 1., (B, H, W, cin)))
    dz = R0.bf16_round(r.normal(0., 1., (B, H, W, cout)))
    S = _splits(_lib.load(), B, H, W, cin, cout)
    dw, db = bb.conv3x3_wgrad_bf16_taps4(_bf16(h), _bf16(dz), cin)
    want_w, want_b = R.wgrad_taps4(h, dz)
    l1_w, l1_b = R.wgrad_taps4(np.abs(h), np.abs(dz))
    K = B * H * W
    c = (K + S + 2) * 2.0 ** -24
    err_w = np.abs(dw.cpu().numpy().astype(np.float64) - want_w)
    err_b = np.abs(db.cpu().numpy().astype(np.float64) - want_b)
    live = np.zeros(want_w.shape, dtype=bool)
    live[:, :, 1:, 1:] = True
    print('wgrad: S = %d, worst err / bound = %.3f (dw) %.3f (db)' % (S, float((err_w[live] / (c * l1_w[live])).max()),
                                                                   float((err_b / (c * l1_b)).max())))
    assert (err_w <= c * l1_w).all() and (err_b <= c * l1_b).all()          # the dead taps: 0 <= 0


# ----------------------------------------------------------------------------- memory contract
@pytest.mark.parametrize('skew', [0, 16])
@pytest.mark.parametrize('shape', [(3, 9, 33, 48, 136), (1, 17, 40, 16, 12), (3, 2, 2, 16, 8)])
def test_memory_contract_of_the_training_wrappers(shape, skew, monkeypatch):
    """Both packings, conv_taps4_plain_bf16 at both tap bases, space_to_depth2_bf16, to_bf16 and conv3x3_wgrad_bf16_taps4 between guard
    bands: inputs inside NaN bands, every device allocation of a wrapper (the split-K workspace included) inside bands with a NaN
    canary payload. No band is touched, every output element is stored, the inputs are unchanged, the values are those of ordinary
    allocations bit for bit."""
    from witw_amd import baseline_bf16 as bb
    from witw_amd import ops
    B, H, W, cin, cout = shape
    r = np.random.RandomState(3)
    h, dz = _wgrad_case(r, B, H, W, cin, cout)
    a = r.randint(-16, 17, size=(B, 2 * H - 1, 2 * W, cin // 4)) / 8.
    inputs = dict(h=_bf16(h), dz=_bf16(dz), dzf=_f32(dz), k3=_f32(r.randint(-1, 2, size=(cout, cin, 3, 3))), bias=_f32(r.randint(-2, 3, size=cout)),
                  k3t=_f32(r.randint(-1, 2, size=(cin, cout, 3, 3))),      # source [cin][cout][3][3]: its data-gradient filter reads cin channels
                  a=_f32(a), scale=_f32(np.full(cin // 4, 2.)), shift=_f32(np.full(cin // 4, 1.)))

    def call(p):
        pk = bb.PackedConvBf16Taps4(p['k3'], p['bias'])
        pk_t = bb.PackedConvBf16Taps4(p['k3t'], None, transpose_flip=True)
        y = bb.conv_taps4_plain_bf16(p['h'], pk, (max(1, H - 1), W), lrelu_slope=0.5)
        dx = bb.conv_taps4_plain_bf16(p['h'], pk_t)
        s = bb.space_to_depth2_bf16(p['a'], (2 * H - 1, 2 * W - 1), p['scale'], p['shift'])
        c = bb.to_bf16(p['dzf'])
        dw, db = bb.conv3x3_wgrad_bf16_taps4(p['h'], p['dz'], cin)
        return pk.wpk, pk_t.wpk, y, dx, s, c, dw, db
    plain = [t.clone() for t in call(inputs)]
    arena = Arena(DEV, skew_bytes=skew)
    with monkeypatch.context() as m:
        m.setattr(bb, 'torch', ArenaTorch(arena))
        m.setattr(ops, 'torch', ArenaTorch(arena))
        placed = {k: arena.place(t, k) for k, t in inputs.items()}
        got = call(placed)
    arena.check(got)
    for g, q in zip(got, plain):
        assert torch.equal(g.view(torch.uint8), q.view(torch.uint8))
    for k, t in inputs.items():
        assert torch.equal(placed[k].view(torch.uint8), t.view(torch.uint8)), k


# ----------------------------------------------------------------------------- encoder step
# Bar of a gradient, relative to its norm. The bar tests/test_baseline_gpu.py holds the fp32 step to against its float64 reference is
# 1e-4, and the mirrored reference rounds where the product rounds. It does not leave fp32 accumulation order alone, though: a value an
# fp32 computation places on the other side of a bf16 tie than float64 does is rounded to the OTHER neighbour, one bf16 ulp away, and at
# the project's smallest legal inputs with B = 2 block 7 has ONE valid output per image, so bn7 normalises two samples per channel:
# its output is +-d / sqrt(d^2 + 4 eps), d = a1 - a2, whose derivative in d is unbounded relative to the value where |d| ~ sqrt(eps).
# The float64 step itself moves by as much when every value gets fp32-sized noise (1.2e-7 relative) in front of its rounding
# (encoder_step(jitter=...), measured on the CPU at 382 x 382: embedding columns of block 5 / 6 / 7 by 5.7e-5 / 2.1e-4 / 1.0e-2, the
# gradients of blocks 1-6 by 0.18-0.23 of their norm, conv7.bias 6.7e-2, bn7.weight 6.3e-3, bn6.bias 5.0e-4, bn7.bias 7.4e-5).
# Measured on the GPU against the mirrored step, 382 x 382 / 383 x 397, relative to the gradient's norm:
#   bn7.bias 1.22e-4 / 1.19e-4, bn6.bias 2.87e-4 / 1.80e-4, bn7.weight 1.40e-2 / 4.48e-3, conv7.bias 3.12e-2 / 3.47e-2,
#   every other gradient 2.31e-1 ... 3.01e-1 (worst: conv1.bias) / 2.21e-1 ... 2.52e-1 (worst: bn3.weight).
# Each bar is twice the worst of the two shapes. What these bars can still tell is a wrong sign, layout or scale of a gradient (a
# distance of 1 or more); the arithmetic itself is held bit for bit by the exact tests above.
GRAD_BAR = {'bn7.bias': 2.5e-4, 'bn6.bias': 5.8e-4, 'bn7.weight': 2.8e-2, 'conv7.bias': 7.0e-2}
GRAD_BAR_OTHER = 6.1e-1
# The embedding, per block of 512 columns (blocks 5, 6, 7): 1e-4 (the fp32 step's bar) + 4 x the float64 step's own movement under that
# jitter, computed in the test: the GPU has such noise at every operation, not only in front of the roundings, and two noise
# realisations lie further apart than one lies from the plain step.
EMBED_ATOL = 1e-4
EMBED_SPREADS = 4.
JITTER = (1.2e-7, 1)
STEP_SHAPES = {'382': (2, 3, 382, 382), '383x397': (2, 3, 383, 397)}


def _load(enc, params):
    with torch.no_grad():
        for i, q in enumerate(params, 1):
            getattr(enc, 'conv%d' % i).weight.copy_(torch.from_numpy(q['w']))
            getattr(enc, 'conv%d' % i).bias.copy_(torch.from_numpy(q['b']))
            bn = getattr(enc, 'bn%d' % i)
            bn.weight.copy_(torch.from_numpy(q['gamma']))
            bn.bias.copy_(torch.from_numpy(q['beta']))
            bn.running_mean.copy_(torch.from_numpy(q['mean']))
            bn.running_var.copy_(torch.from_numpy(q['var']))
    return enc.to(DEV).train()


@functools.lru_cache(maxsize=None)
def _step_inputs(tag):
    shape = STEP_SHAPES[tag]
    params = R0.make_params(31)
    x = synth.images_u8(17, 3, shape)
    df = np.random.RandomState(5).normal(0., 1., (shape[0], 1536)).astype(np.float32)
    return params, x, df


@functools.lru_cache(maxsize=None)
def _reference_step(tag):
    """computed once per shape and shared; never modified"""
    params, x, df = _step_inputs(tag)
    return R.encoder_step(x, params, df)


def _gate_band(enc, i, z_std):
    """How far from zero a conv output of block i may lie and still fall on the other side on the GPU. fp32 accumulation moves it by
    1e-4 x max(1, std) at the most (the band tests/test_baseline_gpu.py uses). From block 3 on the input h_i is a ROUNDED value of an fp32
    affine whose statistics differ from the float64 ones in their last bits: where the two fall on different sides of a bf16 tie, h_i
    differs by one bf16 ulp, 2^-7 |h| at the most, and the output by that times the weight it meets; up to 8 such inputs in one window
    are allowed for (a window has 4 x Cin >= 512 of them, a flip needs the fp32 value within ~1e-6 of a tie)."""
    band = 1e-4 * max(1., z_std)
    if 3 <= i <= 4:
        h = enc._last_saved[i - 1][0]
        band += 8 * 2.0 ** -7 * float(h.float().abs().max()) * float(getattr(enc, 'conv%d' % i).weight.detach().abs().max())
    if i > 4:       # behind the bf16 blocks the same differences arrive through fp32 layers: bounded by block 4's band, amplified by a BatchNorm
        band = 1e-2 * max(1., z_std)
    return band


@functools.lru_cache(maxsize=None)
def _reference_spread(tag):
    """the float64 step's own movement under JITTER: (max |embedding difference| per block of 512 columns, per block i the max
    difference of the batch mean and of the batch variance)"""
    params, x, df = _step_inputs(tag)
    f_j, _g, _pre, stats_j = R.encoder_step(x, params, df, jitter=JITTER)
    f_0, _g, _pre, stats_0 = _reference_step(tag)
    d = np.abs(f_j - f_0)
    return ([float(d[:, 512 * k:512 * (k + 1)].max()) for k in range(3)],
            [(float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max())) for a, b in zip(stats_j, stats_0)])


def _gpu_step(tag, gates_from=None):
    """-> (encoder, embedding, flips): one forward / backward; gates_from = the reference's conv outputs: the backward takes the
    reference's side of every LeakyReLU gate, which may differ only where the conv output is within rounding of zero"""
    from witw_amd import cvig_baseline as cb
    params, x, df = _step_inputs(tag)
    enc = _load(cb.SurfaceEncoder(train_precision='bf16'), params)
    enc.keep_activations = True
    acts = {}
    f = enc(torch.from_numpy(x).to(DEV), lrelu_acts=acts)
    flips = 0
    if gates_from is not None:
        for i in range(1, 8):
            _h, a, (vh, vw), *_rest = enc._last_saved[i - 1]
            z = torch.from_numpy(gates_from[i - 1]).permute(0, 2, 3, 1).to(DEV)          # [B,vh,vw,co] float64
            differ = (a[:, :vh, :vw] > 0) != (z > 0)
            n = int(differ.sum())
            if n:
                assert float(z[differ].abs().max()) < _gate_band(enc, i, float(z.std())), 'block %d: a gate differs away from zero' % i
                want = torch.zeros(a.shape, dtype=torch.bool, device=DEV)
                want[:, :vh, :vw] = z > 0
                inside = torch.zeros_like(want)
                inside[:, :vh, :vw] = True
                mag = a.abs()
                acts[i] = torch.where(inside & (want != (a > 0)), torch.where(want, mag + 1e-30, -mag), a).contiguous()
                flips += n
    f.backward(torch.from_numpy(df).to(DEV))
    return enc, f.detach(), flips


@pytest.mark.parametrize('tag', sorted(STEP_SHAPES))
def test_encoder_step_against_the_rounding_mirrored_float64_step(tag):
    """SurfaceEncoder(train_precision='bf16').train() at the project's smallest inputs, B = 2: embedding, the 28 gradients, the running
    statistics; then Adam and a second forward: the bf16 filters are re-packed from the new master weights."""
    from witw_amd import cvig_fov
    params, x, df = _step_inputs(tag)
    f_ref, g_ref, pre, stats = _reference_step(tag)
    enc, f, flips = _gpu_step(tag, gates_from=pre)
    print('%s: %d LeakyReLU gates within rounding of zero taken from the reference' % (tag, flips))
    # a gate can differ only where the conv output lies inside _gate_band of zero: for most outputs that band is 1e-4 of a value of unit
    # scale whose density at zero is ~0.4: 4e-5 of the gates could, and only those whose two computations actually straddle zero do
    n_gates = sum(int(np.prod(z.shape)) for z in pre)
    assert flips <= 1e-4 * n_gates, (flips, n_gates)
    for i in (2, 3, 4):
        assert enc._last_saved[i - 1][0].dtype == torch.bfloat16 and enc._last_saved[i - 1][1].dtype == torch.float32
    assert enc._last_saved[0][0].dtype == torch.float32 and enc._last_saved[4][0].dtype == torch.float32
    err = np.abs(f.cpu().numpy() - f_ref)
    err = [float(err[:, 512 * k:512 * (k + 1)].max()) for k in range(3)]
    bars = [EMBED_ATOL + EMBED_SPREADS * s for s in _reference_spread(tag)[0]]
    print('%s: embedding max |err| per block 5 / 6 / 7: %s, bars %s' % (tag, ['%.2e' % e for e in err], ['%.2e' % b for b in bars]))
    worst = {}
    for i in range(1, 8):
        conv, bn = getattr(enc, 'conv%d' % i), getattr(enc, 'bn%d' % i)
        for name, p, ref in (('conv%d.weight' % i, conv.weight, g_ref[i - 1]['dw']), ('conv%d.bias' % i, conv.bias, g_ref[i - 1]['db']),
                             ('bn%d.weight' % i, bn.weight, g_ref[i - 1]['dgamma']), ('bn%d.bias' % i, bn.bias, g_ref[i - 1]['dbeta'])):
            got = p.grad.detach().cpu().numpy().astype(np.float64)
            worst[name] = float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-300))
    for name in sorted(worst, key=worst.get, reverse=True):
        print('%s: %s deviates by %.2e of its norm' % (tag, name, worst[name]))
    assert all(e <= b for e, b in zip(err, bars)), (err, bars)
    over = {k: v for k, v in worst.items() if v > GRAD_BAR.get(k, GRAD_BAR_OTHER)}
    assert not over, over
    # running statistics and the batch counter advance as in the fp32 step: momentum 0.1, unbiased variance. Tolerance: the fp32 step's
    # (rtol 1e-4, atol 1e-6) + the momentum's share of 4 x the float64 step's own movement of that batch statistic (see EMBED_SPREADS)
    stat_spread = _reference_spread(tag)[1]
    vh, vw = x.shape[2], x.shape[3]
    for i, q in enumerate(params, 1):
        bn = getattr(enc, 'bn%d' % i)
        vh, vw = (vh - 4) // 2 + 1, (vw - 4) // 2 + 1
        n = x.shape[0] * vh * vw
        mean, var = stats[i - 1]
        assert int(bn.num_batches_tracked) == 1
        unb = n / max(1, n - 1)
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), 0.9 * q['mean'] + 0.1 * mean, rtol=1e-4,
                                   atol=1e-6 + 0.1 * EMBED_SPREADS * stat_spread[i - 1][0])
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), 0.9 * q['var'] + 0.1 * var * unb, rtol=1e-4,
                                   atol=1e-6 + 0.1 * EMBED_SPREADS * stat_spread[i - 1][1] * unb)
    # a second step behind Adam: the version key re-packs the bf16 filters
    before = {i: (enc._packed[('bf16', i)][0], enc._packed[('bf16', i)][1].wpk.clone(), enc._packed[('bf16_t', i)][1].wpk.clone()) for i in (2, 3, 4)}
    opt = cvig_fov.Adam(list(enc.parameters()), lr=1e-3)
    opt.step()
    f2 = enc(torch.from_numpy(x).to(DEV))
    f2.backward(torch.from_numpy(df).to(DEV))
    for i in (2, 3, 4):
        assert enc._packed[('bf16', i)][0] != before[i][0]
        assert not torch.equal(enc._packed[('bf16', i)][1].wpk.view(torch.int16), before[i][1].view(torch.int16))
        assert not torch.equal(enc._packed[('bf16_t', i)][1].wpk.view(torch.int16), before[i][2].view(torch.int16))
        k3 = enc._layer_k3(i, pack=False)
        fresh = __import__('witw_amd.baseline_bf16', fromlist=['x']).PackedConvBf16Taps4(k3, getattr(enc, 'conv%d' % i).bias)
        assert torch.equal(enc._packed[('bf16', i)][1].wpk.view(torch.int16), fresh.wpk.view(torch.int16))
    assert not torch.equal(f2.detach(), f)
    assert int(enc.bn1.num_batches_tracked) == 2


def test_two_identical_steps_give_identical_bits():
    enc_a, f_a, _ = _gpu_step('382')
    enc_b, f_b, _ = _gpu_step('382')
    assert torch.equal(f_a.view(torch.int32), f_b.view(torch.int32))
    for pa, pb in zip(enc_a.parameters(), enc_b.parameters()):
        assert torch.equal(pa.grad.view(torch.int32), pb.grad.view(torch.int32))
    for ba, bb_ in zip(enc_a.buffers(), enc_b.buffers()):
        assert torch.equal(ba, bb_)


# ----------------------------------------------------------------------------- surface
def test_train_precision_knob_trains_and_leaves_the_default_alone():
    from witw_amd import _lib
    from witw_amd import cvig_baseline as cb
    params, x, df = _step_inputs('382')
    xg = torch.from_numpy(x).to(DEV)
    enc16 = _load(cb.SurfaceEncoder(train_precision='bf16'), params)
    enc32 = _load(cb.SurfaceEncoder(), params)
    assert enc32.train_precision == 'fp32' and enc16.precision == 'fp32'
    f16, f32 = enc16(xg), enc32(xg)
    f16.backward(torch.from_numpy(df).to(DEV))
    f32.backward(torch.from_numpy(df).to(DEV))
    assert not torch.equal(f16.detach(), f32.detach())                      # another arithmetic ...
    # ... of the same function. The distance to the fp32 step is recorded, not held to a bar: this only tells the same
    # function from another one (unrelated vectors of one norm lie sqrt(2) of it apart)
    d = float((f16.detach() - f32.detach()).norm() / f32.detach().norm())
    print('embedding: bf16 training forward %.2e of the norm from the fp32 one' % d)
    assert d < 0.5
    for (name, p16), p32 in zip(enc16.named_parameters(), enc32.parameters()):
        assert p16.grad is not None and bool(torch.isfinite(p16.grad).all()) and p16.grad.dtype == torch.float32
        print('%s: bf16 gradient %.2e of the norm from the fp32 one' % (name, float((p16.grad - p32.grad).norm() / p32.grad.norm())))
    assert ('bf16', 2) not in enc32._packed and enc16._packed[2][1] is None      # no filter image of the other arithmetic is packed
    # the eval forward of a bf16-trained encoder is `precision`'s: fp32 here, bit for bit the fp32 encoder's on the same state
    enc16.load_state_dict(enc32.state_dict())
    with torch.no_grad():
        assert torch.equal(enc16.eval()(xg), enc32.eval()(xg))
    with pytest.raises(_lib.WitwError):
        _load(cb.SurfaceEncoder(bands=4, orientation=True, train_precision='bf16'),
              R0.make_params(31, inputs=6))(torch.zeros((2, 6, 382, 382), device=DEV))
    both = _load(cb.OverheadEncoder(precision='bf16', train_precision='bf16'), params)      # what train(train_precision='bf16') builds
    assert bool(torch.isfinite(both(xg)).all())
    with torch.no_grad():
        assert bool(torch.isfinite(both.eval()(xg)).all())


def test_train_driver_runs_two_epochs_in_bf16(tmp_path, monkeypatch, capsys):
    """train(train_precision='bf16') on a synthetic set, in the style of tests/test_drivers_gpu.py: two epochs, bf16 training steps,
    the validation phase on the bf16 eval forward, fp32 checkpoints in the usual format"""
    from PIL import Image
    from witw_amd import cvig_baseline as cb
    n = 6
    rows = []
    for i in range(n):
        for kind, hw in (('overhead', (400, 400)), ('surface', (200, 800))):
            arr = synth.images_u8(3, 10 * i + (kind == 'surface'), (3,) + hw).transpose(1, 2, 0)
            Image.fromarray(np.ascontiguousarray(arr).astype(np.uint8)).save(str(tmp_path / ('%s%d.png' % (kind, i))))
        rows.append('%s,%s' % (tmp_path / ('overhead%d.png' % i), tmp_path / ('surface%d.png' % i)))
    csv = tmp_path / 'train.csv'
    csv.write_text('\n'.join(rows) + '\n')
    monkeypatch.chdir(tmp_path)
    seen = []
    real = cb.SurfaceEncoder.forward

    def spy(self, x, lrelu_acts=None):
        seen.append((self.training, self.precision, self.train_precision))
        return real(self, x, lrelu_acts)
    monkeypatch.setattr(cb.SurfaceEncoder, 'forward', spy)
    best = cb.train(dataset='cvusa', val_quantity=2, batch_size=2, num_workers=0, num_epochs=2, csv_path=str(csv), train_precision='bf16')
    assert best is not None and np.isfinite(best)
    assert (True, 'bf16', 'bf16') in seen and (False, 'bf16', 'bf16') in seen and all(s[1:] == ('bf16', 'bf16') for s in seen)
    sd = torch.load(str(tmp_path / 'weights' / 'surface_best.pth'), map_location='cpu')
    assert sorted(sd) == sorted(cb.SurfaceEncoder().state_dict()) and all(v.dtype in (torch.float32, torch.int64) for v in sd.values())
    assert 'new best' in capsys.readouterr().out
