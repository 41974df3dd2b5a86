"""The Winograd F(2,3)-along-H form of conv3x3_nhwc_f32_kernel (witw_conv3x3_fwd_wino): parity with an fp64 oracle for every
converted class and workgroup shape, NW = 4 and 8 bitwise equal, the same instantiation names as the direct form, the switch,
and a training forward that keeps the direct form."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from witw_amd import ops
    return ops


def _ref(x_nhwc, w, b, circ, pool):
    """fp64 Conv2d(3x3, pad 1) [+ circular W padding] + ReLU [+ MaxPool2d(2)], NHWC out"""
    x = x_nhwc.double().permute(0, 3, 1, 2)
    if circ:
        x = torch.cat([x[..., -1:], x, x[..., :1]], dim=3)
        y = F.conv2d(F.pad(x, (0, 0, 1, 1)), w.double(), b.double())
    else:
        y = F.conv2d(x, w.double(), b.double(), padding=1)
    y = torch.relu(y)
    if pool:
        y = F.max_pool2d(y, 2)
    return y.permute(0, 2, 3, 1)


def _run(ops, x, pk, circ, pool, nw):
    old = os.environ.get('WITW_CONV_NW')
    os.environ['WITW_CONV_NW'] = str(nw)
    try:
        y = ops.conv3x3_fwd(x, pk, circular=circ, relu=True, pool=pool)
        torch.cuda.synchronize()
        return y, ops.last_kernel_variant(), ops.last_conv_form()
    finally:
        if old is None:
            del os.environ['WITW_CONV_NW']
        else:
            os.environ['WITW_CONV_NW'] = old


# (cin, cout, pool): the three converted classes <128,1,false>, <128,1,true>, <64,1,true>
CLASSES = [(64, 128, False), (128, 128, True), (64, 64, True)]


@pytest.mark.parametrize('cin,cout,pool', CLASSES)
@pytest.mark.parametrize('circ', [False, True])
@pytest.mark.parametrize('H,W', [(16, 64), (13, 72)])       # whole tiles; odd H and ragged W
def test_wino_matches_fp64_and_keeps_the_instantiation(cin, cout, pool, circ, H, W):
    ops = _ops()
    g = torch.Generator().manual_seed(cin * 7 + cout + H + W + int(pool) + 2 * int(circ))
    B = 2
    x = torch.relu(torch.randn(B, H, W, cin, generator=g)).cuda()
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).cuda()
    b = ((torch.rand(cout, generator=g) - 0.5) * 0.1).cuda()
    pk_d = ops.PackedConv(w, b)
    pk_w = ops.PackedConv(w, b, wino=True)
    ref = _ref(x, w, b, circ, pool)
    tn = 128 if cout >= 128 else 64
    outs = {}
    for nw in (4, 8):
        yd, vd, fd = _run(ops, x, pk_d, circ, pool, nw)
        yw, vw, fw = _run(ops, x, pk_w, circ, pool, nw)
        assert fd == 'direct' and fw == 'wino_h2'
        assert vw == vd == 'conv3x3_nhwc_f32_kernel<%d,1,%s,%d,0,9>' % (tn, 'true' if pool else 'false', nw)
        assert yw.shape == ref.shape
        scale = ref.abs().max().item()
        err = (yw.double() - ref).abs().max().item()
        assert err <= 3e-5 * scale, (nw, err, scale)
        outs[nw] = yw
    assert torch.equal(outs[4], outs[8]), 'NW = 4 and NW = 8 must compute every output with the same arithmetic'


def test_switch_and_ineligible_launches_take_the_direct_form():
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    x = torch.relu(torch.randn(1, 8, 64, 64, generator=g)).cuda()
    w = (torch.randn(128, 64, 3, 3, generator=g) * 0.06).cuda()
    b = torch.zeros(128).cuda()
    pk_d, pk_w = ops.PackedConv(w, b), ops.PackedConv(w, b, wino=True)
    y_d = ops.conv3x3_fwd(x, pk_d)
    assert ops.last_conv_form() == 'direct'
    prev = ops.conv_wino(False)
    try:
        assert prev is True or prev is False
        y_off = ops.conv3x3_fwd(x, pk_w)
        assert ops.last_conv_form() == 'direct'
        assert torch.equal(y_off, y_d), 'switched off, a Winograd-packed filter runs the direct form bit for bit'
    finally:
        ops.conv_wino(prev)
    ops.conv_wino(True)
    try:
        ops.conv3x3_fwd(x, pk_w)
        assert ops.last_conv_form() == 'wino_h2'
        ops.conv3x3_fwd(x, pk_w, stride_h=2)            # stride 2: direct
        assert ops.last_conv_form() == 'direct'
        gate = torch.ones(1, 8, 64, 128, device='cuda')
        ops.conv3x3_fwd(x, pk_w, gate=gate)             # gated (backward) launch: direct
        assert ops.last_conv_form() == 'direct'
        x32 = x[:, :, :32].contiguous()                 # narrow map: geometry 1, direct
        ops.conv3x3_fwd(x32, pk_w)
        assert ops.last_conv_form() == 'direct'
    finally:
        ops.conv_wino(prev)


def test_training_forward_is_direct_and_inference_is_winograd(monkeypatch):
    ops = _ops()
    from witw_amd import cvig_fov
    enc = cvig_fov.FOV_DSM(circ_padding=True).cuda()
    x = torch.rand(2, 3, 32, 128, generator=torch.Generator().manual_seed(3)).cuda()
    forms = []
    real = ops.conv3x3_fwd

    def spy(*a, **k):
        out = real(*a, **k)
        forms.append((ops.last_kernel_variant(), ops.last_conv_form()))
        return out

    monkeypatch.setattr(ops, 'conv3x3_fwd', spy)
    enc._run(x, {}, keep_from=0)
    assert forms and all(f == 'direct' for _, f in forms), forms
    forms.clear()
    enc._run(x, {}, keep_from=None)
    assert any(f == 'wino_h2' for _, f in forms), forms
    for v, f in forms:
        if f == 'wino_h2':
            assert ',1,' in v and v.endswith(',0,9>'), v
