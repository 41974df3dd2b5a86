"""Tile runs of the Winograd form of conv3x3_nhwc_f32_kernel (witw_conv3x3_wino_run): a launch starts at most one workgroup per CU
and each walks a run of tiles with one continuous K loop. Every case compares runs on against runs off (one workgroup per tile)
bitwise, with the workgroup count forced small (WITW_CONV_WINO_WGS) so that a run holds more than one tile on any device, and
asserts the instantiation name and the form of both launches. One case checks parity with an fp64 reference.

Cout = 64 without a pool is no class of the Winograd form (conv3x3_nhwc_f32_kernel<64,1,false,*,0,9> is direct only): that case of
the chunk-count grid still compares the two settings bitwise and asserts the direct form for both."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

WGS = (1, 3, 8)


def _ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from witw_amd import ops
    return ops


def _data(B, H, W, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(B, H, W, cin, generator=g)).cuda()
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).cuda()
    b = ((torch.rand(cout, generator=g) - 0.5) * 0.1).cuda()
    return x, w, b


def _run(ops, x, pk, circ, pool, nw, run, wgs=None):
    """one launch with runs on / off, NW forced, the workgroup count forced when given -> (y, instantiation, form)"""
    env = {'WITW_CONV_NW': str(nw), 'WITW_CONV_WINO_WGS': None if wgs is None else str(wgs)}
    old = {k: os.environ.get(k) for k in env}
    prev = ops.conv_wino_run(run)
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        y = ops.conv3x3_fwd(x, pk, circular=circ, relu=True, pool=pool)
        torch.cuda.synchronize()
        return y, ops.last_kernel_variant(), ops.last_conv_form()
    finally:
        ops.conv_wino_run(prev)
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _on_equals_off(ops, x, w, b, circ, pool, nw, wgs_list=WGS):
    cout = w.shape[0]
    pk = ops.PackedConv(w, b, wino=True)
    tn = 128 if cout >= 128 else 64
    name = 'conv3x3_nhwc_f32_kernel<%d,1,%s,%d,0,9>' % (tn, 'true' if pool else 'false', nw)
    form = 'wino_h2' if (tn == 128 or pool) else 'direct'
    y_off, v_off, f_off = _run(ops, x, pk, circ, pool, nw, False)
    assert (v_off, f_off) == (name, form)
    for wgs in wgs_list:
        y_on, v_on, f_on = _run(ops, x, pk, circ, pool, nw, True, wgs)
        assert (v_on, f_on) == (name, form), wgs
        assert torch.equal(y_on, y_off), 'runs of %d workgroups differ from one workgroup per tile' % wgs
    return y_off


def test_switch_reports_and_restores():
    ops = _ops()
    prev = ops.conv_wino_run()
    assert ops.conv_wino_run(False) == prev
    assert ops.conv_wino_run(prev) is False
    assert ops.conv_wino_run() == prev


@pytest.mark.parametrize('pool', [False, True])
@pytest.mark.parametrize('nw', [8, 4])
@pytest.mark.parametrize('cout', [64, 192])
@pytest.mark.parametrize('cin', [8, 16, 24])
def test_chunk_counts_at_the_first_last_boundary(cin, cout, nw, pool):
    """nkc = 1 (an item's only chunk is its first and its last), 2 and 3"""
    ops = _ops()
    x, w, b = _data(3, 16, 128, cin, cout, 100 + cin + cout + nw + int(pool))
    _on_equals_off(ops, x, w, b, True, pool, nw)


@pytest.mark.parametrize('circ', [True, False])
@pytest.mark.parametrize('pool', [False, True])
def test_run_seams(circ, pool):
    """B = 2, H = 16, W = 192, Cout = 128 at NW = 8: 2 n tiles x (2 images x 2 tile rows x 3 tile columns). With one workgroup the
    single run crosses every change of n tile, tile row and image; its first and last items hold the wrap / zero columns."""
    ops = _ops()
    x, w, b = _data(2, 16, 192, 16, 128, 7 + int(circ) + 2 * int(pool))
    _on_equals_off(ops, x, w, b, circ, pool, 8)


@pytest.mark.parametrize('B,H,W,cin,cout,pool,nw', [
    (3, 16, 128, 16, 128, False, 8),      # 32 indices of the padded XCD map, 24 tiles: holes inside the runs, 3 does not divide them
    (3, 8, 64, 16, 128, False, 8),        # one spatial tile per image, fewer spatial tiles than XCDs (plain map)
    (3, 8, 64, 16, 128, True, 4),
    (2, 16, 128, 24, 68, True, 8),        # second n tile holds 4 of its 64 channels
    (1, 13, 72, 8, 192, False, 4),        # odd H, ragged W
])
def test_ragged_ends(B, H, W, cin, cout, pool, nw):
    ops = _ops()
    x, w, b = _data(B, H, W, cin, cout, 31 + H + W + cout)
    _on_equals_off(ops, x, w, b, True, pool, nw, wgs_list=(1, 3, 5, 8, 1000))      # 1000: more workgroups than items


def test_an_image_does_not_depend_on_the_batch():
    ops = _ops()
    x, w, b = _data(5, 16, 128, 24, 128, 77)
    pk = ops.PackedConv(w, b, wino=True)
    for pool in (False, True):
        y5, _, f5 = _run(ops, x, pk, True, pool, 8, True, 3)
        y1, _, f1 = _run(ops, x[3:4].contiguous(), pk, True, pool, 8, True, 3)
        assert f5 == f1 == 'wino_h2'
        assert torch.equal(y1[0], y5[3])


def test_parity_with_fp64():
    """tolerance of test_conv_wino_gpu.py: 3e-5 x the largest reference output"""
    ops = _ops()
    x, w, b = _data(2, 16, 192, 64, 128, 5)
    y = _on_equals_off(ops, x, w, b, True, True, 8, wgs_list=(3,))
    xx = x.double().permute(0, 3, 1, 2)
    xx = torch.cat([xx[..., -1:], xx, xx[..., :1]], dim=3)
    ref = F.max_pool2d(torch.relu(F.conv2d(F.pad(xx, (0, 0, 1, 1)), w.double(), b.double())), 2).permute(0, 2, 3, 1)
    y_on, _, form = _run(ops, x, ops.PackedConv(w, b, wino=True), True, True, 8, True, 3)
    assert form == 'wino_h2' and torch.equal(y_on, y)
    scale = ref.abs().max().item()
    err = (y_on.double() - ref).abs().max().item()
    print('max error %.3g, scale %.3g' % (err, scale))
    assert err <= 3e-5 * scale, (err, scale)
