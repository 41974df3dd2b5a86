"""LDS-DMA staging of the Winograd form of conv3x3_nhwc_f32_kernel (witw_conv3x3_wino_dma): the K chunks of a launch reach the LDS
by buffer loads that write it directly instead of through registers. Nothing arithmetic differs, so every case compares the two
staging forms bitwise, asserts the Winograd form and the instantiation name of both launches, and runs inside guard bands
(tests/mem_arena.py): input and filter images stand between NaN canaries, the output is pre-filled with a canary.

The shapes are the smallest that reach every staging edge: Cin 8 / 16 / 24 (one chunk: prologue and last-chunk copy only; both
stage parities; three chunks), a partial first n tile, a whole one, a second (third, without the pool: that class starts at Cout
128) holding 4 channels, H 2 / 3 / 9 / 10 (tile rows above and below the image, a ragged last row pair), W 64 / 66 / 70 / 130
(ragged last column tile, the wrap across the seam), both paddings, pool on and off, NW 4 and 8, batch 1 and 3, tile runs off and
on (workgroup count forced small, WITW_CONV_WINO_WGS, so that a run holds several tiles). One case per class also compares with
the direct form at the tolerance of tests/test_conv_wino_gpu.py, 3e-5 x the largest output."""
import os

import pytest
import torch

from tests.mem_arena import Arena, ArenaTorch

pytestmark = pytest.mark.gpu

CINS = (8, 16, 24)
COUTS_POOL = (4, 64, 68)            # <64,1,true>: a partial n tile, a whole one, a second holding 4 channels
COUTS_PLAIN = (132, 128, 196)       # <128,1,false>: the third / fourth n tile holds 4 channels
HS = (2, 3, 9, 10)
WS = (64, 66, 70, 130)
BMAX, HMAX, WMAX, CMAX = 3, 10, 130, 24


def _ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from witw_amd import ops
    return ops


@pytest.fixture(scope='module')
def data():
    """one random image and one filter, cut to size by every case; left unchanged"""
    g = torch.Generator().manual_seed(2026)
    x = torch.relu(torch.randn(BMAX, HMAX, WMAX, CMAX, generator=g))
    w = torch.randn(196, CMAX, 3, 3, generator=g) * (2.0 / (9 * 16)) ** 0.5
    b = (torch.rand(196, generator=g) - 0.5) * 0.1
    return x.cuda(), w.cuda(), b.cuda()


class _Filters(object):
    """PackedConv per (cin, cout), its device images moved between NaN canaries of an arena that lives as long as the test"""

    def __init__(self, ops, data):
        self.ops, self.data, self.arena, self.cache = ops, data, Arena('cuda'), {}

    def get(self, cin, cout):
        if (cin, cout) not in self.cache:
            _x, w, b = self.data
            pk = self.ops.PackedConv(w[:cout, :cin].contiguous(), b[:cout].contiguous(), wino=True)
            pk.wpk, pk.wpk_wino, pk.bias = (self.arena.place(t, label=n) for t, n in
                                            ((pk.wpk, 'wpk'), (pk.wpk_wino, 'wpk_wino'), (pk.bias, 'bias')))
            self.cache[(cin, cout)] = pk
        return self.cache[(cin, cout)]


def _launch(ops, x, pk, circ, pool, nw, dma, run, wgs, wino=True, want_code=False):
    """one launch -> (outputs, instantiation, form)"""
    env = {'WITW_CONV_NW': str(nw), 'WITW_CONV_WINO_WGS': str(wgs) if (run and wgs) else None}
    old = {k: os.environ.get(k) for k in env}
    prev = ops.conv_wino_dma(dma), ops.conv_wino_run(run), ops.conv_wino(wino)
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        y = ops.conv3x3_fwd(x, pk, circular=circ, relu=True, pool=pool, want_pool_code=want_code)
        torch.cuda.synchronize()
        return y, ops.last_kernel_variant(), ops.last_conv_form()
    finally:
        ops.conv_wino_dma(prev[0])
        ops.conv_wino_run(prev[1])
        ops.conv_wino(prev[2])
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _dma_equals_registers(ops, monkeypatch, filters, data, B, H, W, cin, cout, circ, pool, nw, run, wgs):
    """both staging forms of one shape inside an arena -> the DMA form's output"""
    pk = filters.get(cin, cout)
    arena = Arena('cuda')
    want_code = pool and (cin == 16)
    with monkeypatch.context() as m:
        m.setattr(ops, 'torch', ArenaTorch(arena))
        x = arena.place(data[0][:B, :H, :W, :cin].contiguous(), label='x')
        got_d, v_d, f_d = _launch(ops, x, pk, circ, pool, nw, True, run, wgs, want_code=want_code)
        got_r, v_r, f_r = _launch(ops, x, pk, circ, pool, nw, False, run, wgs, want_code=want_code)
    case = (B, H, W, cin, cout, circ, pool, nw, run, wgs)
    name = 'conv3x3_nhwc_f32_kernel<%d,1,%s,%d,0,9>' % (128 if cout >= 128 else 64, 'true' if pool else 'false', nw)
    assert (v_d, f_d) == (name, 'wino_h2') and (v_r, f_r) == (name, 'wino_h2'), case
    arena.check([got_d, got_r])
    if want_code:
        assert torch.equal(got_d[1], got_r[1]), case
        got_d, got_r = got_d[0], got_r[0]
    assert got_d.shape == (B, H // 2 if pool else H, W // 2 if pool else W, cout), case
    assert torch.equal(got_d, got_r), 'LDS-DMA staging differs from register staging: %s' % (case,)
    return got_d


def test_switch_reports_and_restores():
    ops = _ops()
    prev = ops.conv_wino_dma()
    assert ops.conv_wino_dma(False) == prev
    assert ops.conv_wino_dma(prev) is False
    assert ops.conv_wino_dma() == prev


@pytest.mark.parametrize('pool', [False, True])
@pytest.mark.parametrize('nw', [8, 4])
def test_dma_equals_register_staging_at_every_staging_edge(nw, pool, data, monkeypatch):
    """every (H, W, padding) of the lists above; Cin, Cout, batch and tile runs cycle through their values underneath (periods 3,
    9, 2 and 4 over 32 cases: every (Cin, Cout) pair, every value beside both paddings)"""
    ops = _ops()
    filters = _Filters(ops, data)
    couts = COUTS_POOL if pool else COUTS_PLAIN
    k = 0
    for H in HS:
        for W in WS:
            for circ in (True, False):
                cin, cout = CINS[k % 3], couts[(k // 3) % 3]
                B = (1, 3)[(k // 2) % 2]
                run = (k // 4 + k) % 2 == 1
                _dma_equals_registers(ops, monkeypatch, filters, data, B, H, W, cin, cout, circ, pool, nw, run, 2)
                k += 1
    filters.arena.check()


@pytest.mark.parametrize('cin', CINS)
def test_tile_runs_of_three_items_and_more(cin, data, monkeypatch):
    """B = 3, H = 10, W = 130, Cout = 68 at NW = 4: 2 n tiles x 27 spatial tiles in 64 indices of the padded XCD map. 8 workgroups
    walk runs of 6 to 8 tiles with holes inside, 1 workgroup walks all 54; every run ends with the chunk that stages from empty
    records. NW = 8: 36 tiles."""
    ops = _ops()
    filters = _Filters(ops, data)
    for nw in (4, 8):
        for circ in (True, False):
            y1 = _dma_equals_registers(ops, monkeypatch, filters, data, 3, 10, 130, cin, 68, circ, True, nw, True, 8)
            y2 = _dma_equals_registers(ops, monkeypatch, filters, data, 3, 10, 130, cin, 68, circ, True, nw, True, 1)
            y3 = _dma_equals_registers(ops, monkeypatch, filters, data, 3, 10, 130, cin, 68, circ, True, nw, False, 0)
            assert torch.equal(y1, y3) and torch.equal(y2, y3)
    filters.arena.check()


@pytest.mark.parametrize('cout,pool', [(132, False), (132, True), (68, True)])      # <128,1,false>, <128,1,true>, <64,1,true>
def test_direct_form_agrees(cout, pool, data, monkeypatch):
    """tolerance of test_conv_wino_gpu.py: 3e-5 x the largest output"""
    ops = _ops()
    filters = _Filters(ops, data)
    for nw in (8, 4):
        y = _dma_equals_registers(ops, monkeypatch, filters, data, 3, 10, 130, 24, cout, True, pool, nw, True, 2)
        x = data[0][:3, :10, :130, :24].contiguous()
        pk = filters.get(24, cout)
        y_dir, _v, form = _launch(ops, x, pk, True, pool, nw, True, True, 2, wino=False)
        assert form == 'direct'
        scale = y_dir.abs().max().item()
        err = (y.double() - y_dir.double()).abs().max().item()
        print('NW %d: max |wino_h2 (DMA) - direct| %.3g, scale %.3g' % (nw, err, scale))
        assert err <= 3e-5 * scale, (nw, err, scale)
    filters.arena.check()
