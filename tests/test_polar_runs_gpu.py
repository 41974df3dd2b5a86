"""polar_from_raw_kernel (csrc/preprocess.hip: Resize -> ImageNormalization -> PolarTransform in one launch) where a wave takes a RUN
of planes: between planes it rebuilds its LDS term tables when the source size changes and switches between the 2:1 HALF path and the
general one. The launcher gives a wave ceil(B * C * n_tile / 24576) planes -- one until B * C >= 97 with the model's 256 tiles -- so
the benchmark and the data path (B = 128) run there and the small batches of tests/test_match_gpu.py do not.

Every comparison is torch.equal against the separate launches (resize_batched / resize_bilinear, then polar_transform), which the
kernel promises to reproduce bit for bit; one case per source kind also meets the oracle's own composition under the 2e-5 that
tests/test_match_gpu.py::test_fused_resize_normalize_polar_against_the_oracle_directly derives.

    forced runs       WITW_PR_PPW = 2, 3, 4, 7 (read on every call) on a table of five images (512,512) (300,777) (512,512) (97,64)
                      (256,256), C = 3 and 5: runs cross image boundaries, start and end on HALF planes, rebuild the tables mid-run
                      and (but for 15 planes in runs of 3) end on a ragged last run; as fp32 planar and as uint8 HWC with cs = C
                      and cs = C + 1 stored bytes per pixel, the spare byte 255 (five channels do not fit cs = 3 or 4: the C = 5
                      tables store 5 and 6);
                      normalisation on (SEM_MEAN / SEM_STD, n_div255 = 3) and off
    natural runs      no variable: 40 x 3 x 60 x 52 uniform fp32, and a table of 20 mixed images x 5 channels; the test computes
                      the launcher's planes per wave from ops.polar_tiles and asserts >= 2
    second geometry   size 128 -> 64 x 256, forced 3, a three-image table whose (256,256) image is that geometry's HALF source
    true division     a divisor with an all-ones significand (1.9999999) inside a run of planes
    batched resize    resize_batched(kind=1) against kind=0 of the same pixels as floats, cs 3 and 4, wfull > width with a
                      wrapping start"""
import numpy as np
import pytest
import torch

from oracle import cvig_fov_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
SIZES = ((512, 512), (300, 777), (512, 512), (97, 64), (256, 256))
PLANE_UNITS = 24576           # the launcher's (tile, run of planes) units: planes per wave = ceil(B * C * n_tile / 24576)


class Table(object):
    """a descriptor table [B,5] int64 = {address, H, W, start column, stored channels} and the tensors it points into (kept alive);
    .planar: the same pixels as fp32 CHW tensors"""

    def __init__(self, seed, sizes, C, kind, cs=None, starts=None):
        g = np.random.Generator(np.random.Philox(key=[seed, C]))
        cs = C if cs is None else cs
        self.B, self.C, self.kind = len(sizes), C, kind
        self.planar, self.src, rows = [], [], []
        for i, (H, W) in enumerate(sizes):
            px = g.integers(0, 256, (H, W, cs), dtype=np.uint8)
            px[:, :, C:] = 255
            self.planar.append(torch.from_numpy(np.ascontiguousarray(px[:, :, :C].transpose(2, 0, 1)).astype(np.float32)))
            t = (torch.from_numpy(px) if kind == 1 else self.planar[-1]).to(DEV).contiguous()
            self.src.append(t)
            rows.append([t.data_ptr(), H, W, 0 if starts is None else starts[i], cs if kind == 1 else 1])
        self.desc = torch.tensor(rows, dtype=torch.int64).to(DEV)


def _norm(C, on):
    return (list(O.SEM_MEAN)[:C], list(O.SEM_STD)[:C], 3) if on else (None, None, None)


def _fused(ops, t, norm, **geo):
    m, s, nd = norm
    return ops.polar_from_raw(desc=t.desc, kind=t.kind, batch=t.B, channels=t.C, mean=m, std=s, n_div255=nd, **geo)


def _separate(ops, t, norm, size=256, h_s=128, w_s=512):
    m, s, nd = norm
    return ops.polar_transform(ops.resize_batched(t.desc, t.B, t.C, (size, size), kind=t.kind, mean=m, std=s, n_div255=nd), h_s, w_s)


SOURCES = [(0, 0), (1, 0), (1, 1)]        # (kind, spare stored bytes per pixel)


@pytest.mark.parametrize('on', [True, False], ids=['norm', 'raw'])
@pytest.mark.parametrize('kind,spare', SOURCES, ids=['f32', 'u8', 'u8spare'])
@pytest.mark.parametrize('C', [3, 5])
@pytest.mark.parametrize('ppw', [2, 3, 4, 7])
def test_forced_runs_equal_the_separate_launches(monkeypatch, ppw, C, kind, spare, on):
    from witw_amd import ops
    t = Table(300 + spare, SIZES, C, kind, C + spare)
    monkeypatch.delenv('WITW_PR_PPW', raising=False)
    ref = _separate(ops, t, _norm(C, on))
    monkeypatch.setenv('WITW_PR_PPW', str(ppw))
    got = _fused(ops, t, _norm(C, on))
    assert got.shape == (5, C, 128, 512) and torch.equal(got, ref), (ppw, C, kind, spare, on, float((got - ref).abs().max()))
    if kind == 1:      # the same pixels as floats, in a run of their own length
        assert torch.equal(got, _fused(ops, Table(300 + spare, SIZES, C, 0, C + spare), _norm(C, on)))


@pytest.mark.parametrize('kind', [0, 1], ids=['f32', 'u8'])
def test_forced_run_meets_the_oracle(monkeypatch, kind):
    """the oracle's own composition, image by image, 2e-5 absolute (derivation: tests/test_match_gpu.py)"""
    from witw_amd import ops
    t = Table(310, SIZES, 3, kind, 3 + kind)
    monkeypatch.setenv('WITW_PR_PPW', '3')
    got = ops.polar_from_raw(desc=t.desc, kind=kind, batch=5, channels=3, mean=list(O.IMG_MEAN), std=list(O.IMG_STD), n_div255=3).cpu()
    for i in range(5):
        ref = O.polar_transform(O.image_normalization(O.resize_pair(torch.zeros(3, 224, 224), t.planar[i])[1]))
        np.testing.assert_allclose(got[i].numpy(), ref.numpy(), rtol=0, atol=2e-5, err_msg=str((kind, i)))


def _natural_ppw(ops, planes, **geo):
    n_tile = ops.polar_tiles(DEV, **geo)[0].shape[0]
    return -(-planes * n_tile // PLANE_UNITS)


def test_natural_runs_equal_the_separate_launches(monkeypatch):
    from witw_amd import ops
    monkeypatch.delenv('WITW_PR_PPW', raising=False)
    assert _natural_ppw(ops, 40 * 3) >= 2 and _natural_ppw(ops, 20 * 5) >= 2        # else the cases below run one plane per wave
    g = np.random.Generator(np.random.Philox(key=[320, 1]))
    x = torch.from_numpy(g.integers(0, 256, (40, 3, 60, 52)).astype(np.float32)).to(DEV)
    for on in (True, False):
        m, s, nd = _norm(3, on)
        ref = ops.polar_transform(ops.resize_bilinear(x, (256, 256), m, s, nd))
        assert torch.equal(ops.polar_from_raw(x, mean=m, std=s, n_div255=nd), ref), on
    t = Table(321, [SIZES[i % 5] for i in range(20)], 5, 0)
    for on in (True, False):
        assert torch.equal(_fused(ops, t, _norm(5, on)), _separate(ops, t, _norm(5, on))), on


def test_second_geometry_forced_run(monkeypatch):
    from witw_amd import ops
    geo = dict(size=128, h_s=64, w_s=256)
    for kind in (0, 1):
        t = Table(330, [(256, 256), (300, 777), (97, 64)], 3, kind, 3 + kind)
        monkeypatch.delenv('WITW_PR_PPW', raising=False)
        ref = _separate(ops, t, _norm(3, True), **geo)
        monkeypatch.setenv('WITW_PR_PPW', '3')
        assert torch.equal(_fused(ops, t, _norm(3, True), **geo), ref), kind


def test_true_division_inside_a_run(monkeypatch):
    """1.9999999 rounds to the fp32 number below 2, whose significand is all ones: div_exact takes the true division for that channel
    and the reciprocal form for its neighbours, plane after plane of one wave"""
    from witw_amd import ops
    norm = ([0.1, -3.0, 0.406], [1.9999999, 7.0, 0.225], 1)
    assert np.float32(1.9999999).view(np.uint32) & 0x7fffff == 0x7fffff
    for kind in (0, 1):
        t = Table(340, SIZES, 3, kind)
        monkeypatch.delenv('WITW_PR_PPW', raising=False)
        ref = _separate(ops, t, norm)
        monkeypatch.setenv('WITW_PR_PPW', '4')
        assert torch.equal(_fused(ops, t, norm), ref), kind


@pytest.mark.parametrize('spare', [0, 1], ids=['cs3', 'cs4'])
def test_batched_resize_of_bytes_equals_that_of_floats(spare):
    """resize_batched(kind=1) against kind=0 on the same pixels: the panorama form, 128 x 160 of 512 columns from a start that wraps
    (the last `start + 160 - 512` columns come from the front), mixed sizes in one table, with and without normalisation"""
    from witw_amd import ops
    sizes, starts = [(120, 400), (97, 64), (512, 512), (300, 777)], [500, 0, 353, 511]
    a = Table(350, sizes, 3, 1, 3 + spare, starts)
    b = Table(350, sizes, 3, 0, 3 + spare, starts)
    for on in (True, False):
        m, s, nd = _norm(3, on)
        ya = ops.resize_batched(a.desc, 4, 3, (128, 160), wfull=512, kind=1, mean=m, std=s, n_div255=nd)
        yb = ops.resize_batched(b.desc, 4, 3, (128, 160), wfull=512, kind=0, mean=m, std=s, n_div255=nd)
        assert torch.equal(ya, yb), (spare, on, float((ya - yb).abs().max()))
    # the wrap itself: the full-width resize, rolled by the start
    full = ops.resize_batched(b.desc.clone().index_fill_(1, torch.tensor([3], device=DEV), 0), 4, 3, (128, 512), wfull=512, kind=0)
    for i, st in enumerate(starts):
        assert torch.equal(yb[i], torch.roll(full[i], -st, dims=2)[:, :, :160]), i
