"""Orientation prior (shift masks) without a GPU: the mask helper's bit patterns, the masked restatement of the oracle, the
geometry behind heatmap's --heading, and the host-side plumbing (errors raised before any launch, chunked mask slices)."""
import os

import numpy as np
import pytest
import torch

from oracle import cvig_fov_oracle as O
from witw_amd import synth

from . import match_window_ref as R


def _bits(word):
    return [k for k in range(64) if (int(word) >> k) & 1]


# ----------------------------------------------------------------------------- orientation_mask
def test_orientation_mask_hand_worked_bit_patterns():
    """deg(k) = k * 5.625 - 180: shift 32 looks along 0, shift 48 along 90, shifts 0 / 63 sit either side of +-180."""
    from witw_amd.cvig_fov import orientation_mask
    m = orientation_mask(0., 0.)
    assert m.dtype == torch.int64 and m.shape == (1,) and _bits(m[0]) == [32]          # width 0: exactly one bit
    assert _bits(orientation_mask(0., 5.625)[0]) == [31, 32, 33]                       # the bound is inclusive
    assert _bits(orientation_mask(0., 5.6)[0]) == [32]
    assert _bits(orientation_mask(90., 12.)[0]) == [46, 47, 48, 49, 50]
    # wrap across +-180: -180 is shift 0, its neighbours are shifts 1 and 63
    assert _bits(orientation_mask(-180., 6.)[0]) == [0, 1, 63]
    assert int(orientation_mask(-180., 6.)[0]) < 0                                     # bit 63: a negative int64 word
    assert _bits(orientation_mask(177., 8.)[0]) == [0, 63]                             # 174.375 (2.625 away), -180 = 180 (3)
    assert _bits(orientation_mask(177., 8.5)[0]) == [0, 62, 63]                        # + 168.75 (8.25); -174.375 is 8.625 away
    assert _bits(orientation_mask(540., 6.)[0]) == [0, 1, 63]                          # the centre itself wraps
    # the nearest shift is always allowed: 179 is 1 degree from shift 0 (-180) and 4.625 from shift 63
    assert _bits(orientation_mask(179., 0.)[0]) == [0]
    assert _bits(orientation_mask(2.8125, 0.)[0]) == [32]                              # midway between 32 and 33: the lower one
    assert _bits(orientation_mask(2.8125, 2.8125)[0]) == [32, 33]
    # >= 180: everything
    assert int(orientation_mask(33., 180.)[0]) == -1 and int(orientation_mask(-70., 1e9)[0]) == -1
    assert _bits(orientation_mask(0., 179.9)[0]) == list(range(1, 64))                 # all but shift 0, 180 away
    # per-query arrays and tensors, broadcasting of a scalar against a vector
    m = orientation_mask(np.array([0., 90.]), torch.tensor([0., 5.625]))
    assert m.shape == (2,) and _bits(m[0]) == [32] and _bits(m[1]) == [47, 48, 49]
    m = orientation_mask([-90., 0., 90.], 0.)
    assert [_bits(w) for w in m] == [[16], [32], [48]]
    # another resolution of the shift axis
    assert _bits(orientation_mask(0., 11.25, output_width_max=32)[0]) == [15, 16, 17]
    assert int(orientation_mask(0., 180., output_width_max=32)[0]) == 2 ** 32 - 1
    for c in np.linspace(-400., 400., 41):                                              # never 0
        for hw in (0., 1., 50.):
            assert int(orientation_mask(c, hw)[0]) != 0


def test_orientation_mask_matches_a_plain_loop():
    from witw_amd.cvig_fov import orientation_mask
    g = np.random.Generator(np.random.Philox(key=[7, 1]))
    c = g.uniform(-360., 360., 50)
    hw = g.uniform(0., 200., 50)
    m = orientation_mask(c, hw)
    for i in range(50):
        d = [abs((k * 5.625 - 180. - c[i] + 180.) % 360. - 180.) for k in range(64)]
        want = [k for k in range(64) if d[k] <= hw[i] or k == int(np.argmin(d))]
        assert _bits(m[i]) == want


def test_orientation_mask_rejects_bad_arguments():
    from witw_amd import _lib
    from witw_amd.cvig_fov import orientation_mask
    with pytest.raises(_lib.WitwError):
        orientation_mask(0., -1.)
    with pytest.raises(_lib.WitwError):
        orientation_mask(float('nan'), 1.)
    with pytest.raises(_lib.WitwError):
        orientation_mask(0., 1., output_width_max=65)


# ----------------------------------------------------------------------------- the restatement
def test_restatement_with_all_bits_set_is_the_oracle(golden_dir):
    g = np.load(os.path.join(golden_dir, 'matching.npz'))
    seed = int(g['seed'])
    for tag in 'abcde':
        bo, bs, we = (int(v) for v in g['%s_shape' % tag])
        ov = torch.from_numpy(synth.embeddings(seed, 100 + ord(tag), (bo, 16, 4, 64)))
        su = torch.from_numpy(synth.embeddings(seed, 200 + ord(tag), (bs, 16, 4, we)))
        ori_r, dist_r = O.match(ov, su)
        for word in (R.ALL, 0):                                   # a zero word = no prior
            mask = torch.full((bs,), word, dtype=torch.int64)
            assert torch.equal(R.correlation(ov, su, mask), O.correlation(ov, su))
            ori, dist = R.match(ov, su, mask)
            assert torch.equal(ori, ori_r) and torch.equal(dist, dist_r)
            ori_f, dist_f, _gap = R.match_fused(ov, su, mask)
            ori_of, dist_of = O.match_fused(ov, su)
            assert torch.equal(ori_f, ori_of) and torch.equal(dist_f, dist_of)
        # a real window: the choice lies inside it, and the fused fp64 form agrees with the materialising one
        mask = R.window_words(np.arange(bs) * 5 % 64, 1 + np.arange(bs) % 9)
        ori, dist = R.match(ov, su, mask)
        assert bool(torch.gather(R.allowed(mask)[None].expand(bo, -1, -1), 2, ori[..., None]).all())
        ori_f, dist_f, gap = R.match_fused(ov, su, mask)
        safe = gap > 1e-3
        assert torch.equal(ori_f[safe], ori[safe])
        np.testing.assert_allclose(dist_f[safe].numpy(), dist[safe].numpy(), rtol=0, atol=1e-5)


# ----------------------------------------------------------------------------- heading -> window
def test_polar_column_bearing_and_heading_window():
    """For a north-up tile, polar column x of 512 looks along bearing 180 + 360 x / 512; the chosen shift is the column (in
    units of 8) of the photo's left edge, so the CSV orientation is the bearing of the left edge wrapped to [-180, 180)."""
    from witw_amd import heatmap
    from witw_amd.cvig_fov import orientation_mask
    yy, xx = np.mgrid[0:256, 0:256]
    for (dx, dy), bearing in (((0, 60), 180.), ((-60, 0), 270.), ((0, -60), 0.), ((60, 0), 90.)):
        # row index grows to the SOUTH in a north-up raster: (dx, dy) = (0, +60) is a blob due south of the centre; the
        # transform's pole is pixel (128, 128), a blob half a pixel off it moves by about a column
        for c0 in (128., 127.5):
            tile = np.exp(-((xx - (c0 + dx)) ** 2 + (yy - (c0 + dy)) ** 2) / (2 * 6. ** 2)).astype(np.float32)
            polar = O.polar_transform(torch.from_numpy(tile)[None])[0]                  # [128,512]
            x = int(polar.sum(0).argmax())
            got = 180. + 360. * x / 512.
            assert abs((got - bearing + 180.) % 360. - 180.) <= 2 * 360. / 512.       # within two polar columns
            if c0 == 128.:
                assert x == int(round((bearing - 180.) % 360. * 512. / 360.))          # columns 0 / 128 / 256 / 384
    # shift k <-> polar column 8k <-> bearing 180 + 360 * 8k / 512, which is the CSV's k * 360 / 64 - 180 up to a full turn
    for k in range(64):
        assert (180. + 360. * 8 * k / 512. - (k * 360. / 64. - 180.)) % 360. == 0.
    # the optical axis is fov / 2 to the right of the left edge
    assert heatmap.heading_window(90., 70, 5.) == (55., 5.)
    assert heatmap.heading_window(10., 70, 20.) == (-25., 20.)
    assert heatmap.heading_window(200., 70) == (165., heatmap.DEFAULT_HEADING_TOLERANCE)
    assert heatmap.heading_window(250., 70, 0.) == (-145., 0.)                         # 215 wraps
    assert heatmap.heading_window(0., 360, 1.) == (-180., 1.)
    assert heatmap.heading_window(None, 70) is None
    with pytest.raises(ValueError):
        heatmap.heading_window(None, 70, 5.)
    with pytest.raises(ValueError):
        heatmap.heading_window(10., 70, -5.)
    # a photo of fov 90 looking due north-east (45): its left edge looks north = shift 32
    c, hw = heatmap.heading_window(45., 90, 0.)
    assert _bits(orientation_mask(c, hw)[0]) == [32]
    # CLI
    with pytest.raises(SystemExit):
        heatmap.main(['--heading-tolerance', '5'])


# ----------------------------------------------------------------------------- host plumbing
def _problem(n=10, we=12, seed=4):
    gal = torch.from_numpy(synth.embeddings(seed, 1, (n, 16, 4, 64)))
    qry = torch.stack([torch.roll(gal[i], -3 * i, dims=2)[:, :, :we] for i in range(n)]) \
        + 6.0 * torch.from_numpy(synth.embeddings(seed, 2, (n, 16, 4, we)))
    mask = R.window_words((np.arange(n) * 7 + 3) % 64, 1 + np.arange(n) % 5)
    return gal, qry.contiguous(), mask


def test_spectral_pass_with_a_mask_is_an_error_before_any_launch():
    from witw_amd import _lib, cvig_fov
    gal, qry, mask = _problem()
    with pytest.raises(_lib.WitwError, match='spectral'):
        cvig_fov.evaluation_ranks(gal, qry, method='dft', shift_mask=mask)
    with pytest.raises(_lib.WitwError, match='spectral'):
        cvig_fov.retrieve(gal, qry, k=3, method='dft', shift_mask=mask)
    with pytest.raises(_lib.WitwError, match='spectral'):
        cvig_fov.retrieve(gal, qry, k=30, method='dft', shift_mask=mask)       # the branch that splits ranks and top-k
    with pytest.raises(_lib.WitwError, match='one word per query'):
        cvig_fov.sharded_ranks(gal, qry, 0, shift_mask=mask[:-1], _match=O.match)
    with pytest.raises(_lib.WitwError, match='one word per query'):
        cvig_fov.match(gal, qry, shift_mask=mask.to(torch.int32))


class _CpuKernels(object):
    """The op set of retrieve() on the masked restatement; records the mask slice of every call."""
    seen = []

    @classmethod
    def match_fwd(cls, ov, su, want_score=False, want_workspace=False, shift_mask=None):
        cls.seen.append((su.shape[0], None if shift_mask is None else shift_mask.clone()))
        if shift_mask is None:
            return O.match(ov, su)
        return R.match(ov, su, shift_mask)

    @staticmethod
    def rank_count_thresh(dist, thr):
        return (dist <= thr[None, :]).sum(0).to(torch.int32)

    @staticmethod
    def topk_smallest(dist, k, index_offset=0):
        order = torch.argsort(dist, dim=0, stable=True)[:k]
        return torch.gather(dist, 0, order).t().contiguous(), (order + index_offset).t().contiguous()


def test_chunked_passes_hand_each_query_chunk_its_slice_of_the_mask():
    from witw_amd import cvig_fov
    n = 10
    gal, qry, mask = _problem(n)
    _, d_ref = R.match(gal, qry, mask)
    ranks_ref = (d_ref <= torch.diagonal(d_ref)[None, :]).sum(0).numpy()
    _, d_free = O.match(gal, qry)
    assert not torch.equal(d_ref, d_free)                       # the windows do change the distances of this problem

    seen = []

    def _match(ov, su, shift_mask=None):
        seen.append(shift_mask.clone())
        return R.match(ov, su, shift_mask)

    r = cvig_fov.sharded_ranks(gal, qry, 0, query_chunk=4, _match=_match, shift_mask=mask,
                               _count=_CpuKernels.rank_count_thresh)
    np.testing.assert_array_equal(r, ranks_ref)
    assert [tuple(m.tolist()) for m in seen] == [tuple(mask[a:a + 4].tolist()) for a in (0, 4, 8)]
    # without a mask the injected op is called as before, without the keyword
    r0 = cvig_fov.sharded_ranks(gal, qry, 0, query_chunk=4, _match=O.match, _count=_CpuKernels.rank_count_thresh)
    np.testing.assert_array_equal(r0, (d_free <= torch.diagonal(d_free)[None, :]).sum(0).numpy())

    for method in ('direct', 'auto'):                           # a mask resolves 'auto' to the direct pass
        _CpuKernels.seen = []
        rk, v, i = cvig_fov.retrieve(gal, qry, k=3, query_chunk=3, method=method, _kernels=_CpuKernels, shift_mask=mask)
        np.testing.assert_array_equal(rk, ranks_ref)
        assert [(nq, tuple(m.tolist())) for nq, m in _CpuKernels.seen] == \
            [(len(mask[a:a + 3]), tuple(mask[a:a + 3].tolist())) for a in (0, 3, 6, 9)]
        order = torch.argsort(d_ref, dim=0, stable=True)[:3]
        assert torch.equal(i, order.t()) and torch.equal(v, torch.gather(d_ref, 0, order).t())
    _CpuKernels.seen = []
    v2, i2 = cvig_fov.retrieve_topk(gal, qry, k=3, query_chunk=10, _kernels=_CpuKernels, shift_mask=mask)
    assert torch.equal(i2, i) and torch.equal(v2, v) and len(_CpuKernels.seen) == 1


def test_cli_orientation_window_parses():
    import argparse
    from witw_amd import cvig_fov
    assert cvig_fov.parse_orientation_window('0,20') == (0., 20.)
    assert cvig_fov.parse_orientation_window('-172.5,0') == (-172.5, 0.)
    for bad in ('10', '1,2,3', 'a,b', '0,-1'):
        with pytest.raises(argparse.ArgumentTypeError):
            cvig_fov.parse_orientation_window(bad)
