"""GPU parity of the masked match (witw_match_fwd_masked and the Python surface above it) against the masked restatement of
the oracle (tests/match_window_ref.py): all four kernel forms, identity with the unmasked entry, ties, backward, ranks /
top-k and the heat-map sweep with a heading."""
import numpy as np
import pytest
import torch

from oracle import cvig_fov_oracle as O
from witw_amd import synth

from . import match_window_ref as R

pytestmark = pytest.mark.gpu

# the shapes of test_match_ragged_shapes_vs_oracle (tests/test_match_gpu.py): they reach the generic, the shift-split, the
# full-width pipelined and the narrow pipelined kernel
SHAPES = [(1, 1, 64), (130, 257, 64), (3, 200, 1), (70, 5, 63), (1101, 130, 64), (1030, 129, 63), (128, 128, 64),
          (128, 128, 12), (128, 128, 33), (128, 128, 17), (100, 77, 64), (128, 128, 1)]
WIDTHS = [1, 2, 5, 16, 33, 64, 'random']
# + a mid-sized batch that takes match_kernel<1, 2> (two overheads x 128 surfaces per workgroup), which none of the twelve reaches
PARITY_SHAPES = SHAPES + [(512, 128, 20)]


def _embeddings(shape):
    bo, bs, we = shape
    return (torch.from_numpy(synth.embeddings(11, bo, (bo, 16, 4, 64))), torch.from_numpy(synth.embeddings(12, bs, (bs, 16, 4, we))))


def _windows(shape, width):
    """per-query random starts; `width` consecutive shifts (circular), or per-query random widths in [1, 64]"""
    bo, bs, we = shape
    g = np.random.Generator(np.random.Philox(key=[bo * 1000 + bs, we * 100 + (0 if width == 'random' else width)]))
    starts = g.integers(0, 64, bs)
    widths = g.integers(1, 65, bs) if width == 'random' else np.full(bs, width)
    return starts, widths, R.window_words(starts, widths)


def _inside(mask, ori):
    """(mask[s] >> orientation[o,s]) & 1 for all pairs"""
    return torch.gather(R.allowed(mask)[None].expand(ori.shape[0], -1, -1), 2, ori.cpu()[..., None]).squeeze(-1)


@pytest.mark.parametrize('shape', PARITY_SHAPES)
def test_masked_match_vs_restatement(shape):
    """Orientation equal to the restatement wherever the fp64 gap between the best and the second-best ALLOWED score exceeds
    1e-3 (the rule of test_match_ragged_shapes_vs_oracle), distance to 1e-5 there; more than 0.95 of the pairs compared. The
    chosen shift is inside the window for EVERY pair; with one allowed shift it is that shift for every pair."""
    from witw_amd import cvig_fov
    ov, su = _embeddings(shape)
    scores = R.scores_pair(ov, su)
    ovg, sug = ov.cuda(), su.cuda()
    for width in WIDTHS:
        starts, _widths, mask = _windows(shape, width)
        ori_r, dist_r, gap = R.match_fused(ov, su, mask, scores)
        safe = gap > 1e-3
        ori, dist = cvig_fov.match(ovg, sug, shift_mask=mask.cuda())
        ori, dist = ori.cpu(), dist.cpu()
        share = safe.float().mean().item()
        print('shape %s width %s: compared share %.4f, max |d - d_ref| %.2e' % (
            shape, width, share, float((dist[safe] - dist_r[safe]).abs().max())))
        assert bool(_inside(mask, ori).all()), 'a shift outside the window was chosen (width %s)' % (width,)
        assert torch.equal(ori[safe], ori_r[safe]), width
        np.testing.assert_allclose(dist[safe].numpy(), dist_r[safe].numpy(), rtol=0, atol=1e-5)
        assert share > 0.95
        if width == 1:
            assert bool(safe.all())
            assert torch.equal(ori, torch.from_numpy(starts.astype(np.int64))[None, :].expand(shape[0], -1))
        assert torch.equal(cvig_fov.correlation(ovg, sug, shift_mask=mask), ori.cuda())      # a CPU mask is moved over


@pytest.mark.parametrize('shape', SHAPES)
def test_all_ones_zero_and_no_mask_give_the_same_bits(shape):
    from witw_amd import ops
    ov, su = _embeddings(shape)
    ovg, sug = ov.cuda(), su.cuda()
    bs = shape[1]
    base = ops.match_fwd(ovg, sug, want_score=True)
    for word in (R.ALL, 0):
        got = ops.match_fwd(ovg, sug, want_score=True, shift_mask=torch.full((bs,), word, dtype=torch.int64, device='cuda'))
        for a, b in zip(got, base):
            assert torch.equal(a, b), word
    # a mix of the two words and of real windows next to them leaves the unrestricted queries alone
    mixed = torch.full((bs,), R.ALL, dtype=torch.int64)
    mixed[::2] = 0
    real = R.window_words(np.arange(bs) % 64, np.full(bs, 3))
    mixed[::3] = real[::3]
    got = ops.match_fwd(ovg, sug, want_score=True, shift_mask=mixed.cuda())
    free = torch.ones(bs, dtype=torch.bool)
    free[::3] = False
    for a, b in zip(got, base):
        assert torch.equal(a[:, free.cuda()], b[:, free.cuda()])
    assert bool(_inside(mixed, got[0]).all())


@pytest.mark.parametrize('shape', [(1030, 129, 63), (1101, 130, 64), (130, 1030, 12), (130, 1030, 40)])
def test_masked_generic_and_pipelined_kernels_give_the_same_bits(shape, monkeypatch):
    """WITW_MATCH_GENERIC=1 sends retrieval-sized problems to match_kernel<2, 2> / <1, 2> instead of the pipelined kernels (as in
    test_narrow_surface_pipelined_kernel_is_bit_identical): under a mask both must choose the same shifts with the same bits."""
    from witw_amd import ops
    ov, su = _embeddings(shape)
    ovg, sug = ov.cuda(), su.cuda()
    for width in (1, 5, 'random'):
        mask = _windows(shape, width)[2].cuda()
        got = ops.match_fwd(ovg, sug, want_score=True, shift_mask=mask)
        monkeypatch.setenv('WITW_MATCH_GENERIC', '1')
        gen = ops.match_fwd(ovg, sug, want_score=True, shift_mask=mask)
        monkeypatch.delenv('WITW_MATCH_GENERIC')
        for a, b in zip(got, gen):
            assert torch.equal(a, b), width
        assert bool(_inside(mask, gen[0]).all())


@pytest.mark.parametrize('n', [3, 128, 600])
def test_masked_ties_first_allowed_index(n):
    """The periodic overhead of test_match_tie_break_first_index: shifts 5, 21, 37, 53 tie exactly on the diagonal. The first
    ALLOWED one wins. n = 3 / 128 / 600: the generic, the shift-split (ties across its two halves) and the pipelined kernel."""
    from witw_amd import cvig_fov
    base = synth.embeddings(3, 1, (n, 16, 4, 16))
    ov = np.tile(base, (1, 1, 1, 4))
    su = np.ascontiguousarray(np.roll(ov, -5, axis=3)[:, :, :, :32])
    ovg, sug = torch.from_numpy(ov).cuda(), torch.from_numpy(su).cuda()
    for bits, want in (([21, 37], 21), ([53, 5], 5), ([37, 53], 37), ([53], 53), ([5, 21, 37, 53], 5), ([6, 53, 20], 53)):
        mask = R.words([bits] * n)
        ori = cvig_fov.correlation(ovg, sug, shift_mask=mask.cuda()).cpu()
        assert torch.equal(torch.diagonal(ori), torch.full((n,), want, dtype=torch.int64)), (bits, want)
        assert bool(_inside(mask, ori).all())
        if n == 3:
            ref = R.correlation(torch.from_numpy(ov), torch.from_numpy(su), mask)
            assert torch.equal(torch.diagonal(ref), torch.full((n,), want, dtype=torch.int64))
    # an all-zero overhead scores 0 at every shift: the first allowed index wins, not shift 0 (orientation only: d = 0/0)
    zero = torch.zeros_like(ovg)
    for bits, want in (([40, 9], 9), ([63], 63), ([33, 32], 32)):
        ori = cvig_fov.correlation(zero, sug, shift_mask=R.words([bits] * n).cuda()).cpu()
        assert torch.equal(ori, torch.full((n, n), want, dtype=torch.int64)), (bits, want)


def test_masked_match_backward_vs_autograd():
    """match(ov, su, shift_mask=m) under autograd against torch autograd through the fp64 restatement with the orientation held
    constant; shapes and tolerance of test_match_backward_rectangular_vs_oracle (tests/test_backward_gpu.py). The backward
    kernels are unchanged: they consume the orientation the masked forward chose."""
    from witw_amd import cvig_fov
    ov = torch.from_numpy(synth.embeddings(21, 1, (37, 16, 4, 64)))
    su = torch.from_numpy(synth.embeddings(22, 1, (29, 16, 4, 33)))
    g = np.random.Generator(np.random.Philox(key=[23, 1]))
    gd = torch.from_numpy(g.standard_normal((37, 29)).astype(np.float32))
    mask = R.window_words(g.integers(0, 64, 29), g.integers(1, 20, 29))
    _, _, gap = R.match_fused(ov, su, mask)
    assert bool((gap > 1e-3).all())                 # no near-tie among the allowed shifts of this problem
    ovr, sur = ov.double().requires_grad_(True), su.double().requires_grad_(True)
    ori_r = R.correlation(ov, su, mask)
    d_r = O.l2_distance(O.crop_overhead(ovr, ori_r, 33), sur)
    (d_r * gd.double()).sum().backward()
    ovg, sug = ov.cuda().requires_grad_(True), su.cuda().requires_grad_(True)
    ori, dg = cvig_fov.match(ovg, sug, shift_mask=mask.cuda())
    (dg * gd.cuda()).sum().backward()
    assert torch.equal(ori.cpu(), ori_r) and not ori.requires_grad
    np.testing.assert_allclose(dg.detach().cpu().numpy(), d_r.detach().float().numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(ovg.grad.cpu().numpy(), ovr.grad.float().numpy(), rtol=0, atol=5e-6)
    np.testing.assert_allclose(sug.grad.cpu().numpy(), sur.grad.float().numpy(), rtol=0, atol=5e-6)
    # the unrestricted match of the same pair has other gradients: the mask did reach the forward
    ov2, su2 = ov.cuda().requires_grad_(True), su.cuda().requires_grad_(True)
    ori2, d2 = cvig_fov.match(ov2, su2)
    assert not torch.equal(ori2, ori)


def test_masked_ranks_and_topk_vs_restatement():
    """ranks / retrieve on a few hundred rows against ranks and top-k from the restated distances, near-equal distances treated
    as test_retrieve_topk_matches_oracle_and_shards does; 'auto' with a mask runs the direct pass; chunking changes nothing."""
    from witw_amd import cvig_fov
    n, we, k = 300, 12, 5
    ov = torch.from_numpy(synth.embeddings(81, 1, (n, 16, 4, 64)))
    su = (torch.stack([torch.roll(ov[i], -int(i % 64), dims=2)[:, :, :we] for i in range(n)])
          + 5.0 * torch.from_numpy(synth.embeddings(81, 2, (n, 16, 4, we)))).contiguous()
    # the prior: the true shift i % 64 lies in a window of 9 shifts placed at random around it
    g = np.random.Generator(np.random.Philox(key=[81, 3]))
    mask = R.window_words((np.arange(n) % 64 - g.integers(0, 9, n)) % 64, np.full(n, 9))
    _, d_ref, _gap = R.match_fused(ov, su, mask)
    ovg, sug = ov.cuda(), su.cuda()
    rk, v, i = cvig_fov.retrieve(ovg, sug, k=k, method='direct', shift_mask=mask.cuda())
    ref_i = torch.argsort(d_ref, dim=0, stable=True)[:k].t()
    srt = torch.sort(d_ref, dim=0).values
    safe = (srt[1:k + 1] - srt[:k]).min(0).values > 1e-5            # queries whose top-(k+1) is free of near-ties
    assert safe.float().mean() > 0.9
    assert torch.equal(i.cpu()[safe], ref_i[safe])
    np.testing.assert_allclose(v.cpu().numpy(), srt[:k].t().numpy(), atol=1e-5)
    d_true = torch.diagonal(d_ref)
    ranks_ref = (d_ref <= d_true[None, :]).sum(0).numpy()
    near = ((d_ref - d_true[None, :]).abs() <= 1e-5).sum(0) > 1       # another row within rounding of the true match's distance
    assert near.float().mean() < 0.1
    np.testing.assert_array_equal(rk[~near.numpy()], ranks_ref[~near.numpy()])
    np.testing.assert_array_equal(cvig_fov.ranks(ovg, sug, shift_mask=mask)[~near.numpy()], ranks_ref[~near.numpy()])
    np.testing.assert_array_equal(cvig_fov.ranks(ovg, sug, shift_mask=mask), rk)
    # the prior changes results: the unrestricted ranks of this problem are not the masked ones
    assert not np.array_equal(cvig_fov.ranks(ovg, sug), rk)
    # 'auto' with a mask = the direct pass, also above the size where 'auto' alone would go spectral
    rk_a, v_a, i_a = cvig_fov.retrieve(ovg, sug, k=k, method='auto', shift_mask=mask)
    assert np.array_equal(rk_a, rk) and torch.equal(v_a, v) and torch.equal(i_a, i)
    old = cvig_fov.SPECTRAL_FROM
    cvig_fov.SPECTRAL_FROM = 100
    try:
        np.testing.assert_array_equal(cvig_fov.evaluation_ranks(ovg, sug, method='auto', shift_mask=mask), rk)
    finally:
        cvig_fov.SPECTRAL_FROM = old
    np.testing.assert_array_equal(cvig_fov.evaluation_ranks(ovg, sug, method='direct', shift_mask=mask), rk)
    # query chunks smaller than Bs: every chunk under its own slice of the mask
    for chunk in (64, 77):
        rk_c, v_c, i_c = cvig_fov.retrieve(ovg, sug, k=k, query_chunk=chunk, shift_mask=mask)
        assert np.array_equal(rk_c, rk) and torch.equal(v_c, v) and torch.equal(i_c, i)
        np.testing.assert_array_equal(cvig_fov.sharded_ranks(ovg, sug, 0, query_chunk=chunk, shift_mask=mask), rk)
        v_t, i_t = cvig_fov.retrieve_topk(ovg, sug, k=k, query_chunk=chunk, shift_mask=mask)
        assert torch.equal(v_t, v) and torch.equal(i_t, i)


def test_sweep_with_heading_stays_inside_the_window(tmp_path):
    """heatmap.sweep(heading=, heading_tolerance=) on the injected tile source of test_sweep_matches_oracle: every CSV
    orientation lies within the window, the rows are sweep_scores' under the same mask."""
    import pandas as pd
    from witw_amd import cvig_fov, heatmap
    fov = 70
    wts = synth.fov_dsm_weights(91)
    se = cvig_fov.FOV_DSM(circ_padding=False, weights=wts).cuda().eval()
    oe = cvig_fov.FOV_DSM(circ_padding=True, weights=wts).cuda().eval()
    strip = synth.images_u8(92, 1, (3, 150, 170))
    photo = torch.from_numpy(synth.images_u8(92, 2, (3, 90, 120)))
    src = heatmap.ArrayTileSource(strip, origin_x=1000., origin_y=5000., pixel_size=1.5)
    bounds, edge, offset = (1030., 4840., 1130., 4960.), 90., 45.
    _ce, _cn, windows = heatmap.tile_windows(bounds, edge, offset)
    su = heatmap.embed_photo(se, photo, fov)
    ov = heatmap.embed_tiles(oe, src, windows, 4)
    free = pd.DataFrame({'orientation': cvig_fov.sweep_scores(ov, su)[0].cpu().numpy()})
    for heading, tol in ((300., 12.), (20., None), (181., 0.)):
        csv = str(tmp_path / ('geomatch_%d.csv' % heading))
        df = heatmap.sweep(3, bounds, edge, offset, fov, None, None, csv, tile_source=src, surface_encoder=se,
                           overhead_encoder=oe, photo=photo, batch_size=4, heading=heading, heading_tolerance=tol)
        back = pd.read_csv(csv)
        assert list(back.columns) == ['x', 'y', 'orientation', 'dissimilarity', 'score'] and len(back) == len(df) == 9
        center, half = heatmap.heading_window(heading, fov, tol)
        assert center == (heading - fov / 2. + 180.) % 360. - 180.
        assert half == (heatmap.DEFAULT_HEADING_TOLERANCE if tol is None else tol)
        mask = cvig_fov.orientation_mask(center, half)
        shifts = np.round((back['orientation'].to_numpy() + 180.) * 64 / 360.).astype(np.int64)
        assert all((int(mask[0]) >> int(k)) & 1 for k in shifts)
        off = np.abs((back['orientation'].to_numpy() - center + 180.) % 360. - 180.)
        assert bool((off <= max(half, 360. / 64 / 2)).all())         # within the tolerance (or the one nearest shift)
        o, d, sc = cvig_fov.sweep_scores(ov, su, shift_mask=mask)
        np.testing.assert_array_equal(df['orientation'].to_numpy(), o.cpu().numpy())
        np.testing.assert_array_equal(df['dissimilarity'].to_numpy(), d.cpu().numpy())
        np.testing.assert_array_equal(df['score'].to_numpy(), sc.cpu().numpy())
        # and the restatement on the same embeddings
        ori_r, d_r = R.match(ov.cpu(), su.cpu(), mask)
        np.testing.assert_array_equal(back['orientation'].to_numpy(), (ori_r.squeeze() * 360 / 64 - 180).numpy())
        np.testing.assert_allclose(back['dissimilarity'].to_numpy(), d_r.squeeze().numpy(), atol=1e-5)
    assert len(free) == 9
    with pytest.raises(ValueError):
        heatmap.sweep(3, bounds, edge, offset, fov, None, None, str(tmp_path / 'x.csv'), tile_source=src, surface_encoder=se,
                      overhead_encoder=oe, photo=photo, heading_tolerance=5.)
