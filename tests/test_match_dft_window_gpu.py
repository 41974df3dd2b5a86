"""Orientation prior on the spectral pass, on the GPU: witw_match_fwd_dft_masked against the masked fp64 restatement
(tests/match_window_ref.py), mask equivalences, degenerate inputs, witw_match_pairs_masked against the masked direct kernel
(bits) and retrieve(method='dft_masked') against retrieve(method='direct') under the same masks (ranks and indices equal)."""
import numpy as np
import pytest
import torch

from witw_amd import synth

from . import match_window_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 64), (33, 31, 12), (70, 5, 63), (130, 257, 64), (517, 529, 40)]


def _pattern_masks(bs, seed):
    """per query, cycling: zero word, all ones, one bit out of {0, 31, 32, 63}, a window 60..4 across the wrap, bits 32-63 only,
    bits 0-31 only, a random word"""
    g = np.random.Generator(np.random.Philox(key=[81, seed]))
    rnd = g.integers(0, 2 ** 63, size=bs, dtype=np.int64) ^ (g.integers(0, 2, size=bs, dtype=np.int64) << 63)
    rows = []
    for s in range(bs):
        kind = s % 7
        if kind == 0:
            rows.append(torch.zeros((), dtype=torch.int64))
        elif kind == 1:
            rows.append(torch.tensor(R.ALL, dtype=torch.int64))
        elif kind == 2:
            rows.append(R.words([[(0, 31, 32, 63)[(s // 7) % 4]]])[0])
        elif kind == 3:
            rows.append(R.window_words([60], [9])[0])
        elif kind == 4:
            rows.append(R.words([list(range(32, 64))])[0])
        elif kind == 5:
            rows.append(R.words([list(range(32))])[0])
        else:
            rows.append(torch.tensor(int(rnd[s]), dtype=torch.int64))
    return torch.stack(rows)


_REF = {}


def _reference(shape):
    """embeddings, masks and the fp64 restatement of one shape, computed once and shared"""
    if shape not in _REF:
        bo, bs, we = shape
        ov = torch.from_numpy(synth.embeddings(11, bo, (bo, 16, 4, 64)))
        su = torch.from_numpy(synth.embeddings(12, bs, (bs, 16, 4, we)))
        mask = _pattern_masks(bs, bo)
        ori, dist, gap = R.match_fused(ov, su, mask)
        scale = ov.double().reshape(bo, -1).norm(dim=1)[:, None] * su.double().reshape(bs, -1).norm(dim=1)[None, :]
        _REF[shape] = (ov, su, mask, ori, dist, gap, scale, R.allowed(mask))
    return _REF[shape]


@pytest.mark.parametrize('shape', SHAPES)
def test_masked_dft_kernel_against_the_fp64_restatement(shape):
    """Every orientation is an allowed shift; it equals the reference wherever the fp64 gap between the two best allowed scores
    exceeds 4e-6 |ov||su| (the bound of test_rank_count_band_and_gap), at most 0.2 % of the pairs are excluded that way (the
    fp64 reference alone excludes 0, 0, 3.3e-4 and 4.4e-4 of the pairs of the last four shapes; single-bit queries have an
    infinite gap and are never excluded); distances within 1e-5 where the orientation agrees; the gap output within
    4e-6 |ov||su| of the allowed gap, +inf where one shift is allowed. Plain, value-only and gap instantiation."""
    from witw_amd import ops
    bo, bs, we = shape
    ov, su, mask, ori_r, dist_r, gap_r, scale, allowed = _reference(shape)
    ovc, suc, mc = ov.cuda(), su.cuda(), mask.cuda()
    clear = gap_r > 4e-6 * scale
    excluded = 1.0 - float(clear.double().mean())
    print('shape %s: excluded share %.2e' % (shape, excluded))
    assert excluded <= 2e-3
    single = (allowed.sum(1) == 1)
    assert bool(clear[:, single].all()) and bool(torch.isinf(gap_r[:, single]).all())
    ori, dist = ops.match_fwd_dft(ovc, suc, shift_mask=mc)                                   # plain
    ori_g, dist_g, gap, _ws = ops.match_fwd_dft(ovc, suc, want_gap=True, shift_mask=mc)      # gap
    dist_v = ops.match_fwd_dft(ovc, suc, want_orientation=False, shift_mask=mc)[1]           # value-only at We = 64
    for o, d in ((ori.cpu(), dist.cpu()), (ori_g.cpu(), dist_g.cpu())):
        assert bool(torch.gather(allowed[None].expand(bo, -1, -1), 2, o[..., None]).all())   # all pairs, no exclusion
        assert torch.equal(o[clear], ori_r[clear])
        same = o == ori_r
        err = float((d - dist_r)[same].abs().max())
        print('shape %s: largest distance error %.2e' % (shape, err))
        assert err <= 1e-5
    same = ori.cpu() == ori_r
    if we == 64:
        assert float((dist_v.cpu() - dist_r)[same].abs().max()) <= 1e-5
    else:
        assert torch.equal(dist_v, dist)
    gap = gap.cpu().double()
    finite = torch.isfinite(gap_r)
    assert bool(torch.isinf(gap[~finite]).all()) and bool((gap[~finite] > 0).all())
    gerr = (gap - gap_r)[finite].abs() / scale[finite] if bool(finite.any()) else torch.zeros(1)
    print('shape %s: largest gap error %.2e |ov||su|' % (shape, float(gerr.max())))
    assert float(gerr.max()) <= 4e-6


@pytest.mark.parametrize('shape', [(130, 257, 64), (33, 31, 12)])
def test_all_ones_zero_and_no_mask_give_the_same_bits(shape):
    from witw_amd import ops
    bo, bs, we = shape
    ov, su = _reference(shape)[:2]
    ovc, suc = ov.cuda(), su.cuda()
    ones = torch.full((bs,), R.ALL, dtype=torch.int64, device='cuda')
    zero = torch.zeros((bs,), dtype=torch.int64, device='cuda')
    for kw in ({}, {'want_orientation': False}, {'want_gap': True}):
        base = ops.match_fwd_dft(ovc, suc, **kw)
        for m in (ones, zero):
            got = ops.match_fwd_dft(ovc, suc, shift_mask=m, **kw)
            for a, b in zip(base[:3], got[:3]):
                assert (a is None and b is None) or torch.equal(a, b)


def test_masked_dft_degenerate_inputs():
    from witw_amd import ops
    rng = np.random.default_rng(11)
    mask = _pattern_masks(70, 3).cuda()
    z_ov, z_su = torch.zeros((40, 16, 4, 64), device='cuda'), torch.zeros((70, 16, 4, 64), device='cuda')
    ori = ops.match_fwd_dft(z_ov, z_su, shift_mask=mask)[0]
    lowest = R.allowed(mask.cpu()).float().argmax(1).cuda()                     # each query's lowest allowed shift
    assert torch.equal(ori, lowest[None, :].expand(40, -1)) and torch.equal(ori, ops.match_fwd(z_ov, z_su, shift_mask=mask)[0])
    ov = torch.from_numpy(rng.standard_normal((40, 16, 4, 64)).astype(np.float32)).cuda()
    su = torch.from_numpy(rng.standard_normal((70, 16, 4, 64)).astype(np.float32)).cuda()
    mixed = su.clone()
    mixed[::2] = float('nan')
    o_ref, d_ref = ops.match_fwd_dft(ov, su, shift_mask=mask)
    o_mix, d_mix = ops.match_fwd_dft(ov, mixed, shift_mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(o_mix[:, 1::2], o_ref[:, 1::2]) and torch.equal(d_mix[:, 1::2], d_ref[:, 1::2])
    assert int(o_mix.min()) >= 0 and int(o_mix.max()) <= 63


@pytest.mark.parametrize('shape', [(130, 257, 64), (128, 128, 12), (40, 9, 1), (100, 77, 63)])
def test_masked_match_pairs_bit_identical_to_masked_match_fwd(shape):
    from witw_amd import _lib, ops
    bo, bs, we = shape
    ov = torch.from_numpy(synth.embeddings(61, bo, (bo, 16, 4, 64))).cuda()
    su = torch.from_numpy(synth.embeddings(62, bs, (bs, 16, 4, we))).cuda()
    mask = _pattern_masks(bs, bo).cuda()
    ori, dist, _score, ws = ops.match_fwd(ov, su, want_score=True, want_workspace=True, shift_mask=mask)
    assert not torch.equal(ori, ops.match_fwd(ov, su)[0])                      # the masks matter here
    g = np.random.Generator(np.random.Philox(key=[63, bo * bs]))
    n = min(bo * bs, 3000)
    flat = torch.from_numpy(g.choice(bo * bs, size=n, replace=False)).cuda()
    po, ps = (flat // bs).to(torch.int32).contiguous(), (flat % bs).to(torch.int32).contiguous()
    lib = _lib.load()
    prev = lib.witw_match_pairs_impl(-1)
    try:
        for impl in (1, 0):
            lib.witw_match_pairs_impl(impl)
            o2, d2 = ops.match_pairs(ov, su, ws[:bo * 64], ws[bo * 64:bo * 64 + bs], po, ps, shift_mask=mask)
            assert torch.equal(o2, ori.reshape(-1)[flat]), impl
            assert torch.equal(d2, dist.reshape(-1)[flat]), impl               # bits, not a tolerance
    finally:
        lib.witw_match_pairs_impl(prev)


def _planted(G, Q, we, noise, seed, near_ties=True):
    """Gallery + queries cut out of gallery rows, plus (near_ties) rows that differ from other rows by one last-place unit in
    a handful of entries and exact duplicates: distances that tie to well inside fp32 rounding or exactly."""
    gen = torch.Generator(device='cuda')
    gen.manual_seed(seed)
    gallery = torch.randn((G, 16, 4, 64), generator=gen, device='cuda')
    shifts = torch.randint(0, 64, (Q,), generator=gen, device='cuda')
    col = (torch.arange(we, device='cuda')[None, :] + shifts[:, None]) % 64
    queries = torch.gather(gallery[:Q], 3, col[:, None, None, :].expand(-1, 16, 4, -1)) \
        + noise * torch.randn((Q, 16, 4, we), generator=gen, device='cuda')
    if near_ties:
        n = min(Q, G // 4)
        src = torch.arange(n, device='cuda')
        dst = G - 1 - src
        gallery[dst] = gallery[src]                                  # duplicates of true matches far away in the gallery
        bump = gallery[dst[::2]].clone()
        bump[:, 0, 0, :3] = torch.nextafter(bump[:, 0, 0, :3], torch.full_like(bump[:, 0, 0, :3], 10.0))
        gallery[dst[::2]] = bump                                     # every other one: three entries one ulp up
    return gallery.contiguous(), queries.contiguous(), shifts


def _retrieval_masks(shifts):
    """a third of the queries: a window of width 1-9 holding the planted shift, a third: one that excludes it, a third: zero"""
    sh = shifts.cpu().numpy()
    q = len(sh)
    widths = 1 + np.arange(q) % 9
    starts = np.where(np.arange(q) % 3 == 0, sh - (np.arange(q) // 3) % widths, sh + 1 + (np.arange(q) % 20)) % 64
    m = R.window_words(starts, widths)
    m[2::3] = 0
    al = R.allowed(m)
    inside = al[torch.arange(q), torch.from_numpy(sh)]
    assert bool(inside[0::3].all()) and not bool(inside[1::3].any())
    return m.cuda()


@pytest.mark.parametrize('we', [64, 12])
def test_masked_dft_retrieve_equals_masked_direct_retrieve(we):
    from witw_amd import cvig_fov
    G, Q = 3000, 300
    gallery, queries, shifts = _planted(G, Q, we, 4.0 if we == 64 else 1.5, seed=7 + we)
    mask = _retrieval_masks(shifts)
    r0, v0, i0 = cvig_fov.retrieve(gallery, queries, k=10, query_chunk=128, shift_mask=mask)
    r1, v1, i1 = cvig_fov.retrieve(gallery, queries, k=10, query_chunk=128, method='dft_masked', shift_mask=mask)
    st = cvig_fov.last_retrieve_stats()
    np.testing.assert_array_equal(r1, r0)
    assert torch.equal(i1, i0)
    assert float((v1 - v0).abs().max()) <= st['eps']
    print('We=%d: %s' % (we, st))
    assert st['masked'] and st['rescored_rank'] > 0 and st['rescored_topk'] > 0 and st['fallback_queries'] <= Q // 50
    assert not np.array_equal(r0, cvig_fov.retrieve(gallery, queries, k=10, query_chunk=128)[0])      # the masks matter
    # the branch that splits ranks and top-k
    r2, v2, i2 = cvig_fov.retrieve(gallery, queries, k=27, query_chunk=128, method='dft_masked', shift_mask=mask)
    r3, v3, i3 = cvig_fov.retrieve(gallery, queries, k=27, query_chunk=128, shift_mask=mask)
    np.testing.assert_array_equal(r2, r0)
    assert torch.equal(i2, i3) and torch.equal(v2, v3)
    # evaluation_ranks: gallery row == query index over the first Q rows
    e0 = cvig_fov.evaluation_ranks(gallery[:Q].contiguous(), queries, method='direct', shift_mask=mask)
    e1 = cvig_fov.evaluation_ranks(gallery[:Q].contiguous(), queries, method='dft_masked', shift_mask=mask)
    np.testing.assert_array_equal(e1, e0)


@pytest.mark.parametrize('we', [64, 12])
def test_dft_masked_without_a_mask_is_dft(we):
    from witw_amd import cvig_fov
    gallery, queries, _ = _planted(3000, 300, we, 4.0 if we == 64 else 1.5, seed=7 + we)
    r0, v0, i0 = cvig_fov.retrieve(gallery, queries, k=10, query_chunk=128, method='dft')
    r1, v1, i1 = cvig_fov.retrieve(gallery, queries, k=10, query_chunk=128, method='dft_masked')
    np.testing.assert_array_equal(r1, r0)
    assert torch.equal(i1, i0) and torch.equal(v1, v0) and cvig_fov.last_retrieve_stats()['masked'] is False
