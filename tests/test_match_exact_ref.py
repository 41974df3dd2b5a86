"""tests/match_exact_ref.py pinned without a GPU: its float64 reference against the oracle, the exactness premise of its data
(fp32 in any summation order = float64), the planted ties of every case of tests/test_match_exact_gpu.py, and -- the point of
the module -- that on every case every deliberately wrong variant of the reference that applies to it changes the expected
orientation, score or distance bits of at least one pair: a kernel with that mistake cannot pass the GPU test of that case.

Large cases form their variants on probe_rows(): the planted rows, the block edges and both ends of the batch. A pair's
expectation depends on its two rows alone (the variants that read a neighbour rewrite the whole batch first), so a pair that
differs on the probe rows differs in the full case."""
import numpy as np
import pytest
import torch

from oracle import cvig_fov_oracle as O
from tests import match_exact_ref as R

SHAPES = sorted(set((c.Bo, c.Bs, c.We) for c in R.CASES))
_ids = lambda v: 'x'.join(str(x) for x in v[:3])


def _probe(Bo, Bs, We):
    ov, su = R.make_data(Bo, Bs, We)
    ro, rs = R.probe_rows(Bo, Bs)
    return ov, su, ro, rs


def _assert_seen(name, base, wrong, mask=None, shift=None, where=''):
    good = R.decide(base, mask=mask, shift=shift)
    bad = R.decide(wrong, mask=mask, shift=shift, variant=name)
    n = int(R.differs(good, bad).sum())
    assert n > 0, 'variant %s (%s) changes no pair %s' % (name, R.VARIANTS[name], where)
    return n


def test_the_cases_reach_the_kernel_forms_they_are_listed_under():
    forms = {}
    for c in R.CASES:
        assert c.form == R.dispatch(c.Bo, c.Bs, c.We, c.generic)
        forms.setdefault(c.form, []).append((c.Bo, c.Bs, c.We))
    assert set(forms) == {'match_kernel<1,1,false>', 'match_kernel_nsplit<16,false>', 'match_kernel_nsplit<32,false>',
                          'match_kernel_nsplit<64,false>', 'match_kernel<1,2,false>', 'match_kernel<2,2,false>',
                          'match_kernel_w64<false>', 'match_kernel_rows<4,false>', 'match_kernel_rows<2,false>',
                          'match_kernel_rows<1,false>'}
    assert forms['match_kernel<1,1,false>'] == [(1, 1, 64), (3, 200, 1), (70, 5, 63)]
    assert forms['match_kernel_rows<4,false>'] == [(510, 129, w) for w in (1, 7, 16)]
    assert forms['match_kernel_rows<2,false>'] == [(510, 129, w) for w in (17, 32)]
    assert forms['match_kernel_rows<1,false>'] == [(510, 129, w) for w in (33, 62)]
    assert forms['match_kernel_w64<false>'] == [(510, 129, 64), (510, 129, 63)]
    assert len(forms['match_kernel<1,2,false>']) == 10 and forms['match_kernel<2,2,false>'] == [(1021, 129, 33), (1021, 129, 64)]
    # the fixed form: one-tile supertiles on the shared shapes, 128-row supertiles with tails of 1..4 M-tiles on the large ones
    sizes = set()
    for Bo, Bs, We, lists in R.FIXED:
        assert R.fixed_rows_per_tile(Bo, Bs) == 32
        for w in lists:
            sh = R.make_shifts(Bo, Bs, We, w)
            assert sh.min() < 0 and sh.max() > 63
            sizes |= set(R.group_sizes(sh))
            assert R.fixed_tiles(sh, 32) == [1]
        assert {1, 31, 32, 33, 65} <= sizes
    for Bo, Bs, We, lists in R.FIXED_BIG:
        assert R.fixed_rows_per_tile(Bo, Bs) == 128
        assert R.fixed_tiles(R.make_shifts(Bo, Bs, We, lists[0]), 128) == [1, 2, 3, 4]
    assert sorted(set(16 if We <= 16 else 32 if We <= 32 else 64 for _, _, We, _ in R.FIXED)) == [16, 32, 64]
    assert sorted(set(16 if We <= 16 else 32 if We <= 32 else 64 for _, _, We, _ in R.FIXED_BIG)) == [16, 32, 64]


def test_reference_equals_the_oracle_in_float64():
    Bo, Bs, We = 9, 11, 17
    ov, su = R.make_data(Bo, Bs, We)
    base = R.build(ov, su)
    to, ts = torch.from_numpy(ov.reshape(Bo, 16, 4, 64)), torch.from_numpy(su.reshape(Bs, 16, 4, We))
    assert np.array_equal(base.sc, O.correlation_scores(to, ts).numpy())
    exp = R.decide(base)
    ori, dist = O.match_fused(to, ts)
    assert np.array_equal(exp.orientation, ori.numpy())
    with np.errstate(invalid='ignore'):
        d64 = 2 * (1 - exp.score / np.sqrt(np.take_along_axis(base.n2w, exp.orientation, 1) * base.n2s[None, :]))
    fin = np.isfinite(d64)
    assert (~fin).sum() == Bo + Bs - 1                                   # the zero overhead and the zero surface: 0/0
    np.testing.assert_allclose(dist.numpy()[fin], d64[fin], rtol=0, atol=1e-6)
    np.testing.assert_allclose(exp.distance[fin], d64[fin], rtol=0, atol=4 * 2.0 ** -23)      # the fp32 restatement: a few ulp of 2
    assert np.array_equal(np.isnan(exp.distance), ~fin)
    # window norm squares against the oracle's materialised crop, surface norm squares directly
    crop = O.crop_overhead(to, torch.from_numpy(exp.orientation), We).numpy()
    assert np.array_equal((crop ** 2).sum(axis=(2, 3, 4)), np.take_along_axis(base.n2w, exp.orientation, 1))
    assert np.array_equal(base.n2s, (su ** 2).sum(axis=(1, 2)))
    # a sub-block, the one-shift form and the scaled flavour are the same numbers
    sub = R.build(ov, su, rows_o=[0, 8], rows_s=[3, 10, 1])
    assert np.array_equal(sub.sc, base.sc[[0, 8]][:, [3, 10, 1]]) and np.array_equal(sub.n2s, base.n2s[[3, 10, 1]])
    shift = R.make_shifts(Bo, Bs, We, 1)
    one = R.build(ov, su, shift=shift)
    a, b = R.decide(base, shift=shift), R.decide(one, shift=shift)
    assert np.array_equal(a.orientation, np.broadcast_to(shift & 63, (Bo, Bs))) and not R.differs(a, b).any()
    m = np.array([1 << int(k) for k in (shift & 63)], dtype=np.uint64)
    assert not R.differs(a, R.decide(base, mask=m)).any()
    o32, s32 = R.as_f32(ov, su, 'dyadic')
    dy = R.build(o32.astype(np.float64).reshape(Bo, 64, 64), s32.astype(np.float64).reshape(Bs, 64, We))
    fl = R.flavoured(base, 'dyadic')
    assert np.array_equal(dy.sc, fl.sc) and np.array_equal(dy.n2w, fl.n2w) and np.array_equal(dy.n2s, fl.n2s)
    assert np.array_equal(R.decide(dy).distance.view(np.uint32), exp.distance.view(np.uint32))     # the scales cancel exactly


@pytest.mark.parametrize('flavour', sorted(R.FLAVOURS))
def test_exactness_premise_fp32_in_any_order_is_float64(flavour):
    """The scores and norm squares of one case summed in fp32 forwards, backwards and pairwise carry the float64 bits."""
    Bo, Bs, We = 70, 5, 63
    ov, su = R.make_data(Bo, Bs, We)
    base = R.flavoured(R.build(ov, su), flavour)
    o32, s32 = R.as_f32(ov, su, flavour)
    o32, s32 = o32.reshape(Bo, 64, 64), s32.reshape(Bs, 64, We)
    rows = [0, 2, 4, Bo - 1]
    prod = np.stack([o32[rows][:, None, :, (np.arange(We) + sh) % 64] * s32[None] for sh in range(64)], axis=2)
    prod = prod.reshape(len(rows), Bs, 64, 64 * We)                       # fp32 products [o,s,shift,K]
    assert prod.dtype == np.float32

    def pairwise(x):
        while x.shape[-1] > 1:
            if x.shape[-1] % 2:
                x = np.concatenate((x, np.zeros_like(x[..., :1])), axis=-1)
            x = x[..., 0::2] + x[..., 1::2]
        return x[..., 0]

    want = base.sc[rows]
    for name, got in (('forward', np.cumsum(prod, axis=-1, dtype=np.float32)[..., -1]),
                      ('reversed', np.cumsum(prod[..., ::-1], axis=-1, dtype=np.float32)[..., -1]), ('pairwise', pairwise(prod))):
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), name
    sq = np.ascontiguousarray((o32 * o32)[:, :, :We]).reshape(Bo, -1)      # the window at shift 0
    for got in (np.cumsum(sq, axis=-1, dtype=np.float32)[:, -1], np.cumsum(sq[:, ::-1], axis=-1, dtype=np.float32)[:, -1], pairwise(sq)):
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), base.n2w[:, 0])
    ssq = (s32 * s32).reshape(Bs, -1)
    assert np.array_equal(pairwise(ssq).astype(np.float64), base.n2s)
    assert np.abs(base.sc).max() <= 65536 * 4 and base.n2w.max() < 2 ** 24 and base.n2s.max() < 2 ** 24 * 2 ** 10


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_every_case_holds_the_planted_ties_and_sees_every_wrong_variant(shape):
    Bo, Bs, We = shape
    ov, su, ro, rs = _probe(Bo, Bs, We)
    base = R.build(ov, su, rows_o=ro, rows_s=rs)
    cross, within, _ = R.tie_stats(base)
    assert cross > 0 and within > 0, (cross, within)
    exp = R.decide(base)
    if Bs > 4:                                                             # the planted rows do what they were planted for
        o0 = int(np.nonzero(ro == 0)[0][0])
        assert [int(exp.orientation[o0, int(np.nonzero(rs == s)[0][0])]) for s in (0, 1, 2)] == [63, 0, 32]
        z = int(np.nonzero(rs == 3)[0][0])
        assert np.all(exp.orientation[:, z] == 0) and np.all(exp.score[:, z] == 0) and np.all(np.isnan(exp.distance[:, z]))
    if Bo >= 3:
        z = int(np.nonzero(ro == 1)[0][0])
        assert np.all(exp.orientation[z] == 0) and np.all(np.isnan(exp.distance[z]))
    assert exp.orientation[-1, -1] == (31 if Bo > 1 else 15) and exp.score[-1, -1] == base.n2s[-1] > 0
    assert np.all(exp.orientation[-1] < 32) and np.all(R.decide(base, variant='second_tile_wins').orientation[-1] >= 32)
    wrong = {name: R.build(ov, su, variant=name, rows_o=ro, rows_s=rs) for name in R.VARIANTS}
    for name in R.VARIANTS:
        if R.applies(name, Bo, Bs, We):
            _assert_seen(name, base, wrong[name], where='unmasked')
    for ms in R.MASK_SETS:
        mask = R.make_mask(Bo, Bs, We, ms)[rs]
        if np.any(mask):                                                   # (the one query of a 1 x 1 case has the word 0 in 'mixed')
            assert R.tie_stats(base, mask)[2] > 0, ms
        for name in R.VARIANTS:
            if R.applies(name, Bo, Bs, We, mask=mask):
                _assert_seen(name, base, wrong[name], mask=mask, where='under mask set ' + ms)
    if Bs > 1:
        mixed = R.make_mask(Bo, Bs, We, 'mixed')
        assert np.any(mixed == 0) and np.any(mixed == R.ALL) and np.any(mixed == R.UPPER)
        cross_m, within_m, _ = R.tie_stats(base, mixed[rs])
        assert cross_m > 0 and within_m > 0


@pytest.mark.parametrize('fixed', R.FIXED + R.FIXED_BIG, ids=_ids)
def test_every_fixed_case_sees_every_wrong_variant(fixed):
    Bo, Bs, We, lists = fixed
    ov, su, ro, rs = _probe(Bo, Bs, We)
    for which in lists:
        full = R.make_shifts(Bo, Bs, We, which)
        # the probe rows and one query of every shift group
        rows = np.array(sorted(set(rs.tolist()) | set(int(np.nonzero((full & 63) == k)[0][0]) for k in np.unique(full & 63))))
        shift = full[rows]
        base = R.build(ov, su, rows_o=ro, rows_s=rows, shift=full)
        for name in R.VARIANTS:
            if R.applies(name, Bo, Bs, We, shift=shift):
                wrong = R.build(ov, su, variant=name, rows_o=ro, rows_s=rows, shift=full)
                _assert_seen(name, base, wrong, shift=shift, where='fixed list %d' % which)
        assert R.applies('fixed_shift_raw', Bo, Bs, We, shift=shift) and not R.applies('last_index_wins', Bo, Bs, We, shift=shift)


def test_rank_counting_reference_on_ties_and_nans():
    D = np.array([[1, 2, np.nan, 1], [1, np.nan, 3, 0], [0.5, 2, 3, 1], [1, 1, 3, np.nan]], dtype=np.float32)
    assert R.rank_count(D).tolist() == [4, 0, 3, 0]
    assert R.rank_count(D, 1).tolist() == [4, 3, 3, 0]
    assert R.rank_count_thresh(D, np.array([1, 2, np.nan, 0.5], dtype=np.float32)).tolist() == [4, 3, 0, 1]
    c, band = R.rank_count_band(D, np.array([1, 2, 3, 1], dtype=np.float32), 0.0)
    assert c.tolist() == [1, 1, 0, 1] and band == [(0, 0), (0, 1), (0, 3), (1, 0), (1, 2), (2, 1), (2, 2), (2, 3), (3, 0), (3, 2)]
