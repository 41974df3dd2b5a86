"""The match forward against the float64 reference of tests/match_exact_ref.py on data on which it is exact: EVERY pair of
every case is compared -- torch.equal on orientation, equality on score, bit equality on distance with NaN at the same places
-- exact ties included; no safe mask, no skipped pair. tests/test_match_exact_ref.py proves on the CPU that each case sees each
kernel mistake listed there.

Kernel forms. witw_match_fwd does not note the instantiation it launches (ops.last_kernel_variant() names the fixed form only),
so the form of an all-pairs case is derived from the dispatch in match_fwd_launch, restated as R.dispatch() and printed per case:
  match_kernel<1,1>              (1,1,64) (3,200,1) (70,5,63)
  match_kernel_nsplit<16|32|64>  (100,77,w), w = 12 | 17 | 33, 64
  match_kernel<1,2>              (258,129,20), and (510,129,w) under WITW_MATCH_GENERIC=1: 2 * 128 = 256 workgroups, below the 512
                                 that match_kernel<2,2> wants
  match_kernel_w64               (510,129,64) (510,129,63)
  match_kernel_rows<4|2|1>       (510,129,w), w = 1, 7, 16 | 17, 32 | 33, 62
  match_kernel<2,2>              (1021,129,33) (1021,129,64) under WITW_MATCH_GENERIC=1 (2 * 256 = 512 workgroups)
each in its unmasked and its masked instantiation (mask sets R.MASK_SETS: windows of 1, 2, 5 and 33 shifts, and words of 0, all
ones, the upper half only, two quarters only, random and sparse words).

Fixed form (ops.match_fwd_fixed; the kernel from ops.last_kernel_variant(), the supertiles from the table the launch leaves in its
workspace). On 256 compute units the shapes of R.FIXED cut their shift groups (sizes 1, 31, 32, 33, 65 among them, shifts
outside 0..63 among them) into 32-row supertiles: fixed_tile<16,1> at (3,200,1), <32,1> at (258,129,20), <64,1> at (510,129,64) and
(510,129,63). (1921,3969,w) for w = 12 | 17 | 33 makes cdiv(Bs,128) * cdiv(Bo,128) = 512 workgroups and so 128-row supertiles,
whose tails reach fixed_tile<16|32|64, 1..4>: every instantiation. 64-row supertiles (sm = 2 in the launcher) are not reached;
they instantiate nothing further.

Pair lists: ops.match_pairs returns orientation and distance (no score), on both settings of witw_match_pairs_impl.

sqrtf. The distance is expected bit for bit, which needs the workspace norms to be the correctly rounded roots: the first
assertion of every all-pairs and fixed case compares all of wn [Bo,64] and sn [Bs] with np.sqrt in float32. Observed on the
MI355X: equal on every entry of every case, so bit equality of the distance stands.

Rank counting runs on these distance matrices without the all-zero overhead row and surface column: how witw_rank_count* treat
a NaN is no documented contract."""
import functools

import numpy as np
import pytest
import torch

from tests import match_exact_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ref(Bo, Bs, We):
    """data and full reference of a shape, computed once per session and never written to"""
    ov, su = R.make_data(Bo, Bs, We)
    base = R.build(ov, su)
    for a in (ov, su) + tuple(base[:3]):
        a.setflags(write=False)
    return ov, su, base


@functools.lru_cache(maxsize=None)
def _ref_fixed(Bo, Bs, We, which):
    ov, su = R.make_data(Bo, Bs, We)
    shift = R.make_shifts(Bo, Bs, We, which)
    return ov, su, shift, R.build(ov, su, shift=shift)


def _cuda(ov, su, flavour):
    o32, s32 = R.as_f32(ov, su, flavour)
    return torch.from_numpy(o32).cuda(), torch.from_numpy(s32).cuda()


def _words(mask):
    return torch.from_numpy(mask.view(np.int64).copy()).cuda()


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), '%s: NaN at other places' % what
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), '%s: %d of %d differ, first at %s: %r != %r' % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def _check(ori, dist, score, exp, what):
    if ori is not None:
        assert ori.dtype == torch.int64
        assert torch.equal(ori.cpu(), torch.from_numpy(exp.orientation)), '%s: orientation, %d pairs differ' % (
            what, int((ori.cpu().numpy() != exp.orientation).sum()))
    if score is not None:
        got = score.cpu().numpy().astype(np.float64)
        assert np.array_equal(got, exp.score), '%s: score, %d pairs differ' % (what, int((got != exp.score).sum()))
    _same_bits(dist.cpu().numpy(), exp.distance, what + ': distance')


def _check_norms(ws, base, Bo, Bs, what):
    wn, sn = R.norms_f32(base)
    w = ws.cpu().numpy()
    _same_bits(w[:Bo * 64].reshape(Bo, 64), wn, what + ': wn against np.sqrt in float32')
    _same_bits(w[Bo * 64:Bo * 64 + Bs], sn, what + ': sn against np.sqrt in float32')


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_all_pairs_forward_every_pair_unmasked_and_masked(case, monkeypatch):
    from witw_amd import ops
    Bo, Bs, We = case.Bo, case.Bs, case.We
    ov, su, base0 = _ref(Bo, Bs, We)
    if case.generic:
        monkeypatch.setenv('WITW_MATCH_GENERIC', '1')
    print('%s -> %s and its masked instantiation (from the dispatch)' % (R.case_id(case), case.form))
    for flavour in R.FLAVOURS:
        base = R.flavoured(base0, flavour)
        o, s = _cuda(ov, su, flavour)
        what = '%s %s' % (R.case_id(case), flavour)
        ori, dist, score, ws = ops.match_fwd(o, s, want_score=True, want_workspace=True)
        _check_norms(ws, base, Bo, Bs, what)
        _check(ori, dist, score, R.decide(base), what + ' unmasked')
        for ms in R.MASK_SETS:
            mask = R.make_mask(Bo, Bs, We, ms)
            ori, dist, score, ws = ops.match_fwd(o, s, want_score=True, want_workspace=True, shift_mask=_words(mask))
            _check(ori, dist, score, R.decide(base, mask=mask), what + ' mask set ' + ms)
        _check_norms(ws, base, Bo, Bs, what + ' masked')


@pytest.mark.parametrize('fixed', R.FIXED + R.FIXED_BIG, ids=lambda f: '%dx%dx%d' % f[:3])
def test_fixed_shift_forward_every_pair(fixed):
    from witw_amd import ops
    Bo, Bs, We, lists = fixed
    big = fixed in R.FIXED_BIG
    wp = 16 if We <= 16 else 32 if We <= 32 else 64
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for which in lists:
        if big:
            ov, su, shift, base0 = _ref_fixed(Bo, Bs, We, which)
        else:
            ov, su, base0 = _ref(Bo, Bs, We)
            shift = R.make_shifts(Bo, Bs, We, which)
        for flavour in R.FLAVOURS:
            base = R.flavoured(base0, flavour)
            o, s = _cuda(ov, su, flavour)
            what = 'fixed %dx%dx%d list %d %s' % (Bo, Bs, We, which, flavour)
            ori, dist, score, ws = ops.match_fwd_fixed(o, s, torch.from_numpy(shift).cuda(), want_score=True, want_workspace=True)
            assert ops.last_kernel_variant() == 'match_fixed_kernel<%d>' % wp
            _check_norms(ws, base, Bo, Bs, what)
            _check(ori, dist, score, R.decide(base, shift=shift), what)
            # the supertiles the launch made, from its own table behind the norms: [0] their number, [2 + 2t] rows << 8 | shift
            tab = ws.cpu().numpy()[Bo * 64 + Bs:].view(np.int32)
            rows = tab[2:2 + 2 * tab[0]:2] >> 8
            mts = sorted(set(((rows + 31) // 32).tolist()))
            print('%s: match_fixed_kernel<%d>, %d supertiles, fixed_tile<%d,MT> for MT in %s' % (what, wp, tab[0], wp, mts))
            assert mts == R.fixed_tiles(shift, R.fixed_rows_per_tile(Bo, Bs, cus))
            if cus == 256:
                assert mts == ([1, 2, 3, 4] if big else [1])
        dist2 = ops.match_fwd_fixed(o, s, torch.from_numpy(shift).cuda(), want_orientation=False)[1]      # the lean call form
        _same_bits(dist2.cpu().numpy(), dist.cpu().numpy(), 'fixed without orientation')


def _pair_list(Bo, Bs, n):
    """n pairs (n % 4 == 3): the corners and the planted rows first, repeats, random pairs behind them"""
    g = np.random.Generator(np.random.Philox(key=[Bo, Bs + 7]))
    po, ps = g.integers(0, Bo, size=n), g.integers(0, Bs, size=n)
    head = [(Bo - 1, Bs - 1), (Bo - 1, Bs - 1), (0, Bs - 1), (Bo - 1, 0), (0, 0), (0, min(1, Bs - 1)), (0, min(2, Bs - 1)),
            (min(1, Bo - 1), min(3, Bs - 1)), (min(2, Bo - 1), Bs - 1), (min(2, Bo - 1), Bs - 1)]
    for i, (a, b) in enumerate(head[:n - 1]):
        po[i], ps[i] = a, b
    po[-1], ps[-1] = po[0], ps[0]
    return po.astype(np.int32), ps.astype(np.int32)


@pytest.mark.parametrize('shape', [(3, 200, 1), (100, 77, 33), (100, 77, 64)], ids=lambda v: '%dx%dx%d' % v)
def test_pair_lists_against_the_reference_on_both_kernels(shape):
    from witw_amd import _lib, ops
    Bo, Bs, We = shape
    ov, su, base0 = _ref(Bo, Bs, We)
    lib = _lib.load()
    prev = lib.witw_match_pairs_impl(-1)
    try:
        for flavour in R.FLAVOURS:
            base = R.flavoured(base0, flavour)
            o, s = _cuda(ov, su, flavour)
            ws = ops.match_fwd(o, s, want_workspace=True)[3]
            wn, sn = ws[:Bo * 64], ws[Bo * 64:Bo * 64 + Bs]
            for n in (203, 7):
                po, ps = _pair_list(Bo, Bs, n)
                assert n % 4 == 3 and (po[0], ps[0]) == (Bo - 1, Bs - 1) == (po[-1], ps[-1])
                for ms in (None, 'mixed', 'win33', 'win1'):
                    mask = None if ms is None else R.make_mask(Bo, Bs, We, ms)
                    exp = R.decide(base, mask=mask)
                    want = R.Expected(exp.orientation[po, ps], exp.score[po, ps], exp.distance[po, ps])
                    for impl in (0, 1):
                        lib.witw_match_pairs_impl(impl)
                        ori, dist = ops.match_pairs(o, s, wn, sn, torch.from_numpy(po).cuda(), torch.from_numpy(ps).cuda(),
                                                    shift_mask=None if mask is None else _words(mask))
                        _check(ori, dist, None, want, 'pairs %s %s n=%d mask %s impl %d' % (shape, flavour, n, ms, impl))
    finally:
        lib.witw_match_pairs_impl(prev)


@pytest.mark.parametrize('shape', [(1, 1, 64), (3, 200, 1), (70, 5, 63), (100, 77, 17)], ids=lambda v: '%dx%dx%d' % v)
def test_unfused_chain_crop_is_the_gather_and_l2_distance_the_fused_bits(shape):
    from witw_amd import ops
    Bo, Bs, We = shape
    ov, su, base0 = _ref(Bo, Bs, We)
    for flavour in R.FLAVOURS:
        base = R.flavoured(base0, flavour)
        o, s = _cuda(ov, su, flavour)
        o64 = R.as_f32(ov, su, flavour)[0].astype(np.float64).reshape(Bo, 64, 64)
        for ms in (None, 'mixed'):
            exp = R.decide(base, mask=None if ms is None else R.make_mask(Bo, Bs, We, ms))
            crop = ops.crop_overhead(o, torch.from_numpy(exp.orientation).cuda(), We)
            assert crop.shape == (Bo, Bs, 16, 4, We)
            col = (np.arange(We)[None, None, :] + exp.orientation[:, :, None]) % 64                       # [Bo,Bs,We]
            want = o64[np.arange(Bo)[:, None, None, None], np.arange(64)[None, None, :, None], col[:, :, None, :]]
            assert np.array_equal(crop.cpu().numpy().reshape(Bo, Bs, 64, We).astype(np.float64), want)
            _same_bits(ops.l2_distance(crop, s).cpu().numpy(), exp.distance, 'l2_distance %s %s mask %s' % (shape, flavour, ms))


@pytest.mark.parametrize('shape,ms', [((3, 200, 1), None), ((258, 129, 20), None), ((100, 77, 64), 'mixed'), ((510, 129, 1), 'win5')],
                         ids=lambda v: 'x'.join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_rank_counting_on_exact_distance_matrices(shape, ms):
    """The counters compare with <=, and these matrices hold many exactly equal distances (tied scores over equal norms, the
    crops at distance 0, periodic rows): a strict comparison, or one off by an ulp, shows here. Without the NaN row / column."""
    from witw_amd import ops
    Bo, Bs, We = shape
    _ov, _su, base = _ref(Bo, Bs, We)
    D = R.decide(base, mask=None if ms is None else R.make_mask(Bo, Bs, We, ms)).distance
    D = np.ascontiguousarray(np.delete(np.delete(D, 1, axis=0), 3, axis=1))
    assert not np.isnan(D).any()
    n_o, n_q = D.shape
    vals, counts = np.unique(D, return_counts=True)
    assert counts.max() > 1 and len(vals) < D.size                           # exact ties are there
    Dg = torch.from_numpy(D).cuda()
    for off in (0, 1, n_o - n_q, -2):
        assert np.array_equal(ops.rank_count(Dg, off).cpu().numpy(), R.rank_count(D, off)), off
    g = np.random.Generator(np.random.Philox(key=[n_o, n_q]))
    thr = D[g.integers(0, n_o, size=n_q), np.arange(n_q)].copy()             # thresholds that ARE entries: <= decides
    thr[::5] = np.nextafter(thr[::5], np.float32(-np.inf))                   # ... and one ulp below
    thr[1::7] = np.float32(np.inf)
    thr[2::7] = np.float32(-1)
    assert np.array_equal(ops.rank_count_thresh(Dg, torch.from_numpy(thr).cuda()).cpu().numpy(), R.rank_count_thresh(D, thr))
    for eps in (0.0, 2.0 ** -12):
        c, po, ps = ops.rank_count_band(Dg, torch.from_numpy(thr).cuda(), eps)
        want_c, want_band = R.rank_count_band(D, thr, eps)
        assert np.array_equal(c.cpu().numpy(), want_c), eps
        assert sorted(zip(po.cpu().tolist(), ps.cpu().tolist())) == want_band, eps
