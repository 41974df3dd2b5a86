"""Orientation profiles on the GPU: witw_match_profile, witw_match_pairs_profile and witw_profile_hypotheses against exact data,
against the forward they promise to carry the bits of, against the oracle and against the numpy restatement of the rule; the
memory contract of the new wrappers; the public surface of cvig_fov and the heat-map CSV.

Forms. witw_match_profile has the profile epilogue on the generic kernel only (tests/match_profile_ref.dispatch):
  match_kernel<1,1,false,true>   (1,1,64) (3,200,1) (70,5,63), and (100,77,33)
  match_kernel<1,2,false,true>   (258,129,20), and (510,129,64) (510,129,17)
  match_kernel<2,2,false,true>   (1021,129,33)
The shapes after "and" reach a forward form WITHOUT a profile epilogue (n-split, w64, rows): there the chain-identity contract
is the whole of the claim -- another kernel's accumulators must hold the same bits."""
import functools

import numpy as np
import pytest
import torch

from tests import match_exact_ref as R
from tests import match_profile_ref as P
from tests.mem_arena import Arena, ArenaTorch

pytestmark = pytest.mark.gpu

EXACT = [(1, 1, 64), (3, 200, 1), (70, 5, 63), (258, 129, 20), (1021, 129, 33)]
OTHER_FORMS = [(100, 77, 33), (510, 129, 64), (510, 129, 17)]      # forward: n-split, w64, rows
sid = lambda s: '%dx%dx%d' % s
# what ops.match_fwd runs on each shape (tests/match_exact_ref.dispatch): the forms the profile's bits are compared with
FORWARD_FORM = {(1, 1, 64): 'match_kernel<1,1,false>', (3, 200, 1): 'match_kernel<1,1,false>', (70, 5, 63): 'match_kernel<1,1,false>',
                (258, 129, 20): 'match_kernel<1,2,false>', (1021, 129, 33): 'match_kernel_rows<1,false>',
                (100, 77, 33): 'match_kernel_nsplit<64,false>', (510, 129, 64): 'match_kernel_w64<false>',
                (510, 129, 17): 'match_kernel_rows<2,false>'}


@functools.lru_cache(maxsize=None)
def _ref(Bo, Bs, We):
    ov, su = R.make_data(Bo, Bs, We)
    base = R.build(ov, su)
    for a in (ov, su) + tuple(base[:3]):
        a.setflags(write=False)
    return ov, su, base


@functools.lru_cache(maxsize=None)
def _normal(Bo, Bs, We):
    """random normal embeddings of a shape (CPU, read-only by convention)"""
    g = torch.Generator().manual_seed(1000 * Bo + 10 * Bs + We)
    return torch.randn((Bo, 16, 4, 64), generator=g), torch.randn((Bs, 16, 4, We), generator=g)


def _variant():
    from witw_amd import ops
    return ops.last_kernel_variant()


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), '%s: NaN at other places' % what
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), '%s: %d of %d differ, first at %s: %r != %r' % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


# ----------------------------------------------------------------------------- 1. exact data
@pytest.mark.parametrize('shape', EXACT, ids=sid)
def test_profile_on_exact_data_every_pair_every_shift(shape):
    from witw_amd import match_profile
    Bo, Bs, We = shape
    ov, su, base0 = _ref(Bo, Bs, We)
    for flavour in R.FLAVOURS:
        base = R.flavoured(base0, flavour)
        o32, s32 = R.as_f32(ov, su, flavour)
        scores, dists, ws = match_profile.match_profile(torch.from_numpy(o32).cuda(), torch.from_numpy(s32).cuda(),
                                                        want_workspace=True)
        assert _variant() == P.dispatch(Bo, Bs, We), (_variant(), P.dispatch(Bo, Bs, We))
        what = '%s %s' % (sid(shape), flavour)
        got = scores.cpu().numpy()
        assert got.shape == (Bo, Bs, 64) and got.dtype == np.float32
        assert np.array_equal(got.astype(np.float64), base.sc), '%s: score_all, %d entries differ' % (
            what, int((got.astype(np.float64) != base.sc).sum()))
        wn, sn = R.norms_f32(base)
        w = ws.cpu().numpy()
        _same_bits(w[:Bo * 64].reshape(Bo, 64), wn, what + ': wn')
        _same_bits(w[Bo * 64:Bo * 64 + Bs], sn, what + ': sn')
        want = P.distance_all_f32(base.sc, base.n2w, base.n2s)
        if Bs > 4:
            assert np.isnan(want[:, 3]).all()                    # the all-zero surface row: 0 / 0 at every shift
        _same_bits(dists.cpu().numpy(), want, what + ': distance_all')


# ----------------------------------------------------------------------------- 2. the bits of the forward
@pytest.mark.parametrize('shape', EXACT + OTHER_FORMS, ids=sid)
def test_profile_carries_the_bits_of_the_forward(shape):
    from witw_amd import match_profile, ops
    Bo, Bs, We = shape
    assert R.dispatch(Bo, Bs, We) == FORWARD_FORM[shape]
    ov, su = (t.cuda() for t in _normal(Bo, Bs, We))
    ori, dist, score, ws = ops.match_fwd(ov, su, want_score=True, want_workspace=True)
    scores, dists, ws_p = match_profile.match_profile(ov, su, want_workspace=True)
    assert _variant() == P.dispatch(Bo, Bs, We)
    assert torch.equal(ws.view(torch.int32), ws_p.view(torch.int32)), 'the workspace is not the forward\'s'
    sc = scores.cpu().numpy()
    first = sc.argmax(axis=-1)                                   # numpy: the first maximal index
    assert np.array_equal(first, ori.cpu().numpy()), '%d orientations differ' % int((first != ori.cpu().numpy()).sum())
    take = lambda a: np.take_along_axis(a, first[:, :, None], 2)[:, :, 0]
    _same_bits(take(sc), score.cpu().numpy(), 'score_all at the orientation')
    _same_bits(take(dists.cpu().numpy()), dist.cpu().numpy(), 'distance_all at the orientation')


# ----------------------------------------------------------------------------- 3. the oracle, with the derived bound
@pytest.mark.parametrize('shape', [(70, 5, 63), (100, 77, 12)], ids=sid)
def test_profile_scores_against_the_oracle_within_the_derived_bound(shape):
    from oracle import cvig_fov_oracle as O
    from witw_amd import match_profile
    Bo, Bs, We = shape
    ov, su = _normal(Bo, Bs, We)
    want = O.correlation_scores(ov.double(), su.double()).numpy()
    bound = P.score_bound(ov.double().numpy().reshape(Bo, 64, 64), su.double().numpy().reshape(Bs, 64, We), We)
    got = match_profile.match_profile(ov.cuda(), su.cuda(), want_distances=False)[0].cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    print('%s: max |error| / bound = %.3g' % (sid(shape), float((err / bound).max())))
    assert (err <= bound).all(), '%d entries beyond (64 We + 2) 2^-24 sum|ov su|, worst ratio %.3g' % (
        int((err > bound).sum()), float((err / bound).max()))


# ----------------------------------------------------------------------------- 4. pair lists
@pytest.mark.parametrize('shape', [(37, 29, 64), (37, 29, 33)], ids=sid)
def test_pair_list_rows_are_the_dense_rows(shape):
    from witw_amd import cvig_fov, match_profile
    Bo, Bs, We = shape
    ov, su = (t.cuda() for t in _normal(Bo, Bs, We))
    scores, dists, ws = match_profile.match_profile(ov, su, want_workspace=True)
    g = torch.Generator().manual_seed(5)
    po = torch.cat((torch.tensor([0, Bo - 1, 7, 7]), torch.randint(0, Bo, (39,), generator=g))).to(torch.int32)
    ps = torch.cat((torch.tensor([0, Bs - 1, 3, 3]), torch.randint(0, Bs, (39,), generator=g))).to(torch.int32)
    assert po.numel() % 4 == 3
    wn, sn = ws[:Bo * 64].clone(), ws[Bo * 64:Bo * 64 + Bs].clone()
    psc, pd = match_profile.match_pairs_profile(ov, su, wn, sn, po.cuda(), ps.cuda())
    assert psc.shape == pd.shape == (43, 64)
    _same_bits(psc.cpu().numpy(), scores[po.long(), ps.long()].cpu().numpy(), 'pair scores')
    _same_bits(pd.cpu().numpy(), dists[po.long(), ps.long()].cpu().numpy(), 'pair distances')
    only_d = match_profile.match_pairs_profile(ov, su, wn, sn, po.cuda(), ps.cuda(), want_scores=False)
    assert only_d[0] is None and torch.equal(only_d[1].view(torch.int32), pd.view(torch.int32))
    # the public surface: int64 indices on the host, norms found by itself, masks gathered per pair
    csc, cd = cvig_fov.orientation_profile(ov, su, pairs=(po.long(), ps.long()))
    assert torch.equal(csc.view(torch.int32), psc.view(torch.int32)) and torch.equal(cd.view(torch.int32), pd.view(torch.int32))
    mask = cvig_fov.orientation_mask(torch.linspace(-170., 170., Bs), 40.)
    dense = cvig_fov.orientation_hypotheses(ov, su, n=3, shift_mask=mask)
    listed = cvig_fov.orientation_hypotheses(ov, su, n=3, shift_mask=mask, pairs=(po, ps))
    for d, l in zip(dense, listed):
        assert l.shape == (43, 3)
        a, b = d[po.long(), ps.long()].cpu().numpy(), l.cpu().numpy()
        assert np.array_equal(a, b, equal_nan=True)


# ----------------------------------------------------------------------------- 5. hypotheses
def _mask_settings(Bs):
    from witw_amd import cvig_fov
    g = np.random.Generator(np.random.Philox(key=[11, Bs]))
    return {
        'none': None,
        'per-query': cvig_fov.orientation_mask(g.uniform(-180., 180., Bs), g.uniform(0., 90., Bs)),
        'shared': cvig_fov.orientation_mask(-170., 25.),                                     # one word, wraps round the ring
        'one-bit': torch.from_numpy((np.uint64(1) << g.integers(0, 64, Bs).astype(np.uint64)).view(np.int64).copy()),
    }


@pytest.mark.parametrize('shape', [(70, 5, 63), (100, 77, 33)], ids=sid)
def test_hypotheses_kernel_equals_the_restatement(shape):
    from witw_amd import match_profile, ops
    Bo, Bs, We = shape
    ov, su = (t.cuda() for t in _normal(Bo, Bs, We))
    scores = match_profile.match_profile(ov, su, want_distances=False)[0]
    sc = scores.cpu().numpy()
    for name, words in _mask_settings(Bs).items():
        per_query = None if words is None else words.expand(Bs).contiguous()
        kw = {} if words is None else {'shift_mask': per_query.cuda()}
        ori = ops.match_fwd(ov, su, **kw)[0].cpu().numpy()
        ref_words = None if words is None else words.numpy()
        for n_hyp in (1, 3, 64):
            for min_sep in (0, 4, 31):
                got = match_profile.profile_hypotheses(scores, n_hyp, min_sep, None if words is None else words.cuda())
                assert got.shape == (Bo, Bs, n_hyp) and got.dtype == torch.int64
                got = got.cpu().numpy()
                want = P.hypotheses(sc, n_hyp, min_sep, ref_words)
                assert np.array_equal(got, want), '%s n_hyp=%d min_sep=%d: %d entries differ' % (
                    name, n_hyp, min_sep, int((got != want).sum()))
                assert np.array_equal(got[:, :, 0], ori), '%s: hypothesis 1 is not match_fwd\'s orientation' % name
        if name == 'one-bit':
            assert (got[:, :, 1:] == -1).all()


def test_public_hypotheses_columns_and_sweep_scores():
    from witw_amd import cvig_fov
    Bo, Bs, We = 70, 5, 63
    ov, su = (t.cuda() for t in _normal(Bo, Bs, We))
    mask = cvig_fov.orientation_mask(torch.tensor([0., 90., -90., 180., 45.]), torch.tensor([180., 30., 5., 0., 60.]))
    shift, deg, dist, score = cvig_fov.orientation_hypotheses(ov, su, n=4, min_separation_deg=22.5, shift_mask=mask, refine=False)
    ori, d0 = cvig_fov.match(ov, su, shift_mask=mask)
    assert torch.equal(shift[..., 0], ori) and torch.equal(dist[..., 0].contiguous().view(torch.int32), d0.view(torch.int32))
    none = shift < 0
    assert bool(none[:, 3, 1:].all()) and not bool(none[:, 0].any())             # a one-bit word; no prior
    assert bool(torch.isnan(deg[none]).all() and torch.isnan(dist[none]).all() and torch.isnan(score[none]).all())
    assert torch.equal(deg[~none], shift[~none].double() * 5.625 - 180.)
    assert torch.equal(score[~none], torch.exp(10. * (1. - dist[~none])))
    sc_all, d_all = cvig_fov.orientation_profile(ov, su)
    assert torch.equal(dist[~none], torch.gather(d_all, -1, shift.clamp(min=0))[~none])
    # refine moves the degrees by at most half a bin and never the shift
    shift_r, deg_r, dist_r, _s = cvig_fov.orientation_hypotheses(ov, su, n=4, shift_mask=mask)
    assert torch.equal(shift_r, shift) and torch.equal(dist_r.view(torch.int32), dist.view(torch.int32))
    delta = cvig_fov.refine_orientation(sc_all.cpu(), shift.cpu())
    assert torch.equal(deg_r.cpu()[~none.cpu()], ((shift.cpu().double() + delta) * 5.625 - 180.)[~none.cpu()])
    assert float((deg_r - deg)[~none].abs().max()) <= 2.8125 and float(delta.abs().max()) > 0
    # sweep_scores: 1 = what it was; M > 1 = a 4th item whose first column is the first three
    three = cvig_fov.sweep_scores(ov, su, shift_mask=mask)
    same = cvig_fov.sweep_scores(ov, su, shift_mask=mask, hypotheses=1)
    four = cvig_fov.sweep_scores(ov, su, shift_mask=mask, hypotheses=4, refine=False)
    assert len(three) == len(same) == 3 and len(four) == 4
    for a, b, c in zip(three, same, four):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(four[3][0], shift) and torch.equal(four[3][1][..., 0], three[0].double())
    assert torch.equal(four[3][2][..., 0], three[1]) and torch.equal(four[3][3][..., 0], three[2])


# ----------------------------------------------------------------------------- 6. memory contract
def _contract_cases():
    from witw_amd import match_profile as M

    def dense(p, we, **kw):
        ov, su = _normal(37, 29, we)
        return M.match_profile(p(ov), p(su), **kw)

    def listed(p, we, **kw):
        ov, su = (t.cuda() for t in _normal(37, 29, we))
        ws = M.match_profile(ov, su, want_scores=False, want_workspace=True)[2]
        g = torch.Generator().manual_seed(6)
        po, ps = torch.randint(0, 37, (51,), generator=g, dtype=torch.int32), torch.randint(0, 29, (51,), generator=g, dtype=torch.int32)
        return M.match_pairs_profile(p(ov), p(su), p(ws[:37 * 64].clone()), p(ws[37 * 64:37 * 64 + 29].clone()), p(po), p(ps), **kw)

    def hyp(p, n_hyp, min_sep, words):
        sc = torch.randn((37, 29, 64), generator=torch.Generator().manual_seed(7))
        return M.profile_hypotheses(p(sc), n_hyp, min_sep, None if words is None else p(words))

    words = torch.from_numpy(np.random.Generator(np.random.Philox(key=[6, 1])).integers(-2 ** 63, 2 ** 63, 29, dtype=np.int64))
    words[0] = 0
    cases = []
    for we in (64, 33, 12):
        cases.append(('match_profile-We%d' % we, lambda p, we=we: dense(p, we, want_workspace=True)))
        cases.append(('match_pairs_profile-We%d' % we, lambda p, we=we: listed(p, we)))
    cases.append(('match_profile-scores-only', lambda p: dense(p, 33, want_distances=False)))
    cases.append(('match_profile-distances-only', lambda p: dense(p, 33, want_scores=False)))
    cases.append(('match_pairs_profile-scores-only', lambda p: listed(p, 33, want_distances=False)))
    cases.append(('match_pairs_profile-distances-only', lambda p: listed(p, 33, want_scores=False)))
    cases.append(('profile_hypotheses-3-4', lambda p: hyp(p, 3, 4, None)))
    cases.append(('profile_hypotheses-64-0-words', lambda p: hyp(p, 64, 0, words)))
    cases.append(('profile_hypotheses-1-31-one-word', lambda p: hyp(p, 1, 31, words[1:2].clone())))
    return cases


def _flat(r):
    return [t for t in (r if isinstance(r, (tuple, list)) else (r,)) if t is not None]


@pytest.mark.parametrize('skew', (0, 16), ids=('aligned', 'skew16'))
@pytest.mark.parametrize('case', _contract_cases(), ids=lambda c: c[0])
def test_memory_contract_of_the_profile_wrappers(case, skew, monkeypatch):
    """As tests/test_memory_contract_gpu.py does for the ops: outputs allocated inside guard bands and pre-filled with a canary,
    inputs placed between NaN bands. No band is touched, every output element is stored (also with the other output NULL),
    inputs are unchanged, and the bits do not depend on where the operands sit."""
    from witw_amd import match_profile as M
    name, fn = case
    plain = _flat(fn(lambda t: t.cuda()))
    arena = Arena('cuda', skew_bytes=skew)
    placed = []

    def place(t):
        placed.append((arena.place(t), t.clone().cpu()))
        return placed[-1][0]

    with monkeypatch.context() as m:
        m.setattr(M, 'torch', ArenaTorch(arena))
        got = fn(place)
    arena.check(got)
    got = _flat(got)
    assert len(got) == len(plain) and placed
    for a, b in zip(got, plain):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), name + ': bits depend on placement'
        if a.is_floating_point():
            assert bool(torch.isfinite(a).all()), name + ': non-finite output from finite inputs between NaN bands'
    for dev, host in placed:
        assert torch.equal(dev.cpu().view(torch.uint8), host.view(torch.uint8)), name + ': an input was written'


# ----------------------------------------------------------------------------- 7. heat map
@functools.lru_cache(maxsize=None)
def _heatmap_parts():
    from witw_amd import cvig_fov, heatmap, synth
    wts = synth.fov_dsm_weights(91)
    se = cvig_fov.FOV_DSM(circ_padding=False, weights=wts).cuda().eval()
    oe = cvig_fov.FOV_DSM(circ_padding=True, weights=wts).cuda().eval()
    strip = synth.images_u8(92, 1, (3, 150, 170))
    photo = torch.from_numpy(synth.images_u8(92, 2, (3, 90, 120)))
    src = heatmap.ArrayTileSource(strip, origin_x=1000., origin_y=5000., pixel_size=1.5)
    return se, oe, photo, src


def _sweep(path, **kw):
    from witw_amd import heatmap
    se, oe, photo, src = _heatmap_parts()
    heatmap.sweep(3, (1030., 4840., 1130., 4960.), 90., 45., 70, None, None, str(path), tile_source=src, surface_encoder=se,
                  overhead_encoder=oe, photo=photo, batch_size=4, **kw)
    return open(str(path), 'rb').read()


def test_heatmap_csv_with_hypotheses(tmp_path):
    import io

    import pandas as pd
    from witw_amd import cvig_fov, heatmap
    today = _sweep(tmp_path / 'a.csv')
    assert _sweep(tmp_path / 'b.csv', hypotheses=1) == today
    three = _sweep(tmp_path / 'c.csv', hypotheses=3)
    head = ['x', 'y', 'orientation', 'dissimilarity', 'score']
    df = pd.read_csv(io.BytesIO(three))
    assert list(df.columns) == head + ['orientation_refined', 'orientation_2', 'dissimilarity_2', 'score_2', 'orientation_3',
                                       'dissimilarity_3', 'score_3'] and len(df) == 9
    first_five = lambda raw: [b','.join(line.split(b',')[:5]) for line in raw.splitlines()]
    assert first_five(three) == today.splitlines()
    assert (df['orientation_refined'] - df['orientation']).abs().max() <= 2.8125
    bins_of = lambda frame, col: np.round((frame[col].to_numpy() + 180.) / 5.625).astype(int) % 64
    bins = lambda col: bins_of(df, col)
    for a, b in (('orientation', 'orientation_2'), ('orientation', 'orientation_3'), ('orientation_2', 'orientation_3')):
        d = np.abs(bins(a) - bins(b))
        assert np.minimum(d, 64 - d).min() > 4                                   # 22.5 degrees = 4 shifts: more than 4 apart
    assert df[['orientation_3', 'dissimilarity_3', 'score_3']].notna().all().all()
    # a heading with a tolerance: every listed orientation lies inside the window; hypotheses that do not exist are empty cells.
    # Bearing 100 at fov 70 puts the window's centre at 65 degrees; +-5 degrees holds the bins 61.875 and 67.5 (shifts 43, 44).
    windowed = _sweep(tmp_path / 'd.csv', hypotheses=3, heading=100., heading_tolerance=5., min_separation=0.)
    dw = pd.read_csv(io.BytesIO(windowed))
    center, half = heatmap.heading_window(100., 70, 5.)
    word = int(cvig_fov.orientation_mask(center, half)[0]) & (2 ** 64 - 1)
    allowed = {k for k in range(64) if (word >> k) & 1}
    assert allowed == {43, 44}
    for col in ('orientation', 'orientation_2'):
        assert dw[col].notna().all()
        assert set((np.round((dw[col].to_numpy() + 180.) / 5.625).astype(int) % 64).tolist()) <= allowed, col
    assert (bins_of(dw, 'orientation') != bins_of(dw, 'orientation_2')).all()
    assert dw[['orientation_3', 'dissimilarity_3', 'score_3']].isna().all().all() and b',,,\n' in windowed.replace(b'\r\n', b'\n')
