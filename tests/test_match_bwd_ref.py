"""tests/match_bwd_ref.py (the float64 reference of tests/test_match_bwd_edges_gpu.py) pinned without a GPU: against float64
autograd through the oracle's crop_overhead and l2_distance, against the reference goldens through the float64 triplet-loss
gradient, and -- for every case of the GPU edge tests -- the geometry the case states against this module's restatement of the
launcher's split heuristic and against the library's own witw_match_bwd_scratch_floats (an export that launches nothing)."""
import os

import numpy as np
import pytest
import torch

from oracle import cvig_fov_oracle as O
from tests import match_bwd_ref as R
from tests import test_match_bwd_edges_gpu as T
from witw_amd import synth


def _case(seed, Bo, Bs, We):
    g = np.random.Generator(np.random.Philox(key=[seed, 17]))
    return (g.standard_normal((Bo, 16, 4, 64)), g.standard_normal((Bs, 16, 4, We)), g.integers(0, 64, size=(Bo, Bs), dtype=np.int64),
            g.standard_normal((Bo, Bs)))


def _autograd64(ov, su, ori, gd):
    ovr, sur = torch.from_numpy(ov).requires_grad_(True), torch.from_numpy(su).requires_grad_(True)
    d = O.l2_distance(O.crop_overhead(ovr, torch.from_numpy(ori), su.shape[3]), sur)
    (d * torch.from_numpy(gd)).sum().backward()
    return d.detach().numpy(), ovr.grad.numpy(), sur.grad.numpy()


@pytest.mark.parametrize('shape', [(5, 3, 33), (3, 4, 64), (2, 2, 1)])
def test_closed_form_equals_float64_autograd(shape):
    ov, su, ori, gd = _case(sum(shape), *shape)
    ori[0, 0], ori[-1, -1] = 63, 0                      # a window that wraps and one that does not
    d, a_ov, a_su = _autograd64(ov, su, ori, gd)
    g_ov, g_su, s_ov, s_su = R.match_bwd_ref(ov, su, ori, gd)
    assert g_ov.dtype == np.float64 and g_ov.shape == ov.shape and g_su.shape == su.shape
    assert np.all(s_ov >= np.abs(g_ov)) and np.all(s_su >= np.abs(g_su)) and np.all(s_su > 0)
    assert R.err(a_ov, g_ov, s_ov) <= 1e-12 and R.err(a_su, g_su, s_su) <= 1e-12
    score, wn, sn = R.kernel_inputs(ov, su, ori)
    assert score.shape == ori.shape and wn.shape == (shape[0], 64) and sn.shape == (shape[1],)
    np.testing.assert_allclose(2 * (1 - score / (np.take_along_axis(wn, ori, 1) * sn[None, :])), d, rtol=0, atol=1e-13)
    # columns no window covers have no term: scale 0 (err() above has held autograd to an exact 0 there)
    if shape[2] == 1:
        covered = np.zeros((shape[0], 64), dtype=bool)
        covered[np.arange(shape[0])[:, None], ori] = True
        assert np.array_equal(s_ov.reshape(shape[0], 64, 64).any(axis=1), covered)


def test_pair_form_is_the_dense_form_of_the_scattered_weights():
    ov, su, ori, _gd = _case(5, 6, 4, 12)
    po = np.array([0, 5, 5, 5, -1, 6, 2, 2, 3], dtype=np.int32)
    ps = np.array([1, 3, 3, 3, 2, 0, 4, -1, 0], dtype=np.int32)
    pw = np.array([1.5, 2.0, -2.0, 0.25, 9.0, 9.0, 9.0, 9.0, -1.0])
    gd, ga, ok = R.pairs_to_dense(po, ps, pw, 6, 4)
    assert ok.tolist() == [True, True, True, True, False, False, False, False, True]
    want = np.zeros((6, 4))
    want[0, 1], want[5, 3], want[3, 0] = 1.5, 0.25, -1.0
    assert np.array_equal(gd, want) and ga[5, 3] == 4.25 and ga.sum() == 6.75
    g_ov, g_su, s_ov, s_su = R.match_bwd_pairs_ref(ov, su, ori, po, ps, pw)
    d_ov, d_su, _, _ = R.match_bwd_ref(ov, su, ori, gd)
    assert np.array_equal(g_ov, d_ov) and np.array_equal(g_su, d_su)
    # rows no valid pair names: no term; the duplicated pair's scale counts every entry of the list
    assert not s_ov[[1, 2, 4]].any() and not s_su[2].any() and s_ov[[0, 3, 5]].reshape(3, 64, 64).any(axis=(1, 2)).all()
    n_ov, n_su = R.match_bwd_ref(ov, su, ori, gd)[2:]                   # the scales had the duplicates been summed first
    assert np.all(s_ov >= n_ov) and np.all(s_su >= n_su) and np.all(s_su[3] > n_su[3]) and np.array_equal(s_su[1], n_su[1])


def test_composed_with_the_triplet_loss_it_reproduces_the_reference_goldens(golden_dir):
    """the goldens a / d / e of matching.npz at the reference's own orientations, within the atol tests/test_backward_gpu.py holds
    the kernels to"""
    g = np.load(os.path.join(golden_dir, 'matching.npz'))
    seed = int(g['seed'])
    for tag in 'ade':
        bo, bs, we = (int(v) for v in g['%s_shape' % tag])
        ov = synth.embeddings(seed, 100 + ord(tag), (bo, 16, 4, 64))
        su = synth.embeddings(seed, 200 + ord(tag), (bs, 16, 4, we))
        ori = g['%s_orientation' % tag]
        score, wn, sn = R.kernel_inputs(ov, su, ori)
        d = torch.from_numpy(2 * (1 - score / (np.take_along_axis(wn, ori, 1) * sn[None, :]))).requires_grad_(True)
        np.testing.assert_allclose(d.detach().numpy(), g['%s_distance' % tag], rtol=0, atol=2e-6)
        loss = O.triplet_loss(d)
        loss.backward()
        np.testing.assert_allclose(loss.item(), float(g['%s_loss' % tag]), rtol=1e-5)
        g_ov, g_su, _, _ = R.match_bwd_ref(ov, su, ori, d.grad.numpy())
        np.testing.assert_allclose(g_ov, g['%s_grad_ov' % tag], rtol=0, atol=2e-6)
        np.testing.assert_allclose(g_su, g['%s_grad_su' % tag], rtol=0, atol=2e-6)


def test_geometry_restates_the_launcher():
    assert R.geometry(1, 1) == (1, 1, 0) and R.geometry(128, 128) == (4, 32, 0) and R.geometry(1024, 128) == (6, 171, 0)
    assert R.geometry(1089, 23) == (34, 33, 1) and R.geometry(31, 1) == (1, 31, 0) and R.geometry(33, 1) == (2, 17, 0)
    from witw_amd import _lib
    lib = _lib.load()
    empties = 0
    for Bs in (1, 5, 20, 23, 29, 128, 767, 768, 800):
        for Bo in range(1, 1400):
            We = 1 + (Bo * 7 + Bs) % 64
            assert int(lib.witw_match_bwd_scratch_floats(Bo, Bs, We)) == R.scratch_floats(Bo, Bs, We), (Bo, Bs, We)
            s, per, empty = R.geometry(Bo, Bs)
            assert s >= 1 and (s - empty - 1) * per < Bo <= (s - empty) * per
            empties += empty > 0
    assert empties >= 1
    assert lib.witw_match_bwd_scratch_floats(0, 4, 4) == -1 and lib.witw_match_bwd_scratch_floats(4, 4, 65) == -1


@pytest.mark.parametrize('c', T.DENSE + T.WRAP + T.ZERO, ids=T.case_id)
def test_every_dense_case_has_the_geometry_it_was_written_for(c):
    """the stated (splits, overheads per split, empty trailing splits) against geometry(), and the library's scratch size against
    splits * Bs * (64 We + 1) (0 with one split): a later change to the heuristic fails here"""
    from witw_amd import _lib
    assert T.scratch_geometry(c) == (c.splits, c.per, c.empty)
    assert (R.geometry(c.Bo, c.Bs) if c.scratch else (1, c.Bo, 0)) == (c.splits, c.per, c.empty)
    s = R.splits(c.Bo, c.Bs)
    assert int(_lib.load().witw_match_bwd_scratch_floats(c.Bo, c.Bs, c.We)) == (s * c.Bs * (64 * c.We + 1) if s > 1 else 0)
    if not c.scratch:           # the forced single split is a different path only where the heuristic would have split
        assert s > 1


def test_the_cases_reach_what_they_name():
    by = {T.case_id(c): c for c in T.CASES}
    c = by['dense-300x800x2']
    assert c.per > 256 and c.per - 256 == 44 and c.splits == 1 and c.Bs > 3 * 256 and c.Bs - 3 * 256 == 32
    c = by['dense-33x768x1']
    assert c.Bs == 3 * 256 and c.splits == 1
    c = by['dense-70x5x63']
    assert c.Bo - (c.splits - 1) * c.per == 22
    c = by['dense-1089x23x3']
    assert c.empty == 1 and (c.splits - 1) * c.per >= c.Bo
    c = by['dense-600x5x64-noscratch']
    assert c.Bo == 256 + 256 + 88
    seg = {}
    for c in T.PAIRS:
        po, ps, pw = T._pair_list(c)
        ok = (po >= 0) & (po < c.Bo) & (ps >= 0) & (ps < c.Bs)
        seg[c.name] = (int(ok.sum()), int(np.bincount(po[ok], minlength=1).max()), int(np.bincount(ps[ok], minlength=1).max()))
        assert po.dtype == np.int32 and ps.dtype == np.int32 and pw.dtype == np.float32 and po.shape == ps.shape == pw.shape == (c.n,)
    assert seg['one'] == (1, 1, 1) and seg['invalid'] == (0, 0, 0)
    assert seg['one_surface'][2] == 600 and seg['one_surface'][1] <= 10 and seg['one_overhead'][1] == 600
    n_ok = seg['ragged'][0]
    po, ps, _ = T._pair_list(by['pairs-ragged-1025-64x64x4'])
    assert 0 < n_ok < 1025 and (po == -1).any() and (po == 64).any() and (ps == -1).any() and (ps == 64).any()
    assert R.cdiv(1025, 1024) == 2                                       # just above a power of two: npad = 2048
    po, ps, _ = T._pair_list(by['pairs-max-8192-64x64x4'])
    assert seg['max'][0] == T.PAIRS_MAX and int(((po == 9) & (ps == 31)).sum()) >= 300
    assert 0 < seg['mixed'][0] < 120


@pytest.mark.parametrize('c', T.CASES, ids=T.case_id)
def test_the_reference_of_every_case_is_not_trivially_small(c):
    """median |ref| / scale over the elements that have a term: above 1e-3 on the inputs the GPU tests use"""
    ex = T.exact(c)
    for side in ('ov', 'su'):
        med = T.median_ref_over_scale(ex['ref_' + side], ex['sc_' + side])
        if isinstance(c, T.Pairs) and not ex['ok'].any():
            assert med is None and not ex['ref_' + side].any()
        else:
            assert med is not None and med > T.NONTRIVIAL, (side, med)
    assert ex['score'].dtype == np.float32 and ex['ws'].shape == (c.Bo * 64 + c.Bs,) and np.isfinite(ex['ws']).all() and (ex['ws'] > 0).all()
