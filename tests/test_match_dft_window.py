"""Orientation prior on the spectral retrieval pass, host logic without a GPU: retrieve(method='dft_masked') on a stand-in op set
whose spectral ops take `shift_mask` (the masked fp64 distance plus a bounded perturbation, the runner-up allowed shift on
near-ties of narrow surfaces -- the worst the kernel may do) against the direct pass under the same mask; which slice of the mask
every op receives; that no op sees the keyword when no mask was given; two ranks with a ragged gallery split."""
import numpy as np
import pytest
import torch

from oracle import cvig_fov_oracle as O
from witw_amd import synth

from . import match_window_ref as R
from .threaded_world import run_ranks


class MaskedSpectralCpu(object):
    """Op set of retrieve() with a masked spectral pass. The bounds are a hundred times the GPU's, so that this small problem
    is full of undecided cases. Every call is recorded as (op, surface batch, mask or None, keyword present)."""
    DISTANCE_EPS = 1e-3
    SCORE_ROUNDING = 2e-4
    calls = []

    @classmethod
    def _note(cls, op, su, kw):
        m = kw.get('shift_mask')
        cls.calls.append((op, su, None if m is None else m.clone(), 'shift_mask' in kw))
        return torch.full((su.shape[0],), R.ALL, dtype=torch.int64) if m is None else m

    @staticmethod
    def match_spectrum(emb, overhead=None):
        return emb

    @classmethod
    def match_fwd(cls, ov, su, want_score=False, want_workspace=False, **kw):
        return R.match_fused(ov, su, cls._note('match_fwd', su, kw))[:2]

    @classmethod
    def match_fwd_dft(cls, ov, su, spec_ov=None, want_orientation=False, want_workspace=False, want_gap=False, **kw):
        mask = cls._note('match_fwd_dft', su, kw)
        we, w = su.shape[3], ov.shape[3]
        sc32, sc = R.scores_pair(ov, su)
        scm = R.masked_scores(sc, mask)
        col = (ov.double() ** 2).sum(dim=(1, 2))
        col2 = torch.cat((col, col[:, :we - 1]), dim=1) if we > 1 else col
        win = col2.unfold(1, we, 1)[:, :w].sum(-1).sqrt()
        sn = su.double().reshape(su.shape[0], -1).norm(dim=1)
        top = scm.topk(2, dim=-1)
        ori = torch.argmax(R.masked_scores(sc32, mask), -1)                      # the direct kernel's choice
        gap = top.values[..., 0] - top.values[..., 1]                            # over the ALLOWED shifts; +inf with one allowed
        scale = ov.double().reshape(ov.shape[0], -1).norm(dim=1)[:, None] * sn[None, :]
        pick = ori
        if we < 64:                                                              # undecided shift: take the other allowed one
            other = torch.where(top.indices[..., 0] == ori, top.indices[..., 1], top.indices[..., 0])
            pick = torch.where(gap <= 3.9 * cls.SCORE_ROUNDING * scale, other, ori)
        val = torch.gather(sc, 2, pick[:, :, None]).squeeze(-1)
        d = 2 * (1 - val / (torch.gather(win, 1, pick) * sn[None, :]))
        dist = (d + 0.9 * cls.DISTANCE_EPS * torch.sin(1e7 * d)).float()
        ws = torch.cat((win.float().reshape(-1), sn.float()))
        if want_gap:
            return None, dist, gap.float(), ws
        return (None, dist, ws) if want_workspace else (None, dist)

    @classmethod
    def match_pairs(cls, ov, su, wn, sn, pair_o, pair_s, want_orientation=True, **kw):
        ori, d, _ = R.match_fused(ov, su, cls._note('match_pairs', su, kw))
        return ori[pair_o.long(), pair_s.long()], d[pair_o.long(), pair_s.long()]

    @staticmethod
    def rank_count_band(dist, thr, eps):
        eps = torch.tensor(eps, dtype=torch.float32)
        lo, hi = (thr - eps)[None, :], (thr + eps)[None, :]
        pairs = torch.nonzero((dist >= lo) & (dist <= hi))
        return (dist < lo).sum(0).to(torch.int32), pairs[:, 0].to(torch.int32).contiguous(), pairs[:, 1].to(torch.int32).contiguous()

    @staticmethod
    def rank_count_thresh(dist, thr):
        return (dist <= thr[None, :]).sum(0).to(torch.int32)

    @staticmethod
    def topk_smallest(dist, k, index_offset=0):
        order = torch.argsort(dist, dim=0, stable=True)[:k]
        v, i = torch.gather(dist, 0, order).t().contiguous(), (order + index_offset).t().contiguous()
        if v.shape[1] < k:
            pad = k - v.shape[1]
            v = torch.cat((v, torch.full((v.shape[0], pad), float('inf'))), 1)
            i = torch.cat((i, torch.full((i.shape[0], pad), -1, dtype=torch.int64)), 1)
        return v, i


class MaskedSpectralCpuResolved(MaskedSpectralCpu):
    """... with the one-sequence band resolution of ops.rank_count_resolved"""

    @classmethod
    def rank_count_resolved(cls, dist, thr, eps, ov, su, wn, sn, **kw):
        cls._note('rank_count_resolved', su, kw)
        c, po, ps = cls.rank_count_band(dist, thr, eps)
        if po.numel():
            mask = kw.get('shift_mask', torch.full((su.shape[0],), R.ALL, dtype=torch.int64))
            d = R.match_fused(ov, su, mask)[1][po.long(), ps.long()]
            c.index_add_(0, ps.long(), (d <= thr[ps.long()]).to(torch.int32))
        return c, torch.tensor([po.numel()], dtype=torch.int32), 1 << 16


N_G, N_Q, CHUNK, K = 60, 40, 16, 5


def _data(we, amp=0.4, seed=51):
    """rows are perturbations of a few prototypes: many distances inside the (widened) rounding band of each other"""
    proto = torch.from_numpy(synth.embeddings(seed, 1, (8, 16, 4, 64)))
    gal = proto[torch.arange(N_G) % 8] + amp * torch.from_numpy(synth.embeddings(seed, 2, (N_G, 16, 4, 64)))
    gal[7] = gal[3]
    noise = torch.from_numpy(synth.embeddings(seed, 3, (N_Q, 16, 4, we)))
    qry = torch.stack([torch.roll(gal[i], -5 * i, dims=2)[:, :, :we] for i in range(N_Q)]) + 0.3 * noise
    # a third of the queries: a window holding the planted shift 5 i, a third: a window that excludes it, a third: no prior
    starts = [(5 * i - 2) % 64 if i % 3 == 0 else (5 * i + 20) % 64 for i in range(N_Q)]
    mask = R.window_words(starts, [1 + i % 9 if i % 3 == 0 else 3 + i % 7 for i in range(N_Q)])
    mask[2::3] = 0
    mask[0] = R.words([[0]])[0]                          # the planted shift of query 0, alone: an infinite gap
    return gal.contiguous(), qry.contiguous(), mask


def _rows_of(su, qry):
    """indices of su's rows in qry (the rows are distinct)"""
    eq = (su[:, None] == qry[None]).flatten(2).all(dim=2)
    assert bool((eq.sum(1) == 1).all())
    return eq.float().argmax(1)


@pytest.mark.parametrize('kernels', [MaskedSpectralCpu, MaskedSpectralCpuResolved])
@pytest.mark.parametrize('we', [64, 12])
def test_masked_spectral_retrieve_equals_direct_and_slices_the_mask(we, kernels):
    from witw_amd import cvig_fov
    gal, qry, mask = _data(we)
    r0, v0, i0 = cvig_fov.retrieve(gal, qry, k=K, query_chunk=CHUNK, method='direct', _kernels=kernels, shift_mask=mask)
    r_free = cvig_fov.retrieve(gal, qry, k=K, query_chunk=CHUNK, method='direct', _kernels=kernels)[0]
    assert not np.array_equal(r0, r_free)                          # the windows do change the ranks of this problem
    kernels.calls = []
    r1, v1, i1 = cvig_fov.retrieve(gal, qry, k=K, query_chunk=CHUNK, method='dft_masked', _kernels=kernels, shift_mask=mask)
    st = cvig_fov.last_retrieve_stats()
    np.testing.assert_array_equal(r1, r0)
    assert torch.equal(i1, i0)
    assert float((v1 - v0).abs().max()) <= st['eps']
    assert st['masked'] is True and st['method'] == 'dft_masked'
    assert st['rescored_rank'] > 0 and st['rescored_topk'] > 0 and (we == 64 or st['rescored_orientation'] > 0)
    # every op saw the words of exactly the queries it was handed
    calls = list(kernels.calls)
    for op, su, m, has_kw in calls:
        assert has_kw and torch.equal(m, mask[_rows_of(su, qry)]), op
    passes = [(su.shape[0], tuple(m.tolist())) for op, su, m, _ in calls if op == 'match_fwd_dft']
    assert passes == [(len(mask[a:a + CHUNK]), tuple(mask[a:a + CHUNK].tolist())) for a in (0, 16, 32)]
    ops_seen = {op for op, _, _, _ in calls}
    assert 'match_pairs' in ops_seen and (kernels is MaskedSpectralCpu or 'rank_count_resolved' in ops_seen)
    assert any(op == 'match_pairs' and su.shape[0] == N_Q for op, su, _, _ in calls)      # the top-k re-scoring: the whole mask
    for n in (16, 8):                                                                      # the true pairs of a chunk: its slice
        assert any(op == 'match_pairs' and su.shape[0] == n for op, su, _, _ in calls)
    # the branch that splits ranks and top-k (k + DFT_MARGIN > 32) hands the mask to both halves
    kernels.calls = []
    r2, v2, i2 = cvig_fov.retrieve(gal, qry, k=27, query_chunk=CHUNK, method='dft_masked', _kernels=kernels, shift_mask=mask)
    rd, vd, idd = cvig_fov.retrieve(gal, qry, k=27, query_chunk=CHUNK, method='direct', _kernels=kernels, shift_mask=mask)
    np.testing.assert_array_equal(r2, r0)
    assert torch.equal(i2, idd) and torch.equal(v2, vd)
    assert {op for op, _, _, _ in kernels.calls} >= {'match_fwd_dft', 'match_fwd'} and all(c[3] for c in kernels.calls)


@pytest.mark.parametrize('kernels', [MaskedSpectralCpu, MaskedSpectralCpuResolved])
def test_without_a_mask_no_op_receives_the_keyword(kernels):
    from witw_amd import cvig_fov
    gal, qry, _mask = _data(12)
    kernels.calls = []
    r1, v1, i1 = cvig_fov.retrieve(gal, qry, k=K, query_chunk=CHUNK, method='dft_masked', _kernels=kernels)
    calls_masked = list(kernels.calls)
    assert calls_masked and not any(has_kw for _, _, _, has_kw in calls_masked)
    assert cvig_fov.last_retrieve_stats()['masked'] is False
    kernels.calls = []
    r2, v2, i2 = cvig_fov.retrieve(gal, qry, k=K, query_chunk=CHUNK, method='dft', _kernels=kernels)
    np.testing.assert_array_equal(r1, r2)
    assert torch.equal(i1, i2) and torch.equal(v1, v2)
    assert [c[0] for c in kernels.calls] == [c[0] for c in calls_masked]
    r0 = cvig_fov.retrieve(gal, qry, k=K, query_chunk=CHUNK, method='direct', _kernels=kernels)[0]
    np.testing.assert_array_equal(r1, r0)


@pytest.mark.parametrize('we', [64, 12])
def test_two_ranks_with_a_ragged_gallery_split_equal_one_process(we):
    from witw_amd import cvig_fov
    gal, qry, mask = _data(we)
    r1, v1, i1 = cvig_fov.retrieve(gal, qry, k=K, query_chunk=CHUNK, method='dft_masked', _kernels=MaskedSpectralCpu, shift_mask=mask)
    cut = 37

    def fn(rank):
        g0, g1 = (0, cut) if rank == 0 else (cut, N_G)
        r, v, i = cvig_fov.retrieve(gal[g0:g1], qry, k=K, shard_begin=g0, query_chunk=CHUNK, method='dft_masked',
                                    _kernels=MaskedSpectralCpu, shift_mask=mask)
        return np.asarray(r), v.clone(), i.clone(), cvig_fov.last_retrieve_stats()['masked']
    for r, v, i, masked in run_ranks(2, fn):
        np.testing.assert_array_equal(r, r1)
        assert torch.equal(i, i1) and masked
        valid = torch.isfinite(v1)
        assert torch.equal(valid, torch.isfinite(v)) and float((v - v1)[valid].abs().max()) <= 2 * MaskedSpectralCpu.DISTANCE_EPS


def test_method_values(monkeypatch):
    from witw_amd import _lib, cvig_fov
    gal, qry, mask = _data(12)
    for k in (3, 30):
        with pytest.raises(_lib.WitwError, match='spectral'):                # 'dft' keeps refusing a mask, before any launch
            cvig_fov.retrieve(gal, qry, k=k, method='dft', shift_mask=mask)
    with pytest.raises(_lib.WitwError, match='spectral'):
        cvig_fov.evaluation_ranks(gal[:N_Q], qry, method='dft', shift_mask=mask)
    with pytest.raises(_lib.WitwError, match='dft_masked'):
        cvig_fov.evaluation_ranks(gal[:N_Q], qry, method='fft')
    with pytest.raises(_lib.WitwError, match='one word per query'):
        cvig_fov.retrieve(gal, qry, k=3, method='dft_masked', shift_mask=mask[:-1], _kernels=MaskedSpectralCpu)
    # evaluation_ranks takes the value, with and without a mask, and ranks like the direct pass
    whole = cvig_fov.retrieve
    monkeypatch.setattr(cvig_fov, 'retrieve', lambda *a, **kw: whole(*a, _kernels=MaskedSpectralCpu, **kw))
    want = whole(gal[:N_Q], qry, k=1, method='direct', _kernels=MaskedSpectralCpu, shift_mask=mask)[0]
    np.testing.assert_array_equal(cvig_fov.evaluation_ranks(gal[:N_Q], qry, method='dft_masked', shift_mask=mask), want)
    want = whole(gal[:N_Q], qry, k=1, method='direct', _kernels=MaskedSpectralCpu)[0]
    np.testing.assert_array_equal(cvig_fov.evaluation_ranks(gal[:N_Q], qry, method='dft_masked'), want)
    assert cvig_fov.Globals.match_method == 'auto'


def test_cli_match_method(monkeypatch):
    from witw_amd import cvig_fov
    seen = {}
    monkeypatch.setattr(cvig_fov, 'init_distributed', lambda *a, **k: None)
    monkeypatch.setattr(cvig_fov, 'test', lambda **kw: seen.update(kw, method=cvig_fov.Globals.match_method))
    for name in ('match_method', 'precision', 'vgg16_weights', 'loss'):
        monkeypatch.setattr(cvig_fov.Globals, name, getattr(cvig_fov.Globals, name))          # restored afterwards
    cvig_fov.main(['--mode', 'test', '--match-method', 'dft_masked', '--orientation-window', '0,20'])
    assert seen['method'] == 'dft_masked' and seen['orientation_window'] == (0., 20.)
    cvig_fov.main(['--mode', 'test'])
    assert seen['method'] == 'auto'
    with pytest.raises(SystemExit):
        cvig_fov.main(['--mode', 'test', '--match-method', 'fft'])
