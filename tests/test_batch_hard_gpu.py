"""Batch-hard soft-margin triplet loss on the HIP kernels (csrc/loss_hard.hip): mining against the torch restatement of the
definition, the pair-list match backward against the dense one, embeddings -> loss -> gradients against autograd through the
oracle, the fused training path without any dense loss gradient, config 3 on 8 rank-threads, and train() with --loss batch_hard."""
import numpy as np
import pytest
import torch

from oracle import cvig_fov_oracle as O
from witw_amd import synth

from .test_batch_hard import restated_loss
from .test_drivers_gpu import _write_dataset
from .threaded_world import run_ranks

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ALPHA = 10.


def _matrix(B, seed, nan_row=False):
    """Distances in [0, 4) with duplicated columns and rows (exact ties), +-inf entries and optionally a NaN row."""
    g = torch.Generator().manual_seed(seed)
    D = torch.rand((B, B), generator=g) * 4
    if B >= 3:
        D[:, B - 1] = D[:, 1]                   # tied columns: row minima must take the lower index
        D[B - 2, :] = D[0, :]                   # tied rows: column minima likewise
        D[1, 1] = float('-inf')                 # a -inf positive (its anchors' terms vanish) and a +inf negative
        D[2, 1] = float('inf')
    if B >= 37:
        D[7, :] = float('inf')                  # a row of +inf: the first +inf wins (the masked diagonal takes part as +inf)
        D[7, 7] = 0.5
        D[10:20, 5] = D[3, 5]                   # ties inside one column
    if nan_row:
        D[B // 2, (B // 2 + 3) % B] = float('nan')
        D[B // 2, (B // 2 + 1) % B] = float('nan')
    return D


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


@pytest.mark.parametrize('B', [2, 3, 37, 128, 1024])
def test_mining_kernel_equals_restatement(B):
    from witw_amd import cvig_fov, ops
    for nan_row in (False, True):
        D = _matrix(B, 100 + B, nan_row)
        Dd = D.to(DEV)
        loss, rv, ri, cv, ci = ops.batch_hard_fwd(Dd, ALPHA)
        loss2, rv2, ri2, cv2, ci2 = ops.batch_hard_fwd(Dd, ALPHA)
        torch.cuda.synchronize()
        for a, b in ((loss, loss2), (rv, rv2), (ri, ri2), (cv, cv2), (ci, ci2)):     # bitwise repeatable
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
        l_r, rv_r, ri_r, cv_r, ci_r = restated_loss(Dd.cpu())
        assert torch.equal(ri.cpu(), ri_r) and torch.equal(ci.cpu(), ci_r), (B, nan_row)
        assert torch.equal(rv.cpu(), rv_r) or (torch.isnan(rv.cpu()) == torch.isnan(rv_r)).all()
        if nan_row:
            assert torch.isnan(loss).item() and torch.isnan(l_r).item()
            continue
        assert _rel(loss.item(), l_r.item()) <= 1e-6, (B, loss.item(), l_r.item())
        # dense gradient of the stand-alone loss against autograd through the restatement
        Dg = Dd.clone().requires_grad_(True)
        cvig_fov.batch_hard_triplet_loss(Dg, ALPHA).backward(torch.tensor(0.7, device=DEV))
        Dc = Dd.cpu().clone().requires_grad_(True)
        (restated_loss(Dc)[0] * 0.7).backward()
        ref = Dc.grad.nan_to_num(0.)
        assert int((Dg.grad.cpu() != 0).sum()) <= 3 * B
        np.testing.assert_allclose(Dg.grad.cpu().numpy(), ref.numpy(), rtol=0, atol=1e-6 * float(ref.abs().max()))
        # the pair list of the full form carries the same gradient
        po, ps, pw = ops.batch_hard_pairs(Dd.diagonal().contiguous(), rv, ri, cv, ci, torch.tensor([0.7], device=DEV), 0, ALPHA)
        dense = torch.zeros((B, B), dtype=torch.float64)
        ok = (po >= 0).cpu()
        dense.index_put_((po.cpu()[ok].long(), ps.cpu()[ok].long()), pw.cpu()[ok].double(), accumulate=True)
        np.testing.assert_allclose(dense.numpy(), Dg.grad.cpu().double().numpy(), rtol=0, atol=1e-7 * float(ref.abs().max()))


@pytest.mark.parametrize('B,b', [(128, 32), (1024, 128), (37, 5)])
def test_slab_mining_merge_and_partials_equal_full_form(B, b):
    from witw_amd import ops
    D = _matrix(B, 7 + B)
    Dd = D.to(DEV)
    loss, rv, ri, cv, ci = ops.batch_hard_fwd(Dd, ALPHA)
    parts_v, parts_i, total = [], [], 0.
    for col0 in range(0, B - b + 1, b):
        slab = Dd[:, col0:col0 + b].contiguous()
        rv_l, ri_l, cv_l, ci_l = ops.batch_hard_slab_mine(slab, col0)
        # local row minima over the slab's columns only (global indices)
        Dm = D[:, col0:col0 + b].clone()
        idx = torch.arange(b)
        Dm[col0 + idx, idx] = float('inf')
        v_r, i_r = Dm.min(dim=1)
        assert torch.equal(ri_l.cpu(), i_r + col0) and torch.equal(rv_l.cpu(), v_r), col0
        assert torch.equal(ci_l.cpu(), ci.cpu()[col0:col0 + b]) and torch.equal(cv_l.cpu(), cv.cpu()[col0:col0 + b])
        parts_v.append(rv_l)
        parts_i.append(ri_l)
    n = len(parts_v)
    rv_m, ri_m = ops.batch_hard_merge_rows(torch.stack(parts_v), torch.stack(parts_i))
    if n * b == B:
        assert torch.equal(ri_m.cpu(), ri.cpu()) and torch.equal(rv_m.cpu(), rv.cpu())
        for k, col0 in enumerate(range(0, B, b)):
            slab = Dd[:, col0:col0 + b].contiguous()
            total += ops.batch_hard_slab_loss(slab, rv, cv[col0:col0 + b].contiguous(), col0, ALPHA).item()
        assert _rel(total / (2. * B), loss.item()) <= 1e-6


def _pairs_case(Bo, Bs, we, seed):
    g = torch.Generator().manual_seed(seed)
    n = 3 * max(Bo, Bs)
    po = torch.randint(0, Bo, (n,), generator=g, dtype=torch.int32)
    ps = torch.randint(0, Bs, (n,), generator=g, dtype=torch.int32)
    po[:6] = 3                                   # a repeated row ...
    ps[6:12] = 2                                 # ... a repeated column ...
    po[12:15], ps[12:15] = 5, 7                  # ... and a duplicated pair
    po[15], ps[16] = -1, -1                      # ignored entries
    pw = torch.randn((n,), generator=g)
    ov = torch.from_numpy(synth.embeddings(seed, 1, (Bo, 16, 4, 64)))
    su = torch.from_numpy(synth.embeddings(seed, 2, (Bs, 16, 4, we)))
    return ov, su, po, ps, pw


@pytest.mark.parametrize('we', [64, 12, 1])
def test_match_bwd_pairs_equals_dense_match_bwd(we):
    from witw_amd import ops
    Bo, Bs = 40, 24
    ov, su, po, ps, pw = _pairs_case(Bo, Bs, we, 300 + we)
    ov, su = ov.to(DEV), su.to(DEV)
    ori, dist, score, ws = ops.match_fwd(ov, su, want_score=True, want_workspace=True)
    args = (ov, su, ori, score, ws, po.to(DEV), ps.to(DEV), pw.to(DEV))
    gov, gsu = ops.match_bwd_pairs(*args)
    gov2, gsu2 = ops.match_bwd_pairs(*args)
    g = torch.zeros((Bo, Bs))
    ok = (po >= 0) & (ps >= 0)
    g.index_put_((po[ok].long(), ps[ok].long()), pw[ok], accumulate=True)
    gov_d, gsu_d = ops.match_bwd(ov, su, ori, score, ws, g.to(DEV).contiguous())
    torch.cuda.synchronize()
    assert torch.equal(gov.view(torch.int32), gov2.view(torch.int32)) and torch.equal(gsu.view(torch.int32), gsu2.view(torch.int32))
    for got, ref in ((gov, gov_d), (gsu, gsu_d)):
        got, ref = got.cpu().double(), ref.cpu().double()
        assert float((got - ref).norm()) <= 1e-6 * float(ref.norm()), float((got - ref).norm() / ref.norm())
    untouched = sorted(set(range(Bo)) - set(po[ok].tolist()))
    if untouched:
        assert (gov.cpu()[untouched] == 0).all()


def _embeddings(B, we, seed):
    ov = torch.from_numpy(synth.embeddings(seed, 1, (B, 16, 4, 64)))
    noise = torch.from_numpy(synth.embeddings(seed, 2, (B, 16, 4, we)))
    shift = (3 * torch.arange(B)) % 64
    col = (torch.arange(we)[None, :] + shift[:, None]) % 64
    su = torch.gather(ov, 3, col[:, None, None, :].expand(-1, 16, 4, -1)) + 2.0 * noise
    return ov.contiguous(), su.contiguous()


@pytest.mark.parametrize('we', [64, 12])
def test_end_to_end_against_oracle_autograd(we):
    from witw_amd import cvig_fov
    B = 16
    ov, su = _embeddings(B, we, 400 + we)
    ovg, sug = ov.to(DEV).requires_grad_(True), su.to(DEV).requires_grad_(True)
    loss, ori, d, rv, ri, cv, ci = cvig_fov.sharded_match_loss(ovg, sug, loss='batch_hard', mined=True)
    loss.backward()
    # oracle: the reference's correlation -> crop -> l2_distance, and the loss restated with the GPU's mined indices
    ovc, suc = ov.clone().requires_grad_(True), su.clone().requires_grad_(True)
    ori_c, D = O.match(ovc, suc)
    assert torch.equal(ori_c, ori.cpu())
    ri_c, ci_c = ri.cpu(), ci.cpu()
    dg = D.diagonal()
    ar = torch.arange(B)
    loss_c = (torch.log(1 + torch.exp(ALPHA * (dg - D[ar, ri_c]))).sum()
              + torch.log(1 + torch.exp(ALPHA * (dg - D[ci_c, ar]))).sum()) / (2 * B)
    loss_c.backward()
    _, _, ri_r, _, ci_r = restated_loss(D.detach())
    assert torch.equal(ri_r, ri_c) and torch.equal(ci_r, ci_c)
    assert abs(loss.item() - loss_c.item()) <= 1e-5
    for got, ref in ((ovg.grad, ovc.grad), (sug.grad, suc.grad)):
        got, ref = got.cpu().double(), ref.double()
        assert float((got - ref).norm()) <= 1e-4 * float(ref.norm())


def test_fused_path_never_runs_a_dense_backward(monkeypatch):
    from witw_amd import cvig_fov, ops

    def dense(*a, **k):
        raise AssertionError('a dense backward ran')
    for name in ('match_bwd', 'batch_hard_bwd', 'triplet_loss_bwd', 'triplet_loss_slab_bwd'):
        monkeypatch.setattr(ops, name, dense)
    ov, su = _embeddings(32, 64, 410)
    ovg, sug = ov.to(DEV).requires_grad_(True), su.to(DEV).requires_grad_(True)
    loss, _, _ = cvig_fov.sharded_match_loss(ovg, sug, loss='batch_hard')
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item() and ovg.grad.abs().sum().item() > 0 and sug.grad.abs().sum().item() > 0


def _encoder_grads(precision, fused):
    from witw_amd import cvig_fov
    wts = synth.fov_dsm_weights(77)
    enc_s = cvig_fov.FOV_DSM(False, weights=wts).to(DEV).train()
    enc_o = cvig_fov.FOV_DSM(True, weights=wts).to(DEV).train()
    enc_s.precision = enc_o.precision = precision
    B = 4
    s = torch.from_numpy(synth.embeddings(78, 1, (B, 3, 128, 512))).to(DEV)
    p = torch.from_numpy(synth.embeddings(78, 2, (B, 3, 128, 512))).to(DEV)
    enc_s._drop_step = enc_o._drop_step = 0
    su, ov = enc_s(s), enc_o(p)
    if fused:
        loss, _, _ = cvig_fov.sharded_match_loss(ov, su, loss='batch_hard')
    else:
        loss = cvig_fov.batch_hard_triplet_loss(cvig_fov.match(ov, su)[1])
    loss.backward()
    params = list(enc_s.parameters()) + list(enc_o.parameters())
    return loss.item(), [None if q.grad is None else q.grad.detach().cpu().double() for q in params]


def test_encoder_training_step_fused_equals_dense():
    loss_f, g_f = _encoder_grads('fp32', True)
    loss_d, g_d = _encoder_grads('fp32', False)
    assert np.isfinite(loss_f) and abs(loss_f - loss_d) <= 1e-5 * max(1., abs(loss_d))
    n = 0
    for a, b in zip(g_f, g_d):
        assert (a is None) == (b is None)
        if a is None:
            continue
        n += 1
        assert float((a - b).norm()) <= 1e-4 * float(b.norm()) + 1e-30
    assert n > 0
    loss_b, g_b = _encoder_grads('bf16', True)
    assert np.isfinite(loss_b) and any(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0 for g in g_b)


def test_config3_batch_hard_over_8_rank_threads_equals_full_matrix():
    from witw_amd import cvig_fov
    B, b, we = 1024, 128, 64
    ov, su = _embeddings(B, we, 420)
    su[b + 9] = su[3]                              # a tie across two slabs
    ov_d, su_d = ov.to(DEV), su.to(DEV)

    def fn(rank):
        torch.cuda.set_device(DEV)
        sl = slice(rank * b, (rank + 1) * b)
        ov_l, su_l = ov_d[sl].clone().requires_grad_(True), su_d[sl].clone().requires_grad_(True)
        loss, ori, d, rv, ri, cv, ci = cvig_fov.sharded_match_loss(ov_l, su_l, loss='batch_hard', mined=True)
        loss.backward()
        torch.cuda.synchronize()
        return loss.item(), ov_l.grad.cpu(), su_l.grad.cpu(), ri.cpu(), ci.cpu()
    res = run_ranks(8, fn)
    ov1, su1 = ov_d.clone().requires_grad_(True), su_d.clone().requires_grad_(True)
    loss1, _, d1, rv1, ri1, cv1, ci1 = cvig_fov.sharded_match_loss(ov1, su1, loss='batch_hard', mined=True)
    loss1.backward()
    _, _, ri_r, _, ci_r = restated_loss(d1.cpu())
    assert torch.equal(ri1.cpu(), ri_r) and torch.equal(ci1.cpu(), ci_r)
    for rank, (loss, g_ov, g_su, ri, ci) in enumerate(res):
        sl = slice(rank * b, (rank + 1) * b)
        assert _rel(loss, loss1.item()) <= 1e-6, (rank, loss, loss1.item())
        assert torch.equal(ri, ri1.cpu()) and torch.equal(ci, ci1.cpu()[sl])
        for got, one in ((g_ov, ov1.grad[sl].cpu()), (g_su, su1.grad[sl].cpu())):
            assert float((got.double() - one.double()).norm()) <= 1e-6 * float(one.double().norm()), rank


def test_train_driver_with_batch_hard_loss(tmp_path, monkeypatch):
    from witw_amd import cvig_fov, ops
    csv = _write_dataset(str(tmp_path), 6)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(cvig_fov.Globals, 'loss', 'batch_hard')

    def dense(*a, **k):
        raise AssertionError('a dense backward ran')
    monkeypatch.setattr(ops, 'match_bwd', dense)
    seen = []

    class SpyAdam(cvig_fov.Adam):
        def __init__(self, params, **kw):
            super().__init__(params, **kw)
            seen.append((self, [q.detach().clone() for q in self.params]))
    monkeypatch.setattr(cvig_fov, 'Adam', SpyAdam)
    best = cvig_fov.train(dataset='cvusa', fov=70, val_quantity=2, batch_size=2, num_workers=0, num_epochs=1, csv_path=csv)
    assert best is not None and np.isfinite(best)
    opt, before = seen[0]
    assert any(not torch.equal(q.detach(), q0) for q, q0 in zip(opt.params, before))
