"""Batch-hard soft-margin triplet loss without a GPU: the C ABI's argument checks, the --loss switch of the two CLIs, and the
host algebra of cvig_fov.sharded_match_loss(..., loss='batch_hard') -- per-rank mining, the rank-order merge of the row minima,
the loss partials and the per-slab pair lists -- driven by CPU restatements of the kernels through the `_kernels=` hook over
gloo (world 2) and the in-process threaded group (world 8, config 3: B = 1024, b = 128). The loss, every rank's embedding
gradients and the mined indices must equal the single-process restatement on the gathered batch."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from witw_amd import synth

from .test_parallel_world8_gloo import CpuKernels, _free_port
from .threaded_world import run_ranks

ALPHA = 10.


# ----------------------------------------------------------------------------- the definition, restated in torch
def restated_loss(D, alpha=ALPHA):
    """-> (loss, rv, ri, cv, ci): the issue's definition, literally."""
    B = D.shape[0]
    Dm = D.masked_fill(torch.eye(B, dtype=torch.bool), float('inf'))
    rv, ri = Dm.min(dim=1)
    cv, ci = Dm.min(dim=0)
    d = D.diagonal()
    loss = (torch.log(1 + torch.exp(alpha * (d - rv))).sum() + torch.log(1 + torch.exp(alpha * (d - cv))).sum()) / (2 * B)
    return loss, rv, ri, cv, ci


def dist64(ov, su, ori):
    """match's distance for the orientations `ori`, float64 and differentiable (correlation -> crop -> l2_distance fused)."""
    we = su.shape[3]
    x = torch.cat((ov, ov[:, :, :, :we - 1]), dim=3) if we > 1 else ov
    sc = F.conv2d(x, su).squeeze(-2)
    col = (ov * ov).sum(dim=(1, 2))
    col2 = torch.cat((col, col[:, :we - 1]), dim=1) if we > 1 else col
    win = col2.unfold(1, we, 1)[:, :ov.shape[3]].sum(-1)
    best = torch.gather(sc, 2, ori[:, :, None]).squeeze(-1)
    wn = torch.gather(win, 1, ori).sqrt()
    sn = su.reshape(su.shape[0], -1).norm(dim=1)
    return 2 * (1 - best / (wn * sn[None, :]))


def orientation(ov, su):
    we = su.shape[3]
    x = torch.cat((ov, ov[:, :, :, :we - 1]), dim=3) if we > 1 else ov
    return torch.argmax(F.conv2d(x, su).squeeze(-2), -1)


def _better(v, i, bv, bi):
    vn, bn = torch.isnan(v), torch.isnan(bv)
    return torch.where(vn != bn, vn, torch.where(vn | (v == bv), i < bi, v < bv))


class BatchHardCpuKernels(CpuKernels):
    """The batch-hard op set of cvig_fov._BatchHardMatchLossFn restated on the CPU (formulas of csrc/loss_hard.hip). Distances
    are taken in float64 and rounded once, so that a pair's distance does not depend on the shard it is computed in."""

    @staticmethod
    def match_fwd(ov, su, want_score=False, want_workspace=False):
        with torch.no_grad():
            ori = orientation(ov, su)
            d = dist64(ov.double(), su.double(), ori).float()
        if want_workspace:
            return ori, d, torch.zeros(1), torch.zeros(1)
        return ori, d

    @staticmethod
    def match_bwd_pairs(ov, su, ori, score, ws, po, ps, pw):
        g = torch.zeros((ov.shape[0], su.shape[0]), dtype=torch.float64)
        ok = (po >= 0) & (ps >= 0)
        g.index_put_((po[ok].long(), ps[ok].long()), pw[ok].double(), accumulate=True)
        with torch.enable_grad():
            ov64 = ov.detach().double().requires_grad_(True)
            su64 = su.detach().double().requires_grad_(True)
            dist64(ov64, su64, ori).backward(g)
        return ov64.grad.float(), su64.grad.float()

    @staticmethod
    def batch_hard_fwd(dist, alpha):
        loss, rv, ri, cv, ci = restated_loss(dist, alpha)
        return loss.reshape(1), rv, ri, cv, ci

    @staticmethod
    def batch_hard_slab_mine(dist, col0):
        b = dist.shape[1]
        idx = torch.arange(b)
        Dm = dist.clone()
        Dm[col0 + idx, idx] = float('inf')
        rv, ri = Dm.min(dim=1)
        cv, ci = Dm.min(dim=0)
        return rv, ri + col0, cv, ci

    @staticmethod
    def batch_hard_merge_rows(rv_parts, ri_parts):
        rv, ri = rv_parts[0].clone(), ri_parts[0].clone()
        for r in range(1, rv_parts.shape[0]):
            take = _better(rv_parts[r], ri_parts[r], rv, ri)
            rv = torch.where(take, rv_parts[r], rv)
            ri = torch.where(take, ri_parts[r], ri)
        return rv, ri

    @staticmethod
    def batch_hard_slab_loss(dist, rv, cv, col0, alpha):
        b = dist.shape[1]
        idx = torch.arange(b)
        d = dist[col0 + idx, idx]
        t = torch.log(1 + torch.exp(alpha * (d - rv[col0 + idx]))) + torch.log(1 + torch.exp(alpha * (d - cv)))
        return t.sum().reshape(1)

    @staticmethod
    def batch_hard_pairs(diag, rv, ri, cv, ci, g_loss, col0, alpha):
        B, b = diag.numel(), cv.numel()
        sc = g_loss.reshape(()) * alpha / (2. * B)
        idx = torch.arange(b)
        wr = sc * torch.sigmoid(alpha * (diag - rv))
        wc = sc * torch.sigmoid(alpha * (diag[col0 + idx] - cv))
        mine = (ri >= col0) & (ri < col0 + b)
        po = torch.cat((col0 + idx, ci, torch.where(mine, torch.arange(B), -1)))
        ps = torch.cat((idx, idx, torch.where(mine, ri - col0, -1)))
        pw = torch.cat((wr[col0 + idx] + wc, -wc, torch.where(mine, -wr, torch.zeros_like(wr))))
        return po.to(torch.int32), ps.to(torch.int32), pw


def planted(B, b, we, seed):
    """Embeddings with planted matches and planted ties: two identical surface columns inside rank 0's slab that are some row's
    hardest negative, two identical columns in the slabs of ranks 0 and 1 that are another row's hardest negative, and two
    identical overhead rows that are a column's hardest negative. -> (ov, su, expected ties)"""
    ov = torch.from_numpy(synth.embeddings(seed, 1, (B, 16, 4, 64)))
    noise = torch.from_numpy(synth.embeddings(seed, 2, (B, 16, 4, we)))
    small = torch.from_numpy(synth.embeddings(seed, 3, (3, 16, 4, 64)))
    shift = (5 * torch.arange(B)) % 64
    col = (torch.arange(we)[None, :] + shift[:, None]) % 64
    su = torch.gather(ov, 3, col[:, None, None, :].expand(-1, 16, 4, -1)) + 2.0 * noise
    r_in, c_in, c_in2 = 5, 3, b - 1             # inside rank 0: row 5 -> columns 3 / b-1
    r_x, c_x, c_x2 = b + 2, 2, b + 4            # across ranks 0 / 1: row b+2 (rank 1) -> columns 2 / b+4
    c_col, r_c, r_c2 = 1, b + 1, b + 6          # column 1 -> overhead rows b+1 / b+6
    su[c_in] = su[r_in] + 0.05 * small[0, :, :, :we]
    su[c_in2] = su[c_in]
    su[c_x] = su[r_x] + 0.05 * small[1, :, :, :we]
    su[c_x2] = su[c_x]
    ov[r_c] = torch.roll(ov[c_col], 0, dims=2) + 0.05 * small[2]
    ov[r_c2] = ov[r_c]
    return ov.contiguous(), su.contiguous(), ((r_in, c_in, c_in2), (r_x, c_x, c_x2), (c_col, r_c, r_c2))


def single_process(ov, su):
    """-> (loss, grad ov, grad su, ri, ci, D) of the restatement on the gathered batch, autograd through the float64 distance."""
    ovf, suf = ov.clone().requires_grad_(True), su.clone().requires_grad_(True)
    ori = orientation(ov, su)
    D = dist64(ovf.double(), suf.double(), ori).float()
    loss, rv, ri, cv, ci = restated_loss(D)
    loss.backward()
    return loss.item(), ovf.grad, suf.grad, ri, ci, D.detach()


def check_ranks(res, ref, b):
    loss_f, gov, gsu, ri_f, ci_f, _ = ref
    for rank, (loss, g_ov, g_su, ri, ci) in enumerate(res):
        sl = slice(rank * b, (rank + 1) * b)
        assert abs(loss - loss_f) <= 1e-6 * abs(loss_f), (rank, loss, loss_f)
        assert torch.equal(ri, ri_f), rank
        assert torch.equal(ci, ci_f[sl]), rank
        np.testing.assert_allclose(g_ov.numpy(), gov[sl].numpy(), rtol=0, atol=1e-6 * float(gov[sl].abs().max()))
        np.testing.assert_allclose(g_su.numpy(), gsu[sl].numpy(), rtol=0, atol=1e-6 * float(gsu[sl].abs().max()))


def check_ties(ref, ties):
    _, _, _, ri, ci, D = ref
    (r_in, c_in, c_in2), (r_x, c_x, c_x2), (c_col, r_c, r_c2) = ties
    assert D[r_in, c_in] == D[r_in, c_in2] and ri[r_in] == c_in          # the planted ties are ties, and the lower index wins
    assert D[r_x, c_x] == D[r_x, c_x2] and ri[r_x] == c_x
    assert D[r_c, c_col] == D[r_c2, c_col] and ci[c_col] == r_c


def _run_rank(ov, su, rank, b):
    from witw_amd import cvig_fov
    sl = slice(rank * b, (rank + 1) * b)
    ov_l, su_l = ov[sl].clone().requires_grad_(True), su[sl].clone().requires_grad_(True)
    loss, ori, d, rv, ri, cv, ci = cvig_fov.sharded_match_loss(ov_l, su_l, loss='batch_hard', mined=True,
                                                               _kernels=BatchHardCpuKernels)
    assert tuple(d.shape) == (ov.shape[0], b) and tuple(ori.shape) == (ov.shape[0], b)
    loss.backward()
    return loss.item(), ov_l.grad.clone(), su_l.grad.clone(), ri.clone(), ci.clone()


# ----------------------------------------------------------------------------- world 2 over gloo
W2_B, W2_b, W2_WE = 16, 8, 8


def _gloo_worker(rank, world, port, out_q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        ov, su, _ = planted(W2_B, W2_b, W2_WE, 61)
        out_q.put((rank,) + _run_rank(ov, su, rank, W2_b))
    finally:
        dist.destroy_process_group()


def test_batch_hard_sharded_gloo_world2_equals_single_process():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    ov, su, ties = planted(W2_B, W2_b, W2_WE, 61)
    ref = single_process(ov, su)
    check_ties(ref, ties)
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    check_ranks([r[1:] for r in res], ref, W2_b)


def test_batch_hard_single_process_hook_equals_restatement():
    """world 1 through the same Function (full-matrix form)"""
    from witw_amd import cvig_fov
    ov, su, ties = planted(W2_B, W2_b, W2_WE, 61)
    ref = single_process(ov, su)
    ov_l, su_l = ov.clone().requires_grad_(True), su.clone().requires_grad_(True)
    loss, _, _, rv, ri, cv, ci = cvig_fov.sharded_match_loss(ov_l, su_l, loss='batch_hard', mined=True, _kernels=BatchHardCpuKernels)
    loss.backward()
    check_ranks([(loss.item(), ov_l.grad, su_l.grad, ri, ci)], ref, W2_B)


# ----------------------------------------------------------------------------- config 3 on 8 rank-threads
C3_B, C3_b, C3_WE = 1024, 128, 4


def test_batch_hard_config3_threaded_world8_equals_single_process():
    ov, su, ties = planted(C3_B, C3_b, C3_WE, 62)
    res = run_ranks(8, lambda rank: _run_rank(ov, su, rank, C3_b))
    ref = single_process(ov, su)
    check_ties(ref, ties)
    check_ranks(res, ref, C3_b)


# ----------------------------------------------------------------------------- C ABI
def test_batch_hard_abi_rejects_bad_arguments_without_gpu():
    from witw_amd import _lib
    lib = _lib.load()
    assert lib.witw_version() >= 200

    def rejects(rc, word):
        assert rc == -1, rc
        msg = lib.witw_last_error()
        assert word in msg, msg

    assert lib.witw_batch_hard_workspace_bytes(1, 1) == -1 and lib.witw_batch_hard_workspace_bytes(8, 0) == -1
    assert lib.witw_batch_hard_workspace_bytes(128, 128) > 0
    # witw_batch_hard_fwd(D, B, alpha, rv, ri, cv, ci, loss, ws, stream)
    rejects(lib.witw_batch_hard_fwd(None, 8, 10., 1, 1, 1, 1, 1, 1, None), b'null')
    rejects(lib.witw_batch_hard_fwd(1, 8, 10., 1, 1, 1, None, 1, 1, None), b'null')
    rejects(lib.witw_batch_hard_fwd(1, 1, 10., 1, 1, 1, 1, 1, 1, None), b'batch')
    # witw_batch_hard_slab_mine(D, Bo, Bs, col0, rv, ri, cv, ci, ws, stream)
    rejects(lib.witw_batch_hard_slab_mine(None, 8, 4, 0, 1, 1, 1, 1, 1, None), b'null')
    rejects(lib.witw_batch_hard_slab_mine(1, 1, 1, 0, 1, 1, 1, 1, 1, None), b'batch')
    rejects(lib.witw_batch_hard_slab_mine(1, 8, 4, 5, 1, 1, 1, 1, 1, None), b'bad slab')      # col0 + b > B
    rejects(lib.witw_batch_hard_slab_mine(1, 8, 0, 0, 1, 1, 1, 1, 1, None), b'bad slab')      # empty slab
    rejects(lib.witw_batch_hard_slab_mine(1, 8, 4, -1, 1, 1, 1, 1, 1, None), b'bad slab')
    # witw_batch_hard_merge_rows(rv_parts, ri_parts, n_parts, B, rv, ri, stream)
    rejects(lib.witw_batch_hard_merge_rows(1, None, 2, 8, 1, 1, None), b'null')
    rejects(lib.witw_batch_hard_merge_rows(1, 1, 2, 1, 1, 1, None), b'batch')
    rejects(lib.witw_batch_hard_merge_rows(1, 1, 0, 8, 1, 1, None), b'shape mismatch')
    # witw_batch_hard_slab_loss(D, rv, cv, Bo, Bs, col0, alpha, partial, stream)
    rejects(lib.witw_batch_hard_slab_loss(1, 1, 1, 8, 4, 0, 10., None, None), b'null')
    rejects(lib.witw_batch_hard_slab_loss(1, 1, 1, 1, 1, 0, 10., 1, None), b'batch')
    rejects(lib.witw_batch_hard_slab_loss(1, 1, 1, 8, 4, 6, 10., 1, None), b'bad slab')
    # witw_batch_hard_pairs(diag, rv, ri, cv, ci, g, B, Bs, col0, alpha, po, ps, pw, stream)
    rejects(lib.witw_batch_hard_pairs(1, 1, 1, 1, 1, None, 8, 4, 0, 10., 1, 1, 1, None), b'null')
    rejects(lib.witw_batch_hard_pairs(1, 1, 1, 1, 1, 1, 1, 1, 0, 10., 1, 1, 1, None), b'batch')
    rejects(lib.witw_batch_hard_pairs(1, 1, 1, 1, 1, 1, 8, 4, 5, 10., 1, 1, 1, None), b'bad slab')
    rejects(lib.witw_batch_hard_pairs(1, 1, 1, 1, 1, 1, 8, 9, 0, 10., 1, 1, 1, None), b'bad slab')
    # witw_batch_hard_bwd(D, rv, ri, cv, ci, g, gD, B, alpha, stream)
    rejects(lib.witw_batch_hard_bwd(1, 1, 1, 1, 1, 1, None, 8, 10., None), b'null')
    rejects(lib.witw_batch_hard_bwd(1, 1, 1, 1, 1, 1, 1, 1, 10., None), b'batch')
    # witw_match_bwd_pairs(ov, su, ori, score, ws, po, ps, pw, n, Bo, Bs, We, gov, gsu, scratch, stream)
    assert lib.witw_match_bwd_pairs_scratch_bytes(0, 8, 8) == -1 and lib.witw_match_bwd_pairs_scratch_bytes(8193, 8, 8) == -1
    assert lib.witw_match_bwd_pairs_scratch_bytes(24, 8, 8) > 0
    rejects(lib.witw_match_bwd_pairs(1, 1, 1, 1, 1, 1, 1, 1, 24, 8, 8, 64, 1, 1, None, None), b'null')
    rejects(lib.witw_match_bwd_pairs(1, 1, 1, None, 1, 1, 1, 1, 24, 8, 8, 64, 1, 1, 1, None), b'null')
    rejects(lib.witw_match_bwd_pairs(1, 1, 1, 1, 1, 1, 1, 1, 24, 8, 8, 65, 1, 1, 1, None), b'bad shape')
    rejects(lib.witw_match_bwd_pairs(1, 1, 1, 1, 1, 1, 1, 1, 24, 0, 8, 64, 1, 1, 1, None), b'bad shape')
    rejects(lib.witw_match_bwd_pairs(1, 1, 1, 1, 1, 1, 1, 1, 0, 8, 8, 64, 1, 1, 1, None), b'pairs')
    rejects(lib.witw_match_bwd_pairs(1, 1, 1, 1, 1, 1, 1, 1, 8193, 8, 8, 64, 1, 1, 1, None), b'pairs')


def test_batch_hard_ops_refuse_cpu_tensors_and_small_batches():
    from witw_amd import _lib, ops
    with pytest.raises(_lib.WitwError):
        ops.batch_hard_fwd(torch.zeros(4, 4))          # no CPU fallback
    from witw_amd import cvig_fov
    with pytest.raises(_lib.WitwError):
        cvig_fov.sharded_match_loss(torch.zeros(2, 16, 4, 64), torch.zeros(2, 16, 4, 64), loss='hardest')


# ----------------------------------------------------------------------------- CLI
@pytest.mark.parametrize('module', ['cvig_fov', 'cvig_semantic'])
def test_loss_flag_sets_globals(module, monkeypatch):
    import importlib
    from witw_amd import cvig_fov
    m = importlib.import_module('witw_amd.' + module)
    assert m.Globals.loss == 'soft_margin'
    calls = []
    monkeypatch.setattr(m.Globals, 'loss', m.Globals.loss)          # restored after the test
    monkeypatch.setattr(m, 'train', lambda **kw: calls.append(('train', m.Globals.loss)))
    monkeypatch.setattr(m, 'test', lambda **kw: calls.append(('test', m.Globals.loss)))
    monkeypatch.setattr(cvig_fov, 'init_distributed', lambda *a, **k: None)
    m.main([])
    assert calls[-1] == ('train', 'soft_margin') and m.Globals.loss == 'soft_margin'
    m.main(['--loss', 'batch_hard'])
    assert calls[-1] == ('train', 'batch_hard') and m.Globals.loss == 'batch_hard'
    with pytest.raises(SystemExit):
        m.main(['--loss', 'semi_hard'])
