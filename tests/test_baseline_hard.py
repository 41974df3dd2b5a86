"""The batch-hard form of cvig_baseline's loss without a GPU: the float64 restatement (tests/baseline_hard_ref.py) against torch
autograd of the definition, the collective choreography of cvig_baseline.sharded_batch_hard_loss (the restatement's CpuKernels for
the six kernel calls) under gloo world 2 and the in-process threaded group with 2 and 8 ranks against the one-process value on the
concatenated batch, the share check, the --loss switch, and the C ABI's argument checks."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import baseline_hard_ref as H
from witw_amd import synth

from .test_baseline_sharded_loss import _free_port
from .threaded_world import run_ranks

B, N = 16, 12
MODES = {'hinge': dict(soft_margin=False, margin=1.0), 'hinge_m03': dict(soft_margin=False, margin=0.3),
         'soft': dict(soft_margin=True, alpha=10.0), 'soft_a2': dict(soft_margin=True, alpha=2.0)}
GRAD_LOSS = 0.37


def _inputs(B=B, n=N, seed=23):
    """-> (surface [B, n], overhead [B, n]) float64: true pairs about 0.5 apart (squared), other rows about 0.6, the hardest ones
    nearer: x = d - min runs over about [-1, 0.9], no term within 2e-2 of a kink, and both margins leave terms active at every B"""
    su = torch.from_numpy(synth.embeddings(seed, 1, (B, n))).double() * (0.3 / n) ** 0.5
    ov = su + torch.from_numpy(synth.embeddings(seed, 2, (B, n))).double() * (0.5 / n) ** 0.5
    return su, ov


def term(x, soft_margin=False, alpha=10.0, margin=1.0):
    return torch.log(1.0 + torch.exp(alpha * x)) if soft_margin else torch.clamp(x + margin, min=0.0)


def _autograd(su, ov, soft_margin=False, alpha=10.0, margin=1.0):
    """masked_fill -> min -> l(...) on T[g][c] = |overhead_g - surface_c|^2, differentiated by torch -> (loss, d surface, d overhead)"""
    y, x = su.clone().requires_grad_(True), ov.clone().requires_grad_(True)
    T = ((x[:, None, :] - y[None, :, :]) ** 2).sum(2)
    Tm = T.masked_fill(torch.eye(T.shape[0], dtype=torch.bool), float('inf'))
    d = torch.diagonal(T)
    loss = (term(d - Tm.min(1)[0], soft_margin, alpha, margin) + term(d - Tm.min(0)[0], soft_margin, alpha, margin)).sum() / (2.0 * T.shape[0])
    (loss * GRAD_LOSS).backward()
    return loss.detach(), y.grad, x.grad


def _close(got, ref, rel=1e-12):
    return float((got - ref).abs().max()) <= rel * float(ref.abs().max())


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('B', [2, 3, 16, 37])
def test_restatement_equals_autograd_of_the_definition(B, mode):
    su, ov = _inputs(B)
    loss, dsu, dov = _autograd(su, ov, **MODES[mode])
    got, dx, dy, (rv, ri, cv, ci), T = H.loss_and_grads(ov, su, GRAD_LOSS, **MODES[mode])
    assert float(loss) > 0 and float(dsu.abs().max()) > 0
    assert abs(float(got) - float(loss)) <= 1e-12 * abs(float(loss))
    assert _close(dx, dov) and _close(dy, dsu)
    # the pair list is the dense dL/dT, which has at most 3B non-zeros, and the mined entries are entries of T
    pg, pc, pw = H.pairs(torch.diagonal(T), rv, ri, cv, ci, torch.tensor(GRAD_LOSS, dtype=torch.float64), 0, **MODES[mode])
    G = H.dense_grad(B, B, pg, pc, pw)
    assert int((G != 0).sum()) <= 3 * B
    Tg = T.clone().requires_grad_(True)
    Tm = Tg.masked_fill(torch.eye(B, dtype=torch.bool), float('inf'))
    d = torch.diagonal(Tg)
    ((term(d - Tm.min(1)[0], **MODES[mode]).sum() + term(d - Tm.min(0)[0], **MODES[mode]).sum()) * (GRAD_LOSS / (2.0 * B))).backward()
    assert _close(G, Tg.grad)
    r = torch.arange(B)
    assert torch.equal(rv, T[r, ri]) and torch.equal(cv, T[ci, r]) and bool((ri != r).all()) and bool((ci != r).all())


def test_restatement_slabs_merge_to_the_whole_matrix():
    """ties across a slab boundary go to the earlier slab, a NaN is the minimum, a one-column slab's own row has (+inf, itself)"""
    su, ov = _inputs(9)
    su[7] = su[1]                   # columns 1 and 7 of T bit-identical: slabs 0 and 2 of width 3
    ov[4, 0] = float('nan')         # row 4 of T all NaN
    T = H.sqdist(ov, su)
    rv, ri, cv, ci = H.mine(T)
    parts = [H.slab_mine(T[:, c0:c0 + 3], c0) for c0 in (0, 3, 6)]
    mv, mi = H.merge_rows(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert torch.equal(mi, ri) and torch.equal(mv.nan_to_num(-1.0), rv.nan_to_num(-1.0))
    assert torch.equal(torch.cat([p[3] for p in parts]), ci)
    assert int(ri[4]) == 0 and bool(torch.isnan(rv[4])) and bool((ci[torch.arange(9) != 4] == 4).all())
    assert not bool(((ri == 7) & (torch.arange(9) != 1)).any())      # column 7 never beats its twin, column 1
    one = H.slab_mine(T[:, 8:9], 8)
    assert float(one[0][8]) == float('inf') and int(one[1][8]) == 8


# ---------------------------------------------------------------------------------------------------------------- N ranks
def _run_rank(su, ov, rank, b, kw):
    from witw_amd import cvig_baseline
    sl = slice(rank * b, (rank + 1) * b)
    s, o = su[sl].clone().requires_grad_(True), ov[sl].clone().requires_grad_(True)
    loss, rv, ri, cv, ci = cvig_baseline.sharded_batch_hard_loss(s, o, mined=True, _kernels=H.CpuKernels, **kw)
    loss.backward(torch.tensor(GRAD_LOSS, dtype=loss.dtype))
    return loss.item(), s.grad.clone(), o.grad.clone(), rv.clone(), ri.clone(), cv.clone(), ci.clone()


def _check_ranks(res, su, ov, b, kw):
    loss, dx, dy, (rv, ri, cv, ci), _T = H.loss_and_grads(ov, su, GRAD_LOSS, **kw)
    assert float(loss) > 0 and float(dx.abs().max()) > 0
    for rank, (got, gs, go, rv_g, ri_g, cv_g, ci_g) in enumerate(res):
        sl = slice(rank * b, (rank + 1) * b)
        assert abs(got - float(loss)) <= 1e-12 * abs(float(loss)), (rank, got, float(loss))
        assert float((gs - dy[sl]).abs().max()) <= 1e-12 * float(dy.abs().max()), rank
        assert float((go - dx[sl]).abs().max()) <= 1e-12 * float(dx.abs().max()), rank
        assert torch.equal(ri_g, ri) and torch.equal(ci_g, ci[sl]) and ri_g.dtype == torch.int64 and ci_g.dtype == torch.int64
        assert torch.equal(rv_g, rv) and torch.equal(cv_g, cv[sl])


def _gloo_worker(rank, world, port, out_q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from witw_amd import _lib, cvig_baseline
        torch.set_num_threads(1)
        su, ov = _inputs()
        out = {mode: _run_rank(su, ov, rank, B // world, kw) for mode, kw in MODES.items()}
        # one rank's form inside a process group: no collective, the whole batch
        s, o = su.clone().requires_grad_(True), ov.clone().requires_grad_(True)
        k = cvig_baseline._hard_kernels
        cvig_baseline._hard_kernels = lambda: H.CpuKernels
        try:
            one = cvig_baseline.batch_hard_triplet_loss(s, o)
        finally:
            cvig_baseline._hard_kernels = k
        one.backward(torch.tensor(GRAD_LOSS, dtype=one.dtype))
        out['one_rank'] = (one.item(), s.grad.clone(), o.grad.clone())
        try:                                                    # 5 + 4 pairs: the share check, raised on both ranks
            lo, hi = (0, 5) if rank == 0 else (5, 9)
            cvig_baseline.sharded_batch_hard_loss(su[lo:hi], ov[lo:hi], _kernels=H.CpuKernels)
            out['unequal'] = None
        except _lib.WitwError as ex:
            out['unequal'] = str(ex)
        out_q.put((rank, {k: (tuple(t.numpy() if isinstance(t, torch.Tensor) else t for t in v) if isinstance(v, tuple) else v)
                          for k, v in out.items()}))             # numpy: no shared-memory handles that die with the sender
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope='module')
def world2():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return [r[1] for r in res]


def _tensors(t):
    return tuple(torch.from_numpy(v) if hasattr(v, 'dtype') and hasattr(v, 'shape') and not isinstance(v, torch.Tensor) else v for v in t)


@pytest.mark.parametrize('mode', sorted(MODES))
def test_sharded_batch_hard_loss_gloo_world2_equals_one_process(world2, mode):
    su, ov = _inputs()
    _check_ranks([_tensors(r[mode]) for r in world2], su, ov, B // 2, MODES[mode])


def test_one_rank_form_inside_a_process_group_takes_no_part_in_it(world2):
    su, ov = _inputs()
    loss, dx, dy, _m, _T = H.loss_and_grads(ov, su, GRAD_LOSS)
    for r in world2:
        got, gs, go = _tensors(r['one_rank'])
        assert abs(got - float(loss)) <= 1e-12 * abs(float(loss)) and _close(gs, dy) and _close(go, dx)


def test_unequal_shares_raise_on_every_rank_gloo(world2):
    assert all(r['unequal'] is not None and 'unequal batch shares' in r['unequal'] and '[5, 4]' in r['unequal'] for r in world2), world2


@pytest.mark.parametrize('mode', ['hinge', 'soft'])
@pytest.mark.parametrize('world', [2, 8])
def test_sharded_batch_hard_loss_rank_threads_equal_one_process(world, mode):
    su, ov = _inputs()
    su[9] = su[2]       # two bit-identical columns of T in different slabs (both worlds): the earlier rank's wins every tie
    res = run_ranks(world, lambda rank: _run_rank(su, ov, rank, B // world, MODES[mode]), timeout=120.0)
    _check_ranks(res, su, ov, B // world, MODES[mode])


def test_unequal_shares_raise_on_every_rank_thread():
    from witw_amd import _lib, cvig_baseline
    su, ov = _inputs()
    spans = [(0, 2), (2, 4), (4, 5)]

    def fn(rank):
        lo, hi = spans[rank]
        try:
            cvig_baseline.sharded_batch_hard_loss(su[lo:hi], ov[lo:hi], _kernels=H.CpuKernels)
        except _lib.WitwError as ex:
            return str(ex)
        return None
    res = run_ranks(3, fn, timeout=120.0)          # returns: no thread was left waiting in a collective
    assert all(m is not None and 'unequal batch shares' in m and '[2, 2, 1]' in m for m in res), res


def test_a_batch_of_one_is_refused_by_name():
    from witw_amd import _lib, cvig_baseline
    su, ov = _inputs()
    with pytest.raises(_lib.WitwError, match='batch 1 < 2'):
        cvig_baseline.sharded_batch_hard_loss(su[:1], ov[:1], _kernels=H.CpuKernels)


# ---------------------------------------------------------------------------------------------------------------- the switch
def test_loss_switch_of_train_and_the_cli(monkeypatch):
    from witw_amd import _lib, cvig_baseline, cvig_fov
    with pytest.raises(_lib.WitwError, match="'exhaustive' or 'batch_hard'"):
        cvig_baseline.train(loss='nonsense')
    calls = []
    monkeypatch.setattr(cvig_baseline, 'train', lambda **kw: calls.append(kw))
    monkeypatch.setattr(cvig_fov, 'init_distributed', lambda *a, **k: None)
    cvig_baseline.main([])
    assert calls[-1] == dict(dataset='cvusa', loss='exhaustive')
    cvig_baseline.main(['--loss', 'batch_hard', '--dataset', 'witw'])
    assert calls[-1] == dict(dataset='witw', loss='batch_hard')
    with pytest.raises(SystemExit):
        cvig_baseline.main(['--loss', 'x'])
    assert len(calls) == 2


def test_wrappers_refuse_cpu_tensors():
    from witw_amd import _lib, baseline_hard, cvig_baseline
    su, ov = _inputs()
    f = su.float()
    with pytest.raises(_lib.WitwError, match='no CPU fallback'):
        baseline_hard.hard_slab_loss(f @ f.t(), f[:, 0], f[:, 0], 0)
    with pytest.raises(_lib.WitwError, match='no CPU fallback'):
        baseline_hard.sqdist_pairs_bwd(f, f, torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0))
    with pytest.raises(_lib.WitwError, match='no CPU fallback'):
        cvig_baseline.batch_hard_triplet_loss(f, ov.float())


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_abi_rejects_bad_arguments_without_gpu():
    from witw_amd import _lib
    lib = _lib.load()

    def rejects(rc, word):
        assert rc == -1, rc
        msg = lib.witw_last_error()
        assert word in msg, msg

    # witw_baseline_hard_slab_loss(T, rv, cv, B, b, col0, soft, alpha, margin, partial, stream)
    rejects(lib.witw_baseline_hard_slab_loss(1, 1, 1, 8, 4, 0, 0, 10., 1., None, None), b'null')
    rejects(lib.witw_baseline_hard_slab_loss(None, 1, 1, 8, 4, 0, 0, 10., 1., 1, None), b'null')
    rejects(lib.witw_baseline_hard_slab_loss(1, 1, 1, 1, 1, 0, 0, 10., 1., 1, None), b'batch 1 < 2')
    rejects(lib.witw_baseline_hard_slab_loss(1, 1, 1, 8, 4, 5, 1, 10., 1., 1, None), b'bad slab')       # col0 + b > B
    rejects(lib.witw_baseline_hard_slab_loss(1, 1, 1, 8, 0, 0, 1, 10., 1., 1, None), b'bad slab')       # empty slab
    rejects(lib.witw_baseline_hard_slab_loss(1, 1, 1, 8, 4, -1, 1, 10., 1., 1, None), b'bad slab')
    # witw_baseline_hard_pairs(diag, rv, ri, cv, ci, g, B, b, col0, soft, alpha, margin, pg, pc, pw, stream)
    rejects(lib.witw_baseline_hard_pairs(1, 1, 1, 1, 1, None, 8, 4, 0, 0, 10., 1., 1, 1, 1, None), b'null')
    rejects(lib.witw_baseline_hard_pairs(1, 1, 1, 1, 1, 1, 8, 4, 0, 0, 10., 1., 1, None, 1, None), b'null')
    rejects(lib.witw_baseline_hard_pairs(1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 10., 1., 1, 1, 1, None), b'batch 1 < 2')
    rejects(lib.witw_baseline_hard_pairs(1, 1, 1, 1, 1, 1, 8, 9, 0, 0, 10., 1., 1, 1, 1, None), b'bad slab')
    rejects(lib.witw_baseline_hard_pairs(1, 1, 1, 1, 1, 1, 8, 4, 5, 0, 10., 1., 1, 1, 1, None), b'bad slab')
    # witw_sqdist_pairs_bwd(x, y, pg, pc, pw, P, dx, dy, B, b, n, workspace, stream) and its workspace query
    assert lib.witw_sqdist_pairs_bwd_workspace_bytes(0, 4, 3) == -1 and lib.witw_sqdist_pairs_bwd_workspace_bytes(4, 0, 3) == -1
    assert lib.witw_sqdist_pairs_bwd_workspace_bytes(4, 4, -1) == -1
    assert lib.witw_sqdist_pairs_bwd_workspace_bytes(1024, 128, 1280) >= 0 and lib.witw_sqdist_pairs_bwd_workspace_bytes(1, 1, 0) >= 0
    rejects(lib.witw_sqdist_pairs_bwd(1, 1, 1, 1, 1, 3, None, None, 4, 4, 8, None, None), b'dx and dy')      # NULL / NULL
    rejects(lib.witw_sqdist_pairs_bwd(None, 1, 1, 1, 1, 3, 1, 1, 4, 4, 8, None, None), b'null')
    rejects(lib.witw_sqdist_pairs_bwd(1, 1, None, 1, 1, 3, 1, 1, 4, 4, 8, None, None), b'null')             # a list of 3 needs its arrays
    rejects(lib.witw_sqdist_pairs_bwd(1, 1, 1, 1, 1, 3, 1, 1, 4, 4, 0, None, None), b'bad shape')
    rejects(lib.witw_sqdist_pairs_bwd(1, 1, 1, 1, 1, 3, 1, 1, 4, 4, 12289, None, None), b'bad shape')
    rejects(lib.witw_sqdist_pairs_bwd(1, 1, 1, 1, 1, 3, 1, 1, 0, 4, 8, None, None), b'bad shape')
    rejects(lib.witw_sqdist_pairs_bwd(1, 1, 1, 1, 1, -1, 1, 1, 4, 4, 8, None, None), b'pairs')
    with pytest.raises(_lib.WitwError):
        _lib.check(-1, 'witw_sqdist_pairs_bwd')
