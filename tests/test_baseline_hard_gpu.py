"""The batch-hard form of cvig_baseline's loss on the GPU: csrc/baseline_loss_hard.hip through witw_amd/baseline_hard.py, the mining
entries of csrc/loss_hard.hip on the baseline's squared distances, and cvig_baseline.batch_hard_triplet_loss /
sharded_batch_hard_loss / the training step on top of them, against the float64 restatement tests/baseline_hard_ref.py.

Inputs (hard_inputs): clustered embeddings built as loss_inputs of tests/test_baseline_head_gpu.py builds them, the seed advanced
on the CPU until the float64 reference has, in every row and column, its minimum at least GAP = 1e-4 (relative) below the
runner-up, and no hard-margin term (margins 1 and 0.3) within KINK = 1e-4 of its kink. fp32 distances err by about 1e-6, so fp32
mining cannot legitimately differ: the mined indices of ALL rows and columns must equal the reference's, none is excused.

Bounds, none taken from a kernel's output: loss 1e-4 relative; dx summed over the slabs, and dy, within 2e-5 of the largest entry of
the float64 gradient; pair weights exact for the hard margin (0, sc or 2 sc in fp32, sc = fp32(grad_loss) / fp32(2B)) and 1e-5 of
each element for the soft margin; rv / cv bitwise the entries of T at the mined indices; the training step by the project's
training-step criterion, every parameter gradient within 1e-4 of its norm (the BatchNorm caveat of
tests/test_baseline_sharded_loss_gpu.py applies: one deep copy of the encoders per sub-batch stands for the replicas, 4 images per
rank keep the last blocks' statistics from degenerating). Every test prints its figures before it asserts.

Measured on an MI355X (worst over the cases of each test, as fractions of the scale the bound is relative to):

  quantity                                              bound    kernel
  mined indices that differ from float64 (72 cases)     0        0
  slab loss, all partitions                             1e-4     1.1e-6
  pair weights per element                              1e-5     9.0e-6 (soft margin; hard margin exact) -- close to the bound: a weight's
                                                                 relative error is alpha x the error of d - min, and the smallest weights
                                                                 (alpha x about -2) carry the whole of it
  dx summed over slabs / dy                             2e-5     1.2e-6 / 9.9e-7
  pair-list backward alone: dx / dy                     2e-5     4.7e-7 / 4.5e-7
  world of one: loss / d surface / d overhead           1e-4 / 2e-5    4.7e-7 / 4.4e-7 / 6.5e-7
  rank-threads (2, 8): loss / d surface / d overhead    1e-4 / 2e-5    1.1e-7 / 2.0e-7 / 5.2e-7
  training step, two rank-threads: loss                 1e-4     equal to 7 digits
  training step: worst parameter gradient               1e-4     2.9e-6 of its norm

Shapes. (B, b, col0): (2, 2, 0) the smallest batch; (3, 1, 2) a one-column last slab whose only candidate for row 2 is its own
masked diagonal (+inf): the merge must take another slab's; (37, 37, 0) / (37, 5, 32) a ragged partition; (300, 44, 256) above the
256-thread stride and off the 64-row column-partial tile; (257, 1, 256) one column per slab. n = 8, n = 13 (off any vector width)
and n = 1536 (the embedding width: 6 column tiles of the pair-list backward)."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import baseline_hard_ref as H
from tests.mem_arena import Arena, ArenaTorch
from tests.test_baseline_head_gpu import GRAD_LOSS, LOSS_CFGS

from .threaded_world import run_ranks

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SLABS = [(2, 2, 0), (3, 1, 2), (37, 37, 0), (37, 5, 32), (300, 44, 256), (257, 1, 256)]
GAP, KINK = 1e-4, 1e-4
MARGINS = (1.0, 0.3)


def _cfg(cfg):
    kw = dict(soft_margin=False, alpha=10.0, margin=1.0)
    kw.update(LOSS_CFGS[cfg])
    return kw


def _gaps(T):
    """float64 T [B, B] -> (smallest relative gap between a row's / column's minimum and its runner-up, smallest distance of a
    hard-margin term from its kink, whether each margin leaves a term active)"""
    B = T.shape[0]
    Tm = T.masked_fill(torch.eye(B, dtype=torch.bool), float('inf'))
    gap = float('inf')
    for M in (Tm, Tm.t()):
        two = torch.topk(M, 2, dim=1, largest=False)[0]
        fin = torch.isfinite(two[:, 1])
        if bool(fin.any()):
            gap = min(gap, float(((two[fin, 1] - two[fin, 0]) / two[fin, 1]).min()))
    d = torch.diagonal(T)
    x = torch.cat([d - Tm.min(1)[0], d - Tm.min(0)[0]])
    return gap, min(float((x + m).abs().min()) for m in MARGINS), all(bool((x + m > 0).any()) for m in MARGINS)


@functools.lru_cache(maxsize=None)
def hard_inputs(B, n):
    """-> (x [B, n] rows of T, y [B, n] columns, seed, gap, kink): clusters of about 8 rows 3 apart on axis 0, |x_i - x_j|^2 ~ 0.6
    inside a cluster, true-pair distance^2 spread over [0.05, 1.5]"""
    K = (B + 7) // 8
    for seed in range(64):
        g = np.random.default_rng([411, B, n, seed])
        x = torch.from_numpy((g.standard_normal((B, n)) * (0.3 / n) ** 0.5).astype(np.float32))
        x[:, 0] += 3.0 * (torch.arange(B) % K).float()
        t = torch.from_numpy(g.uniform(0.05, 1.5, (B, 1)).astype(np.float32)).sqrt()
        y = x + t * torch.from_numpy((g.standard_normal((B, n)) * n ** -0.5).astype(np.float32))
        gap, kink, active = _gaps(H.sqdist(x.double(), y.double()))
        if gap >= GAP and kink > KINK and active:
            return x, y, seed, gap, kink
    raise AssertionError('no seed keeps the minima %g apart and the terms clear of the kink at B=%d n=%d' % (GAP, B, n))


@functools.lru_cache(maxsize=None)
def hard_refs(B, n, cfg):
    """float64 (loss, dx, dy, (rv, ri, cv, ci), T) of the whole batch; shared, never modified"""
    x, y, _seed, gap, kink = hard_inputs(B, n)
    assert gap >= GAP and kink > KINK
    return H.loss_and_grads(x.double(), y.double(), GRAD_LOSS, **_cfg(cfg))


def _partition(B, b, col0):
    out, c = [], 0
    while c < col0:
        out.append((c, min(b, col0 - c)))
        c += out[-1][1]
    out.append((col0, b))
    assert col0 + b == B
    return out


def _relmax(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _run_slabs(x, y, parts, kw):
    """every slab of the partition on the GPU, the exchanges of the ranks done by hand -> dict(loss, T {col0}, slab_rows {col0:
    (rv, ri)}, rv, ri [B] merged, cv, ci [B] concatenated, pairs {col0: (pg, pc, pw)}, dx [B, n] summed in fp32, dy [B, n])"""
    from witw_amd import baseline_hard as bh
    from witw_amd import ops
    B = x.shape[0]
    gl = torch.tensor([GRAD_LOSS], device=x.device)
    ys = {c0: y[c0:c0 + w].contiguous() for c0, w in parts}
    T = {c0: ops.pairwise_sqdist(x, ys[c0]) for c0, _w in parts}
    diag = torch.cat([T[c0][c0:c0 + w].diagonal() for c0, w in parts]).contiguous()                     # the all-gather
    mined = {c0: ops.batch_hard_slab_mine(T[c0], c0) for c0, _w in parts}
    rv, ri = ops.batch_hard_merge_rows(torch.stack([mined[c0][0] for c0, _w in parts]),               # the all-gather of [w, B]
                                       torch.stack([mined[c0][1] for c0, _w in parts]))
    partial = sum(bh.hard_slab_loss(T[c0], rv, mined[c0][2], c0, **kw) for c0, _w in parts)            # the all-reduce
    pairs, dx, dy = {}, torch.zeros_like(x), []
    for c0, _w in parts:
        pairs[c0] = bh.hard_pairs(diag, rv, ri, mined[c0][2], mined[c0][3], gl, c0, **kw)
        gx, gy = bh.sqdist_pairs_bwd(x, ys[c0], *pairs[c0])
        dx += gx                                                                                        # the reduce-scatter's sum
        dy.append(gy)
    return dict(loss=partial / (2.0 * B), T=T, slab_rows={c0: mined[c0][:2] for c0, _w in parts}, rv=rv, ri=ri,
                cv=torch.cat([mined[c0][2] for c0, _w in parts]), ci=torch.cat([mined[c0][3] for c0, _w in parts]), pairs=pairs, dx=dx,
                dy=torch.cat(dy))


@pytest.mark.parametrize('cfg', sorted(LOSS_CFGS))
@pytest.mark.parametrize('n', [8, 13, 1536])
@pytest.mark.parametrize('B,b,col0', SLABS)
def test_slab_kernels_against_float64(B, b, col0, n, cfg):
    x, y, seed, gap, kink = hard_inputs(B, n)
    loss, dx, dy, (rv, ri, cv, ci), T64 = hard_refs(B, n, cfg)
    kw = _cfg(cfg)
    parts = _partition(B, b, col0)
    got = _run_slabs(x.to(DEV), y.to(DEV), parts, kw)
    torch.cuda.synchronize()
    Tg = torch.cat([got['T'][c0] for c0, _w in parts], 1).cpu()
    r = torch.arange(B)
    # mining: every index the reference's, every value an entry of the fp32 T, bit for bit
    wrong = int((got['ri'].cpu() != ri).sum()) + int((got['ci'].cpu() != ci).sum())
    print('slabs B=%d b=%d col0=%d n=%d %s (%d slabs, seed %d, gap %.1e, kink %.1e): %d of %d mined indices differ from float64'
          % (B, b, col0, n, cfg, len(parts), seed, gap, kink, wrong, 2 * B))
    assert wrong == 0
    assert torch.equal(_bits(got['rv'].cpu()), _bits(Tg[r, ri])) and torch.equal(_bits(got['cv'].cpu()), _bits(Tg[ci, r]))
    if b == 1:      # the one-column slab that holds column col0: row col0 has only its masked diagonal there
        v, i = got['slab_rows'][col0]
        assert float(v[col0]) == float('inf') and int(got['ri'][col0]) != col0 and int(i[col0]) in (-1, col0)
    # pair lists: indices exact, weights exact (hard margin) or 1e-5 of each element
    sc32 = np.float32(GRAD_LOSS) / np.float32(2.0 * B)
    e_w = 0.0
    for c0, w in parts:
        pg, pc, pw = (t.cpu() for t in got['pairs'][c0])
        rg, rc, rw = H.pairs(torch.diagonal(T64), rv, ri, cv[c0:c0 + w], ci[c0:c0 + w], torch.tensor(GRAD_LOSS, dtype=torch.float64), c0, **kw)
        assert pg.dtype == torch.int32 and pg.numel() == 2 * w + B
        assert torch.equal(pg, rg) and torch.equal(pc, rc), c0
        if kw['soft_margin']:
            err = (pw.double() - rw).abs() / rw.abs().clamp(min=1e-300)          # an exact zero must be an exact zero
            e_w = max(e_w, float(err.max()))
        else:
            units = torch.round(rw / (GRAD_LOSS / (2.0 * B)))                    # -1, 0, 1 or 2 times sc
            want = torch.from_numpy((units.numpy().astype(np.float32) * sc32).astype(np.float32))
            assert torch.equal(pw, want), c0
    e_loss = abs(got['loss'].item() - loss.item()) / abs(loss.item())
    e1, e2 = _relmax(got['dx'], dx), _relmax(got['dy'], dy)
    print('  loss %.6e rel err %.1e; soft pair weights %.1e per element; dx %.1e dy %.1e of their max' % (loss.item(), e_loss, e_w, e1, e2))
    assert float(loss) > 0 and float(dx.abs().max()) > 0
    assert e_loss <= 1e-4
    assert e_w <= 1e-5
    assert e1 <= 2e-5 and e2 <= 2e-5


def test_same_call_twice_gives_the_same_bits():
    B, b, col0, n = 300, 44, 256, 1536
    x, y = (t.to(DEV) for t in hard_inputs(B, n)[:2])
    for cfg in ('hard_m1', 'soft_a10'):
        runs = [_run_slabs(x, y, _partition(B, b, col0), _cfg(cfg)) for _ in range(2)]
        torch.cuda.synchronize()
        for key in ('loss', 'rv', 'ri', 'cv', 'ci', 'dx', 'dy'):
            assert torch.equal(_bits(runs[0][key]), _bits(runs[1][key])), key


# ---------------------------------------------------------------------------------------------------------------- exact selection
def test_ties_go_to_the_lowest_index_and_a_nan_is_the_minimum():
    """constructed, not random: bit-identical y rows (two columns of T identical) inside a slab and across a slab boundary,
    bit-identical x rows, and one NaN embedding row; two slabs of 6 columns, n = 13"""
    B, b, n = 12, 6, 13
    g = np.random.default_rng(5)
    x = torch.from_numpy(g.standard_normal((B, n)).astype(np.float32))
    y = torch.from_numpy(g.standard_normal((B, n)).astype(np.float32))
    near = lambda t, k: t + 0.01 * torch.from_numpy(g.standard_normal(n).astype(np.float32)) * k      # noqa: E731
    y[2] = near(x[4], 1)
    y[5] = y[2]                 # row 4: columns 2 and 5 identical, both in slab 0 -> 2
    y[3] = near(x[9], 1)
    y[8] = y[3]                 # row 9: columns 3 (slab 0) and 8 (slab 1) identical -> 3, by the merge
    x[7] = near(y[1], 1)
    x[10] = x[7]                # column 1: rows 7 and 10 identical -> 7
    for nan_row in (None, 6):
        xx = x.clone()
        if nan_row is not None:
            xx[nan_row] = float('nan')
        xd, yd = xx.to(DEV), y.to(DEV)
        parts = [(0, b), (b, b)]
        got = _run_slabs(xd, yd, parts, _cfg('hard_m1'))
        soft = _run_slabs(xd, yd, parts, _cfg('soft_a10'))
        torch.cuda.synchronize()
        Tg = torch.cat([got['T'][0], got['T'][b]], 1).cpu()
        assert torch.equal(_bits(Tg[:, 2]), _bits(Tg[:, 5])) and torch.equal(_bits(Tg[:, 3]), _bits(Tg[:, 8]))
        assert torch.equal(_bits(Tg[7]), _bits(Tg[10]))
        ri, ci = got['ri'].cpu(), got['ci'].cpu()
        # the restatement on the GPU's own fp32 T: same values, so the same selection, index for index and bit for bit
        rv_r, ri_r, cv_r, ci_r = H.mine(Tg)
        print('nan row %s: ri %s ci %s' % (nan_row, ri.tolist(), ci.tolist()))
        assert torch.equal(ri, ri_r) and torch.equal(ci, ci_r)
        assert torch.equal(_bits(got['rv'].cpu().nan_to_num(-1.0)), _bits(rv_r.nan_to_num(-1.0)))
        assert torch.equal(_bits(got['cv'].cpu().nan_to_num(-1.0)), _bits(cv_r.nan_to_num(-1.0)))
        assert int(ri[4]) == 2 and int(ri[9]) == 3 and int(ci[1]) == (7 if nan_row is None else nan_row)
        assert int(got['slab_rows'][b][1][9]) == 8          # slab 1 on its own finds the twin; the earlier rank wins the merge
        if nan_row is None:
            assert bool(torch.isfinite(got['loss']).all()) and not bool(torch.isnan(soft['loss']).any())     # soft: exp as written may overflow
        else:
            others = torch.arange(B) != nan_row
            assert int(ri[nan_row]) == 0 and bool(torch.isnan(got['rv'][nan_row]))             # the first NaN of row 6 is column 0
            assert bool((ci[others] == nan_row).all()) and bool(torch.isnan(got['cv'].cpu()[others]).all())
            assert bool(torch.isnan(got['loss']).all()) and bool(torch.isnan(soft['loss']).all())

# ---------------------------------------------------------------------------------------------------------------- pair-list backward
def _pairs_bwd_case(name):
    g = np.random.default_rng(9)
    B, b, n = (300, 44, 1536) if name in ('hub', 'random') else (37, 5, 13)
    x = torch.from_numpy(g.standard_normal((B, n)).astype(np.float32))
    y = torch.from_numpy(g.standard_normal((b, n)).astype(np.float32))
    P = 3 * B
    pg = torch.from_numpy(g.integers(0, B, P).astype(np.int32))
    pc = torch.from_numpy(g.integers(0, b, P).astype(np.int32))
    pw = torch.from_numpy(g.standard_normal(P).astype(np.float32))
    if name == 'empty':
        pg, pc, pw = pg[:0], pc[:0], pw[:0]
    elif name == 'skipped':                                     # (-1, -1, w), and indices past either end
        pg[::3], pc[::3] = -1, -1
        pg[1], pc[2] = B, b
        pg[4], pc[5] = -7, 1 << 20
    elif name == 'duplicates':
        pg[:40], pc[:40] = 3, 2                                 # one pair forty times ...
        pg[40:80] = 11                                          # ... and one row forty times
    elif name == 'hub':                                         # every row paired with column 0: one dy row collects all B pairs
        pg, pc, pw = torch.arange(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32), pw[:B]
    return x, y, pg, pc, pw


@pytest.mark.parametrize('name', ['empty', 'skipped', 'duplicates', 'hub', 'random'])
def test_sqdist_pairs_bwd_against_float64(name):
    from witw_amd import baseline_hard as bh
    x, y, pg, pc, pw = _pairs_bwd_case(name)
    dx64, dy64 = H.sqdist_pairs_bwd(x.double(), y.double(), pg, pc, pw.double())
    dev = [t.to(DEV) for t in (x, y, pg, pc, pw)]
    dx, dy = bh.sqdist_pairs_bwd(*dev)
    dx1, none1 = bh.sqdist_pairs_bwd(*dev, need_dy=False)
    none2, dy2 = bh.sqdist_pairs_bwd(*dev, need_dx=False)
    dx3, dy3 = bh.sqdist_pairs_bwd(*dev)
    torch.cuda.synchronize()
    assert none1 is None and none2 is None
    for a, c in ((dx, dx1), (dx, dx3), (dy, dy2), (dy, dy3)):                    # one output alone, and a second run: the same bits
        assert torch.equal(_bits(a), _bits(c))
    if name == 'empty':
        print('P = 0: every row zero')
        assert not bool(dx.any()) and not bool(dy.any()) and not bool(dx64.any())
        return
    scale = max(float(dx64.abs().max()), float(dy64.abs().max()))
    e1, e2 = float((dx.cpu().double() - dx64).abs().max()) / scale, float((dy.cpu().double() - dy64).abs().max()) / scale
    zero_rows = (dx64 == 0).all(1)
    print('%s B=%d b=%d n=%d P=%d: dx %.1e dy %.1e of the largest entry; %d rows of dx without a pair'
          % (name, x.shape[0], y.shape[0], x.shape[1], pg.numel(), e1, e2, int(zero_rows.sum())))
    assert e1 <= 2e-5 and e2 <= 2e-5
    assert not bool(dx.cpu()[zero_rows].any())                                  # rows without a pair are written, as zeros
    if name == 'hub':
        assert not bool(dy.cpu()[1:].any()) and bool(dy.cpu()[0].any())


# ---------------------------------------------------------------------------------------------------------------- end to end
def _check_mined(out, ref, sl):
    rv, ri, cv, ci = ref
    assert torch.equal(out[1].cpu(), ri) and torch.equal(out[3].cpu(), ci[sl]) and out[1].dtype == torch.int64
    assert float((out[0].cpu().double() - rv).abs().max()) <= 1e-5 * float(rv.abs().max())
    assert float((out[2].cpu().double() - cv[sl]).abs().max()) <= 1e-5 * float(cv.abs().max())


@pytest.mark.parametrize('cfg', sorted(LOSS_CFGS))
@pytest.mark.parametrize('B', [2, 37, 257])
def test_world_of_one_and_the_one_rank_form(B, cfg):
    from witw_amd import cvig_baseline, ops, parallel
    assert parallel.world() == 1
    n = 1536
    x, y, _seed, _gap, _kink = hard_inputs(B, n)
    loss, dx, dy, mined, _T = hard_refs(B, n, cfg)
    worst = [0.0, 0.0, 0.0]
    for form in ('sharded', 'one_rank'):
        su, ov = y.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
        if form == 'sharded':
            got, *m = cvig_baseline.sharded_batch_hard_loss(su, ov, mined=True, **LOSS_CFGS[cfg])
            _check_mined(m, mined, slice(0, B))
        else:
            got = cvig_baseline.batch_hard_triplet_loss(su, ov, **LOSS_CFGS[cfg])
        assert ops.last_kernel_variant() == 'baseline_hard_loss_kernel'
        with torch.autograd.set_multithreading_enabled(False):      # the variant is recorded per calling thread: keep the backward on this one
            got.backward(torch.tensor(GRAD_LOSS, device=DEV))
        assert ops.last_kernel_variant() == 'sqdist_pairs_bwd_kernel<dx:1,dy:1>'
        assert got.dim() == 0
        worst = [max(a, c) for a, c in zip(worst, (abs(got.item() - loss.item()) / abs(loss.item()), _relmax(su.grad, dy), _relmax(ov.grad, dx)))]
    print('world of one B=%d %s: loss rel err %.1e; d surface %.1e d overhead %.1e of their max' % (B, cfg, *worst))
    assert worst[0] <= 1e-4 and worst[1] <= 2e-5 and worst[2] <= 2e-5


@pytest.mark.parametrize('cfg', ['hard_m1', 'soft_a10'])
@pytest.mark.parametrize('B', [16, 40])
@pytest.mark.parametrize('world', [2, 8])
def test_rank_threads_hold_the_global_loss_and_their_gradient_rows(world, B, cfg):
    from witw_amd import cvig_baseline
    n, b = 1536, B // world
    x, y, _seed, _gap, _kink = hard_inputs(B, n)
    loss, dx, dy, mined, _T = hard_refs(B, n, cfg)
    xd, yd = x.to(DEV), y.to(DEV)

    def fn(rank):
        torch.cuda.set_device(DEV)
        sl = slice(rank * b, (rank + 1) * b)
        su, ov = yd[sl].clone().requires_grad_(True), xd[sl].clone().requires_grad_(True)
        got, *m = cvig_baseline.sharded_batch_hard_loss(su, ov, mined=True, **LOSS_CFGS[cfg])
        got.backward(torch.tensor(GRAD_LOSS, device=DEV))
        torch.cuda.synchronize()
        return got.item(), su.grad.cpu(), ov.grad.cpu(), [t.cpu() for t in m]
    res = run_ranks(world, fn, timeout=120.0)
    worst = [0.0, 0.0, 0.0]
    for rank, (got, gsu, gov, m) in enumerate(res):
        sl = slice(rank * b, (rank + 1) * b)
        _check_mined(m, mined, sl)
        worst[0] = max(worst[0], abs(got - loss.item()) / abs(loss.item()))
        worst[1] = max(worst[1], float((gsu.double() - dy[sl]).abs().max() / dy.abs().max()))
        worst[2] = max(worst[2], float((gov.double() - dx[sl]).abs().max() / dx.abs().max()))
    print('world %d B=%d %s: loss rel err %.1e; d surface %.1e, reduce-scattered d overhead %.1e of the gradients\' max' % (world, B, cfg, *worst))
    assert worst[0] <= 1e-4 and worst[1] <= 2e-5 and worst[2] <= 2e-5


def test_unequal_shares_raise_on_every_rank():
    from witw_amd import _lib, cvig_baseline
    x, y = (t.to(DEV) for t in hard_inputs(37, 1536)[:2])
    spans = [(0, 2), (2, 4), (4, 5)]

    def fn(rank):
        torch.cuda.set_device(DEV)
        lo, hi = spans[rank]
        try:
            cvig_baseline.sharded_batch_hard_loss(y[lo:hi].contiguous(), x[lo:hi].contiguous())
        except _lib.WitwError as ex:
            return str(ex)
        return None
    res = run_ranks(3, fn, timeout=120.0)          # returns: no thread was left waiting in a collective
    assert all(m is not None and 'unequal batch shares' in m and '[2, 2, 1]' in m for m in res), res


def test_training_step_on_two_rank_threads_is_the_two_replica_step():
    """encoders -> sharded_batch_hard_loss -> backward -> OverlappedGradReducer on two rank-threads of 4 images each, against the
    single-process form of the same semantics: one deep copy of the encoders per sub-batch (each keeps its own batch statistics),
    batch_hard_triplet_loss on the concatenated embeddings, the copies' parameter gradients summed."""
    from witw_amd import cvig_baseline, parallel, synth
    torch.manual_seed(3)
    se0, oe0 = cvig_baseline.SurfaceEncoder().to(DEV).train(), cvig_baseline.OverheadEncoder().to(DEV).train()
    xs = torch.from_numpy(synth.images_u8(22, 1, (8, 3, 382, 382))).to(DEV)
    xo = torch.from_numpy(synth.images_u8(22, 2, (8, 3, 382, 382))).to(DEV)
    copies = [(copy.deepcopy(se0), copy.deepcopy(oe0)) for _ in range(2)]
    su = torch.cat([copies[k][0](xs[4 * k:4 * k + 4]) for k in range(2)])
    ov = torch.cat([copies[k][1](xo[4 * k:4 * k + 4]) for k in range(2)])
    ref_loss = cvig_baseline.batch_hard_triplet_loss(su, ov)
    ref_loss.backward()
    torch.cuda.synchronize()
    ref_grads = [(pa.grad + pb.grad).double().cpu() for e in range(2) for pa, pb in zip(copies[0][e].parameters(), copies[1][e].parameters())]
    names = [side + '.' + nm for side, enc in (('surface', se0), ('overhead', oe0)) for nm, _p in enc.named_parameters()]

    def fn(rank):
        torch.cuda.set_device(DEV)
        se, oe = copy.deepcopy(se0), copy.deepcopy(oe0)
        reducer = parallel.OverlappedGradReducer([se, oe])
        sl = slice(4 * rank, 4 * rank + 4)
        loss = cvig_baseline.sharded_batch_hard_loss(se(xs[sl]), oe(xo[sl]))
        loss.backward()
        reducer.wait()
        grads = [p.grad.double().cpu() for p in list(se.parameters()) + list(oe.parameters())]
        torch.cuda.synchronize()
        reducer.close()
        return loss.item(), grads
    res = run_ranks(2, fn, timeout=300.0)
    worst = (0.0, '')
    for rank, (loss, grads) in enumerate(res):
        print('rank %d: loss %.6f (two-replica form %.6f)' % (rank, loss, ref_loss.item()))
        assert abs(loss - ref_loss.item()) <= 1e-4 * abs(ref_loss.item())
        devs = [(float((g - gr).norm() / gr.norm()), name) for name, g, gr in zip(names, grads, ref_grads)]
        worst = max([worst] + devs)
        print('rank %d: worst parameter-gradient deviation %.2e of its norm (%s)' % ((rank,) + max(devs)))
        for dev, name in devs:
            assert dev <= 1e-4, (rank, name, dev)
    assert all(float(gr.norm()) > 0 for gr in ref_grads)
    print('worst parameter-gradient deviation %.2e of its norm (%s)' % worst)


# ---------------------------------------------------------------------------------------------------------------- memory contract
def _contract_cases(B, b, col0, n, kw):
    """name -> (inputs {name: tensor}, call(bh, placed inputs) -> outputs) for the three wrappers at one shape"""
    from witw_amd import baseline_hard as bh
    from witw_amd import ops
    x, y = (t.to(DEV) for t in hard_inputs(B, n)[:2])
    ys = y[col0:col0 + b].contiguous()
    T = ops.pairwise_sqdist(x, ys)
    diag = torch.diagonal(ops.pairwise_sqdist(x, y)).contiguous()
    rv, ri, _cv, _ci = ops.batch_hard_slab_mine(ops.pairwise_sqdist(x, y), 0)
    _rv, _ri, cv, ci = ops.batch_hard_slab_mine(T, col0)
    gl = torch.tensor([GRAD_LOSS], device=DEV)
    pg, pc, pw = bh.hard_pairs(diag, rv, ri, cv, ci, gl, col0, **kw)
    none = dict(x=x, y=ys, pg=pg[:0].clone(), pc=pc[:0].clone(), pw=pw[:0].clone())
    return {
        'loss': (dict(T=T, rv=rv, cv=cv), lambda m, p: m.hard_slab_loss(p['T'], p['rv'], p['cv'], col0, **kw)),
        'pairs': (dict(diag=diag, rv=rv, ri=ri, cv=cv, ci=ci, gl=gl),
                  lambda m, p: m.hard_pairs(p['diag'], p['rv'], p['ri'], p['cv'], p['ci'], p['gl'], col0, **kw)),
        'bwd': (dict(x=x, y=ys, pg=pg, pc=pc, pw=pw), lambda m, p: m.sqdist_pairs_bwd(p['x'], p['y'], p['pg'], p['pc'], p['pw'])),
        'bwd_dx': (dict(x=x, y=ys, pg=pg, pc=pc, pw=pw), lambda m, p: m.sqdist_pairs_bwd(p['x'], p['y'], p['pg'], p['pc'], p['pw'], need_dy=False)[0]),
        'bwd_dy': (dict(x=x, y=ys, pg=pg, pc=pc, pw=pw), lambda m, p: m.sqdist_pairs_bwd(p['x'], p['y'], p['pg'], p['pc'], p['pw'], need_dx=False)[1]),
        'bwd_none': (none, lambda m, p: m.sqdist_pairs_bwd(p['x'], p['y'], p['pg'], p['pc'], p['pw'])),
    }


@pytest.mark.parametrize('skew', [0, 16])
@pytest.mark.parametrize('cfg', ['hard_m1', 'soft_a10'])
@pytest.mark.parametrize('B,b,col0,n', [(2, 1, 1, 8), (37, 5, 32, 13), (300, 44, 256, 1536)], ids=['2x1x8', '37x5x13', '300x44x1536'])
def test_memory_contract_of_the_wrappers(B, b, col0, n, cfg, skew, monkeypatch):
    """Every wrapper of baseline_hard between guard bands (tests/mem_arena.py): inputs inside NaN bands, every device allocation
    of the wrapper inside guard bands with a canary payload. No band is touched, every output element is stored (rows without a
    pair as zeros), the inputs are unchanged and the values are those of ordinary allocations, bit for bit."""
    from witw_amd import baseline_hard as bh
    for name, (inputs, call) in _contract_cases(B, b, col0, n, _cfg(cfg)).items():
        plain = call(bh, inputs)
        plain = [t.clone() for t in (plain if isinstance(plain, tuple) else (plain,))]
        arena = Arena(DEV, skew_bytes=skew)
        with monkeypatch.context() as m:
            m.setattr(bh, 'torch', ArenaTorch(arena))
            placed = {k: arena.place(t, k) for k, t in inputs.items()}
            got = call(bh, placed)
        arena.check(got)
        got = got if isinstance(got, tuple) else (got,)
        assert len(got) == len(plain)
        for a, c in zip(got, plain):
            assert torch.equal(_bits(a), _bits(c)), name
        for k, t in inputs.items():
            assert torch.equal(_bits(placed[k]), _bits(t)), (name, k)
