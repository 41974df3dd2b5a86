"""cvig_baseline's exhaustive loss on column slabs of the global batch (csrc/baseline_loss_slab.hip through
witw_amd/baseline_parallel.py) and cvig_baseline.sharded_exhaustive_loss on top of them, against the float64 expectations the
dense test already has: loss_inputs / loss_refs / LOSS_CFGS of tests/test_baseline_head_gpu.py (tests/baseline_head_ref.py), and
tests/baseline_slab_ref.py for the sums only the slab form has.

Bounds, none taken from a kernel's output: loss 1e-4 relative and every embedding gradient within 2e-5 of its largest entry (the
dense test's own); rowsig / colsig 1e-5 of each element (hard margin: counts, exact as long as no term sits on the kink, which
loss_inputs keeps 1e-4 away; soft margin: a term's relative error is alpha x the error of d_positive - d_negative, about 5e-7 for
in-cluster distances of about 1); the whole training step by the project's training-step criterion, every parameter gradient
within 1e-4 of its norm. Every test prints its figures before it asserts.

Measured on an MI355X (worst over the cases of each test, as fractions of the scale the bound is relative to):

  quantity                                              bound    kernel
  slab loss, all partitions                             1e-4     1.2e-6
  rowsig / colsig per element                           1e-5     4.1e-6 / 5.5e-6 (soft margin; hard margin exact)
  dx summed over slabs / dy                             2e-5     6.4e-7 / 6.4e-7
  world of one: loss / d surface / d overhead           1e-4 / 2e-5    3.3e-7 / 6.4e-7 / 6.4e-7
  rank-threads (2, 8): loss / d surface / d overhead    1e-4 / 2e-5    3.5e-7 / 4.3e-7 / 5.1e-7
  training step, two rank-threads: loss                 1e-4     equal to 7 digits
  training step: worst parameter gradient               1e-4     9.9e-5 of its norm -- close to the bound. With 2 images per rank the last
                                                                 blocks' BatchNorm sees 2 values per channel (a 1 x 1 map), whose backward cancels
                                                                 almost exactly: what is left of those gradients is rounding of the loss gradient
                                                                 magnified, and the slab and the dense backward sum in different orders.

Shapes. (B, b, col0): (2, 2, 0) the smallest batch as one slab; (3, 1, 2) a one-column last slab; (37, 37, 0) / (37, 5, 32) an odd
batch as one slab and in slabs of 5 (32 = 6 x 5 + 2: a ragged middle slab); (300, 44, 256) B above the 256-thread stride, off it,
more than one 64-row tile of G per workgroup; (257, 1, 256) the diagonal entry in the last row, one column per slab. n = 8 leaves
248 lanes of a 256-column workgroup idle, n = 1536 is the embedding width (6 column tiles)."""
import copy

import pytest
import torch

from tests import baseline_head_ref as R
from tests import baseline_slab_ref as S
from tests.mem_arena import Arena, ArenaTorch
from tests.test_baseline_head_gpu import GRAD_LOSS, LOSS_CFGS, loss_inputs, loss_refs

from .threaded_world import run_ranks

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SLABS = [(2, 2, 0), (3, 1, 2), (37, 37, 0), (37, 5, 32), (300, 44, 256), (257, 1, 256)]


def _cfg(cfg):
    """LOSS_CFGS entry -> (soft_margin, alpha, margin) with the defaults of the loss"""
    kw = dict(soft_margin=False, alpha=10.0, margin=1.0)
    kw.update(LOSS_CFGS[cfg])
    return kw


def _partition(B, b, col0):
    """slabs (col0, width) that tile the B columns and hold (col0, b): width b from the left, a ragged one in front of col0"""
    out, c = [], 0
    while c < col0:
        out.append((c, min(b, col0 - c)))
        c += out[-1][1]
    out.append((col0, b))
    assert col0 + b == B
    return out


def _relmax(got, ref):
    return float((R.f64(got) - ref).abs().max() / ref.abs().max())


def _run_slabs(a, b, parts, kw):
    """every slab of the partition on the GPU, the exchanges of the ranks done by hand -> (loss, rowsig [B], {col0: colsig},
    G [B,B], dx [B,n] summed over the slabs in fp32, dy [B,n])"""
    from witw_amd import baseline_parallel as bp
    from witw_amd import ops
    B = a.shape[0]
    gl = torch.tensor([GRAD_LOSS], device=a.device)
    T = {c0: ops.pairwise_sqdist(a, b[c0:c0 + w].contiguous()) for c0, w in parts}
    diag = torch.cat([T[c0][c0:c0 + w].diagonal() for c0, w in parts]).contiguous()                     # the all-gather
    partial = sum(bp.exhaustive_loss_slab_fwd(T[c0], diag, c0, **kw) for c0, _w in parts)               # the all-reduce
    sig = {c0: bp.exhaustive_loss_slab_sig(T[c0], diag, c0, **kw) for c0, _w in parts}
    rowsig = torch.stack([sig[c0][0] for c0, _w in parts]).sum(0)                                       # the all-reduce
    G, dx, dy = [], torch.zeros_like(a), []
    for c0, w in parts:
        g = bp.exhaustive_loss_slab_bwd(T[c0], diag, rowsig, sig[c0][1], gl, c0, **kw)
        gx, gy = bp.sqdist_rect_bwd(a, b[c0:c0 + w].contiguous(), g)
        G.append(g)
        dx += gx                                                                                        # the reduce-scatter's sum
        dy.append(gy)
    return partial / (2.0 * B * (B - 1)), rowsig, {c0: sig[c0][1] for c0, _w in parts}, torch.cat(G, 1), dx, torch.cat(dy)


@pytest.mark.parametrize('cfg', sorted(LOSS_CFGS))
@pytest.mark.parametrize('n', [8, 1536])
@pytest.mark.parametrize('B,b,col0', SLABS)
def test_slab_kernels_against_float64(B, b, col0, n, cfg):
    a, bb, _seed, _gaps = loss_inputs(B, n)
    loss, d1, d2 = loss_refs(B, n, cfg)
    kw = _cfg(cfg)
    parts = _partition(B, b, col0)
    got_loss, rowsig, colsig, _G, dx, dy = _run_slabs(a.to(DEV), bb.to(DEV), parts, kw)
    # float64 definitions of the two sums, on the float64 distances
    T64 = R.pairwise_sqdist(a.double(), bb.double())
    diag64 = torch.diagonal(T64).clone()
    sig64 = {c0: S.slab_sig(T64[:, c0:c0 + w], diag64, c0, **kw) for c0, w in parts}
    row64 = torch.stack([sig64[c0][0] for c0, _w in parts]).sum(0)

    def rel(got, ref):          # per element; an exact zero (no active term) must be an exact zero
        err = (R.f64(got) - ref).abs()
        return float((err / ref.abs().clamp(min=1e-300)).max())

    e_row = rel(rowsig, row64)
    e_col = max(rel(colsig[c0], sig64[c0][1]) for c0, _w in parts)
    e_loss = abs(got_loss.item() - loss.item()) / abs(loss.item())
    e1, e2 = _relmax(dx, d1), _relmax(dy, d2)
    print('slabs B=%d b=%d col0=%d n=%d %s (%d slabs): loss rel err %.1e; rowsig %.1e colsig %.1e per element; dx %.1e dy %.1e of their max'
          % (B, b, col0, n, cfg, len(parts), e_loss, e_row, e_col, e1, e2))
    assert e_loss <= 1e-4
    assert e_row <= 1e-5 and e_col <= 1e-5
    assert e1 <= 2e-5 and e2 <= 2e-5


@pytest.mark.parametrize('cfg', sorted(LOSS_CFGS))
@pytest.mark.parametrize('B', [2, 37, 257])
def test_world_of_one_runs_the_slab_path(B, cfg):
    from witw_amd import cvig_baseline, ops, parallel
    assert parallel.world() == 1
    n = 1536
    a, bb, _seed, _gaps = loss_inputs(B, n)
    loss, d1, d2 = loss_refs(B, n, cfg)
    su, ov = a.to(DEV).requires_grad_(True), bb.to(DEV).requires_grad_(True)
    got = cvig_baseline.sharded_exhaustive_loss(su, ov, **LOSS_CFGS[cfg])
    assert ops.last_kernel_variant() == 'exhaustive_slab_partials_kernel'
    with torch.autograd.set_multithreading_enabled(False):      # the variant is recorded per calling thread: keep the backward on this one
        got.backward(torch.tensor(GRAD_LOSS, device=DEV))
    assert ops.last_kernel_variant().startswith('sqdist_rect_bwd_kernel<dx:')
    e_loss = abs(got.item() - loss.item()) / abs(loss.item())
    e1, e2 = _relmax(su.grad, d1), _relmax(ov.grad, d2)
    print('world of one B=%d %s: loss rel err %.1e; d surface %.1e d overhead %.1e of their max' % (B, cfg, e_loss, e1, e2))
    assert got.dim() == 0 and e_loss <= 1e-4
    assert e1 <= 2e-5 and e2 <= 2e-5


def test_same_call_twice_gives_the_same_bits():
    B, b, col0, n = 300, 44, 256, 1536
    a, bb, _seed, _gaps = loss_inputs(B, n)
    ad, bd = a.to(DEV), bb.to(DEV)
    for cfg in ('hard_m1', 'soft_a10'):
        runs = [_run_slabs(ad, bd, _partition(B, b, col0), _cfg(cfg)) for _ in range(2)]
        torch.cuda.synchronize()
        for x, y in zip(runs[0], runs[1]):
            if isinstance(x, dict):
                assert all(torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) for k in x)
            else:
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- rank-threads
@pytest.mark.parametrize('cfg', ['hard_m1', 'soft_a10'])
@pytest.mark.parametrize('B', [16, 40])
@pytest.mark.parametrize('world', [2, 8])
def test_rank_threads_hold_the_global_loss_and_their_gradient_rows(world, B, cfg):
    from witw_amd import cvig_baseline
    n, b = 1536, B // world
    a, bb, _seed, _gaps = loss_inputs(B, n)
    loss, d1, d2 = loss_refs(B, n, cfg)
    ad, bd = a.to(DEV), bb.to(DEV)

    def fn(rank):
        torch.cuda.set_device(DEV)
        sl = slice(rank * b, (rank + 1) * b)
        su, ov = ad[sl].clone().requires_grad_(True), bd[sl].clone().requires_grad_(True)
        got = cvig_baseline.sharded_exhaustive_loss(su, ov, **LOSS_CFGS[cfg])
        got.backward(torch.tensor(GRAD_LOSS, device=DEV))
        torch.cuda.synchronize()
        return got.item(), su.grad.cpu(), ov.grad.cpu()
    res = run_ranks(world, fn, timeout=120.0)
    worst = [0.0, 0.0, 0.0]
    for rank, (got, gsu, gov) in enumerate(res):
        sl = slice(rank * b, (rank + 1) * b)
        worst[0] = max(worst[0], abs(got - loss.item()) / abs(loss.item()))
        worst[1] = max(worst[1], float((gsu.double() - d1[sl]).abs().max() / d1.abs().max()))
        worst[2] = max(worst[2], float((gov.double() - d2[sl]).abs().max() / d2.abs().max()))
    print('world %d B=%d %s: loss rel err %.1e; d surface %.1e, reduce-scattered d overhead %.1e of the gradients\' max' % (world, B, cfg, *worst))
    assert worst[0] <= 1e-4 and worst[1] <= 2e-5 and worst[2] <= 2e-5


def test_unequal_shares_raise_on_every_rank():
    from witw_amd import _lib, cvig_baseline
    a, bb, _seed, _gaps = loss_inputs(37, 1536)
    ad, bd = a.to(DEV), bb.to(DEV)
    spans = [(0, 2), (2, 4), (4, 5)]

    def fn(rank):
        torch.cuda.set_device(DEV)
        lo, hi = spans[rank]
        try:
            cvig_baseline.sharded_exhaustive_loss(ad[lo:hi].contiguous(), bd[lo:hi].contiguous())
        except _lib.WitwError as ex:
            return str(ex)
        return None
    res = run_ranks(3, fn, timeout=120.0)          # returns: no thread was left waiting in a collective
    assert all(m is not None and 'unequal batch shares' in m and '[2, 2, 1]' in m for m in res), res


# ---------------------------------------------------------------------------------------------------------------- whole step
def test_training_step_on_two_rank_threads_is_the_two_replica_step():
    """encoders -> sharded_exhaustive_loss -> backward -> OverlappedGradReducer on two rank-threads, against the single-process
    form of the same semantics: one deep copy of the encoders per sub-batch (each keeps its own batch statistics, as an
    nn.DataParallel replica does), the dense loss on the concatenated embeddings, the copies' parameter gradients summed. Both
    forms run the same forward kernels on the same inputs, so the LeakyReLU gates agree bit for bit."""
    from witw_amd import cvig_baseline, parallel, synth
    torch.manual_seed(3)
    se0, oe0 = cvig_baseline.SurfaceEncoder().to(DEV).train(), cvig_baseline.OverheadEncoder().to(DEV).train()
    xs = torch.from_numpy(synth.images_u8(21, 1, (4, 3, 382, 382))).to(DEV)
    xo = torch.from_numpy(synth.images_u8(21, 2, (4, 3, 382, 382))).to(DEV)
    # single process: copy k sees sub-batch k
    copies = [(copy.deepcopy(se0), copy.deepcopy(oe0)) for _ in range(2)]
    su = torch.cat([copies[k][0](xs[2 * k:2 * k + 2]) for k in range(2)])
    ov = torch.cat([copies[k][1](xo[2 * k:2 * k + 2]) for k in range(2)])
    ref_loss = cvig_baseline.exhaustive_minibatch_triplet_loss(su, ov)
    ref_loss.backward()
    torch.cuda.synchronize()
    ref_grads = [(pa.grad + pb.grad).double().cpu() for e in range(2) for pa, pb in zip(copies[0][e].parameters(), copies[1][e].parameters())]
    names = [side + '.' + nm for side, enc in (('surface', se0), ('overhead', oe0)) for nm, _p in enc.named_parameters()]

    def fn(rank):
        torch.cuda.set_device(DEV)
        se, oe = copy.deepcopy(se0), copy.deepcopy(oe0)
        reducer = parallel.OverlappedGradReducer([se, oe])
        sl = slice(2 * rank, 2 * rank + 2)
        loss = cvig_baseline.sharded_exhaustive_loss(se(xs[sl]), oe(xo[sl]))
        loss.backward()
        reducer.wait()
        grads = [p.grad.double().cpu() for p in list(se.parameters()) + list(oe.parameters())]
        own = [t.clone() for t in (se.bn1.running_mean, oe.bn7.running_var)]
        se._layer(1)                                    # the eval fold of this rank's OWN statistics: the broadcast must retire it
        parallel.broadcast_buffers(cvig_baseline._bn_modules(se, oe))
        torch.cuda.synchronize()
        bufs = {side + '.' + nm: t.cpu() for side, enc in (('surface', se), ('overhead', oe)) for nm, t in enc.named_buffers()}
        folded = se._layer(1)[1].cpu()                  # the eval fold is rebuilt from the broadcast statistics
        reducer.close()
        return loss.item(), grads, [t.cpu() for t in own], bufs, folded
    res = run_ranks(2, fn, timeout=300.0)
    first = {side + '.' + nm: t.cpu() for side, e in (('surface', 0), ('overhead', 1)) for nm, t in copies[0][e].named_buffers()}
    second = {side + '.' + nm: t.cpu() for side, e in (('surface', 0), ('overhead', 1)) for nm, t in copies[1][e].named_buffers()}
    assert not torch.equal(first['surface.bn1.running_mean'], second['surface.bn1.running_mean'])      # the sub-batches do differ
    fold_ref = (copies[0][0].bn1.weight / torch.sqrt(copies[0][0].bn1.running_var + copies[0][0].bn1.eps)).cpu()
    worst = (0.0, '')
    for rank, (loss, grads, own, bufs, folded) in enumerate(res):
        print('rank %d: loss %.6f (two-replica form %.6f)' % (rank, loss, ref_loss.item()))
        assert abs(loss - ref_loss.item()) <= 1e-4 * abs(ref_loss.item())
        for name, g, gr in zip(names, grads, ref_grads):
            dev = float((g - gr).norm() / gr.norm())
            worst = max(worst, (dev, name))
            assert float(gr.norm()) > 0 and dev <= 1e-4, (rank, name, dev)
        # before the broadcast rank k held the statistics of replica k; after it every rank holds the first replica's
        mine = (first, second)[rank]
        assert torch.equal(own[0], mine['surface.bn1.running_mean']) and torch.equal(own[1], mine['overhead.bn7.running_var'])
        for name, t in bufs.items():
            assert torch.equal(t, first[name]), (rank, name)
        assert torch.equal(folded, fold_ref)
    print('worst parameter-gradient deviation %.2e of its norm (%s)' % worst)


# ---------------------------------------------------------------------------------------------------------------- memory contract
def _contract_cases(B, b, col0, n, kw):
    """name -> (inputs {name: tensor}, call(bp, placed inputs) -> outputs) for the four wrappers at one shape"""
    a, bb, _seed, _gaps = loss_inputs(B, n)
    ad, bd = a.to(DEV), bb.to(DEV)
    from witw_amd import baseline_parallel as bp
    from witw_amd import ops
    y = bd[col0:col0 + b].contiguous()
    T = ops.pairwise_sqdist(ad, y)
    diag = torch.diagonal(ops.pairwise_sqdist(ad, bd)).contiguous()
    rowsig, colsig = bp.exhaustive_loss_slab_sig(T, diag, col0, **kw)
    rowsig = rowsig + 1.0           # stands for the other slabs' part
    gl = torch.tensor([GRAD_LOSS], device=DEV)
    G = bp.exhaustive_loss_slab_bwd(T, diag, rowsig, colsig, gl, col0, **kw)
    return {
        'fwd': (dict(T=T, diag=diag), lambda m, p: m.exhaustive_loss_slab_fwd(p['T'], p['diag'], col0, **kw)),
        'sig': (dict(T=T, diag=diag), lambda m, p: m.exhaustive_loss_slab_sig(p['T'], p['diag'], col0, **kw)),
        'bwd': (dict(T=T, diag=diag, rowsig=rowsig, colsig=colsig, gl=gl),
                lambda m, p: m.exhaustive_loss_slab_bwd(p['T'], p['diag'], p['rowsig'], p['colsig'], p['gl'], col0, **kw)),
        'rect': (dict(x=ad, y=y, G=G), lambda m, p: m.sqdist_rect_bwd(p['x'], p['y'], p['G'])),
        'rect_dx': (dict(x=ad, y=y, G=G), lambda m, p: m.sqdist_rect_bwd(p['x'], p['y'], p['G'], need_dy=False)[0]),
        'rect_dy': (dict(x=ad, y=y, G=G), lambda m, p: m.sqdist_rect_bwd(p['x'], p['y'], p['G'], need_dx=False)[1]),
    }


@pytest.mark.parametrize('skew', [0, 16])
@pytest.mark.parametrize('cfg', ['hard_m1', 'soft_a10'])
@pytest.mark.parametrize('B,b,col0,n', [(2, 1, 1, 8), (37, 5, 32, 70), (300, 44, 256, 1536)], ids=['2x1x8', '37x5x70', '300x44x1536'])
def test_memory_contract_of_the_wrappers(B, b, col0, n, cfg, skew, monkeypatch):
    """Every wrapper of baseline_parallel between guard bands (tests/mem_arena.py): inputs inside NaN bands, every device
    allocation of the wrapper (outputs and workspace) inside guard bands with a canary payload. No band is touched, every
    output element is stored, the inputs are unchanged and the values are those of ordinary allocations, bit for bit."""
    from witw_amd import baseline_parallel as bp
    for name, (inputs, call) in _contract_cases(B, b, col0, n, _cfg(cfg)).items():
        plain = call(bp, inputs)
        plain = [t.clone() for t in (plain if isinstance(plain, tuple) else (plain,))]
        arena = Arena(DEV, skew_bytes=skew)
        with monkeypatch.context() as m:
            m.setattr(bp, 'torch', ArenaTorch(arena))
            placed = {k: arena.place(t, k) for k, t in inputs.items()}
            got = call(bp, placed)
        arena.check(got)
        got = got if isinstance(got, tuple) else (got,)
        assert len(got) == len(plain)
        for x, y in zip(got, plain):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
        for k, t in inputs.items():
            assert torch.equal(placed[k].view(torch.int32), t.view(torch.int32)), (name, k)
