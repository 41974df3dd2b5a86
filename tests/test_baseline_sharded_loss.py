"""world_size-2 CPU (gloo) tests of cvig_baseline's multi-rank host logic, spawned as tests/test_parallel_gloo.py does: the
collective choreography of sharded_exhaustive_loss (float64 stand-ins of tests/baseline_slab_ref.py for the five kernel calls)
against the single-process oracle loss on the global batch, the validation phase's sharding of every global batch, and
parallel.broadcast_buffers. One pair of processes serves all tests."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import cvig_baseline_oracle as O
from witw_amd import synth

B, N_IN, N_EMB = 6, 24, 16
MODES = {'hinge': dict(soft_margin=False, margin=1.0), 'soft': dict(soft_margin=True, alpha=10.0)}
VAL_ITEMS, VAL_BATCH = 11, 4


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _toy_encoders():
    torch.manual_seed(7)
    return torch.nn.Linear(N_IN, N_EMB).double(), torch.nn.Linear(N_IN, N_EMB).double()


def _inputs():
    return (torch.from_numpy(synth.embeddings(11, 1, (B, N_IN))).double(), torch.from_numpy(synth.embeddings(11, 2, (B, N_IN))).double())


def _worker(rank, world, port, out_q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from tests.baseline_slab_ref import CpuKernels
        from witw_amd import cvig_baseline, parallel
        torch.set_num_threads(2)
        out = {}
        xs, xo = _inputs()
        b0, b1 = parallel.shard_range(B)
        for mode, kw in MODES.items():
            su_enc, ov_enc = _toy_encoders()
            loss = cvig_baseline.sharded_exhaustive_loss(su_enc(xs[b0:b1]), ov_enc(xo[b0:b1]), _kernels=CpuKernels, **kw)
            loss.backward()
            params = list(su_enc.parameters()) + list(ov_enc.parameters())
            assert parallel.all_reduce_grads(params) == sum(p.numel() for p in params)
            out[mode] = (loss.item(), [p.grad.numpy().copy() for p in params])
        # the validation phase: this rank's share of every global batch, gathered
        items = torch.arange(VAL_ITEMS * 3, dtype=torch.float64).reshape(VAL_ITEMS, 3)
        shares = list(cvig_baseline.GlobalBatchShares(VAL_ITEMS, VAL_BATCH, rank, world))
        out['val_shares'] = shares
        out['val_batches'] = [parallel.all_gather_ragged(items[idx]).numpy().copy() for idx in shares]
        # running statistics: rank 0's survive
        bn = torch.nn.BatchNorm1d(5)
        with torch.no_grad():
            bn.running_mean.fill_(rank + 1.0)
            bn.running_var.fill_(10.0 * (rank + 1))
            bn.num_batches_tracked.fill_(3 + rank)
            bn.weight.fill_(rank + 0.5)
        parallel.broadcast_buffers([bn])
        out['bn'] = (bn.running_mean.numpy().copy(), bn.running_var.numpy().copy(), int(bn.num_batches_tracked), float(bn.weight[0]),
                     getattr(bn.running_mean, '_witw_version', 0))
        out_q.put((rank, out))       # numpy: no shared-memory handles that die with the sender
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope='module')
def world2():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return [r[1] for r in res]


@pytest.mark.parametrize('mode', sorted(MODES))
def test_sharded_exhaustive_loss_world2_equals_the_oracle_on_the_global_batch(world2, mode):
    """loss (normaliser 2B(B-1) with the GLOBAL B) and the toy encoders' weight gradients after all_reduce_grads"""
    xs, xo = _inputs()
    su_enc, ov_enc = _toy_encoders()
    ref = O.exhaustive_minibatch_triplet_loss(su_enc(xs), ov_enc(xo), **MODES[mode])
    ref.backward()
    grads_ref = [p.grad for p in list(su_enc.parameters()) + list(ov_enc.parameters())]
    assert ref.item() > 0 and all(float(g.abs().max()) > 0 for g in grads_ref)
    for r in world2:
        loss, grads = r[mode]
        assert abs(loss - ref.item()) <= 1e-12 * abs(ref.item())
        for g, gr in zip(grads, grads_ref):
            np.testing.assert_allclose(g, gr.numpy(), rtol=1e-9, atol=1e-12 * float(gr.abs().max()))


def test_validation_shares_gather_to_the_single_process_batches(world2):
    items = np.arange(VAL_ITEMS * 3, dtype=np.float64).reshape(VAL_ITEMS, 3)
    single = [items[i:i + VAL_BATCH] for i in range(0, VAL_ITEMS, VAL_BATCH)]       # DataLoader(shuffle=False, drop_last=False)
    assert [len(s) for s in single] == [4, 4, 3]
    for r in world2:
        assert len(r['val_batches']) == len(single)
        for got, want in zip(r['val_batches'], single):
            np.testing.assert_array_equal(got, want)
    both = [a + b for a, b in zip(world2[0]['val_shares'], world2[1]['val_shares'])]
    assert both == [list(range(i, min(i + VAL_BATCH, VAL_ITEMS))) for i in range(0, VAL_ITEMS, VAL_BATCH)]


def test_broadcast_buffers_leaves_rank0_values_on_both_ranks(world2):
    for rank, r in enumerate(world2):
        mean, var, tracked, weight, version = r['bn']
        assert (mean == 1.0).all() and (var == 10.0).all() and tracked == 3
        assert weight == rank + 0.5          # parameters are not its business
        assert version == 1                  # the eval fold keyed on it is rebuilt
