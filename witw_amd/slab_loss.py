"""The column-slab protocol of the global-batch losses, once: rank r evaluates all B overhead embeddings against its own b surface
embeddings (a [B, b] slab of the distance matrix; the full [B, B] matrix is never built on one GPU).

  forward   all-gather of the overhead embeddings          open_slab           phase 'overhead_all_gather'
            all-gather of the diagonal (B floats)          gather_diagonal     phase 'diagonal_all_gather'
            batch-hard: per-rank row minima, merged        mine_global         phase 'row_minima_all_gather'
            all-reduce of the loss partial                 sum_partial         phase 'loss_partial_all_reduce'
  backward  reduce-scatter of the overhead gradients       scatter_overhead_grad   phase 'overhead_grad_reduce_scatter'
            (every rank holds the part that flows through ITS surfaces; the surface gradients are complete locally)

The four autograd functions on it -- cvig_fov._ShardedMatchLossFn / _BatchHardMatchLossFn, cvig_baseline._ShardedExhaustiveLossFn /
_ShardedBatchHardLossFn -- keep the calls that differ (which distance, which loss kernels, which backward), what they save and
their normaliser, and each says which of the steps it skips on one rank (`on`). The phase names are what bench.py's
collectives.per_phase_ms is keyed on.
"""
import torch

from . import _lib, parallel


def open_slab(overhead_local, surface_local, who=None, always=False, sharded=True):
    """The slab prologue -> (ov_all [B, ...], su [b, ...], b, col0, B, world): both sides contiguous, the overhead side gathered
    (at world 1 only where the caller `always` runs its collectives). who: the caller's public name -- then both sides must be
    [b, n] of one shape and, decided on gathered data so that every rank raises and none is left waiting, every rank must bring
    the same b. sharded=False: one slab b = B, whatever process group there is."""
    world, rank = (parallel.world(), parallel.rank()) if sharded else (1, 0)
    su = surface_local.contiguous()
    b = su.shape[0]
    if who is not None:
        if overhead_local.shape != su.shape or su.dim() != 2:
            raise _lib.WitwError('%s: need [b, n] embeddings of one shape, got %s and %s'
                                 % (who, tuple(surface_local.shape), tuple(overhead_local.shape)))
        if world > 1:
            with parallel.phase('batch_share_all_gather'):
                shares = parallel._all_gather_cat(torch.tensor([b], dtype=torch.int64, device=su.device)).tolist()
            if len(set(shares)) != 1:
                raise _lib.WitwError('%s: unequal batch shares across the ranks %s -- every rank must bring the same number of pairs '
                                     '(train with drop_last)' % (who, shares))
    if always or world > 1:
        with parallel.phase('overhead_all_gather'):
            ov_all = parallel._all_gather_cat(overhead_local.contiguous())
    else:
        ov_all = overhead_local.contiguous()
    return ov_all, su, b, rank * b, ov_all.shape[0], world


def gather_diagonal(dist, col0, b, on):
    """the B true-pair distances: this rank's b of them lie on the diagonal of rows [col0, col0 + b) of its slab"""
    own = dist[col0:col0 + b].diagonal().contiguous()
    if not on:
        return own
    with parallel.phase('diagonal_all_gather'):
        return parallel._all_gather_cat(own)


def mine_global(k, dist, col0, on):
    """-> (rv [B], ri [B], cv [b], ci [b]): every row's and every own column's hardest negative over the GLOBAL batch -- the slab's
    row minima of all ranks ([w, B] values + global column indices) merged in rank order, the lowest index wins a tie"""
    with parallel.phase('row_minima_all_gather'):
        rv, ri, cv, ci = k.batch_hard_slab_mine(dist, col0)
        if on:
            rv, ri = k.batch_hard_merge_rows(parallel._all_gather_cat(rv[None]), parallel._all_gather_cat(ri[None]))
    return rv, ri, cv, ci


def sum_partial(partial, on):
    """partial() -- this rank's share of the loss sum, float32 [1] -- summed over the ranks"""
    with parallel.phase('loss_partial_all_reduce'):
        part = partial()
        if on:
            parallel.all_reduce_sum_(part)
    return part


def scatter_overhead_grad(gov_all, b, on):
    """[B, ...] gradients of the gathered overhead embeddings (None: not needed) -> the sum over the ranks of this rank's b rows"""
    if gov_all is None or not on:
        return gov_all
    with parallel.phase('overhead_grad_reduce_scatter'):
        return parallel.reduce_scatter_rows(gov_all, b)
