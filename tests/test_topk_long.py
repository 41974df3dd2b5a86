"""Candidate lists longer than 32 places, CPU side: the slice loop of ops.topk_smallest (ops._topk_slices) and the merge of the
shards' lists (retrieval._merge_topk) on a torch rendering of the kernels' rule -- a run returns the n smallest rows in the order
(distance, gallery index), NaN counted as +inf, and a resumed run only the rows strictly behind its bound; a bound with index -1
(the missing candidate) has nothing behind it. The lists must equal the stable sort of the whole column."""
import pytest
import torch

from oracle import cvig_fov_oracle as O
from witw_amd import _lib, cvig_fov, ops, synth

from .threaded_world import run_ranks


def _run(dist, n, row_offset, bound=None):
    """one run of the kernels over dist [Bo,Bs]: n places per query, behind bound = (values [Bs], indices [Bs]) if given"""
    d = torch.where(torch.isnan(dist), torch.full_like(dist, float('inf')), dist)
    bo, bs = d.shape
    rows = torch.arange(bo) + row_offset
    vals = torch.full((bs, n), float('inf'))
    idx = torch.full((bs, n), -1, dtype=torch.int64)
    for q in range(bs):
        keep = torch.ones(bo, dtype=torch.bool)
        if bound is not None:
            bv, bi = float(bound[0][q]), int(bound[1][q])
            keep = (d[:, q] > bv) | ((d[:, q] == bv) & (rows > bi)) if bi != -1 else ~keep
        cand = torch.nonzero(keep).squeeze(1)                       # ascending rows: a stable sort breaks ties by the row
        order = cand[torch.sort(d[cand, q], stable=True).indices][:n]
        vals[q, :order.numel()] = d[order, q]
        idx[q, :order.numel()] = rows[order]
    return vals, idx


def _sliced(dist, k, row_offset=0):
    """ops.topk_smallest's long form with the two C entries replaced by _run"""
    bs = dist.shape[1]
    calls = []

    def first(n):
        calls.append(n)
        return _run(dist, n, row_offset)

    def resume(n, bv, bi):
        calls.append(n)
        return _run(dist, n, row_offset, (bv.clone(), bi.clone()))
    out = ops._topk_slices(k, first, resume, torch.empty((bs, k)), torch.empty((bs, k), dtype=torch.int64), torch.empty((bs,)),
                           torch.empty((bs,), dtype=torch.int64))
    return out, calls


def _expected(dist, k, row_offset=0):
    d = torch.where(torch.isnan(dist), torch.full_like(dist, float('inf')), dist)
    v, i = torch.sort(d.t().contiguous(), dim=1, stable=True)
    pad = max(0, k - d.shape[0])
    v = torch.cat((v[:, :k], torch.full((d.shape[1], pad), float('inf'))), dim=1)
    i = torch.cat((i[:, :k] + row_offset, torch.full((d.shape[1], pad), -1, dtype=torch.int64)), dim=1)
    return v, i


def _inputs(bo, bs, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = torch.rand((bo, bs), generator=g)
    five = torch.randint(0, 5, (bo, bs), generator=g).float()       # runs of equal values across every boundary of 32
    equal = rnd.clone()
    equal[:, 0] = 0.25
    inf = five.clone()
    inf[torch.rand((bo, bs), generator=g) < 0.6] = float('inf')
    nan = inf.clone()
    nan[torch.rand((bo, bs), generator=g) < 0.3] = float('nan')
    return {'random': rnd, 'five_values': five, 'equal_column': equal, 'inf': inf, 'nan': nan}


@pytest.mark.parametrize('bo,bs,k,off', [(100, 5, 33, 0), (257, 3, 100, 1000003), (70, 4, 64, 0), (31, 2, 65, 7), (1, 3, 100, 0),
                                         (130, 2, 128, 0)])
def test_slice_loop_equals_the_stable_sort(bo, bs, k, off):
    for name, dist in _inputs(bo, bs, 10 * bo + k).items():
        (v, i), calls = _sliced(dist, k, off)
        ev, ei = _expected(dist, k, off)
        assert torch.equal(v, ev) and torch.equal(i, ei), name
        assert calls == [32] * (k // 32) + ([k % 32] if k % 32 else []), calls
        for row in i.tolist():
            present = [x for x in row if x != -1]
            assert len(present) == len(set(present)) == min(k, bo), name


def test_range_of_k_is_checked_before_anything_runs():
    class Untouchable(object):
        def __getattr__(self, name):
            raise AssertionError('retrieve touched %s before refusing k' % name)
    gal, qry = torch.zeros((4, 16, 4, 64)), torch.zeros((2, 16, 4, 64))
    for k in (0, ops.TOPK_MAX + 1):
        with pytest.raises(_lib.WitwError, match=r'k=%d outside \[1,1024\]' % k):
            cvig_fov.retrieve(gal, qry, k=k, _kernels=Untouchable())
        with pytest.raises(_lib.WitwError, match=r'k=%d outside \[1,1024\]' % k):
            cvig_fov.retrieve_topk(gal, qry, k=k, method='dft', _kernels=Untouchable())
    assert ops.TOPK_LIST == 32 and ops.TOPK_MAX == 1024


def test_new_entry_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.witw_topk_smallest_after(1, 1, 1, 100, 10, 33, 0, 1, 1, None, None) == -1 and b'k=33' in lib.witw_last_error()
    assert lib.witw_topk_smallest_after(1, 1, 1, 100, 10, 0, 0, 1, 1, None, None) == -1 and b'k=0' in lib.witw_last_error()
    assert lib.witw_topk_smallest_after(1, 1, 1, 100, 10, 32, 0, None, 1, None, None) == -1 and b'null bound' in lib.witw_last_error()
    assert lib.witw_topk_smallest_after(1, 1, 1, 100, 10, 32, 0, 1, None, None, None) == -1 and b'null bound' in lib.witw_last_error()
    assert lib.witw_topk_smallest_after(None, 1, 1, 100, 10, 32, 0, 1, 1, None, None) == -1 and b'null' in lib.witw_last_error()
    assert lib.witw_topk_smallest_after(1, 1, 1, 0, 10, 32, 0, 1, 1, None, None) == -1 and b'bad shape' in lib.witw_last_error()


class SlicedKernels(object):
    """the op set of retrieve's direct pass: float64 distances rounded once (a pair's distance must not depend on its shard) and
    the long form of topk_smallest on the rule above"""
    rank_count_thresh = None

    @staticmethod
    def match_fwd(ov, su, want_score=False, want_workspace=False):
        return O.match_fused(ov, su)

    @staticmethod
    def topk_smallest(dist, k, row_offset=0):
        return _sliced(dist, k, row_offset)[0]


def test_three_ragged_shards_merged_at_k_100_equal_the_unsharded_list():
    split = [131, 0, 89]
    G, Q, we, k = sum(split), 9, 12, 100
    gal = torch.from_numpy(synth.embeddings(61, 1, (G, 16, 4, 64)))
    gal[150], gal[200] = gal[3], gal[3]                              # equal distances in two shards: the merge breaks them by index
    qry = torch.from_numpy(synth.embeddings(61, 2, (Q, 16, 4, we))).contiguous()
    v1, i1 = cvig_fov.retrieve_topk(gal, qry, k=k, query_chunk=4, _kernels=SlicedKernels)
    ev, ei = _expected(O.match_fused(gal, qry)[1], k)
    assert torch.equal(v1, ev) and torch.equal(i1, ei)
    assert bool(((i1 == 3).any(1) & (i1 == 150).any(1) & (i1 == 200).any(1)).any())

    def fn(rank):
        g0 = sum(split[:rank])
        return cvig_fov.retrieve_topk(gal[g0:g0 + split[rank]], qry, k=k, shard_begin=g0, query_chunk=4, _kernels=SlicedKernels)
    for v, i in run_ranks(3, fn):
        assert torch.equal(v, v1) and torch.equal(i, i1)
    # a list longer than the whole gallery: the places beyond its rows are missing candidates on every rank
    k = 256
    v2, i2 = cvig_fov.retrieve_topk(gal, qry, k=k, _kernels=SlicedKernels)
    assert torch.equal(i2[:, :G], _expected(O.match_fused(gal, qry)[1], G)[1]) and bool((i2[:, G:] == -1).all())
    for v, i in run_ranks(3, lambda rank: cvig_fov.retrieve_topk(gal[sum(split[:rank]):sum(split[:rank + 1])], qry, k=k,
                                                                 shard_begin=sum(split[:rank]), _kernels=SlicedKernels)):
        assert torch.equal(v, v2) and torch.equal(i, i2)
