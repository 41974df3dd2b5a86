"""Candidate lists longer than 32 places on the device: ops.topk_smallest above k = 32 is ceil(k / 32) runs of the top-k kernels,
each resuming the exact scan behind the last place of the run before (witw_topk_smallest_after). Expected lists: the first k
entries of torch.sort(column, stable=True) on the CPU -- ties to the lower index, the kernels' order -- compared with torch.equal.

Shapes: csrc/match.hip splits the gallery rows over workgroups from Bo = 513 on (topk_splits: at least 512 rows per split) and
takes the threshold shortcut (the k best of the first 1,024 rows bound admission) from Bo = 16 * 1,024 rows and 8 splits on, which
Bs <= 16,384 gives; 512 / 513 and 16,384 are in the table with few queries. Every Bo, Bs, k and row_offset of the table below
occurs in some case. The memory contract of the new entry and of the long form follows at the end (tests/mem_arena.py)."""

import numpy as np
import pytest
import torch

from tests.mem_arena import Arena, ArenaTorch

from .threaded_world import run_ranks

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
BIG = 1000003
#        Bo     Bs   k    row_offset
CASES = [(1, 1, 33, 0), (31, 63, 64, BIG), (33, 65, 65, 0), (100, 130, 100, BIG), (257, 1, 300, 0), (257, 63, 33, 0),
         (100, 65, 64, 0), (33, 130, 100, 0), (512, 65, 65, BIG), (513, 63, 100, 0), (513, 130, 64, BIG), (16384, 65, 100, BIG),
         (16384, 3, 33, 0)]


def _ops():
    from witw_amd import ops
    return ops


def _inputs(bo, bs, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = torch.rand((bo, bs), generator=g)
    five = torch.randint(0, 5, (bo, bs), generator=g).float()       # runs of equal values across every boundary of 32
    equal = rnd.clone()
    equal[:, bs // 2] = 0.25                                        # an all-equal column
    inf = five.clone()
    inf[torch.rand((bo, bs), generator=g) < 0.6] = float('inf')     # fewer finite rows than places in many columns
    inf[:, 0] = float('inf')
    nan = inf.clone()
    nan[torch.rand((bo, bs), generator=g) < 0.3] = float('nan')
    return {'random': rnd, 'five_values': five, 'equal_column': equal, 'inf': inf, 'nan': nan}


def _expected(dist, k, row_offset=0):
    """first k of the stable sort of every column (NaN as +inf: the kernels' rule), places beyond the rows present (+inf, -1)"""
    d = torch.where(torch.isnan(dist), torch.full_like(dist, float('inf')), dist)
    v, i = torch.sort(d.t().contiguous(), dim=1, stable=True)
    pad = max(0, k - d.shape[0])
    v = torch.cat((v[:, :k], torch.full((d.shape[1], pad), float('inf'))), dim=1)
    i = torch.cat((i[:, :k] + row_offset, torch.full((d.shape[1], pad), -1, dtype=torch.int64)), dim=1)
    return v, i


@pytest.mark.parametrize('bo,bs,k,off', CASES, ids=['%dx%d-k%d-off%d' % c for c in CASES])
def test_long_lists_equal_the_stable_sort_and_extend_the_short_list(bo, bs, k, off):
    ops = _ops()
    for name, dist in _inputs(bo, bs, 100 * bo + bs).items():
        d = dist.to(DEV)
        v, i = ops.topk_smallest(d, k, row_offset=off)
        v, i = v.cpu(), i.cpu()
        ev, ei = _expected(dist, k, off)
        assert torch.equal(i, ei), (name, int((i != ei).sum()), (i != ei).nonzero()[:4].tolist())
        assert torch.equal(v, ev), name
        # prefix property: the first 32 places of the k = 100 list are the k = 32 list bit for bit; no row is listed twice
        v100, i100 = ops.topk_smallest(d, 100, row_offset=off)
        v32, i32 = ops.topk_smallest(d, 32, row_offset=off)
        assert torch.equal(v100[:, :32].contiguous().view(torch.int32), v32.view(torch.int32)) and torch.equal(i100[:, :32], i32), name
        srt = torch.sort(i100, dim=1).values
        assert not bool(((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] != -1)).any()), name
        assert bool(((i100 != -1).sum(1) == min(100, bo)).all()), name


def test_refusals(monkeypatch):
    ops = _ops()
    from witw_amd import _lib
    d = torch.rand((50, 7), device=DEV)
    launched = []
    check = _lib.check
    with monkeypatch.context() as m:
        m.setattr(_lib, 'check', lambda rc, what: (launched.append(what), check(rc, what))[1])
        for k in (0, 1025):
            with pytest.raises(_lib.WitwError, match=r'k=%d outside \[1,1024\]' % k):
                ops.topk_smallest(d, k)
        ops.topk_smallest(d, 33)
    assert launched == ['witw_topk_smallest_ws', 'witw_topk_smallest_after']      # the refused calls reached no entry
    lib = _lib.load()
    v = torch.full((7, 33), -1.0, device=DEV)
    i = torch.full((7, 33), -7, dtype=torch.int64, device=DEV)
    bv, bi = torch.zeros((7,), device=DEV), torch.zeros((7,), dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.witw_topk_smallest_after(d.data_ptr(), v.data_ptr(), i.data_ptr(), 50, 7, 33, 0, bv.data_ptr(), bi.data_ptr(), None, st) == -1
    assert b'k=33' in lib.witw_last_error()
    for nv, ni in ((None, bi.data_ptr()), (bv.data_ptr(), None), (None, None)):
        assert lib.witw_topk_smallest_after(d.data_ptr(), v.data_ptr(), i.data_ptr(), 50, 7, 32, 0, nv, ni, None, st) == -1
        assert b'null bound' in lib.witw_last_error()
    torch.cuda.synchronize()
    assert bool((v == -1.0).all()) and bool((i == -7).all())          # nothing ran


# ---------------------------------------------------------------------------------------------------- retrieve_topk(k=100)
G, Q, K = 300, 70, 100


def _embeddings(we):
    g = torch.Generator().manual_seed(700 + we)
    return torch.randn((G, 16, 4, 64), generator=g).to(DEV), torch.randn((Q, 16, 4, we), generator=g).to(DEV)


def _sorted_lists(dist, k):
    v, i = torch.sort(dist.t().contiguous().cpu(), dim=1, stable=True)
    return v[:, :k], i[:, :k]


@pytest.mark.parametrize('we', [64, 12])
def test_retrieve_topk_100_direct_fixed_and_dft(we):
    ops = _ops()
    from witw_amd import cvig_fov
    gal, qry = _embeddings(we)
    ev, ei = _sorted_lists(ops.match_fwd(gal, qry)[1], K)
    v, i = cvig_fov.retrieve_topk(gal, qry, k=K, method='direct')
    assert tuple(i.shape) == (Q, K) and torch.equal(i.cpu(), ei) and torch.equal(v.cpu(), ev)
    shift = torch.randint(0, 64, (Q,), generator=torch.Generator().manual_seed(we)).to(DEV)
    fv, fi = _sorted_lists(ops.match_fwd_fixed(gal, qry, shift)[1], K)
    v, i = cvig_fov.retrieve_topk(gal, qry, k=K, method='fixed', known_shift=shift)
    assert torch.equal(i.cpu(), fi) and torch.equal(v.cpu(), fv)
    assert not torch.equal(fi, ei)                                   # the prior matters
    # spectral: no room for the candidate margin in 32 places, so the lists are the direct pass's and the ranks the spectral pass's
    r_direct = cvig_fov.retrieve(gal, qry, k=K, method='direct')[0]
    r, v, i = cvig_fov.retrieve(gal, qry, k=K, method='dft')
    np.testing.assert_array_equal(r, r_direct)
    assert torch.equal(i.cpu(), ei) and torch.equal(v.cpu(), ev)
    # a two-chunk pass and a list longer than the gallery
    v, i = cvig_fov.retrieve_topk(gal, qry, k=G + 20, query_chunk=48)
    full_v, full_i = _sorted_lists(ops.match_fwd(gal, qry)[1], G)
    assert torch.equal(i[:, :G].cpu(), full_i) and bool((i[:, G:] == -1).all()) and bool(torch.isinf(v[:, G:]).all())


def test_retrieve_topk_100_over_three_ragged_shards():
    from witw_amd import cvig_fov
    gal, qry = _embeddings(12)
    gal[250] = gal[2]                                                # equal distances in two shards
    v1, i1 = cvig_fov.retrieve_topk(gal, qry, k=K)
    split = [173, 0, 127]

    def fn(rank):
        torch.cuda.set_device(DEV)
        g0 = sum(split[:rank])
        out = cvig_fov.retrieve_topk(gal[g0:g0 + split[rank]].contiguous(), qry, k=K, shard_begin=g0)
        torch.cuda.synchronize()
        return out
    for v, i in run_ranks(3, fn):
        assert torch.equal(i, i1) and torch.equal(v, v1)


# ---------------------------------------------------------------------------------------------------- memory contract
def _contract_inputs(bo, bs):
    dist = _inputs(bo, bs, bo + bs)['five_values']
    dist[::7, :] += torch.rand((len(range(0, bo, 7)), bs), generator=torch.Generator().manual_seed(bo))
    return dist


@pytest.mark.parametrize('skew', [0, 16])
@pytest.mark.parametrize('bo,bs,k', [(100, 29, 70), (1100, 29, 100)], ids=['single-pass', 'split-rows'])
def test_memory_contract_of_the_long_form(bo, bs, k, skew, monkeypatch):
    """ops.topk_smallest(k > 32) with every allocation of ops -- the list, the slices, the bound arrays, the workspace -- an
    interior view between guard bands and the distances between NaN bands: no band touched, every place stored, the distances
    unmodified, the result that of ordinary allocations. Bs = 29 is ragged against the 64-query tile; 1,100 rows are 3 splits."""
    ops = _ops()
    dist = _contract_inputs(bo, bs)
    assert (ops._lib.load().witw_topk_workspace_bytes(bo, bs, 32) > 0) == (bo > 512)
    plain = ops.topk_smallest(dist.to(DEV), k, row_offset=1000)
    arena = Arena(DEV, skew_bytes=skew)
    with monkeypatch.context() as m:
        m.setattr(ops, 'torch', ArenaTorch(arena))
        d = arena.place(dist, 'distance')
        got = ops.topk_smallest(d, k, row_offset=1000)
        assert len(arena.live) == 1 + 2 + 2 + (bo > 512) + 2 * -(-k // 32)      # distances, list, bounds, workspace, slices
        arena.check(got)
    assert torch.equal(d.cpu().view(torch.int32), dist.view(torch.int32))
    ev, ei = _expected(dist, k, 1000)
    for x, y, e in zip(got, plain, (ev, ei)):
        assert torch.equal(x, y) and torch.equal(x.cpu(), e)


@pytest.mark.parametrize('skew', [0, 16])
@pytest.mark.parametrize('bo,bs,k', [(100, 29, 32), (1100, 29, 17), (16384, 29, 32)], ids=['single-pass', 'split-rows', 'threshold'])
def test_memory_contract_of_the_new_entry(bo, bs, k, skew):
    """witw_topk_smallest_after called directly: distances and bounds between NaN bands, outputs and workspace between guard bands.
    The bound of query q is place 5 + q of its column's list, so the result is places 6 + q onward."""
    ops = _ops()
    lib = ops._lib.load()
    dist = _contract_inputs(bo, bs)
    sv, si = _expected(dist, bo, 1000)
    at = torch.arange(bs) + 5
    bound_v, bound_i = sv[torch.arange(bs), at].contiguous(), si[torch.arange(bs), at].contiguous()
    arena = Arena(DEV, skew_bytes=skew)
    d, bv, bi = arena.place(dist, 'distance'), arena.place(bound_v, 'after_value'), arena.place(bound_i, 'after_index')
    v, i = arena.empty((bs, k), torch.float32), arena.empty((bs, k), torch.int64)
    nws = lib.witw_topk_workspace_bytes(bo, bs, k)
    assert (nws > 0) == (bo > 512)
    ws = arena.empty((nws,), torch.uint8) if nws else None
    rc = lib.witw_topk_smallest_after(d.data_ptr(), v.data_ptr(), i.data_ptr(), bo, bs, k, 1000, bv.data_ptr(), bi.data_ptr(),
                                      ws.data_ptr() if nws else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.witw_last_error()
    arena.check((v, i))
    for placed, src in ((d, dist), (bv, bound_v), (bi, bound_i)):
        assert torch.equal(placed.cpu().view(torch.int32), src.view(torch.int32))
    for q in range(bs):
        assert torch.equal(v[q].cpu(), sv[q, 6 + q:6 + q + k]) and torch.equal(i[q].cpu(), si[q, 6 + q:6 + q + k]), q
