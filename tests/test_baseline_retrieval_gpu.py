"""cvig_baseline gallery retrieval on the device: the three entries of csrc/baseline_retrieval.hip against float64 and against the
direct kernel's bits, retrieve(method='gemm') against method='direct' and a CPU sort of the full matrix, sharding, the memory
contract of the entries (tests/mem_arena.py) and the test() driver.

Shapes (Ng, Nq, n). The GEMM tile is 128 gallery rows x 128 queries in 32 x 32 MFMA tiles, K runs in stages of 32 floats and rows
are loaded 16 bytes at a time when n is a multiple of 4: (1,1,1) one element of one tile; (31,33,3) / (33,31,70) either side of an
MFMA tile, K below one stage / two full stages and a tail of 6 on the scalar loads; (129,65,1536) two gallery tiles, 48 full
stages on the vector loads; (257,130,1537) three by two tiles with a K tail of one float on rows that are not 16-byte aligned;
(65537,3,8) 513 gallery tiles on gridDim.x, the first row count witw_pairwise_sqdist refuses. The band is never calibrated here:
every bound below is cvig_baseline.band_eps or gamma_n, written out in the test."""
import os

import numpy as np
import pytest
import torch

from tests.mem_arena import Arena

from .threaded_world import run_ranks

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
U = 2.0 ** -24
SHAPES = [(1, 1, 1), (31, 33, 3), (33, 31, 70), (129, 65, 1536), (257, 130, 1537), (65537, 3, 8)]
IDS = ['%dx%dx%d' % s for s in SHAPES]


def gamma(m):
    return m * U / (1 - m * U)


def _mods():
    from witw_amd import baseline_retrieval, cvig_baseline, ops
    return ops, baseline_retrieval, cvig_baseline


def _inputs(ng, nq, n, seed):
    """name -> (g, q) on the CPU"""
    ops = _mods()[0]
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=gen)      # noqa: E731
    g = ops.embed_normalize_(rn(ng, n).to(DEV)).cpu()
    out = {'normalized': (g, ops.embed_normalize_(rn(nq, n).to(DEV)).cpu())}
    hg, hq = 1e-3 * rn(ng, n), 1e-3 * rn(nq, n)
    hg[torch.arange(ng), torch.randint(0, n, (ng,), generator=gen)] = 1e3
    hq[torch.arange(nq), torch.randint(0, n, (nq,), generator=gen)] = -1e3
    out['huge_and_tiny'] = (hg, hq)
    rows = torch.arange(nq) % ng
    out['cancellation'] = (g, g[rows] + 1e-4 * rn(nq, n))
    out['duplicates'] = (g, g[rows].clone())
    return out


def _ref_sq(g, q):
    """float64 sum (g - q)^2 [Ng, Nq], in row blocks"""
    g, q = g.double(), q.double()
    step = max(1, (1 << 24) // max(1, q.numel()))
    return torch.cat([((g[r:r + step, None, :] - q[None, :, :]) ** 2).sum(-1) for r in range(0, g.shape[0], step)])


@pytest.mark.parametrize('ng,nq,n', SHAPES, ids=IDS)
def test_gemm_and_norms_within_the_derived_bound_of_float64(ng, nq, n):
    _ops, br, cb = _mods()
    for name, (g, q) in _inputs(ng, nq, n, 1000 * n + ng).items():
        gd, qd = g.to(DEV), q.to(DEV)
        gn, qn = br.row_sqnorm(gd), br.row_sqnorm(qd)
        for x, xn in ((g, gn), (q, qn)):
            exact = (x.double() ** 2).sum(1)
            assert bool(((xn.cpu().double() - exact).abs() <= gamma(n) * exact).all()), (name, 'row_sqnorm')
        D = br.sqdist_gemm(gd, qd, gn, qn).cpu().double()
        bound = 3 * gamma(n + 16) * (gn.cpu().double()[:, None] + qn.cpu().double()[None, :])      # band_eps per element
        assert bound.max().item() == pytest.approx(cb.band_eps(n, gn.max().item(), qn.max().item()), rel=1e-12)
        err = (D - _ref_sq(g, q)).abs()
        print('%s %s: largest share of the bound %.4f' % ((ng, nq, n), name, float((err / bound).max())))
        assert bool((err <= bound).all()), (name, float((err / bound).max()))
        assert bool((D >= 0).all())


@pytest.mark.parametrize('ng,nq,n', SHAPES[:5], ids=IDS[:5])
def test_pairs_are_the_direct_kernels_bits(ng, nq, n):
    ops, br, _cb = _mods()
    gen = torch.Generator().manual_seed(ng + n)
    for name, (g, q) in _inputs(ng, nq, n, 7 * n + nq).items():
        gd, qd = g.to(DEV), q.to(DEV)
        pg = torch.randint(0, ng, (300,), generator=gen)
        pq = torch.randint(0, nq, (300,), generator=gen)
        pg[100:200], pq[100:200] = pg[:100], pq[:100]                # repeated pairs
        desc = torch.argsort(pg * nq + pq, descending=True)
        for a, b in ((pg, pq), (pg[desc], pq[desc]), (pg[:1], pq[:1])):
            for root in (False, True):
                full = ops.pairwise_sqdist(gd, qd, take_sqrt=root)
                got = br.sqdist_pairs(gd, qd, a.to(DEV, torch.int32), b.to(DEV, torch.int32), take_sqrt=root)
                assert torch.equal(got.view(torch.int32), full[a.to(DEV), b.to(DEV)].view(torch.int32)), (name, root, a.numel())
    assert br.sqdist_pairs(gd, qd, torch.zeros((0,), dtype=torch.int32, device=DEV), torch.zeros((0,), dtype=torch.int32, device=DEV)).numel() == 0


# ---------------------------------------------------------------------------------------------------- index-exactness
G, Q, E = 2000, 300, 1536


def _cpu_reference(D):
    """D [G, Q] Euclidean on the CPU -> (ranks int64 [Q], stable sort of every column: values, indices)"""
    nq = D.shape[1]
    ranks = (D <= D[torch.arange(nq), torch.arange(nq)][None, :]).sum(0).numpy().astype('int64')
    v, i = torch.sort(D.t().contiguous(), dim=1, stable=True)
    return ranks, v, i


@pytest.fixture(scope='module')
def hard():
    """2,000 gallery rows (50 exact duplicates of other rows, 50 that differ from another row in the last bit of one component),
    300 queries = their true row plus noise at graded levels (below). Computed once, never modified."""
    ops, _br, cb = _mods()
    gen = torch.Generator().manual_seed(2024)
    gal = ops.embed_normalize_(torch.randn((G, E), generator=gen).to(DEV))
    gal[1900:1950] = gal[100:150]
    near = gal[200:250].clone().view(torch.int32)
    near[torch.arange(50), torch.randint(0, E, (50,), generator=gen).to(DEV)] += 1
    gal[1950:2000] = near.view(torch.float32)
    # graded: query q is its true row pulled towards the origin (where every row is about equally far) by 10^-(0 .. 2.3), plus
    # noise of 0.05 per component -- the last third of the queries loses its true row among hundreds of others, while every norm
    # stays that of an embedding (one eps serves the whole pass: a query set of very unequal norms would widen everyone's band)
    pull = 10.0 ** -torch.linspace(0, 2.3, Q)
    qry = (pull[:, None] * gal[:Q].cpu() + 0.05 * torch.randn((Q, E), generator=gen)).to(DEV)
    ranks, v, i = _cpu_reference(ops.pairwise_sqdist(gal, qry, take_sqrt=True).cpu())
    # the input admits the condition below: in float64 the band of the derived eps around each true squared distance holds at
    # most 5 % of the pairs (0.4 % here)
    g64, q64 = gal.cpu().double(), qry.cpu().double()
    gn, qn = (g64 ** 2).sum(1), (q64 ** 2).sum(1)
    sq = (gn[:, None] + qn[None, :] - 2 * g64 @ q64.t()).clamp(min=0)
    eps = cb.band_eps(E, gn.max().item() * (1 + gamma(E)), qn.max().item() * (1 + gamma(E)))
    share = float(((sq - sq[torch.arange(Q), torch.arange(Q)][None, :]).abs() <= eps).double().mean())
    print('share of the pairs inside the float64 band: %.5f' % share)
    assert share <= 0.05
    assert ranks.min() == 1 and ranks.max() >= 200 and len(set(ranks.tolist())) > 50       # ranks spread from 1 to hundreds
    return {'gal': gal, 'qry': qry, 'ranks': ranks, 'v': v, 'i': i}


@pytest.mark.parametrize('k', [1, 10, 40, 100])
def test_gemm_equals_direct_equals_the_cpu_sort(hard, k):
    _ops, _br, cb = _mods()
    rd, vd, idd = cb.retrieve(hard['gal'], hard['qry'], k=k, method='direct')
    rg, vg, ig = cb.retrieve(hard['gal'], hard['qry'], k=k, method='gemm')
    st = cb.last_retrieve_stats()
    print('k=%d: %s' % (k, st))
    np.testing.assert_array_equal(rd, hard['ranks'])
    np.testing.assert_array_equal(rg, hard['ranks'])
    assert torch.equal(ig, idd) and torch.equal(vg.view(torch.int32), vd.view(torch.int32))
    assert torch.equal(ig.cpu(), hard['i'][:, :k]) and torch.equal(vg.cpu(), hard['v'][:, :k])
    # not by re-scoring everything
    assert st['pairs'] == G * Q and st['rescored_rank'] / st['pairs'] <= 0.05 and st['fallback_queries'] == 0
    assert st['rescored_topk'] == Q * (k + cb.GEMM_MARGIN) and st['eps'] > 0


def test_well_separated_input_equals_float64_ranks():
    """Collinear rows x_i u (x_i = 1.1^i) and queries y_j u: every distance is |x_i - y_j| |u|, and for every query the sorted
    float64 distances are at least 1e-3 apart relatively (checked), far above fp32 rounding: float64 ranks are THE ranks."""
    ops, _br, cb = _mods()
    gen = torch.Generator().manual_seed(7)
    n_rows = 40
    u = torch.randn((E,), generator=gen)
    x = 1.1 ** torch.arange(n_rows, dtype=torch.float64)
    y = x * torch.tensor([1.04, 1.3, 0.88, 1.7] * 10, dtype=torch.float64)
    gal, qry = (x[:, None] * u.double()).float(), (y[:, None] * u.double()).float()
    d64 = torch.sqrt(_ref_sq(gal, qry))
    srt = torch.sort(d64, dim=0).values
    assert float(((srt[1:] - srt[:-1]) / srt[1:]).min()) >= 1e-3
    r64 = (d64 <= d64[torch.arange(n_rows), torch.arange(n_rows)][None, :]).sum(0).numpy().astype('int64')
    assert r64.max() >= 3
    g, q = gal.to(DEV), qry.to(DEV)
    np.testing.assert_array_equal(cb.ranks(g, q), r64)
    for method in ('direct', 'gemm'):
        r, _v, i = cb.retrieve(g, q, k=5, method=method)
        np.testing.assert_array_equal(r, r64)
        assert torch.equal(i.cpu(), torch.sort(d64.t(), dim=1, stable=True).indices[:, :5])
        np.testing.assert_array_equal(cb.evaluation_ranks(g, q, method=method), r64)


# ---------------------------------------------------------------------------------------------------- sharding
def test_three_ragged_shards_equal_the_unsharded_call(hard):
    _ops, _br, cb = _mods()
    split = [1200, 0, 800]

    def fn(rank):
        torch.cuda.set_device(DEV)
        g0 = sum(split[:rank])
        out = [cb.retrieve(hard['gal'][g0:g0 + split[rank]].contiguous(), hard['qry'], k=10, shard_begin=g0, query_chunk=128, method=m)
               for m in ('direct', 'gemm')]
        torch.cuda.synchronize()
        return out
    for per_method in run_ranks(3, fn):
        for r, v, i in per_method:
            np.testing.assert_array_equal(r, hard['ranks'])
            assert torch.equal(i.cpu(), hard['i'][:, :10]) and torch.equal(v.cpu(), hard['v'][:, :10])


def test_gallery_beyond_65535_rows_whole_and_sharded():
    """70,000 rows x 16: the direct route's blocks of 65,535 rows and the GEMM grid beyond gridDim.y's limit; whole, and as shards
    of 66,000 / 0 / 4,000 rows."""
    ops, _br, cb = _mods()
    gen = torch.Generator().manual_seed(70)
    gal = torch.randn((70000, 16), generator=gen)
    qry = (gal[:5] + torch.tensor([0.01, 0.5, 1.0, 1.5, 2.0])[:, None] * torch.randn((5, 16), generator=gen)).to(DEV)
    gal[69990:69995] = gal[:5]                                       # equal distances either side of the block boundary
    gal = gal.to(DEV)
    D = torch.cat([ops.pairwise_sqdist(gal[r:r + 35000], qry, take_sqrt=True) for r in (0, 35000)]).cpu()
    ranks, ev, ei = _cpu_reference(D)
    assert ranks.max() > 100
    for method in ('direct', 'gemm'):
        r, v, i = cb.retrieve(gal, qry, k=10, method=method)
        np.testing.assert_array_equal(r, ranks)
        assert torch.equal(i.cpu(), ei[:, :10]) and torch.equal(v.cpu(), ev[:, :10])
        np.testing.assert_array_equal(cb.evaluation_ranks(gal, qry, method=method), ranks)
    split = [66000, 0, 4000]

    def fn(rank):
        torch.cuda.set_device(DEV)
        g0 = sum(split[:rank])
        out = [cb.retrieve(gal[g0:g0 + split[rank]], qry, k=10, shard_begin=g0, method=m) for m in ('direct', 'gemm')]
        torch.cuda.synchronize()
        return out
    for per_method in run_ranks(3, fn):
        for r, v, i in per_method:
            np.testing.assert_array_equal(r, ranks)
            assert torch.equal(i.cpu(), ei[:, :10]) and torch.equal(v.cpu(), ev[:, :10])


# ---------------------------------------------------------------------------------------------------- memory contract
@pytest.mark.parametrize('skew', [0, 16])
@pytest.mark.parametrize('ng,nq,n', [(37, 29, 70), (257, 130, 1537)], ids=['37x29x70', '257x130x1537'])
def test_memory_contract_of_the_three_entries(ng, nq, n, skew):
    """Each entry called directly: inputs between NaN bands, outputs between guard bands; every output element stored, no band
    touched, the inputs unmodified, the values those of ordinary allocations."""
    ops, br, _cb = _mods()
    lib = ops._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    g, q = _inputs(ng, nq, n, ng + n)['cancellation']
    gen = torch.Generator().manual_seed(skew + n)
    pg = torch.randint(0, ng, (333,), generator=gen).to(torch.int32)
    pq = torch.randint(0, nq, (333,), generator=gen).to(torch.int32)
    plain_gn, plain_qn = br.row_sqnorm(g.to(DEV)), br.row_sqnorm(q.to(DEV))
    plain_D = br.sqdist_gemm(g.to(DEV), q.to(DEV), plain_gn, plain_qn)
    plain_p = br.sqdist_pairs(g.to(DEV), q.to(DEV), pg.to(DEV), pq.to(DEV), take_sqrt=True)
    arena = Arena(DEV, skew_bytes=skew)
    ga, qa = arena.place(g, 'gallery'), arena.place(q, 'queries')
    gn, qn = arena.empty((ng,), torch.float32), arena.empty((nq,), torch.float32)
    assert lib.witw_row_sqnorm(ga.data_ptr(), gn.data_ptr(), ng, n, st) == 0, lib.witw_last_error()
    assert lib.witw_row_sqnorm(qa.data_ptr(), qn.data_ptr(), nq, n, st) == 0, lib.witw_last_error()
    arena.check((gn, qn))
    assert torch.equal(gn, plain_gn) and torch.equal(qn, plain_qn)
    ga, qa = arena.place(g, 'gallery'), arena.place(q, 'queries')
    gna, qna = arena.place(gn.cpu(), 'gallery norms'), arena.place(qn.cpu(), 'query norms')
    D = arena.empty((ng, nq), torch.float32)
    assert lib.witw_sqdist_gemm(ga.data_ptr(), qa.data_ptr(), gna.data_ptr(), qna.data_ptr(), D.data_ptr(), ng, nq, n, st) == 0, lib.witw_last_error()
    arena.check((D,))
    assert torch.equal(D, plain_D)
    ga, qa = arena.place(g, 'gallery'), arena.place(q, 'queries')
    pga, pqa = arena.place(pg, 'pair_g'), arena.place(pq, 'pair_q')
    out = arena.empty((333,), torch.float32)
    assert lib.witw_sqdist_pairs(ga.data_ptr(), qa.data_ptr(), pga.data_ptr(), pqa.data_ptr(), out.data_ptr(), 333, n, 1, st) == 0, lib.witw_last_error()
    arena.check((out,))
    assert torch.equal(out, plain_p)
    for placed, src in ((ga, g), (qa, q), (pga, pg), (pqa, pq)):
        assert torch.equal(placed.cpu().view(torch.int32), src.view(torch.int32))


def test_entries_refuse_bad_arguments():
    ops, _br, _cb = _mods()
    lib = ops._lib.load()
    x = torch.zeros((4, 8), device=DEV)
    p = x.data_ptr()
    assert lib.witw_row_sqnorm(p, None, 4, 8, None) == -1 and b'null' in lib.witw_last_error()
    assert lib.witw_sqdist_gemm(p, p, p, p, p, 4, 4, 12289, None) == -1 and b'bad shape' in lib.witw_last_error()
    assert lib.witw_sqdist_gemm(p, p, p, p, p, 0, 4, 8, None) == -1 and b'bad shape' in lib.witw_last_error()
    assert lib.witw_sqdist_pairs(p, p, None, None, p, 3, 8, 0, None) == -1 and b'null' in lib.witw_last_error()


# ---------------------------------------------------------------------------------------------------- driver
def test_test_driver_prints_the_same_table_under_gemm(tmp_path, monkeypatch, capsys):
    from PIL import Image
    from witw_amd import cvig_baseline as cb
    from witw_amd import synth
    rows = []
    for i in range(5):
        Image.fromarray(synth.images_u8(72, i, (400, 400, 3)).astype(np.uint8)).save(os.path.join(tmp_path, 'ov_%d.png' % i))
        Image.fromarray(synth.images_u8(73, i, (200, 800, 3)).astype(np.uint8)).save(os.path.join(tmp_path, 'su_%d.png' % i))
        rows.append('ov_%d.png,su_%d.png' % (i, i))
    csv = os.path.join(tmp_path, 'pairs.csv')
    with open(csv, 'w') as f:
        f.write('\n'.join(rows) + '\n')
    monkeypatch.chdir(tmp_path)
    os.makedirs('weights')
    torch.manual_seed(5)
    torch.save(cb.SurfaceEncoder().state_dict(), os.path.join('weights', 'surface_best.pth'))
    torch.save(cb.OverheadEncoder().state_dict(), os.path.join('weights', 'overhead_best.pth'))
    tables, prints = [], []
    for method in (None, 'gemm', 'direct'):
        torch.manual_seed(9)                                         # SyncedRotation draws its angles from torch's generator
        tables.append(cb.test(dataset='cvusa', batch_size=4, num_workers=0, csv_path=csv, match_method=method))
        prints.append(capsys.readouterr().out)
    assert 'Top  1:' in prints[0] and 'Locations: 5' in prints[0]
    assert prints[1] == prints[0] and prints[2] == prints[0] and tables[1] == tables[0] and tables[2] == tables[0]
