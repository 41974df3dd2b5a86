"""The host layer of the matching path pinned without a GPU: which op sees which slice of which orientation prior, and in which
order the ranks exchange data.

* retrieve(method='fixed') / retrieve_topk / sharded_ranks(known_shift=) against retrieve(method='direct') under the one-bit masks
  1 << (shift & 63), on a float64 op set (a pair's distance does not depend on its shard): ranks, values and indices are EQUAL, in
  one process and on two rank-threads with ragged gallery shards (14 + 9, and 23 + 0: a rank without rows).
* the call trace of retrieve() for every resolved method and kind of prior -- op, operand shapes, which prior keyword with how
  many entries -- and the collectives of a two-rank run, against literal lists recorded from the implementation these tests were
  written for: same calls, same exchanges, same order.
* the band-overflow redo of the spectral pass (a list capacity of 0 sends every chunk with a band through it)."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from witw_amd import cvig_fov, parallel, synth

from . import match_window_ref as R
from .test_match_dft_window import MaskedSpectralCpuResolved
from .threaded_world import run_ranks


class Fp64Kernels(MaskedSpectralCpuResolved):
    """the masked float64 op set with the fixed forward: the distance R.match_fused gives under the one-bit word of the shift"""

    @classmethod
    def match_fwd_fixed(cls, ov, su, shift, want_score=False, want_workspace=False, want_orientation=True):
        ori, d, _gap = R.match_fused(ov, su, torch.ones_like(shift) << (shift & 63))
        return (ori if want_orientation else None), d


def _onebit(shift):
    return torch.ones_like(shift) << (shift & 63)


# ----------------------------------------------------------------------------- fixed retrieval == one-bit masks
N_G, N_Q, WE, CHUNK, K = 23, 11, 8, 4, 3


def _fixed_problem():
    gal = torch.from_numpy(synth.embeddings(61, 1, (N_G, 16, 4, 64)))
    gal[7] = gal[3]                                                   # an exact tie between two gallery rows
    shift = (7 * torch.arange(N_Q) + 3) % 64
    shift[0], shift[1] = 0, 63
    planted = torch.where(torch.arange(N_Q) % 2 == 0, shift, (shift + 9) % 64)      # every other query is known wrongly
    qry = torch.stack([torch.roll(gal[i], -int(planted[i]), dims=2)[:, :, :WE] for i in range(N_Q)]) \
        + 3.0 * torch.from_numpy(synth.embeddings(61, 2, (N_Q, 16, 4, WE)))
    return gal.contiguous(), qry.contiguous(), shift + 64 * (torch.arange(N_Q) % 3)      # & 63 is part of the contract


def _fixed_calls(gal, qry, shift, g0=0):
    """(ranks, values, indices) of retrieve(method='fixed'), retrieve_topk's lists, sharded_ranks' ranks and the shift slices
    sharded_ranks handed its injected match"""
    seen = []

    def match(ov, su, known_shift):
        seen.append(tuple(known_shift.tolist()))
        return Fp64Kernels.match_fwd_fixed(ov, su, known_shift)

    r, v, i = cvig_fov.retrieve(gal, qry, k=K, shard_begin=g0, query_chunk=CHUNK, method='fixed', _kernels=Fp64Kernels,
                                known_shift=shift)
    vt, it = cvig_fov.retrieve_topk(gal, qry, k=K, shard_begin=g0, query_chunk=CHUNK, method='fixed', _kernels=Fp64Kernels,
                                    known_shift=shift)
    rs = cvig_fov.sharded_ranks(gal, qry, g0, query_chunk=CHUNK, _match=match, _count=Fp64Kernels.rank_count_thresh,
                                known_shift=shift)
    return np.asarray(r), v.clone(), i.clone(), vt.clone(), it.clone(), np.asarray(rs), seen


@pytest.fixture(scope='module')
def fixed_reference():
    gal, qry, shift = _fixed_problem()
    r, v, i = cvig_fov.retrieve(gal, qry, k=K, query_chunk=CHUNK, method='direct', _kernels=Fp64Kernels, shift_mask=_onebit(shift))
    r_free = cvig_fov.retrieve(gal, qry, k=K, query_chunk=CHUNK, method='direct', _kernels=Fp64Kernels)[0]
    assert not np.array_equal(r, r_free)                              # the known shifts do change the ranks of this problem
    return gal, qry, shift, np.asarray(r), v, i


def _assert_fixed_equals_reference(got, ref, slices):
    _gal, _qry, _shift, r0, v0, i0 = ref
    r, v, i, vt, it, rs, seen = got
    np.testing.assert_array_equal(r, r0)
    assert torch.equal(v, v0) and torch.equal(i, i0)
    assert torch.equal(vt, v0) and torch.equal(it, i0)
    np.testing.assert_array_equal(rs, r0)
    assert seen == slices


def test_fixed_retrieval_equals_one_bit_masks(fixed_reference):
    gal, qry, shift = fixed_reference[:3]
    slices = [tuple(shift[a:a + CHUNK].tolist()) for a in range(0, N_Q, CHUNK)]
    _assert_fixed_equals_reference(_fixed_calls(gal, qry, shift), fixed_reference, slices)


@pytest.mark.parametrize('split', [(14, 9), (23, 0)])
def test_fixed_retrieval_on_two_ranks_with_ragged_shards(fixed_reference, split):
    gal, qry, shift = fixed_reference[:3]
    slices = [tuple(shift[a:a + CHUNK].tolist()) for a in range(0, N_Q, CHUNK)]

    def fn(rank):
        g0 = sum(split[:rank])
        return _fixed_calls(gal[g0:g0 + split[rank]], qry, shift, g0)
    for rank, got in enumerate(run_ranks(2, fn)):
        _assert_fixed_equals_reference(got, fixed_reference, slices if split[rank] else [])      # no rows: no match call


# ----------------------------------------------------------------------------- call trace
class Recording(object):
    """An op set that hands every call to `inner` and logs it as 'op <shape of every tensor operand> <prior keyword>[entries]'.
    The shift of match_fwd_fixed (its third operand) is logged as known_shift[n]."""

    def __init__(self, inner):
        self.inner, self.log = inner, []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)          # AttributeError for an op the inner set lacks, as hasattr() expects
        if not callable(fn):
            return fn

        def call(*a, **kw):
            a_t = [t for t in a if isinstance(t, torch.Tensor)]
            prior = ['%s[%d]' % (key, kw[key].shape[0]) for key in ('shift_mask', 'known_shift') if key in kw]
            if name == 'match_fwd_fixed':
                prior.append('known_shift[%d]' % a_t.pop(2).shape[0])
            self.log.append(' '.join([name] + ['x'.join(str(n) for n in t.shape) for t in a_t] + prior))
            return fn(*a, **kw)
        return call


T_G, T_Q, T_CHUNK = 40, 10, 4


def _trace_problem(we):
    """Well separated rows plus exact duplicates, so that what is re-scored follows from the structure: rows 3 / 7 tie for
    query 3 (its candidates are re-scored), and query 5 looks like the twelve equal rows 20..31 -- more ties than candidates
    are kept, the direct fallback."""
    gal = torch.from_numpy(synth.embeddings(71, 1, (T_G, 16, 4, 64)))
    gal[7] = gal[3]
    gal[20:32] = gal[20]
    src = list(range(T_Q))
    src[5] = 20
    shift = (5 * torch.arange(T_Q) + 2) % 64
    qry = torch.stack([torch.roll(gal[src[i]], -int(shift[i]), dims=2)[:, :, :we] for i in range(T_Q)]) \
        + 0.5 * torch.from_numpy(synth.embeddings(71, 2, (T_Q, 16, 4, we)))
    mask = R.window_words([(int(s) - 2) % 64 for s in shift], [1 + i % 6 + 2 for i in range(T_Q)])
    mask[2::3] = 0                                                    # a third of the queries: no prior
    return gal.contiguous(), qry.contiguous(), mask, shift


TRACE_CASES = {
    'direct': dict(method='direct', k=3),
    'direct_mask': dict(method='direct', k=3, prior='mask'),
    'fixed': dict(method='fixed', k=3, prior='shift'),
    'dft': dict(method='dft', k=3),
    'dft_masked': dict(method='dft_masked', k=3, prior='mask'),
    'dft_masked_k27': dict(method='dft_masked', k=27, prior='mask'),      # k + DFT_MARGIN > 32: ranks spectral, lists direct
}


def _traced_retrieve(case, we, gal=None, g0=0):
    full, qry, mask, shift = _trace_problem(we)
    cfg = TRACE_CASES[case]
    prior = {'mask': {'shift_mask': mask}, 'shift': {'known_shift': shift}, None: {}}[cfg.get('prior')]
    kn = Recording(Fp64Kernels)
    out = cvig_fov.retrieve(full if gal is None else gal, qry, k=cfg['k'], shard_begin=g0, query_chunk=T_CHUNK, method=cfg['method'],
                            _kernels=kn, **prior)
    return kn.log, out


# recorded call by call; match_pairs' last two operands are the pair lists, so their lengths are the pairs re-scored
TRACES = {('dft', 8): ['match_spectrum 40x16x4x64',
              'match_fwd_dft 40x16x4x64 4x16x4x8',
              'match_pairs 40x16x4x64 4x16x4x8 2560 4 12 12',
              'match_pairs 40x16x4x64 4x16x4x8 2560 4 4 4',
              'rank_count_resolved 40x4 4 40x16x4x64 4x16x4x8 2560 4',
              'topk_smallest 40x4',
              'match_fwd_dft 40x16x4x64 4x16x4x8',
              'match_pairs 40x16x4x64 4x16x4x8 2560 4 14 14',
              'match_pairs 40x16x4x64 4x16x4x8 2560 4 4 4',
              'rank_count_resolved 40x4 4 40x16x4x64 4x16x4x8 2560 4',
              'topk_smallest 40x4',
              'match_fwd_dft 40x16x4x64 2x16x4x8',
              'match_pairs 40x16x4x64 2x16x4x8 2560 2 3 3',
              'match_pairs 40x16x4x64 2x16x4x8 2560 2 2 2',
              'rank_count_resolved 40x2 2 40x16x4x64 2x16x4x8 2560 2',
              'topk_smallest 40x2',
              'match_pairs 40x16x4x64 10x16x4x8 2560 10 63 63',
              'match_fwd 40x16x4x64 1x16x4x8',
              'topk_smallest 40x1'],
 ('dft', 64): ['match_spectrum 40x16x4x64',
               'match_fwd_dft 40x16x4x64 4x16x4x64',
               'match_pairs 40x16x4x64 4x16x4x64 2560 4 4 4',
               'rank_count_resolved 40x4 4 40x16x4x64 4x16x4x64 2560 4',
               'topk_smallest 40x4',
               'match_fwd_dft 40x16x4x64 4x16x4x64',
               'match_pairs 40x16x4x64 4x16x4x64 2560 4 4 4',
               'rank_count_resolved 40x4 4 40x16x4x64 4x16x4x64 2560 4',
               'topk_smallest 40x4',
               'match_fwd_dft 40x16x4x64 2x16x4x64',
               'match_pairs 40x16x4x64 2x16x4x64 2560 2 2 2',
               'rank_count_resolved 40x2 2 40x16x4x64 2x16x4x64 2560 2',
               'topk_smallest 40x2',
               'match_pairs 40x16x4x64 10x16x4x64 2560 10 72 72',
               'match_fwd 40x16x4x64 1x16x4x64',
               'topk_smallest 40x1'],
 ('dft_masked', 8): ['match_spectrum 40x16x4x64',
                     'match_fwd_dft 40x16x4x64 4x16x4x8 shift_mask[4]',
                     'match_pairs 40x16x4x64 4x16x4x8 2560 4 5 5 shift_mask[4]',
                     'match_pairs 40x16x4x64 4x16x4x8 2560 4 4 4 shift_mask[4]',
                     'rank_count_resolved 40x4 4 40x16x4x64 4x16x4x8 2560 4 shift_mask[4]',
                     'topk_smallest 40x4',
                     'match_fwd_dft 40x16x4x64 4x16x4x8 shift_mask[4]',
                     'match_pairs 40x16x4x64 4x16x4x8 2560 4 6 6 shift_mask[4]',
                     'match_pairs 40x16x4x64 4x16x4x8 2560 4 4 4 shift_mask[4]',
                     'rank_count_resolved 40x4 4 40x16x4x64 4x16x4x8 2560 4 shift_mask[4]',
                     'topk_smallest 40x4',
                     'match_fwd_dft 40x16x4x64 2x16x4x8 shift_mask[2]',
                     'match_pairs 40x16x4x64 2x16x4x8 2560 2 7 7 shift_mask[2]',
                     'match_pairs 40x16x4x64 2x16x4x8 2560 2 2 2 shift_mask[2]',
                     'rank_count_resolved 40x2 2 40x16x4x64 2x16x4x8 2560 2 shift_mask[2]',
                     'topk_smallest 40x2',
                     'match_pairs 40x16x4x64 10x16x4x8 2560 10 63 63 shift_mask[10]',
                     'match_fwd 40x16x4x64 1x16x4x8 shift_mask[1]',
                     'topk_smallest 40x1'],
 ('dft_masked', 64): ['match_spectrum 40x16x4x64',
                      'match_fwd_dft 40x16x4x64 4x16x4x64 shift_mask[4]',
                      'match_pairs 40x16x4x64 4x16x4x64 2560 4 4 4 shift_mask[4]',
                      'rank_count_resolved 40x4 4 40x16x4x64 4x16x4x64 2560 4 shift_mask[4]',
                      'topk_smallest 40x4',
                      'match_fwd_dft 40x16x4x64 4x16x4x64 shift_mask[4]',
                      'match_pairs 40x16x4x64 4x16x4x64 2560 4 4 4 shift_mask[4]',
                      'rank_count_resolved 40x4 4 40x16x4x64 4x16x4x64 2560 4 shift_mask[4]',
                      'topk_smallest 40x4',
                      'match_fwd_dft 40x16x4x64 2x16x4x64 shift_mask[2]',
                      'match_pairs 40x16x4x64 2x16x4x64 2560 2 2 2 shift_mask[2]',
                      'rank_count_resolved 40x2 2 40x16x4x64 2x16x4x64 2560 2 shift_mask[2]',
                      'topk_smallest 40x2',
                      'match_pairs 40x16x4x64 10x16x4x64 2560 10 54 54 shift_mask[10]',
                      'match_fwd 40x16x4x64 1x16x4x64 shift_mask[1]',
                      'topk_smallest 40x1'],
 ('dft_masked_k27', 8): ['match_spectrum 40x16x4x64',
                         'match_fwd_dft 40x16x4x64 4x16x4x8 shift_mask[4]',
                         'match_pairs 40x16x4x64 4x16x4x8 2560 4 5 5 shift_mask[4]',
                         'match_pairs 40x16x4x64 4x16x4x8 2560 4 4 4 shift_mask[4]',
                         'rank_count_resolved 40x4 4 40x16x4x64 4x16x4x8 2560 4 shift_mask[4]',
                         'topk_smallest 40x4',
                         'match_fwd_dft 40x16x4x64 4x16x4x8 shift_mask[4]',
                         'match_pairs 40x16x4x64 4x16x4x8 2560 4 6 6 shift_mask[4]',
                         'match_pairs 40x16x4x64 4x16x4x8 2560 4 4 4 shift_mask[4]',
                         'rank_count_resolved 40x4 4 40x16x4x64 4x16x4x8 2560 4 shift_mask[4]',
                         'topk_smallest 40x4',
                         'match_fwd_dft 40x16x4x64 2x16x4x8 shift_mask[2]',
                         'match_pairs 40x16x4x64 2x16x4x8 2560 2 7 7 shift_mask[2]',
                         'match_pairs 40x16x4x64 2x16x4x8 2560 2 2 2 shift_mask[2]',
                         'rank_count_resolved 40x2 2 40x16x4x64 2x16x4x8 2560 2 shift_mask[2]',
                         'topk_smallest 40x2',
                         'match_pairs 40x16x4x64 10x16x4x8 2560 10 21 21 shift_mask[10]',
                         'match_fwd 40x16x4x64 1x16x4x8 shift_mask[1]',
                         'topk_smallest 40x1',
                         'match_fwd 40x16x4x64 4x16x4x8 shift_mask[4]',
                         'topk_smallest 40x4',
                         'match_fwd 40x16x4x64 4x16x4x8 shift_mask[4]',
                         'topk_smallest 40x4',
                         'match_fwd 40x16x4x64 2x16x4x8 shift_mask[2]',
                         'topk_smallest 40x2'],
 ('dft_masked_k27', 64): ['match_spectrum 40x16x4x64',
                          'match_fwd_dft 40x16x4x64 4x16x4x64 shift_mask[4]',
                          'match_pairs 40x16x4x64 4x16x4x64 2560 4 4 4 shift_mask[4]',
                          'rank_count_resolved 40x4 4 40x16x4x64 4x16x4x64 2560 4 shift_mask[4]',
                          'topk_smallest 40x4',
                          'match_fwd_dft 40x16x4x64 4x16x4x64 shift_mask[4]',
                          'match_pairs 40x16x4x64 4x16x4x64 2560 4 4 4 shift_mask[4]',
                          'rank_count_resolved 40x4 4 40x16x4x64 4x16x4x64 2560 4 shift_mask[4]',
                          'topk_smallest 40x4',
                          'match_fwd_dft 40x16x4x64 2x16x4x64 shift_mask[2]',
                          'match_pairs 40x16x4x64 2x16x4x64 2560 2 2 2 shift_mask[2]',
                          'rank_count_resolved 40x2 2 40x16x4x64 2x16x4x64 2560 2 shift_mask[2]',
                          'topk_smallest 40x2',
                          'match_pairs 40x16x4x64 10x16x4x64 2560 10 21 21 shift_mask[10]',
                          'match_fwd 40x16x4x64 1x16x4x64 shift_mask[1]',
                          'topk_smallest 40x1',
                          'match_fwd 40x16x4x64 4x16x4x64 shift_mask[4]',
                          'topk_smallest 40x4',
                          'match_fwd 40x16x4x64 4x16x4x64 shift_mask[4]',
                          'topk_smallest 40x4',
                          'match_fwd 40x16x4x64 2x16x4x64 shift_mask[2]',
                          'topk_smallest 40x2'],
 ('direct', 8): ['match_fwd 40x16x4x64 4x16x4x8',
                 'rank_count_thresh 40x4 4',
                 'topk_smallest 40x4',
                 'match_fwd 40x16x4x64 4x16x4x8',
                 'rank_count_thresh 40x4 4',
                 'topk_smallest 40x4',
                 'match_fwd 40x16x4x64 2x16x4x8',
                 'rank_count_thresh 40x2 2',
                 'topk_smallest 40x2'],
 ('direct', 64): ['match_fwd 40x16x4x64 4x16x4x64',
                  'rank_count_thresh 40x4 4',
                  'topk_smallest 40x4',
                  'match_fwd 40x16x4x64 4x16x4x64',
                  'rank_count_thresh 40x4 4',
                  'topk_smallest 40x4',
                  'match_fwd 40x16x4x64 2x16x4x64',
                  'rank_count_thresh 40x2 2',
                  'topk_smallest 40x2'],
 ('direct_mask', 8): ['match_fwd 40x16x4x64 4x16x4x8 shift_mask[4]',
                      'rank_count_thresh 40x4 4',
                      'topk_smallest 40x4',
                      'match_fwd 40x16x4x64 4x16x4x8 shift_mask[4]',
                      'rank_count_thresh 40x4 4',
                      'topk_smallest 40x4',
                      'match_fwd 40x16x4x64 2x16x4x8 shift_mask[2]',
                      'rank_count_thresh 40x2 2',
                      'topk_smallest 40x2'],
 ('direct_mask', 64): ['match_fwd 40x16x4x64 4x16x4x64 shift_mask[4]',
                       'rank_count_thresh 40x4 4',
                       'topk_smallest 40x4',
                       'match_fwd 40x16x4x64 4x16x4x64 shift_mask[4]',
                       'rank_count_thresh 40x4 4',
                       'topk_smallest 40x4',
                       'match_fwd 40x16x4x64 2x16x4x64 shift_mask[2]',
                       'rank_count_thresh 40x2 2',
                       'topk_smallest 40x2'],
 ('fixed', 8): ['match_fwd_fixed 40x16x4x64 4x16x4x8 known_shift[4]',
                'rank_count_thresh 40x4 4',
                'topk_smallest 40x4',
                'match_fwd_fixed 40x16x4x64 4x16x4x8 known_shift[4]',
                'rank_count_thresh 40x4 4',
                'topk_smallest 40x4',
                'match_fwd_fixed 40x16x4x64 2x16x4x8 known_shift[2]',
                'rank_count_thresh 40x2 2',
                'topk_smallest 40x2'],
 ('fixed', 64): ['match_fwd_fixed 40x16x4x64 4x16x4x64 known_shift[4]',
                 'rank_count_thresh 40x4 4',
                 'topk_smallest 40x4',
                 'match_fwd_fixed 40x16x4x64 4x16x4x64 known_shift[4]',
                 'rank_count_thresh 40x4 4',
                 'topk_smallest 40x4',
                 'match_fwd_fixed 40x16x4x64 2x16x4x64 known_shift[2]',
                 'rank_count_thresh 40x2 2',
                 'topk_smallest 40x2']}


@pytest.mark.parametrize('we', [8, 64])
@pytest.mark.parametrize('case', sorted(TRACE_CASES))
def test_retrieve_call_trace(case, we):
    log, (ranks, v, i) = _traced_retrieve(case, we)
    assert log == TRACES[case, we]
    # and whatever the pass, the answer is that of the direct one under the same prior
    full, qry, mask, shift = _trace_problem(we)
    k = TRACE_CASES[case]['k']
    prior = {'mask': mask, 'shift': _onebit(shift), None: None}[TRACE_CASES[case].get('prior')]
    r0, _v0, i0 = cvig_fov.retrieve(full, qry, k=k, query_chunk=T_CHUNK, method='direct', _kernels=Fp64Kernels, shift_mask=prior)
    np.testing.assert_array_equal(ranks, r0)
    assert torch.equal(i, i0)


# ----------------------------------------------------------------------------- collectives of a two-rank run
T_SPLIT = (27, 13)


def _two_rank_exchanges(monkeypatch):
    """every parallel.all_reduce_sum_ / parallel._all_gather_cat of both ranks, as 'name shape', through one call of each chunked
    path: direct under a mask, fixed, the masked spectral pass on narrow surfaces, sharded_ranks at known shifts"""
    logs = {0: [], 1: []}
    for name in ('all_reduce_sum_', '_all_gather_cat'):
        def wrapped(t, _name=name, _fn=getattr(parallel, name)):
            logs[dist.get_rank()].append('%s %s' % (_name, 'x'.join(str(n) for n in t.shape)))
            return _fn(t)
        monkeypatch.setattr(parallel, name, wrapped)
    full, qry, mask, shift = _trace_problem(8)

    def fn(rank):
        g0 = sum(T_SPLIT[:rank])
        gal = full[g0:g0 + T_SPLIT[rank]]
        for method, prior in (('direct', {'shift_mask': mask}), ('fixed', {'known_shift': shift}), ('dft_masked', {'shift_mask': mask})):
            logs[rank].append('-- ' + method)
            cvig_fov.retrieve(gal, qry, k=3, shard_begin=g0, query_chunk=T_CHUNK, method=method, _kernels=Fp64Kernels, **prior)
        logs[rank].append('-- sharded_ranks')
        cvig_fov.sharded_ranks(gal, qry, g0, query_chunk=T_CHUNK, _count=Fp64Kernels.rank_count_thresh, known_shift=shift,
                               _match=lambda ov, su, known_shift: Fp64Kernels.match_fwd_fixed(ov, su, known_shift))
    run_ranks(2, fn)
    return logs


# the same on both ranks; the spectral pass ends with its candidate lists, the best outsider, the exact candidate distances of
# the 7 undecided queries and the fallback query's direct lists
EXCHANGES = ['-- direct',
 'all_reduce_sum_ 4',
 'all_reduce_sum_ 4',
 'all_reduce_sum_ 2',
 'all_reduce_sum_ 10',
 '_all_gather_cat 1x10x3',
 '_all_gather_cat 1x10x3',
 '-- fixed',
 'all_reduce_sum_ 4',
 'all_reduce_sum_ 4',
 'all_reduce_sum_ 2',
 'all_reduce_sum_ 10',
 '_all_gather_cat 1x10x3',
 '_all_gather_cat 1x10x3',
 '-- dft_masked',
 'all_reduce_sum_ 4',
 'all_reduce_sum_ 4',
 'all_reduce_sum_ 2',
 'all_reduce_sum_ 10',
 '_all_gather_cat 1x10x9',
 '_all_gather_cat 1x10x9',
 '_all_gather_cat 1x10',
 'all_reduce_sum_ 7x9',
 '_all_gather_cat 1x1x3',
 '_all_gather_cat 1x1x3',
 '-- sharded_ranks',
 'all_reduce_sum_ 4',
 'all_reduce_sum_ 4',
 'all_reduce_sum_ 2',
 'all_reduce_sum_ 10']


def test_two_rank_exchanges_in_order(monkeypatch):
    logs = _two_rank_exchanges(monkeypatch)
    assert logs[0] == EXCHANGES and logs[1] == EXCHANGES


# ----------------------------------------------------------------------------- band overflow
class OverflowingKernels(Fp64Kernels):
    """a band list without room: every chunk whose band is not empty reports an overflow and is redone through rank_count_band"""
    redone = 0

    @classmethod
    def rank_count_resolved(cls, dist, thr, eps, ov, su, wn, sn, **kw):
        cls.redone -= 1                                 # the stand-in counts its band through rank_count_band itself
        c, n, _cap = super().rank_count_resolved(dist, thr, eps, ov, su, wn, sn, **kw)
        return torch.full_like(c, -1000), n, 0          # counts of an overflowed list are not to be used

    @classmethod
    def rank_count_band(cls, dist, thr, eps):
        cls.redone += 1
        return super().rank_count_band(dist, thr, eps)


@pytest.mark.parametrize('chunk', [4, 16])      # several chunks: the pass is run again; one chunk: its distances were kept
@pytest.mark.parametrize('we', [8, 64])
def test_band_overflow_is_redone(we, chunk):
    full, qry, mask, _shift = _trace_problem(we)
    r0 = cvig_fov.retrieve(full, qry, k=3, query_chunk=chunk, method='direct', _kernels=Fp64Kernels, shift_mask=mask)[0]
    OverflowingKernels.redone = 0
    kn = Recording(OverflowingKernels)
    r1 = cvig_fov.retrieve(full, qry, k=3, query_chunk=chunk, method='dft_masked', _kernels=kn, shift_mask=mask)[0]
    np.testing.assert_array_equal(r1, r0)
    assert OverflowingKernels.redone > 0
    passes = [line for line in kn.log if line.startswith('match_fwd_dft')]
    assert len(passes) == (1 if chunk == 16 else 3 + OverflowingKernels.redone)
    assert cvig_fov.last_retrieve_stats()['rescored_rank'] == 0            # min(pairs in the band, capacity 0)
