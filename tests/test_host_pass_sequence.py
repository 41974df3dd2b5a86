"""The exchanges of the sharded losses and of the gallery retrieval, in order, without a process group and without a GPU.

The oracle tests of these paths (test_parallel_world8_gloo, test_batch_hard, test_baseline_sharded_loss, test_baseline_hard,
test_baseline_retrieval, test_match_host_paths) pin WHAT is computed; this file pins the sequence it is computed in: every
parallel.phase that is opened and closed, every collective with the shape it carries and every op-set call with its operands'
shapes, as ONE ordered list per case. parallel.world / rank / phase / _all_gather_cat / all_reduce_sum_ / reduce_scatter_rows (and
torch.distributed.all_reduce, which the GEMM pass calls for its MAX) are replaced by recording stand-ins that report a world of 1
or 2 on rank 0 -- a gather returns `world` copies of its operand, a sum its operand, the reduce-scatter the first rows -- and the op
sets are the torch renderings the tests above define, behind a recording wrapper.

The literal lists in SEQUENCES were produced by running this recorder (`python -m tests.test_host_pass_sequence` prints them) on
the commit BEFORE the shared host modules witw_amd/slab_loss.py and witw_amd/retrieval.py existed, and pasted here: the four
autograd functions and the two retrieval passes must keep making the same calls in the same order.

Shapes: losses b = 3 pairs per rank (baseline width 8, cvig_fov [3, 2, 2, 64] against [3, 2, 2, 8]); retrieval 7 gallery rows from
shard_begin = 1 on, 5 queries (query 0's true row lies outside the shard), query_chunk = 2: three chunks, the last ragged; k = 3
and a k that leaves no room for the pass's candidate margin."""
import pprint

import pytest
import torch
import torch.distributed as dist

from witw_amd import cvig_baseline, cvig_fov, ops, parallel

from . import baseline_hard_ref, baseline_slab_ref
from . import match_window_ref as R
from .test_baseline_retrieval import _kernels as gemm_kernels
from .test_batch_hard import BatchHardCpuKernels
from .test_match_dft_window import MaskedSpectralCpu, MaskedSpectralCpuResolved
from .test_parallel_world8_gloo import CpuKernels


def _shape(t):
    return 'x'.join(str(n) for n in t.shape) if t.dim() else 'scalar'


class Recorder(object):
    """one ordered log of phases, collectives and op-set calls under a reported world size"""

    def __init__(self, monkeypatch, world):
        self.log, self.world = [], world
        log = self.log

        class phase(object):
            def __init__(self, name):
                self.name = name

            def __enter__(self):
                log.append('phase %s {' % self.name)
                return self

            def __exit__(self, *exc):
                log.append('}')
                return False

        def all_gather_cat(t):
            log.append('_all_gather_cat %s' % _shape(t))
            return torch.cat([t.contiguous()] * world)

        def all_reduce_sum_(t):
            log.append('all_reduce_sum_ %s' % _shape(t))
            return t

        def reduce_scatter_rows(t, rows):
            log.append('reduce_scatter_rows %s %d' % (_shape(t), rows))
            return t[:rows].contiguous()

        def dist_all_reduce(t, op=dist.ReduceOp.SUM):
            log.append('dist.all_reduce %s %s' % ('MAX' if op == dist.ReduceOp.MAX else 'SUM', _shape(t)))

        monkeypatch.setattr(parallel, 'world', lambda: world)
        monkeypatch.setattr(parallel, 'rank', lambda: 0)
        monkeypatch.setattr(parallel, 'phase', phase)
        monkeypatch.setattr(parallel, '_all_gather_cat', all_gather_cat)
        monkeypatch.setattr(parallel, 'all_reduce_sum_', all_reduce_sum_)
        monkeypatch.setattr(parallel, 'reduce_scatter_rows', reduce_scatter_rows)
        monkeypatch.setattr(dist, 'all_reduce', dist_all_reduce)

    def ops(self, inner):
        """`inner` with every call logged as 'op <shape of every tensor operand> <prior keyword>[entries]'"""
        log = self.log

        class Ops(object):
            def __getattr__(self, name):
                fn = getattr(inner, name)          # AttributeError for an op the inner set lacks, as hasattr() expects
                if not callable(fn):
                    return fn

                def call(*a, **kw):
                    prior = ['%s[%d]' % (key, kw[key].shape[0]) for key in ('shift_mask', 'known_shift') if key in kw]
                    log.append(' '.join(['op', name] + [_shape(t) for t in a if isinstance(t, torch.Tensor)] + prior))
                    return fn(*a, **kw)
                return call
        return Ops()


# ----------------------------------------------------------------------------- losses
LOSS_B = 3


def _loss_inputs(fov):
    g = torch.Generator().manual_seed(7)
    if fov:
        ov = torch.randn((LOSS_B, 2, 2, 64), generator=g)
        su = torch.stack([torch.roll(ov[i], -5 * i, dims=2)[:, :, :8] for i in range(LOSS_B)]) + 0.3 * torch.randn((LOSS_B, 2, 2, 8), generator=g)
    else:
        ov = torch.randn((LOSS_B, 8), generator=g)
        su = ov + 0.3 * torch.randn((LOSS_B, 8), generator=g)
    return ov.requires_grad_(True), su.requires_grad_(True)


def _loss_case(rec, name):
    if name == 'fov_soft_margin':
        ov, su = _loss_inputs(True)
        loss = cvig_fov.sharded_match_loss(ov, su, _kernels=rec.ops(CpuKernels))[0]
    elif name == 'fov_batch_hard':
        ov, su = _loss_inputs(True)
        loss = cvig_fov.sharded_match_loss(ov, su, loss='batch_hard', _kernels=rec.ops(BatchHardCpuKernels))[0]
    elif name == 'baseline_exhaustive':
        ov, su = _loss_inputs(False)
        loss = cvig_baseline.sharded_exhaustive_loss(su, ov, soft_margin=True, _kernels=rec.ops(baseline_slab_ref.CpuKernels))
    elif name == 'baseline_batch_hard':
        ov, su = _loss_inputs(False)
        loss = cvig_baseline.sharded_batch_hard_loss(su, ov, soft_margin=True, _kernels=rec.ops(baseline_hard_ref.CpuKernels))
    else:
        assert name == 'baseline_batch_hard_one_rank'
        ov, su = _loss_inputs(False)
        loss = cvig_baseline.batch_hard_triplet_loss(su, ov, soft_margin=True)
    rec.log.append('-- backward')
    loss.backward()
    assert tuple(ov.grad.shape) == tuple(ov.shape) and tuple(su.grad.shape) == tuple(su.shape)


LOSS_CASES = [(name, world) for name in ('fov_soft_margin', 'fov_batch_hard', 'baseline_exhaustive', 'baseline_batch_hard')
              for world in (1, 2)] + [('baseline_batch_hard_one_rank', 2)]      # inside a group of two it takes no part in it


def _run_loss(monkeypatch, name, world):
    rec = Recorder(monkeypatch, world)
    monkeypatch.setattr(cvig_baseline, '_hard_kernels', lambda: rec.ops(baseline_hard_ref.CpuKernels))
    _loss_case(rec, name)
    return rec.log


# ----------------------------------------------------------------------------- retrieval
N_G, N_Q, G0, CHUNK = 7, 5, 1, 2
K_ROOMY = 3
K_TIGHT = {'fov': 32 - cvig_fov.DFT_MARGIN + 1, 'baseline': ops.TOPK_MAX - cvig_baseline.GEMM_MARGIN + 1}


def _fov_problem():
    """gallery rows 1..7 (local 0..6), query q looks like global row q: query 0's true row is not in the shard; local rows 2 / 5
    are equal, so query 3 has a tie among its first places"""
    g = torch.Generator().manual_seed(13)
    gal = torch.randn((N_G, 2, 2, 64), generator=g)
    gal[5] = gal[2]
    src = [6, 0, 1, 2, 3]
    qry = torch.stack([torch.roll(gal[src[q]], -7 * q, dims=2) for q in range(N_Q)]) + 0.3 * torch.randn((N_Q, 2, 2, 64), generator=g)
    mask = R.window_words([(7 * q - 2) % 64 for q in range(N_Q)], [5, 3, 6, 4, 7])
    mask[2] = 0
    return gal.contiguous(), qry.contiguous(), mask


def _baseline_problem():
    g = torch.Generator().manual_seed(17)
    gal = torch.randn((N_G, 8), generator=g)
    gal[5] = gal[2]
    qry = gal[[6, 0, 1, 2, 3]] + 0.3 * torch.randn((N_Q, 8), generator=g)
    return gal.contiguous(), qry.contiguous()


RETRIEVE_KINDS = {
    'dft_resolved': ('fov', 'dft', MaskedSpectralCpuResolved, False),
    'dft_two_step': ('fov', 'dft', MaskedSpectralCpu, False),
    'dft_masked_resolved': ('fov', 'dft_masked', MaskedSpectralCpuResolved, True),
    'gemm': ('baseline', 'gemm', None, False),
}
RETRIEVE_CASES = [(kind, k, world) for kind in RETRIEVE_KINDS for k in ('roomy', 'tight') for world in (1, 2)
                  if (kind, k) != ('dft_two_step', 'tight')]      # the tight k changes the lists only, not the band


def _run_retrieve(monkeypatch, kind, k, world):
    model, method, inner, masked = RETRIEVE_KINDS[kind]
    rec = Recorder(monkeypatch, world)
    k = K_ROOMY if k == 'roomy' else K_TIGHT[model]
    if model == 'fov':
        gal, qry, mask = _fov_problem()
        out = cvig_fov.retrieve(gal, qry, k=k, shard_begin=G0, query_chunk=CHUNK, method=method, _kernels=rec.ops(inner),
                                **({'shift_mask': mask} if masked else {}))
        stats = cvig_fov.last_retrieve_stats()
    else:
        gal, qry = _baseline_problem()
        out = cvig_baseline.retrieve(gal, qry, k=k, shard_begin=G0, query_chunk=CHUNK, method=method, _kernels=rec.ops(gemm_kernels()))
        stats = cvig_baseline.last_retrieve_stats()
    assert out[0].shape == (N_Q,) and tuple(out[1].shape) == (N_Q, k) and tuple(out[2].shape) == (N_Q, k)
    rec.log.append('-- stats ' + ' '.join('%s=%s' % (key, stats[key]) for key in sorted(stats) if key != 'eps'))
    return rec.log


# ----------------------------------------------------------------------------- the recorded sequences
_FOV_STATS = '-- stats fallback_queries=0 masked=%s method=%s pairs=35.0 rescored_orientation=0 rescored_rank=5 rescored_topk=%d rescored_true=4'
_GEMM_STATS = '-- stats fallback_queries=0 method=gemm pairs=35.0 rescored_rank=5 rescored_topk=%d rescored_true=4'

SEQUENCES = {
    ('baseline_batch_hard', 1): [
        'phase slab_distances {',
        'op pairwise_sqdist 3x8 3x8',
        '}',
        'phase row_minima_all_gather {',
        'op batch_hard_slab_mine 3x3',
        '}',
        'phase loss_partial_all_reduce {',
        'op hard_slab_loss 3x3 3 3',
        '}',
        '-- backward',
        'phase slab_backward {',
        'op hard_pairs 3 3 3 3 3 scalar',
        'op sqdist_pairs_bwd 3x8 3x8 9 9 9',
        '}'],
    ('baseline_batch_hard', 2): [
        'phase batch_share_all_gather {',
        '_all_gather_cat 1',
        '}',
        'phase overhead_all_gather {',
        '_all_gather_cat 3x8',
        '}',
        'phase slab_distances {',
        'op pairwise_sqdist 6x8 3x8',
        '}',
        'phase diagonal_all_gather {',
        '_all_gather_cat 3',
        '}',
        'phase row_minima_all_gather {',
        'op batch_hard_slab_mine 6x3',
        '_all_gather_cat 1x6',
        '_all_gather_cat 1x6',
        'op batch_hard_merge_rows 2x6 2x6',
        '}',
        'phase loss_partial_all_reduce {',
        'op hard_slab_loss 6x3 6 3',
        'all_reduce_sum_ 1',
        '}',
        '-- backward',
        'phase slab_backward {',
        'op hard_pairs 6 6 6 3 3 scalar',
        'op sqdist_pairs_bwd 6x8 3x8 12 12 12',
        '}',
        'phase overhead_grad_reduce_scatter {',
        'reduce_scatter_rows 6x8 3',
        '}'],
    ('baseline_batch_hard_one_rank', 2): [
        'phase slab_distances {',
        'op pairwise_sqdist 3x8 3x8',
        '}',
        'phase row_minima_all_gather {',
        'op batch_hard_slab_mine 3x3',
        '}',
        'phase loss_partial_all_reduce {',
        'op hard_slab_loss 3x3 3 3',
        '}',
        '-- backward',
        'phase slab_backward {',
        'op hard_pairs 3 3 3 3 3 scalar',
        'op sqdist_pairs_bwd 3x8 3x8 9 9 9',
        '}'],
    ('baseline_exhaustive', 1): [
        'phase slab_distances {',
        'op pairwise_sqdist 3x8 3x8',
        '}',
        'phase loss_partial_all_reduce {',
        'op exhaustive_loss_slab_fwd 3x3 3',
        'all_reduce_sum_ 1',
        '}',
        '-- backward',
        'phase row_sums_all_reduce {',
        'op exhaustive_loss_slab_sig 3x3 3',
        'all_reduce_sum_ 3',
        '}',
        'phase slab_backward {',
        'op exhaustive_loss_slab_bwd 3x3 3 3 3 scalar',
        'op sqdist_rect_bwd 3x8 3x8 3x3',
        '}',
        'phase overhead_grad_reduce_scatter {',
        'reduce_scatter_rows 3x8 3',
        '}'],
    ('baseline_exhaustive', 2): [
        'phase batch_share_all_gather {',
        '_all_gather_cat 1',
        '}',
        'phase overhead_all_gather {',
        '_all_gather_cat 3x8',
        '}',
        'phase slab_distances {',
        'op pairwise_sqdist 6x8 3x8',
        '}',
        'phase diagonal_all_gather {',
        '_all_gather_cat 3',
        '}',
        'phase loss_partial_all_reduce {',
        'op exhaustive_loss_slab_fwd 6x3 6',
        'all_reduce_sum_ 1',
        '}',
        '-- backward',
        'phase row_sums_all_reduce {',
        'op exhaustive_loss_slab_sig 6x3 6',
        'all_reduce_sum_ 6',
        '}',
        'phase slab_backward {',
        'op exhaustive_loss_slab_bwd 6x3 6 6 3 scalar',
        'op sqdist_rect_bwd 6x8 3x8 6x3',
        '}',
        'phase overhead_grad_reduce_scatter {',
        'reduce_scatter_rows 6x8 3',
        '}'],
    ('dft_masked_resolved', 'roomy', 1): [
        'op match_spectrum 7x2x2x64',
        'op match_fwd_dft 7x2x2x64 2x2x2x64 shift_mask[2]',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 1 1 shift_mask[2]',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2 shift_mask[2]',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 2x2x2x64 shift_mask[2]',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 2 2 shift_mask[2]',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2 shift_mask[2]',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 1x2x2x64 shift_mask[1]',
        'op match_pairs 7x2x2x64 1x2x2x64 448 1 1 1 shift_mask[1]',
        'all_reduce_sum_ 1',
        'op rank_count_resolved 7x1 1 7x2x2x64 1x2x2x64 448 1 shift_mask[1]',
        'op topk_smallest 7x1',
        'all_reduce_sum_ 5',
        'op match_pairs 7x2x2x64 5x2x2x64 448 5 21 21 shift_mask[5]',
        'all_reduce_sum_ 3x9',
        _FOV_STATS % (True, 'dft_masked', 21)],
    ('dft_masked_resolved', 'roomy', 2): [
        'op match_spectrum 7x2x2x64',
        'op match_fwd_dft 7x2x2x64 2x2x2x64 shift_mask[2]',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 1 1 shift_mask[2]',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2 shift_mask[2]',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 2x2x2x64 shift_mask[2]',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 2 2 shift_mask[2]',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2 shift_mask[2]',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 1x2x2x64 shift_mask[1]',
        'op match_pairs 7x2x2x64 1x2x2x64 448 1 1 1 shift_mask[1]',
        'all_reduce_sum_ 1',
        'op rank_count_resolved 7x1 1 7x2x2x64 1x2x2x64 448 1 shift_mask[1]',
        'op topk_smallest 7x1',
        'all_reduce_sum_ 5',
        '_all_gather_cat 1x5x9',
        '_all_gather_cat 1x5x9',
        '_all_gather_cat 1x5',
        'op match_pairs 7x2x2x64 5x2x2x64 448 5 45 45 shift_mask[5]',
        'all_reduce_sum_ 5x9',
        _FOV_STATS % (True, 'dft_masked', 45)],
    ('dft_masked_resolved', 'tight', 1): [
        'op match_spectrum 7x2x2x64',
        'op match_fwd_dft 7x2x2x64 2x2x2x64 shift_mask[2]',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 1 1 shift_mask[2]',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2 shift_mask[2]',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 2x2x2x64 shift_mask[2]',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 2 2 shift_mask[2]',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2 shift_mask[2]',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 1x2x2x64 shift_mask[1]',
        'op match_pairs 7x2x2x64 1x2x2x64 448 1 1 1 shift_mask[1]',
        'all_reduce_sum_ 1',
        'op rank_count_resolved 7x1 1 7x2x2x64 1x2x2x64 448 1 shift_mask[1]',
        'op topk_smallest 7x1',
        'all_reduce_sum_ 5',
        'op match_pairs 7x2x2x64 5x2x2x64 448 5 7 7 shift_mask[5]',
        'all_reduce_sum_ 1x7',
        'op match_fwd 7x2x2x64 2x2x2x64 shift_mask[2]',
        'op topk_smallest 7x2',
        'op match_fwd 7x2x2x64 2x2x2x64 shift_mask[2]',
        'op topk_smallest 7x2',
        'op match_fwd 7x2x2x64 1x2x2x64 shift_mask[1]',
        'op topk_smallest 7x1',
        _FOV_STATS % (True, 'dft_masked', 7)],
    ('dft_masked_resolved', 'tight', 2): [
        'op match_spectrum 7x2x2x64',
        'op match_fwd_dft 7x2x2x64 2x2x2x64 shift_mask[2]',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 1 1 shift_mask[2]',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2 shift_mask[2]',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 2x2x2x64 shift_mask[2]',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 2 2 shift_mask[2]',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2 shift_mask[2]',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 1x2x2x64 shift_mask[1]',
        'op match_pairs 7x2x2x64 1x2x2x64 448 1 1 1 shift_mask[1]',
        'all_reduce_sum_ 1',
        'op rank_count_resolved 7x1 1 7x2x2x64 1x2x2x64 448 1 shift_mask[1]',
        'op topk_smallest 7x1',
        'all_reduce_sum_ 5',
        '_all_gather_cat 1x5x7',
        '_all_gather_cat 1x5x7',
        '_all_gather_cat 1x5',
        'op match_pairs 7x2x2x64 5x2x2x64 448 5 35 35 shift_mask[5]',
        'all_reduce_sum_ 5x7',
        'op match_fwd 7x2x2x64 2x2x2x64 shift_mask[2]',
        'op topk_smallest 7x2',
        'op match_fwd 7x2x2x64 2x2x2x64 shift_mask[2]',
        'op topk_smallest 7x2',
        'op match_fwd 7x2x2x64 1x2x2x64 shift_mask[1]',
        'op topk_smallest 7x1',
        '_all_gather_cat 1x5x27',
        '_all_gather_cat 1x5x27',
        'op topk_smallest 54x5',
        _FOV_STATS % (True, 'dft_masked', 35)],
    ('dft_resolved', 'roomy', 1): [
        'op match_spectrum 7x2x2x64',
        'op match_fwd_dft 7x2x2x64 2x2x2x64',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 1 1',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 2x2x2x64',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 2 2',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 1x2x2x64',
        'op match_pairs 7x2x2x64 1x2x2x64 448 1 1 1',
        'all_reduce_sum_ 1',
        'op rank_count_resolved 7x1 1 7x2x2x64 1x2x2x64 448 1',
        'op topk_smallest 7x1',
        'all_reduce_sum_ 5',
        'op match_pairs 7x2x2x64 5x2x2x64 448 5 21 21',
        'all_reduce_sum_ 3x9',
        _FOV_STATS % (False, 'dft', 21)],
    ('dft_resolved', 'roomy', 2): [
        'op match_spectrum 7x2x2x64',
        'op match_fwd_dft 7x2x2x64 2x2x2x64',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 1 1',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 2x2x2x64',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 2 2',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 1x2x2x64',
        'op match_pairs 7x2x2x64 1x2x2x64 448 1 1 1',
        'all_reduce_sum_ 1',
        'op rank_count_resolved 7x1 1 7x2x2x64 1x2x2x64 448 1',
        'op topk_smallest 7x1',
        'all_reduce_sum_ 5',
        '_all_gather_cat 1x5x9',
        '_all_gather_cat 1x5x9',
        '_all_gather_cat 1x5',
        'op match_pairs 7x2x2x64 5x2x2x64 448 5 45 45',
        'all_reduce_sum_ 5x9',
        _FOV_STATS % (False, 'dft', 45)],
    ('dft_resolved', 'tight', 1): [
        'op match_spectrum 7x2x2x64',
        'op match_fwd_dft 7x2x2x64 2x2x2x64',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 1 1',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 2x2x2x64',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 2 2',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 1x2x2x64',
        'op match_pairs 7x2x2x64 1x2x2x64 448 1 1 1',
        'all_reduce_sum_ 1',
        'op rank_count_resolved 7x1 1 7x2x2x64 1x2x2x64 448 1',
        'op topk_smallest 7x1',
        'all_reduce_sum_ 5',
        'op match_pairs 7x2x2x64 5x2x2x64 448 5 7 7',
        'all_reduce_sum_ 1x7',
        'op match_fwd 7x2x2x64 2x2x2x64',
        'op topk_smallest 7x2',
        'op match_fwd 7x2x2x64 2x2x2x64',
        'op topk_smallest 7x2',
        'op match_fwd 7x2x2x64 1x2x2x64',
        'op topk_smallest 7x1',
        _FOV_STATS % (False, 'dft', 7)],
    ('dft_resolved', 'tight', 2): [
        'op match_spectrum 7x2x2x64',
        'op match_fwd_dft 7x2x2x64 2x2x2x64',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 1 1',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 2x2x2x64',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 2 2',
        'all_reduce_sum_ 2',
        'op rank_count_resolved 7x2 2 7x2x2x64 2x2x2x64 448 2',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 1x2x2x64',
        'op match_pairs 7x2x2x64 1x2x2x64 448 1 1 1',
        'all_reduce_sum_ 1',
        'op rank_count_resolved 7x1 1 7x2x2x64 1x2x2x64 448 1',
        'op topk_smallest 7x1',
        'all_reduce_sum_ 5',
        '_all_gather_cat 1x5x7',
        '_all_gather_cat 1x5x7',
        '_all_gather_cat 1x5',
        'op match_pairs 7x2x2x64 5x2x2x64 448 5 35 35',
        'all_reduce_sum_ 5x7',
        'op match_fwd 7x2x2x64 2x2x2x64',
        'op topk_smallest 7x2',
        'op match_fwd 7x2x2x64 2x2x2x64',
        'op topk_smallest 7x2',
        'op match_fwd 7x2x2x64 1x2x2x64',
        'op topk_smallest 7x1',
        '_all_gather_cat 1x5x27',
        '_all_gather_cat 1x5x27',
        'op topk_smallest 54x5',
        _FOV_STATS % (False, 'dft', 35)],
    ('dft_two_step', 'roomy', 1): [
        'op match_spectrum 7x2x2x64',
        'op match_fwd_dft 7x2x2x64 2x2x2x64',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 1 1',
        'all_reduce_sum_ 2',
        'op rank_count_band 7x2 2',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 1 1',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 2x2x2x64',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 2 2',
        'all_reduce_sum_ 2',
        'op rank_count_band 7x2 2',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 3 3',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 1x2x2x64',
        'op match_pairs 7x2x2x64 1x2x2x64 448 1 1 1',
        'all_reduce_sum_ 1',
        'op rank_count_band 7x1 1',
        'op match_pairs 7x2x2x64 1x2x2x64 448 1 1 1',
        'op topk_smallest 7x1',
        'all_reduce_sum_ 5',
        'op match_pairs 7x2x2x64 5x2x2x64 448 5 21 21',
        'all_reduce_sum_ 3x9',
        _FOV_STATS % (False, 'dft', 21)],
    ('dft_two_step', 'roomy', 2): [
        'op match_spectrum 7x2x2x64',
        'op match_fwd_dft 7x2x2x64 2x2x2x64',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 1 1',
        'all_reduce_sum_ 2',
        'op rank_count_band 7x2 2',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 1 1',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 2x2x2x64',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 2 2',
        'all_reduce_sum_ 2',
        'op rank_count_band 7x2 2',
        'op match_pairs 7x2x2x64 2x2x2x64 448 2 3 3',
        'op topk_smallest 7x2',
        'op match_fwd_dft 7x2x2x64 1x2x2x64',
        'op match_pairs 7x2x2x64 1x2x2x64 448 1 1 1',
        'all_reduce_sum_ 1',
        'op rank_count_band 7x1 1',
        'op match_pairs 7x2x2x64 1x2x2x64 448 1 1 1',
        'op topk_smallest 7x1',
        'all_reduce_sum_ 5',
        '_all_gather_cat 1x5x9',
        '_all_gather_cat 1x5x9',
        '_all_gather_cat 1x5',
        'op match_pairs 7x2x2x64 5x2x2x64 448 5 45 45',
        'all_reduce_sum_ 5x9',
        _FOV_STATS % (False, 'dft', 45)],
    ('fov_batch_hard', 1): [
        'phase slab_match {',
        'op match_fwd 3x2x2x64 3x2x2x8',
        '}',
        'op batch_hard_fwd 3x3',
        '-- backward',
        'phase slab_match_backward {',
        'op batch_hard_pairs 3 3 3 3 3 scalar',
        'op match_bwd_pairs 3x2x2x64 3x2x2x8 3x3 1 1 9 9 9',
        '}'],
    ('fov_batch_hard', 2): [
        'phase overhead_all_gather {',
        '_all_gather_cat 3x2x2x64',
        '}',
        'phase slab_match {',
        'op match_fwd 6x2x2x64 3x2x2x8',
        '}',
        'phase diagonal_all_gather {',
        '_all_gather_cat 3',
        '}',
        'phase row_minima_all_gather {',
        'op batch_hard_slab_mine 6x3',
        '_all_gather_cat 1x6',
        '_all_gather_cat 1x6',
        'op batch_hard_merge_rows 2x6 2x6',
        '}',
        'phase loss_partial_all_reduce {',
        'op batch_hard_slab_loss 6x3 6 3',
        'all_reduce_sum_ 1',
        '}',
        '-- backward',
        'phase slab_match_backward {',
        'op batch_hard_pairs 6 6 6 3 3 scalar',
        'op match_bwd_pairs 6x2x2x64 3x2x2x8 6x3 1 1 12 12 12',
        '}',
        'phase overhead_grad_reduce_scatter {',
        'reduce_scatter_rows 6x2x2x64 3',
        '}'],
    ('fov_soft_margin', 1): [
        'phase overhead_all_gather {',
        '_all_gather_cat 3x2x2x64',
        '}',
        'phase slab_match {',
        'op match_fwd 3x2x2x64 3x2x2x8',
        '}',
        'phase diagonal_all_gather {',
        '_all_gather_cat 3',
        '}',
        'phase loss_partial_all_reduce {',
        'op triplet_loss_slab_fwd 3x3 3',
        'all_reduce_sum_ 1',
        '}',
        '-- backward',
        'phase row_sigmoid_all_reduce {',
        'op triplet_loss_slab_sig 3x3 3',
        'all_reduce_sum_ 3',
        '}',
        'phase slab_match_backward {',
        'op triplet_loss_slab_bwd 3x3 3 3 3 scalar',
        'op match_bwd 3x2x2x64 3x2x2x8 3x3 1 1 3x3',
        '}',
        'phase overhead_grad_reduce_scatter {',
        'reduce_scatter_rows 3x2x2x64 3',
        '}'],
    ('fov_soft_margin', 2): [
        'phase overhead_all_gather {',
        '_all_gather_cat 3x2x2x64',
        '}',
        'phase slab_match {',
        'op match_fwd 6x2x2x64 3x2x2x8',
        '}',
        'phase diagonal_all_gather {',
        '_all_gather_cat 3',
        '}',
        'phase loss_partial_all_reduce {',
        'op triplet_loss_slab_fwd 6x3 6',
        'all_reduce_sum_ 1',
        '}',
        '-- backward',
        'phase row_sigmoid_all_reduce {',
        'op triplet_loss_slab_sig 6x3 6',
        'all_reduce_sum_ 6',
        '}',
        'phase slab_match_backward {',
        'op triplet_loss_slab_bwd 6x3 6 6 3 scalar',
        'op match_bwd 6x2x2x64 3x2x2x8 6x3 1 1 6x3',
        '}',
        'phase overhead_grad_reduce_scatter {',
        'reduce_scatter_rows 6x2x2x64 3',
        '}'],
    ('gemm', 'roomy', 1): [
        'op row_sqnorm 7x8',
        'op row_sqnorm 5x8',
        'op sqdist_gemm 7x8 2x8 7 2',
        'op sqdist_pairs 7x8 2x8 1 1',
        'all_reduce_sum_ 2',
        'op rank_count_band 7x2 2',
        'op sqdist_pairs 7x8 2x8 1 1',
        'op topk_smallest 7x2',
        'op sqdist_gemm 7x8 2x8 7 2',
        'op sqdist_pairs 7x8 2x8 2 2',
        'all_reduce_sum_ 2',
        'op rank_count_band 7x2 2',
        'op sqdist_pairs 7x8 2x8 3 3',
        'op topk_smallest 7x2',
        'op sqdist_gemm 7x8 1x8 7 1',
        'op sqdist_pairs 7x8 1x8 1 1',
        'all_reduce_sum_ 1',
        'op rank_count_band 7x1 1',
        'op sqdist_pairs 7x8 1x8 1 1',
        'op topk_smallest 7x1',
        'all_reduce_sum_ 5',
        'op sqdist_pairs 7x8 5x8 35 35',
        'all_reduce_sum_ 5x35',
        _GEMM_STATS % 35],
    ('gemm', 'roomy', 2): [
        'op row_sqnorm 7x8',
        'op row_sqnorm 5x8',
        'dist.all_reduce MAX 2',
        'op sqdist_gemm 7x8 2x8 7 2',
        'op sqdist_pairs 7x8 2x8 1 1',
        'all_reduce_sum_ 2',
        'op rank_count_band 7x2 2',
        'op sqdist_pairs 7x8 2x8 1 1',
        'op topk_smallest 7x2',
        'op sqdist_gemm 7x8 2x8 7 2',
        'op sqdist_pairs 7x8 2x8 2 2',
        'all_reduce_sum_ 2',
        'op rank_count_band 7x2 2',
        'op sqdist_pairs 7x8 2x8 3 3',
        'op topk_smallest 7x2',
        'op sqdist_gemm 7x8 1x8 7 1',
        'op sqdist_pairs 7x8 1x8 1 1',
        'all_reduce_sum_ 1',
        'op rank_count_band 7x1 1',
        'op sqdist_pairs 7x8 1x8 1 1',
        'op topk_smallest 7x1',
        'all_reduce_sum_ 5',
        '_all_gather_cat 1x5x35',
        '_all_gather_cat 1x5',
        'op sqdist_pairs 7x8 5x8 70 70',
        'all_reduce_sum_ 5x70',
        _GEMM_STATS % 70],
    ('gemm', 'tight', 1): [
        'op row_sqnorm 7x8',
        'op row_sqnorm 5x8',
        'op sqdist_gemm 7x8 2x8 7 2',
        'op sqdist_pairs 7x8 2x8 1 1',
        'all_reduce_sum_ 2',
        'op rank_count_band 7x2 2',
        'op sqdist_pairs 7x8 2x8 1 1',
        'op sqdist_gemm 7x8 2x8 7 2',
        'op sqdist_pairs 7x8 2x8 2 2',
        'all_reduce_sum_ 2',
        'op rank_count_band 7x2 2',
        'op sqdist_pairs 7x8 2x8 3 3',
        'op sqdist_gemm 7x8 1x8 7 1',
        'op sqdist_pairs 7x8 1x8 1 1',
        'all_reduce_sum_ 1',
        'op rank_count_band 7x1 1',
        'op sqdist_pairs 7x8 1x8 1 1',
        'all_reduce_sum_ 5',
        'op pairwise_sqdist 7x8 2x8',
        'op topk_smallest 7x2',
        'op pairwise_sqdist 7x8 2x8',
        'op topk_smallest 7x2',
        'op pairwise_sqdist 7x8 1x8',
        'op topk_smallest 7x1',
        _GEMM_STATS % 0],
    ('gemm', 'tight', 2): [
        'op row_sqnorm 7x8',
        'op row_sqnorm 5x8',
        'dist.all_reduce MAX 2',
        'op sqdist_gemm 7x8 2x8 7 2',
        'op sqdist_pairs 7x8 2x8 1 1',
        'all_reduce_sum_ 2',
        'op rank_count_band 7x2 2',
        'op sqdist_pairs 7x8 2x8 1 1',
        'op sqdist_gemm 7x8 2x8 7 2',
        'op sqdist_pairs 7x8 2x8 2 2',
        'all_reduce_sum_ 2',
        'op rank_count_band 7x2 2',
        'op sqdist_pairs 7x8 2x8 3 3',
        'op sqdist_gemm 7x8 1x8 7 1',
        'op sqdist_pairs 7x8 1x8 1 1',
        'all_reduce_sum_ 1',
        'op rank_count_band 7x1 1',
        'op sqdist_pairs 7x8 1x8 1 1',
        'all_reduce_sum_ 5',
        'op pairwise_sqdist 7x8 2x8',
        'op topk_smallest 7x2',
        'op pairwise_sqdist 7x8 2x8',
        'op topk_smallest 7x2',
        'op pairwise_sqdist 7x8 1x8',
        'op topk_smallest 7x1',
        '_all_gather_cat 1x5x993',
        '_all_gather_cat 1x5x993',
        'op topk_smallest 1986x5',
        _GEMM_STATS % 0],
}


@pytest.mark.parametrize('name,world', LOSS_CASES)
def test_loss_sequence(monkeypatch, name, world):
    assert _run_loss(monkeypatch, name, world) == SEQUENCES[name, world]


@pytest.mark.parametrize('kind,k,world', RETRIEVE_CASES)
def test_retrieve_sequence(monkeypatch, kind, k, world):
    assert _run_retrieve(monkeypatch, kind, k, world) == SEQUENCES[kind, k, world]


if __name__ == '__main__':
    recorded = {}
    for case in LOSS_CASES + RETRIEVE_CASES:
        with pytest.MonkeyPatch.context() as mp:
            recorded[case] = (_run_loss if len(case) == 2 else _run_retrieve)(mp, *case)
    print('SEQUENCES = {')
    for case in sorted(recorded, key=repr):
        print('    %r: [\n        %s],' % (case, ',\n        '.join(pprint.pformat(line, width=140) for line in recorded[case])))
    print('}')
