#!/usr/bin/env python
"""cvig_baseline loss timing: the batch-hard loss step (csrc/baseline_loss_hard.hip + the mining of csrc/loss_hard.hip) at the shapes
tools/bench_baseline_loss.py times the exhaustive step at.

One step = distances -> loss -> embedding gradients on prepared [B, 1536] embeddings, timed with device events after warm-up; the
forms of a case alternate step by step in one process so that they see the same machine state. Cases, each for the hard and the
soft margin and for a hub input (every row of this rank's side equal: one column is the hardest negative of all B rows, so one
row of dy collects B pairs):
  slab B b    one rank's slab work at (1024, 128) rank 1's columns and (16, 16) the whole batch, kernels only: the all-gathered
              inputs are prepared beforehand and the collectives are left out, as in bench_baseline_loss.py's slab case. Timed as
              a whole and call by call, next to the exhaustive slab step on the same inputs in the same process.
  full B      B = 16: batch_hard_triplet_loss forward + backward through autograd, next to sharded_exhaustive_loss as a world of one.
--parent-json: the JSON tools/bench_baseline_loss.py of the parent commit wrote in the same session; its numbers at these shapes are
copied under `parent_exhaustive`. Writes profiles/baseline_hard_loss.json (--out) and prints one JSON line per case."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_baseline_loss import N, _emb, _timed  # noqa: E402
from witw_amd import baseline_hard as bh  # noqa: E402
from witw_amd import baseline_parallel as bp  # noqa: E402
from witw_amd import cvig_baseline, ops  # noqa: E402

SHAPES = ((1024, 128, 128), (16, 16, 0))          # (B, b, col0)
# kernel launches of one step, from the entries' launch lists
LAUNCHES = {'pairwise_sqdist': 1, 'batch_hard_slab_mine': 3, 'batch_hard_merge_rows': 1, 'hard_slab_loss': 1, 'hard_pairs': 1,
            'sqdist_pairs_bwd': 1}


def slab_case(B, b, col0, steps, warmup, soft, hub):
    x, y_all = _emb(B, 800 + B)
    if hub:
        y_all = y_all[col0:col0 + 1].expand(B, N).contiguous()
    y = y_all[col0:col0 + b].contiguous()
    kw = dict(soft_margin=soft)
    diag = torch.diagonal(ops.pairwise_sqdist(x, y_all)).contiguous()
    g = torch.ones((1,), device='cuda')
    T = ops.pairwise_sqdist(x, y)
    rv1, ri1, cv, ci = ops.batch_hard_slab_mine(T, col0)
    rv, ri = ops.batch_hard_merge_rows(rv1[None], ri1[None])
    pg, pc, pw = bh.hard_pairs(diag, rv, ri, cv, ci, g, col0, **kw)
    longest = int(torch.bincount(pc[pc >= 0].long(), minlength=b).max())

    def whole():
        t = ops.pairwise_sqdist(x, y)
        v, i, c, k = ops.batch_hard_slab_mine(t, col0)
        v, i = ops.batch_hard_merge_rows(v[None], i[None])
        bh.hard_slab_loss(t, v, c, col0, **kw)
        bh.sqdist_pairs_bwd(x, y, *bh.hard_pairs(diag, v, i, c, k, g, col0, **kw))

    def exhaustive():
        t = ops.pairwise_sqdist(x, y)
        bp.exhaustive_loss_slab_fwd(t, diag, col0, **kw)
        rs, cs = bp.exhaustive_loss_slab_sig(t, diag, col0, **kw)
        bp.sqdist_rect_bwd(x, y, bp.exhaustive_loss_slab_bwd(t, diag, rs, cs, g, col0, **kw))
    parts = {'whole': whole, 'exhaustive_whole': exhaustive,
             'pairwise_sqdist': lambda: ops.pairwise_sqdist(x, y),
             'slab_mine': lambda: ops.batch_hard_slab_mine(T, col0),
             'merge_rows': lambda: ops.batch_hard_merge_rows(rv1[None], ri1[None]),
             'hard_slab_loss': lambda: bh.hard_slab_loss(T, rv, cv, col0, **kw),
             'hard_pairs': lambda: bh.hard_pairs(diag, rv, ri, cv, ci, g, col0, **kw),
             'pairs_bwd': lambda: bh.sqdist_pairs_bwd(x, y, pg, pc, pw),
             'pairs_bwd_dx': lambda: bh.sqdist_pairs_bwd(x, y, pg, pc, pw, need_dy=False),
             'pairs_bwd_dy': lambda: bh.sqdist_pairs_bwd(x, y, pg, pc, pw, need_dx=False)}
    r = _timed(parts, steps, warmup)
    out = {'case': 'slab', 'B': B, 'b': b, 'col0': col0, 'soft_margin': soft, 'hub': hub, 'pairs': int(pg.numel()),
           'longest_dy_segment': longest, 'launches': sum(LAUNCHES.values())}
    for k, (med, mn) in r.items():
        out[k + '_ms_median'], out[k + '_ms_min'] = med, mn
    return out


def full_case(B, steps, warmup, soft):
    a, b = _emb(B, 700 + B)

    def hard():
        s, o = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        cvig_baseline.batch_hard_triplet_loss(s, o, soft_margin=soft).backward()

    def exhaustive():
        s, o = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        cvig_baseline.sharded_exhaustive_loss(s, o, soft_margin=soft).backward()
    r = _timed({'batch_hard': hard, 'exhaustive_slab_world1': exhaustive}, steps, warmup)
    out = {'case': 'full', 'B': B, 'soft_margin': soft}
    for k, (med, mn) in r.items():
        out[k + '_ms_median'], out[k + '_ms_min'] = med, mn
    return out


def parent_numbers(path):
    """the parent tool's cases at this tool's shapes: its slab case (1024, 128) and its full case B = 16 (the slab path at b = B)"""
    with open(path) as f:
        doc = json.load(f)
    keep = [c for c in doc['cases'] if (c['case'] == 'slab' and (c['B'], c['b']) == (1024, 128)) or (c['case'] == 'full' and c['B'] == 16)]
    return {'tool': 'tools/bench_baseline_loss.py of the parent commit, same session and device', 'device': doc['device'],
            'steps': doc['steps'], 'warmup': doc['warmup'], 'cases': keep}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--parent-json', default=None)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'baseline_hard_loss.json'))
    args = ap.parse_args(argv)
    torch.zeros(1, device='cuda')
    res = []
    for soft in (False, True):
        for B, b, col0 in SHAPES:
            for hub in (False, True):
                res.append(slab_case(B, b, col0, args.steps, args.warmup, soft, hub))
                print(json.dumps(res[-1]), flush=True)
        res.append(full_case(16, args.steps, args.warmup, soft))
        print(json.dumps(res[-1]), flush=True)
    doc = {'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup, 'n': N, 'launches_per_step': LAUNCHES,
           'cases': res}
    if args.parent_json:
        doc['parent_exhaustive'] = parent_numbers(args.parent_json)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
