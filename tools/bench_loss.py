#!/usr/bin/env python
"""Loss-step timing: soft-margin (dense dL/dD + dense match backward) against batch-hard (mining + pair-list match backward).

One step = match forward + loss forward + loss backward + match backward, timed with device events after warm-up; the two
losses alternate step by step in one process so that both see the same machine state. Cases:
  full360  B = 128, fov 360 (We = 64): match + triplet_loss  vs  sharded_match_loss(loss='batch_hard') on one rank
  full70   B = 128, fov 70  (We = 12): the same
  slab     the [1024,128] column slab of one rank of config 3 (B = 1024 over 8 ranks), kernels only (the collectives are left
           out: all-gathers of the diagonal / row minima and the loss all-reduce are the same few KB for both losses)
Prints one JSON line per case: median / min step time in ms of each loss.
Kernel times: run under `rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_loss.py`."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from witw_amd import cvig_fov, ops, synth  # noqa: E402


def _emb(B, we, seed):
    ov = torch.from_numpy(synth.embeddings(seed, 1, (B, 16, 4, 64)))
    su = torch.from_numpy(synth.embeddings(seed, 2, (B, 16, 4, we)))
    return ov.cuda(), su.cuda()


def full_steps(B, we):
    ov, su = _emb(B, we, 900 + we)

    def soft():
        o, s = ov.clone().requires_grad_(True), su.clone().requires_grad_(True)
        _, d = cvig_fov.match(o, s)
        cvig_fov.triplet_loss(d).backward()

    def hard():
        o, s = ov.clone().requires_grad_(True), su.clone().requires_grad_(True)
        loss, _, _ = cvig_fov.sharded_match_loss(o, s, loss='batch_hard')
        loss.backward()
    return soft, hard


def slab_steps(B, b, world):
    ov, su = _emb(B, 64, 901)
    su = su[:b].contiguous()
    col0 = b        # rank 1
    g = torch.ones((1,), device='cuda')

    def soft():
        ori, d, score, ws = ops.match_fwd(ov, su, want_score=True, want_workspace=True)
        diag = torch.diagonal(d[col0:col0 + b]).contiguous().repeat(world)
        ops.triplet_loss_slab_fwd(d, diag, col0)
        rowsig, colsig = ops.triplet_loss_slab_sig(d, diag, col0)
        gd = ops.triplet_loss_slab_bwd(d, diag, rowsig, colsig, g, col0)
        ops.match_bwd(ov, su, ori, score, ws, gd)

    def hard():
        ori, d, score, ws = ops.match_fwd(ov, su, want_score=True, want_workspace=True)
        diag = torch.diagonal(d[col0:col0 + b]).contiguous().repeat(world)
        rv_l, ri_l, cv, ci = ops.batch_hard_slab_mine(d, col0)
        rv, ri = ops.batch_hard_merge_rows(rv_l[None].expand(world, -1).contiguous(), ri_l[None].expand(world, -1).contiguous())
        ops.batch_hard_slab_loss(d, rv, cv, col0)
        po, ps, pw = ops.batch_hard_pairs(diag, rv, ri, cv, ci, g, col0)
        ops.match_bwd_pairs(ov, su, ori, score, ws, po, ps, pw)
    return soft, hard


def time_pair(soft, hard, steps, warmup):
    for _ in range(warmup):
        soft()
        hard()
    torch.cuda.synchronize()
    t = {'soft_margin': [], 'batch_hard': []}
    for _ in range(steps):
        for name, fn in (('soft_margin', soft), ('batch_hard', hard)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t[name].append(e0.elapsed_time(e1))
    out = {}
    for name, v in t.items():
        v = sorted(v)
        out[name + '_ms_median'] = round(v[len(v) // 2], 4)
        out[name + '_ms_min'] = round(v[0], 4)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--cases', default='full360,full70,slab')
    args = ap.parse_args(argv)
    torch.zeros(1, device='cuda')
    cases = {'full360': lambda: full_steps(128, 64), 'full70': lambda: full_steps(128, 12),
             'slab': lambda: slab_steps(1024, 128, 8)}
    for name in args.cases.split(','):
        soft, hard = cases[name]()
        r = time_pair(soft, hard, args.steps, args.warmup)
        r['case'] = name
        r['steps'] = args.steps
        print(json.dumps(r), flush=True)


if __name__ == '__main__':
    main()
