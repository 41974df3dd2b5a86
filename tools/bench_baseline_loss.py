#!/usr/bin/env python
"""cvig_baseline loss timing: the dense exhaustive loss against its column-slab form (csrc/baseline_loss_slab.hip).

One step = forward + backward of the loss alone on prepared [B, 1536] embeddings, timed with device events after warm-up; the
forms of a case alternate step by step in one process so that they see the same machine state. Cases:
  full B      B in {16, 32, 128}: exhaustive_minibatch_triplet_loss (dense kernels)  vs  sharded_exhaustive_loss as a world of one
              (the slab path at b = B, col0 = 0). Launches per step are counted from the op calls and their launch lists.
  slab B b    one rank's slab work at (1024, 128) and (128, 16), rank 1's columns, kernels only: the all-gathered inputs are
              prepared beforehand and the collectives (B x 1536 embeddings, 2 x B floats, one float; a [B, 1536] reduce-scatter)
              are left out. Timed as a whole and call by call; for the rectangular backward the tool also prints the time the
              naive form's traffic would take, B b n reads of 4 bytes per side at L2_TBS.
Writes profiles/baseline_sharded_loss.json (--out) and prints one JSON line per case."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from witw_amd import baseline_parallel as bp  # noqa: E402
from witw_amd import cvig_baseline, ops, synth  # noqa: E402

N = 1536
L2_TBS = 17.0        # TB/s chip-wide for rows every workgroup shares, served by the XCDs' L2 (measured gather rate, 16.8-18.8)
# kernel launches of one step, from the entries' launch lists (torch's own small kernels -- clone, diagonal copy, divide -- aside)
LAUNCHES = {'dense': {'pairwise_sqdist': 1, 'exhaustive_triplet_loss': 2, 'exhaustive_triplet_loss_bwd': 3},
            'slab': {'pairwise_sqdist': 1, 'exhaustive_loss_slab_fwd': 2, 'exhaustive_loss_slab_sig': 1, 'exhaustive_loss_slab_bwd': 1,
                     'sqdist_rect_bwd': 2}}


def _emb(B, seed):
    """clustered like training embeddings late in a run: true pairs close, so that both hinge branches are taken"""
    a = torch.from_numpy(synth.embeddings(seed, 1, (B, N))) * 0.02
    b = a + torch.from_numpy(synth.embeddings(seed, 2, (B, N))) * 0.02
    return a.cuda(), b.cuda()


def _timed(fns, steps, warmup):
    """{name: fn} alternating -> {name: (median ms, min ms)}"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(steps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t[name].append(e0.elapsed_time(e1))
    return {k: (round(sorted(v)[len(v) // 2], 4), round(min(v), 4)) for k, v in t.items()}


def full_case(B, steps, warmup, soft):
    a, b = _emb(B, 700 + B)

    def dense():
        s, o = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        cvig_baseline.exhaustive_minibatch_triplet_loss(s, o, soft_margin=soft).backward()

    def slab():
        s, o = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        cvig_baseline.sharded_exhaustive_loss(s, o, soft_margin=soft).backward()
    r = _timed({'dense': dense, 'slab_world1': slab}, steps, warmup)
    return {'case': 'full', 'B': B, 'soft_margin': soft, 'dense_ms_median': r['dense'][0], 'dense_ms_min': r['dense'][1],
            'slab_world1_ms_median': r['slab_world1'][0], 'slab_world1_ms_min': r['slab_world1'][1],
            'launches_dense': sum(LAUNCHES['dense'].values()), 'launches_slab': sum(LAUNCHES['slab'].values())}


def slab_case(B, b, steps, warmup, soft):
    x, y_all = _emb(B, 800 + B)
    col0 = b                                              # rank 1
    y = y_all[col0:col0 + b].contiguous()
    kw = dict(soft_margin=soft)
    diag = torch.diagonal(ops.pairwise_sqdist(x, y_all)).contiguous()
    g = torch.ones((1,), device='cuda')
    T = ops.pairwise_sqdist(x, y)
    rowsig, colsig = bp.exhaustive_loss_slab_sig(T, diag, col0, **kw)
    G = bp.exhaustive_loss_slab_bwd(T, diag, rowsig, colsig, g, col0, **kw)

    def whole():
        t = ops.pairwise_sqdist(x, y)
        bp.exhaustive_loss_slab_fwd(t, diag, col0, **kw)
        rs, cs = bp.exhaustive_loss_slab_sig(t, diag, col0, **kw)
        gg = bp.exhaustive_loss_slab_bwd(t, diag, rs, cs, g, col0, **kw)
        bp.sqdist_rect_bwd(x, y, gg)
    parts = {'whole': whole,
             'pairwise_sqdist': lambda: ops.pairwise_sqdist(x, y),
             'slab_fwd': lambda: bp.exhaustive_loss_slab_fwd(T, diag, col0, **kw),
             'slab_sig': lambda: bp.exhaustive_loss_slab_sig(T, diag, col0, **kw),
             'slab_bwd': lambda: bp.exhaustive_loss_slab_bwd(T, diag, rowsig, colsig, g, col0, **kw),
             'rect_bwd_dx': lambda: bp.sqdist_rect_bwd(x, y, G, need_dy=False),
             'rect_bwd_dy': lambda: bp.sqdist_rect_bwd(x, y, G, need_dx=False)}
    r = _timed(parts, steps, warmup)
    out = {'case': 'slab', 'B': B, 'b': b, 'soft_margin': soft, 'launches': sum(LAUNCHES['slab'].values())}
    for k, (med, mn) in r.items():
        out[k + '_ms_median'], out[k + '_ms_min'] = med, mn
    out['rect_bwd_naive_traffic_bytes_per_side'] = 4 * B * b * N
    out['rect_bwd_naive_traffic_ms_per_side_at_l2_rate'] = round(4e-9 * B * b * N / L2_TBS, 4)
    bp.sqdist_rect_bwd(x, y, G)
    out['rect_bwd_variant'] = ops.last_kernel_variant()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'baseline_sharded_loss.json'))
    args = ap.parse_args(argv)
    torch.zeros(1, device='cuda')
    res = []
    for soft in (False, True):
        for B in (16, 32, 128):
            res.append(full_case(B, args.steps, args.warmup, soft))
            print(json.dumps(res[-1]), flush=True)
        for B, b in ((1024, 128), (128, 16)):
            res.append(slab_case(B, b, args.steps, args.warmup, soft))
            print(json.dumps(res[-1]), flush=True)
    with open(args.out, 'w') as f:
        json.dump({'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup, 'n': N, 'l2_tbs_assumed': L2_TBS,
                   'launches_per_step': LAUNCHES, 'cases': res}, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
