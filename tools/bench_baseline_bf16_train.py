#!/usr/bin/env python
"""Training step of cvig_baseline (BASELINE config 1: 32 pairs, surface 500 x 500, overhead 512 x 512, uint8-valued inputs) under
train_precision='fp32' and train_precision='bf16':

  * one full step -- both encoders forward and backward in train mode, the exhaustive minibatch triplet loss, Adam -- between two
    device events, fp32 and bf16 alternating round-robin in one process (drift of the box falls on both alike), median of --rounds
    with minimum and maximum;
  * per bf16 launch of the bf16 step (blocks 2-4 of both encoders: forward, data gradient, weight gradient = nine launches per
    encoder): time per launch between device events (ops.PROFILE), algorithmic FLOP (4 taps) / time as TF/s and as a share of the
    2,500 TF/s bf16 matrix peak.

The condition for the bf16 path to exist: its median lies below the fp32 median by more than the larger of the two min-max ranges
(`faster_beyond_noise`). Run it under `timeout`. --json PATH keeps the table (profiles/baseline_bf16_train.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from witw_amd import cvig_baseline as cb  # noqa: E402
from witw_amd import ops, synth  # noqa: E402

PEAK_TFLOPS = 2500.0
PRECISIONS = ('fp32', 'bf16')


def _event_ms(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _row(v):
    return {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v), 'all_ms': v}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--pairs', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--json', default=None, metavar='PATH')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    su = torch.from_numpy(synth.images_u8(90, 0, (args.pairs, 3, 500, 500))).to(dev)
    ov = torch.from_numpy(synth.images_u8(90, 1, (args.pairs, 3, 512, 512))).to(dev)
    enc, opt = {}, {}
    for prec in PRECISIONS:
        torch.manual_seed(1)      # the same initial weights under both
        enc[prec] = (cb.SurfaceEncoder(train_precision=prec).to(dev).train(), cb.OverheadEncoder(train_precision=prec).to(dev).train())
        opt[prec] = cb.Adam(list(enc[prec][0].parameters()) + list(enc[prec][1].parameters()))

    def step(prec):
        s, o = enc[prec]
        loss = cb.exhaustive_minibatch_triplet_loss(s(su), o(ov))
        opt[prec].zero_grad()
        loss.backward()
        opt[prec].step()

    for _ in range(args.warmup):
        for prec in PRECISIONS:
            step(prec)
    torch.cuda.synchronize()
    times = {prec: [] for prec in PRECISIONS}
    for _ in range(args.rounds):
        for prec in PRECISIONS:
            times[prec].append(_event_ms(lambda: step(prec)))
    out = {'pairs': args.pairs, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0), 'step_ms': {p: _row(v) for p, v in times.items()}}
    f32, b16 = out['step_ms']['fp32'], out['step_ms']['bf16']
    noise = max(f32['max_ms'] - f32['min_ms'], b16['max_ms'] - b16['min_ms'])
    out['speedup'] = f32['median_ms'] / b16['median_ms']
    out['faster_beyond_noise'] = bool(f32['median_ms'] - b16['median_ms'] > noise)

    # per bf16 launch of the bf16 step: every profiled launch bracketed by events (serialises nothing: one stream)
    per = {}
    for _ in range(args.rounds):
        ops.PROFILE, ops.PROFILE_BY_KERNEL = [], {}
        step('bf16')
        torch.cuda.synchronize()
        for i, (variant, flop, e0, e1) in enumerate(ops.PROFILE):
            per.setdefault((i, str(variant)), []).append((flop, e0.elapsed_time(e1)))
        ops.PROFILE = ops.PROFILE_BY_KERNEL = None
    launches, bf_ms = [], 0.0
    for (i, variant), v in sorted(per.items()):
        if 'bf16' not in variant:
            continue
        flop, ms = v[0][0], statistics.median(t for _f, t in v)
        bf_ms += ms
        launches.append({'launch': i, 'variant': variant, 'gflop': flop / 1e9, 'median_ms': ms, 'tflops': flop / ms / 1e9,
                         'of_bf16_peak': flop / ms / 1e9 / PEAK_TFLOPS})
    out['bf16_launches'] = launches
    out['bf16_launches_ms'] = bf_ms
    out['bf16_launches_share_of_bf16_step'] = bf_ms / b16['median_ms']
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
    return 0 if out['faster_beyond_noise'] else 1


if __name__ == '__main__':
    sys.exit(main())
