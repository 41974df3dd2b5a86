#!/usr/bin/env python
"""Eval step of cvig_baseline (BASELINE config 1: 32 pairs, surface 500 x 500, overhead 512 x 512, uint8-valued inputs) under
precision='fp32' and precision='bf16':

  * the eval forward of both encoders between two device events, fp32 and bf16 alternating round-robin in one process (drift of the
    box falls on both alike), median of --rounds with minimum and maximum;
  * per bf16 kernel instantiation (blocks 1-4 of both encoders): time per launch between device events (ops.PROFILE), algorithmic
    FLOP (4 taps; 16 for the first block) / time as TF/s and as a share of the 2,500 TF/s bf16 matrix peak;
  * the time of blocks 5-7 (the fp32 split-K launches + pooling) inside the bf16 step, and its share of the step.

The condition for the bf16 path to exist: its median lies below the fp32 median by more than the larger of the two min-max ranges
(`faster_beyond_noise`). Run it under `timeout`. --json PATH keeps the table (profiles/baseline_bf16.json)."""
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
PRECISIONS = ('fp32', 'bf16')      # the third value, 'bf16_all', has tools/bench_baseline_bf16_all.py


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
    torch.manual_seed(0)
    su = torch.from_numpy(synth.images_u8(90, 0, (args.pairs, 3, 500, 500))).to(dev)
    ov = torch.from_numpy(synth.images_u8(90, 1, (args.pairs, 3, 512, 512))).to(dev)
    enc = {}
    for prec in PRECISIONS:
        torch.manual_seed(1)
        enc[prec] = (cb.SurfaceEncoder(precision=prec).to(dev).eval(), cb.OverheadEncoder(precision=prec).to(dev).eval())

    def step(prec):
        s, o = enc[prec]
        return s(su), o(ov)

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

    # per launch of the bf16 step: every conv launch bracketed by events (serialises nothing: one stream)
    per = {}
    for _ in range(args.rounds):
        ops.PROFILE, ops.PROFILE_BY_KERNEL = [], {}
        step('bf16')
        torch.cuda.synchronize()
        for i, (variant, flop, e0, e1) in enumerate(ops.PROFILE):
            per.setdefault((i, str(variant)), []).append((flop, e0.elapsed_time(e1)))
        ops.PROFILE = ops.PROFILE_BY_KERNEL = None
    launches, tail_ms = [], 0.0
    for (i, variant), v in sorted(per.items()):
        flop, ms = v[0][0], statistics.median(t for _f, t in v)
        launches.append({'launch': i, 'variant': variant, 'gflop': flop / 1e9, 'median_ms': ms, 'tflops': flop / ms / 1e9,
                         'of_bf16_peak': flop / ms / 1e9 / PEAK_TFLOPS if 'bf16_taps4' in variant else None})
        if 'bf16_taps4' not in variant and 'first4x4' not in variant:
            tail_ms += ms
    out['bf16_step_launches'] = launches
    out['blocks_5_7_conv_ms'] = tail_ms
    out['blocks_5_7_conv_share_of_bf16_step'] = tail_ms / b16['median_ms']
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
    return 0 if out['faster_beyond_noise'] else 1


if __name__ == '__main__':
    sys.exit(main())
