#!/usr/bin/env python
"""Eval step of cvig_baseline (BASELINE config 1: 32 pairs, surface 500 x 500, overhead 512 x 512, uint8-valued inputs) under all three
precisions, 'fp32', 'bf16' (blocks 1-4 on the bf16 MFMA) and 'bf16_all' (blocks 5-7 as well):

  * the eval forward of both encoders between two device events, the three precisions alternating round-robin in one process (drift of
    the box falls on all alike), median of --rounds with minimum and maximum;
  * per launch of the 'bf16_all' step (ops.PROFILE: every conv launch between device events): algorithmic FLOP / time as TF/s and, for
    the bf16 kernels, as a share of the 2,500 TF/s bf16 matrix peak. The split-K record brackets the conv launch alone, not its finish;
  * --sweep: conv + finish of blocks 5-7 at the step's shapes for every candidate split-K factor (docs/experiments.md keeps the table).

The condition for the 'bf16_all' path to exist: its median lies below the 'bf16' median of the same run by more than the larger of the
two min-max ranges (`faster_beyond_noise`). Run it under `timeout`. --json PATH keeps the table (profiles/baseline_bf16_all.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from witw_amd import _lib, baseline_bf16, ops, synth  # noqa: E402
from witw_amd import cvig_baseline as cb  # noqa: E402

PEAK_TFLOPS = 2500.0
PRECISIONS = ('fp32', 'bf16', 'bf16_all')
SWEEP = (1, 2, 3, 4, 6, 8, 12, 16, 32)


def _event_ms(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _row(v):
    return {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v), 'all_ms': v}


def block_shapes(B, H, W):
    """(block, n_images, g, cell h, cell w, valid h, valid w) of blocks 5-7 for B images of H x W"""
    vh, vw, g, out, cell = H, W, 1, [], None
    for i in range(1, 8):
        vh, vw = (vh - 4) // 2 + 1, (vw - 4) // 2 + 1
        if i >= 5:
            out.append((i, B, g, cell[0], cell[1], vh, vw))
        if 4 <= i < 7:
            cell = ((vh + 1) // 2, (vw + 1) // 2)
            g = 1 if i == 4 else max(1, min(16 // cell[0], 16 // cell[1]))
    return out


def sweep(pairs, side, rounds, dev):
    lib = _lib.load()
    rows = []
    for blk, n, g, h, w, vh, vw in block_shapes(pairs, side, side):
        Bm = -(-n // (g * g))
        x = torch.randint(-2, 3, (Bm, g * h, g * w, 2048), device=dev).to(torch.bfloat16)
        pk = baseline_bf16.PackedConvBf16Taps4(torch.randn((512, 2048, 3, 3), device=dev) * 0.02, torch.zeros(512, device=dev))
        chosen = lib.witw_conv3x3_bf16_taps4_ksplit(Bm, g * h, g * w, 2048, 512)
        flop = 2.0 * 2048 * 512 * 4 * vh * vw * n
        for S in SWEEP:
            run = lambda: baseline_bf16.conv_taps4_splitk_bf16(x, pk, n, g, (vh, vw), ksplit=S)      # noqa: E731
            for _ in range(3):
                run()
            t = [_event_ms(run) for _ in range(rounds)]
            rows.append({'input_side': side, 'block': blk, 'mosaic': [Bm, g * h, g * w], 'workgroups_S1': 4 * Bm * (-(-g * h // 16)) * (-(-g * w // 16)),
                         'ksplit': S, 'chosen': S == chosen, 'conv_plus_finish_ms': {k: v for k, v in _row(t).items() if k != 'all_ms'}, 'tflops': flop / statistics.median(t) / 1e9,
                         'workspace_mb': S * Bm * g * h * g * w * 512 * 4 / 1e6})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--pairs', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sweep', action='store_true', help='also time blocks 5-7 at every candidate split-K factor')
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
    b16, ball = out['step_ms']['bf16'], out['step_ms']['bf16_all']
    noise = max(b16['max_ms'] - b16['min_ms'], ball['max_ms'] - ball['min_ms'])
    out['speedup_over_bf16'] = b16['median_ms'] / ball['median_ms']
    out['speedup_over_fp32'] = out['step_ms']['fp32']['median_ms'] / ball['median_ms']
    out['faster_beyond_noise'] = bool(b16['median_ms'] - ball['median_ms'] > noise)
    e = {p: torch.cat(step(p), 1).double() for p in PRECISIONS}
    out['embedding_distance_of_norm'] = {p: float(((e['bf16_all'] - e[p]).norm(dim=1) / e['fp32'].norm(dim=1)).max()) for p in ('fp32', 'bf16')}

    # per launch of the bf16_all step: every conv launch bracketed by events (serialises nothing: one stream)
    per = {}
    for _ in range(args.rounds):
        ops.PROFILE, ops.PROFILE_BY_KERNEL = [], {}
        step('bf16_all')
        torch.cuda.synchronize()
        for i, (variant, flop, e0, e1) in enumerate(ops.PROFILE):
            per.setdefault((i, str(variant)), []).append((flop, e0.elapsed_time(e1)))
        ops.PROFILE = ops.PROFILE_BY_KERNEL = None
    launches, tail_ms = [], 0.0
    for (i, variant), v in sorted(per.items()):
        flop, ms = v[0][0], statistics.median(t for _f, t in v)
        launches.append({'launch': i, 'variant': variant, 'gflop': flop / 1e9, 'median_ms': ms, 'tflops': flop / ms / 1e9,
                         'of_bf16_peak': flop / ms / 1e9 / PEAK_TFLOPS if 'bf16_taps4' in variant else None})
        if 'bf16_taps4_splitk' in variant:
            tail_ms += ms
    out['bf16_all_step_launches'] = launches
    out['blocks_5_7_conv_ms'] = tail_ms
    out['blocks_5_7_conv_share_of_bf16_all_step'] = tail_ms / ball['median_ms']
    lib = _lib.load()
    out['ksplit'] = {str(side): [lib.witw_conv3x3_bf16_taps4_ksplit(-(-n // (g * g)), g * h, g * w, 2048, 512)
                                 for _b, n, g, h, w, _vh, _vw in block_shapes(args.pairs, side, side)] for side in (500, 512)}
    if args.sweep:
        out['ksplit_sweep'] = sweep(args.pairs, 500, args.rounds, dev) + sweep(args.pairs, 512, args.rounds, dev)
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
    return 0 if out['faster_beyond_noise'] else 1


if __name__ == '__main__':
    sys.exit(main())
