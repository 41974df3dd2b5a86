#!/usr/bin/env python
"""Throughput of the fused match kernel at retrieval-like sizes (development aid)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from witw_amd import ops  # noqa: E402


F32_MFMA_PEAK = 157.3e12      # FLOP/s, v_mfma_f32_32x32x2_f32 on all 1,024 matrix pipes of an MI355X (spec; 155e12 measured)


def _time(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def fixed_table(a):
    """witw_match_fwd_fixed against the masked direct and the masked spectral kernel on the same inputs and one-bit words. Every
    shape is warmed up, the three paths alternate over `rounds` rounds (the median is reported), a window is at least ~0.2 s of
    work except for the direct kernel at 125,000 x 1,024 (0.5 s a launch: one launch per round). Distances only (no orientation
    matrix), spectra cached, as retrieval runs the passes."""
    import json
    import statistics
    dev = torch.device('cuda:0')
    rows = []
    for bo, bs in ((128, 128), (125000, 1024)):
        for we in (64, 12):
            ov = torch.randn((bo, 16, 4, 64), device=dev)
            su = torch.randn((bs, 16, 4, we), device=dev)
            spec_g, spec_q = ops.match_spectrum(ov, overhead=True), ops.match_spectrum(su, overhead=False)
            for shifts in ('one', 'random'):
                sh = torch.full((bs,), 32, dtype=torch.int64, device=dev) if shifts == 'one' else torch.randint(0, 64, (bs,), device=dev)
                words = torch.where(sh == 63, torch.full_like(sh, -2 ** 63), torch.ones_like(sh) << sh.clamp(max=62))
                paths = {
                    'fixed': lambda: ops.match_fwd_fixed(ov, su, sh, want_orientation=False),
                    'masked': lambda: ops.match_fwd(ov, su, shift_mask=words),
                    'dft_masked': lambda: ops.match_fwd_dft(ov, su, spec_ov=spec_g, spec_su=spec_q, want_orientation=False, shift_mask=words),
                }
                d_f, d_m = paths['fixed']()[1], paths['masked']()[1]
                same = bool(torch.equal(d_f, d_m))
                del d_f, d_m
                big = bo * bs > 1 << 20
                reps = {'fixed': 20 if big else 2000, 'masked': 1 if big else 2000, 'dft_masked': 10 if big else 2000}
                for run in paths.values():
                    run()
                torch.cuda.synchronize()
                ms = {k: [] for k in paths}
                for _ in range(3 if big else 5):
                    for k, run in paths.items():
                        ms[k].append(_time(run, reps[k]))
                med = {k: statistics.median(v) for k, v in ms.items()}
                flop = 2.0 * 64 * we * bo * bs
                row = {'Bo': bo, 'Bs': bs, 'We': we, 'shifts': shifts, 'bit_identical_to_masked': same,
                       'ms': med, 'ms_all': ms, 'fixed_tflops': flop / med['fixed'] / 1e9,
                       'fixed_fraction_of_f32_mfma_peak': flop / (med['fixed'] * 1e-3) / F32_MFMA_PEAK}
                rows.append(row)
                print('Bo=%d Bs=%d We=%d shifts=%s: fixed %.3f ms (%.1f TF/s, %.0f %% of the fp32 MFMA peak) | masked %.3f ms | '
                      'dft_masked %.3f ms | same bits as masked: %s' % (bo, bs, we, shifts, med['fixed'], row['fixed_tflops'],
                                                                       100 * row['fixed_fraction_of_f32_mfma_peak'], med['masked'],
                                                                       med['dft_masked'], same), flush=True)
            del ov, su, spec_g, spec_q
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'f32_mfma_peak_flops': F32_MFMA_PEAK, 'rows': rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bo', type=int, default=8192)
    ap.add_argument('--bs', type=int, default=1024)
    ap.add_argument('--we', type=int, default=64)
    ap.add_argument('--mask-width', type=int, default=0, metavar='N',
                    help='restrict every query to a window of N consecutive shifts at a random start (witw_match_fwd_masked); '
                         '0 = no mask (witw_match_fwd)')
    ap.add_argument('--dft', action='store_true',
                    help='time the spectral pass (witw_match_fwd_dft on cached spectra, value-only at --we 64 as retrieval runs it; '
                         'with --mask-width: witw_match_fwd_dft_masked)')
    ap.add_argument('--reps', type=int, default=3, help='timed launches')
    ap.add_argument('--fixed', action='store_true',
                    help='known orientation: time witw_match_fwd_fixed next to the two other ways to the same answer -- '
                         'witw_match_fwd_masked and witw_match_fwd_dft_masked under one-bit words -- alternating them, at '
                         '128 x 128 and 125,000 x 1,024, fov 360 (We 64) and fov 70 (We 12), all queries at one shift (the aligned '
                         'protocol) and at random shifts; --json PATH keeps the table')
    ap.add_argument('--json', default=None, metavar='PATH', help='--fixed: write the measurements here')
    a = ap.parse_args()
    if a.fixed:
        return fixed_table(a)
    dev = torch.device('cuda:0')
    ov = torch.randn((a.bo, 16, 4, 64), device=dev)
    su = torch.randn((a.bs, 16, 4, a.we), device=dev)
    mask = None
    if a.mask_width:
        if not 1 <= a.mask_width <= 64:
            ap.error('--mask-width must lie in [1, 64]')
        start = torch.randint(0, 64, (a.bs,), device=dev)
        window = (1 << a.mask_width) - 1                       # rotated left by `start` inside 64 bits, built bit by bit
        bits = torch.zeros((a.bs,), dtype=torch.int64, device=dev)
        for j in range(64):
            if (window >> j) & 1:
                k = (start + j) % 64
                bits |= torch.where(k == 63, torch.full_like(k, -2 ** 63), torch.ones_like(k) << k.clamp(max=62))
        mask = bits
    masked = {} if mask is None else {'shift_mask': mask}
    if a.dft:
        spec_g, spec_q = ops.match_spectrum(ov, overhead=True), ops.match_spectrum(su, overhead=False)

        def run():
            return ops.match_fwd_dft(ov, su, spec_ov=spec_g, spec_su=spec_q, want_orientation=False, **masked)
    else:
        def run():
            return ops.match_fwd(ov, su, **masked)
    for _ in range(2):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    n = a.reps
    for _ in range(n):
        ori, d = run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    fl = 2.0 * a.bo * a.bs * 64 * 64 * a.we
    print('%s Bo=%d Bs=%d We=%d mask-width=%d: %.3f ms  %.1f TF/s%s  (%.1f M pairs/s)' % (
        'match_dft' if a.dft else 'match', a.bo, a.bs, a.we, a.mask_width, ms, fl / ms / 1e9,
        ' (of the direct form)' if a.dft else '', a.bo * a.bs / ms / 1e3))


if __name__ == '__main__':
    main()
