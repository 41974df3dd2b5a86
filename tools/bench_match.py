#!/usr/bin/env python
"""Throughput of the fused match kernel at retrieval-like sizes (development aid)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from witw_amd import ops  # noqa: E402


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
    a = ap.parse_args()
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
