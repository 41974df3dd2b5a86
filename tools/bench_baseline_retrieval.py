#!/usr/bin/env python
"""Time of cvig_baseline gallery retrieval at the BASELINE config-5 shape (125,000 gallery rows x 10,000 queries x 1,536 per GPU):

  * witw_sqdist_gemm alone on one query chunk (125,000 x 4,096 x 1,536), as TF/s against the 157.3 TF/s fp32 matrix peak;
  * cvig_baseline.retrieve(k=10) under method='gemm';
  * the same call under method='direct' -- the difference-form kernel, the only route before the GEMM pass existed.

Every form is warmed up, then the two retrieve methods alternate over --rounds repetitions (round-robin, so that drift of the box
falls on both alike); the median, minimum and maximum per form are reported. The kernel is one call between two device events;
a retrieve call reads its ranks back, so it is wall time between two device synchronisations. The re-scored share of the pairs
comes from cvig_baseline.last_retrieve_stats(). Embeddings: random normal rows through ops.embed_normalize_, queries = their
true row plus noise. --json PATH keeps the table (profiles/baseline_retrieval.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from witw_amd import baseline_retrieval as br  # noqa: E402
from witw_amd import cvig_baseline as cb  # noqa: E402
from witw_amd import ops  # noqa: E402

PEAK_TFLOPS = 157.3


def _event_ms(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _wall_ms(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _row(v):
    return {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v), 'all_ms': v}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--gallery', type=int, default=125000)
    ap.add_argument('--queries', type=int, default=10000)
    ap.add_argument('--chunk', type=int, default=4096)
    ap.add_argument('--width', type=int, default=1536)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5, help='alternating repetitions per retrieve method')
    ap.add_argument('--kernel-rounds', type=int, default=15)
    ap.add_argument('--json', default=None, metavar='PATH')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    gen = torch.Generator(dev).manual_seed(1)
    gal = ops.embed_normalize_(torch.randn((a.gallery, a.width), generator=gen, device=dev))
    qry = gal[:a.queries] + 0.05 * torch.randn((a.queries, a.width), generator=gen, device=dev)
    rows = {}

    gn, qn = br.row_sqnorm(gal), br.row_sqnorm(qry)
    chunk = qry[:a.chunk].contiguous()
    kernel = lambda: br.sqdist_gemm(gal, chunk, gn, qn[:a.chunk])      # noqa: E731
    kernel()
    kernel()
    rows['sqdist_gemm'] = _row([_event_ms(kernel) for _ in range(a.kernel_rounds)])
    flop = 2.0 * a.gallery * chunk.shape[0] * a.width
    rows['sqdist_gemm']['tflops'] = flop / (rows['sqdist_gemm']['median_ms'] * 1e-3) / 1e12
    rows['sqdist_gemm']['share_of_peak'] = rows['sqdist_gemm']['tflops'] / PEAK_TFLOPS
    print('sqdist_gemm %d x %d x %d: median %.3f ms = %.1f TF/s (%.2f of %.1f)' % (
        a.gallery, chunk.shape[0], a.width, rows['sqdist_gemm']['median_ms'], rows['sqdist_gemm']['tflops'],
        rows['sqdist_gemm']['share_of_peak'], PEAK_TFLOPS), flush=True)

    out = {}
    runs = {m: (lambda m=m: out.__setitem__(m, cb.retrieve(gal, qry, k=a.k, query_chunk=a.chunk, method=m))) for m in ('gemm', 'direct')}
    for run in runs.values():
        run()
    stats = None
    ms = {m: [] for m in runs}
    for _ in range(a.rounds):
        for m, run in runs.items():
            ms[m].append(_wall_ms(run))
            if m == 'gemm':
                stats = cb.last_retrieve_stats()
    same = bool((out['gemm'][0] == out['direct'][0]).all() and torch.equal(out['gemm'][2], out['direct'][2])
                and torch.equal(out['gemm'][1], out['direct'][1]))
    for m, v in ms.items():
        rows['retrieve_' + m] = _row(v)
        print('retrieve(k=%d, %r): median %.1f ms (min %.1f, max %.1f, %d repetitions)' % (a.k, m, statistics.median(v), min(v), max(v), len(v)),
              flush=True)
    rescored = (stats['rescored_rank'] + stats['rescored_topk'] + stats['rescored_true']) / stats['pairs']
    print('gemm / direct = %.3f; re-scored share of the pairs %.2e (%s); same ranks, lists and distances: %s' % (
        rows['retrieve_gemm']['median_ms'] / rows['retrieve_direct']['median_ms'], rescored, stats, same), flush=True)
    res = {'device': torch.cuda.get_device_name(0), 'gallery': a.gallery, 'queries': a.queries, 'chunk': a.chunk, 'width': a.width, 'k': a.k,
           'timing': 'kernel: one call between two device events; retrieve: wall time between device synchronisations, methods '
                     'alternating round-robin; median over the rounds', 'peak_tflops': PEAK_TFLOPS, 'rows': rows, 'gemm_stats': stats,
           'rescored_share': rescored, 'gemm_equals_direct': same}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
