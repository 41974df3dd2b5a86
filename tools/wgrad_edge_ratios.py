#!/usr/bin/env python
"""Measured error of every case of tests/test_wgrad_edges_gpu.py -> profiles/wgrad_edges.json.

Per case: the kernel's err against the float64 reference (max |got - ref| / scale, tests/wgrad_ref.py), the err of fp32 CPU
autograd on the same operands, and their ratio -- the figure the test bounds by MARGIN (and by one fp32 ulp of the scale from
below). Needs the GPU.

    python tools/wgrad_edge_ratios.py [--out profiles/wgrad_edges.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wgrad_edges.json'))
    args = ap.parse_args()
    from tests import test_wgrad_edges_gpu as T
    from tests.mem_arena import Arena
    arena = Arena('cuda:0')
    rows = [T.measure(c, arena)[0] for c in T.CASES]

    def worst(key):
        return [{'id': r['id'], key: r[key]} for r in sorted((r for r in rows if r[key] is not None), key=lambda r: -r[key])[:3]]
    out = {
        'what': 'err = max |got - float64 reference| / scale per case; ratio = kernel err / err of fp32 CPU autograd (same operands)',
        'margin': T.MARGIN, 'floor_fp32_ulp_of_scale': T.FLOOR,
        'worst_ratio_dw': worst('ratio_dw'), 'worst_ratio_db': worst('ratio_db'),
        'worst_err_dw_ulp': worst('err_dw_ulp'), 'worst_err_db_ulp': worst('err_db_ulp'),
        'cases': rows,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    for key in ('worst_ratio_dw', 'worst_ratio_db', 'worst_err_dw_ulp', 'worst_err_db_ulp'):
        print(key, json.dumps(out[key]))
    print('%d cases -> %s' % (len(rows), args.out))


if __name__ == '__main__':
    main()
