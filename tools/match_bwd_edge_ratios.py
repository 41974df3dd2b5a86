#!/usr/bin/env python
"""Measured error of every case of tests/test_match_bwd_edges_gpu.py -> profiles/match_bwd_edges.json.

Per case: the kernel's err against the float64 reference (max |got - ref| / scale, tests/match_bwd_ref.py) for grad_ov and
grad_su, the err of fp32 CPU autograd through the oracle's crop and distance functions on the same operands and orientations,
their ratio -- the figure the test bounds by MARGIN (and by one fp32 ulp of the scale from below) -- and the case's geometry.
Every case runs once. Needs the GPU.

    python tools/match_bwd_edge_ratios.py [--out profiles/match_bwd_edges.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'match_bwd_edges.json'))
    args = ap.parse_args()
    from tests import test_match_bwd_edges_gpu as T
    from tests.mem_arena import Arena
    arena = Arena('cuda:0')
    rows = [T.measure(c, arena)[0] for c in T.CASES]

    def worst(key):
        return [{'id': r['id'], key: r[key]} for r in sorted((r for r in rows if r[key] is not None), key=lambda r: -r[key])[:3]]
    out = {
        'what': 'err = max |got - float64 reference| / scale per case; ratio = kernel err / err of fp32 CPU autograd through the '
                'oracle\'s crop_overhead and l2_distance (same operands, same orientations)',
        'margin': T.MARGIN, 'floor_fp32_ulp_of_scale': T.FLOOR,
        'worst_ratio_ov': worst('ratio_ov'), 'worst_ratio_su': worst('ratio_su'),
        'worst_err_ov_ulp': worst('err_ov_ulp'), 'worst_err_su_ulp': worst('err_su_ulp'),
        'cases': rows,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    for key in ('worst_ratio_ov', 'worst_ratio_su', 'worst_err_ov_ulp', 'worst_err_su_ulp'):
        print(key, json.dumps(out[key]))
    print('%d cases -> %s' % (len(rows), args.out))


if __name__ == '__main__':
    main()
