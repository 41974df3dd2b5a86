#!/usr/bin/env python
"""Time of ops.topk_smallest by list length on one retrieval chunk (125,000 x 4,096 fp32 distances): k <= 32 is one run of the
top-k kernels, a longer list ceil(k / 32) runs that each resume behind the run before (witw_topk_smallest_after).

Every k is warmed up, then the lengths alternate over --rounds repetitions (round-robin, so that drift of the box falls on all of
them alike) and the median per length is reported; each timing is one call between two device events.

--parent-lib PATH: another build of the library with the plain entries (the parent commit's) is loaded into the same process and
its witw_topk_smallest_ws takes turns with this build's at k <= 32, both through the same few lines (allocations as
ops.topk_smallest makes them), so that the two differ in the library alone. --json PATH keeps the table."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from witw_amd import _lib, ops  # noqa: E402


def _plain_entries(path):
    """the two plain top-k entries of the library at `path`, typed as _lib types them"""
    lib = ctypes.CDLL(path)
    for name in ('witw_topk_workspace_bytes', 'witw_topk_smallest_ws'):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def _plain_call(lib, d, k):
    """ops.topk_smallest at k <= 32, on `lib`"""
    Bo, Bs = d.shape
    vals = torch.empty((Bs, k), dtype=torch.float32, device=d.device)
    idx = torch.empty((Bs, k), dtype=torch.int64, device=d.device)
    nws = lib.witw_topk_workspace_bytes(Bo, Bs, k)
    ws = torch.empty((nws,), dtype=torch.uint8, device=d.device) if nws > 0 else None
    rc = lib.witw_topk_smallest_ws(d.data_ptr(), vals.data_ptr(), idx.data_ptr(), Bo, Bs, k, 0, ws.data_ptr() if nws > 0 else None,
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return vals, idx


def _ms(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--bo', type=int, default=125000)
    ap.add_argument('--bs', type=int, default=4096)
    ap.add_argument('--ks', default='10,32,64,128,512', help='list lengths, comma separated')
    ap.add_argument('--rounds', type=int, default=15, help='alternating repetitions per length')
    ap.add_argument('--parent-lib', default=None, metavar='PATH', help="the parent commit's libwitw_hip.so, timed at k <= 32")
    ap.add_argument('--json', default=None, metavar='PATH')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    ks = [int(x) for x in a.ks.split(',')]
    d = torch.rand((a.bo, a.bs), generator=torch.Generator(dev).manual_seed(1), device=dev)
    runs = {'k%d' % k: (lambda k=k: ops.topk_smallest(d, k)) for k in ks}
    same = {}
    if a.parent_lib:
        head, parent = _plain_entries(_lib.lib_path()), _plain_entries(a.parent_lib)
        for k in (k for k in ks if k <= ops.TOPK_LIST):
            runs['k%d_head_plain' % k] = lambda k=k: _plain_call(head, d, k)
            runs['k%d_parent_plain' % k] = lambda k=k: _plain_call(parent, d, k)
            (v0, i0), (v1, i1) = _plain_call(head, d, k), _plain_call(parent, d, k)
            same['k%d' % k] = bool(torch.equal(v0, v1) and torch.equal(i0, i1))
    for run in runs.values():      # every length and library warmed up
        run()
        run()
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    for _ in range(a.rounds):
        for name, run in runs.items():
            ms[name].append(_ms(run))
    rows = {}
    for name, v in ms.items():
        rows[name] = {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v), 'all_ms': v}
        print('%-18s median %.3f ms  (min %.3f, max %.3f, %d repetitions)' % (name, rows[name]['median_ms'], min(v), max(v), len(v)), flush=True)
    out = {'device': torch.cuda.get_device_name(0), 'Bo': a.bo, 'Bs': a.bs, 'dtype': 'float32', 'rounds': a.rounds,
           'timing': 'one call between two device events; lengths (and libraries) alternate round-robin; median over the rounds',
           'parent_lib_timed': bool(a.parent_lib), 'parent_same_bits_as_head': same, 'rows': rows}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
