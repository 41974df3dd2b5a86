#!/usr/bin/env python
"""Record the C-ABI call sequence of the FOV_DSM encoders, one canonical JSON file per configuration.

    python tools/trace_encoder_calls.py --out DIR

After _lib.load() the library handle is replaced by a proxy that notes, for every witw_* call, the entry name, the value of
each integer / float argument and null / non-null for each pointer (per _lib.SIGNATURES), then forwards the call. Two commits
whose files compare equal issue the same launches with the same arguments: what a refactor of the Python side has to show.
Only public API and _lib.SIGNATURES are used, so the file runs unchanged on older commits. A failing call raises
(_lib.check) and ends the run.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from witw_amd import _lib, cvig_fov, cvig_semantic, ops, parallel  # noqa: E402

CALLS = []


class Recorder(object):
    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        res, argtypes = _lib.SIGNATURES[name]

        def call(*args):
            rec = [name]
            for a, t in zip(args, argtypes):
                if t is ctypes.c_void_p:
                    rec.append('ptr' if (a.value if isinstance(a, ctypes.c_void_p) else a) else 'null')
                else:
                    rec.append(a)
            ret = fn(*args)
            CALLS.append(rec + ['->', ret] if res in (ctypes.c_int, ctypes.c_longlong) else rec)
            return ret
        setattr(self, name, call)
        return call


def encoder(module, circ, precision, fuse=None):
    enc = module.FOV_DSM(circ_padding=circ, seed=3).to('cuda')
    enc.precision, enc.fuse_first2 = precision, fuse
    return enc


def train_steps(enc, x, bucket=False):
    """two training steps through cvig_fov.Adam: the second one re-packs every trainable layer's filter images"""
    enc.train()
    opt = cvig_fov.Adam([p for p in enc.parameters() if p.requires_grad], lr=1e-4)
    if bucket:      # one rank: the wgrad kernels write straight into the bucket's views (GradBucket.direct())
        enc._grad_bucket = parallel.GradBucket(opt.params)
    for _step in range(2):
        opt.zero_grad()
        enc(x).square().sum().backward()
        if bucket and len(enc._grad_bucket.touched) != len(opt.params):      # set by notify() only: autograd was not involved
            raise SystemExit('GradBucket: the backward did not write its gradients directly')
        opt.step()


def run(module, circ, precision, fuse=None, batch=8, bucket=False, infer=True):
    torch.manual_seed(0)
    enc = encoder(module, circ, precision, fuse)
    x = torch.randn(batch, enc.in_channels, 128, 512, generator=torch.Generator().manual_seed(1)).to('cuda')
    if infer:
        enc.eval()
        with torch.no_grad():
            enc(x)
        if precision == 'bf16':
            enc.forward_bf16(x)
        if precision == 'fp16x3':
            enc.forward_f16x3(x)
    train_steps(enc, x, bucket)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    _lib._LIB = Recorder(_lib.load())
    mods = (('fov', cvig_fov), ('semantic', cvig_semantic))
    configs = []
    for mname, m in mods:
        for circ in (False, True):
            for prec in ('fp32', 'fp16x3'):
                configs.append(('%s_circ%d_%s' % (mname, circ, prec), dict(module=m, circ=circ, precision=prec)))
            for fuse in (True, False):
                configs.append(('%s_circ%d_bf16_fuse%d' % (mname, circ, fuse), dict(module=m, circ=circ, precision='bf16', fuse=fuse)))
    big = 128
    if not ops.gatebits_dgrad_ok(big, 128, 512, 64, 64):
        raise SystemExit('gatebits_dgrad_ok is false at batch %d: the fused training first layers would not be covered' % big)
    configs.append(('semantic_circ0_bf16_fuse1_b%d' % big, dict(module=cvig_semantic, circ=False, precision='bf16', fuse=True, batch=big, infer=False)))
    for mname, m in mods:
        for prec in ('fp32', 'bf16'):
            configs.append(('%s_circ1_%s_bucket' % (mname, prec), dict(module=m, circ=True, precision=prec, bucket=True, infer=False)))
    total = 0
    for name, kw in configs:
        del CALLS[:]
        run(**kw)
        with open(os.path.join(args.out, name + '.json'), 'w') as f:
            f.write(json.dumps(CALLS, sort_keys=True, separators=(',', ':')) + '\n')
        print('%-36s %5d calls' % (name, len(CALLS)), flush=True)
        total += len(CALLS)
        torch.cuda.empty_cache()
    print('%d configurations, %d recorded calls' % (len(configs), total))


if __name__ == '__main__':
    main()
