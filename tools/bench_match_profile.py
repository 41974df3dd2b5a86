#!/usr/bin/env python
"""Cost of the orientation profile next to the match it extends: match_profile against ops.match_fwd on the same operands, and
match_pairs_profile against ops.match_pairs on one pair list. Writes profiles/match_profile.json.

Method: device events around `reps` back-to-back launches (a window of ~0.2 s or more), every shape warmed up first, the paths
of a shape alternate over five rounds and the median is reported with all rounds beside it. No threshold is asserted: this is
the first measurement of these kernels. --parent-lib names a libwitw_hip.so built from the parent commit; its witw_match_fwd is
then timed through ctypes on the same operands, alternating with this build's, and the record states both ratios."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from witw_amd import match_profile, ops  # noqa: E402

F32_MFMA_PEAK = 157.3e12      # FLOP/s, v_mfma_f32_32x32x2_f32 on all 1,024 matrix pipes of an MI355X (spec)
SHAPES = ((128, 128, 64), (4096, 1, 12), (4096, 128, 64))      # a minibatch; a heat-map sweep at fov 70; a retrieval chunk
N_PAIRS = 40960


def _time(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _measure(paths, rounds=5, window_ms=200.):
    for run in paths.values():
        run()
    torch.cuda.synchronize()
    reps = {k: max(3, int(window_ms / max(_time(run, 3), 1e-3))) for k, run in paths.items()}
    ms = {k: [] for k in paths}
    for _ in range(rounds):
        for k, run in paths.items():
            ms[k].append(_time(run, reps[k]))
    return {k: statistics.median(v) for k, v in ms.items()}, ms, reps


def _parent_match_fwd(path, ov, su):
    """witw_match_fwd of another build of the library on (ov, su), outputs preallocated: a launch and nothing else"""
    lib = ctypes.CDLL(path)
    fn = lib.witw_match_fwd
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
    Bo, Bs, We = ov.shape[0], su.shape[0], su.shape[3]
    ori = torch.empty((Bo, Bs), dtype=torch.int64, device=ov.device)
    dist = torch.empty((Bo, Bs), dtype=torch.float32, device=ov.device)
    ws = torch.empty(Bo * 64 + Bs, dtype=torch.float32, device=ov.device)

    def run():
        rc = fn(ov.data_ptr(), su.data_ptr(), Bo, Bs, We, ori.data_ptr(), dist.data_ptr(), None, ws.data_ptr(),
                torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    return run, (ori, dist)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                    'match_profile.json'))
    ap.add_argument('--parent-lib', default=None, help='libwitw_hip.so of the parent commit (optional)')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    rows = []
    for bo, bs, we in SHAPES:
        g = torch.Generator(device='cpu').manual_seed(bo + bs + we)
        ov = torch.randn((bo, 16, 4, 64), generator=g).to(dev)
        su = torch.randn((bs, 16, 4, we), generator=g).to(dev)
        paths = {
            'match_fwd': lambda: ops.match_fwd(ov, su),
            'match_profile': lambda: match_profile.match_profile(ov, su),
            'match_profile_scores_only': lambda: match_profile.match_profile(ov, su, want_distances=False),
        }
        ori, dist = ops.match_fwd(ov, su)
        sc, ds = match_profile.match_profile(ov, su)
        first = sc.argmax(dim=-1)      # (torch's arg-max returns the first maximum on this data: no exact ties among normal scores)
        same = bool(torch.equal(first, ori) and torch.equal(torch.gather(ds, -1, first[..., None])[..., 0], dist))
        if a.parent_lib:
            paths['match_fwd_parent'], (p_ori, p_dist) = _parent_match_fwd(a.parent_lib, ov, su)
            paths['match_fwd_parent']()
            same = same and bool(torch.equal(p_ori, ori) and torch.equal(p_dist, dist))
        del sc, ds, first
        med, ms, reps = _measure(paths)
        flop = 2.0 * 64 * (64 * we) * bo * bs
        row = {'Bo': bo, 'Bs': bs, 'We': we, 'form': ops.last_kernel_variant(),
               'first_argmax_and_values_equal_match_fwd': same, 'ms': med, 'ms_all': ms, 'reps': reps,
               'profile_over_match_fwd': med['match_profile'] / med['match_fwd'],
               'profile_tflops': flop / med['match_profile'] / 1e9,
               'profile_fraction_of_f32_mfma_peak': flop / (med['match_profile'] * 1e-3) / F32_MFMA_PEAK,
               'output_bytes': 2 * 4 * 64 * bo * bs}
        if a.parent_lib:
            row['profile_over_parent_match_fwd'] = med['match_profile'] / med['match_fwd_parent']
            row['match_fwd_over_parent_match_fwd'] = med['match_fwd'] / med['match_fwd_parent']
        rows.append(row)
        print('Bo=%d Bs=%d We=%d: match_fwd %.4f ms | match_profile %.4f ms (x%.2f, %.1f TF/s) | scores only %.4f ms%s | bits: %s'
              % (bo, bs, we, med['match_fwd'], med['match_profile'], row['profile_over_match_fwd'], row['profile_tflops'],
                 med['match_profile_scores_only'],
                 ' | parent match_fwd %.4f ms' % med['match_fwd_parent'] if a.parent_lib else '', same), flush=True)
        del ov, su
    # the pair list: 40,960 pairs (4,096 queries x 10 candidates) of a 4,096 x 4,096 problem at full width
    bo = bs = 4096
    g = torch.Generator(device='cpu').manual_seed(7)
    ov = torch.randn((bo, 16, 4, 64), generator=g).to(dev)
    su = torch.randn((bs, 16, 4, 64), generator=g).to(dev)
    po = torch.randint(0, bo, (N_PAIRS,), generator=g, dtype=torch.int32).to(dev)
    ps = torch.arange(bs, dtype=torch.int32).repeat_interleave(N_PAIRS // bs).to(dev)
    ws = ops.match_fwd_fixed(ov, su[:1], torch.zeros(1, dtype=torch.int64, device=dev), want_workspace=True)[3]
    wn = ws[:bo * 64].contiguous()
    sn = ops.match_fwd_fixed(ov[:1], su, torch.zeros(bs, dtype=torch.int64, device=dev), want_workspace=True)[3][64:64 + bs].contiguous()
    paths = {
        'match_pairs': lambda: ops.match_pairs(ov, su, wn, sn, po, ps),
        'match_pairs_profile': lambda: match_profile.match_pairs_profile(ov, su, wn, sn, po, ps),
    }
    p_ori, p_dist = ops.match_pairs(ov, su, wn, sn, po, ps)
    sc, ds = match_profile.match_pairs_profile(ov, su, wn, sn, po, ps)
    first = sc.argmax(dim=-1)
    same = bool(torch.equal(first, p_ori) and torch.equal(torch.gather(ds, -1, first[:, None])[:, 0], p_dist))
    med, ms, reps = _measure(paths)
    hyp = {'profile_hypotheses_3': lambda: match_profile.profile_hypotheses(sc, 3, 4)}
    hmed, hms, hreps = _measure(hyp)
    pair_row = {'n_pairs': N_PAIRS, 'Bo': bo, 'Bs': bs, 'We': 64, 'first_argmax_and_values_equal_match_pairs': same, 'ms': med,
                'ms_all': ms, 'reps': reps, 'pairs_profile_over_match_pairs': med['match_pairs_profile'] / med['match_pairs'],
                'profile_hypotheses_3_ms': hmed['profile_hypotheses_3'], 'profile_hypotheses_3_ms_all': hms['profile_hypotheses_3']}
    print('%d pairs, We=64: match_pairs %.4f ms | match_pairs_profile %.4f ms (x%.2f) | 3 hypotheses of them %.4f ms | bits: %s'
          % (N_PAIRS, med['match_pairs'], med['match_pairs_profile'], pair_row['pairs_profile_over_match_pairs'],
             hmed['profile_hypotheses_3'], same), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, 'w') as f:
        json.dump({'device': torch.cuda.get_device_name(0), 'f32_mfma_peak_flops': F32_MFMA_PEAK,
                   'method': 'device events around back-to-back launches, >= 0.2 s windows, 5 alternating rounds, median',
                   'parent_match_fwd_timed': bool(a.parent_lib), 'rows': rows, 'pairs': pair_row}, f, indent=1)


if __name__ == '__main__':
    main()
