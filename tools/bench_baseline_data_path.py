#!/usr/bin/env python
"""cvig_baseline's two data paths, 'reference' and 'packed' (cvig_baseline.Globals.data_path), in one process on one GPU:

  (a) preprocess only: GpuPreprocess on a batch that is already resident -- the per-sample route on float32 CHW tensors (one
      rotation, one roll / resize, one row doubling per sample, two stacks) against the two batched launches on staged uint8 HWC
      images, same angles, outputs compared bit for bit; device events, the two routes alternating, median of --rounds; the
      batched route's bytes (source bytes read once + fp32 outputs written) per second next to the 6.29 TB/s a float4 copy reaches;
  (b) disk -> embeddings: a synthetic JPEG data set of the same shapes through the loaders of cvig_baseline.test() (workers in
      {4, 16}), encoders in eval mode with precision='bf16_all': pairs per second of a whole pass (host clock around a pass that ends
      in a device synchronise) and of the pass behind its first batch (steady: without the workers' start), the two paths
      alternating, median of --passes; where the main process spends a pass (waiting for the loader, staging, enqueueing), see
      one_pass; and the encoders alone on resident input: the ceiling.

CVUSA shapes: overhead 750 x 750, panorama 224 x 1232; WITW shapes: overhead 512 x 512, photos of mixed sizes.
Required: 'packed' not slower than 'reference' at either worker count, the batched route not slower than the per-sample one; the
exit status says so. --json PATH keeps the table (profiles/baseline_data_path.json). Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from witw_amd import cvig_baseline as cb  # noqa: E402
from witw_amd import cvig_fov  # noqa: E402

HBM_COPY_TBS = 6.29          # measured float4 copy on the MI355X (of 8.0 TB/s nominal)
OVERHEAD = {'cvusa': (750, 750), 'witw': (512, 512)}
PANORAMA = (224, 1232)
PHOTOS = [(375, 500), (480, 640), (600, 400), (333, 500), (512, 512), (427, 640)]


def surface_size(dataset, i):
    return PANORAMA if dataset == 'cvusa' else PHOTOS[i % len(PHOTOS)]


def _picture(g, h, w):
    """noise at a quarter of the resolution, enlarged: files of a photograph's size rather than of white noise"""
    return g.integers(0, 256, size=(h // 4 + 1, w // 4 + 1, 3), dtype=np.uint8).repeat(4, 0).repeat(4, 1)[:h, :w]


def _write_pair(args):
    from PIL import Image
    root, dataset, i = args
    g = np.random.Generator(np.random.Philox(key=[91, i]))
    Image.fromarray(_picture(g, *OVERHEAD[dataset])).save(os.path.join(root, 'ov_%05d.jpg' % i), quality=90)
    Image.fromarray(_picture(g, *surface_size(dataset, i))).save(os.path.join(root, 'su_%05d.jpg' % i), quality=90)


def make_dataset(root, dataset, n_pairs, n_unique, procs=8):
    """n_pairs CSV rows over n_unique distinct JPEG pairs, in the CSV layout of the data set (as witw_amd.e2e.make_dataset builds its own)"""
    import multiprocessing as mp
    os.makedirs(root, exist_ok=True)
    n_unique = min(n_pairs, n_unique)
    with mp.get_context('spawn').Pool(procs) as pool:
        pool.map(_write_pair, [(root, dataset, i) for i in range(n_unique)], chunksize=4)
    csv = os.path.join(root, 'pairs.csv')
    with open(csv, 'w') as f:
        if dataset == 'witw':
            f.write(','.join('c%d' % i for i in range(17)) + '\n')
        for i in range(n_pairs):
            su, ov = 'su_%05d.jpg' % (i % n_unique), 'ov_%05d.jpg' % (i % n_unique)
            f.write('%s,%s\n' % (ov, su) if dataset == 'cvusa' else ','.join(['x'] * 15 + [su, ov]) + '\n')
    return csv


def _event_ms(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _row(v, unit):
    return {'median_' + unit: statistics.median(v), 'min_' + unit: min(v), 'max_' + unit: max(v)}


def preprocess_only(dataset, B, rounds, warmup, dev):
    g = np.random.Generator(np.random.Philox(key=[92, B]))
    samples = [{'surface': g.integers(0, 256, size=surface_size(dataset, i) + (3,), dtype=np.uint8),
                'overhead': g.integers(0, 256, size=OVERHEAD[dataset] + (3,), dtype=np.uint8)} for i in range(B)]
    angles = [(37.3 + 101.7 * i) % 360. for i in range(B)]
    resident = {k: [torch.from_numpy(s[k].astype(np.float32).transpose(2, 0, 1).copy()).to(dev) for s in samples] for k in ('surface', 'overhead')}
    prep = cb.GpuPreprocess(dataset, device=dev)
    staged = prep.stage(cb.collate_packed(samples), angles)
    routes = {'per_sample_f32': lambda: prep(resident, angles), 'batched_u8': lambda: prep(staged)}
    a, b = routes['per_sample_f32'](), routes['batched_u8']()
    same = bool(torch.equal(a['surface'], b['surface']) and torch.equal(a['overhead'], b['overhead']))
    moved = sum(s['surface'].size + s['overhead'].size for s in samples) + 4 * (b['surface'].numel() + b['overhead'].numel())
    del a, b
    for _ in range(warmup):
        for run in routes.values():
            run()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, run in routes.items():
            t[k].append(_event_ms(run) * 1e3)
    out = {'dataset': dataset, 'batch': B, 'bit_identical': same, 'us_per_batch': {k: _row(v, 'us') for k, v in t.items()},
           'batched_bytes': moved}
    med = {k: statistics.median(v) for k, v in t.items()}
    out['batched_tb_per_s'] = moved / med['batched_u8'] / 1e6
    out['batched_of_hbm_copy'] = out['batched_tb_per_s'] / HBM_COPY_TBS
    out['speedup'] = med['per_sample_f32'] / med['batched_u8']
    return out


class _Clock(object):
    """host seconds spent inside a callable, and how often it ran"""

    def __init__(self, fn):
        self.fn, self.seconds, self.calls = fn, 0., 0

    def __call__(self, *a, **kw):
        t = time.perf_counter()
        try:
            return self.fn(*a, **kw)
        finally:
            self.seconds += time.perf_counter() - t
            self.calls += 1


class _ClockedLoader(object):
    """a DataLoader whose iterator's creation (the workers start) and every next() (the main process waits for a batch) are timed"""

    def __init__(self, loader):
        self.loader, self.start_s, self.wait_s = loader, 0., 0.

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        t = time.perf_counter()
        it = iter(self.loader)
        self.start_s += time.perf_counter() - t
        while True:
            t = time.perf_counter()
            try:
                raw = next(it)
            except StopIteration:
                return
            finally:
                self.wait_s += time.perf_counter() - t
            yield raw


def one_pass(dataset, csv, data_path, batch, workers, encoders):
    """The loop of cvig_baseline.test() up to the embeddings, from the pieces test() itself is made of (_open_dataset, _staging,
    _embed_share; not test(): that adds the checkpoint load and the ranking), with host clocks on its stages. The clock starts
    AFTER _staging: the ring of the packed path (cvig_fov.make_staging) is allocated and closed outside every figure.
    -> {'pairs', 'seconds', 'pairs_per_s' (whole pass), 'first_batch_s' (worker start + the first batch), 'steady_pairs_per_s'
    (everything behind the first batch), and the main process's host seconds: 'workers_start_s' (iter(loader)), 'loader_wait_s'
    (blocked in next(loader)), 'stage_s' (GpuPreprocess.stage: copies queued, decode launches, the damage-flag wait; packed
    only), 'embed_s' (preprocess + both encoders enqueued; on the reference path the per-sample copies to the device too)}"""
    packed = data_path == 'packed'
    data_set = cb._open_dataset(dataset, csv, packed)
    prep, loader_kw, feed = cb._staging(dataset, data_set, batch, workers, packed)
    loader = _ClockedLoader(torch.utils.data.DataLoader(data_set, batch_size=batch, shuffle=False, drop_last=False, num_workers=workers, **loader_kw))
    prep.stage = stage = _Clock(prep.stage)
    embed = _Clock(cb._embed_share)
    torch.manual_seed(3)
    torch.cuda.synchronize()
    n = first_n = 0
    first_s = None
    t0 = time.perf_counter()
    for raw in feed(loader):
        su, _ov = embed(prep, encoders[0], encoders[1], raw)
        n += su.shape[0]
        if first_s is None:
            torch.cuda.synchronize()
            first_s, first_n = time.perf_counter() - t0, n
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if prep.ring is not None:
        del loader.loader
        prep.ring.close()
    return {'pairs': n, 'seconds': dt, 'pairs_per_s': n / dt, 'first_batch_s': first_s, 'steady_pairs_per_s': (n - first_n) / (dt - first_s),
            'workers_start_s': loader.start_s, 'loader_wait_s': loader.wait_s, 'stage_s': stage.seconds, 'embed_s': embed.seconds}


STAGES = ('seconds', 'first_batch_s', 'workers_start_s', 'loader_wait_s', 'stage_s', 'embed_s')


def disk_to_embeddings(dataset, root, pairs, unique, batch, workers_list, passes, dev):
    csv = make_dataset(os.path.join(root, dataset), dataset, pairs, unique)
    torch.manual_seed(1)
    encoders = (cb.SurfaceEncoder(precision='bf16_all').to(dev).eval(), cb.OverheadEncoder(precision='bf16_all').to(dev).eval())
    sh = (2 * PANORAMA[0], PANORAMA[1]) if dataset == 'cvusa' else (500, 500)
    su = torch.rand((batch, 3) + sh, device=dev) * 255.
    ov = torch.rand((batch, 3) + OVERHEAD[dataset], device=dev) * 255.

    def alone():
        with torch.no_grad():
            encoders[0](su), encoders[1](ov)

    for _ in range(3):
        alone()
    torch.cuda.synchronize()
    enc_ms = statistics.median(_event_ms(alone) for _ in range(15))
    out = {'dataset': dataset, 'pairs': pairs, 'distinct_files': min(pairs, unique), 'batch': batch, 'batches_per_pass': -(-pairs // batch),
           'precision': 'bf16_all', 'encoders_alone': {'ms_per_batch': enc_ms, 'pairs_per_s': batch / enc_ms * 1e3}, 'workers': {}}
    for workers in workers_list:
        one_pass(dataset, csv, 'packed', batch, workers, encoders)          # warm-up: the page cache, every kernel's code object
        runs = {'reference': [], 'packed': []}
        for _ in range(passes):
            for path in runs:
                runs[path].append(one_pass(dataset, csv, path, batch, workers, encoders))
                assert runs[path][-1]['pairs'] == pairs
        row = {'whole_pass': {k: _row([r['pairs_per_s'] for r in v], 'pairs_per_s') for k, v in runs.items()},
               'steady': {k: _row([r['steady_pairs_per_s'] for r in v], 'pairs_per_s') for k, v in runs.items()},
               'median_host_seconds_per_pass': {k: {st: statistics.median(r[st] for r in v) for st in STAGES} for k, v in runs.items()}}
        for key in ('whole_pass', 'steady'):
            row[key]['packed_over_reference'] = row[key]['packed']['median_pairs_per_s'] / row[key]['reference']['median_pairs_per_s']
            row[key]['packed_of_encoders_alone'] = row[key]['packed']['median_pairs_per_s'] / out['encoders_alone']['pairs_per_s']
        out['workers'][str(workers)] = row
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--datasets', nargs='+', default=['cvusa', 'witw'], choices=['cvusa', 'witw'])
    ap.add_argument('--batches', nargs='+', type=int, default=[32, 16])
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--pairs', type=int, default=1024, help='(b): rows of the data set')
    ap.add_argument('--unique', type=int, default=64, help='(b): distinct JPEG pairs behind them')
    ap.add_argument('--workers', nargs='+', type=int, default=[4, 16])
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--skip-disk', action='store_true', help='(a) only')
    ap.add_argument('--dir', default=None, help='where the data set is written (default: a temporary directory)')
    ap.add_argument('--json', default=None, metavar='PATH')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'device': torch.cuda.get_device_name(0), 'hbm_copy_tb_per_s': HBM_COPY_TBS, 'rounds': args.rounds, 'preprocess_only': [], 'disk_to_embeddings': []}
    for dataset in args.datasets:
        for B in args.batches:
            out['preprocess_only'].append(preprocess_only(dataset, B, args.rounds, args.warmup, dev))
    ok = all(r['bit_identical'] and r['speedup'] >= 1.0 for r in out['preprocess_only'])
    if not args.skip_disk:
        with tempfile.TemporaryDirectory(dir=args.dir) as root:
            for dataset in args.datasets:
                out['disk_to_embeddings'].append(disk_to_embeddings(dataset, root, args.pairs, args.unique, args.batches[0], args.workers, args.passes, dev))
        ok = ok and all(w[key]['packed_over_reference'] >= 1.0 for r in out['disk_to_embeddings'] for w in r['workers'].values() for key in ('whole_pass', 'steady'))
    out['requirements_met'] = bool(ok)
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
