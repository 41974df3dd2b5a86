#!/usr/bin/env python
"""What a loader worker pays for a PROGRESSIVE file (host only, one thread): the progressive entropy decoder of libwitw_jpeg.so
(jpeg.open_file(progressive=True) + decode_into: coefficient blocks, the GPU does the rest) against Pillow's whole decode of the same
bytes (what the worker does with the flag off). 512 x 512 images of photographic statistics (tests/golden/gen_jpeg_fixtures.py's
generator), saved progressive at quality 88; per file: the median over the passes of (time of one pass over all files / files).
Writes profiles/jpeg_progressive.json.   python tools/bench_jpeg_progressive.py [--files 64] [--passes 7]

--corpus 440: the same for 4:4:0 files (jpeg.SAMPLING_440; tests/jpeg_440_craft.py: the 4:2:2 timing images re-crafted as 4:4:0 from
their transposed coefficient blocks, i.e. losslessly transposed). Opt-in on, a worker pays what DEVICE_ENTROPY leaves it -- the header
parse and marker scan (entropy_plan, the default 'all'), or the host Huffman decode (decode_into); opt-in off, Pillow's whole decode.
Writes profiles/jpeg_440.json, keeping an 'e2e' block that is already there.
--e2e-440 DIR: the GPU half of that profile. A synthetic data set (witw_amd/e2e.py) whose 224 x 224 surfaces are re-crafted as 4:4:0,
then `bench.py --mode e2e --workers 4 --precision bf16` as child processes, WITW_JPEG_440=1 and unset in alternating rounds; the
median of each goes into the 'e2e' block of profiles/jpeg_440.json.

--device-scans worker | device | e2e: the three measurements of the DEVICE route of progressive files (jpeg.PROGRESSIVE_DEVICE), each
into its block of profiles/jpeg_progressive_device.json. worker (no GPU; --key NAME files it under another name, e.g. a second box):
scan_plan() per file against the host progressive decode and Pillow. device: the stage launches over 128 files against the
self-synchronising kernel on their sequential twins, hip events, median of 7 after a warm-up. e2e (--e2e-dir DIR): a synthetic data
set re-saved progressive, `bench.py --mode e2e --workers 4 --precision bf16` as child processes with the device route, the host route
and neither, in alternating rounds."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def picture(g, h, w):
    from PIL import Image
    small = g.integers(0, 256, size=(h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
    img = np.asarray(Image.fromarray(small).resize((w + 16, h + 16), Image.BICUBIC))[8:8 + h, 8:8 + w]
    return np.clip(img.astype(np.int16) + g.integers(-20, 21, size=(h, w, 3)), 0, 255).astype(np.uint8)


def per_file_us(fn, blobs, passes):
    fn(blobs)                                            # first touch outside the timing
    t = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn(blobs)
        t.append((time.perf_counter() - t0) / len(blobs) * 1e6)
    return statistics.median(t), min(t)


def corpus_440(a):
    import torch
    from PIL import Image
    from tests import jpeg_440_craft as C4
    from witw_amd import jpeg
    torch.set_num_threads(1)
    g = np.random.Generator(np.random.Philox(key=[2026, 440]))
    s422, s440 = [], []
    for _ in range(a.files):
        bio = io.BytesIO()
        Image.fromarray(picture(g, a.size, a.size)).save(bio, 'JPEG', quality=a.quality, subsampling=1)
        s422.append(bio.getvalue())
        src = jpeg.read_coef(s422[-1])
        s440.append(C4.write(a.size, a.size, *C4.transposed(src)))
    first = jpeg.open_file(s440[0], h1v2=True)
    coef = np.empty((int(first.info[5]), 64), dtype=np.int16)
    qt = np.empty((int(first.info[2]), 64), dtype=np.uint16)

    def host_huffman(blobs):
        for b in blobs:
            if not jpeg.open_file(b, h1v2=True).decode_into(coef, qt):
                raise RuntimeError('decode failed')

    def plan(blobs):
        for b in blobs:
            if jpeg.open_file(b, h1v2=True).entropy_plan() is None:
                raise RuntimeError('no plan')

    def pillow(blobs):
        for b in blobs:
            Image.open(io.BytesIO(b)).load()

    for b, s in zip(s440, s422):                          # the numbers below are about a decoder that is right
        assert np.array_equal(jpeg.read_coef(b, h1v2=True).coef, C4.transposed(jpeg.read_coef(s))[0])
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(b))), C4.decode(first.info, *C4.transposed(jpeg.read_coef(s))))
    res = {}
    for name, fn, blobs in (('440_host_header_and_marker_scan', plan, s440), ('440_host_entropy_decode', host_huffman, s440),
                            ('440_pillow_full_decode', pillow, s440), ('422_host_entropy_decode', host_huffman, s422),
                            ('422_pillow_full_decode', pillow, s422)):
        med, best = per_file_us(fn, blobs, a.passes)
        res[name] = {'us_per_file_median': round(med, 1), 'us_per_file_best': round(best, 1)}
    pil = res['440_pillow_full_decode']['us_per_file_median']
    return {'what': '%d 4:4:0 JPEG files, %d x %d, quality %d (the 4:2:2 files Pillow writes, losslessly transposed); one thread; per file = '
                    'median over %d passes of (pass time / files). Opt-in off a worker pays 440_pillow_full_decode; opt-in on, '
                    '440_host_header_and_marker_scan under DEVICE_ENTROPY all (the default), 440_host_entropy_decode with it off'
                    % (a.files, a.size, a.size, a.quality, a.passes),
            'mean_file_bytes': {'440': int(np.mean([len(b) for b in s440])), '422': int(np.mean([len(b) for b in s422]))},
            'results': res,
            '440_host_entropy_decode_over_pillow_full_decode': round(res['440_host_entropy_decode']['us_per_file_median'] / pil, 3),
            '440_host_header_and_marker_scan_over_pillow_full_decode': round(res['440_host_header_and_marker_scan']['us_per_file_median'] / pil, 4),
            'pillow': Image.__version__ if hasattr(Image, '__version__') else None}


def _recraft_surface(path):
    from tests import jpeg_440_craft as C4
    from witw_amd import jpeg
    from PIL import Image
    a = np.asarray(Image.open(path))
    bio = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(a.transpose(1, 0, 2))).save(bio, 'JPEG', quality=90, subsampling=1)
    src = jpeg.read_coef(bio.getvalue())
    data = C4.write(int(src.info[1]), int(src.info[0]), *C4.transposed(src))
    with open(path + '.tmp', 'wb') as f:
        f.write(data)
    os.replace(path + '.tmp', path)
    return len(data)


def e2e_440(a):
    """disk -> embeddings, 4 loader workers, bf16 encoders; surfaces 4:4:0; opt-in on against off, alternating rounds, medians"""
    import multiprocessing as mp
    import subprocess
    from witw_amd import e2e
    procs = min(16, len(os.sched_getaffinity(0)))
    _csv, n_unique, _size = e2e.make_dataset(a.e2e_440, a.e2e_pairs, procs=procs)      # (its manifest keeps bench.py from writing the files again)
    with mp.get_context('spawn').Pool(procs) as pool:
        sizes = pool.map(_recraft_surface, [os.path.join(a.e2e_440, 'su_%05d.jpg' % i) for i in range(n_unique)], chunksize=8)
    runs = {'on': [], 'off': []}
    for r in range(a.rounds):
        for mode in (('on', 'off') if r % 2 == 0 else ('off', 'on')):
            env = dict(os.environ)
            env.pop('WITW_JPEG_440', None)
            if mode == 'on':
                env['WITW_JPEG_440'] = '1'
            fd_path = os.path.join(a.e2e_440, 'detail_%s_%d.json' % (mode, r))
            cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--mode', 'e2e', '--e2e-pairs', str(a.e2e_pairs), '--workers', '4',
                   '--precision', 'bf16', '--e2e-dir', a.e2e_440, '--no-decode-scaling', '--detail-out', fd_path]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                raise RuntimeError('bench.py --mode e2e failed (%d): %s' % (p.returncode, p.stderr[-800:]))
            line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1])
            d = json.load(open(fd_path)) if os.path.exists(fd_path) else line
            runs[mode].append({'pairs_per_s': d.get('value', line.get('value')), 'steady_state_pairs_per_s': d.get('steady_state_pairs_per_s')})
            print(mode, r, runs[mode][-1], flush=True)
    med = {m: statistics.median(x['pairs_per_s'] for x in v) for m, v in runs.items()}
    steady = {m: statistics.median(x['steady_state_pairs_per_s'] or 0 for x in v) for m, v in runs.items()}
    return {'what': 'disk -> embeddings (bench.py --mode e2e): %d pairs over %d distinct, overhead 512 x 512 4:2:0 (Pillow), surface 224 x 224 '
                    '4:4:0 (mean %d bytes); 4 loader workers, bf16 encoders, batch 128; WITW_JPEG_440=1 against unset in %d alternating '
                    'rounds, one child process each; medians' % (a.e2e_pairs, n_unique, int(np.mean(sizes)), a.rounds),
            'pairs_per_s_median': med, 'steady_state_pairs_per_s_median': steady, 'on_over_off': round(med['on'] / med['off'], 3),
            'steady_state_on_over_off': round(steady['on'] / max(1e-9, steady['off']), 3), 'rounds': runs}


def _timing_set(a):
    """the tool's 64-file set: (progressive files, their sequential twins)"""
    from PIL import Image
    g = np.random.Generator(np.random.Philox(key=[2026, 88]))
    prog, seq = [], []
    for _ in range(a.files):
        img = Image.fromarray(picture(g, a.size, a.size))
        for blobs, kw in ((prog, {'progressive': True}), (seq, {})):
            bio = io.BytesIO()
            img.save(bio, 'JPEG', quality=a.quality, **kw)
            blobs.append(bio.getvalue())
    return prog, seq


def device_scans_worker(a):
    """what a loader worker pays per progressive file on the device route (open_file + scan_plan: a byte scan) against the host route
    (open_file + decode_into) and Pillow's whole decode; one thread, no GPU"""
    import torch
    from PIL import Image
    from witw_amd import jpeg
    torch.set_num_threads(1)
    prog, _seq = _timing_set(a)
    first = jpeg.open_file(prog[0], progressive=True)
    coef = np.empty((int(first.info[5]), 64), dtype=np.int16)
    qt = np.empty((int(first.info[2]), 64), dtype=np.uint16)

    def plan(blobs):
        for b in blobs:
            if jpeg.open_file(b, progressive='device').scan_plan() is None:
                raise RuntimeError('no plan')

    def host(blobs):
        for b in blobs:
            if not jpeg.open_file(b, progressive=True).decode_into(coef, qt):
                raise RuntimeError('decode failed')

    def pillow(blobs):
        for b in blobs:
            Image.open(io.BytesIO(b)).load()

    res = {}
    for name, fn in (('scan_plan', plan), ('host_progressive_entropy_decode', host), ('pillow_full_decode', pillow)):
        med, best = per_file_us(fn, prog, a.passes)
        res[name] = {'us_per_file_median': round(med, 1), 'us_per_file_best': round(best, 1)}
    res['scan_plan_over_host_decode'] = round(res['scan_plan']['us_per_file_median'] / res['host_progressive_entropy_decode']['us_per_file_median'], 4)
    res['scan_plan_over_pillow'] = round(res['scan_plan']['us_per_file_median'] / res['pillow_full_decode']['us_per_file_median'], 4)
    res['plan_bytes'] = int(jpeg.open_file(prog[0], progressive='device').scan_plan()[0].size)
    try:
        res['cpu'] = next(ln.split(':', 1)[1].strip() for ln in open('/proc/cpuinfo') if ln.startswith('model name'))
    except (OSError, StopIteration):
        pass
    return res


def device_scans_device(a):
    """device time of the stage launches over 128 progressive files (the 64-file set twice) against the self-synchronising kernel on
    their sequential twins: events around the launches, median of 7 after a warm-up; both checked against the host decoder first"""
    import torch
    from witw_amd import _lib, jpeg, ops
    dev = torch.device('cuda:0')
    prog, seq = _timing_set(a)
    prog, seq = (prog + prog)[:128], (seq + seq)[:128]
    lib, st = _lib.load(), ops._stream()

    def rows_of(blobs, planner, extra):
        items = [jpeg.open_file(b, progressive='device') for b in blobs]
        plans = [planner(it)[0] for it in items]
        blocks = np.array([int(it.info[5]) for it in items], dtype=np.int64)
        first = np.cumsum(blocks) - blocks
        coef = torch.zeros((int(blocks.sum()), 64), dtype=torch.int16, device=dev)
        keep, rows = [coef], []
        for it, plan, f0 in zip(items, plans, first):
            raw = np.zeros((it.data.size + 24 + 7) // 8 * 8, dtype=np.uint8)
            raw[:it.data.size] = it.data
            rb, pb = torch.from_numpy(raw).to(dev), torch.from_numpy(np.concatenate([plan, np.zeros(16, np.uint8)])).to(dev)
            row = [rb.data_ptr(), pb.data_ptr(), coef.data_ptr() + int(f0) * 128, it.data.size]
            if extra:
                sc = torch.empty(((it.data.size + 32 + 7) // 8 * 8,), dtype=torch.uint8, device=dev)
                keep.append(sc)
                row += [sc.data_ptr(), 0]
            keep += [rb, pb]
            rows.append(row)
        return torch.tensor(rows, dtype=torch.int64, device=dev), coef, plans, keep, first, blocks

    pf, pcoef, pplans, _k1, pfirst, pblocks = rows_of(prog, lambda it: it.scan_plan(), False)
    sf, scoef, _sp, _k2, _sfirst, _sb = rows_of(seq, lambda it: it.entropy_plan(), True)
    errors = torch.zeros((128,), dtype=torch.int32, device=dev)
    sizes = [jpeg.prog_launch_sizes(p) for p in pplans]
    segs, scans, stages = max(s & 0xffffffff for s in sizes), max((s >> 32) & 0xff for s in sizes), max(s >> 40 for s in sizes)

    def run_prog():
        for stage in range(stages):
            _lib.check(lib.witw_jpeg_progressive_stage(pf.data_ptr(), 128, stage, scans, segs, errors.data_ptr(), st), 'witw_jpeg_progressive_stage')

    def run_seq():
        _lib.check(lib.witw_jpeg_huffman_selfsync_threads(sf.data_ptr(), 128, 1024, errors.data_ptr(), st), 'witw_jpeg_huffman_selfsync_threads')

    def timed(fn, coef):
        t = []
        for i in range(8):                                   # the first is the warm-up
            coef.zero_()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i:
                t.append(e0.elapsed_time(e1))
        return statistics.median(t), min(t)

    p_med, p_best = timed(run_prog, pcoef)
    s_med, s_best = timed(run_seq, scoef)
    assert int(errors.sum().item()) == 0
    want = jpeg.read_coef(prog[0], progressive=True).coef     # the numbers are about a decoder that is right: both hold the host's blocks
    assert np.array_equal(pcoef[:int(pblocks[0])].cpu().numpy(), want) and np.array_equal(scoef[:int(pblocks[0])].cpu().numpy(), want)
    return {'files': 128, 'stages': stages, 'scans': scans,
            'progressive_stage_launches_ms': {'median': round(p_med, 3), 'best': round(p_best, 3)},
            'sequential_twins_selfsync_1024_ms': {'median': round(s_med, 3), 'best': round(s_best, 3)},
            'progressive_over_sequential': round(p_med / s_med, 2),
            'how': 'hip events around the launches on the work stream, coefficient area zeroed and the device idle before each; 7 timed after 1 warm-up'}


def _resave_progressive(path):
    from PIL import Image
    img = Image.open(path)
    img.load()
    img.save(path + '.tmp', format='JPEG', quality=90, progressive=True)
    os.replace(path + '.tmp', path)
    return os.path.getsize(path)


def device_scans_e2e(a):
    """disk -> embeddings, 4 loader workers, bf16 encoders, every file progressive: device route (WITW_JPEG_PROGRESSIVE_DEVICE=1) against
    the host route (WITW_JPEG_PROGRESSIVE=1) and against Pillow in the worker (neither), alternating rounds, medians"""
    import multiprocessing as mp
    import subprocess
    from witw_amd import e2e
    procs = min(16, len(os.sched_getaffinity(0)))
    _csv, n_unique, _size = e2e.make_dataset(a.e2e_dir, a.e2e_pairs, procs=procs)
    names = [os.path.join(a.e2e_dir, '%s_%05d.jpg' % (t, i)) for i in range(n_unique) for t in ('ov', 'su')]
    with mp.get_context('spawn').Pool(procs) as pool:
        sizes = pool.map(_resave_progressive, names, chunksize=8)
    modes = {'device': {'WITW_JPEG_PROGRESSIVE_DEVICE': '1'}, 'host': {'WITW_JPEG_PROGRESSIVE': '1'}, 'pillow': {}}
    runs = {m: [] for m in modes}
    for r in range(a.rounds):
        order = list(modes) if r % 2 == 0 else list(modes)[::-1]
        for mode in order:
            env = dict(os.environ)
            env.pop('WITW_JPEG_PROGRESSIVE', None)
            env.pop('WITW_JPEG_PROGRESSIVE_DEVICE', None)
            env.update(modes[mode])
            fd_path = os.path.join(a.e2e_dir, 'detail_%s_%d.json' % (mode, r))
            cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--mode', 'e2e', '--e2e-pairs', str(a.e2e_pairs), '--workers', '4',
                   '--precision', 'bf16', '--e2e-dir', a.e2e_dir, '--no-decode-scaling', '--detail-out', fd_path]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                raise RuntimeError('bench.py --mode e2e failed (%d): %s' % (p.returncode, p.stderr[-800:]))
            line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1])
            d = json.load(open(fd_path)) if os.path.exists(fd_path) else line
            runs[mode].append({'pairs_per_s': d.get('value', line.get('value')), 'steady_state_pairs_per_s': d.get('steady_state_pairs_per_s')})
            print(mode, r, runs[mode][-1], flush=True)
    med = {m: statistics.median(x['pairs_per_s'] for x in v) for m, v in runs.items()}
    steady = {m: statistics.median(x['steady_state_pairs_per_s'] or 0 for x in v) for m, v in runs.items()}
    return {'what': 'disk -> embeddings (bench.py --mode e2e): %d pairs over %d distinct, overhead 512 x 512 and surface 224 x 224, every file '
                    're-saved progressive (quality 90, mean %d bytes); 4 loader workers, bf16 encoders, batch 128; %d alternating rounds, one '
                    'child process each; medians. device = WITW_JPEG_PROGRESSIVE_DEVICE=1, host = WITW_JPEG_PROGRESSIVE=1 (scans decoded in '
                    'the worker), pillow = neither (the default)' % (a.e2e_pairs, n_unique, int(np.mean(sizes)), a.rounds),
            'pairs_per_s_median': med, 'steady_state_pairs_per_s_median': steady,
            'device_over_host': round(med['device'] / med['host'], 3), 'device_over_pillow': round(med['device'] / med['pillow'], 3), 'rounds': runs}


def device_scans(a):
    out_path = a.out if a.out != os.path.join(ROOT, 'profiles', 'jpeg_progressive.json') else os.path.join(ROOT, 'profiles', 'jpeg_progressive_device.json')
    try:
        out = json.load(open(out_path))
    except (OSError, ValueError):
        out = {}
    out['what'] = ('progressive files with their scans decoded on the device (opt-in, WITW_JPEG_PROGRESSIVE_DEVICE=1): %d files, %d x %d, '
                   'quality %d, 4:2:0, 10 scans each' % (a.files, a.size, a.size, a.quality))
    if a.device_scans == 'worker':
        out[a.key] = device_scans_worker(a)
    elif a.device_scans == 'device':
        out['device'] = device_scans_device(a)
    else:
        out['e2e'] = device_scans_e2e(a)
    for k in ('worker', 'device', 'e2e'):
        out.setdefault(k, 'unmeasured')
    with open(out_path, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--device-scans', choices=['worker', 'device', 'e2e'], default=None,
                    help='the device-scans legs -> profiles/jpeg_progressive_device.json (worker: no GPU; --key names its block)')
    ap.add_argument('--key', default='worker')
    ap.add_argument('--e2e-dir', default=None, metavar='DIR')
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--passes', type=int, default=7)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--quality', type=int, default=88)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_progressive.json'))
    ap.add_argument('--corpus', choices=['progressive', '440'], default='progressive')
    ap.add_argument('--e2e-440', default=None, metavar='DIR')
    ap.add_argument('--e2e-pairs', type=int, default=4096)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    assert a.files >= 64 and a.passes >= 5
    if a.device_scans:
        assert a.device_scans != 'e2e' or a.e2e_dir
        device_scans(a)
        return
    if a.corpus == '440' or a.e2e_440:
        out_path = a.out if a.out != ap.get_default('out') else os.path.join(ROOT, 'profiles', 'jpeg_440.json')
        try:
            out = json.load(open(out_path))
        except (OSError, ValueError):
            out = {}
        if a.e2e_440:
            out['e2e'] = e2e_440(a)
        else:
            out = dict(corpus_440(a), **({'e2e': out['e2e']} if 'e2e' in out else {}))
            try:
                out['cpu'] = next(ln.split(':', 1)[1].strip() for ln in open('/proc/cpuinfo') if ln.startswith('model name'))
            except (OSError, StopIteration):
                pass
        out.setdefault('e2e', 'unmeasured')
        with open(out_path, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
        print(json.dumps(out))
        return
    import torch
    from PIL import Image
    from witw_amd import jpeg
    torch.set_num_threads(1)
    g = np.random.Generator(np.random.Philox(key=[2026, 88]))
    prog, seq = [], []
    for _ in range(a.files):
        img = Image.fromarray(picture(g, a.size, a.size))
        for blobs, kw in ((prog, {'progressive': True}), (seq, {})):
            bio = io.BytesIO()
            img.save(bio, 'JPEG', quality=a.quality, **kw)
            blobs.append(bio.getvalue())
    first = jpeg.open_file(prog[0], progressive=True)
    coef = np.empty((int(first.info[5]), 64), dtype=np.int16)
    qt = np.empty((int(first.info[2]), 64), dtype=np.uint16)

    def ours(blobs):
        for b in blobs:
            if not jpeg.open_file(b, progressive=True).decode_into(coef, qt):
                raise RuntimeError('decode failed')

    def pillow(blobs):
        for b in blobs:
            Image.open(io.BytesIO(b)).load()

    for p, s in zip(prog, seq):                          # the numbers below are about a decoder that is right
        assert np.array_equal(jpeg.read_coef(p, progressive=True).coef, jpeg.read_coef(s).coef)
    res = {}
    for name, fn, blobs in (('progressive_host_entropy_decode', ours, prog), ('progressive_pillow_full_decode', pillow, prog),
                            ('sequential_host_entropy_decode', ours, seq), ('sequential_pillow_full_decode', pillow, seq)):
        med, best = per_file_us(fn, blobs, a.passes)
        res[name] = {'us_per_file_median': round(med, 1), 'us_per_file_best': round(best, 1)}
    ratio = res['progressive_host_entropy_decode']['us_per_file_median'] / res['progressive_pillow_full_decode']['us_per_file_median']
    cpu = ''
    try:
        cpu = next(ln.split(':', 1)[1].strip() for ln in open('/proc/cpuinfo') if ln.startswith('model name'))
    except (OSError, StopIteration):
        pass
    out = {'what': '%d progressive JPEG files, %d x %d, quality %d, 4:2:0, %d scans each; one thread; per file = median over %d passes of '
                   '(pass time / files)' % (a.files, a.size, a.size, a.quality, prog[0].count(b'\xff\xda'), a.passes),
           'mean_file_bytes': {'progressive': int(np.mean([len(b) for b in prog])), 'sequential': int(np.mean([len(b) for b in seq]))},
           'results': res,
           'progressive_host_entropy_decode_over_pillow_full_decode': round(ratio, 3),
           'pillow': Image.__version__ if hasattr(Image, '__version__') else None, 'cpu': cpu}
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
