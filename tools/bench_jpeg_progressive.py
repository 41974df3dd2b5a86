#!/usr/bin/env python
"""What a loader worker pays for a PROGRESSIVE file (host only, one thread): the progressive entropy decoder of libwitw_jpeg.so
(jpeg.open_file(progressive=True) + decode_into: coefficient blocks, the GPU does the rest) against Pillow's whole decode of the same
bytes (what the worker does with the flag off). 512 x 512 images of photographic statistics (tests/golden/gen_jpeg_fixtures.py's
generator), saved progressive at quality 88; per file: the median over the passes of (time of one pass over all files / files).
Writes profiles/jpeg_progressive.json.   python tools/bench_jpeg_progressive.py [--files 64] [--passes 7]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--passes', type=int, default=7)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--quality', type=int, default=88)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_progressive.json'))
    a = ap.parse_args()
    assert a.files >= 64 and a.passes >= 5
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
