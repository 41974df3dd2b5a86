"""The host JPEG decoder with its progressive part (csrc_host/jpeg_coef.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer, as
a stand-alone program (tools/jpeg_prog_check.cpp: file bytes, coefficient area and tables in heap blocks of exactly their size): the
clean files of tests/test_jpeg_progressive.py, every truncation of one small progressive file and 2,000 single-byte corruptions of it
must run through without a report. Nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from . import jpeg_prog_craft as PC
from .test_jpeg_progressive import crafted_cases, flat_blocks_file, picture, save, source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_progressive_decoder_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    gxx = shutil.which('g++')
    if not gxx:
        pytest.skip('no g++ on this box')
    exe = str(tmp_path / 'jpeg_prog_check')
    # the runtimes are linked statically: the program does not depend on the order in which shared libraries get loaded
    build = subprocess.run([gxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                            '-static-libasan', '-static-libubsan', '-o', exe,
                            os.path.join(ROOT, 'witw_amd', 'csrc_host', 'jpeg_coef.cpp'), os.path.join(ROOT, 'tools', 'jpeg_prog_check.cpp')],
                           capture_output=True, text=True)
    if build.returncode != 0:
        if 'asan' in build.stderr or 'ubsan' in build.stderr or 'sanitize' in build.stderr:
            pytest.skip('this compiler cannot link the sanitizer runtimes')
        raise AssertionError(build.stderr[-3000:])
    clean, damaged = [], []

    def put(group, name, data):
        path = str(tmp_path / name)
        with open(path, 'wb') as f:
            f.write(data)
        group.append(path)

    for sampling in ('grey', '444', '422', '420'):
        for (h, w) in ((8, 8), (17, 9), (40, 56), (64, 64)):
            put(clean, 'twin_%s_%dx%d.jpg' % (sampling, h, w), save(picture(h * 100 + w, h, w, grey=sampling == 'grey'), sampling, 95, progressive=True))
    for name, sampling, size, script, kw in crafted_cases():
        _seq, src = source(sampling, size[0], size[1], **kw)
        put(clean, name + '.jpg', PC.write(size[0], size[1], src.coef, src.qt, sampling, script))
    put(clean, 'flat.jpg', flat_blocks_file()[2])
    small = save(picture(1709, 17, 9), '420', 90, progressive=True)
    for n in range(len(small)):
        put(damaged, 'cut_%04d.jpg' % n, small[:n])
    g = np.random.Generator(np.random.Philox(key=[31, 2000]))
    for k in range(2000):
        b = bytearray(small)
        b[int(g.integers(0, len(b)))] = int(g.integers(0, 256))
        put(damaged, 'flip_%04d.jpg' % k, bytes(b))
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    p = subprocess.run([exe] + clean + damaged, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and 'Sanitizer' not in p.stderr and 'runtime error' not in p.stderr, (p.returncode, p.stderr[-3000:])
    lines = p.stdout.splitlines()
    assert len(lines) == len(clean) + len(damaged)
    assert all(ln.startswith('1 0 ') for ln in lines[:len(clean)]), [ln for ln in lines[:len(clean)] if not ln.startswith('1 0 ')]
    # the damaged ones: every cut is refused; most flips are noticed, none goes unanswered
    cuts = lines[len(clean):len(clean) + len(small)]
    assert all(ln.split()[0] == '-1' or ln.split()[1] == '-3' for ln in cuts), [ln for ln in cuts if ln.split()[1] not in ('-', '-3')][:5]
    assert all(ln.split()[0] in ('-2', '-1', '0', '1') for ln in lines[len(clean):])
