"""Issue order of the Winograd K loop of conv3x3_nhwc_f32_kernel (csrc/conv3x3.hip, conv_wino_h2) in the assembly hipcc writes for
gfx950 -- no GPU needed. In the 96-MFMA loop of every instantiation that carries the form:
  * every ds_read_b128 is issued at least 4 of the wave's own MFMAs ahead of the first instruction that reads its result, counted
    around the back edge (4 MFMAs of 32x32x2 f32 hold the matrix pipe 256 cycles, several LDS latencies),
  * s_waitcnt lgkmcnt(0), the full LDS drain, stands only directly before the chunk's s_barrier."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
CONVERTED = ['ILi128ELi1ELb0ELi8ELi0ELi9EE', 'ILi128ELi1ELb0ELi4ELi0ELi9EE', 'ILi128ELi1ELb1ELi8ELi0ELi9EE',
             'ILi128ELi1ELb1ELi4ELi0ELi9EE', 'ILi64ELi1ELb1ELi8ELi0ELi9EE', 'ILi64ELi1ELb1ELi4ELi0ELi9EE']
MIN_MFMAS_AHEAD = 4
# instructions whose first operand is a source too (no register result)
NO_DEST = ('ds_write', 'ds_store', 'buffer_store', 'global_store', 'flat_store', 'scratch_store', 'v_cmp', 'v_cmpx', 's_')


@pytest.fixture(scope='module')
def listing(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    out = str(tmp_path_factory.mktemp('isa') / 'conv3x3.s')
    src = os.path.join(ROOT, 'witw_amd', 'csrc', 'conv3x3.hip')
    sys.path.insert(0, ROOT)
    from witw_amd import build
    flags = [f for f in build.FLAGS if f not in ('-fPIC',)]
    subprocess.check_call([HIPCC] + flags + ['--cuda-device-only', '-S', '-o', out, src], stderr=subprocess.DEVNULL)
    return open(out).read()


def _body(text, inst):
    m = re.search(r'^(_ZN\S*conv3x3_nhwc_f32_kernel%s\S*):.*?\.Lfunc_end' % inst, text, re.S | re.M)
    assert m, inst
    return m.group(0).splitlines()


def _loops(lines):
    """bodies (header label .. backward branch) of the loops that issue MFMAs"""
    labels = {l.split(':')[0]: i for i, l in enumerate(lines) if re.match(r'^\.LBB\d+_\d+:', l)}
    out = []
    for i, l in enumerate(lines):
        m = re.match(r'\s*s_(?:c)?branch\w*\s+(\.LBB\d+_\d+)', l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            body = lines[labels[m.group(1)]:i + 1]
            if any(b.strip().startswith('v_mfma') for b in body):
                out.append(body)
    return out


def _vregs(operand):
    """architectural VGPRs an operand names"""
    regs = set()
    for a, b in re.findall(r'(?<![\w\]])v\[(\d+):(\d+)\]', operand):
        regs.update(range(int(a), int(b) + 1))
    regs.update(int(a) for a in re.findall(r'(?<![\w\[])v(\d+)\b', operand))
    return regs


def _instructions(body):
    """(mnemonic, registers written, registers read) of every instruction of a loop body, in order"""
    out = []
    for line in body:
        line = line.split(';')[0].strip()
        if not line or line.endswith(':') or line.startswith('.'):
            continue
        mnem, _, rest = line.partition(' ')
        ops = [o.strip() for o in rest.split(',')] if rest.strip() else []
        if mnem.startswith(NO_DEST) or not ops:
            dst, srcs = set(), ops
        else:
            dst, srcs = _vregs(ops[0]), ops[1:]
        out.append((mnem, dst, set().union(*[_vregs(o) for o in srcs]) if srcs else set(), line))
    return out


def _winograd_loop(listing, inst):
    loops = [b for b in _loops(_body(listing, inst)) if sum(1 for l in b if l.strip().startswith('v_mfma')) == 96]
    assert loops, 'no 96-MFMA Winograd K loop in %s' % inst
    return _instructions(min(loops, key=len))


def read_distances(ins):
    """for every ds_read_b128 of the loop: (line, MFMAs issued between it and the first reader of its result, around the back edge)"""
    out = []
    n = len(ins)
    for i, (mnem, dst, _, line) in enumerate(ins):
        if not mnem.startswith('ds_read_b128'):
            continue
        live, mfmas, found = set(dst), 0, False
        for k in range(1, n + 1):
            m2, d2, s2, _ = ins[(i + k) % n]
            if s2 & live:
                found = True
                break
            live -= d2                      # overwritten before any use: that part of the result is dead
            if not live:
                break
            if m2.startswith('v_mfma'):
                mfmas += 1
        if found:
            out.append((line, mfmas))
    return out


@pytest.mark.parametrize('inst', CONVERTED)
def test_fragment_reads_run_ahead_of_their_consumers(listing, inst):
    dist = read_distances(_winograd_loop(listing, inst))
    assert len(dist) >= 36, (inst, len(dist))         # 24 input-row and 12 filter fragments per K chunk
    print(inst, 'MFMAs between a ds_read_b128 and its first reader:', sorted(d for _, d in dist))
    late = [(l, d) for l, d in dist if d < MIN_MFMAS_AHEAD]
    assert not late, (inst, late)


@pytest.mark.parametrize('inst', CONVERTED)
def test_full_lds_drain_only_at_the_barrier(listing, inst):
    ins = _winograd_loop(listing, inst)
    assert sum(1 for m, _, _, _ in ins if m == 's_barrier') == 1, inst
    drains = [i for i, (m, _, _, l) in enumerate(ins) if m == 's_waitcnt' and re.search(r'lgkmcnt\(0\)', l)]
    print(inst, 'full LDS drains in the loop:', len(drains))
    stray = [ins[i][3] + ' -> ' + ins[i + 1][3] for i in drains if i + 1 >= len(ins) or ins[i + 1][0] != 's_barrier']
    assert not stray, (inst, stray)
