"""Build libwitw_hip.so (the C-ABI shared library) in-tree with hipcc for gfx950.

hipcc cross-compiles without a GPU; the built .so travels to the GPU box with the repo
snapshot (it is git-ignored, not gpurun-ignored).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libwitw_hip.so')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-fPIC', '-std=c++17', '-ffp-contract=off', '-Wall', '-Wno-unused-function']


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.hip'))


def stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = sources() + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h')]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    """Compile and link; serialised across processes with a file lock (N ranks may import at once)."""
    if not force and not stale():
        return LIB
    import fcntl
    os.makedirs(os.path.join(HERE, 'build'), exist_ok=True)
    with open(os.path.join(HERE, 'build', '.lock'), 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and not stale():      # another process built it while we waited
                return LIB
            return _build_locked(verbose)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


# Three kernels issue their LDS fragment reads by hand (asm volatile ds_read_b128 + counted s_waitcnt lgkmcnt): they are correct only
# while the compiler keeps every fragment register untouched between a read and its wait. That was validated (parity tests + fuzz
# against the oracle) for the register allocations below; a compiler that allocates differently gets the slower, compiler-scheduled
# kernels instead until the parity tests have been re-run and the table updated. Each guard: the kernel-resource-usage remarks of
# `kernel`'s instantiations (mangled template arguments -> (VGPRs, spilled VGPRs, scratch bytes per lane) under hipcc of ROCm 7.2.0)
# are compared with `table` after every compile; a mismatch leaves `marker`, which _lib.load() reads AFTER the build (so a process
# that triggers the build itself is covered) and reports through _lib.guards() / the bench line's `guards` field.
#   s16:    conv3x3_bf16_s16_kernel<POOL, TRAIN> -> the 32x32x16 kernel (witw_conv3x3_bf16_mfma16(0));      force: WITW_BF_S16=1
#   wres:   conv3x3_bf16_wres_kernel<REC, GATE>  -> layer 5 on the tiled kernels (witw_conv3x3_bf16_wres(0)); force: WITW_BF_WRES=1
#   first2: conv_first2_bf16_kernel<CW, REC, TRAIN> -> layers 0 and 2 as two launches (FOV_DSM.fuse_first2); force: WITW_F2=1
S16_VALIDATED = {'ILb0ELb0EE': (256, 10, 44), 'ILb1ELb0EE': (256, 1, 8), 'ILb0ELb1EE': (256, 10, 44), 'ILb1ELb1EE': (256, 2, 12)}
S16_MARKER = os.path.join(HERE, 'build', 's16_unvalidated')
WRES_VALIDATED = {'ILb0ELi0EE': (209, 0, 0), 'ILb0ELi1EE': (229, 0, 0),      # <REC, GATE>: plain forward; gated (dgrad) form, round 5;
                  'ILb0ELi2EE': (221, 0, 0)}                                # gate as one bit per output (round 6)
WRES_MARKER = os.path.join(HERE, 'build', 'wres_unvalidated')
F2_VALIDATED = {'ILi4ELb0ELb0EE': (254, 0, 0), 'ILi8ELb0ELb0EE': (256, 0, 0),      # <CW, REC, TRAIN>: the two inference forms;
                'ILi8ELb0ELb1EE': (256, 0, 0)}                                     # the training form of cvig_semantic (round 6)
F2_MARKER = os.path.join(HERE, 'build', 'first2_unvalidated')


def _check_table(remarks, kernel, table, marker, consequence):
    """kernel-resource-usage remarks of `kernel`'s instantiations against `table`; writes / clears `marker`"""
    import re
    found, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r'Function Name: \S*%s(IL\w+?)EvNS' % kernel, line)
        if m:
            cur = m.group(1)
            found[cur] = {}
            continue
        if 'Function Name:' in line:
            cur = None
        if cur is None:
            continue
        for key, pat in (('vgprs', r' VGPRs: (\d+)'), ('spill', r'VGPRs Spill: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)')):
            m = re.search(pat, line)
            if m:
                found[cur][key] = int(m.group(1))
    bad = []
    for inst, want in table.items():
        got = found.get(inst)
        if not got or (got.get('vgprs'), got.get('spill'), got.get('scratch')) != want:
            bad.append('%s: validated %s, this compiler %s' % (inst, want, got))
    if bad:
        with open(marker, 'w') as f:
            f.write('\n'.join(bad) + '\n')
        print('WARNING: %s compiled with a register allocation that has not been validated; %s (see witw_amd/build.py):\n  %s'
              % (kernel, consequence, '\n  '.join(bad)), flush=True)
    elif os.path.exists(marker):
        os.remove(marker)


def _check_s16(remarks):
    _check_table(remarks, 'conv3x3_bf16_s16_kernel', S16_VALIDATED, S16_MARKER, 'the 32x32x16 bf16 kernel is used instead')


def _check_wres(remarks):
    _check_table(remarks, 'conv3x3_bf16_wres_kernel', WRES_VALIDATED, WRES_MARKER, 'layer 5 runs on the tiled kernels instead')


def _check_first2(remarks):
    _check_table(remarks, 'conv_first2_bf16_kernel', F2_VALIDATED, F2_MARKER, 'layers 0 and 2 run as two launches instead')


CHECKED = {'conv3x3_bf16.hip': lambda r: _check_s16(r), 'conv3x3_bf16_wres.hip': lambda r: _check_wres(r),
           'conv_first2_bf16.hip': lambda r: _check_first2(r)}


def guard_markers():
    """name -> (marker path, environment variable that forces the hand-scheduled kernel); read at call time (tests repoint them)"""
    return {'s16': (S16_MARKER, 'WITW_BF_S16'), 'wres': (WRES_MARKER, 'WITW_BF_WRES'), 'first2': (F2_MARKER, 'WITW_F2')}


def _build_locked(verbose):
    objs = []
    procs = []
    os.makedirs(os.path.join(HERE, 'build'), exist_ok=True)
    for src in sources():
        obj = os.path.join(HERE, 'build', os.path.basename(src)[:-4] + '.o')
        objs.append(obj)
        cmd = [HIPCC] + FLAGS + ['-c', src, '-o', obj]
        checked = CHECKED.get(os.path.basename(src))
        if checked:
            cmd.insert(-4, '-Rpass-analysis=kernel-resource-usage')
        if verbose:
            print(' '.join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd, stderr=subprocess.PIPE if checked else None, text=True if checked else None), checked))
    for cmd, p, checked in procs:
        err = p.communicate()[1] if checked else None
        if p.wait() != 0:
            if err:
                sys.stderr.write(err)
            raise RuntimeError('hipcc failed: ' + ' '.join(cmd))
        if checked:
            checked(err or '')
    tmp = LIB + '.tmp.%d' % os.getpid()
    cmd = [HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', tmp] + objs
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(tmp, LIB)                       # atomic: a concurrent dlopen never sees a half-written file
    return LIB


HOST_SRC = os.path.join(HERE, 'csrc_host', 'jpeg_coef.cpp')
HOST_DEPS = [HOST_SRC, os.path.join(CSRC, 'jpeg_layout.h')]      # the plan / info layouts, shared with csrc/jpeg.hip
HOST_LIB = os.path.join(HERE, 'libwitw_jpeg.so')


def host_stale():
    return not os.path.exists(HOST_LIB) or any(os.path.getmtime(d) > os.path.getmtime(HOST_LIB) for d in HOST_DEPS)


def build_host(force=False, verbose=True):
    """libwitw_jpeg.so: the host-only part of the data path (JPEG entropy decoding, csrc_host/jpeg_coef.cpp), plain g++ --
    DataLoader workers load it without ever mapping the HIP runtime."""
    if not force and not host_stale():
        return HOST_LIB
    import fcntl
    os.makedirs(os.path.join(HERE, 'build'), exist_ok=True)
    with open(os.path.join(HERE, 'build', '.lock_host'), 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if force or host_stale():
                tmp = HOST_LIB + '.tmp.%d' % os.getpid()
                cmd = [os.environ.get('CXX', 'g++'), '-O3', '-fPIC', '-shared', '-std=c++17', '-Wall', '-o', tmp, HOST_SRC]
                if verbose:
                    print(' '.join(cmd), flush=True)
                subprocess.check_call(cmd)
                os.replace(tmp, HOST_LIB)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return HOST_LIB


if __name__ == '__main__':
    build(force='--force' in sys.argv)
    build_host(force='--force' in sys.argv)
    print(LIB)
    print(HOST_LIB)
