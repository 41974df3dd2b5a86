"""Code-generation properties of the Winograd F(2,3)-along-H form of conv3x3_nhwc_f32_kernel (csrc/conv3x3.hip, conv_wino_h2), on
the assembly hipcc writes for gfx950 -- no GPU needed. Every instantiation that carries the form (<128,1,*,*,0,9>, <64,1,true,*,0,9>):
  * spills no register and stays within 256 VGPRs (two waves per SIMD),
  * its Winograd K loop (96 MFMAs per K chunk) holds the 96 input-transform instructions as single v_add_f32 / v_sub_f32 and no
    packed f32 VALU (v_pk_add_f32 / v_pk_mul_f32 beside MFMAs cost issue cycles the single forms do not)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
CONVERTED = ['ILi128ELi1ELb0ELi8ELi0ELi9EE', 'ILi128ELi1ELb0ELi4ELi0ELi9EE', 'ILi128ELi1ELb1ELi8ELi0ELi9EE',
             'ILi128ELi1ELb1ELi4ELi0ELi9EE', 'ILi64ELi1ELb1ELi8ELi0ELi9EE', 'ILi64ELi1ELb1ELi4ELi0ELi9EE']


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


def _meta(text, inst):
    """kernel metadata entry (amdhsa.kernels) of one instantiation -> {key: int}"""
    for entry in re.split(r'\n  - (?=\.agpr_count:)', text[text.index('amdhsa.kernels:'):]):    # entries: keys in alphabetical order
        if re.search(r'\.name:\s+\S*conv3x3_nhwc_f32_kernel%s' % inst, entry):
            return {k: int(v) for k, v in re.findall(r'^\s*\.(\w+):\s+(\d+)\s*$', entry, re.M)}
    raise AssertionError('no metadata for %s' % inst)


@pytest.mark.parametrize('inst', CONVERTED)
def test_converted_instantiations_fit_two_waves_per_simd_without_spills(listing, inst):
    m = _meta(listing, inst)
    assert m['vgpr_spill_count'] == 0, (inst, m)
    # .vgpr_count counts the unified file (architectural VGPRs, then AGPRs); the 4-wave forms may use AGPRs (one wave per SIMD)
    assert m['vgpr_count'] - m.get('agpr_count', 0) <= 256, (inst, m)
    if 'ELi8ELi0' in inst:
        assert m['vgpr_count'] <= 256, (inst, m)


@pytest.mark.parametrize('inst', CONVERTED)
def test_winograd_loop_transforms_with_single_f32_adds(listing, inst):
    loops = [b for b in _loops(_body(listing, inst)) if sum(1 for l in b if l.strip().startswith('v_mfma')) == 96]
    assert loops, 'no 96-MFMA Winograd K loop in %s' % inst
    body = min(loops, key=len)
    assert not [l for l in body if re.match(r'\s*v_pk_(add|mul|fma)_f32', l)], inst
    assert sum(1 for l in body if re.match(r'\s*v_(add|sub|subrev)_f32', l)) >= 96, inst
