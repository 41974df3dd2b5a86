"""tests/first_layer_ref.py against torch in float64, and the proof that its data can tell a wrong first-layer kernel from a right
one. Conditions held on every case (stated, not measured; a case that misses one is given other data, never another threshold):

    every expected value is its own fp32 rounding (bf16 rows: the value before the store)
    with ReLU, 30 % .. 70 % of the outputs are > 0
    dyadic:  lo != 0 on >= 30 % of the outputs, with and without the ReLU
    round16: >= 25 % of the non-zero operands change under rounding to bf16, each of the four factors occurs
    each wrong variant of first_layer_ref.VARIANT_NAMES changes the expected bits of every case it applies to

test_report_of_measured_shares prints, per case family, the extremes of the measured shares next to these caps (pytest -s). Measured
over the table: positive share 0.31 .. 0.62; dyadic lo != 0 >= 0.32 under the ReLU, >= 0.61 without; round16 operands changed 1.00 (every
factor moves under rounding).

A batch that fills the chip (rows 'persist', 'edge') is looked at through its first two images: the images are drawn independently."""
import functools

import numpy as np
import pytest
import torch

from tests import conv_epilogue_ref as E
from tests import first_layer_ref as R
from tests import pool_ref as P

IDS = [k.id for k in R.KEYS]


@functools.lru_cache(maxsize=None)
def _d(k):
    return R.data(k, R.NOMINAL_CU, 2)          # two images of each case: small enough to keep


def _torch_conv(x, w, b, circ):
    t = torch.from_numpy(np.array(x, dtype=np.float64))
    t = torch.nn.functional.pad(t, (0, 0, 1, 1))
    t = torch.nn.functional.pad(t, (1, 1, 0, 0), mode='circular' if circ else 'constant')
    return torch.nn.functional.conv2d(t, torch.from_numpy(np.array(w, dtype=np.float64)), torch.from_numpy(np.array(b, dtype=np.float64))).numpy()


@pytest.mark.parametrize('k', R.KEYS, ids=IDS)
def test_reference_equals_torch_float64(k):
    d = _d(k)
    xr = d.xr if d.sel is None else d.xr[list(d.sel)]
    assert np.array_equal(_torch_conv(xr, d.wr, d.b, k.circ), d.z)         # exact data: any summation order gives these bits
    if k.row == 'bf16':
        assert np.array_equal(R.round_bf16(R.round_bf16(d.x)), d.xr) and np.array_equal(E.bf16_bits(d.wr).view(np.uint16).astype(np.uint32) << 16,
                                                                                       E.f32_bits(d.wr).view(np.uint32))
    else:
        assert d.xr is d.x and d.wr is d.w


@pytest.mark.parametrize('k', R.KEYS, ids=IDS)
def test_conditions(k):
    d = _d(k)
    assert R.conditions(k, d) == []
    assert E.is_f32(d.z) and E.is_f32(R.relu(d.z))
    for t in (d.x, d.w, d.b):
        assert E.is_f32(t)
    if k.data == 'ints':
        for t in (d.x, d.w, d.b, d.z):
            assert np.array_equal(t, np.rint(t))
        if k.row == 'split':
            assert not (R.expected(k, d, True)[..., 1, :] & 0x7fff).any()
    if k.data == 'dyadic':
        assert set(np.unique(np.abs(d.w))) <= {0.0, 1.0, 2.0 ** -12} and np.array_equal(d.x, np.rint(d.x)) and float(np.abs(d.x).max()) <= 8
        assert np.array_equal(d.b * 4096, np.rint(d.b * 4096)) and np.array_equal(d.z * 4096, np.rint(d.z * 4096))
        # the sum of the magnitudes bounds every partial sum, whatever the order
        bound = P.conv3x3(np.abs(d.x[:2]), np.abs(d.w), np.abs(d.b), k.circ)
        assert float(bound.max()) < 2.0 ** 10
    if k.data == 'round16':
        assert set(np.unique(np.abs(d.xr))) <= {0.0, 1.0, 1.0 + 2.0 ** -6} and set(np.unique(np.abs(d.wr))) <= {0.0, 1.0, 1.0 + 2.0 ** -6}
        bound = P.conv3x3(np.abs(d.xr[:2]), np.abs(d.wr), np.abs(d.b), k.circ)
        assert float(bound.max()) < 2.0 ** 7 and np.array_equal(d.z * 4096, np.rint(d.z * 4096))
    if k.big:
        B, tiles = k.batch(), k.tiles if k.row == 'persist' else 4          # 'edge' borrows the batch of (9, 66): 4 tiles an image
        ok = [n for n in range(1, B + 1) if n * tiles >= 4 * R.NOMINAL_CU and (n * tiles) % (2 * R.NOMINAL_CU) != 0]
        assert ok == [B] and d.x.shape[0] == B


@pytest.mark.parametrize('k', R.KEYS, ids=IDS)
def test_wrong_variants_change_the_answer(k):
    d = _d(k)
    assert R.unchanged_variants(k, d) == []
    for on in R.RELUS:
        names = [n for n, _a in R.wrong_variants(k, d, on)]
        assert 'tap pairs (2i, 2i+1) swapped' in names
        assert ('bias added after the ReLU' in names) == on
        assert ('zero padding instead of wrap' in names) == bool(k.circ)
        assert ('channel 3 dropped' in names) == (k.C >= 4)
        assert ('hi and lo swapped' in names) == (k.row == 'split')
        assert ('operands truncated to bf16' in names) == (k.row == 'bf16' and k.data == 'round16')
        assert ('output rounded twice' in names) == (k.row == 'bf16' and k.data == 'round16' and k.H * k.W > 1)


@pytest.mark.parametrize('circ', P.PADS)
@pytest.mark.parametrize('shape', P.FIRST2_SHAPES, ids=lambda s: '%dx%dx%dx%d' % s)
def test_first_two_layers_wrong_variants(shape, circ):
    want_y, want_bits = R.first2_answers(shape, circ)
    c = P.first2_case(*shape, circ)
    mid = P.conv3x3_exact(c.x, c.w0, c.b0, circ)
    assert 0.30 <= float((mid > 0).mean()) <= 0.70
    assert np.array_equal(_torch_conv(c.x, c.w0, c.b0, circ), mid)
    # the byte layout, spelled out once: channel c is bit c & 7 of byte c >> 3
    for ch in (0, 7, 8, 13, 63):
        assert np.array_equal((want_bits[..., ch >> 3] >> (ch & 7)) & 1, (R.nhwc(mid)[..., ch] > 0).astype(np.uint8))
    names = []
    for name, y, bits in R.first2_wrong_variants(shape, circ):
        assert not np.array_equal(bits, want_bits), name
        assert y is None or not np.array_equal(y, want_y), name
        names.append(name)
    assert 'gate bit order reversed' in names and ('channel 3 dropped' in names) == (shape[1] >= 4)


def test_every_wrong_variant_is_applied_somewhere():
    seen = set()
    for k in R.KEYS:
        if not k.big and (k.H, k.W) in ((3, 12), (1, 1)):
            for on in R.RELUS:
                seen.update(n for n, _a in R.wrong_variants(k, _d(k), on))
    seen.update(n for n, _y, _b in R.first2_wrong_variants(P.FIRST2_SHAPES[2], True))
    assert seen == set(R.VARIANT_NAMES)


def test_table_counts():
    """the rows of tests/test_first_layer_gpu.py's table: keys x relu on / off"""
    n = {}
    for k in R.KEYS:
        row = k.row if k.row != 'bf16' else 'bf16<%d>' % (4 if k.C <= 4 else 8)
        n[row] = n.get(row, 0) + len(R.RELUS)
    assert n == {'f32': 192, 'split': 36, 'persist': 64, 'edge': 4, 'bf16<4>': 192, 'bf16<8>': 192}
    assert {k.variant() for k in R.KEYS} == {R.TILE_KERNEL, R.PERSIST_KERNEL, 'conv3x3_first_bf16_kernel<4>', 'conv3x3_first_bf16_kernel<8>'}
    assert R.persist_batch((9, 66), 256) == 257 and R.persist_batch((8, 130), 256) == 342 and R.persist_batch((9, 66), 304) == 305


def test_pack_layouts():
    for C in (1, 3, 4):
        w = R.pack_probe(C)
        f = R.pack_f32(w)
        assert f.shape == (5, 2, 64, 4) and not f[4, 1].any() and not f[..., C:].any()
        assert f[2, 1, 17, C - 1] == w[17, C - 1, 1, 2]                      # tap 5 = (kh 1, kw 2)
        b = R.pack_bf16(w)
        assert b.shape == (3, 2, 64, 8) and not b[2, 0, :, 4:].any() and not b[2, 1].any()      # taps 9, 10, 11
        assert b[1, 1, 5, 4 + C - 1] == w[5, C - 1, 2, 1] and b[2, 0, 5, 0] == w[5, 0, 2, 2]      # taps 7 and 8
    for C in (5, 8):
        w = R.pack_probe(C)
        b = R.pack_bf16(w)
        assert b.shape == (5, 2, 64, 8) and not b[4, 1].any() and not b[..., C:].any() and b[3, 0, 63, 4] == w[63, 4, 2, 0]
    assert np.array_equal(R.round_bf16(np.asarray(R.FACTORS)), [1.0, 1.0, 1.0, 1.0 + 2.0 ** -6])
    assert np.array_equal(R.trunc_bf16(np.asarray(R.FACTORS)), [1.0, 1.0 - 2.0 ** -8, 1.0, 1.0 + 2.0 ** -7])


def test_report_of_measured_shares():
    """per case family, the extremes of the measured shares against the caps (printed; the caps themselves: test_conditions)"""
    fam = {}
    for k in R.KEYS:
        s = R.shares(k, _d(k))
        f = fam.setdefault((k.row, k.data), {'n': 0, 'pos': [1.0, 0.0], 'lo1': 1.0, 'lo0': 1.0, 'chg': 1.0})
        f['n'] += 1
        f['pos'] = [min(f['pos'][0], s['positive']), max(f['pos'][1], s['positive'])]
        if k.data == 'dyadic':
            f['lo1'], f['lo0'] = min(f['lo1'], s['lo_nonzero_relu1']), min(f['lo0'], s['lo_nonzero_relu0'])
        if k.data == 'round16':
            f['chg'] = min(f['chg'], s['operands_changed'])
    for (row, kind), f in sorted(fam.items()):
        line = '%-8s %-8s %3d keys  positive %.3f .. %.3f (cap 0.30 .. 0.70)' % (row, kind, f['n'], f['pos'][0], f['pos'][1])
        if kind == 'dyadic':
            line += '  lo != 0 >= %.3f relu, %.3f plain (cap 0.30)' % (f['lo1'], f['lo0'])
        if kind == 'round16':
            line += '  operands changed >= %.3f (cap 0.25)' % f['chg']
        print(line)
        assert 0.30 <= f['pos'][0] and f['pos'][1] <= 0.70
