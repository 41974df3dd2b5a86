"""tests/conv_epilogue_ref.py against torch in float64, and the proof that its data can tell a wrong kernel from a right one: for
every case of the table, caps on magnitudes and shares (stated, not measured), and a list of deliberately wrong variants -- each a
bug a kernel could have while a training loss still falls -- that must change the expected output of every case they apply to.

Dropout2d scale against activation order is not in the list on purpose: both scales are >= 0 and ReLU / LeakyReLU are positively
homogeneous, so the order does not change a value (tests/conv_epilogue_ref.py)."""
import numpy as np
import pytest
import torch

from oracle import cvig_fov_oracle as O
from tests import conv_epilogue_ref as R

IDS = [c.id for c in R.CASES]


def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def _sel(c, a):
    d = R.case_data(c)
    return a if d.sel is None else a[list(d.sel)]


def _same(a, b):
    """equal as fp32 bit patterns (tells -0.0 from +0.0)"""
    return np.array_equal(R.f32_bits(a), R.f32_bits(b))


def _torch_epilogue(z, c, d):
    if d.drop is not None:
        z = z * _t(_sel(c, d.drop))[:, :, None, None]
    if c.act == 'relu':
        z = torch.where(z > 0, z, torch.zeros_like(z))
    elif c.act == 'lrelu':
        z = torch.nn.functional.leaky_relu(z, R.SLOPE)
    if d.post_scale is not None:
        z = z * _t(d.post_scale)[None, :, None, None] + _t(d.post_shift)[None, :, None, None]
    return z


@pytest.mark.parametrize('c', R.CASES, ids=IDS)
def test_reference_equals_torch_float64(c):
    d = R.case_data(c)
    x = _sel(c, d.x)
    if c.site == 'dgrad':
        xin = torch.zeros((x.shape[0], c.cout, c.H, c.W), dtype=torch.float64, requires_grad=True)
        O.conv3x3(xin, _t(d.w), None, c.sh, c.circ).backward(_t(x))
        assert np.array_equal(xin.grad.numpy(), d.z) and np.array_equal(d.z, np.rint(d.z))
        # the identity the kernels use: a stride-1 conv of the zero-interleaved gradient with the transposed, rotated filter
        assert np.array_equal(_identity(c, d), d.z)
        z = xin.grad
    else:
        w = R.flipped(d.w) if c.site == 'tflip' else d.w
        z = O.conv3x3(_t(x), _t(w), None if d.b is None else _t(d.b), c.sh, c.circ)
        assert np.array_equal(z.numpy(), d.z)
    assert _same(_torch_epilogue(z, c, d).numpy(), d.ungated)


def _interleaved(c, dz, odd=False, last_live=False):
    if c.sh == 1:
        return dz
    xi = np.zeros(dz.shape[:2] + (c.H, c.W))
    if odd:
        n = len(range(1, c.H, 2))
        xi[:, :, 1::2] = dz[:, :, :n]
    else:
        xi[:, :, ::2] = dz
        if last_live:
            xi[:, :, -1] = dz[:, :, (c.H - 1) >> 1]
    return xi


def _identity(c, d, filt=None, **kw):
    return R.conv(_interleaved(c, _sel(c, d.x), **kw), R.flipped(d.w) if filt is None else filt, None, 1, c.circ)


@pytest.mark.parametrize('c', R.CASES, ids=IDS)
def test_caps(c):
    d = R.case_data(c)
    stages = [d.x, d.w, d.z, d.ungated, d.want] + [t for t in (d.b, d.drop, d.post_scale, d.post_shift) if t is not None]
    if d.drop is not None:
        stages.append(d.z * _sel(c, d.drop)[:, :, None, None])
        for row in d.drop:
            assert (row == 0).any() and (row == R.KEEP).any() and set(np.unique(row)) <= {0.0, R.KEEP}
    for t in stages:
        assert float(np.abs(t).max()) <= R.CAP and R.is_f32(t)
    if c.prec == 'f16':
        assert float(np.abs(d.want).max()) <= 65504.0
    if c.site != 'dgrad' and c.act != 'none':
        pre = d.z if d.drop is None else d.z * _sel(c, d.drop)[:, :, None, None]
        assert (pre < 0).mean() >= 0.20 and (pre > 0).mean() >= 0.20
    if c.gate:
        k = d.gate_kind
        opened = d.gate > 0
        assert np.array_equal(opened, np.isin(k, R.GATE_OPEN))
        assert opened.mean() >= 0.25 and (~opened).mean() >= 0.25
        closed = float((~opened).sum())
        kinds = R.gate_kinds(c.prec)
        assert np.isposinf(d.gate[k == 7]).all()
        for q in (3, 4, 5):
            assert (k == q).sum() >= 0.05 * closed, R.GATE_KINDS[q]
        assert np.array_equal(np.signbit(d.gate[k == 5]), np.ones(int((k == 5).sum()), dtype=bool))
        assert not np.signbit(d.gate[k == 4]).any()
        normal, sub = R.GATE_FORMATS[c.prec]
        assert (d.gate[k == 1] == normal).all() and (d.gate[k == 2] == sub).all() and normal > 0 and sub > 0
        for q in kinds:
            assert ((k == q) & (d.ungated != 0)).any(), 'no %s gate over a non-zero output' % R.GATE_KINDS[q]
        # the gate survives its own encoding
        if c.prec == 'bf16':
            assert np.array_equal(R.bf16_bits(d.gate).view(np.uint16).astype(np.uint32) << 16, R.f32_bits(d.gate).view(np.uint32))
        elif c.prec == 'f16':
            s = R.split_bits(d.gate.transpose(0, 2, 3, 1))
            hi, lo = s[..., 0, :].view(np.float16).astype(np.float64), s[..., 1, :].view(np.float16).astype(np.float64)
            assert np.array_equal((hi + lo).reshape(d.gate.transpose(0, 2, 3, 1).shape), d.gate.transpose(0, 2, 3, 1))
            assert np.array_equal(hi > 0, (hi + lo) > 0) and not lo[np.isinf(hi)].any() and (lo[hi > 0] < 0).any() and (lo[hi < 0] > 0).any()
            assert not ((hi == 0) & (lo != 0)).any()
        else:
            assert np.isnan(d.gate[k == 6]).all()


def _wrong_variants(c, d):
    """(name, output) of every wrong variant that applies to the case"""
    out = []
    x = _sel(c, d.x)
    drop = None if d.drop is None else _sel(c, d.drop)

    def finish(z, gate=d.gate, select=True, dr=drop, affine_first=False):
        if affine_first:
            v = z if dr is None else z * dr[:, :, None, None]
            v = v * d.post_scale[None, :, None, None] + d.post_shift[None, :, None, None]
            v = R.relu(v) if c.act == 'relu' else R.lrelu(v, R.SLOPE)
        else:
            v = R.epilogue(z, dr, c.act, R.SLOPE, d.post_scale, d.post_shift)
        if gate is None:
            return v
        with np.errstate(invalid='ignore'):
            return R.gate_select(v, gate) if select else v * (gate > 0)

    if c.site != 'dgrad':
        w = R.flipped(d.w) if c.site == 'tflip' else d.w
        if c.drop and d.b is not None:
            zb = R.conv(x, w, None, c.sh, c.circ) * drop[:, :, None, None] + d.b[None, :, None, None]
            out.append(('bias after the Dropout2d scale', finish(zb, dr=None)))
        if c.post and c.act != 'none':
            out.append(('affine before the activation', finish(d.z, affine_first=True)))
        out.append(('circular wrap and zero padding exchanged', finish(R.conv(x, w, d.b, c.sh, not c.circ))))
        if c.sh == 2 and c.H > 1:
            up = np.concatenate([x[:, :, 1:], np.zeros_like(x[:, :, :1])], axis=2)
            out.append(('stride-2 row origin off by one', finish(R.conv(up, w, d.b, 2, c.circ))))
        if c.site == 'tflip':
            out.append(('filter transposed but not rotated', finish(R.conv(x, d.w.transpose(1, 0, 2, 3), None, c.sh, c.circ))))
            if c.cin == c.cout:
                out.append(('filter rotated but not transposed', finish(R.conv(x, d.w[:, :, ::-1, ::-1], None, c.sh, c.circ))))
    else:
        out.append(('circular wrap and zero padding exchanged', finish(R.dgrad(x, d.w, (c.H, c.W), c.sh, not c.circ))))
        if c.H * c.W > 1:      # on a 1 x 1 map only the centre row's taps count and (wrapped) they all meet the same pixel: a rotation is invisible
            out.append(('filter transposed but not rotated', finish(_identity(c, d, filt=d.w.transpose(1, 0, 2, 3)))))
        if c.cin == c.cout:
            out.append(('filter rotated but not transposed', finish(_identity(c, d, filt=d.w[:, :, ::-1, ::-1]))))
        if c.sh == 2:
            out.append(('interleaved rows on odd rows', finish(_identity(c, d, odd=True))))
            if c.H % 2 == 0:
                out.append(('the last row of an even out_h treated as live', finish(_identity(c, d, last_live=True))))
    if c.gate:
        g = d.gate
        if (d.ungated < 0).any():
            out.append(('gate as a multiplication by (gate > 0)', finish(d.z, select=False)))
        B, C, H, W = g.shape
        if H * W == 1:
            pass                   # one pixel: both layouts are the same offsets
        elif c.store == 'nchw':    # the buffer is NCHW; read with NHWC offsets
            out.append(('gate indexed NHWC under an NCHW output', finish(d.z, gate=g.reshape(B, H, W, C).transpose(0, 3, 1, 2))))
        else:                      # the buffer is NHWC; read with NCHW offsets
            buf = np.ascontiguousarray(g.transpose(0, 2, 3, 1))
            out.append(('gate indexed NCHW under an NHWC output', finish(d.z, gate=buf.reshape(B, C, H, W))))
        if W > 1:
            out.append(('gate shifted by one pixel in x', finish(d.z, gate=np.roll(g, 1, axis=3))))
        out.append(('gate shifted by one channel', finish(d.z, gate=np.roll(g, 1, axis=1))))
    return out


@pytest.mark.parametrize('c', R.CASES, ids=IDS)
def test_wrong_variants_change_the_answer(c):
    d = R.case_data(c)
    names = []
    for name, alt in _wrong_variants(c, d):
        assert alt.shape == d.want.shape
        assert not _same(alt, d.want), name
        names.append(name)
    assert 'circular wrap and zero padding exchanged' in names


def test_every_wrong_variant_is_applied_somewhere():
    seen = set()
    for c in R.CASES:
        if c.big:
            continue
        seen.update(n for n, _a in _wrong_variants(c, R.case_data(c)))
    assert len(seen) == 13, sorted(seen)


def test_table_names_every_instantiation():
    """13 fp32, 8 tiled bf16 + the 16x16x32 training form + the gated weight-resident one, 8 split-fp16; every fp32 (instantiation, store) pair with and without a gate"""
    names = {c.variant() for c in R.CASES}
    f32 = {'conv3x3_nhwc_f32_kernel<%d,%d,false,%d,%d,9>' % (tn, sh, nw, geo)
           for tn in (64, 128) for sh in (1, 2) for nw, geo in ((4, 0), (8, 0), (4, 1))} | {'conv3x3_nhwc_f32_kernel<128,1,false,8,2,9>'}
    low = {'%s<%d,%d,false,%d>' % (k, tn, sh, nw) for k in ('conv3x3_nhwc_bf16_kernel', 'conv3x3_nhwc_f16x3_kernel')
           for tn in (64, 128) for sh in (1, 2) for nw in (4, 8)}
    assert names == f32 | low | {'conv3x3_bf16_s16_kernel<false,true>', 'conv3x3_bf16_wres_kernel<gate>'}
    pairs = {(c.variant(), c.store, c.gate) for c in R.CASES if c.prec == 'f32'}
    for v in f32 - {'conv3x3_nhwc_f32_kernel<128,1,false,8,2,9>'}:
        for store in ('slab', 'generic', 'nchw'):
            for gate in (False, True):
                assert (v, store, gate) in pairs, (v, store, gate)
    for c in R.CASES:
        assert (c.store == 'generic') == (c.prec == 'f32' and c.store != 'nchw' and c.cout % 4 != 0)
    assert len(R.CASES) <= 205


def test_encoders():
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.0, 0.0, 160.0, 2049.0, 2.0 ** -133, 1.0 + 2.0 ** -12, -(1.0 - 2.0 ** -13),
                  2.0 ** -25, 2.0 ** -24, 0.125, 31.96875, 255.5, -319.0], dtype=np.float64)
    assert np.array_equal(R.bf16_bits(v), torch.from_numpy(v.astype(np.float32)).bfloat16().view(torch.int16).numpy())      # torch rounds to nearest even too
    assert R.bf16_bits(np.array([1.0 + 2.0 ** -8]))[0] == 0x3f80 and R.bf16_bits(np.array([1.0 + 3 * 2.0 ** -8]))[0] == 0x3f82      # ties to even
    s = R.split_bits(v)
    hi, lo = s[:, 0, :].view(np.float16).astype(np.float64).ravel(), s[:, 1, :].view(np.float16).astype(np.float64).ravel()
    assert np.array_equal(hi, v.astype(np.float16).astype(np.float64))
    exact = np.abs(v - (hi + lo).ravel()) == 0
    assert exact[[0, 3, 4, 5, 6, 8, 9, 11, 13, 14, 15]].all()
    assert s[0, 0, 3] == np.int16(-0x8000) and s[0, 1, 3] == 0 and s[1, 0, 2] == 0 and s[1, 1, 2] == 0      # -0.0 keeps its sign in hi; 2^-25 is zero in both
    assert np.array_equal(R.f32_bits(np.array([-0.0, 0.0, np.inf])), np.array([-2 ** 31, 0, 0x7f800000], dtype=np.int64).astype(np.int32))
