"""Edge sweep of the weight-gradient entries against a float64 reference, and the parts of their ABI that witw_amd.ops never uses.

Entries: witw_conv3x3_wgrad, witw_conv3x3_wgrad_taps4 (csrc/conv3x3_wgrad.hip), witw_conv3x3_wgrad_bf16, witw_conv3x3_wgrad_bf16_nhwc
(and its 16x16x32 form; csrc/wgrad_bf16.hip), witw_conv3x3_wgrad_f16x3 (csrc/wgrad_f16x3.hip), called through tests/wgrad_abi.py
with dw, db and a NaN-filled workspace between guard bands.

Every case is chosen for a K-split geometry -- how many splits, how many chunks per split (cps), how many trailing splits whose
chunk range is empty -- and states it; the test first asserts the geometry against the library (the exported split count of the
fp32 entry, the workspace size of the others) and against this module's restatement of the launcher's heuristic, so a change to
the heuristic fails here loudly instead of leaving a case that no longer exercises what it was written for.

Parity. err = max |got - ref| / scale per element, ref and scale in float64 from tests/wgrad_ref.py (scale = the same sum over
absolute values; scale 0 demands an exact 0). The yardstick is the err of fp32 CPU autograd through the oracle's convolution on
the same operands, i.e. the error of ANOTHER fp32 summation order of the same terms. The kernel may have 4 times that (two
fp32 summation orders of the same terms err like independent random walks of similar length; 4 is the margin between two such
walks' maxima), and never less than one fp32 ulp of the scale (2^-23: a sum of one or two terms can be exact on the CPU).
bf16 operands are bf16-exact fp32 values (exact products, so again only the summation order differs). The fp16x3 entry carries
each operand as fp16 hi + fp16 lo (22 significant bits) and drops the lo * lo product; measured on its own, its three cases need
no room for that: the worst is 1.36 ulp of the scale at a ratio of 1.36, so it is held to the same bound as the others.

The parity bounds cannot see a change of summation ORDER in the split-K reduction (they sit 4 x above another order), so
test_reduction_is_the_stated_fp32_order pins it: it reads the partials a launch left in the caller's workspace, adds them on the
CPU in the documented order (csrc/wgrad_common.h) with one fp32 tensor add per partial, and demands the bits of dw and db.

Measured on the MI355X (profiles/wgrad_edges.json, written by tools/wgrad_edge_ratios.py from these cases): see DESIGN.md section 4.3.
"""
import collections
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import cvig_fov_oracle as O
from tests import wgrad_abi as A
from tests import wgrad_ref as R
from tests.mem_arena import Arena, canary_int

pytestmark = pytest.mark.gpu

MARGIN = 4.0                    # kernel err <= MARGIN x the err of fp32 CPU autograd on the same operands ...
FLOOR = R.F32_ULP               # ... and never below one fp32 ulp of the scale

Case = collections.namedtuple('Case', 'entry B H W Cin Cout sh circ cin_real splits cps empty mfma16 acc note')


def _c(entry, B, H, W, Cin, Cout, sh, circ, geom, cin_real=None, mfma16=False, acc=False, note=''):
    return Case(entry, B, H, W, Cin, Cout, sh, bool(circ), cin_real or Cin, geom[0], geom[1], geom[2], mfma16, acc, note)


def case_id(c):
    s = '%s%s-%dx%dx%dx%d-%d-s%d-%s' % (c.entry, '16' if c.mfma16 else '', c.B, c.H, c.W, c.Cin, c.Cout, c.sh, 'circ' if c.circ else 'zero')
    return s + ('-real%d' % c.cin_real if c.cin_real != c.Cin else '')


# ------------------------------------------------------------------------------------------------ the launchers' split heuristics, restated
def cdiv(a, b):
    return -(-a // b)


def mfma16_applies(c):
    return c.mfma16 and c.entry == 'bf16_nhwc' and c.sh == 1 and c.W % 32 == 0 and c.Cin > 32 and c.Cout > 64


def chunks_of(c):
    """K chunks of the case: what one staged step of the entry's kernel covers"""
    Ho = A.out_rows(c.H, c.sh)
    if c.entry in ('f32', 'taps4'):           # one output row x up to 64 columns of one image
        return c.B * Ho * cdiv(c.W, 64)
    if c.entry == 'bf16_octet':               # one image octet x 2 rows (1 at stride 2) x 8 columns
        return cdiv(c.B, 8) * cdiv(Ho, 1 if c.sh == 2 else 2) * cdiv(c.W, 8)
    if c.entry == 'bf16_nhwc':                # one image x 8 rows (4 at stride 2) x 16 columns; 16x16x32 form: 4 rows x 32 columns
        if mfma16_applies(c):
            return c.B * cdiv(Ho, 4) * cdiv(c.W, 32)
        return c.B * cdiv(Ho, 4 if c.sh == 2 else 8) * cdiv(c.W, 16)
    if c.entry == 'f16x3':                    # one image octet x one row x 8 columns
        return cdiv(c.B, 8) * Ho * cdiv(c.W, 8)
    raise ValueError(c.entry)


def splits_of(c, cu_count=256):
    """wgrad_splits (csrc/wgrad_common.h) on each entry's WgradTiling: witw_conv3x3_wgrad_splits / WG_F32, wgrad_bf16_tiling,
    wgrad_nh_tiling, WG_HX"""
    if c.entry in ('f32', 'taps4'):
        want = cdiv(1024, cdiv(c.Cin, 64) * cdiv(c.Cout, 64))
    elif c.entry == 'bf16_octet':
        want = cdiv(256, cdiv(c.Cin, 64) * cdiv(c.Cout, 128))
    elif c.entry == 'bf16_nhwc':
        want = cdiv(cu_count, cdiv(c.Cin, 64) * cdiv(c.Cout, 128))
    else:
        want = cdiv(256, cdiv(c.Cin, 64) * cdiv(c.Cout, 64))
    return max(1, min(want, chunks_of(c)))


def geometry(c, cu_count=256):
    """(splits, chunks per split, trailing splits with an empty chunk range)"""
    s, n = splits_of(c, cu_count), chunks_of(c)
    cps = cdiv(n, s)
    return s, cps, s - cdiv(n, cps)


# ------------------------------------------------------------------------------------------------ cases
def _both(entry, B, H, W, Cin, Cout, sh, geom, **kw):
    return [_c(entry, B, H, W, Cin, Cout, sh, circ, geom, **kw) for circ in (False, True)]


F32 = []
F32 += _both('f32', 1, 1, 1, 8, 8, 1, (1, 1, 0), acc=True, note='one pixel per chunk (npix = 1, odd)')
F32 += _both('f32', 1, 31, 8, 64, 64, 1, (31, 1, 0), acc=True, note='31 splits: wgrad_reduce_kernel')
F32 += _both('f32', 1, 32, 8, 64, 64, 1, (32, 1, 0), acc=True, note='32 splits: wgrad_reduce_wide_kernel')
F32 += _both('f32', 3, 100, 12, 128, 128, 1, (256, 2, 106), acc=True, note='4 tiles, 300 chunks: 106 empty trailing splits')
F32 += _both('f32', 7, 43, 12, 128, 128, 1, (256, 2, 105), note='301 chunks: the last used split holds one chunk')
F32 += _both('f32', 2, 16, 130, 256, 256, 1, (64, 2, 16), note='16 tiles, 3 segments per row, 96 chunks, cps 2: split boundaries in mid-row')
F32 += _both('f32', 2, 5, 65, 8, 72, 1, (20, 1, 0), note='a second column segment of one pixel')
F32 += [_c('f32', 2, 5, 63, 64, 64, 1, True, (10, 1, 0), note='odd npix in a single segment; the next halo column wraps to real data')]
F32 += _both('f32', 2, 2, 24, 64, 64, 2, (2, 1, 0), note='stride 2, Ho = 1')
F32 += _both('f32', 2, 1, 24, 64, 64, 2, (2, 1, 0), note='stride 2, H = 1')
F32 += _both('f32', 2, 7, 24, 64, 64, 2, (8, 1, 0), note='stride 2, odd H')
for _cin in (4, 12, 20):
    for _cout in (4, 12, 68):
        F32 += _both('f32', 2, 6, 20, _cin, _cout, 1, (12, 1, 0), note='channel counts = 4 mod 8')
for _cin, _real in ((8, 3), (8, 5), (16, 13)):
    F32 += _both('f32', 2, 6, 20, _cin, 12, 1, (12, 1, 0), cin_real=_real, acc=True, note='cin_real < Cin; the padded channels of x hold data')
for _cin in (12, 16, 24):
    F32 += [_c('taps4', 2, 9, 70, _cin, 40, 1, False, (36, 1, 0), acc=True,
               note='2x2 sub-window, %s; two segments (64 + 6)' % ('packed (tap, ci) rows' if _cin <= 16 else 'unpacked'))]

LOW = [
    # batch-octet bf16: chunk = image octet x 2 rows (1 at stride 2) x 8 columns, 64 x 128 tiles, 256 / tiles splits
    _c('bf16_octet', 3, 2, 5, 16, 32, 1, True, (1, 1, 0), acc=True, note='one chunk, one split'),
    _c('bf16_octet', 3, 100, 48, 16, 16, 1, False, (256, 2, 106), acc=True, note='300 chunks on 256 splits: 106 empty'),
    _c('bf16_octet', 8, 10, 117, 128, 256, 2, True, (64, 2, 26), note='4 tiles, 75 chunks on 64 splits: the last used split holds one'),
    # NHWC bf16, 32x32x16: chunk = image x 8 rows (4 at stride 2) x 16 columns, one split per CU and tile
    _c('bf16_nhwc', 1, 5, 9, 16, 16, 1, True, (1, 1, 0), acc=True, note='one chunk, one split'),
    _c('bf16_nhwc', 12, 40, 80, 16, 32, 1, False, (256, 2, 106), acc=True, note='300 chunks on 256 splits: 106 empty'),
    _c('bf16_nhwc', 5, 24, 80, 128, 256, 2, True, (64, 2, 26), note='4 tiles, 75 chunks on 64 splits: the last used split holds one'),
    # NHWC bf16, 16x16x32 (witw_conv3x3_wgrad_bf16_mfma16(1)): chunk = image x 4 rows x 32 columns
    _c('bf16_nhwc', 1, 4, 32, 64, 128, 1, True, (1, 1, 0), mfma16=True, acc=True, note='one chunk, one split'),
    _c('bf16_nhwc', 5, 20, 128, 128, 256, 1, False, (64, 2, 14), mfma16=True, acc=True, note='4 tiles, 100 chunks on 64 splits: 14 empty'),
    _c('bf16_nhwc', 5, 12, 160, 128, 256, 1, True, (64, 2, 26), mfma16=True, note='75 chunks on 64 splits: the last used split holds one'),
    # fp16x3: chunk = image octet x one row x 8 columns, 64 x 64 tiles, two partials per split
    _c('f16x3', 3, 1, 5, 16, 16, 1, True, (1, 1, 0), acc=True, note='one chunk, one split'),
    _c('f16x3', 3, 50, 48, 16, 16, 1, False, (256, 2, 106), acc=True, note='300 chunks on 256 splits: 106 empty'),
    _c('f16x3', 8, 9, 117, 128, 128, 2, True, (64, 2, 26), note='4 tiles, 75 chunks on 64 splits: the last used split holds one'),
]

# the 2x2 sub-window form once more at the two shapes every entry's accumulate mode runs at (appended: a case's place seeds its operands)
TAPS4_ACC = [
    _c('taps4', 1, 1, 40, 12, 8, 1, False, (1, 1, 0), acc=True, note='packed; one chunk, one split: wgrad_reduce_kernel'),
    _c('taps4', 3, 100, 12, 128, 128, 1, False, (256, 2, 106), acc=True, note='unpacked; 4 tiles, 300 chunks: 106 empty trailing splits'),
]

CASES = F32 + LOW + TAPS4_ACC
assert len({case_id(c) for c in CASES}) == len(CASES)


# ------------------------------------------------------------------------------------------------ operands, references
def _randn(seed, stream, shape):
    g = np.random.Generator(np.random.Philox(key=[seed, stream]))
    return torch.from_numpy(g.standard_normal(shape, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def reference(c):
    """per case, once: CPU operands (all Cin channels of x carry data), the float64 reference and scale on the cin_real real
    channels, and the err of fp32 CPU autograd through the oracle's convolution on the same operands"""
    Ho = A.out_rows(c.H, c.sh)
    seed = 1000 + CASES.index(c)
    x, dz = _randn(seed, 1, (c.B, c.Cin, c.H, c.W)), _randn(seed, 2, (c.B, c.Cout, Ho, c.W))
    if c.entry.startswith('bf16'):
        x, dz = x.bfloat16().float(), dz.bfloat16().float()
    taps4 = c.entry == 'taps4'
    xr = x[:, :c.cin_real].contiguous()
    ref_w, ref_b = R.wgrad_ref(xr, dz, c.sh, c.circ, taps4)
    sc_w, sc_b = R.wgrad_scale(xr, dz, c.sh, c.circ, taps4)
    w = torch.zeros((c.Cout, c.cin_real, 3, 3), requires_grad=True)
    b = torch.zeros((c.Cout,), requires_grad=True)
    O.conv3x3(xr, w, b, c.sh, c.circ).backward(dz)
    ag_w = w.grad.clone()
    if taps4:                   # the full form's first tap row / column belong to another filter
        ag_w[:, :, 0, :] = 0
        ag_w[:, :, :, 0] = 0
    out = dict(x=x, dz=dz, ref_w=ref_w, ref_b=ref_b, sc_w=sc_w, sc_b=sc_b,
               ag_w=R.err(ag_w, ref_w, sc_w), ag_b=R.err(b.grad, ref_b, sc_b))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def bounds(c):
    ref = reference(c)
    return max(MARGIN * ref['ag_w'], FLOOR), max(MARGIN * ref['ag_b'], FLOOR)


@contextlib.contextmanager
def kernel_form(c):
    """the 16x16x32 form of the NHWC entry through the library's switch, for the cases that name it (the switch also changes the
    split count, so it is set before the workspace is sized)"""
    from witw_amd import _lib
    lib = _lib.load()
    prev = lib.witw_conv3x3_wgrad_bf16_mfma16(1 if c.mfma16 else 0)
    try:
        yield
    finally:
        lib.witw_conv3x3_wgrad_bf16_mfma16(prev)


def dims(c):
    return (c.B, c.H, c.W, c.Cin, c.Cout, c.sh)


def check_premise(c):
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    got = A.lib_splits(c.entry, *dims(c))
    assert got == c.splits, '%s: the launcher uses %d splits, the case was written for %d' % (case_id(c), got, c.splits)
    assert geometry(c, cu) == (c.splits, c.cps, c.empty), (case_id(c), geometry(c, cu), (c.splits, c.cps, c.empty))
    assert c.cps == cdiv(chunks_of(c), c.splits) and c.empty == c.splits - cdiv(chunks_of(c), c.cps)
    if c.mfma16:
        assert mfma16_applies(c)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def launch(c, arena, opnd=None, **kw):
    if opnd is None:
        ref = reference(c)
        opnd = A.operands(c.entry, ref['x'], ref['dz'])
    out = A.run(c.entry, opnd, dims(c), c.cin_real, c.circ, arena, **kw)
    if c.entry == 'bf16_nhwc':
        from witw_amd import ops
        form = 'conv3x3_wgrad_bf16_nhwc16_kernel<1,4>' if c.mfma16 else 'conv3x3_wgrad_bf16_nhwc_kernel<%d,' % c.sh
        assert ops.last_kernel_variant().startswith(form), ops.last_kernel_variant()
    return out


def measure(c, arena=None):
    """the case's premise, then two launches on NaN workspaces -> (row, (dw, db), (dw2, db2)). row holds the errs against the float64
    reference, the yardstick's, their ratios and the bounds: what the parity test asserts and what tools/wgrad_edge_ratios.py records"""
    ref = reference(c)
    arena = arena or Arena('cuda:0')
    with kernel_form(c):
        check_premise(c)
        opnd = A.operands(c.entry, ref['x'], ref['dz'])
        first = launch(c, arena, opnd)
        second = launch(c, arena, opnd)
    dw, db = first
    assert dw.shape == (c.Cout, c.cin_real, 3, 3) and db.shape == (c.Cout,)
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), 'NaN from the workspace reached the result'
    e_w, e_b = R.err(dw, ref['ref_w'], ref['sc_w']), R.err(db, ref['ref_b'], ref['sc_b'])
    b_w, b_b = bounds(c)
    row = dict(id=case_id(c), splits=c.splits, cps=c.cps, empty_splits=c.empty, note=c.note, err_dw=e_w, err_db=e_b,
               autograd_err_dw=ref['ag_w'], autograd_err_db=ref['ag_b'], bound_dw=b_w, bound_db=b_b,
               ratio_dw=e_w / ref['ag_w'] if ref['ag_w'] > 0 else None, ratio_db=e_b / ref['ag_b'] if ref['ag_b'] > 0 else None,
               err_dw_ulp=e_w / R.F32_ULP, err_db_ulp=e_b / R.F32_ULP)
    return row, first, second


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_parity_repeatable_whatever_the_workspace_held(c):
    """premise; float64 parity of dw and db within the case's bound; finite although the workspace held NaN (an empty split is
    right only because its workgroups still store a zero tile); no guard band touched, every element stored; same bits twice"""
    row, (dw, db), (dw2, db2) = measure(c)
    print('%(id)s: err dw %(err_dw).3g (autograd %(autograd_err_dw).3g, bound %(bound_dw).3g), db %(err_db).3g (autograd '
          '%(autograd_err_db).3g, bound %(bound_db).3g)' % row)
    assert row['err_dw'] <= row['bound_dw'], 'dw: err %(err_dw).3g of the scale, fp32 autograd %(autograd_err_dw).3g, bound %(bound_dw).3g' % row
    assert row['err_db'] <= row['bound_db'], 'db: err %(err_db).3g of the scale, fp32 autograd %(autograd_err_db).3g, bound %(bound_db).3g' % row
    if c.entry == 'taps4':
        assert not bool(dw[:, :, 0, :].any()) and not bool(dw[:, :, :, 0].any())
    assert same_bits(dw, dw2) and same_bits(db, db2)


@pytest.mark.parametrize('c', [c for c in CASES if c.acc], ids=case_id)
def test_accumulate_is_one_fp32_add(c):
    """accumulate = 1: every element of dw / db becomes (old value) + (what accumulate = 0 stores), one fp32 add -- bit for bit;
    twice gives (G0 + p) + p; db = NULL leaves dw's contract alone; the dead taps of the 2x2 sub-window form keep G0; with
    cin_real < Cin nothing outside [Cout][cin_real][3][3] is touched (guard bands)"""
    ref = reference(c)
    arena = Arena('cuda:0')
    gen = torch.Generator('cuda:0').manual_seed(77 + CASES.index(c))
    G0 = torch.randn((c.Cout, c.cin_real, 3, 3), generator=gen, device='cuda:0')
    g0 = torch.randn((c.Cout,), generator=gen, device='cuda:0')
    with kernel_form(c):
        check_premise(c)
        opnd = A.operands(c.entry, ref['x'], ref['dz'])
        p_w, p_b = launch(c, arena, opnd)
        a_w, a_b = launch(c, arena, opnd, accumulate=1, dw_init=G0, db_init=g0)
        aa_w, aa_b = launch(c, arena, opnd, accumulate=1, dw_init=a_w, db_init=a_b)
        n_w, n_b = launch(c, arena, opnd, accumulate=1, dw_init=G0, want_db=False)
    assert bool(p_w.any()) and bool(p_b.any()) and bool(torch.isfinite(p_w).all()) and bool(torch.isfinite(p_b).all())
    assert same_bits(a_w, G0 + p_w), 'dw: %d element(s) differ from G0 + plain' % int((bits(a_w) != bits(G0 + p_w)).sum())
    assert same_bits(a_b, g0 + p_b), 'db: %d element(s) differ from g0 + plain' % int((bits(a_b) != bits(g0 + p_b)).sum())
    assert same_bits(aa_w, (G0 + p_w) + p_w) and same_bits(aa_b, (g0 + p_b) + p_b)
    assert n_b is None and same_bits(n_w, G0 + p_w)
    if c.entry == 'taps4':
        for t in (a_w, aa_w, n_w):
            assert same_bits(t[:, :, 0, :], G0[:, :, 0, :]) and same_bits(t[:, :, :, 0], G0[:, :, :, 0])


def _order_cases():
    """existing cases whose workspace is re-reduced on the CPU: both fp32 reduce kernels at their threshold, empty splits, padded
    input channels, both forms of the 2x2 sub-window, and every case of the 16-bit entries that runs on 32x32x16 (plus the
    16x16x32 case with empty splits)"""
    f32 = [c for c in F32 if c.entry == 'f32']
    picked = [c for c in f32 if c.splits in (31, 32) or (c.B, c.H, c.W, c.Cin, c.Cout) == (3, 100, 12, 128, 128)]
    picked += [c for c in f32 if c.cin_real < c.Cin][:1]
    picked += TAPS4_ACC
    picked += [c for c in LOW if not c.mfma16 or c.empty == 14]
    return picked


def _fp32_sum(parts, wide):
    """parts [k][...] fp32 on the CPU -> their sum in the kernels' order, one elementwise fp32 add per partial.
    serial (wgrad_reduce_kernel): ((0 + p[0]) + p[1]) + ...; wide (wgrad_reduce_wide_kernel): eight group sums over
    k = g, g + 8, ..., each serial from zero, then group 0's sum + group 1's + ... + group 7's"""
    def serial(seq):
        s = torch.zeros_like(parts[0])
        for p in seq:
            s = s + p
        return s
    if not wide:
        return serial(parts)
    groups = [serial(parts[g::8]) for g in range(8)]
    s = groups[0]
    for g in range(1, 8):
        s = s + groups[g]
    return s


@pytest.mark.parametrize('c', _order_cases(), ids=case_id)
def test_reduction_is_the_stated_fp32_order(c):
    """dw and db are, bit for bit, the partials the launch left in the workspace added in the documented order: serial from
    zero everywhere, except the fp32 entries at >= 32 splits (eight interleaved group sums, then the groups in order).
    Workspace: weight partials [parts][taps][Cin][Cout], bias partials [bparts][Cout] at float offset parts * 9 * Cin * Cout."""
    from witw_amd import _lib
    ref = reference(c)
    arena = Arena('cuda:0')
    with kernel_form(c):
        check_premise(c)
        rc, dw, db, ws = A.call(c.entry, A.operands(c.entry, ref['x'], ref['dz']), dims(c), c.cin_real, c.circ, arena)
    _lib.check(rc, 'wgrad entry %r' % c.entry)
    arena.check((dw, db))
    ws, dw, db = ws.cpu(), dw.cpu(), db.cpu()
    taps = 4 if c.entry == 'taps4' else 9
    parts = 2 * c.splits if c.entry == 'f16x3' else c.splits
    bparts = A.f16x3_bias_parts(c.B, c.H, c.W, c.sh) if c.entry == 'f16x3' else c.splits
    wide = c.entry in ('f32', 'taps4') and c.splits >= 32
    n, b0 = taps * c.Cin * c.Cout, parts * 9 * c.Cin * c.Cout
    assert ws.numel() == b0 + bparts * c.Cout
    s_w = _fp32_sum(ws[:parts * n].view(parts, taps, c.Cin, c.Cout), wide)[:, :c.cin_real]      # [taps][cin_real][Cout]
    s_b = _fp32_sum(ws[b0:].view(bparts, c.Cout), wide)
    if taps == 9:
        want = s_w.view(3, 3, c.cin_real, c.Cout).permute(3, 2, 0, 1)
    else:
        want = torch.zeros((c.Cout, c.cin_real, 3, 3))
        for t in range(4):
            want[:, :, 1 + (t >> 1), 1 + (t & 1)] = s_w[t].t()
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(s_b).all()), 'a partial was left unwritten'
    assert same_bits(dw, want.contiguous()), 'dw: %d element(s) differ' % int((bits(dw) != bits(want)).sum())
    assert same_bits(db, s_b), 'db: %d element(s) differ' % int((bits(db) != bits(s_b)).sum())


REFUSALS = [  # entry, (B, H, W, Cin, Cout, stride_h), cin_real, what
    ('f32', (2, 6, 20, 6, 8, 1), 6, 'Cin = 6'),
    ('taps4', (2, 6, 20, 6, 8, 1), 6, 'Cin = 6'),
    ('bf16_octet', (2, 6, 20, 12, 16, 1), 12, 'Cin = 12'),
    ('bf16_nhwc', (2, 6, 20, 12, 16, 1), 12, 'Cin = 12'),
    ('f16x3', (2, 6, 20, 12, 16, 1), 12, 'Cin = 12'),
    ('f16x3', (2, 6, 20, 16, 24, 1), 16, 'bias gradient at Cout = 24: Cout / 8 = 3 does not divide 256'),
]
for _e in A.ENTRIES:
    REFUSALS += [(_e, (2, 6, 20, 16, 16, 1), 0, 'cin_real = 0'), (_e, (2, 6, 20, 16, 16, 1), 17, 'cin_real = Cin + 1')]
    if _e != 'taps4':
        REFUSALS += [(_e, (2, 6, 20, 16, 16, 3), 16, 'stride 3')]


@pytest.mark.parametrize('r', REFUSALS, ids=lambda r: '%s-%s' % (r[0], r[3].split(':')[0].replace(' ', '')))
def test_refusals_return_an_error_and_write_nothing(r):
    entry, d, cin_real, what = r
    B, H, W, Cin, Cout, sh = d
    arena = Arena('cuda:0')
    gen = torch.Generator('cuda:0').manual_seed(5)
    # operands as large as any reading of the shape could want (nothing should be read at all)
    opnd = [torch.randn((8 * 9 * 32 * 32 * 16,), generator=gen, device='cuda:0') for _ in range(3 if entry == 'f16x3' else 2)]
    rc, dw, db, ws = A.call(entry, opnd, d, cin_real, False, arena, dw_shape=(Cout, Cin + 1, 3, 3), ws_floats=1 << 16)
    assert rc != 0, '%s accepted %s' % (entry, what)
    assert A.last_error(), 'an error code without a message'
    torch.cuda.synchronize()
    canary = canary_int(torch.float32)
    assert bool((bits(dw) == canary).all()) and bool((bits(db) == canary).all()), 'a refused call stored to dw / db'
    assert bool(torch.isnan(ws).all()), 'a refused call stored to the workspace'
    arena.check()
    if 'bias' in what:      # the precedent: the same call without the bias gradient is served
        x, dz = _randn(9, 1, (B, Cin, H, W)), _randn(9, 2, (B, Cout, A.out_rows(H, sh), W))
        dw2, _ = A.run('f16x3', A.operands('f16x3', x, dz), d, Cin, False, arena, want_db=False)
        assert bool(torch.isfinite(dw2).all())


def test_split_restatements_match_the_library():
    """splits_of / chunks_of above against the library's workspace entries over a sweep of shapes (both forms of the NHWC entry)"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    g = np.random.Generator(np.random.Philox(key=[3, 3]))
    n = 0
    for entry in A.ENTRIES:
        for mfma16 in ((False, True) if entry == 'bf16_nhwc' else (False,)):
            for _ in range(200):
                B, H, W = int(g.integers(1, 20)), int(g.integers(1, 70)), int(g.integers(1, 11)) * int(g.choice([1, 7, 16, 32]))
                Cin, Cout = 8 * int(g.integers(1, 40)), 8 * int(g.integers(1, 40))
                sh = 1 if entry == 'taps4' else int(g.integers(1, 3))
                c = _c(entry, B, H, W, Cin, Cout, sh, False, (0, 0, 0), mfma16=mfma16)
                with kernel_form(c):
                    assert A.lib_splits(entry, B, H, W, Cin, Cout, sh) == splits_of(c, cu), (case_id(c), splits_of(c, cu))
                n += mfma16_applies(c)
    assert n >= 10          # the sweep reached the 16x16x32 form's own chunk shape
