"""Edge sweep of the match backward against a float64 reference: witw_match_bwd (csrc/match.hip) and witw_match_bwd_pairs
(csrc/loss_hard.hip), called through ctypes with outputs, scratch and operands between guard bands (tests/mem_arena.py) and the
scratch of the dense entry filled with NaN, so a split that fails to write its slab shows in the result.

Orientations are the test's own (uniform in [0, 64) from a fixed seed, or forced), so no case depends on the forward kernels or
on an arg-max near-tie; score, window norms and surface norms are the float64 values of tests/match_bwd_ref.py rounded to fp32.
One case takes all three from ops.match_fwd instead. Embeddings come from synth.embeddings, gD is standard normal.

Every dense case states the geometry it was written for -- (splits of the overheads, overheads per split, trailing splits whose
overhead range is empty) -- and the test asserts it against the library (tests/test_match_bwd_ref.py does the same without a
GPU), so a change to the split heuristic fails loudly instead of emptying a case.

Parity (the criterion of tests/test_wgrad_edges_gpu.py). err = max |got - ref| / scale per element, ref and scale in float64
(scale = the same sum over the absolute values of its terms; scale 0 demands an exact 0). The yardstick is the err of fp32 CPU
autograd through the oracle's crop_overhead and l2_distance at the same operands and the same orientations (not O.match, whose
own arg-max may differ), i.e. of ANOTHER fp32 evaluation of the same terms. The kernel may have MARGIN = 4 times that (two fp32
summation orders of the same terms err like independent random walks; 4 is the margin between two such walks' maxima) and is
never held below one fp32 ulp (2^-23) of the scale. Where the crop tensor of a case would not fit in memory the yardstick runs
over blocks of overhead rows, surface gradients accumulated by autograd from block to block: still fp32 autograd through the
same two functions. For a pair list the yardstick sums one term per list entry, as the kernels do (pair_blocks: a repeated
pair goes to as many backward passes as it has entries; indexing the distance matrix once with the whole list would add the
weights of a repeated pair first and sum fewer terms than the kernel). Every case also asserts that the median of |ref| / scale over the elements that have a term is above 1e-3,
so that cancellation cannot make the bound vacuous (a list without one valid pair has no such element: there every output must
be an exact 0).

Measured on the MI355X (profiles/match_bwd_edges.json, written by tools/match_bwd_edge_ratios.py from these cases; DESIGN.md
section 4.8): no case needs more than the margin. The worst ratios are 3.68 (grad_su of the 600 entries that name one surface:
1.03 ulp of the scale from the kernel's sequential 600-term sum, 0.28 ulp from autograd's ten blocks of 64), 3.30 (grad_su at
600 x 5 without scratch) and 3.09 (grad_ov of the 600 entries that name one overhead); no element is off by more than 3.2 ulp of
its scale. With the distance matrix indexed once by the whole list -- the yardstick as first written, 64 terms for that surface
instead of 600 -- the first of these ratios was 4.9 at the same kernel error; the margin was left alone and the yardstick made
to sum the kernel's terms. Where a window has few columns (We 3 and 4: dense-1089x23x3, pairs-ragged) the yardstick's maximum on
grad_ov is 266 and 42 ulp: autograd computes the score c itself in fp32, and where an element's self term 2 c ov / (wn^3 sn)
dominates and c is small from cancellation, c's error is the element's. The kernels are handed c and stay at 2.7 and 2.4 ulp
there, so the bound of those two grad_ov checks is looser than a summation-order bound; test_forward_outputs_plug_in has the
kernel consume the forward's own fp32 score.
"""
import collections
import functools

import numpy as np
import pytest
import torch

from oracle import cvig_fov_oracle as O
from tests import match_bwd_ref as R
from tests.mem_arena import Arena
from witw_amd import synth

pytestmark = pytest.mark.gpu

MARGIN = 4.0                    # kernel err <= MARGIN x the err of fp32 CPU autograd on the same operands ...
FLOOR = R.F32_ULP               # ... and never below one fp32 ulp of the scale
NONTRIVIAL = 1e-3               # median |ref| / scale of the elements that have a term
YARDSTICK_BLOCK = 1 << 25       # elements of the [rows, Bs, 16, 4, 64] tensor autograd builds behind crop_overhead, per block
PAIRS_MAX = 8192                # csrc/loss_hard.hip

Dense = collections.namedtuple('Dense', 'Bo Bs We splits per empty scratch ori gd seed note')
Pairs = collections.namedtuple('Pairs', 'name n Bo Bs We seed note')


def _d(Bo, Bs, We, geom, seed, note, scratch=True, ori='rand', gd='randn'):
    return Dense(Bo, Bs, We, geom[0], geom[1], geom[2], scratch, ori, gd, seed, note)


def case_id(c):
    if isinstance(c, Pairs):
        return 'pairs-%s-%d-%dx%dx%d' % (c.name, c.n, c.Bo, c.Bs, c.We)
    s = 'dense-%dx%dx%d' % (c.Bo, c.Bs, c.We)
    return s + ('' if c.scratch else '-noscratch') + ('' if c.ori == 'rand' else '-ori_' + c.ori) + ('' if c.gd == 'randn' else '-' + c.gd)


# ------------------------------------------------------------------------------------------------ cases
DENSE = [
    _d(1, 1, 64, (1, 1, 0), 11, 'direct store, one partner'),
    _d(37, 29, 33, (2, 19, 0), 12, 'the shape of test_backward_gpu.py, now against float64'),
    _d(70, 5, 63, (3, 24, 0), 13, 'We 63; the last split holds 22 overheads'),
    _d(33, 768, 1, (1, 33, 0), 14, 'We 1; three surface chunks in the ov kernel'),
    _d(300, 800, 2, (1, 300, 0), 15, 'a second overhead chunk of 44 in the su kernel with direct store; four surface chunks, the last of 32'),
    _d(1089, 23, 3, (34, 33, 1), 16, 'the last split is empty and must contribute zeros'),
    _d(600, 5, 64, (1, 600, 0), 17, 'scratch = NULL, one block per surface: chunks of 256, 256 and 88', scratch=False),
]
WRAP = [_d(37, 29, we, (2, 19, 0), 20 + we, 'window wrap, orientations %s' % mode, ori=mode)
        for we in (64, 1) for mode in ('zero', 'max', 'alt')]
ZERO = [_d(37, 29, 33, (2, 19, 0), 30, 'one zero row and one zero column of gD: exact zeros', gd='zero_rowcol')]
ONE_SIDED = [DENSE[1], DENSE[4]]
REAL_USE = DENSE[1]

PAIRS = [
    Pairs('one', 1, 64, 64, 12, 41, 'npad = 2; every other row exactly 0'),
    Pairs('one_surface', 600, 64, 64, 12, 42, 'every ps = 7, po cycling: an su segment of 600 = chunks of 256, 256 and 88'),
    Pairs('one_overhead', 600, 64, 64, 12, 43, 'every po = 5, ps cycling: the same in the ov kernel'),
    Pairs('ragged', 1025, 64, 64, 4, 44, 'npad 2048 with 1,023 padding keys; -1, o = Bo and s = Bs entries dropped'),
    Pairs('max', PAIRS_MAX, 64, 64, 4, 45, 'PAIRS_MAX: 64 KB of LDS, eight keys per thread; one pair repeated 300 times'),
    Pairs('invalid', 40, 64, 64, 12, 46, 'no valid pair: both gradients exactly zero everywhere'),
    Pairs('mixed', 120, 40, 24, 64, 364, 'the list of test_batch_hard_gpu.py, now against float64'),
]

CASES = DENSE + WRAP + ZERO + PAIRS
assert len({case_id(c) for c in CASES}) == len(CASES)


def scratch_geometry(c):
    """(splits, overheads per split, empty trailing splits) the launcher uses for the case"""
    return R.geometry(c.Bo, c.Bs) if c.scratch else (1, c.Bo, 0)


# ------------------------------------------------------------------------------------------------ operands, references
def _gen(seed, stream):
    return np.random.Generator(np.random.Philox(key=[seed, stream]))


def _orientations(c):
    if isinstance(c, Pairs) or c.ori == 'rand':
        return _gen(c.seed, 1).integers(0, 64, size=(c.Bo, c.Bs), dtype=np.int64)
    if c.ori == 'alt':
        return (63 * ((np.arange(c.Bo)[:, None] + np.arange(c.Bs)[None, :]) & 1)).astype(np.int64)
    return np.full((c.Bo, c.Bs), {'zero': 0, 'max': 63}[c.ori], dtype=np.int64)


def _pair_list(c):
    """(po, ps, pw): int32, int32, fp32 numpy"""
    g = _gen(c.seed, 3)
    n, Bo, Bs = c.n, c.Bo, c.Bs
    po, ps = g.integers(0, Bo, size=n).astype(np.int32), g.integers(0, Bs, size=n).astype(np.int32)
    pw = g.standard_normal(n, dtype=np.float32)
    if c.name == 'one':
        po[:], ps[:] = 17, 42
    elif c.name == 'one_surface':
        po[:], ps[:] = np.arange(n) % Bo, 7
    elif c.name == 'one_overhead':
        po[:], ps[:] = 5, np.arange(n) % Bs
    elif c.name == 'ragged':
        po[3::97] = -1
        ps[5::89] = -1
        po[7::83] = Bo
        ps[11::79] = Bs
    elif c.name == 'max':
        po[1000:8192:24], ps[1000:8192:24] = 9, 31         # 300 entries of one pair, spread through the list
        assert int(((po == 9) & (ps == 31)).sum()) >= 300
    elif c.name == 'invalid':
        po[0::2] = -1
        ps[1::2] = Bs
    elif c.name == 'mixed':
        from tests.test_batch_hard_gpu import _pairs_case
        _ov, _su, tpo, tps, tpw = _pairs_case(Bo, Bs, c.We, c.seed)
        po, ps, pw = tpo.numpy(), tps.numpy(), tpw.numpy()
        assert po.shape == (n,)
    return po, ps, pw


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def exact(c):
    """per case, once: CPU operands, the float64 reference with its scales and the float64 kernel inputs"""
    if isinstance(c, Pairs) and c.name == 'mixed':
        from tests.test_batch_hard_gpu import _pairs_case
        tov, tsu = _pairs_case(c.Bo, c.Bs, c.We, c.seed)[:2]
        ov, su = tov.numpy(), tsu.numpy()
    else:
        ov, su = synth.embeddings(c.seed, 1, (c.Bo, 16, 4, 64)), synth.embeddings(c.seed, 2, (c.Bs, 16, 4, c.We))
    ori = _orientations(c)
    out = dict(ov=ov, su=su, ori=ori)
    if isinstance(c, Pairs):
        po, ps, pw = _pair_list(c)
        gd, ga, ok = R.pairs_to_dense(po, ps, pw, c.Bo, c.Bs)
        out.update(po=po, ps=ps, pw=pw, ok=ok)
        ref = R.match_bwd_ref(ov, su, ori, gd, ga)
    else:
        gd = _gen(c.seed, 2).standard_normal((c.Bo, c.Bs), dtype=np.float32)
        if c.gd == 'zero_rowcol':
            gd[c.Bo // 3, :] = 0
            gd[:, c.Bs // 2] = 0
        out.update(gd=gd)
        ref = R.match_bwd_ref(ov, su, ori, gd)
    score, wn, sn = R.kernel_inputs(ov, su, ori)
    out.update(ref_ov=ref[0], ref_su=ref[1], sc_ov=ref[2], sc_su=ref[3], score=score.astype(np.float32),
               ws=np.concatenate([wn.ravel(), sn]).astype(np.float32))
    return _freeze(out)


def median_ref_over_scale(ref, scale):
    """median |ref| / scale over the elements that have a term (None: no such element)"""
    live = scale > 0
    return float(np.median(np.abs(ref[live]) / scale[live])) if live.any() else None


def autograd_f32(ov, su, ori, blocks):
    """fp32 CPU autograd through the oracle's crop_overhead and l2_distance at the orientations `ori`. blocks: (rows, weigh)
    pairs -- overhead rows (a slice or indices) and a function of their distances d [len(rows), Bs] -> scalar; each block is
    one backward, the gradients accumulated by autograd from block to block -> (grad_ov, grad_su) fp32"""
    ovr = torch.from_numpy(np.array(ov)).requires_grad_(True)
    sur = torch.from_numpy(np.array(su)).requires_grad_(True)
    ori = torch.from_numpy(np.array(ori))
    for rows, weigh in blocks:
        if not isinstance(rows, slice):
            rows = torch.from_numpy(np.asarray(rows, dtype=np.int64))
        n = ori[rows].shape[0]
        assert n == 1 or n * sur.shape[0] * 4096 <= YARDSTICK_BLOCK
        weigh(O.l2_distance(O.crop_overhead(ovr[rows], ori[rows], sur.shape[3]), sur)).backward()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)      # noqa: E731
    return zero(ovr), zero(sur)


def dense_blocks(gd):
    """sum(gD * d) over blocks of consecutive overhead rows that keep the tensor behind the crop's gather within YARDSTICK_BLOCK"""
    gd = torch.from_numpy(np.array(gd))
    Bo, Bs = gd.shape
    n = max(1, YARDSTICK_BLOCK // (Bs * 4096))
    return [(slice(o0, min(Bo, o0 + n)), lambda d, o0=o0: (d * gd[o0:o0 + d.shape[0]]).sum()) for o0 in range(0, Bo, n)]


def pair_blocks(po, ps, pw, ok, Bs):
    """sum(pw[i] * d[po[i], ps[i]]) over the valid entries, ONE TERM PER LIST ENTRY as in the kernels: block k holds the k-th
    occurrence of every (o, s) in list order, so no block names a pair twice and autograd never adds two weights before it
    multiplies (indexing d once with the whole list would: its backward accumulates the weights of a repeated pair first, and
    the yardstick would then sum fewer terms than the kernel -- 64 instead of 600 where every entry names one surface)"""
    idx = np.flatnonzero(ok)
    cell = po[idx].astype(np.int64) * Bs + ps[idx]
    order = np.argsort(cell, kind='stable')
    first = np.flatnonzero(np.r_[True, cell[order][1:] != cell[order][:-1]])
    occ = np.empty(len(idx), dtype=np.int64)
    occ[order] = np.arange(len(idx)) - np.repeat(first, np.diff(np.r_[first, len(idx)]))
    blocks = []
    for k in range(int(occ.max()) + 1 if len(idx) else 0):
        sel = idx[occ == k]
        rows, inv = np.unique(po[sel], return_inverse=True)
        r, s, w = torch.from_numpy(inv.astype(np.int64)), torch.from_numpy(ps[sel].astype(np.int64)), torch.from_numpy(pw[sel])
        blocks.append((rows, lambda d, r=r, s=s, w=w: (w * d[r, s]).sum()))
    return blocks


@functools.lru_cache(maxsize=None)
def yardstick(c):
    """(err of grad_ov, err of grad_su) of fp32 CPU autograd on the case's operands against its float64 reference"""
    ex = exact(c)
    blocks = pair_blocks(ex['po'], ex['ps'], ex['pw'], ex['ok'], c.Bs) if isinstance(c, Pairs) else dense_blocks(ex['gd'])
    g_ov, g_su = autograd_f32(ex['ov'], ex['su'], ex['ori'], blocks)
    return R.err(g_ov, ex['ref_ov'], ex['sc_ov']), R.err(g_su, ex['ref_su'], ex['sc_su'])


def bound(yard):
    return max(MARGIN * yard, FLOOR)


# ------------------------------------------------------------------------------------------------ the entries, through ctypes
def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def device_operands(c, arena, ex=None):
    """the case's inputs on the device, each between NaN bands (a stray read that is multiplied poisons the result)"""
    ex = ex or exact(c)
    dev = arena.device
    names = ('ov', 'su', 'ori', 'score', 'ws') + (('po', 'ps', 'pw') if isinstance(c, Pairs) else ('gd',))
    return {k: arena.place(torch.from_numpy(np.array(ex[k])).to(dev), label=k) for k in names}


def launch_dense(c, arena, opnd, want_ov=True, want_su=True):
    """one witw_match_bwd; the scratch (if the case passes one) is a fresh NaN-filled allocation -> (grad_ov, grad_su)"""
    from witw_amd import _lib, ops
    lib = _lib.load()
    n = int(lib.witw_match_bwd_scratch_floats(c.Bo, c.Bs, c.We)) if c.scratch else 0
    assert n == (R.scratch_floats(c.Bo, c.Bs, c.We) if c.scratch else 0)
    scratch = None
    if n > 0:
        scratch = arena.empty((n,))
        scratch.fill_(float('nan'))
    gov = arena.empty((c.Bo, 16, 4, 64)) if want_ov else None
    gsu = arena.empty((c.Bs, 16, 4, c.We)) if want_su else None
    p = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    rc = lib.witw_match_bwd(p(opnd['ov']), p(opnd['su']), p(opnd['ori']), p(opnd['score']), p(opnd['ws']), p(opnd['gd']),
                            p(gov), p(gsu), p(scratch), c.Bo, c.Bs, c.We, ops._stream())
    _lib.check(rc, 'witw_match_bwd')
    arena.check((gov, gsu))
    return gov, gsu


def launch_pairs(c, arena, opnd):
    """one witw_match_bwd_pairs on a fresh canary-filled scratch -> (grad_ov, grad_su)"""
    from witw_amd import _lib, ops
    lib = _lib.load()
    nb = int(lib.witw_match_bwd_pairs_scratch_bytes(c.n, c.Bo, c.Bs))
    assert nb == 4 * (2 * c.n + 2 * c.Bo + 2 * c.Bs)
    scratch = arena.empty((nb,), torch.uint8)
    gov, gsu = arena.empty((c.Bo, 16, 4, 64)), arena.empty((c.Bs, 16, 4, c.We))
    rc = lib.witw_match_bwd_pairs(opnd['ov'].data_ptr(), opnd['su'].data_ptr(), opnd['ori'].data_ptr(), opnd['score'].data_ptr(),
                                  opnd['ws'].data_ptr(), opnd['po'].data_ptr(), opnd['ps'].data_ptr(), opnd['pw'].data_ptr(), c.n,
                                  c.Bo, c.Bs, c.We, gov.data_ptr(), gsu.data_ptr(), scratch.data_ptr(), ops._stream())
    _lib.check(rc, 'witw_match_bwd_pairs')
    arena.check((gov, gsu))
    return gov, gsu


def check_premise(c):
    if isinstance(c, Pairs):
        assert 1 <= c.n <= PAIRS_MAX
        return
    from witw_amd import _lib
    want = (c.splits, c.per, c.empty)
    assert scratch_geometry(c) == want, '%s: geometry %s, the case was written for %s' % (case_id(c), scratch_geometry(c), want)
    got = int(_lib.load().witw_match_bwd_scratch_floats(c.Bo, c.Bs, c.We))
    splits = R.splits(c.Bo, c.Bs)
    assert got == (splits * c.Bs * (64 * c.We + 1) if splits > 1 else 0), (case_id(c), got, splits)


def measure(c, arena=None):
    """the case's premise, then two launches -> (row, (gov, gsu), (gov2, gsu2)). row holds the errs against the float64 reference,
    the yardstick's, their ratios and the bounds: what the parity tests assert and what tools/match_bwd_edge_ratios.py records"""
    ex = exact(c)
    arena = arena or Arena('cuda:0')
    check_premise(c)
    opnd = device_operands(c, arena)
    run = launch_pairs if isinstance(c, Pairs) else launch_dense
    first, second = run(c, arena, opnd), run(c, arena, opnd)
    return row_of(c, ex, first[0], first[1], yardstick(c)), first, second


def row_of(c, ex, gov, gsu, yard):
    e_ov, e_su = R.err(gov, ex['ref_ov'], ex['sc_ov']), R.err(gsu, ex['ref_su'], ex['sc_su'])
    if isinstance(c, Pairs):
        geom = dict(pairs=c.n, valid_pairs=int(ex['ok'].sum()),
                    longest_ov_segment=int(np.bincount(ex['po'][ex['ok']], minlength=1).max()) if ex['ok'].any() else 0,
                    longest_su_segment=int(np.bincount(ex['ps'][ex['ok']], minlength=1).max()) if ex['ok'].any() else 0)
    else:
        geom = dict(zip(('splits', 'overheads_per_split', 'empty_splits'), scratch_geometry(c)))
    return dict(id=case_id(c), note=c.note, err_ov=e_ov, err_su=e_su, autograd_err_ov=yard[0], autograd_err_su=yard[1],
                bound_ov=bound(yard[0]), bound_su=bound(yard[1]), ratio_ov=e_ov / yard[0] if yard[0] > 0 else None,
                ratio_su=e_su / yard[1] if yard[1] > 0 else None, err_ov_ulp=e_ov / R.F32_ULP, err_su_ulp=e_su / R.F32_ULP,
                median_ref_over_scale_ov=median_ref_over_scale(ex['ref_ov'], ex['sc_ov']),
                median_ref_over_scale_su=median_ref_over_scale(ex['ref_su'], ex['sc_su']), **geom)


def assert_parity(row, expect_terms=True):
    print('%(id)s: err ov %(err_ov).3g (autograd %(autograd_err_ov).3g, bound %(bound_ov).3g), su %(err_su).3g (autograd '
          '%(autograd_err_su).3g, bound %(bound_su).3g)' % row)
    for side in ('ov', 'su'):
        med = row['median_ref_over_scale_' + side]
        if expect_terms:
            assert med is not None and med > NONTRIVIAL, 'grad_%s: median |ref| / scale %r: the bound would be vacuous' % (side, med)
        else:
            assert med is None
        assert row['err_' + side] <= row['bound_' + side], \
            'grad_%s: err %.3g of the scale, fp32 autograd %.3g, bound %.3g' % (side, row['err_' + side], row['autograd_err_' + side],
                                                                                row['bound_' + side])


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize('c', DENSE + WRAP + ZERO, ids=case_id)
def test_dense_parity_whatever_the_scratch_held(c):
    """premise; float64 parity of grad_ov and grad_su within the case's bound, exact zeros where an element has no term; finite
    although the scratch held NaN (an empty split is right only because its blocks still store a zero slab and a zero self
    term); no guard band touched, every element stored; same bits twice"""
    row, (gov, gsu), (gov2, gsu2) = measure(c)
    assert bool(torch.isfinite(gov).all()) and bool(torch.isfinite(gsu).all()), 'NaN from the scratch reached the result'
    assert_parity(row)
    assert same_bits(gov, gov2) and same_bits(gsu, gsu2)
    if c.gd == 'zero_rowcol':
        ex = exact(c)
        assert not ex['sc_ov'][c.Bo // 3].any() and not ex['sc_su'][c.Bs // 2].any() and ex['sc_ov'][0].all() and ex['sc_su'][0].all()
        assert not bool(gov[c.Bo // 3].any()) and not bool(gsu[c.Bs // 2].any())


@pytest.mark.parametrize('c', ONE_SIDED, ids=case_id)
def test_one_sided_calls_equal_the_two_sided_call(c):
    """grad_su = NULL and grad_ov = NULL (the sharded loss asks for one side at a time): the requested side bit for bit"""
    arena = Arena('cuda:0')
    check_premise(c)
    opnd = device_operands(c, arena)
    gov, gsu = launch_dense(c, arena, opnd)
    gov1, none_su = launch_dense(c, arena, opnd, want_su=False)
    none_ov, gsu1 = launch_dense(c, arena, opnd, want_ov=False)
    assert none_su is None and none_ov is None
    assert bool(gov.any()) and bool(gsu.any())
    assert same_bits(gov1, gov) and same_bits(gsu1, gsu)


def test_forward_outputs_plug_in():
    """orientation, score and workspace as ops.match_fwd leaves them: the reference and the yardstick are evaluated at the GPU's
    orientations, the bound is the same"""
    from witw_amd import ops
    c = REAL_USE
    ex = dict(exact(c))
    arena = Arena('cuda:0')
    ovd, sud = torch.from_numpy(np.array(ex['ov'])).cuda(), torch.from_numpy(np.array(ex['su'])).cuda()
    ori, _dist, score, ws = ops.match_fwd(ovd, sud, want_score=True, want_workspace=True)
    ex['ori'] = ori.cpu().numpy()
    assert ex['ori'].shape == (c.Bo, c.Bs) and ex['ori'].min() >= 0 and ex['ori'].max() < 64
    ref = R.match_bwd_ref(ex['ov'], ex['su'], ex['ori'], ex['gd'])
    ex.update(ref_ov=ref[0], ref_su=ref[1], sc_ov=ref[2], sc_su=ref[3])
    g_ov, g_su = autograd_f32(ex['ov'], ex['su'], ex['ori'], dense_blocks(ex['gd']))
    yard = R.err(g_ov, ex['ref_ov'], ex['sc_ov']), R.err(g_su, ex['ref_su'], ex['sc_su'])
    opnd = device_operands(c, arena)
    opnd.update(ori=arena.place(ori, 'ori'), score=arena.place(score, 'score'), ws=arena.place(ws[:c.Bo * 64 + c.Bs], 'ws'))
    gov, gsu = launch_dense(c, arena, opnd)
    assert_parity(row_of(c, ex, gov, gsu, yard))


@pytest.mark.parametrize('c', PAIRS, ids=case_id)
def test_pairs_parity_repeatable_and_zero_rows(c):
    """float64 parity of both gradients; two consecutive calls bit-identical (fixed order, no atomics); the rows no valid pair
    names exactly 0; no guard band touched, every element stored"""
    ex = exact(c)
    row, (gov, gsu), (gov2, gsu2) = measure(c)
    assert_parity(row, expect_terms=bool(ex['ok'].any()))
    assert same_bits(gov, gov2) and same_bits(gsu, gsu2)
    named_o, named_s = set(ex['po'][ex['ok']].tolist()), set(ex['ps'][ex['ok']].tolist())
    free_o, free_s = sorted(set(range(c.Bo)) - named_o), sorted(set(range(c.Bs)) - named_s)
    if free_o:
        assert not bool(gov[free_o].any())
    if free_s:
        assert not bool(gsu[free_s].any())
    if named_o:
        assert bool(gov[sorted(named_o)].flatten(1).any(dim=1).all()) and bool(gsu[sorted(named_s)].flatten(1).any(dim=1).all())
