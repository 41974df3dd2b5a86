"""Data on which the match forward is EXACT, its float64 reference, and deliberately wrong forms of that reference (test
infrastructure of tests/test_match_exact_ref.py and tests/test_match_exact_gpu.py; CPU only).

Data. ov [Bo,16,4,64] and su [Bs,16,4,We] hold integers in [-4, 4] (flavour 'int'), or the same integers scaled by 2^-3 and
2^5 (flavour 'dyadic'). Every product and every partial sum of a score is then an integer (times 2^2) below 2^24 in magnitude
(|score| <= 4096 * 16), and so is every partial sum of a norm square (< 2^24, times 2^-6 / 2^10): v_mfma_f32_32x32x2f32, the
fma chain of the pair kernels, fp32 in any order and float64 all hold the same numbers. Orientation and score have one right
answer on every pair, exact ties included, and the distance is whatever the kernel's own fp32 epilogue makes of exact inputs.

Planted structure (plant(); as far as the batch has rows for it -- a 1 x 1 problem holds one pair):
  overhead rows   o % 7 == 2 and the LAST row: period 32 along the last axis (shifts s, s+32 tie: two accumulator tiles);
                  o % 7 == 4 (and row 0 of a one-row batch): period 16 (s, s+16, s+32, s+48 tie); row 1: all zero.
  surface rows    0, 1, 2: exact crops of overhead 0 at shifts 63, 0, 32; 3: all zero (64 scores of 0, orientation 0, 0/0 = NaN);
                  the LAST row: the crop of the last overhead row (period 32) at shift 31, so it ties 31 against 63 there.
The last rows take precedence over the numbered ones.

Reference (build() / decide()): scores[o,s,shift] = sum_{ch,k<We} ov[o,ch,(k+shift)%64] * su[s,ch,k] in float64 (one matmul per
shift; sums of integers below 2^53 are exact in any order), norm squares as float64 integers; orientation = first arg-max over
the shifts the query's mask word allows (a word of 0 = all), score = that maximum. The expected DISTANCE is the kernel's
epilogue restated in np.float32, rounded after every operation (the library is built with -ffp-contract=off and without
fast-math): wn = sqrt(f32(n2_window)), sn = sqrt(f32(n2_surface)), d = 2 * (1 - v / (wn * sn)).

Wrong variants (VARIANTS): the same functions with one kernel mistake each; tests/test_match_exact_ref.py proves that every
case can see every variant that applies to it.
"""
import collections
import contextlib

import numpy as np
import torch

SHIFTS = 64
CH = 64                      # 16 x 4 embedding rows
FLAVOURS = {'int': (0, 0), 'dyadic': (-3, 5)}      # powers of two on ov / su

Case = collections.namedtuple('Case', 'Bo Bs We generic form')


def dispatch(Bo, Bs, We, generic=False, masked=False):
    """match_fwd_launch (csrc/match.hip) restated: the kernel instantiation a shape reaches; `generic` = WITW_MATCH_GENERIC=1."""
    cdiv = lambda a, b: (a + b - 1) // b
    gx = cdiv(Bs, 128)
    m = 'true' if masked else 'false'
    pipelined = gx * cdiv(Bo, 4) >= 256 and not generic
    if pipelined and We >= 63:
        return 'match_kernel_w64<%s>' % m
    if pipelined:
        return 'match_kernel_rows<%d,%s>' % (4 if We <= 16 else 2 if We <= 32 else 1, m)
    if gx * cdiv(Bo, 4) >= 512:
        return 'match_kernel<2,2,%s>' % m
    if gx * cdiv(Bo, 2) >= 256:
        return 'match_kernel<1,2,%s>' % m
    if cdiv(Bs, 64) * cdiv(Bo, 2) >= 96:
        return 'match_kernel_nsplit<%d,%s>' % (16 if We <= 16 else 32 if We <= 32 else 64, m)
    return 'match_kernel<1,1,%s>' % m


def _case(Bo, Bs, We, generic=False):
    return Case(Bo, Bs, We, generic, dispatch(Bo, Bs, We, generic))


# all-pairs cases: the smallest shapes that reach each kernel form (the dispatch arithmetic above; 129 surfaces keep the
# 128-surface block edge and a ragged tail live, 510 / 1021 overheads a ragged last block of 2 / 1 overhead rows)
SMALL = [_case(1, 1, 64), _case(3, 200, 1), _case(70, 5, 63)]
NSPLIT = [_case(100, 77, w) for w in (12, 17, 33, 64)]
HALF = [_case(258, 129, 20)]
W64 = [_case(510, 129, 64), _case(510, 129, 63)]
ROWS = [_case(510, 129, w) for w in (1, 7, 16, 17, 32, 33, 62)]
GENERIC = [_case(510, 129, c.We, True) for c in W64 + ROWS]      # 2 * 128 = 256 workgroups < 512: match_kernel<1,2>
GENERIC22 = [_case(1021, 129, 33, True), _case(1021, 129, 64, True)]      # 2 * 256 = 512 workgroups: match_kernel<2,2>
CASES = SMALL + NSPLIT + HALF + W64 + ROWS + GENERIC + GENERIC22


def case_id(c):
    return '%dx%dx%d%s' % (c.Bo, c.Bs, c.We, '-generic' if c.generic else '')


# ----------------------------------------------------------------------------- data
def _rng(Bo, Bs, We, stream):
    return np.random.Generator(np.random.Philox(key=[(Bo << 20) + Bs, (We << 8) + stream]))


def plant(ov, su):
    """The planted structure of the module docstring, in place on integer-valued [Bo,64,64] / [Bs,64,We] arrays."""
    Bo, Bs, We = ov.shape[0], su.shape[0], su.shape[2]
    for o in range(Bo):
        if o % 7 == 2:
            ov[o, :, 32:] = ov[o, :, :32]
        if o % 7 == 4 or Bo == 1:
            ov[o] = np.tile(ov[o, :, :16], (1, 4))
    if Bo >= 3:
        ov[1] = 0
    if Bo > 1:
        ov[Bo - 1, :, 32:] = ov[Bo - 1, :, :32]
    crop = lambda o, shift: ov[o][:, (np.arange(We) + shift) % 64]
    for s, shift in ((0, 63), (1, 0), (2, 32)):
        if s < Bs - 1:
            su[s] = crop(0, shift)
    if 3 < Bs - 1:
        su[3] = 0
    su[Bs - 1] = crop(Bo - 1, 31)
    return ov, su


def make_data(Bo, Bs, We):
    """-> integer-valued float64 (ov [Bo,64,64], su [Bs,64,We]) with the planted structure."""
    g = _rng(Bo, Bs, We, 1)
    ov = g.integers(-4, 5, size=(Bo, CH, 64)).astype(np.float64)
    su = g.integers(-4, 5, size=(Bs, CH, We)).astype(np.float64)
    return plant(ov, su)


def as_f32(ov, su, flavour):
    """the fp32 embeddings the kernels get: [Bo,16,4,64] / [Bs,16,4,We], scaled by the flavour's powers of two (exact)"""
    eo, es = FLAVOURS[flavour]
    return (np.ascontiguousarray((ov * 2.0 ** eo).astype(np.float32).reshape(-1, 16, 4, 64)),
            np.ascontiguousarray((su * 2.0 ** es).astype(np.float32).reshape(su.shape[0], 16, 4, su.shape[2])))


# ----------------------------------------------------------------------------- masks and shift lists
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
UPPER = np.uint64(0xFFFFFFFF00000000)            # of two shifts s, s+32 that tie, only the higher one
ODD16 = np.uint64(0xFFFF0000FFFF0000)            # of s, s+16, s+32, s+48 only s+16 and s+48
MASK_SETS = ('win1', 'win2', 'win5', 'win33', 'mixed')


def _words(bit_lists):
    out = np.zeros(len(bit_lists), dtype=np.uint64)
    for i, bits in enumerate(bit_lists):
        for k in bits:
            out[i] |= np.uint64(1) << np.uint64(k)
    return out


def make_mask(Bo, Bs, We, name):
    """uint64 [Bs] mask words. 'winN': the N consecutive shifts (circular) from a start per query -- 16, 63, 0, 31 for the
    first four queries, random behind them. 'mixed', by s % 6: a word of 0, UPPER, a random word, all ones, ODD16, a sparse word
    of one to three bits (bit 63 among them on every other one)."""
    g = _rng(Bo, Bs, We, 2 + MASK_SETS.index(name))
    if name.startswith('win'):
        width = int(name[3:])
        starts = g.integers(0, 64, size=Bs)
        starts[:4] = np.array([16, 63, 0, 31])[:min(4, Bs)]
        return _words([[(int(a) + j) % 64 for j in range(width)] for a in starts])
    out = np.zeros(Bs, dtype=np.uint64)
    rnd = g.integers(0, 2 ** 64, size=Bs, dtype=np.uint64)
    for s in range(Bs):
        role = s % 6
        if role == 1:
            out[s] = UPPER
        elif role == 2:
            out[s] = rnd[s] if rnd[s] else ALL
        elif role == 3:
            out[s] = ALL
        elif role == 4:
            out[s] = ODD16
        elif role == 5:
            bits = [int(b) for b in g.integers(0, 64, size=int(g.integers(1, 4)))]
            out[s] = _words([bits + ([63] if (s // 6) % 2 else [])])[0]
    return out


def make_shifts(Bo, Bs, We, which):
    """int64 [Bs] shift list of the fixed form; `which` = 0 | 1 | 2. The multiset of shift & 63 holds groups of 65, 33 and 31
    queries (which = 0; shifts 63, 0, 32; with 162 queries or more also 32 and 1), of 32, 1 and 33 (which = 1; shifts 31, 63, 5)
    or of 129, 33, 65, 97, 31 and 32 (which = 2: supertiles of 128 rows with tails of 1 to 4 M-tiles), as far as Bs reaches,
    random other shifts behind them; the groups are interleaved over the batch (a random permutation) and every third entry is
    moved outside 0..63 by a multiple of 64 (negative ones included)."""
    g = _rng(Bo, Bs, We, 20 + which)
    plan = (((65, 63), (33, 0), (31, 32)), ((32, 31), (1, 63), (33, 5)),
            ((129, 63), (33, 0), (65, 32), (97, 31), (31, 5), (32, 7)))[which]
    vals = []
    for n, sh in plan:
        vals += [sh] * n
    if Bs >= 162 and which == 0:          # room for every size in one list
        vals += [31] * 32 + [7] * 1
    vals = vals[:Bs]
    used = set(v for v in vals)
    free = [k for k in range(64) if k not in used]
    vals += [free[int(i)] for i in g.integers(0, len(free), size=Bs - len(vals))]
    vals = np.array(vals, dtype=np.int64)[g.permutation(Bs)]
    vals[::3] += 64 * np.array([-1, 1, -3, 1000, 2, -1000])[np.arange(len(vals[::3])) % 6]
    return vals


def group_sizes(shift):
    return sorted(set(np.bincount(shift & 63, minlength=64).tolist()) - {0})


def fixed_rows_per_tile(Bo, Bs, cus=256):
    """witw_match_fwd_fixed restated: surfaces per supertile (32 * sm) on a chip of `cus` compute units"""
    cdiv = lambda a, b: (a + b - 1) // b
    sm = 4
    while sm > 1 and cdiv(Bs, 32 * sm) * cdiv(Bo, 128) < 2 * cus:
        sm >>= 1
    return 32 * sm


def fixed_tiles(shift, rows_per_tile):
    """the M-tile counts (fixed_tile<WP,MT>) of the supertiles fixed_group_kernel cuts the shift groups into"""
    mts = set()
    for c in np.bincount(shift & 63, minlength=64).tolist():
        for t in range(0, c, rows_per_tile):
            mts.add((min(rows_per_tile, c - t) + 31) // 32)
    return sorted(mts)


# the fixed form: (Bo, Bs, We, shift lists). The first four share data and scores with the all-pairs cases and reach
# match_fixed_kernel<16 | 32 | 64> with one M-tile per supertile (32-row supertiles: fixed_tile<WP,1>); the last three are
# large enough for 128-row supertiles on 256 compute units (cdiv(Bs,128) * cdiv(Bo,128) = 512) and reach fixed_tile<WP,1..4>.
FIXED = [(3, 200, 1, (0, 1)), (258, 129, 20, (0, 1)), (510, 129, 64, (0, 1)), (510, 129, 63, (0, 1))]
FIXED_BIG = [(1921, 3969, 12, (2,)), (1921, 3969, 17, (2,)), (1921, 3969, 33, (2,))]


# ----------------------------------------------------------------------------- wrong variants
VARIANTS = collections.OrderedDict([
    ('last_index_wins', 'an arg-max step compares >= : the LAST maximal shift wins a tie'),
    ('second_tile_wins', 'the merge of the two 32-shift accumulator tiles (or of the two shift-half waves) compares >= : a '
                         'maximum in shifts 32..63 wins against an equal one in 0..31'),
    ('wrap63', 'the window wraps at 63 instead of 64: column (k + shift) % 63'),
    ('pad_column_read', 'odd We: the pad column of Wp = (We + 1) & ~1 is not zeroed, the float behind the row is multiplied in'),
    ('mask_ignored', 'a mask word is ignored'),
    ('zero_word_forbids', 'a mask word of 0 is taken as "nothing allowed" instead of "no prior"'),
    ('forbidden_higher_wins', 'a forbidden lane gets its index + 64 but keeps its score: a higher forbidden score wins'),
    ('fixed_shift_raw', 'the fixed form does not take the shift & 63 where it writes orientation and looks the window norm up'),
    ('wnorm_we_plus_1', 'the window norm is taken over We + 1 columns'),
    ('wnorm_shift0', 'the window norm is taken at shift 0 instead of at the winning shift'),
    ('snorm_padded', 'odd We: the surface norm is taken over the padded width Wp, the float behind every row included'),
    ('ragged_neighbour', 'the last row of a ragged batch (surface and overhead) reads its neighbour'),
])


def applies(variant, Bo, Bs, We, mask=None, shift=None):
    """Whether the mistake can show at all on this shape / call form."""
    if variant in ('last_index_wins', 'second_tile_wins'):      # under masks: some word must allow two shifts 32 apart
        return shift is None and (mask is None or bool(np.any(allowed_bits(mask)[:, :32] & allowed_bits(mask)[:, 32:])))
    if variant in ('pad_column_read', 'snorm_padded'):
        return We % 2 == 1
    if variant in ('mask_ignored', 'forbidden_higher_wins') and (mask is None or not np.any((mask != 0) & (mask != ALL))):
        return False                            # no word forbids anything
    if variant == 'mask_ignored':
        return True
    if variant == 'forbidden_higher_wins':      # a one-row batch is its period-16 row: a maximum every 16 shifts, so a word has
        if mask is not None and Bo == 1:        # to forbid a whole residue class of 16 before a forbidden score can be higher
            bits = allowed_bits(mask).reshape(-1, 4, 16)
            return bool(np.any(~bits.any(axis=1)))
        return True
    if variant == 'zero_word_forbids':
        return mask is not None and bool(np.any(mask == 0))
    if variant == 'fixed_shift_raw':
        return shift is not None and bool(np.any((shift < 0) | (shift > 63)))
    if variant == 'wnorm_shift0':
        return We < 64              # a 64-column window is the whole row at every shift
    if variant == 'ragged_neighbour':
        return Bo > 1 or Bs > 1
    return True


# ----------------------------------------------------------------------------- reference
Base = collections.namedtuple('Base', 'sc n2w n2s We')      # scores [Bo,Bs,64], window / surface norm squares [Bo,64] / [Bs]


@contextlib.contextmanager
def _threads(n=16):
    prev = torch.get_num_threads()
    torch.set_num_threads(min(n, prev))
    try:
        yield
    finally:
        torch.set_num_threads(prev)


def _behind_row(su):
    """[Bs,64]: the float that lies behind each (surface, embedding row) in the contiguous tensor -- column We of that row; 0
    behind the very last row."""
    Bs, _, We = su.shape
    flat = np.append(su.reshape(-1), 0.0)
    return flat[(np.arange(Bs * CH) + 1) * We].reshape(Bs, CH)


def build(ov, su, variant=None, rows_o=None, rows_s=None, shift=None):
    """float64 scores and norm squares of the pairs rows_o x rows_s (default: all). `shift` (int64 [Bs]): only the score at
    shift[s] & 63 is formed, sc is [Bo,Bs,1] (the fixed form on problems too large for 64 scores per pair)."""
    ov, su = ov.copy(), su.copy()
    Bo, Bs, We = ov.shape[0], su.shape[0], su.shape[2]
    if variant == 'ragged_neighbour':
        if Bs > 1:
            su[Bs - 1] = su[Bs - 2]
        if Bo > 1:
            ov[Bo - 1] = ov[Bo - 2]
    pad = _behind_row(su)
    rows_o = np.arange(Bo) if rows_o is None else np.asarray(rows_o)
    rows_s = np.arange(Bs) if rows_s is None else np.asarray(rows_s)
    ov, su, pad = ov[rows_o], su[rows_s], pad[rows_s]
    mod = 63 if variant == 'wrap63' else 64
    if variant == 'pad_column_read':
        su = np.concatenate((su, pad[:, :, None]), axis=2)
    K = su.shape[2]
    sc = np.zeros((len(rows_o), len(rows_s), SHIFTS if shift is None else 1))
    with _threads():
        if shift is None:
            b = torch.from_numpy(np.ascontiguousarray(su.reshape(len(rows_s), CH * K).T))
            for sh in range(SHIFTS):
                a = np.ascontiguousarray(ov[:, :, (np.arange(K) + sh) % mod]).reshape(len(rows_o), CH * K)
                sc[:, :, sh] = (torch.from_numpy(a) @ b).numpy()
        else:
            t = (np.asarray(shift)[rows_s] & 63)
            for sh in np.unique(t):
                sel = np.nonzero(t == sh)[0]
                a = np.ascontiguousarray(ov[:, :, (np.arange(K) + sh) % mod]).reshape(len(rows_o), CH * K)
                b = torch.from_numpy(np.ascontiguousarray(su[sel].reshape(len(sel), CH * K).T))
                sc[:, sel, 0] = (torch.from_numpy(a) @ b).numpy()
    col = (ov * ov).sum(axis=1)                                    # [Bo,64] column energies
    width = We + 1 if variant == 'wnorm_we_plus_1' else We
    n2w = np.stack([col[:, (np.arange(width) + sh) % 64].sum(axis=1) for sh in range(SHIFTS)], axis=1)
    n2s = (su[:, :, :We] ** 2).sum(axis=(1, 2))
    if variant == 'snorm_padded' and We % 2 == 1:
        n2s = n2s + (pad ** 2).sum(axis=1)
    return Base(sc, n2w, n2s, We)


def flavoured(base, flavour):
    """The reference of the scaled flavour from the integer one: powers of two move through every sum exactly."""
    eo, es = FLAVOURS[flavour]
    if eo == 0 and es == 0:
        return base
    return Base(base.sc * 2.0 ** (eo + es), base.n2w * 4.0 ** eo, base.n2s * 4.0 ** es, base.We)


def allowed_bits(mask):
    """uint64 [Bs] -> bool [Bs,64]; a word of 0 allows every shift."""
    bits = ((mask[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    bits[mask == 0] = True
    return bits


def norms_f32(base):
    """the workspace the launch leaves: wn [Bo,64], sn [Bs] as correctly rounded fp32 roots of the exact norm squares"""
    return np.sqrt(base.n2w.astype(np.float32)), np.sqrt(base.n2s.astype(np.float32))


def distance_f32(v, n2w_sel, n2s):
    """The kernels' epilogue in np.float32, one rounding per operation: 2 * (1 - v / (sqrt(n2w) * sqrt(n2s)))."""
    with np.errstate(all='ignore'):
        wn = np.sqrt(n2w_sel.astype(np.float32))
        sn = np.sqrt(n2s.astype(np.float32))
        q = v.astype(np.float32) / (wn * sn[None, :])
        return np.float32(2) * (np.float32(1) - q)


Expected = collections.namedtuple('Expected', 'orientation score distance')


def decide(base, mask=None, shift=None, variant=None):
    """-> Expected(orientation int64 [Bo,Bs], score float64, distance float32) of match_fwd (mask: uint64 [Bs] or None) or of
    match_fwd_fixed (shift: int64 [Bs], any integers)."""
    sc, n2w = base.sc, base.n2w
    Bo, Bs = sc.shape[:2]
    if shift is not None:
        raw = np.broadcast_to(np.asarray(shift, dtype=np.int64)[None, :], (Bo, Bs))
        ori = raw & 63
        v = sc[:, :, 0] if sc.shape[2] == 1 else np.take_along_axis(sc, ori[:, :, None], 2)[:, :, 0]
        if variant == 'fixed_shift_raw':      # wn[og * 64 + shift] without the & 63, as far as the workspace reaches
            flat = np.clip(np.arange(Bo)[:, None] * 64 + raw, 0, Bo * 64 - 1)
            return Expected(raw.copy(), v, distance_f32(v, n2w.reshape(-1)[flat], base.n2s))
        at = np.zeros_like(ori) if variant == 'wnorm_shift0' else ori
        return Expected(ori.copy(), v, distance_f32(v, np.take_along_axis(n2w, at, 1), base.n2s))
    if mask is None or variant == 'mask_ignored':
        ok = np.ones((Bs, SHIFTS), dtype=bool)
    else:
        ok = allowed_bits(mask)
    if variant == 'forbidden_higher_wins':
        mx = sc.max(axis=-1)
        ismax = sc == mx[:, :, None]
        good = ismax & ok[None]
        ori = np.where(good.any(axis=-1), good.argmax(axis=-1), ismax.argmax(axis=-1))
    else:
        msc = np.where(ok[None], sc, -np.inf)
        mx = msc.max(axis=-1)
        ismax = msc == mx[:, :, None]
        ori = ismax.argmax(axis=-1)                                          # the first maximal index
        if variant == 'last_index_wins':
            ori = 63 - ismax[:, :, ::-1].argmax(axis=-1)
        elif variant == 'second_tile_wins':
            hi = ismax[:, :, 32:]
            ori = np.where(hi.any(axis=-1), 32 + hi.argmax(axis=-1), ori)
    ori = ori.astype(np.int64)
    v = mx.copy()
    if variant == 'zero_word_forbids' and mask is not None:      # 64 lanes of -inf and index + 64: shift 0 & 63 wins
        ori[:, mask == 0] = 0
        v[:, mask == 0] = -np.inf
    at = np.zeros_like(ori) if variant == 'wnorm_shift0' else ori
    return Expected(ori, v, distance_f32(v, np.take_along_axis(n2w, at, 1), base.n2s))


def differs(a, b):
    """bool [Bo,Bs]: pairs on which two Expected disagree in orientation, score or distance bits (NaN equals NaN)."""
    same_v = (a.score == b.score) | (np.isnan(a.score) & np.isnan(b.score))
    same_d = (a.distance.view(np.uint32) == b.distance.view(np.uint32)) | (np.isnan(a.distance) & np.isnan(b.distance))
    return (a.orientation != b.orientation) | ~same_v | ~same_d


def tie_stats(base, mask=None):
    """-> (pairs whose winner lies in shifts 0..31 with an equal allowed score in 32..63, pairs whose winner has an equal
    allowed score in its own half, pairs whose unmasked winner the mask forbids)."""
    ok = np.ones((base.sc.shape[1], SHIFTS), dtype=bool) if mask is None else allowed_bits(mask)
    msc = np.where(ok[None], base.sc, -np.inf)
    ismax = msc == msc.max(axis=-1)[:, :, None]
    win = ismax.argmax(axis=-1)
    lo, hi = ismax[:, :, :32].sum(axis=-1), ismax[:, :, 32:].sum(axis=-1)
    cross = (win < 32) & (hi > 0)
    within = np.where(win < 32, lo, hi) > 1
    free = base.sc.argmax(axis=-1)
    forbidden = ~ok[np.arange(base.sc.shape[1])[None, :], free]
    return int(cross.sum()), int(within.sum()), int(forbidden.sum())


def probe_rows(Bo, Bs, n_o=24, n_s=40):
    """Rows of a large case on which the CPU proof forms its variants: the planted rows, the block edges and both ends."""
    ro = sorted(set([o for o in list(range(n_o)) + [126, 127, 128, 129, Bo - 4, Bo - 3, Bo - 2, Bo - 1] if 0 <= o < Bo]))
    rs = sorted(set([s for s in list(range(n_s)) + [63, 64, 126, 127, 128, Bs - 2, Bs - 1] if 0 <= s < Bs]))
    return np.array(ro), np.array(rs)


# ----------------------------------------------------------------------------- rank counting on a distance matrix (numpy, IEEE)
def rank_count(D, true_offset=0):
    """#{o : D[o,q] <= D[q + true_offset, q]}; 0 where that row does not exist. A NaN compares false on either side."""
    Bo, Bs = D.shape
    t = np.arange(Bs) + true_offset
    ok = (t >= 0) & (t < Bo)
    with np.errstate(invalid='ignore'):
        dt = D[np.clip(t, 0, Bo - 1), np.arange(Bs)]
        return np.where(ok, (D <= dt[None, :]).sum(axis=0), 0).astype(np.int32)


def rank_count_thresh(D, thr):
    with np.errstate(invalid='ignore'):
        return (D <= thr[None, :]).sum(axis=0).astype(np.int32)


def rank_count_band(D, thr, eps):
    """-> (counts of d < thr - eps, the sorted (o, q) with thr - eps <= d <= thr + eps); the bounds in fp32 as the kernel forms them"""
    lo, hi = thr - np.float32(eps), thr + np.float32(eps)
    with np.errstate(invalid='ignore'):
        below = D < lo[None, :]
        band = ~below & (D <= hi[None, :])
    o, q = np.nonzero(band)
    return below.sum(axis=0).astype(np.int32), sorted(zip(o.tolist(), q.tolist()))
