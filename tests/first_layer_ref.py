"""float64 reference of the image entry path's first layer -- witw_conv3x3_first_fwd (csrc/conv_first.hip: the fp32 tile-per-workgroup
and persistent kernels, the split-fp16 store, the bf16 kernels of 4 and 8 values per pixel), the filter images of
witw_conv3x3_first_pack, and the inference form and layer-0 gate bits of csrc/conv_first2_bf16.hip -- on data where every kernel is
exact whatever its summation order, so that tests/test_first_layer_gpu.py compares bits. Built on tests/pool_ref.py (conv3x3, _pad,
_tern, first2_exact) and the encoders of tests/conv_epilogue_ref.py (f32_bits, bf16_bits, split_bits).

    z = conv3x3(x, w) + bias      zero rows above / below; zero or (circular) wrapped columns; stride 1; C -> 64 channels
    v = relu(z) or z              y = NHWC fp32 | bf16 = one rounding of v | split-fp16 hi = fp16(v), lo = fp16(v - hi)
    bf16 kernels: x and w are rounded to bf16 (nearest even) first, the bias is not; products and sums in fp32 (here: float64)

Data sets:

    ints     x, w in {-1, 0, 1} (pool_ref.first2_operands' densities), integer bias in [-2, 2]: every partial sum a small integer, exact
             in fp32 and bf16; a split output has lo = +0.0
    dyadic   x integers in [-8, 8], w in {0, +-1, +-2^-12}, bias an integer in [-2, 2] plus a multiple of 2^-12: every partial sum is a
             multiple of 2^-12 below 2^10, exact in fp32, and most outputs are not fp16 numbers: lo != 0
    round16  ternary x and w, each non-zero element times one factor of FACTORS = 1 + 2^-9 (below half a bf16 ulp: down), 1 - 2^-9
             (half an ulp of the binade BELOW 1: a tie, up to the even 1.0; truncation gives 1 - 2^-8), 1 + 2^-8 (a tie, down to the
             even 1.0), 1 + 2^-7 + 2^-8 (a tie, up to the even 1 + 2^-6); integer bias in [-6, 6]. The rounded operands are +-1 and
             +-(1 + 2^-6): products of two 8-bit significands, and at most 72 of them plus the bias stay below 2^7 in multiples of
             2^-12, exact in fp32, so the bf16 output is ONE rounding of the float64 sum. (The wider bias puts outputs in [4, 8),
             where a bf16 tie is an odd multiple of 2^-6 and a squared factor's 2^-12 sits above it: there a store that rounds
             through fp16 first differs.)

data() draws a case's operands from the first of 32 seeds under which the case meets the conditions that tests/test_first_layer_ref.py
asserts (shares of positive outputs, of lo != 0, of operands that change under rounding; every wrong variant that applies changes the
expected bits): the conditions are properties of the data alone, no kernel is consulted.

Batches: 2, or 'cu' = persist_batch(): the smallest batch whose tiles reach the persistent kernel's threshold of 4 tiles per compute
unit without being a multiple of its 2 workgroups per unit, so that workgroups walk unequal runs of tiles."""
import collections
import functools

import numpy as np
import torch

from tests import conv_epilogue_ref as E
from tests import pool_ref as P

NOMINAL_CU = 256
SHAPES = ((1, 1), (3, 12), (8, 64), (9, 65), (13, 99), (5, 130))
SPLIT_SHAPES = ((3, 12), (9, 65), (13, 99))
PERSIST_SHAPES = ((9, 66), (8, 130))
EDGE_SHAPE = (9, 65)            # one column short of the persistent kernel's bound: stays on the tile-per-workgroup kernel at any batch
FACTORS = (1.0 + 2.0 ** -9, 1.0 - 2.0 ** -9, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8)
TILE_KERNEL, PERSIST_KERNEL = 'conv3x3_first_kernel', 'conv3x3_first_persist_kernel'


# ================================================================================ the case table
_Key = collections.namedtuple('Key', 'row C H W data circ')


class Key(_Key):
    """row 'f32' (fp32 store), 'split' (split-fp16 store), 'persist', 'edge' ((9, 65) at the persistent batch), 'bf16' (either CW);
    one Key stands for two GPU cases, relu on and off, which share operands and z"""
    __slots__ = ()

    @property
    def id(self):
        return '%s-C%d-%dx%d-%s-%s' % (self.row, self.C, self.H, self.W, self.data, 'circ' if self.circ else 'zero')

    @property
    def big(self):
        return self.row in ('persist', 'edge')

    @property
    def tiles(self):
        return ((self.W + 63) // 64) * ((self.H + 7) // 8)

    def batch(self, cu=NOMINAL_CU):
        return persist_batch(PERSIST_SHAPES[0] if self.row == 'edge' else (self.H, self.W), cu) if self.big else 2

    def variant(self):
        if self.row == 'bf16':
            return 'conv3x3_first_bf16_kernel<%d>' % (4 if self.C <= 4 else 8)
        return PERSIST_KERNEL if self.row == 'persist' else TILE_KERNEL


def persist_batch(hw, cu):
    """the smallest B with B * tiles >= 4 * cu and (B * tiles) % (2 * cu) != 0"""
    tiles = ((hw[1] + 63) // 64) * ((hw[0] + 7) // 8)
    B = -(-4 * cu // tiles)
    while (B * tiles) % (2 * cu) == 0:
        B += 1
    return B


def _keys():
    out = []
    for circ in P.PADS:
        for data in ('ints', 'dyadic'):
            out += [Key('f32', C, H, W, data, circ) for C in (1, 2, 3, 4) for (H, W) in SHAPES]
            out += [Key('persist', C, H, W, data, circ) for C in (1, 2, 3, 4) for (H, W) in PERSIST_SHAPES]
        out += [Key('split', C, H, W, 'dyadic', circ) for C in (1, 3, 4) for (H, W) in SPLIT_SHAPES]
        out += [Key('edge', 3, EDGE_SHAPE[0], EDGE_SHAPE[1], 'dyadic', circ)]
        for data in ('ints', 'round16'):
            out += [Key('bf16', C, H, W, data, circ) for C in (1, 2, 3, 4, 5, 6, 7, 8) for (H, W) in SHAPES]
    return out


KEYS = _keys()
assert len({k.id for k in KEYS}) == len(KEYS)
RELUS = (True, False)


# ================================================================================ data
def round_bf16(a):
    """nearest-even rounding to bf16, by torch"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().double().numpy()


def trunc_bf16(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0xffff0000)
    return u.view(np.float32).astype(np.float64)


def operands(kind, seed, B, C, H, W):
    """-> x [B,C,H,W], w [64,C,3,3], b [64] float64, every value an fp32 number (what the kernel is handed)"""
    g = np.random.Generator(np.random.Philox(key=[seed, C * 100000 + H * W]))
    pw = min(0.5, 4.0 / (9.0 * C * 0.5))
    if kind == 'ints':
        x = P._tern(g, (B, C, H, W), 0.5)
        w = P._tern(g, (64, C, 3, 3), pw)
        b = g.integers(-2, 3, (64,)).astype(np.float64)
    elif kind == 'dyadic':
        x = g.integers(-8, 9, (B, C, H, W)).astype(np.float64)
        r, p1 = g.random((64, C, 3, 3)), min(0.4, 3.0 / (9.0 * C))      # +-1 with probability p1, +-2^-12 with 0.4, else 0
        w = (g.integers(0, 2, (64, C, 3, 3)) * 2 - 1) * np.where(r < p1, 1.0, np.where(r < p1 + 0.4, 2.0 ** -12, 0.0))
        b = g.integers(-2, 3, (64,)) + g.integers(-2048, 2049, (64,)) * 2.0 ** -12
    else:
        assert kind == 'round16'
        f = np.asarray(FACTORS)
        x = P._tern(g, (B, C, H, W), 0.5) * f[g.integers(0, 4, (B, C, H, W))]
        w = P._tern(g, (64, C, 3, 3), pw) * f[g.integers(0, 4, (64, C, 3, 3))]
        b = g.integers(-6, 7, (64,)).astype(np.float64)
    for t in (x, w, b):
        assert E.is_f32(t)
    return x, w, b


class Data(object):
    """read-only arrays of one Key: x, w, b as handed to the kernel; xr, wr as the kernel multiplies them (bf16 rows: rounded);
    z = conv + bias of the images sel (None: all), float64 NCHW"""

    def __init__(self, **kw):
        for k, v in kw.items():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
            setattr(self, k, v)


def nhwc(a):
    return np.ascontiguousarray(np.asarray(a).transpose(0, 2, 3, 1))


def relu(v):
    return np.where(v > 0, v, 0.0)


def encode(k, v_nchw, twice=False, swap=False):
    """the output's bit patterns, NHWC (split: [B,H,W,8,2,8]); twice: rounded fp32 -> fp16 -> bf16; swap: lo stored before hi"""
    v = nhwc(v_nchw)
    if k.row == 'bf16':
        if twice:
            v = v.astype(np.float16).astype(np.float64)
        return E.bf16_bits(v)
    if k.row == 'split':
        s = E.split_bits(v)
        return np.ascontiguousarray(s[..., ::-1, :]) if swap else s
    assert E.is_f32(v)
    return E.f32_bits(v)


def expected(k, d, on):
    return encode(k, relu(d.z) if on else d.z)


def _rounded(k, x, w):
    return (round_bf16(x), round_bf16(w)) if k.row == 'bf16' else (x, w)


def _seed(k, salt):
    s = salt
    for ch in '-'.join(str(t) for t in (k.C, k.H, k.W, k.data, int(k.circ))):          # rows share operands: the same image, every kernel
        s = (s * 131 + ord(ch)) % 1000003
    return s


def _build(k, cu, salt, n_sel):
    B = k.batch(cu)
    x, w, b = operands(k.data, _seed(k, salt), B, k.C, k.H, k.W)
    xr, wr = _rounded(k, x, w)
    sel = None if n_sel is None or n_sel >= B else tuple(range(n_sel))
    z = P.conv3x3(xr if sel is None else xr[list(sel)], wr, b, k.circ)
    return Data(x=x, w=w, b=b, xr=xr, wr=wr, z=z, sel=sel)


@functools.lru_cache(maxsize=4)
def data(k, cu=NOMINAL_CU, n_sel=None):
    """the case's operands and float64 answer; n_sel: only the first n_sel images are answered (the CPU test's look at a large batch --
    images are drawn independently, so what holds for two of them holds for the batch)"""
    salt = choose_salt(k)
    return _build(k, cu, salt, n_sel)


@functools.lru_cache(maxsize=None)
def choose_salt(k):
    """the first seed under which the case's first two images meet every condition (module docstring). Rows that differ only in
    the kernel they reach mostly choose the same seed, but need not."""
    for salt in range(32):
        d = _build(k, NOMINAL_CU, salt, 2)
        if not conditions(k, d) and not unchanged_variants(k, d):
            return salt
    raise AssertionError('no seed of 32 gives %s its conditions: %s %s' % (k.id, conditions(k, d), unchanged_variants(k, d)))


# ================================================================================ conditions (tests/test_first_layer_ref.py asserts them)
def shares(k, d):
    """the measured shares of one case"""
    out = {'positive': float((d.z > 0).mean())}
    if k.data == 'dyadic':
        for on in RELUS:
            s = E.split_bits(nhwc(relu(d.z) if on else d.z))
            out['lo_nonzero_relu%d' % on] = float(((s[..., 1, :] & 0x7fff) != 0).mean())
    if k.data == 'round16':
        ops_ = np.concatenate([d.x.ravel(), d.w.ravel()])
        nz = ops_[ops_ != 0]
        out['operands_changed'] = float((round_bf16(nz) != nz).mean())
        out['factors'] = [int((np.abs(nz) == f).sum()) for f in FACTORS]
    return out


def conditions(k, d):
    """-> the list of conditions the case misses (empty: none)"""
    s, bad = shares(k, d), []
    if not 0.30 <= s['positive'] <= 0.70:
        bad.append('positive share %.3f outside [0.30, 0.70]' % s['positive'])
    if k.data == 'dyadic' and min(s['lo_nonzero_relu1'], s['lo_nonzero_relu0']) < 0.30:
        bad.append('lo != 0 on %.3f / %.3f of the outputs < 0.30' % (s['lo_nonzero_relu1'], s['lo_nonzero_relu0']))
    if k.data == 'round16' and (s['operands_changed'] < 0.25 or min(s['factors']) == 0):
        bad.append('operands changed by rounding %.3f < 0.25, or a factor missing %s' % (s['operands_changed'], s['factors']))
    if not E.is_f32(d.z) or float(np.abs(d.z).max()) >= (2.0 ** 10 if k.data == 'dyadic' else P.MAX_ABS_Z):
        bad.append('z is not exact in fp32')
    return bad


# ================================================================================ wrong variants
def _swap_pairs(w):
    """taps 2i and 2i+1 exchanged, i = 0..3 (tap = 3 kh + kw)"""
    t = w.reshape(w.shape[0], w.shape[1], 9).copy()
    t[:, :, [0, 1, 2, 3, 4, 5, 6, 7]] = t[:, :, [1, 0, 3, 2, 5, 4, 7, 6]]
    return t.reshape(w.shape)


def _conv_wrap2(x, w, b):
    """circular, but the left halo column is taken from column W - 2"""
    B, _c, H, W = x.shape
    xp = P._pad(x, True)
    xp[:, :, 1:-1, 0] = x[:, :, :, W - 2]
    z = np.zeros((B, w.shape[0], H, W)) + b[None, :, None, None]
    for kh in range(3):
        for kw in range(3):
            z += np.einsum('bihw,oi->bohw', xp[:, :, kh:kh + H, kw:kw + W], w[:, :, kh, kw], optimize=True)
    return z


def layer0_variants(C, H, W, circ, x, w, b):
    """(name, z) of every wrong first-layer convolution that applies to the shape:
    transposed -- not on a 1 x 1 map under zero padding, where only the centre tap meets a pixel; tap 8 -- needs a row below;
    channel 3 -- needs one; the two wrap variants -- circular padding (and a second column to take the halo from)"""
    out = []
    if not (H == 1 and W == 1 and not circ):
        out.append(('taps kh/kw transposed', P.conv3x3(x, np.ascontiguousarray(w.transpose(0, 1, 3, 2)), b, circ)))
    if H > 1:
        w8 = w.copy()
        w8[:, :, 2, 2] = 0.0
        out.append(('tap 8 dropped', P.conv3x3(x, w8, b, circ)))
    out.append(('tap pairs (2i, 2i+1) swapped', P.conv3x3(x, _swap_pairs(w), b, circ)))
    if C >= 4:
        w3 = w.copy()
        w3[:, 3] = 0.0
        out.append(('channel 3 dropped', P.conv3x3(x, w3, b, circ)))
    if circ and W >= 2:
        out.append(('wrap taken from column W-2', _conv_wrap2(x, w, b)))
    if circ:
        out.append(('zero padding instead of wrap', P.conv3x3(x, w, b, False)))
    return out


VARIANT_NAMES = ('taps kh/kw transposed', 'tap 8 dropped', 'tap pairs (2i, 2i+1) swapped', 'channel 3 dropped', 'wrap taken from column W-2',
                 'zero padding instead of wrap', 'bias added after the ReLU', 'operands truncated to bf16', 'output rounded twice',
                 'hi and lo swapped', 'gate bit order reversed')


def wrong_variants(k, d, on):
    """(name, bit patterns) of every wrong variant that applies to the case with relu `on`.
    'output rounded twice' (fp32 -> fp16 -> bf16) needs an output in [4, 8) holding an odd multiple of 2^-6 plus a squared factor's
    2^-12: round16 data on more than one pixel (a 1 x 1 map sums at most 3 products per channel)."""
    xs = d.x if d.sel is None else d.x[list(d.sel)]
    xr = d.xr if d.sel is None else d.xr[list(d.sel)]
    fin = (lambda z: relu(z)) if on else (lambda z: z)
    out = [(n, encode(k, fin(z))) for n, z in layer0_variants(k.C, k.H, k.W, k.circ, xr, d.wr, d.b)]
    if on:
        out.append(('bias added after the ReLU', encode(k, relu(d.z - d.b[None, :, None, None]) + d.b[None, :, None, None])))
    if k.row == 'bf16' and k.data == 'round16':
        out.append(('operands truncated to bf16', encode(k, fin(P.conv3x3(trunc_bf16(xs), trunc_bf16(d.w), d.b, k.circ)))))
        if k.H * k.W > 1:
            out.append(('output rounded twice', encode(k, fin(d.z), twice=True)))
    if k.row == 'split':
        out.append(('hi and lo swapped', encode(k, fin(d.z), swap=True)))
    return out


def unchanged_variants(k, d):
    """the wrong variants that leave the expected bits of the case unchanged (must be empty)"""
    bad = []
    for on in RELUS:
        want = expected(k, d, on)
        bad += ['%s (relu %d)' % (n, on) for n, alt in wrong_variants(k, d, on) if np.array_equal(alt, want)]
    return bad


# ================================================================================ filter images of witw_conv3x3_first_pack
def pack_probe(C):
    """w [64,C,3,3]: 128 + n + 64 * (ch & 1) in the significand, the tap and ch >> 1 in the exponent: 576 C distinct bf16 numbers"""
    n, ch, tap = np.meshgrid(np.arange(64), np.arange(C), np.arange(9), indexing='ij')
    w = (128.0 + n + 64 * (ch & 1)) * 2.0 ** (tap + 9 * (ch >> 1) - 20)
    assert len(np.unique(w)) == w.size and np.array_equal(round_bf16(w), w)
    return w.reshape(64, C, 3, 3)


def pack_f32(w):
    """-> float64 [5,2,64,4]: wf[i][h][n][ch] = w[n][ch][tap 2i + h], zero for tap 9 and ch >= C"""
    C = w.shape[1]
    t = w.reshape(64, C, 9)
    out = np.zeros((5, 2, 64, 4))
    for i in range(5):
        for h in range(2):
            if 2 * i + h < 9:
                out[i, h, :, :C] = t[:, :, 2 * i + h]
    return out


def pack_bf16(w):
    """-> bf16 values as float64. C <= 4: [3,2,64,8], slot[i][h][n] = (w[n][0..3][tap 4i + 2h], w[n][0..3][tap 4i + 2h + 1]);
    C > 4: [5,2,64,8], slot[i][h][n] = w[n][0..7][tap 2i + h]; zero for taps >= 9 and channels >= C"""
    C = w.shape[1]
    t = round_bf16(w).reshape(64, C, 9)
    if C <= 4:
        out = np.zeros((3, 2, 64, 8))
        for i in range(3):
            for h in range(2):
                for e in range(2):
                    if 4 * i + 2 * h + e < 9:
                        out[i, h, :, 4 * e:4 * e + C] = t[:, :, 4 * i + 2 * h + e]
        return out
    out = np.zeros((5, 2, 64, 8))
    for i in range(5):
        for h in range(2):
            if 2 * i + h < 9:
                out[i, h, :, :C] = t[:, :, 2 * i + h]
    return out


# ================================================================================ the fused first two layers (csrc/conv_first2_bf16.hip)
def gate_bytes(mid_z, reverse=False):
    """layer 0's ReLU gate [B,64,H,W] -> uint8 [B,H,W,8]: bit c & 7 of byte c >> 3 = (value of channel c > 0)"""
    on = nhwc(mid_z > 0).astype(np.uint8)
    B, H, W, _c = on.shape
    on = on.reshape(B, H, W, 8, 8)
    sh = np.arange(8)[::-1] if reverse else np.arange(8)
    return (on << sh).sum(axis=-1).astype(np.uint8)


def first2_answers(shape, circ):
    """-> (pooled output as bf16 bit patterns NHWC, gate bytes) of pool_ref.first2_case"""
    c = P.first2_case(*shape, circ)
    return E.bf16_bits(nhwc(c.pooled)), gate_bytes(P.conv3x3_exact(c.x, c.w0, c.b0, circ))


def first2_wrong_variants(shape, circ):
    """(name, pooled bits, gate bytes) under every wrong layer 0 that applies, and the reversed bit order"""
    B, C, H, W = shape
    c = P.first2_case(*shape, circ)
    out = []
    for name, mid in layer0_variants(C, H, W, circ, c.x, c.w0, c.b0):
        pooled = P.pool_ref(P.conv3x3(relu(mid), c.w2, c.b2, circ))[0]
        out.append((name, E.bf16_bits(nhwc(pooled)) if float(np.abs(pooled).max()) <= 256 else None, gate_bytes(mid)))
    out.append(('gate bit order reversed', None, gate_bytes(P.conv3x3_exact(c.x, c.w0, c.b0, circ), reverse=True)))
    return out
