"""float64 reference of the UNPOOLED conv3x3 launch -- witw_conv3x3_fwd_ex / _bf16_fwd_ex / _f16x3_fwd_ex, which is every forward layer
without a pool and, on the transposed and tap-rotated filter, the data gradient of every layer -- written from the definitions, on
data where every kernel is exact whatever its summation order, so that tests/test_conv_epilogue_gpu.py compares bits.

    forward:  z = conv3x3(x, w) + bias          zero rows above / below; zero or (circular) wrapped columns; stride (stride_h, 1)
              v = z * drop[b, c]                Dropout2d scale, 0 or 1.25
              v = act(v)                        none / ReLU / LeakyReLU(slope)
              v = v * post_scale[c] + post_shift[c]
              y = v where gate > 0, +0.0 elsewhere      a SELECT: -0.0, +0.0, negatives and NaN close the gate, and a closed output has
                                                        the bits of +0.0 also where v was negative, dropped or not finite
    dgrad:    dx[b, ci, sh*i + kh - 1, (j + kw - 1) mod-or-clip W] += dz[b, co, i, j] * w[co, ci, kh, kw]      the adjoint, as a scatter

The Dropout2d scale is applied before the activation. The opposite order is NOT among the wrong variants that
tests/test_conv_epilogue_ref.py tells apart: both scales are >= 0 and ReLU / LeakyReLU are positively homogeneous, act(s v) = s act(v)
for s >= 0, so the order does not change a value. (ReLU is `v if v > 0 else +0.0`: of a -0.0, which a negative value times the scale 0
is, it gives +0.0 -- IEEE 754-2019 maximum, and what v_max_f32 returns.)

Exact data: forward operands from pool_ref.exact_operands (x, w in {-1, 0, 1}, integer bias, |z| <= 128), gradients from
pool_ref.grad_ints (+-1 .. +-3) with ternary filters; drop in {0, 1.25}, slope 0.25, post_scale in {-0.5, 0.5, 1, 2}, post_shift a
small integer: every intermediate is a multiple of 2^-5 below 2^14, exact in fp32, and a bf16 / split-fp16 output is one rounding of
it (bf16_bits, split_bits). Gate tensors (gate_values) mix positives -- the smallest positive normal and subnormal of the gate's
format among them -- with +inf, negatives, +0.0, -0.0 and, in fp32, NaN (the 16-bit kernels' NaN gates: test_16bit_nan_gate_is_closed). A split-fp16 gate's sign lives in hi; an element with hi = +0.0 and
lo != 0 does not exist: hi = fp16(v) is zero only for |v| <= 2^-25, half the smallest subnormal, and then lo = fp16(v - 0) is the
same rounding of the same number, zero again.

The cases (CASES; shared by the CPU and the GPU tests) and the source location each reaches, witw_amd/csrc/:

    conv3x3.hip        `if (!POOL && !p.out_nchw && (p.Cout & 3) == 0)`: the LDS-slab store, gate as f32x4       store 'slab'
                       `else if (!POOL)` -> emit(): per-element stores, gate as a scalar at the NHWC offset         store 'generic' (Cout % 4 != 0)
                       the same, `if (p.out_nchw)` offset                                                           store 'nchw'
                       each under conv3x3_nhwc_f32_kernel<TN,SH,false,NW,GEO,9>, TN 64 / 128, SH 1 / 2, (NW, GEO) = (4,0), (8,0), (4,1: maps
                       of at most 32 columns), and <128,1,false,8,2,9> (zero-interleaved rows not multiplied) with its twin <..,8,0,9>
                       in_offset(): `if (p.dil_h)` rows, `if (p.circ)` columns                                      site 'dgrad' sh 2, circ
                       pack_weights_kernel(transpose_flip)                                                          sites 'dgrad', 'tflip'
    conv3x3_bf16.hip   conv3x3_nhwc_bf16_kernel<TN,SH,false,4 / 8>: `(p.Cout & 7) == 0` slab store with gate_open() on u16x8,
                       emit() for the fp32 NCHW map; conv3x3_bf16_s16_kernel<false,true>: flush()                   prec 'bf16'
    conv3x3_bf16_wres.hip  conv3x3_bf16_wres_kernel<gate>: gate_mask() (one case: the gated data gradient of a 64-channel layer)  flag 'wres'
    conv3x3_f16x3.hip  conv3x3_nhwc_f16x3_kernel<TN,SH,false,4 / 8>: store_split8() with the gate's hi plane, emit() prec 'f16'

A site 'tflip' case is a stride-2 launch on the transpose_flip packing (the gate and the scale on the SH = 2 instantiations); its
answer is forward() with the filter w_t[n, k, kh, kw] = w[k, n, 2 - kh, 2 - kw] that the packing is documented to build.
Batch 'cu' stands for one image per compute unit (the 8-wave bf16 / split-fp16 kernels start only where the grid fills the chip);
the answers then describe the images pool_ref.pick(B)."""
import collections
import functools

import numpy as np

from tests import pool_ref as P

SLOPE = 0.25
KEEP = 1.25
CAP = 2.0 ** 14
POST_SCALES = (-0.5, 0.5, 1.0, 2.0)
NOMINAL_CU = 256           # what 'cu' means without a device (tests/test_conv_epilogue_ref.py)


# ================================================================================ the operation
def conv(x, w, b, stride_h, circular):
    """z[b, co, i, j] = bias[co] + sum_{ci, kh, kw} Xpad[b, ci, stride_h * i + kh, j + kw] * w[co, ci, kh, kw], float64; Xpad = x with a
    zero row above and below and a zero (circular: wrapped) column left and right"""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    B, _c, H, W = x.shape
    Ho = (H - 1) // stride_h + 1
    xp = P._pad(x, bool(circular))
    z = np.zeros((B, w.shape[0], Ho, W), dtype=np.float64)
    if b is not None:
        z += np.asarray(b, dtype=np.float64)[None, :, None, None]
    with np.errstate(invalid='ignore'):
        for kh in range(3):
            for kw in range(3):
                rows = xp[:, :, kh:kh + stride_h * (Ho - 1) + 1:stride_h, kw:kw + W]
                z += np.einsum('bihw,oi->bohw', rows, w[:, :, kh, kw], optimize=True)
    return z


def relu(v):
    return np.where(v > 0, v, 0.0)


def lrelu(v, slope):
    return np.where(v > 0, v, v * slope)


def epilogue(z, drop=None, act='none', slope=SLOPE, post_scale=None, post_shift=None):
    """Dropout2d scale -> activation -> per-channel affine, of z = conv + bias"""
    v = z
    with np.errstate(invalid='ignore'):
        if drop is not None:
            v = v * drop[:, :, None, None]
        if act == 'relu':
            v = relu(v)
        elif act == 'lrelu':
            v = lrelu(v, slope)
        else:
            assert act == 'none'
        if post_scale is not None:
            v = v * post_scale[None, :, None, None] + post_shift[None, :, None, None]
    return v


def gate_select(v, gate):
    """v exactly where gate > 0, +0.0 everywhere else (a NaN gate compares false: closed)"""
    if gate is None:
        return v
    with np.errstate(invalid='ignore'):
        return np.where(gate > 0, v, 0.0)


def forward(x, w, b, stride_h, circular, drop=None, act='none', slope=SLOPE, post_scale=None, post_shift=None, gate=None):
    return gate_select(epilogue(conv(x, w, b, stride_h, circular), drop, act, slope, post_scale, post_shift), gate)


def dgrad(dz, w, in_hw, stride_h, circular):
    """the adjoint of conv at x: dz [B,Co,Ho,W], w [Co,Ci,3,3] -> dx [B,Ci,H,W], every product scattered to the input it came from"""
    dz, w = np.asarray(dz, dtype=np.float64), np.asarray(w, dtype=np.float64)
    H, W = in_hw
    B, _co, Ho, Wz = dz.shape
    assert Wz == W and Ho == (H - 1) // stride_h + 1
    dx = np.zeros((B, w.shape[1], H, W), dtype=np.float64)
    with np.errstate(invalid='ignore'):
        for kh in range(3):
            for kw in range(3):
                t = np.einsum('bohw,oi->bihw', dz, w[:, :, kh, kw], optimize=True)      # [B,Ci,Ho,W]: lands at (sh*i + kh - 1, j + kw - 1)
                for i in range(Ho):
                    r = stride_h * i + kh - 1
                    if not 0 <= r < H:
                        continue
                    for j in range(W):
                        c = j + kw - 1
                        if circular:
                            c %= W
                        elif not 0 <= c < W:
                            continue
                        dx[:, :, r, c] += t[:, :, i, j]
    return dx


def flipped(w):
    """w [K,N,3,3] -> w_t [N,K,3,3], w_t[n, k, kh, kw] = w[k, n, 2 - kh, 2 - kw]: what transpose_flip packs"""
    return np.ascontiguousarray(np.asarray(w).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


# ================================================================================ output encoders (arrays in any layout)
def f32_bits(v):
    f = np.asarray(v, dtype=np.float64).astype(np.float32)
    return np.ascontiguousarray(f).view(np.int32)


def is_f32(v):
    """the fp32 round trip of v is the identity (NaN counts as itself)"""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return bool(np.all((v.astype(np.float32).astype(np.float64) == v) | np.isnan(v)))


def bf16_bits(v):
    """one round-to-nearest-even of the exact (fp32-representable) value to bf16; an infinity (of a gate) is itself"""
    assert is_f32(v) and not np.isnan(v).any()
    u = np.ascontiguousarray(np.asarray(v, dtype=np.float64).astype(np.float32)).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16).view(np.int16)


def split_bits(v_nhwc):
    """[.., C] -> split-fp16 [.., C/8, 2, 8]: hi = fp16(v), lo = fp16(v - hi); an infinity (of a gate) is hi = inf, lo = 0"""
    v = np.asarray(v_nhwc, dtype=np.float64)
    inf = np.isinf(v)
    assert v.shape[-1] % 8 == 0 and float(np.abs(np.where(inf, 0.0, v)).max(initial=0.0)) <= 65504.0
    hi = v.astype(np.float16)
    lo = np.where(inf, 0.0, v - np.where(inf, 0.0, hi.astype(np.float64))).astype(np.float16)
    out = np.empty(v.shape[:-1] + (v.shape[-1] // 8, 2, 8), dtype=np.int16)
    out[..., 0, :] = hi.view(np.int16).reshape(v.shape[:-1] + (-1, 8))
    out[..., 1, :] = lo.view(np.int16).reshape(v.shape[:-1] + (-1, 8))
    return out


# ================================================================================ data
# smallest positive normal and subnormal of the gate's format; fp32 gates also hold NaN
GATE_FORMATS = {'f32': (2.0 ** -126, 2.0 ** -149), 'bf16': (2.0 ** -126, 2.0 ** -133), 'f16': (2.0 ** -14, 2.0 ** -24)}
GATE_KINDS = ('positive', 'min_normal', 'min_subnormal', 'negative', 'plus_zero', 'minus_zero', 'nan', 'plus_inf')
GATE_OPEN = (0, 1, 2, 7)


def gate_kinds(prec):
    """the kinds a gate of this format holds (NaN: fp32 only; the 16-bit kernels' NaN has a test of its own)"""
    return tuple(q for q in range(8) if q != 6 or prec == 'f32')


def gate_values(seed, shape, prec):
    """-> (gate float64, kind uint8 indexing GATE_KINDS), half open and half closed. Every value is a number of the format: fp32 any
    multiple of 2^-10 below 2^10, bf16 8 significant bits, split-fp16 14 significant bits in [0.5, 2) (so that lo != 0, either sign)"""
    g = np.random.Generator(np.random.Philox(key=[seed, 4242]))
    slot = g.integers(0, 16, shape)
    kind = np.select([slot < 5, slot == 5, slot == 6, slot == 7, slot < 11, slot < 13, slot < 15], [0, 7, 1, 2, 3, 4, 5], 6 if prec == 'f32' else 3)
    if prec == 'f32':
        mag = g.integers(1, 2 ** 20, shape) * 2.0 ** -10
    elif prec == 'bf16':
        mag = g.integers(1, 256, shape) * 2.0 ** -4
    else:
        mag = g.integers(2 ** 12, 2 ** 14, shape) * 2.0 ** -13
    normal, sub = GATE_FORMATS[prec]
    gate = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5], [mag, normal, sub, -mag, 0.0, -0.0], np.nan)
    gate = np.where(kind == 7, np.inf, gate)
    return gate, kind.astype(np.uint8)


def drop_scales(seed, B, C):
    """[B,C] in {0, 1.25}: a quarter of each image's channels (at least one) dropped, the rest kept"""
    g = np.random.Generator(np.random.Philox(key=[seed, 99]))
    d = np.full((B, C), KEEP)
    for b in range(B):
        d[b, g.permutation(C)[:max(1, C // 4)]] = 0.0
    return d


def post_affine(seed, C):
    g = np.random.Generator(np.random.Philox(key=[seed, 55]))
    return np.asarray(POST_SCALES)[g.integers(0, 4, C)], g.integers(-2, 3, C).astype(np.float64)


# ================================================================================ the case table
_Case = collections.namedtuple('Case', 'prec site B H W cin cout sh out_h circ store drop act post gate nw flags')


class Case(_Case):
    """prec 'f32' / 'bf16' / 'f16'; site 'fwd' (x [B,cin,H,W] -> [B,cout,Ho,W], stride sh), 'tflip' (the same on the transpose_flip
    packing of w [cin,cout,3,3]) or 'dgrad' (dz [B,cin,Hz,W] -> dx [B,cout,H,W] of a stride-sh conv with w [cin,cout,3,3]; sh = 2 is the
    zero-interleaved launch, out_h = H); store 'slab' / 'generic' / 'nchw'; nw: waves asked of the fp32 launcher; flags: 'dilskip0'
    (witw_conv3x3_dil_skip(0)), 'mfma16off' / 's16' (witw_conv3x3_bf16_mfma16), 'wres' (the weight-resident kernel must take it)"""
    __slots__ = ()

    @property
    def id(self):
        sw = ''.join(k for k, on in (('D', self.drop), ('P', self.post), ('G', self.gate)) if on)
        return '-'.join(str(t) for t in (self.prec, self.site, '%sx%dx%d' % (self.B, self.H, self.W), '%dto%d' % (self.cin, self.cout),
                                         's%d' % self.sh, 'circ' if self.circ else 'zero', self.store, self.act + sw,
                                         'nw%s' % self.nw) + tuple(self.flags))

    def batch(self, cu=NOMINAL_CU):
        return cu if self.B == 'cu' else self.B

    @property
    def big(self):
        """a batch that fills the chip: only the images pool_ref.pick(B) are compared"""
        return self.B == 'cu' or self.B > 8

    @property
    def dilated(self):
        return self.site == 'dgrad' and self.sh == 2

    @property
    def launch_sh(self):
        return 1 if self.site == 'dgrad' else self.sh

    def variant(self):
        """the kernel instantiation the launcher must pick, as witw_last_kernel_variant() spells it"""
        tn = 128 if self.cout >= 128 else 64
        if self.prec == 'f32':
            if self.W <= 32:
                nw, geo = 4, 1          # narrow geometry: 4 waves whatever is asked
            else:
                nw = self.nw
                geo = 2 if (self.dilated and tn == 128 and nw == 8 and 'dilskip0' not in self.flags) else 0
            return 'conv3x3_nhwc_f32_kernel<%d,%d,false,%d,%d,9>' % (tn, self.launch_sh, nw, geo)
        if 's16' in self.flags:
            return 'conv3x3_bf16_s16_kernel<false,true>'
        if 'wres' in self.flags:
            return 'conv3x3_bf16_wres_kernel<gate>'
        name = 'conv3x3_nhwc_bf16_kernel' if self.prec == 'bf16' else 'conv3x3_nhwc_f16x3_kernel'
        return '%s<%d,%d,false,%d>' % (name, tn, self.launch_sh, 8 if self.big else 4)


def _case(prec, site, hw, cin, cout, sh=1, circ=False, store='slab', drop=False, act='relu', post=False, gate=False, nw=None, flags=(),
          B=2):
    H, W = hw
    if site == 'dgrad':
        act = 'none'
    return Case(prec, site, B, H, W, cin, cout, sh, H if (site == 'dgrad' and sh == 2) else None, bool(circ), store, drop, act, post, gate,
                nw, tuple(flags))


WIDE = ((5, 33), (8, 64), (9, 70), (13, 130))
NARROW = ((1, 1), (2, 17), (5, 12), (17, 32))
# dilated launches: out_h = 2 Hp - 1 and 2 Hp, each under both paddings
DIL_WIDE = (((5, 33), False), ((5, 33), True), ((8, 64), False), ((8, 64), True))
DIL_NARROW = (((5, 12), False), ((5, 12), True), ((2, 17), False), ((2, 17), True))


class _Cycle(object):
    def __init__(self, items):
        self.items, self.k = tuple(items), 0

    def __call__(self):
        self.k += 1
        return self.items[(self.k - 1) % len(self.items)]


def _fp32_cases():
    """every unpooled 9-tap instantiation x {plain, scale, LeakyReLU + affine, NCHW, ragged Cout, gated NCHW, gated ragged, gated dgrad /
    tflip, dilated gated dgrad}. Cout 134 is the ragged count of the 128-channel tile (70 cannot reach it)."""
    out = []
    for tn in (64, 128):
        for sh in (1, 2):
            for nw, geo in ((4, 0), (8, 0), (4, 1)):
                shape, cin, circ = _Cycle(NARROW if geo else WIDE), _Cycle((8, 24, 64)), _Cycle((False, True))
                cout = _Cycle((16, 64, 72) if tn == 64 else (128, 200))
                ragged = 70 if tn == 64 else 134
                ask = 8 if geo else nw          # narrow: 8 waves are asked for and 4 run
                mk = functools.partial(_case, 'f32', sh=sh, nw=ask)
                out.append(mk('fwd', shape(), cin(), cout(), circ=circ()))
                out.append(mk('fwd', shape(), cin(), cout(), circ=circ(), drop=True))
                out.append(mk('fwd', shape(), cin(), cout(), circ=circ(), act='lrelu', post=True))
                out.append(mk('fwd', shape(), cin(), cout(), circ=circ(), store='nchw'))
                out.append(mk('fwd', shape(), cin(), ragged, circ=circ(), store='generic', drop=True))
                out.append(mk('fwd', shape(), cin(), cout(), circ=circ(), store='nchw', drop=True, act='lrelu', gate=True))
                out.append(mk('fwd', shape(), cin(), ragged, circ=circ(), store='generic', act='none', post=True, gate=True))
                sq = 64 if tn == 64 else 128
                if sh == 1:
                    out.append(mk('dgrad', shape(), sq if tn == 64 else 24, sq, circ=circ(), drop=True, gate=True))
                    for hw, c in (DIL_NARROW if geo else DIL_WIDE):
                        if tn == 128 and nw == 8 and not geo:      # <128,1,false,8,2,9>, and its twin under dil_skip(0)
                            out.append(_case('f32', 'dgrad', hw, cin(), cout(), sh=2, circ=c, drop=True, gate=True, nw=ask))
                            out.append(_case('f32', 'dgrad', hw, out[-1].cin, out[-1].cout, sh=2, circ=c, drop=True, gate=True, nw=ask,
                                             flags=('dilskip0',)))
                        else:
                            out.append(_case('f32', 'dgrad', hw, cin(), cout(), sh=2, circ=c, drop=True, gate=True, nw=ask))
                else:
                    out.append(mk('tflip', shape(), sq if tn == 64 else 24, sq, circ=circ(), drop=True, act='none', gate=True))
    return out


def _low_cases(prec):
    """bf16 / split-fp16: the 4-wave instantiations at B = 2, the 8-wave ones at one image per CU"""
    bf = prec == 'bf16'
    out = []
    for tn in (64, 128):
        for sh in (1, 2):
            shape, circ = _Cycle((WIDE[2], NARROW[2], WIDE[0], NARROW[3], WIDE[3], NARROW[1], WIDE[1])), _Cycle((False, True))
            cin = _Cycle((16, 48, 64) if bf else (8, 24, 64))
            cout = _Cycle(((16, 64) if bf else (16, 64, 72)) if tn == 64 else ((128,) if bf else (128, 200)))
            mk = functools.partial(_case, prec, sh=sh)
            out.append(mk('fwd', shape(), cin(), cout(), circ=circ(), drop=True))
            for co in ((16, 72) if tn == 64 else (200,)):
                out.append(mk('fwd', shape(), cin(), co, circ=circ(), store='nchw', drop=True))
            if sh == 1:
                out.append(mk('dgrad', shape(), 64 if tn == 64 else cin(), 64 if tn == 64 else cout(), circ=circ(), drop=True, gate=True))
                out.append(mk('dgrad', NARROW[0], cin(), tn if bf else (72 if tn == 64 else 200), circ=True, drop=True, gate=True))
                for hw, c in DIL_WIDE[:2] + DIL_NARROW[2:] + DIL_WIDE[2:3] + DIL_NARROW[1:2]:
                    out.append(_case(prec, 'dgrad', hw, cin(), cout(), sh=2, circ=c, drop=True, gate=True))
            else:
                out.append(mk('tflip', shape(), cin(), cout(), circ=circ(), drop=True, act='none', gate=True))
            # 8 waves: Ho % 8 == 0 and a grid that fills its last round of workgroups -> one image per CU, 8 x 64 outputs each
            big = functools.partial(_case, prec, B='cu', cin=32, cout=tn, flags=('mfma16off',) if (bf and tn == 128 and sh == 1) else ())
            out.append(big('fwd', (8 * sh, 64), sh=sh, circ=circ(), drop=True))
            if sh == 1:
                out.append(big('dgrad', (8, 64), sh=1, circ=circ(), drop=True, gate=True))
                out.append(big('dgrad', (8, 64), sh=2, circ=circ(), drop=True, gate=True))
            else:
                out.append(big('tflip', (16, 64), sh=2, circ=circ(), drop=True, act='none', gate=True))
    if bf:
        out.append(_case('bf16', 'dgrad', (8, 64), 32, 128, sh=2, circ=True, drop=True, gate=True, B='cu', flags=('s16',)))
        # the weight-resident kernel takes a gated stride-1 launch of 64 input channels without a Dropout2d scale once 8192 (8 x 16 tile,
        # 64-channel block) units fill it: 256 images x 4 tiles x 8 blocks is the smallest such launch on an 8 x 64 map
        out.append(_case('bf16', 'dgrad', (8, 64), 64, 512, sh=1, circ=True, gate=True, B=256, flags=('wres',)))
    return out


CASES = _fp32_cases() + _low_cases('bf16') + _low_cases('f16')
assert len({c.id for c in CASES}) == len(CASES)


# ================================================================================ operands and answers of a case
class Data(object):
    """read-only numpy arrays of one case, all NCHW float64: x (the launch's input: x or dz), w, b (None: no bias), drop, post_scale,
    post_shift, gate, gate_kind, z (conv + bias, or the plain dgrad), ungated (before the gate), want (the answer); sel = the images
    that z / ungated / want / gate describe (None: all)"""

    def __init__(self, **kw):
        for k, v in kw.items():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
            setattr(self, k, v)


def _seed(c):
    s = 0
    for ch in c.id:
        s = (s * 131 + ord(ch)) % 1000003
    return s


@functools.lru_cache(maxsize=None)
def case_data(c, cu=NOMINAL_CU):
    seed = _seed(c)
    B = c.batch(cu)
    sel = tuple(P.pick(B)) if c.big else None
    g = np.random.Generator(np.random.Philox(key=[seed, 7]))
    if c.site == 'dgrad':
        Hz = (c.H - 1) // c.sh + 1
        x = P.grad_ints(seed, (B, c.cin, Hz, c.W))
        w = P._tern(g, (c.cin, c.cout, 3, 3), min(0.5, 5.0 / (9.0 * c.cin)))
        b = None
    elif c.site == 'tflip':
        x = P._tern(g, (B, c.cin, c.H, c.W), 0.25)
        w = P._tern(g, (c.cin, c.cout, 3, 3), min(0.5, 5.0 / (9.0 * c.cin * 0.25)))
        b = None
    else:
        x, w, b = P.exact_operands(seed, B, c.cin, c.cout, c.H, c.W)
    xs = x if sel is None else x[list(sel)]
    if c.site == 'dgrad':
        z = dgrad(xs, w, (c.H, c.W), c.sh, c.circ)
    else:
        z = conv(xs, flipped(w) if c.site == 'tflip' else w, b, c.sh, c.circ)
        assert float(np.abs(z).max()) <= P.MAX_ABS_Z
    drop = drop_scales(seed, B, c.cout) if c.drop else None
    ps, pt = post_affine(seed, c.cout) if c.post else (None, None)
    ungated = epilogue(z, None if drop is None else (drop if sel is None else drop[list(sel)]), c.act, SLOPE, ps, pt)
    gate = kind = None
    if c.gate:
        # the first seed whose every kind of gate value meets a non-zero output (a 1 x 1 map holds few elements)
        for salt in range(64):
            gate, kind = gate_values(seed + 7919 * salt, ungated.shape, c.prec)
            if all(((kind == q) & (ungated != 0)).any() for q in gate_kinds(c.prec)):
                break
    return Data(x=x, w=w, b=b, drop=drop, post_scale=ps, post_shift=pt, gate=gate, gate_kind=kind, z=z, ungated=ungated,
                want=gate_select(ungated, gate), sel=sel)
