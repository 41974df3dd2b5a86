"""float64 restatement of witw_conv3x3_bf16_fwd_taps4 (include/witw_hip.h) and of the bf16 eval forward of cvig_baseline's encoders
(SurfaceEncoder(precision='bf16')): the arithmetic in float64, rounded to bf16 (nearest-even) at exactly the points the product
rounds -- the filters of blocks 2-4 at pack time, the outputs of blocks 1-3 at the store -- and nowhere else. Knows nothing of
witw_amd. `variant` names one deliberately WRONG kernel (tests/test_baseline_bf16_ref.py proves the exact cases tell each from the
right one)."""
import numpy as np

TN = 128        # output channels per packed filter tile (the documented layout of witw_conv3x3_bf16_pack_weights_taps4)

VARIANTS = ('affine_first', 'bias_last', 'taps_transposed', 'taps_01', 's2d_swapped', 'valid_h+1', 'valid_h-1', 'valid_w+1', 'valid_w-1',
            'nonzero_outside', 'double_round', 'trunc_filters')


def bf16_round(a):
    """float64 -> the nearest bf16 value (8 significant bits, ties to even), as float64; normal range only"""
    a = np.asarray(a, dtype=np.float64)
    m, e = np.frexp(a)
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)


def bf16_trunc(a):
    """towards zero instead"""
    a = np.asarray(a, dtype=np.float64)
    m, e = np.frexp(a)
    return np.ldexp(np.trunc(m * 256.0) / 256.0, e)


def bf16_half_up(a):
    """a store that reaches bf16 'via a truncation': half an ulp added to the magnitude of the fp32 value, the low 16 bits cut off.
    Rounds a second time where nearest-even had already decided: every tie goes away from zero."""
    bits = np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = ((bits + 0x8000) >> 16) << 16
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


def bf16_bits(a):
    """the uint16 pattern of values that are bf16 numbers"""
    f = np.ascontiguousarray(a, dtype=np.float32)
    assert np.array_equal(f.astype(np.float64), np.asarray(a, dtype=np.float64)), 'not fp32 values'
    b = f.view(np.uint32)
    assert not (b & 0xffff).any(), 'not bf16 values'
    return (b >> 16).astype(np.uint16)


def f32_bits(a):
    f = np.ascontiguousarray(a, dtype=np.float32)
    assert np.array_equal(f.astype(np.float64), np.asarray(a, dtype=np.float64)), 'not fp32 values'
    return f.view(np.uint32)


def pack_taps4(k3, variant=None):
    """[cout][cin][3][3] -> the bf16 image wpk[nt][kc][tap = ty*2+tx][g][n][j] = bf16(k3[nt*128 + n][kc*16 + g*8 + j][1+ty][1+tx]),
    zeros past cout / cin, as float64 of shape [nt, kc, 4, 2, 128, 8]"""
    k3 = np.asarray(k3, dtype=np.float64)
    co, ci = k3.shape[:2]
    nt, nkc = -(-co // TN), -(-ci // 16)
    w = np.zeros((nt * TN, nkc * 16, 2, 2))
    w[:co, :ci] = k3[:, :, 1:3, 1:3]
    w = bf16_trunc(w) if variant == 'trunc_filters' else bf16_round(w)
    return w.reshape(nt, TN, nkc, 2, 8, 4).transpose(0, 2, 5, 3, 1, 4)


def taps4_filter(k3, variant=None, rounding=True):
    """the [cout][cin][2][2] filter the kernel multiplies by: tap (ty, tx) = k3[.., 1+ty, 1+tx], rounded once"""
    k3 = np.asarray(k3, dtype=np.float64)
    w = k3[:, :, 0:2, 0:2] if variant == 'taps_01' else k3[:, :, 1:3, 1:3]
    if variant == 'taps_transposed':
        w = w.transpose(0, 1, 3, 2)
    if not rounding:
        return w
    return bf16_trunc(w) if variant == 'trunc_filters' else bf16_round(w)


def preact(x, k3, bias, variant=None, rounding=True):
    """conv + bias over the whole H x W map: [B,H,W,Cout] (x zero past H / W)"""
    x = np.asarray(x, dtype=np.float64)
    B, H, W, C = x.shape
    w = taps4_filter(k3, variant, rounding)
    xp = np.zeros((B, H + 1, W + 1, C))
    xp[:, :H, :W] = x
    out = np.zeros((B, H, W, w.shape[0]))
    for ty in range(2):
        for tx in range(2):
            out += (xp[:, ty:ty + H, tx:tx + W].reshape(-1, C) @ w[:, :, ty, tx].T).reshape(B, H, W, -1)
    return out + np.asarray(bias, dtype=np.float64)


def l1_bound(x, k3, bias):
    """max over the outputs of sum |x| |w| + |bias|: no partial sum of any order exceeds it"""
    return float(preact(np.abs(x), np.abs(np.asarray(k3, dtype=np.float64)), np.abs(bias), rounding=False).max())


PREACT_VARIANTS = ('taps_transposed', 'taps_01', 'bias_last', 'trunc_filters')      # the variants that change conv + bias itself


def conv_taps4(x, k3, bias, slope, scale, shift, valid_hw, out_f32=False, variant=None, rounding=True, pre=None):
    """-> [B, ceil(vh/2), ceil(vw/2), 4*Cout] float64: the values witw_conv3x3_bf16_fwd_taps4 stores. pre: conv + bias of this
    variant, if the caller has it already"""
    vh, vw = valid_hw
    bias = np.asarray(bias, dtype=np.float64)
    if pre is not None:
        v = pre
    elif variant == 'bias_last':
        v = preact(x, k3, np.zeros_like(bias), variant, rounding)
    else:
        v = preact(x, k3, bias, variant, rounding)
    B, H, W, N = v.shape

    def lrelu(t):
        return np.where(t > 0, t, t * slope)

    def affine(t):
        return t if scale is None else t * np.asarray(scale, dtype=np.float64) + np.asarray(shift, dtype=np.float64)

    if variant == 'affine_first':
        v = lrelu(affine(v))
    elif variant == 'bias_last':
        v = affine(lrelu(v)) + bias
    else:
        v = affine(lrelu(v))
    if rounding and not out_f32:
        v = bf16_half_up(v) if variant == 'double_round' else bf16_round(v)
    h2, w2 = (vh + 1) // 2, (vw + 1) // 2
    mh = vh + (variant == 'valid_h+1') - (variant == 'valid_h-1')
    mw = vw + (variant == 'valid_w+1') - (variant == 'valid_w-1')
    full = np.zeros((B, 2 * h2, 2 * w2, N))
    ch, cw = min(H, 2 * h2), min(W, 2 * w2)
    full[:, :ch, :cw] = v[:, :ch, :cw]
    if variant != 'nonzero_outside':
        full[:, mh:] = 0.
        full[:, :, mw:] = 0.
    y = full.reshape(B, h2, 2, w2, 2, N)
    y = y.transpose(0, 1, 3, 4, 2, 5) if variant == 's2d_swapped' else y.transpose(0, 1, 3, 2, 4, 5)
    return np.ascontiguousarray(y).reshape(B, h2, w2, 4 * N)


def out_bits(y, out_f32):
    return f32_bits(y) if out_f32 else bf16_bits(y)


# ----------------------------------------------------------------------------- exact cases
class Case(object):
    """One exact case: ternary x, a filter with NZ non-zeros (+-1) per output channel, integer bias and shift, post_scale a power of
    two or 1.25: with |conv + bias| <= NZ + 2 = 8 every partial sum, every epilogue value and every output is a bf16 number."""
    NZ = 6

    def __init__(self, name, B, H, W, Cin, Cout, valid, slope, scale, out_f32, seed):
        self.name, self.B, self.H, self.W, self.Cin, self.Cout = name, B, H, W, Cin, Cout
        self.valid, self.slope, self.scale_kind, self.out_f32, self.seed = valid, slope, scale, out_f32, seed

    def data(self):
        r = np.random.RandomState(self.seed)
        x = r.randint(-1, 2, size=(self.B, self.H, self.W, self.Cin)).astype(np.float64)
        k3 = r.randint(-1, 2, size=(self.Cout, self.Cin, 3, 3)).astype(np.float64)      # taps outside {1,2}^2 must not matter
        live = np.zeros((self.Cout, self.Cin * 4))
        for n in range(self.Cout):
            idx = r.choice(self.Cin * 4, size=self.NZ, replace=False)
            live[n, idx] = r.choice([-1., 1.], size=self.NZ)
        k3[:, :, 1:3, 1:3] = live.reshape(self.Cout, self.Cin, 2, 2)
        bias = r.randint(-2, 3, size=self.Cout).astype(np.float64)
        if self.scale_kind is None:
            scale = shift = None
        else:
            scale = (r.choice([0.5, 1., 2.], size=self.Cout) if self.scale_kind == 'pow2' else np.full(self.Cout, 1.25)) * \
                r.choice([-1., 1.], size=self.Cout, p=[0.25, 0.75])
            shift = r.randint(-2, 3, size=self.Cout).astype(np.float64)
        return x, k3, bias, scale, shift

    def expected(self, variant=None):
        x, k3, bias, scale, shift = self.data()
        key = variant if variant in PREACT_VARIANTS else None
        cache = self.__dict__.setdefault('_pre', {})
        if key not in cache:
            cache[key] = preact(x, k3, np.zeros_like(bias) if key == 'bias_last' else bias, key)
        return conv_taps4(x, k3, bias, self.slope, scale, shift, self.valid, self.out_f32, variant, pre=cache[key])

    def applies(self, variant):
        """can this wrong kernel differ from the right one on this case at all?"""
        vh, vw = self.valid
        if variant in ('double_round', 'trunc_filters'):
            return False                      # every value is a bf16 number: any rounding gives it back (rounding_case's business)
        if variant == 'valid_h+1':
            return vh % 2 == 1 and vh < self.H
        if variant == 'valid_w+1':
            return vw % 2 == 1 and vw < self.W
        if variant == 'nonzero_outside':
            return (vh % 2 == 1 and vh < self.H) or (vw % 2 == 1 and vw < self.W)
        if variant == 'affine_first':
            return self.scale_kind is not None
        return True


def _cases():
    # tile of the kernel: 8 rows x 32 columns x 128 output channels; K chunks of 16 input channels
    c = [
        Case('small', 1, 5, 7, 16, 24, (4, 6), 0.25, 'pow2', False, 1),             # smaller than a tile in both directions
        Case('tile', 1, 8, 32, 48, 128, (8, 32), 0.5, '1.25', False, 2),              # exactly a tile, valid = the map
        Case('tile+1', 3, 9, 33, 48, 136, (8, 32), 0.25, '1.25', True, 3),            # tile + 1 in H, W and the Cout tile; valid = H-1, W-1
        Case('odd_valid', 3, 10, 35, 16, 24, (9, 33), 0.5, 'pow2', True, 4),          # odd valid sizes: a computed row / column outside
        Case('k256', 1, 9, 34, 256, 128, (8, 33), 0.5, None, False, 5),               # many K chunks; even x odd valid; no affine
        Case('k1024', 1, 6, 6, 1024, 24, (5, 5), 0.25, 'pow2', False, 6),
        Case('ragged13', 2, 9, 33, 16, 13, (8, 33), 0.5, '1.25', False, 10),         # Cout % 8 != 0: the element-wise store, bf16 ...
        Case('ragged133', 1, 5, 7, 48, 133, (5, 6), 0.25, 'pow2', True, 12),          # ... and fp32, second Cout tile ragged
        Case('block2_382', 1, 95, 95, 256, 128, (94, 94), 0.25, '1.25', False, 7),    # the three block geometries at a 382-pixel input
        Case('block3_382', 1, 47, 47, 512, 256, (46, 46), 0.5, 'pow2', False, 8),
        Case('block4_382', 1, 23, 23, 1024, 512, (22, 22), 0.25, '1.25', True, 9),
    ]
    return c


CASES = _cases()


def rounding_case(out_f32=False):
    """Operands = a ternary value times a factor below, on and above a bf16 tie: the filter (rounded by the pack kernel) carries
    1 + 2^-8 (a tie: to even, down) / 1 + 3 2^-8 (a tie: to even, up) / each -+ 2^-16; the store sees small integers times the same
    factors through post_scale. -> (x, k3, bias, scale, shift, slope, valid)"""
    r = np.random.RandomState(11)
    B, H, W, Cin, Cout = 2, 9, 33, 48, 40
    f = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 - 2.0 ** -16, 1 + 2.0 ** -8 + 2.0 ** -16, 1 + 3 * 2.0 ** -8 - 2.0 ** -16,
                  1 + 3 * 2.0 ** -8 + 2.0 ** -16])
    x = r.randint(-1, 2, size=(B, H, W, Cin)).astype(np.float64)
    k3 = np.zeros((Cout, Cin, 3, 3))
    for n in range(Cout):
        idx = r.choice(Cin * 4, size=3, replace=False)
        live = np.zeros(Cin * 4)
        # channels below 20: plain +-1 filters (the store's rounding alone); from 20 on: factors in the filter (the pack's rounding)
        live[idx] = r.choice([-1., 1.], size=3) * (1. if n < 20 else f[n % 6])
        k3[n, :, 1:3, 1:3] = live.reshape(Cin, 2, 2)
    bias = np.zeros(Cout)
    scale = np.where(np.arange(Cout) < 20, f[np.arange(Cout) % 6], 1.)
    shift = np.zeros(Cout)
    return x, k3, bias, scale, shift, 0.5, (8, 32)


# ----------------------------------------------------------------------------- encoder
def encoder_forward(x, params, p=3., rounding=True):
    """SurfaceEncoder(precision='bf16') in eval mode, in float64. x [B,C,H,W] raw 0..255 values, params as
    oracle.cvig_baseline_oracle.encoder_forward takes them. rounding=False: that oracle in float64."""
    import torch
    import torch.nn.functional as F
    t = torch.as_tensor(np.asarray(x, dtype=np.float64))
    t = t / 255.
    t = -1. + 2. * t
    feats = []
    for i, q in enumerate(params):
        w = np.asarray(q['w'], dtype=np.float64)
        if rounding and 1 <= i <= 3:          # blocks 2-4: bf16 filters
            w = bf16_round(w)
        t = F.conv2d(t, torch.as_tensor(w), torch.as_tensor(np.asarray(q['b'], dtype=np.float64)), stride=2, padding=0)
        t = F.leaky_relu(t, 0.2)
        g, b, m, v = (torch.as_tensor(np.asarray(q[k], dtype=np.float64)) for k in ('gamma', 'beta', 'mean', 'var'))
        scale = g / torch.sqrt(v + 1e-5)
        t = t * scale[None, :, None, None] + (b - m * scale)[None, :, None, None]
        if rounding and i <= 2:               # blocks 1-3 store bf16
            t = torch.as_tensor(bf16_round(t.numpy()))
        if i >= 4:
            feats.append(torch.pow(torch.mean(torch.pow(F.relu(t), p), [2, 3]), 1. / p))
    f = torch.cat(feats, 1)
    return (f / torch.unsqueeze(torch.pow(torch.linalg.norm(f, dim=1), 0.5), 1)).numpy()


def make_params(seed, inputs=3):
    """seeded weights from the reference's init (model/cvig_baseline.py:255-262) and non-trivial running statistics, fp32 values"""
    r = np.random.RandomState(seed)
    widths = [inputs, 64, 128, 256, 512, 512, 512, 512]
    out = []
    for i in range(7):
        f = lambda a: a.astype(np.float32)
        out.append({'w': f(r.normal(0., 0.02, (widths[i + 1], widths[i], 4, 4))), 'b': f(r.normal(0., 0.02, widths[i + 1])),
                    'gamma': f(r.normal(1., 0.02, widths[i + 1])), 'beta': f(r.normal(0., 0.02, widths[i + 1])),
                    'mean': f(r.normal(0., 0.05, widths[i + 1])), 'var': f(r.uniform(0.02, 0.2, widths[i + 1]))})
    return out
