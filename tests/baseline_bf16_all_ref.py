"""float64 restatement of the bf16 form of blocks 5-7 of cvig_baseline's encoders (SurfaceEncoder(precision='bf16_all')):
witw_conv3x3_bf16_fwd_taps4_splitk (raw partial sums of chunk-aligned K slices over a g x g mosaic), witw_taps4_splitk_finish (sum in
slice order, bias -> LeakyReLU -> affine, gather of the valid outputs), witw_space_to_depth2_mosaic_bf16 (the re-layout with one
nearest-even rounding) and the whole eval forward. Builds on tests/baseline_bf16_ref.py; knows nothing of witw_amd. `variant` names
one deliberately WRONG kernel (tests/test_baseline_bf16_all_ref.py proves the exact cases tell each from the right one)."""
import numpy as np

from tests import baseline_bf16_ref as R

CONV_VARIANTS = ('slice_dropped', 'slice_twice', 'slice_boundary', 'taps_transposed', 'tap_rows_swapped', 'cell_swapped', 'cell_pitch_valid',
                 'bias_per_slice', 'lrelu_first')
RELAYOUT_VARIANTS = ('s2d_swapped', 'cell_swapped', 'double_round', 'trunc')


def slices(nkc, S):
    """[kc0, kc1) of the S slices of nkc chunks of 16 channels: the first nkc % S one chunk longer (include/witw_hip.h)"""
    assert 1 <= S <= nkc
    base, rem = divmod(nkc, S)
    out, k = [], 0
    for s in range(S):
        out.append((k, k + base + (s < rem)))
        k = out[-1][1]
    assert k == nkc
    return out


def splitk_partials(x, k3, S, variant=None):
    """x [Bm,H,W,Cin] (Cin % 16 == 0; values that are bf16 numbers), k3 [cout][cin <= Cin][3][3] -> ws [S,Bm,H,W,cout]: slice s of
    sum_{ty,tx,c} x[b,y+ty,x+tx,c] * bf16(k3[n,c,1+ty,1+tx]), x zero past H / W"""
    x = np.asarray(x, dtype=np.float64)
    Bm, H, W, C = x.shape
    assert C % 16 == 0
    w = np.zeros((k3.shape[0], C, 2, 2))
    w[:, :k3.shape[1]] = R.taps4_filter(k3, 'taps_transposed' if variant == 'taps_transposed' else None)
    if variant == 'tap_rows_swapped':
        w = w[:, :, ::-1]
    xp = np.zeros((Bm, H + 1, W + 1, C))
    xp[:, :H, :W] = x
    sl = slices(C // 16, S)
    if variant == 'slice_boundary':       # every slice runs one chunk past its end (the last one cannot)
        sl = [(a, min(b + 1, C // 16)) for a, b in sl]
    ws = np.zeros((S, Bm, H, W, w.shape[0]))
    for s, (k0, k1) in enumerate(sl):
        c0, c1 = 16 * k0, 16 * k1
        for ty in range(2):
            for tx in range(2):
                ws[s] += (xp[:, ty:ty + H, tx:tx + W, c0:c1].reshape(-1, c1 - c0) @ w[:, c0:c1, ty, tx].T).reshape(Bm, H, W, -1)
    return ws


def finish(ws, bias, slope, scale, shift, n_images, g, valid, variant=None):
    """ws [S,Bm,g*h,g*w,C] -> y [n_images,vh,vw,C] = affine(lrelu(sum_s ws[s] + bias)) at the valid outputs of every cell"""
    S, Bm, H, W, C = ws.shape
    h, w = H // g, W // g
    vh, vw = valid
    bias = np.asarray(bias, dtype=np.float64)

    def lrelu(t):
        return t if slope is None else np.where(t > 0, t, t * slope)
    parts = [ws[s] for s in range(S)]
    if variant == 'slice_dropped':
        parts = parts[:-1]
    if variant == 'slice_twice':
        parts = parts + [parts[0]]
    if variant == 'lrelu_first':
        v = sum(lrelu(t) for t in parts) + bias
    else:
        v = lrelu(sum(parts) + (bias * S if variant == 'bias_per_slice' else bias))
    if scale is not None:
        v = v * np.asarray(scale, dtype=np.float64) + np.asarray(shift, dtype=np.float64)
    ph, pw = (h - 1, w - 1) if variant == 'cell_pitch_valid' else (h, w)
    y = np.zeros((n_images, vh, vw, C))
    for b in range(n_images):
        bm, cell = divmod(b, g * g)
        cy, cx = divmod(cell, g)
        if variant == 'cell_swapped':
            cy, cx = cx, cy
        y[b] = v[bm, cy * ph:cy * ph + vh, cx * pw:cx * pw + vw]
    return y


def s2d_mosaic(y, g, variant=None, rounding=True):
    """y [B,H,W,C] -> [ceil(B/g^2), g*H2, g*W2, 4C], channel ((h&1)*2 + (w&1))*C + c, rounded once to bf16, +0.0 where no source exists"""
    y = np.asarray(y, dtype=np.float64)
    B, H, W, C = y.shape
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    if rounding:
        y = {'double_round': R.bf16_half_up, 'trunc': R.bf16_trunc}.get(variant, R.bf16_round)(y)
    pad = np.zeros((B, 2 * H2, 2 * W2, C))
    pad[:, :H, :W] = y
    t = pad.reshape(B, H2, 2, W2, 2, C)
    t = t.transpose(0, 1, 3, 4, 2, 5) if variant == 's2d_swapped' else t.transpose(0, 1, 3, 2, 4, 5)
    t = t.reshape(B, H2, W2, 4 * C)
    Bm = -(-B // (g * g))
    out = np.zeros((Bm, g * H2, g * W2, 4 * C))
    for b in range(B):
        bm, cell = divmod(b, g * g)
        cy, cx = divmod(cell, g)
        if variant == 'cell_swapped':
            cy, cx = cx, cy
        out[bm, cy * H2:(cy + 1) * H2, cx * W2:(cx + 1) * W2] = t[b]
    return out


# ----------------------------------------------------------------------------- exact cases
class Case(object):
    """One exact case of the split-K conv + finish: the operands of baseline_bf16_ref.Case (ternary x, NZ = 6 non-zeros (+-1) per
    output channel, integer bias and shift, post_scale a power of two or 1.25) laid out as a g x g mosaic of n_images cells of
    h x w, cells without an image zero. |x| |w| summed + |bias| <= 8: every partial sum of any order and any slicing is exact."""
    NZ = R.Case.NZ

    def __init__(self, name, n_images, g, h, w, Cin, Cout, valid, slope, scale, ksplits, seed):
        self.name, self.n_images, self.g, self.h, self.w, self.Cin, self.Cout = name, n_images, g, h, w, Cin, Cout
        self.valid, self.slope, self.scale_kind, self.ksplits, self.seed = valid, slope, scale, ksplits, seed
        self.Bm = -(-n_images // (g * g))

    def data(self):
        x, k3, bias, scale, shift = R.Case(self.name, self.Bm, self.g * self.h, self.g * self.w, self.Cin, self.Cout, self.valid, self.slope,
                                           self.scale_kind, True, self.seed).data()
        for b in range(self.n_images, self.Bm * self.g * self.g):      # cells past the last image
            bm, cell = divmod(b, self.g * self.g)
            cy, cx = divmod(cell, self.g)
            x[bm, cy * self.h:(cy + 1) * self.h, cx * self.w:(cx + 1) * self.w] = 0.
        return x, k3, bias, scale, shift

    def partials(self, S, variant=None):
        x, k3 = self.data()[:2]
        return splitk_partials(x, k3, S, variant)

    def expected(self, S, variant=None):
        _x, _k3, bias, scale, shift = self.data()
        return finish(self.partials(S, variant), bias, self.slope, scale, shift, self.n_images, self.g, self.valid, variant)

    def applies(self, variant, S):
        if variant in ('slice_dropped', 'slice_boundary', 'bias_per_slice', 'lrelu_first'):
            return S >= 2
        if variant == 'cell_swapped':
            return self.g >= 2
        if variant == 'cell_pitch_valid':
            return self.g >= 2 and self.valid[0] < self.h and self.valid[1] < self.w
        return True


def _cases():
    # tile of the kernel: 16 rows x 16 columns x 128 output channels; K chunks of 16 input channels, S slices of whole chunks
    return [
        Case('tile_k16', 1, 1, 16, 16, 16, 128, (16, 16), 0.5, '1.25', (1,), 1),              # exactly one tile, one chunk
        Case('tile_k32', 1, 1, 16, 16, 32, 128, (16, 16), 0.25, 'pow2', (1, 2), 2),           # two chunks: one slice, or one chunk each
        Case('k48', 1, 1, 16, 16, 48, 128, (15, 16), 0.5, None, (2, 3), 3),                   # uneven slices 2 + 1; one chunk per slice
        Case('k64', 5, 2, 7, 7, 64, 24, (6, 6), 0.25, 'pow2', (1, 2, 3, 4), 4),               # split-K invariance: every S up to Cin/16
        Case('mosaic_g5', 27, 5, 3, 3, 32, 24, (2, 2), 0.5, '1.25', (2,), 5),                 # 15 x 15, Bm = 2, last mosaic: 23 empty cells
        Case('mosaic_g2', 7, 2, 7, 7, 32, 40, (6, 6), 0.25, 'pow2', (1, 2), 6),               # 14 x 14, Bm = 2, one empty cell
        Case('ragged_17x18', 2, 1, 17, 18, 32, 24, (16, 17), 0.5, '1.25', (2,), 7),           # four tiles, ragged in both directions
        Case('cout136', 1, 1, 16, 16, 32, 136, (16, 16), 0.25, 'pow2', (2,), 8),              # second, ragged n tile; wide store
        Case('cout12', 3, 1, 5, 7, 32, 12, (5, 6), 0.5, '1.25', (1, 2), 9),                   # Cout % 8 == 4: the element-wise store
        Case('block5_valid', 3, 1, 15, 15, 32, 128, (14, 14), 0.25, None, (2,), 10),          # valid = cell - 1, as the encoder runs block 5
    ]


CASES = _cases()
CASE_SPLITS = [(c, S) for c in CASES for S in c.ksplits]
CASE_SPLIT_IDS = ['%s-S%d' % (c.name, S) for c, S in CASE_SPLITS]


def case(name):
    return [c for c in CASES if c.name == name][0]


# B not a multiple of g^2, odd H and W, g = 1, 2, 5, C = 8 (16-byte stores) and 12 (8-byte stores)
RELAYOUT_SHAPES = [(3, 5, 7, 8, 1), (3, 5, 7, 12, 2), (7, 13, 13, 8, 2), (27, 5, 5, 12, 5), (26, 6, 5, 8, 5)]


def relayout_data(B, H, W, C, seed=0):
    """fp32 values below, on and above bf16 ties (baseline_bf16_ref.rounding_case's factors times small integers), as float64"""
    r = np.random.RandomState(100 + seed)
    f = np.array([1., 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 - 2.0 ** -16, 1 + 2.0 ** -8 + 2.0 ** -16, 1 + 3 * 2.0 ** -8 - 2.0 ** -16,
                  1 + 3 * 2.0 ** -8 + 2.0 ** -16])
    v = r.randint(-4, 5, size=(B, H, W, C)) * f[r.randint(0, 7, size=(B, H, W, C))] * 2.0 ** r.randint(-3, 4, size=(B, H, W, C))
    assert np.array_equal(np.float32(v).astype(np.float64), v)
    return v


# ----------------------------------------------------------------------------- encoder
def encoder_forward_all(x, params, p=3.):
    """SurfaceEncoder(precision='bf16_all') in eval mode, in float64: bf16 filters in blocks 2-7, the activations rounded (nearest-even,
    once) at the inputs of blocks 2-7, the pooled features of blocks 5-7 from their unrounded outputs. x [B,C,H,W] raw 0..255 values."""
    import torch
    import torch.nn.functional as F
    t = torch.as_tensor(np.asarray(x, dtype=np.float64))
    t = -1. + 2. * (t / 255.)
    feats = []
    for i, q in enumerate(params):
        w = np.asarray(q['w'], dtype=np.float64)
        if i >= 1:
            w = R.bf16_round(w)
        t = F.conv2d(t, torch.as_tensor(w), torch.as_tensor(np.asarray(q['b'], dtype=np.float64)), stride=2, padding=0)
        t = F.leaky_relu(t, 0.2)
        g, b, m, v = (torch.as_tensor(np.asarray(q[k], dtype=np.float64)) for k in ('gamma', 'beta', 'mean', 'var'))
        scale = g / torch.sqrt(v + 1e-5)
        t = t * scale[None, :, None, None] + (b - m * scale)[None, :, None, None]
        if i >= 4:
            feats.append(torch.pow(torch.mean(torch.pow(F.relu(t), p), [2, 3]), 1. / p))
        if i <= 5:
            t = torch.as_tensor(R.bf16_round(t.numpy()))
    f = torch.cat(feats, 1)
    return (f / torch.unsqueeze(torch.pow(torch.linalg.norm(f, dim=1), 0.5), 1)).numpy()
