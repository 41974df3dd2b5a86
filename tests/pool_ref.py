"""float64 reference of the fused conv3x3 + ReLU + MaxPool2d(2,2) as the training backward sees it -- the pooled value, the arg-max
code the forward records in its place of the unpooled activation, and the gradient the code routes -- on data where EVERY kernel is
exact whatever its summation order, so that tests/test_pool_codes_gpu.py can compare bits instead of tolerances.

    z      = conv3x3(x, w, b)            zero rows above / below; zero or (circular) wrapped columns, as oracle.cvig_fov_oracle.conv3x3
    pooled = max_pool2d(relu(z), 2, 2)   floor: an odd last row / column of z belongs to no window
    code   = dy * 2 + dx of the FIRST position, in scan order (0,0), (0,1), (1,0), (1,1), that attains the window's maximum of z
    dz     = autograd of pooled at z:    gy at the coded position where the window's maximum is > 0, +0.0 everywhere else

Exact data (exact_operands): x and w drawn from {-1, 0, 1}, sparse, and an integer bias in [-2, 2]. Every product is -1, 0 or 1 and
every partial sum a small integer: exact in fp32, in bf16 operands with fp32 accumulation, and in fp16 hi / lo with lo = 0; the
Winograd F(2,3) filter transform adds halves of such integers, exact too. conv3x3_exact() refuses operands whose |z| passes 128, so
the pooled output is also a bf16 / fp16 number (integers up to 256 / 2048) and is compared bit for bit.

The tables at the end name every case of tests/test_pool_codes_gpu.py; tests/test_pool_ref.py checks, on the CPU, that each of them
really exercises the arg-max rule (enough positive windows, enough ties at the maximum, every code the answer often enough)."""
import functools

import numpy as np

MAX_ABS_Z = 128.0


def _tern(g, shape, p):
    """{-1, 0, 1}, non-zero with probability p"""
    return (g.integers(0, 2, shape) * 2 - 1) * (g.random(shape) < p).astype(np.float64)


def exact_operands(seed, B, Cin, Cout, H, W, px=0.25, terms=5.0):
    """-> x [B,Cin,H,W], w [Cout,Cin,3,3], b [Cout], float64 holding small integers. px: share of non-zero inputs; the filter's share is
    chosen so that an output sums about `terms` non-zero products (a spread of a few units: windows tie often, yet not always)."""
    g = np.random.Generator(np.random.Philox(key=[seed, Cin * 1000 + Cout]))
    x = _tern(g, (B, Cin, H, W), px)
    w = _tern(g, (Cout, Cin, 3, 3), min(0.5, terms / (9.0 * Cin * px)))
    b = g.integers(-2, 3, (Cout,)).astype(np.float64)
    return x, w, b


def grad_ints(seed, shape):
    """a pooled-output gradient of small non-zero integers (+-1 .. +-3): exact in every format, and never mistaken for a routed zero"""
    g = np.random.Generator(np.random.Philox(key=[seed, 77]))
    return (g.integers(1, 4, shape) * (g.integers(0, 2, shape) * 2 - 1)).astype(np.float64)


def _pad(x, circular):
    B, C, H, W = x.shape
    xp = np.zeros((B, C, H + 2, W + 2), dtype=np.float64)
    xp[:, :, 1:-1, 1:-1] = x
    if circular:
        xp[:, :, 1:-1, 0] = x[:, :, :, -1]
        xp[:, :, 1:-1, -1] = x[:, :, :, 0]
    return xp


def conv3x3(x, w, b, circular):
    """z[b, co, h, w] = bias[co] + sum_{ci, kh, kw} Xpad[b, ci, h + kh, w + kw] * w[co, ci, kh, kw], float64, stride 1"""
    x, w, b = (np.asarray(t, dtype=np.float64) for t in (x, w, b))
    B, _c, H, W = x.shape
    xp = _pad(x, bool(circular))
    z = np.zeros((B, w.shape[0], H, W), dtype=np.float64) + b[None, :, None, None]
    for kh in range(3):
        for kw in range(3):
            z += np.einsum('bihw,oi->bohw', xp[:, :, kh:kh + H, kw:kw + W], w[:, :, kh, kw], optimize=True)
    return z


def conv3x3_exact(x, w, b, circular):
    """conv3x3 of exact_operands-style data; AssertionError unless every operand is an integer and max |z| <= 128"""
    for t in (x, w, b):
        assert np.array_equal(t, np.rint(t)), 'operands must be integers'
    z = conv3x3(x, w, b, circular)
    assert float(np.abs(z).max()) <= MAX_ABS_Z, 'max |conv| = %g passes %g: not exact in bf16' % (float(np.abs(z).max()), MAX_ABS_Z)
    return z


def windows(z):
    """[B,C,H,W] -> [B,C,H//2,W//2,4]: the 2x2 windows in scan order (index dy * 2 + dx)"""
    B, C, H, W = z.shape
    Hp, Wp = H // 2, W // 2
    return z[:, :, :2 * Hp, :2 * Wp].reshape(B, C, Hp, 2, Wp, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, Hp, Wp, 4)


def pool_ref(z):
    """-> (pooled = max_pool2d(relu(z)) float64, code uint8, m = the windows' maxima of z), each [B,C,H//2,W//2]"""
    win = windows(z)
    m = win.max(axis=-1)
    code = win.argmax(axis=-1).astype(np.uint8)          # numpy's argmax is the first maximum
    return np.maximum(m, 0.0) + 0.0, code, m


def route_ref(z, gy):
    """gradient of sum(gy * max_pool2d(relu(z))) at z: gy at the coded position of the windows whose maximum is > 0, +0.0 elsewhere
    (the windows gated by the ReLU, and an odd last row / column)"""
    _pooled, code, m = pool_ref(z)
    B, C, H, W = z.shape
    Hp, Wp = H // 2, W // 2
    dz = np.zeros_like(z)
    live = np.where(m > 0, gy, 0.0)
    for q in range(4):
        dz[:, :, (q >> 1):2 * Hp:2, (q & 1):2 * Wp:2] = np.where(code == q, live, 0.0)
    return dz


def scatter_ref(dy_bits, code, H, W):
    """the scatter alone, on bit patterns: dy_bits (any integer dtype) and code, both [B,Hp,Wp,C] -> [B,H,W,C] of the same dtype with
    dy's bits at position (2h + code // 2, 2w + code % 2) and zero bits (+0.0) everywhere else"""
    B, Hp, Wp, C = dy_bits.shape
    assert code.shape == dy_bits.shape and H >= 2 * Hp and W >= 2 * Wp
    out = np.zeros((B, H, W, C), dtype=dy_bits.dtype)
    for q in range(4):
        out[:, (q >> 1):2 * Hp:2, (q & 1):2 * Wp:2, :] = np.where(code == q, dy_bits, 0).astype(dy_bits.dtype)
    return out


def shares(z):
    """what makes a case a test of the arg-max rule: the share of windows with a positive maximum, among those the share that attain it
    at two or more positions, and for each code the share of the positive windows it is the answer of"""
    win = windows(z)
    _pooled, code, m = pool_ref(z)
    pos = m > 0
    n_pos = max(1, int(pos.sum()))
    tied = ((win == m[..., None]).sum(axis=-1) >= 2) & pos
    return {'positive': float(pos.mean()), 'tied': float(tied.sum()) / n_pos,
            'codes': [float(((code == q) & pos).sum()) / n_pos for q in range(4)]}


# ---- the fused first two layers (csrc/conv_first2_bf16.hip): C -> 64 conv + ReLU, then 64 -> 64 conv + ReLU + pool
def first2_operands(seed, B, C, H, W):
    """x [B,C,H,W], (w0 [64,C,3,3], b0), (w2 [64,64,3,3], b2): integers; the layer between them then holds small non-negative
    integers (exact in bf16) and the second conv sums a few of those"""
    g = np.random.Generator(np.random.Philox(key=[seed, C * 100000 + H * W]))
    x = _tern(g, (B, C, H, W), 0.5)
    w0 = _tern(g, (64, C, 3, 3), min(0.5, 4.0 / (9.0 * C * 0.5)))
    b0 = g.integers(-2, 3, (64,)).astype(np.float64)
    w2 = _tern(g, (64, 64, 3, 3), 6.0 / (9.0 * 64))
    b2 = g.integers(-2, 3, (64,)).astype(np.float64)
    return x, w0, b0, w2, b2


def first2_exact(x, w0, b0, w2, b2, circular):
    """z of the second layer over relu(first layer), float64, both layers under the same padding"""
    mid = np.maximum(conv3x3_exact(x, w0, b0, circular), 0.0)
    return conv3x3_exact(mid, w2, b2, circular)


# ---- the cases of tests/test_pool_codes_gpu.py
PADS = (False, True)       # zero, circular

# fp32, conv3x3_fwd(pool, want_pool_code): (site, H, W, Cin, Cout), B = 2, stride 1
FP32_CASES = (
    [('narrow', H, W, ci, co) for (H, W) in ((6, 24), (7, 17)) for (ci, co) in ((8, 64), (16, 128))] +
    [('slab', H, W, ci, co) for (H, W) in ((10, 70), (9, 65), (16, 64)) for (ci, co) in ((8, 64), (16, 128), (16, 136))] +
    [('generic', H, W, ci, co) for (H, W) in ((10, 70), (9, 65)) for (ci, co) in ((8, 66), (16, 130))] +
    [('wino', H, W, ci, co) for (H, W) in ((16, 64), (13, 72)) for (ci, co) in ((64, 64), (128, 128))])

# bf16 tiled kernel and split-fp16: (H, W, Cin, Cout), B = 2
LOW_CASES = [(H, W, ci, co) for (H, W) in ((8, 64), (9, 70), (6, 24)) for (ci, co) in ((16, 64), (32, 128))]

# the 16x16x32 TRAIN instantiation: one workgroup per (image, 8 rows) here, and the launcher wants the last round of one workgroup
# per CU at least 90 % full (csrc/api.hip witw_fills_rounds): on 256 CUs 2 B >= 0.9 * 256, i.e. B = 116 is the smallest batch
S16_CASE = (116, 16, 64, 32, 128)


def pick(B):
    """the images of a large batch that are compared (as tests/test_large_grid_parity_gpu.py: both ends, the middle, an odd index)"""
    return sorted({0, B // 3, B // 2 + 1, B - 1})


FIRST2_SHAPES = [(2, 3, 20, 70), (1, 5, 10, 34), (2, 4, 8, 32)]


class Case(object):
    """one case's operands and float64 answers, NCHW numpy arrays, read-only: x, w, b (first2: x, w0, b0, w2, b2), z, pooled, code,
    m, gy, dz; sel = the images of x that z and the rest describe (None: all)"""

    def __init__(self, **kw):
        for k, v in kw.items():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
            setattr(self, k, v)


def _answers(z, seed, **kw):
    pooled, code, m = pool_ref(z)
    gy = grad_ints(seed, pooled.shape)
    return Case(z=z, pooled=pooled, code=code, m=m, gy=gy, dz=route_ref(z, gy), **kw)


@functools.lru_cache(maxsize=None)
def conv_case(B, H, W, Cin, Cout, circular, sel=None):
    """operands and answers of one conv + pool case, computed once per process and shared"""
    seed = 1000 * H + W + (500000 if circular else 0)
    x, w, b = exact_operands(seed, B, Cin, Cout, H, W)
    xs = x if sel is None else x[list(sel)]
    return _answers(conv3x3_exact(xs, w, b, circular), seed, x=x, w=w, b=b, sel=sel)


@functools.lru_cache(maxsize=None)
def first2_case(B, C, H, W, circular):
    seed = 1000 * H + W + (500000 if circular else 0)
    x, w0, b0, w2, b2 = first2_operands(seed, B, C, H, W)
    return _answers(first2_exact(x, w0, b0, w2, b2, circular), seed, x=x, w0=w0, b0=b0, w2=w2, b2=b2, sel=None)


def all_cases():
    """(label, thunk -> Case) of every case the GPU file runs"""
    out = []
    for circ in PADS:
        for site, H, W, ci, co in FP32_CASES:
            out.append(('fp32-%s-%dx%d-%d-%d-circ%d' % (site, H, W, ci, co, circ), functools.partial(conv_case, 2, H, W, ci, co, circ)))
        for H, W, ci, co in LOW_CASES:
            out.append(('low-%dx%d-%d-%d-circ%d' % (H, W, ci, co, circ), functools.partial(conv_case, 2, H, W, ci, co, circ)))
        B, H, W, ci, co = S16_CASE
        out.append(('s16-%dx%dx%d-%d-%d-circ%d' % (B, H, W, ci, co, circ), functools.partial(conv_case, B, H, W, ci, co, circ, tuple(pick(B)))))
        for B, C, H, W in FIRST2_SHAPES:
            out.append(('first2-%dx%dx%dx%d-circ%d' % (B, C, H, W, circ), functools.partial(first2_case, B, C, H, W, circ)))
    return out
