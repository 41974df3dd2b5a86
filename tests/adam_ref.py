"""Adam references for tests/test_adam_ref.py (CPU) and tests/test_adam_gpu.py.

step32: adam_kernel / adam_multi_kernel (csrc/conv3x3_wgrad.hip) restated operation for operation in np.float32, every operation
rounded once, in the kernel's order:
    mi = m*b1 + g*(1-b1);  vi = v*b2 + (g*g)*(1-b2);  denom = sqrtf(vi)/bc2_sqrt + eps;  p = p + (-(lr/bc1)) * (mi/denom)
with bc1 = (float)(1 - pow((double)b1, step)) and bc2_sqrt = (float)sqrt(1 - pow((double)b2, step)) formed in double from the
fp32 betas and rounded once, as witw_adam_step does on the host. The library is built with -ffp-contract=off and without
fast-math, and device sqrtf and division are correctly rounded, so the device must give these bits in p, m and v.

step64: torch.optim.Adam's formula (no weight decay, no amsgrad) in float64.

VARIANTS: deliberately wrong restatements; the tests check that each changes the expected bits, so that a kernel with that
mistake could not pass.
"""
import math

import numpy as np

f32 = np.float32
U = 2.0 ** -24          # unit roundoff of fp32

VARIANTS = ('eps_in_root', 'eps_times_sqrt_bc2', 'bc_swapped', 'step_plus_1', 'step_minus_1', 'g_not_squared', 'm_used_before_update',
            'no_root')


def hyper32(lr, b1, b2, eps):
    """the hyper-parameters as the C entry receives them (float arguments)"""
    return f32(lr), f32(b1), f32(b2), f32(eps)


def bias_terms(b1, b2, step):
    """(bc1, bc2_sqrt) as witw_adam_step forms them: in double from the fp32 betas, rounded once"""
    b1, b2 = float(f32(b1)), float(f32(b2))
    with np.errstate(all='ignore'):
        return f32(1.0 - math.pow(b1, step)), f32(math.sqrt(1.0 - math.pow(b2, step)))


def step32(p, g, m, v, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, variant=None, ftype=f32):
    """one update of fp32 arrays -> (p, m, v), new arrays; `variant` selects one of VARIANTS. ftype=np.float64 runs the same
    expressions (variant included) on the same fp32 inputs without the fp32 roundings: how far a variant moves the result."""
    assert variant is None or variant in VARIANTS
    p, g, m, v = (np.asarray(a, dtype=f32).astype(ftype) for a in (p, g, m, v))
    lr, b1, b2, eps = (ftype(x) for x in hyper32(lr, b1, b2, eps))
    t = step + 1 if variant == 'step_plus_1' else step - 1 if variant == 'step_minus_1' else step
    bc1, bc2s = bias_terms(b1, b2, t)
    if variant == 'bc_swapped':
        with np.errstate(all='ignore'):
            bc1, bc2s = f32(1.0 - math.pow(float(b2), t)), f32(math.sqrt(1.0 - math.pow(float(b1), t)))
    bc1, bc2s = ftype(bc1), ftype(bc2s)
    one = ftype(1)
    with np.errstate(all='ignore'):
        mi = m * b1 + g * (one - b1)
        sq = g if variant == 'g_not_squared' else g * g
        vi = v * b2 + sq * (one - b2)
        if variant == 'eps_in_root':
            denom = np.sqrt(vi + eps) / bc2s
        elif variant == 'eps_times_sqrt_bc2':
            denom = np.sqrt(vi) / bc2s + eps * bc2s
        elif variant == 'no_root':
            denom = vi / bc2s + eps
        else:
            denom = np.sqrt(vi) / bc2s + eps
        used = m if variant == 'm_used_before_update' else mi
        pn = p + (-(lr / bc1)) * (used / denom)
    for a in (pn, mi, vi):
        assert a.dtype == ftype
    return pn, mi, vi


def step64(p, g, m, v, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's update in float64 -> (p, m, v)"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps = float(lr), float(b1), float(b2), float(eps)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = np.sqrt(v) / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def step_bound(p, g, m, v, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, carried=0, m_abs=None):
    """|step32 - step64| allowed per element of (p, m, v), both run from the same fp32 state with the fp32 hyper-parameters
    (pass hyper32's values to step64), normal numbers throughout. With u = 2^-24 and first-order terms:
      m:  three roundings (m*b1, g*(1-b1), the add; 1-b1 is exact for b1 in [0.5, 1)): <= 2u * A, A = |m*b1| + |g*(1-b1)|.
      v:  g*g, *(1-b2), v*b2, the add, all terms positive: relative <= 3u.
      denom: sqrt halves v's 3u and adds u (2.5u); bc2_sqrt is itself a rounded number (u) and the division rounds (u): 4.5u;
             adding eps > 0 rounds once more: relative <= 5.5u.
      update d = (lr/bc1) * (mi/denom): bc1 rounded (u), lr/bc1 (u), mi/denom (u), the product (u), denom's 5.5u: 9.5u |d|,
             plus mi's own error carried through: 2u * A * (lr/bc1) / denom.
      p:  the final add rounds once: u |p_new|.
    `carried` = number of earlier fp32 steps whose rounding is still inside m and v (0 for one step from a shared state). With
    m_abs = the same recursion run on |g| (m_abs_t = b1*m_abs_(t-1) + (1-b1)|g_t|, which bounds the sum of the absolute
    contributions to m_t) the error of m obeys e_t <= b1*e_(t-1) + 2u*A_t <= 2u*t*A_t because A_t >= b1*A_(t-1); v likewise
    carries 3u per step (1.5u each in denom). Here p, m, v are the float64 run's state. The bound returned for p is that of
    this step's update alone; the caller adds the bounds of the earlier steps. A factor 1.01 covers every second-order term
    (they are O(u) smaller)."""
    lr, b1, b2, eps = (float(x) for x in hyper32(lr, b1, b2, eps))
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    p64, m64, v64 = step64(p, g, m, v, step, lr, b1, b2, eps)
    A = (np.abs(m) if m_abs is None else np.asarray(m_abs, dtype=np.float64)) * b1 + np.abs(g) * (1 - b1)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = np.sqrt(v64) / math.sqrt(bc2) + eps
    d = np.abs((lr / bc1) * (m64 / denom))
    k = 1 + carried
    bm = 2 * U * A * k
    bv = 3 * U * v64 * k
    bp = U * np.abs(p64) + (9.5 + 1.5 * carried) * U * d + bm * (lr / bc1) / denom
    return 1.01 * bp, 1.01 * bm, 1.01 * bv


def bits(a):
    a = np.ascontiguousarray(a, dtype=f32)
    return a.view(np.int32)


def operands(kind, n, seed):
    """(p, g, m, v) fp32 arrays of the operand classes of the tests"""
    r = np.random.RandomState(seed)
    p = (r.randn(n) * 0.05).astype(f32)
    if kind == 'normal':                       # N(0, 0.01^2) gradients, fresh state
        return p, (r.randn(n) * 0.01).astype(f32), np.zeros(n, f32), np.zeros(n, f32)
    if kind == 'near_eps':                     # |g| log-uniform in [1e-8, 1e-6]: sqrt(v) is of the order of eps
        g = (10.0 ** r.uniform(-8, -6, n) * r.choice([-1.0, 1.0], n)).astype(f32)
        return p, g, np.zeros(n, f32), np.zeros(n, f32)
    if kind == 'carried':                      # non-zero moments carried in
        return p, (r.randn(n) * 0.01).astype(f32), (r.randn(n) * 0.01).astype(f32), (r.rand(n) * 1e-4 + 1e-9).astype(f32)
    if kind == 'zero':                         # g = 0 with m = v = 0; p holds -0.0 and +0.0 too
        p[::3] = f32(-0.0)
        if n > 1:
            p[1::3] = f32(0.0)
        return p, np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32)
    raise ValueError(kind)
