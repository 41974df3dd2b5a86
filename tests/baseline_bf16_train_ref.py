"""float64 restatement of the bf16 TRAINING arithmetic of cvig_baseline's blocks 2-4 (SurfaceEncoder(train_precision='bf16'),
include/witw_hip.h: witw_conv3x3_bf16_fwd_taps4_plain, witw_conv3x3_bf16_pack_weights_taps4_ex, witw_space_to_depth2_bf16,
witw_conv3x3_wgrad_bf16_taps4): everything in float64, rounded to bf16 (nearest-even, once) at exactly the three places the product
rounds -- a filter (from the master weights), a block's input h_i, a block's output gradient dz_i -- and nowhere else. Built on
tests/baseline_bf16_ref.py; knows nothing of witw_amd. The one-block functions are numpy in the space-to-depth / 2x2-tap form the
kernels run; encoder_step is torch float64 autograd over Conv2d(k=4, s=2) -> LeakyReLU -> BatchNorm2d(train) with the roundings as
straight-through casts (tests/test_baseline_bf16_train_ref.py holds the two forms against each other)."""
import numpy as np

from tests.baseline_bf16_ref import bf16_round


# ----------------------------------------------------------------------------- one block, the form the kernels run
def fwd_filter(k3, rounding=True):
    """[cout][cin][3][3] -> the forward taps [cout][cin][2][2]: tap (ty, tx) = k3[.., 1+ty, 1+tx], rounded once"""
    w = np.asarray(k3, dtype=np.float64)[:, :, 1:3, 1:3]
    return bf16_round(w) if rounding else w.copy()


def dgrad_filter(k3, rounding=True):
    """[cout][cin][3][3] -> the data-gradient taps [cin][cout][2][2]: tap (ty, tx) of (ci, co) = k3[co][ci][2-ty][2-tx]: the taps
    {0,1}^2 of the transposed filter rotated by 180 degrees, rounded once"""
    w = np.asarray(k3, dtype=np.float64).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1][:, :, 0:2, 0:2]
    return bf16_round(w) if rounding else w.copy()


def conv_plain(x, w4, bias, tap_base, valid_hw=None, slope=None):
    """out[b,r,c,n] = act(sum_{ty,tx} sum_ci x[b,r+ty-off,c+tx-off,ci] * w4[n,ci,ty,tx] + bias[n]), off = 1 - tap_base, x zero outside
    the map; +0 outside the valid region. x [B,H,W,C] -> [B,H,W,Cout]"""
    x = np.asarray(x, dtype=np.float64)
    B, H, W, C = x.shape
    off = 1 - tap_base
    xp = np.zeros((B, H + 2, W + 2, C))
    xp[:, 1:H + 1, 1:W + 1] = x
    out = np.zeros((B, H, W, w4.shape[0]))
    for ty in range(2):
        for tx in range(2):
            r0, c0 = 1 + ty - off, 1 + tx - off
            out += (xp[:, r0:r0 + H, c0:c0 + W].reshape(-1, C) @ w4[:, :, ty, tx].T).reshape(B, H, W, -1)
    if bias is not None:
        out = out + np.asarray(bias, dtype=np.float64)
    if slope is not None:
        out = np.where(out > 0, out, out * slope)
    if valid_hw is not None:
        out[:, valid_hw[0]:] = 0.
        out[:, :, valid_hw[1]:] = 0.
    return out


def wgrad_taps4(h, dz, cin_real=None):
    """-> (dk3 [Cout][cin_real][3][3] with dk3[n,ci,1+ty,1+tx] = sum_{b,r,c} dz[b,r,c,n] * h[b,r+ty,c+tx,ci] (h zero past H / W) and
    zeros at the five other taps, db [Cout] = sum dz)"""
    h, dz = np.asarray(h, dtype=np.float64), np.asarray(dz, dtype=np.float64)
    B, H, W, C = h.shape
    N = dz.shape[3]
    hp = np.zeros((B, H + 1, W + 1, C))
    hp[:, :H, :W] = h
    dk3 = np.zeros((N, C, 3, 3))
    for ty in range(2):
        for tx in range(2):
            dk3[:, :, 1 + ty, 1 + tx] = dz.reshape(-1, N).T @ hp[:, ty:ty + H, tx:tx + W].reshape(-1, C)
    return dk3[:, :cin_real if cin_real else C], dz.reshape(-1, N).sum(0)


def space_to_depth2(a, valid_hw, scale=None, shift=None, rounding=True):
    """[B,Hp,Wp,C] -> [B,ceil(vh/2),ceil(vw/2),4C]: channel (dy*2+dx)*C+c = a[2h2+dy, 2w2+dx, c] * scale[c] + shift[c] inside the valid
    region, rounded once; +0 outside it whatever the shift"""
    a = np.asarray(a, dtype=np.float64)
    B, _hp, _wp, C = a.shape
    vh, vw = valid_hw
    h2, w2 = (vh + 1) // 2, (vw + 1) // 2
    v = a[:, :vh, :vw]
    if scale is not None:
        v = v * np.asarray(scale, dtype=np.float64) + np.asarray(shift, dtype=np.float64)
    if rounding:
        v = bf16_round(v)
    full = np.zeros((B, 2 * h2, 2 * w2, C))
    full[:, :vh, :vw] = v
    return np.ascontiguousarray(full.reshape(B, h2, 2, w2, 2, C).transpose(0, 1, 3, 2, 4, 5)).reshape(B, h2, w2, 4 * C)


def conv4x4_to_k3(w):
    """[co][ci][4][4] -> [co][4ci][3][3]: tap (1+ta, 1+tb) of channel (dy*2+dx)*ci + c = w[co][c][2ta+dy][2tb+dx], zeros elsewhere"""
    w = np.asarray(w, dtype=np.float64)
    co, ci = w.shape[:2]
    k3 = np.zeros((co, 4 * ci, 3, 3))
    for ta in range(2):
        for tb in range(2):
            for dy in range(2):
                for dx in range(2):
                    q = dy * 2 + dx
                    k3[:, q * ci:(q + 1) * ci, 1 + ta, 1 + tb] = w[:, :, 2 * ta + dy, 2 * tb + dx]
    return k3


def k3_to_conv4x4(dk3, ci):
    dk3 = np.asarray(dk3, dtype=np.float64)
    w = np.zeros((dk3.shape[0], ci, 4, 4))
    for ta in range(2):
        for tb in range(2):
            for dy in range(2):
                for dx in range(2):
                    q = dy * 2 + dx
                    w[:, :, 2 * ta + dy, 2 * tb + dx] = dk3[:, q * ci:(q + 1) * ci, 1 + ta, 1 + tb]
    return w


def depth_to_space2(g, C, out_hw):
    """inverse of space_to_depth2's re-layout for a gradient: [B,h2,w2,4C] -> [B,H,W,C] (cropped to out_hw)"""
    B, h2, w2, _ = g.shape
    full = g.reshape(B, h2, w2, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * h2, 2 * w2, C)
    return full[:, :out_hw[0], :out_hw[1]]


def block_step(a_prev, valid_prev, scale, shift, w, b, gamma, beta, dy, slope=0.2, eps=1e-5, rounding=True):
    """One block i in {2,3,4} in the kernels' form: a_prev [B,Hp,Wp,Cp] fp32-valued activation of block i-1 (valid region valid_prev),
    its train-mode BatchNorm affine (scale, shift), the block's Conv2d weights w [co][ci][4][4] / b, its BatchNorm gamma / beta, and
    dy = dL/d(BatchNorm output) [B,vh,vw,co]. -> dict: h (rounded input), a (LeakyReLU(conv)), y (BatchNorm output), dz, dw, db,
    dgamma, dbeta, dh (gradient at h, [B,H,W,4Cp])"""
    k3 = conv4x4_to_k3(w)
    h = space_to_depth2(a_prev, valid_prev, scale, shift, rounding)
    vh, vw = (valid_prev[0] - 4) // 2 + 1, (valid_prev[1] - 4) // 2 + 1
    a = conv_plain(h, fwd_filter(k3, rounding), b, 1, (vh, vw), slope)
    av = a[:, :vh, :vw]
    mean, var = av.mean((0, 1, 2)), av.var((0, 1, 2))
    invstd = 1. / np.sqrt(var + eps)
    xhat = (av - mean) * invstd
    y = xhat * gamma + beta
    dgamma, dbeta = (dy * xhat).sum((0, 1, 2)), dy.sum((0, 1, 2))
    n = av.shape[0] * vh * vw
    da = gamma * invstd * (dy - dbeta / n - xhat * dgamma / n)
    dzv = da * np.where(av > 0, 1., slope)
    dz = np.zeros_like(a)
    dz[:, :vh, :vw] = bf16_round(dzv) if rounding else dzv
    dk3, db = wgrad_taps4(h, dz)
    dh = conv_plain(dz, dgrad_filter(k3, rounding), None, 0)
    return {'h': h, 'a': a, 'y': y, 'dz': dz, 'dw': k3_to_conv4x4(dk3, w.shape[1]), 'db': db, 'dgamma': dgamma, 'dbeta': dbeta, 'dh': dh}


# ----------------------------------------------------------------------------- the encoder's training step
def _ste(jitter=None):
    """jitter = (sigma, seed): every value is multiplied by 1 + sigma N(0,1) in front of its rounding -- what an fp32 computation of
    the same value does to it; the distance between the jittered and the plain step is the step's own sensitivity to that"""
    import torch
    rs = np.random.RandomState(jitter[1]) if jitter else None

    def bf16_round_(a):
        a = np.asarray(a, dtype=np.float64)
        return bf16_round(a * (1. + jitter[0] * rs.normal(size=a.shape)) if jitter else a)

    class RoundFwd(torch.autograd.Function):      # a value rounded on the way forward, the gradient passes
        @staticmethod
        def forward(ctx, t):
            return torch.as_tensor(bf16_round_(t.detach().numpy()))

        @staticmethod
        def backward(ctx, g):
            return g

    class RoundBwd(torch.autograd.Function):      # the gradient rounded on the way back
        @staticmethod
        def forward(ctx, t):
            return t.view_as(t)

        @staticmethod
        def backward(ctx, g):
            return torch.as_tensor(bf16_round_(g.numpy()))

    return RoundFwd.apply, RoundBwd.apply


def encoder_step(x, params, df, p=3., rounding=True, gates=None, jitter=None):
    """SurfaceEncoder(train_precision='bf16').train() forward and backward in float64: x [B,C,H,W] raw 0..255 values, params a list of 7
    dicts w, b, gamma, beta (fp32 values), df = dL/d(embedding) [B,1536]. Blocks 2-4 (rounding=True): filter, input and output gradient
    rounded once each; jitter: see _ste. gates: {block i: bool [B,co,vh,vw]} replaces the LeakyReLU gate of block i in the backward (None: its own).
    -> (embedding [B,1536], grads: list of 7 dicts dw, db, dgamma, dbeta, pre: list of the 7 conv outputs [B,co,vh,vw],
        stats: list of 7 (batch mean, biased batch variance))"""
    import torch
    import torch.nn.functional as F
    rf, rb = _ste(jitter)
    t = torch.as_tensor(np.asarray(x, dtype=np.float64))
    t = t / 255.
    t = -1. + 2. * t
    leaves, pre, stats, feats = [], [], [], []
    for i, q in enumerate(params, 1):
        lv = {k: torch.tensor(np.asarray(q[k], dtype=np.float64), requires_grad=True) for k in ('w', 'b', 'gamma', 'beta')}
        leaves.append(lv)
        on = rounding and 2 <= i <= 4
        z = F.conv2d(rf(t) if on else t, rf(lv['w']) if on else lv['w'], lv['b'], stride=2, padding=0)
        if on:
            z = rb(z)
        pre.append(z.detach().numpy())
        if gates is not None and i in gates:      # LeakyReLU with a given gate: linear in z on either side
            gt = torch.as_tensor(np.asarray(gates[i]))
            a = torch.where(gt, z, z * 0.2)
        else:
            a = F.leaky_relu(z, 0.2)
        mean, var = a.mean((0, 2, 3)), a.var((0, 2, 3), unbiased=False)
        stats.append((mean.detach().numpy(), var.detach().numpy()))
        t = (a - mean[None, :, None, None]) / torch.sqrt(var + 1e-5)[None, :, None, None] * lv['gamma'][None, :, None, None] + \
            lv['beta'][None, :, None, None]
        if i >= 5:
            feats.append(torch.pow(torch.mean(torch.pow(F.relu(t), p), [2, 3]), 1. / p))
    f = torch.cat(feats, 1)
    f = f / torch.unsqueeze(torch.pow(torch.linalg.norm(f, dim=1), 0.5), 1)
    (f * torch.as_tensor(np.asarray(df, dtype=np.float64))).sum().backward()
    grads = [{'d' + k: lv[k].grad.numpy() for k in ('w', 'b', 'gamma', 'beta')} for lv in leaves]
    return f.detach().numpy(), grads, pre, stats
