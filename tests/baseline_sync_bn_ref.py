"""float64 numpy restatement of the four split BatchNorm entries of csrc/baseline_bn_sync.hip (include/witw_hip.h), the reference of
tests/test_baseline_sync_bn_gpu.py. Written from the header's formulas, not from the kernels; tests/test_baseline_sync_bn_ref.py
checks it on its own against the one-shot statistics and torch's float64 autograd.

Maps are NHWC [B, Hp, Wp, C] with a valid region (H, W); everything outside it is never read. A "part" is a [2C] vector.

    partial_stats       part[c] = S1 = sum (a - pivot[c]),  part[C + c] = S2 = sum (a - pivot[c])^2
    finalize_stats      n = count: mean = pivot + S1/n, var = max(0, S2/n - (S1/n)^2) (biased), invstd = (var + eps)^-1/2,
                        scale = gamma invstd, shift = beta - mean scale, running = (1 - m) running + m stat (variance n/(n-1));
                        count <= 1 raises, as the entry refuses it
    bwd_partial         part[c] = sum dy,  part[C + c] = sum dy xhat,  xhat = (a - mean[c]) invstd[c]
    bwd_apply           dz = lrelu'(a) gamma invstd (dy - sums[c]/n - xhat sums[C + c]/n) on the valid region, 0 outside;
                        lrelu'(a) = 1 for a > 0, slope otherwise (a = LeakyReLU(z) has the sign of z)
"""
import collections

import numpy as np

Stats = collections.namedtuple('Stats', 'mean var invstd scale shift running_mean running_var')


def f64(x):
    return np.asarray(x, dtype=np.float64)


def partial_stats(a, valid_hw, pivot):
    H, W = valid_hw
    d = f64(a)[:, :H, :W, :] - f64(pivot)
    return np.concatenate((d.sum(axis=(0, 1, 2)), (d * d).sum(axis=(0, 1, 2))))


def finalize_stats(part_sum, pivot, count, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1):
    if count <= 1:
        raise ValueError('finalize_stats: needs more than one value per channel')
    part_sum, n = f64(part_sum), float(count)
    C = part_sum.shape[0] // 2
    dm = part_sum[:C] / n
    mean = f64(pivot) + dm
    var = np.maximum(part_sum[C:] / n - dm * dm, 0.0)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = f64(gamma) * invstd
    shift = f64(beta) - mean * scale
    rm = rv = None
    if running_mean is not None:
        rm = (1.0 - momentum) * f64(running_mean) + momentum * mean
        rv = (1.0 - momentum) * f64(running_var) + momentum * (var * n / (n - 1.0))
    return Stats(mean, var, invstd, scale, shift, rm, rv)


def bwd_partial(a, dy, valid_hw, mean, invstd):
    H, W = valid_hw
    xh = (f64(a)[:, :H, :W, :] - f64(mean)) * f64(invstd)
    g = f64(dy)[:, :H, :W, :]
    return np.concatenate((g.sum(axis=(0, 1, 2)), (g * xh).sum(axis=(0, 1, 2))))


def bwd_apply(a, dy, valid_hw, mean, invstd, gamma, sums, count, slope=0.2):
    H, W = valid_hw
    a, sums, n = f64(a), f64(sums), float(count)
    C = a.shape[3]
    av = a[:, :H, :W, :]
    xh = (av - f64(mean)) * f64(invstd)
    da = f64(gamma) * f64(invstd) * (f64(dy)[:, :H, :W, :] - sums[:C] / n - xh * sums[C:] / n)
    dz = np.zeros(a.shape, dtype=np.float64)
    dz[:, :H, :W, :] = np.where(av > 0, da, da * slope)
    return dz


def space_to_depth2(dy, valid_hw, cp):
    """[B, Hp, Wp, C] -> the layout dy_s2d_cp = cp names: [B, ceil(H/2), ceil(W/2), cp], channel ((h & 1) * 2 + (w & 1)) * C + c; the
    channels from 4C on and the cells without a source hold a value that would show in any sum that read it"""
    H, W = valid_hw
    B, _Hp, _Wp, C = dy.shape
    out = np.full((B, (H + 1) // 2, (W + 1) // 2, cp), 57.0, dtype=dy.dtype)
    for h in range(H):
        for w in range(W):
            k = ((h & 1) * 2 + (w & 1)) * C
            out[:, h >> 1, w >> 1, k:k + C] = dy[:, h, w, :]
    return out
