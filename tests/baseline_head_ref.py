"""Plain torch restatement of cvig_baseline's head and training-step formulas (model/cvig_baseline.py:267-315), the reference of
tests/test_baseline_head_gpu.py. Written from the formulas, not from csrc/baseline.hip:

    BatchNorm2d(train)   mean_c, var_c (biased) over the valid pixels of every image; invstd = (var + eps)^-1/2;
                         y = a * scale + shift with scale = gamma * invstd, shift = beta - mean * scale;
                         running = (1 - m) * running + m * stat, the variance unbiased (n / (n - 1)) there.        :267-275
    GeM                  f[b, c] = (mean_{h, w} relu(y[b, h, w, c])^p)^(1/p)                                        :272-276
    normalisation        f / |f|^(1/2) per row                                                                     :278
    distances            D[i, j] = sum_k (b[j, k] - a[i, k])^2, optionally its square root                         :307-308, :458
    exhaustive loss      sum_{i != j} l(D_ii - D_ij) + l(D_ii - D_ji) over 2 B (B - 1) terms,
                         l(x) = log(1 + exp(alpha x)) (soft) or relu(x + margin) (hard)                            :286-315
    depth-to-space(2)    dx[b, h, w, c] = g[b, h // 2, w // 2, ((h & 1) * 2 + (w & 1)) * C + c]

Every function computes in the dtype of its arguments: float64 gives the reference, float32 gives "the reference's own
arithmetic", whose error against float64 the GPU tests turn into their bounds. Maps are NHWC with a valid region (H, W) inside a
padded (Hp, Wp), as the ops take them. Backwards come from autograd through these functions.
"""
import collections

import torch

BnStats = collections.namedtuple('BnStats', 'mean var invstd scale shift running_mean running_var')


def f64(t):
    return t.detach().cpu().double()


def bn_train_stats(a, valid_hw, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1):
    """-> BnStats over the valid region of a [B, Hp, Wp, C]; the running entries are the UPDATED buffers (None without buffers)."""
    H, W = valid_hw
    v = a[:, :H, :W, :]
    n = v.shape[0] * H * W
    mean = v.mean(dim=(0, 1, 2))
    var = ((v - mean) ** 2).mean(dim=(0, 1, 2))
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    rm = rv = None
    if running_mean is not None:
        rm = (1.0 - momentum) * running_mean + momentum * mean
        rv = (1.0 - momentum) * running_var + momentum * (var * n / (n - 1.0))
    return BnStats(mean, var, invstd, scale, shift, rm, rv)


def bn_lrelu(z, valid_hw, gamma, beta, slope=0.2, eps=1e-5):
    """BatchNorm2d(train)(LeakyReLU(z)) on the valid region -> y [B, H, W, C] (differentiable in z, gamma, beta)."""
    H, W = valid_hw
    a = torch.nn.functional.leaky_relu(z[:, :H, :W, :], slope)
    s = bn_train_stats(a, (H, W), gamma, beta, eps=eps)
    return a * s.scale + s.shift


def gem_pool(x, valid_hw, p=3.0, scale=None, shift=None):
    """-> f [B, C]: GeM with exponent p over the valid region, after the per-channel affine when one is given."""
    H, W = valid_hw
    y = x[:, :H, :W, :]
    if scale is not None:
        y = y * scale + shift
    return torch.pow(torch.mean(torch.pow(torch.relu(y), p), dim=(1, 2)), 1.0 / p)


def embed_normalize(f):
    return f / torch.unsqueeze(torch.pow(torch.linalg.norm(f, dim=1), 0.5), 1)


def pairwise_sqdist(a, b, take_sqrt=False, rows=16):
    """D [Na, Nb] from the differences themselves, `rows` rows of a at a time (the [rows, Nb, n] differences are the memory)."""
    out = []
    for i in range(0, a.shape[0], rows):
        d = torch.sum((b[None, :, :] - a[i:i + rows, None, :]) ** 2, dim=2)
        out.append(torch.sqrt(d) if take_sqrt else d)
    return torch.cat(out, 0)


def triplet_terms(D, margin=1.0):
    """the hard-margin arguments x + margin of every term, [2, B, B - 1]: what must stay clear of the kink at 0"""
    B = D.shape[0]
    off = ~torch.eye(B, dtype=torch.bool)
    dii = torch.diagonal(D)[:, None]
    return torch.stack(((dii - D)[off].reshape(B, B - 1), (dii - D.t())[off].reshape(B, B - 1))) + margin


def exhaustive_triplet_loss_from_D(D, soft_margin=False, alpha=10.0, margin=1.0):
    """The loss as a function of D[i, j] = |embed1_i - embed2_j|^2. Anchor embed1_i: positive distance D_ii, negatives D_ij;
    anchor embed2_i: positive D_ii, negatives D_ji (the reference's roll over the batch visits every j != i once)."""
    B = D.shape[0]
    off = ~torch.eye(B, dtype=torch.bool)
    dii = torch.diagonal(D)[:, None]
    x = torch.cat(((dii - D)[off], (dii - D.t())[off]))
    terms = torch.log(1.0 + torch.exp(alpha * x)) if soft_margin else torch.relu(x + margin)
    return torch.sum(terms) / (2 * B * (B - 1))


def exhaustive_triplet_loss(embed1, embed2, soft_margin=False, alpha=10.0, margin=1.0):
    return exhaustive_triplet_loss_from_D(pairwise_sqdist(embed1, embed2), soft_margin, alpha, margin)


def exhaustive_triplet_loss_grads(embed1, embed2, grad_loss, soft_margin=False, alpha=10.0, margin=1.0, rows=16):
    """-> (loss, D, d embed1, d embed2) by autograd, in two stages so that the [B, B, n] differences never exist at once:
    dL/dD from the loss over a leaf D, then the distance rows `rows` at a time, each back-propagated with its rows of dL/dD."""
    e1 = embed1.detach().clone().requires_grad_(True)
    e2 = embed2.detach().clone().requires_grad_(True)
    with torch.no_grad():
        D = pairwise_sqdist(e1, e2, rows=rows)
    Dl = D.clone().requires_grad_(True)
    loss = exhaustive_triplet_loss_from_D(Dl, soft_margin, alpha, margin)
    (G,) = torch.autograd.grad(loss * grad_loss, Dl)
    for i in range(0, e1.shape[0], rows):
        pairwise_sqdist(e1[i:i + rows], e2, rows=rows).backward(G[i:i + rows])
    return loss.detach(), D, e1.grad, e2.grad


def depth_to_space2(g, hp_wp, valid_hw, C, add=None):
    """g [B, ceil(H/2), ceil(W/2), >= 4C] -> dx [B, Hp, Wp, C]: the indexing definition, element by element; zeros outside."""
    (Hp, Wp), (H, W) = hp_wp, valid_hw
    dx = torch.zeros((g.shape[0], Hp, Wp, C), dtype=g.dtype)
    for h in range(H):
        for w in range(W):
            k = ((h & 1) * 2 + (w & 1)) * C
            dx[:, h, w, :] = g[:, h >> 1, w >> 1, k:k + C]
    if add is not None:
        dx[:, :H, :W, :] += add[:, :H, :W, :]
    return dx
