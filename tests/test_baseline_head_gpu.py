"""Op-level values of cvig_baseline's head and training-step kernels (csrc/baseline.hip, everything but the convolutions) against
the float64 restatement in tests/baseline_head_ref.py: witw_bn_train_stats, witw_gem_pool(_bwd), witw_embed_normalize(_bwd),
witw_pairwise_sqdist, witw_exhaustive_triplet_loss(_bwd), witw_depth_to_space2, and one chain through all of them in the order
cvig_baseline.py calls them. Everything goes through witw_amd.ops; inputs are seeded Philox draws; padding around a valid region
is filled with a value that would show in any sum that read it.

Bounds. None comes from a kernel's output. Fixed ones are the project's existing ones:

  per-channel statistics   1e-5 relative (dgamma / dbeta of test_bn_lrelu_backward_against_autograd). invstd, scale and
                           running_var are positive and bounded per channel, |got - ref| <= 1e-5 |ref|; mean, shift and running_mean
                           are sums that may cancel, so they are bounded by 1e-5 of the largest magnitude of their terms over the
                           channels: sqrt(mean^2 + var) for mean, |beta| + |mean * scale| for shift, 0.9 |running_0| + 0.1 |mean|
                           for running_mean.
  element-wise gradients   2e-5 x max |ref| (dz of the same test): gem_pool_bwd, embed_normalize_bwd, de1 / de2, the chain's dz.
  losses                   rtol 1e-4 (test_baseline_loss_and_ranks).
  true-pair distances      1e-5 relative per element: (b - a)^2 summed directly keeps it, |a|^2 + |b|^2 - 2 a.b cannot (its
                           rounding is 6e-8 of |a|^2 ~ 1 against distances^2 of 1e-6).

Forward values without an existing bound (gem_pool, embed_normalize_, pairwise_sqdist) are bounded per case by
max(8 x e32, 1e-6 x max |ref|), e32 = max |fp32 - float64| of the restatement run in fp32 CPU torch on the same input (the
reference's own arithmetic; 8 x for another, fixed, summation order). Every test prints its figures before it asserts.

Measured (worst over the cases of each test; errors as fractions of the scale the bound is relative to). "fp32 torch" is the CPU
run the bound comes from or is confirmed by; "kernel" is an MI355X; "before" is the same kernel before this file existed, where it
missed the bound -- plain sums of a and a^2 in witw_bn_train_stats, one running sum in witw_pairwise_sqdist:

  quantity                                    bound               fp32 torch   kernel     before
  bn mean / invstd           (9 shapes)       1e-5                3e-8 / 1e-7  3e-7 / 1e-6   invstd 8e-5 (n = 2), 6e-5 (n = 3)
  bn scale / shift                            1e-5                2e-7 / 9e-8  1e-6 / 1e-6
  bn running mean / var                       1e-5                9e-8 / 1e-7  1e-7 / 3e-7
  bn invstd, |mean| / std = 0                 1e-5                6e-8         3e-7       1e-7
  bn invstd, |mean| / std = 1                 1e-5                8e-8         6e-7       3e-7
  bn invstd, |mean| / std = 16                1e-5                7e-8         4e-7       4.4e-5 (row kernel), 1.3e-5 (scalar)
  bn invstd, |mean| / std = 64                1e-5                8e-8         7e-7       6.4e-4 (row kernel), 3.2e-4 (scalar)
  gem_pool f                                  max(8 e32, 1e-6)    1.1e-7       1.4e-7
  gem_pool_bwd dy                             2e-5                -            3.4e-7
  embed_normalize_ f                          max(8 e32, 1e-6)    6e-8         6e-8
  embed_normalize_bwd dg                      2e-5                -            2e-7
  pairwise_sqdist D                           max(8 e32, 1e-6)    1.2e-7       3.9e-7     2.0e-6 at n = 1536 (bound 1.0e-6)
  true-pair distances (per element)           1e-5                1.6e-7       5.3e-7
  loss                                        1e-4                2e-7         1.1e-6
  de1 / de2                                   2e-5                -            7e-7
  chain loss / dz                             1e-4 / 2e-5         -            3e-7 / 1.4e-6
"""
import functools

import numpy as np
import pytest
import torch

from tests import baseline_head_ref as R

pytestmark = pytest.mark.gpu

JUNK = 57.0           # fills the padding of every input map: far outside the data, so a read of it moves any sum or mean


def _rng(stream, *case):
    return np.random.Generator(np.random.Philox(key=[stream, sum(int(v) * 4099 ** i for i, v in enumerate(case))]))


def _f32(g, shape, scale=1.0):
    return torch.from_numpy(g.standard_normal(shape, dtype=np.float32) * np.float32(scale))


def _dev(*ts):
    out = tuple(t.to('cuda:0') for t in ts)
    return out if len(out) > 1 else out[0]


def _pad_junk(x, valid_hw):
    H, W = valid_hw
    x[:, H:] = JUNK
    x[:, :, W:] = JUNK
    return x


def _maxerr(got, ref):
    return float((R.f64(got) - ref).abs().max())


def _fp32_bound(ref64, ref32):
    """max(8 x error of the fp32 restatement, 1e-6 x max |ref|) -> (bound, e32)"""
    e32 = _maxerr(ref32, ref64)
    return max(8.0 * e32, 1e-6 * float(ref64.abs().max())), e32


# ---------------------------------------------------------------------------------------------------------------- BatchNorm statistics

BN_SHAPES = [(3, 10, 12, (9, 11), 6),            # scalar sums
             (2, 6, 10, (6, 9), 12),             # scalar sums, C % 4 == 0
             (2, 6, 10, (5, 10), 20),            # scalar sums, C % 4 == 0
             (3, 7, 9, (5, 9), 64),              # row kernel
             (2, 4, 4, (3, 3), 512),             # row kernel, Q = 128
             (2, 3, 3, (2, 2), 1024),            # row kernel, one phase
             (5, 300, 3, (300, 3), 8),           # 1,500 rows, rows_per_block = 2
             (1, 1, 2, (1, 2), 64),              # n = 2, the smallest legal
             (3, 1, 1, (1, 1), 512)]             # block 7 of the golden step


def bn_case(shape, r=None):
    """-> (a [B,Hp,Wp,C] fp32 with junk padding, gamma, beta, running_mean0, running_var0). r: every channel of the valid region is
    standardised in float64 and given its own std s_c in [0.5, 2] and the mean +-r s_c, so |mean| / std = r up to fp32 rounding."""
    B, Hp, Wp, (H, W), C = shape
    g = _rng(401, B, Hp, Wp, C, 0 if r is None else r + 1)
    a = _f32(g, (B, Hp, Wp, C))
    if r is not None:
        v = a[:, :H, :W].double()
        v = (v - v.mean(dim=(0, 1, 2))) / v.var(dim=(0, 1, 2), unbiased=False).sqrt()
        s = torch.from_numpy(g.uniform(0.5, 2.0, (C,)))
        sign = torch.from_numpy(g.integers(0, 2, (C,)) * 2.0 - 1.0)
        a[:, :H, :W] = (v * s + r * s * sign).float()
    _pad_junk(a, (H, W))
    gamma, beta = 1 + 0.1 * _f32(g, (C,)), 0.1 * _f32(g, (C,))
    rm0, rv0 = 0.5 * _f32(g, (C,)), 0.5 + torch.from_numpy(g.random((C,), dtype=np.float32))
    return a, gamma, beta, rm0, rv0


def bn_errors(shape, a, gamma, beta, rm0, rv0, got):
    """got: (mean, invstd, scale, shift, running_mean, running_var) of an fp32 run -> each one's error as a fraction of its scale"""
    _B, _Hp, _Wp, valid, _C = shape
    s = R.bn_train_stats(a.double(), valid, gamma.double(), beta.double(), rm0.double(), rv0.double(), eps=1e-5, momentum=0.1)
    mean, invstd, scale, shift, rm, rv = (R.f64(t) for t in got)

    def rel(x, ref):
        return float(((x - ref).abs() / ref.abs()).max())

    def frac(x, ref, terms):
        return float((x - ref).abs().max() / terms.max())

    return {'mean': frac(mean, s.mean, torch.sqrt(s.mean ** 2 + s.var)), 'invstd': rel(invstd, s.invstd), 'scale': rel(scale, s.scale),
            'shift': frac(shift, s.shift, beta.double().abs() + (s.mean * s.scale).abs()),
            'running_mean': frac(rm, s.running_mean, 0.9 * rm0.double().abs() + 0.1 * s.mean.abs()),
            'running_var': rel(rv, s.running_var)}


def bn_fp32_torch(shape, a, gamma, beta, rm0, rv0):
    """torch's own fp32 BatchNorm (the reference's arithmetic) in the layout of `got` above"""
    _B, _Hp, _Wp, (H, W), _C = shape
    rm, rv = rm0.clone(), rv0.clone()
    x = a[:, :H, :W].permute(0, 3, 1, 2).contiguous()
    _y, mean, invstd = torch.native_batch_norm(x, gamma, beta, rm, rv, True, 0.1, 1e-5)
    scale = gamma * invstd
    return mean, invstd, scale, beta - mean * scale, rm, rv


def _run_bn(shape, r=None):
    from witw_amd import ops
    a, gamma, beta, rm0, rv0 = bn_case(shape, r)
    rm, rv = _dev(rm0.clone(), rv0.clone())
    mean, invstd, scale, shift = ops.bn_train_stats(_dev(a), shape[3], _dev(gamma), _dev(beta), rm, rv, eps=1e-5, momentum=0.1)
    err = bn_errors(shape, a, gamma, beta, rm0, rv0, (mean, invstd, scale, shift, rm, rv))
    e32 = bn_errors(shape, a, gamma, beta, rm0, rv0, bn_fp32_torch(shape, a, gamma, beta, rm0, rv0))
    print('bn_train_stats %s r=%s: kernel %s | fp32 torch %s' % (shape, r, {k: '%.1e' % v for k, v in err.items()},
                                                                {k: '%.1e' % v for k, v in e32.items()}))
    return err


@pytest.mark.parametrize('shape', BN_SHAPES)
def test_bn_train_stats_against_float64(shape):
    err = _run_bn(shape)
    for k, v in err.items():
        assert v <= 1e-5, (k, v)


@pytest.mark.parametrize('r', [0, 1, 16, 64])
@pytest.mark.parametrize('shape', [BN_SHAPES[0], BN_SHAPES[3]])
def test_bn_train_stats_conditioning(shape, r):
    """|mean| / std = r in every channel: 16 is the worst of the committed golden step (13.6 in block 7) rounded up, 64 four times
    that. A one-pass variance s1/n - mean^2 in fp32 loses r^2 x 6e-8 of invstd; sums about a pivot near the data do not."""
    err = _run_bn(shape, r)
    for k, v in err.items():
        assert v <= 1e-5, (k, v)


# ---------------------------------------------------------------------------------------------------------------- GeM

GEM_REGIONS = [(1, 1, (1, 1)), (4, 4, (2, 3)), (7, 9, (5, 9)), (13, 13, (13, 13))]


def gem_case(C, region, p, affine):
    Hp, Wp, (H, W) = region
    B = 3
    g = _rng(402, C, Hp, Wp, int(p * 10), int(affine))
    x = _pad_junk(_f32(g, (B, Hp, Wp, C)), (H, W))
    if affine:
        scale, shift = 1 + 0.1 * _f32(g, (C,)), 0.1 * _f32(g, (C,))
        if C > 1:            # channel 0 is negative everywhere after the affine: f = 0 exactly, and so is its gradient
            scale[0], shift[0] = -1.0, -(float(x[:, :H, :W, 0].abs().max()) + 1.0)
    else:
        scale, shift = torch.ones(C), torch.zeros(C)
    ldf = C + 64 + 7
    df = _f32(g, (B, ldf))
    base = _f32(g, (B, Hp, Wp, C))            # what the accumulating backward adds to: zeros in the padding, as depth_to_space2 leaves it
    base[:, H:] = 0
    base[:, :, W:] = 0
    return x, scale, shift, ldf, df, base


def gem_refs(x, valid, p, scale, shift, df_cols):
    """-> (f float64, f of the fp32 restatement, dy float64 on the valid region: the gradient at y = x * scale + shift, which is what
    witw_gem_pool_bwd hands to the BatchNorm backward, for the gradient df_cols at f; which f[b, c] are not 0)"""
    H, W = valid
    yr = (x.double()[:, :H, :W] * scale.double() + shift.double()).requires_grad_(True)
    f = R.gem_pool(yr, valid, p)
    (f * df_cols.double()).sum().backward()
    # f[b, c] = 0 means every pixel of that image and channel is negative: f stays 0 around such an input, so its gradient is 0
    # there -- autograd has none to give (pow(0, 1/p) differentiates to inf, times 0 from relu^p)
    live = f.detach() > 0
    dy = torch.where(live[:, None, None, :], yr.grad, torch.zeros((), dtype=torch.float64))
    assert bool(torch.isfinite(dy).all())
    with torch.no_grad():
        f32 = R.gem_pool(x, valid, p, scale, shift)
        assert torch.equal(f.detach(), R.gem_pool(x.double(), valid, p, scale.double(), shift.double()))
    return f.detach(), f32, dy, live


@pytest.mark.parametrize('region', GEM_REGIONS)
@pytest.mark.parametrize('C', [1, 63, 64, 65, 512])
def test_gem_pool_forward_and_backward(C, region):
    from witw_amd import ops
    Hp, Wp, (H, W) = region
    for p in (3.0, 2.5):
        for affine in (False, True):
            x, scale, shift, ldf, df, base = gem_case(C, region, p, affine)
            xd, scd, shd, dfd, based = _dev(x, scale, shift, df, base)
            for col0 in (0, 64, ldf - C):
                f64_, f32_, dy64, live = gem_refs(x, (H, W), p, scale, shift, df[:, col0:col0 + C])
                assert not (affine and C > 1) or not bool(live[:, 0].any())
                fill = torch.from_numpy(_rng(403, C, col0).standard_normal((x.shape[0], ldf), dtype=np.float32))
                out = _dev(fill.clone())
                ops.gem_pool(xd, (H, W), out, col0, p, scd if affine else None, shd if affine else None)
                got = out.cpu()
                keep = torch.ones(ldf, dtype=torch.bool)
                keep[col0:col0 + C] = False
                assert torch.equal(got[:, keep].view(torch.int32), fill[:, keep].view(torch.int32)), 'neighbouring columns changed'
                bound, e32 = _fp32_bound(f64_, f32_)
                err = _maxerr(got[:, ~keep], f64_)
                print('gem_pool C=%d %s p=%s affine=%s col0=%d: err %.2e, fp32 torch %.2e, bound %.2e (max |f| %.2e)'
                      % (C, region, p, affine, col0, err, e32, bound, float(f64_.abs().max())))
                assert err <= bound
                assert bool((got[:, ~keep][~live] == 0).all())
                # backward, fresh: zeros in the padding and in the dead channel, values against autograd
                dy = ops.gem_pool_bwd(xd, scd, shd, out, dfd, (H, W), col0, p)
                dyc = dy.cpu()
                assert bool(torch.isfinite(dyc).all())
                assert float(dyc[:, H:].abs().sum()) == 0.0 and float(dyc[:, :, W:].abs().sum()) == 0.0
                assert bool((dyc[:, :H, :W][~live[:, None, None, :].expand(-1, H, W, -1)] == 0).all())
                scale_dy = float(dy64.abs().max())
                err = _maxerr(dyc[:, :H, :W], dy64)
                print('gem_pool_bwd: err %.2e of max |dy| %.2e' % (err / scale_dy, scale_dy))
                assert err <= 2e-5 * scale_dy
                # accumulating: the same values added to what is there, the padding left as it is
                acc = ops.gem_pool_bwd(xd, scd, shd, out, dfd, (H, W), col0, p, out=based.clone())
                assert torch.equal(acc, based + dy)


# ---------------------------------------------------------------------------------------------------------------- normalisation

@pytest.mark.parametrize('B,n', [(1, 1), (3, 161), (2, 256), (2, 257), (3, 1536)])
def test_embed_normalize_forward_and_backward(B, n):
    from witw_amd import ops
    g = _rng(404, B, n)
    f0 = _f32(g, (B, n)).abs() + 0.01          # GeM outputs are non-negative
    df = _f32(g, (B, n))
    fr = f0.double().requires_grad_(True)
    ref = R.embed_normalize(fr)
    (ref * df.double()).sum().backward()
    bound, e32 = _fp32_bound(ref.detach(), R.embed_normalize(f0))
    got = ops.embed_normalize_(_dev(f0.clone()))
    err = _maxerr(got, ref.detach())
    print('embed_normalize_ (%d, %d): err %.2e, fp32 torch %.2e, bound %.2e' % (B, n, err, e32, bound))
    assert err <= bound
    dg = ops.embed_normalize_bwd(_dev(f0), _dev(df))
    scale = float(fr.grad.abs().max())
    err = _maxerr(dg, fr.grad)
    print('embed_normalize_bwd: err %.2e of max |dg| %.2e' % (err / scale, scale))
    assert err <= 2e-5 * scale


# ---------------------------------------------------------------------------------------------------------------- distances

@pytest.mark.parametrize('take_sqrt', [False, True])
@pytest.mark.parametrize('Na,Nb,n', [(1, 1, 1), (37, 29, 70), (3, 257, 1536), (300, 300, 64)])
def test_pairwise_sqdist_against_float64(Na, Nb, n, take_sqrt):
    from witw_amd import ops
    g = _rng(405, Na, Nb, n)
    a, b = _f32(g, (Na, n)), _f32(g, (Nb, n))
    ref = R.pairwise_sqdist(a.double(), b.double(), take_sqrt)
    bound, e32 = _fp32_bound(ref, R.pairwise_sqdist(a, b, take_sqrt))
    got = ops.pairwise_sqdist(_dev(a), _dev(b), take_sqrt=take_sqrt)
    assert got.shape == (Na, Nb)
    err = _maxerr(got, ref)
    print('pairwise_sqdist (%d, %d, %d) sqrt=%s: err %.2e, fp32 torch %.2e, bound %.2e (max |D| %.2e)'
          % (Na, Nb, n, take_sqrt, err, e32, bound, float(ref.abs().max())))
    assert err <= bound


@pytest.mark.parametrize('take_sqrt', [False, True])
def test_pairwise_sqdist_keeps_the_small_distances_of_true_pairs(take_sqrt):
    """b = a + 1e-3 noise with |a| ~ |noise| ~ 1: the true-pair distances^2 are 1e-6 next to 2 for every other pair."""
    from witw_amd import ops
    g = _rng(406, int(take_sqrt))
    a = _f32(g, (37, 1536), 1536 ** -0.5)
    b = a + 1e-3 * _f32(g, (37, 1536), 1536 ** -0.5)
    ref = R.pairwise_sqdist(a.double(), b.double(), take_sqrt)
    assert float(torch.diagonal(ref).max()) < (2e-3 if take_sqrt else 4e-6)
    got = R.f64(ops.pairwise_sqdist(_dev(a), _dev(b), take_sqrt=take_sqrt))
    rel = ((got - ref).abs() / ref)
    e32 = ((R.pairwise_sqdist(a, b, take_sqrt).double() - ref).abs() / ref)
    print('true pairs sqrt=%s: worst relative error %.2e (diagonal %.2e), fp32 torch %.2e'
          % (take_sqrt, float(rel.max()), float(torch.diagonal(rel).max()), float(e32.max())))
    assert float(rel.max()) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- exhaustive loss

LOSS_CFGS = {'hard_m1': dict(soft_margin=False, margin=1.0), 'hard_m03': dict(soft_margin=False, margin=0.3),
             'soft_a10': dict(soft_margin=True, alpha=10.0), 'soft_a2': dict(soft_margin=True, alpha=2.0)}
GRAD_LOSS = 0.37
KINK = 1e-4


@functools.lru_cache(maxsize=None)
def loss_inputs(B, n):
    """Embeddings in clusters of about 8 rows, centres 3 apart on axis 0 (distances^2 >= 9 across clusters: terms far below the
    kink, zero gradient); inside a cluster |a_i - a_j|^2 ~ 0.6 and the true-pair distance^2 t_i^2 is spread over [0.05, 1.5], so
    x = D_ii - D_ij runs over about [-2, 0.9] and both margins cut through the terms -- which terms are active depends on D_ii and
    D_jj alike. The seed is advanced until no hard-margin term of the float64 reference is within KINK of x + margin = 0
    (and, for the batches of 2 and 3, until some term is active)."""
    K = (B + 7) // 8
    for seed in range(64):
        g = _rng(407, B, n, seed)
        a = _f32(g, (B, n), (0.3 / n) ** 0.5)
        a[:, 0] += 3.0 * (torch.arange(B) % K).float()
        t = torch.from_numpy(g.uniform(0.05, 1.5, (B, 1)).astype(np.float32)).sqrt()
        b = a + t * _f32(g, (B, n), n ** -0.5)
        D = R.pairwise_sqdist(a.double(), b.double())
        terms = [R.triplet_terms(D, m) for m in (1.0, 0.3)]
        gaps = [float(x.abs().min()) for x in terms]
        if min(gaps) > KINK and all(bool((x > 0).any()) for x in terms):          # and each margin leaves some term active
            return a, b, seed, gaps
    raise AssertionError('no seed keeps the hard-margin terms clear of the kink at B=%d n=%d' % (B, n))


@functools.lru_cache(maxsize=None)
def loss_refs(B, n, cfg):
    a, b, _seed, _gaps = loss_inputs(B, n)
    loss, D, d1, d2 = R.exhaustive_triplet_loss_grads(a.double(), b.double(), GRAD_LOSS, **LOSS_CFGS[cfg])
    if not LOSS_CFGS[cfg]['soft_margin']:
        x = R.triplet_terms(D, LOSS_CFGS[cfg]['margin'])
        assert float(x.abs().min()) > KINK
        near = x[x > -4.0]          # the terms inside a cluster; the others are 9 and more below
        assert B < 37 or 0.05 < float((near > 0).double().mean()) < 0.95, 'the margin must cut through the terms'
    return loss, d1, d2


@pytest.mark.parametrize('cfg', sorted(LOSS_CFGS))
@pytest.mark.parametrize('n', [8, 1536])
@pytest.mark.parametrize('B', [2, 3, 37, 256, 257, 300])
def test_exhaustive_triplet_loss_and_backward(B, n, cfg):
    from witw_amd import ops
    a, b, seed, gaps = loss_inputs(B, n)
    loss, d1, d2 = loss_refs(B, n, cfg)
    kw = LOSS_CFGS[cfg]
    ad, bd = _dev(a, b)
    D = ops.pairwise_sqdist(ad, bd)
    got = ops.exhaustive_triplet_loss(D, **kw)
    g1, g2 = ops.exhaustive_triplet_loss_bwd(ad, bd, D, torch.tensor([GRAD_LOSS], device=ad.device), **kw)
    e1, e2 = _maxerr(g1, d1) / float(d1.abs().max()), _maxerr(g2, d2) / float(d2.abs().max())
    print('loss B=%d n=%d %s (seed %d, nearest term to the kink %.1e): loss %.6e rel err %.1e; de1 %.1e de2 %.1e of their max'
          % (B, n, cfg, seed, min(gaps), loss.item(), abs(got.item() - loss.item()) / abs(loss.item()), e1, e2))
    assert float(loss) > 0 and float(d1.abs().max()) > 0
    assert abs(got.item() - loss.item()) <= 1e-4 * abs(loss.item())
    assert e1 <= 2e-5 and e2 <= 2e-5


# ---------------------------------------------------------------------------------------------------------------- depth-to-space

@pytest.mark.parametrize('case', [(2, 7, 9, (5, 9), 6, 24), (1, 8, 8, (8, 8), 8, 32), (3, 6, 7, (5, 6), 3, 16), (2, 5, 5, (1, 1), 64, 256),
                                  (2, 4, 6, (4, 5), 5, 24)])
def test_depth_to_space2_is_the_indexing_definition_and_inverts_space_to_depth(case):
    from witw_amd import ops
    B, Hp, Wp, (H, W), C, Cp = case
    g = _rng(408, Hp, Wp, C)
    gs = _f32(g, (B, (H + 1) // 2, (W + 1) // 2, Cp))
    add = _pad_junk(_f32(g, (B, Hp, Wp, C)), (H, W))
    like = torch.empty((B, Hp, Wp, C), device='cuda:0')
    for ad in (None, add):
        got = ops.depth_to_space2(_dev(gs), like, (H, W), add=None if ad is None else _dev(ad)).cpu()
        want = R.depth_to_space2(gs, (Hp, Wp), (H, W), C, add=ad)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    x = _dev(_pad_junk(_f32(g, (B, Hp, Wp, C)), (H, W)))
    back = ops.depth_to_space2(ops.space_to_depth2(x, valid_hw=(H, W), cpad=Cp), like, (H, W))
    want = torch.zeros_like(x)
    want[:, :H, :W] = x[:, :H, :W]
    assert torch.equal(back.view(torch.int32), want.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- the chain

CHAIN_MAPS = [(16, 16, (13, 13)), (8, 8, (5, 5)), (4, 4, (1, 1))]         # blocks 5-7: valid 13 x 13, 5 x 5, 1 x 1 inside their padded maps
CHAIN_B, CHAIN_C, CHAIN_P = 5, 64, 3.0


def chain_case():
    g = _rng(409)
    sides = []
    for _side in range(2):
        maps = []
        for Hp, Wp, (H, W) in CHAIN_MAPS:
            z = _f32(g, (CHAIN_B, Hp, Wp, CHAIN_C))
            # GeM of an all-negative map is 0 with no derivative: beta keeps some pixel of every (image, channel) positive -- on the
            # 1 x 1 map that is the only pixel, and |xhat| <= (n - 1) / sqrt(n) = 1.79 over n = 5 samples
            gamma, beta = 1 + 0.1 * _f32(g, (CHAIN_C,)), (2.5 if (H, W) == (1, 1) else 0.3) + 0.1 * _f32(g, (CHAIN_C,))
            # the gradient the next block's data-gradient conv hands to blocks 5 and 6, in its space-to-depth layout (none for block 7)
            up = None if (H, W) == (1, 1) else 0.05 * _f32(g, (CHAIN_B, (H + 1) // 2, (W + 1) // 2, 4 * CHAIN_C))
            maps.append((z, gamma, beta, up))
        sides.append(maps)
    return sides


def chain_reference(sides, soft_margin):
    """float64 autograd of the restatement: loss + sum_i <y_i, up_i> (the second term is what hands `up` to blocks 5 and 6)"""
    zs, embeds, extra = [], [], 0.0
    for maps in sides:
        feats = []
        for (Hp, Wp, valid), (z, gamma, beta, up) in zip(CHAIN_MAPS, maps):
            zr = z.double().requires_grad_(True)
            zs.append(zr)
            y = R.bn_lrelu(zr, valid, gamma.double(), beta.double())
            feats.append(R.gem_pool(y, valid, CHAIN_P))
            assert float(feats[-1].detach().min()) > 0
            if up is not None:
                extra = extra + (y * R.depth_to_space2(up.double(), valid, valid, CHAIN_C)).sum()
        embeds.append(R.embed_normalize(torch.cat(feats, 1)))
    loss = R.exhaustive_triplet_loss(embeds[0], embeds[1], soft_margin=soft_margin)
    (loss * GRAD_LOSS + extra).backward()
    return loss.detach(), [zr.grad for zr in zs], R.triplet_terms(R.pairwise_sqdist(embeds[0], embeds[1]).detach(), 1.0)


@pytest.mark.parametrize('soft_margin', [False, True])
def test_head_chain_forward_and_backward(soft_margin):
    """BatchNorm statistics -> GeM of three maps into one [B, 192] row -> normalisation -> distances -> loss, and back through
    exhaustive_triplet_loss_bwd, embed_normalize_bwd, gem_pool_bwd (fresh for the last map, onto depth_to_space2's output for the
    other two) and bn_lrelu_bwd, in the order cvig_baseline._EncoderTrainFn calls them, for both encoders' sides."""
    from witw_amd import ops
    sides = chain_case()
    loss_ref, dz_ref, terms = chain_reference(sides, soft_margin)
    assert soft_margin or float(terms.abs().min()) > KINK
    nC = CHAIN_C * len(CHAIN_MAPS)
    embeds, saved = [], []
    for maps in sides:
        gfeat = torch.empty((CHAIN_B, nC), device='cuda:0')
        keep = []
        for i, ((Hp, Wp, valid), (z, gamma, beta, up)) in enumerate(zip(CHAIN_MAPS, maps)):
            a = _dev(_pad_junk(torch.nn.functional.leaky_relu(z, 0.2), valid))
            gm = _dev(gamma)
            mean, invstd, scale, shift = ops.bn_train_stats(a, valid, gm, _dev(beta))
            ops.gem_pool(a, valid, gfeat, CHAIN_C * i, CHAIN_P, scale, shift)
            keep.append((a, valid, gm, mean, invstd, scale, shift, up))
        embeds.append(ops.embed_normalize_(gfeat.clone()))
        saved.append((gfeat, keep))
    D = ops.pairwise_sqdist(embeds[0], embeds[1])
    kw = dict(soft_margin=soft_margin, alpha=10.0, margin=1.0)
    loss = ops.exhaustive_triplet_loss(D, **kw)
    print('chain soft=%s: loss %.6e, rel err %.1e' % (soft_margin, loss_ref.item(), abs(loss.item() - loss_ref.item()) / loss_ref.item()))
    assert abs(loss.item() - loss_ref.item()) <= 1e-4 * abs(loss_ref.item())
    des = ops.exhaustive_triplet_loss_bwd(embeds[0], embeds[1], D, torch.tensor([GRAD_LOSS], device='cuda:0'), **kw)
    k = 0
    for (gfeat, keep), de in zip(saved, des):
        dg = ops.embed_normalize_bwd(gfeat, de)
        got = {}
        for i in (2, 1, 0):
            a, valid, gm, mean, invstd, scale, shift, up = keep[i]
            if up is None:
                dy = ops.gem_pool_bwd(a, scale, shift, gfeat, dg, valid, CHAIN_C * i, CHAIN_P)
            else:
                dy = ops.depth_to_space2(_dev(up), a, valid)
                ops.gem_pool_bwd(a, scale, shift, gfeat, dg, valid, CHAIN_C * i, CHAIN_P, out=dy)
            got[i], _dgamma, _dbeta = ops.bn_lrelu_bwd(a, dy, valid, mean, invstd, gm, 0.2)
        for i in range(3):
            H, W = keep[i][1]
            want = dz_ref[k][:, :H, :W]
            k += 1
            dz = got[i].cpu()
            assert float(dz[:, H:].abs().sum()) == 0.0 and float(dz[:, :, W:].abs().sum()) == 0.0
            scale_dz = float(want.abs().max())
            err = _maxerr(dz[:, :H, :W], want)
            print('chain dz map %d: err %.2e of max |dz| %.2e' % (i, err / scale_dz, scale_dz))
            assert scale_dz > 0 and err <= 2e-5 * scale_dz
