"""tests/baseline_head_ref.py (the float64 reference of the cvig_baseline head tests) tied to what the project already trusts:
oracle/cvig_baseline_oracle.py (itself pinned to the reference by tests/test_oracle_golden.py), the four loss goldens of
tests/golden/baseline.npz, and torch's own float64 BatchNorm. CPU only."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cvig_baseline_oracle as OB
from tests import baseline_head_ref as R
from witw_amd import synth


def _rng(stream, *case):
    return np.random.Generator(np.random.Philox(key=[stream, sum(int(v) * 4099 ** i for i, v in enumerate(case))]))


def _t(g, shape, scale=1.0):
    return torch.from_numpy(g.standard_normal(shape) * scale)          # float64


def test_loss_restatement_meets_the_reference_goldens(golden_dir):
    g = np.load(os.path.join(golden_dir, 'baseline.npz'))
    seed = int(g['seed'])
    e1 = torch.from_numpy(synth.embeddings(seed, 600, (5, 1536))) * 0.018
    e2 = e1 + torch.from_numpy(synth.embeddings(seed, 601, (5, 1536))) * 0.02
    # The goldens are the reference's fp32 run, so float64 differs from them by the golden's own rounding: distances of 0.6 and 1.6
    # carry 6e-8 each, which is 2e-6 of loss_hard (terms of 0.01-0.1) and up to 1e-5 of loss_hard_m03 (terms of a few 1e-3); in
    # loss_soft every term is log(1 + 4.5e-5) with the sum 1 + 4.5e-5 rounded to fp32's 6e-8 grid, up to 1.3e-3 of the term (the
    # rtol test_baseline_loss_and_ranks gives it too); loss_soft_a2's terms are O(0.1).
    for key, (a, b), kw, rtol in (('loss_hard', (e1, e2), {}, 2e-6), ('loss_soft', (e1, e2), {'soft_margin': True}, 1e-3),
                                  ('loss_hard_m03', (e1 * 0.55, e2 * 0.55), {'margin': 0.3}, 1e-5),
                                  ('loss_soft_a2', (e1, e2), {'soft_margin': True, 'alpha': 2.}, 2e-6)):
        np.testing.assert_allclose(R.exhaustive_triplet_loss(a.double(), b.double(), **kw).item(), float(g[key]), rtol=rtol)
        # the restatement run in fp32 is the reference's arithmetic: one fp32 rounding of the final sum at the most
        np.testing.assert_allclose(R.exhaustive_triplet_loss(a, b, **kw).item(), float(g[key]), rtol=2e-7)


@pytest.mark.parametrize('B,n', [(2, 8), (3, 5), (7, 33), (37, 16)])
@pytest.mark.parametrize('kw', [{}, {'margin': 0.3}, {'soft_margin': True}, {'soft_margin': True, 'alpha': 2.}])
def test_loss_and_distances_against_the_oracle(B, n, kw):
    g = _rng(301, B, n)
    e1 = _t(g, (B, n), 0.5)
    e2 = e1 + _t(g, (B, n), 0.4)
    want = OB.exhaustive_minibatch_triplet_loss(e1, e2, **kw)          # the roll form, in float64
    got = R.exhaustive_triplet_loss(e1, e2, **kw)
    assert got.dtype == torch.float64
    np.testing.assert_allclose(got.item(), want.item(), rtol=1e-12)
    # gradients: autograd through the oracle's roll form against the two-stage autograd of the restatement
    a, b = e1.clone().requires_grad_(True), e2.clone().requires_grad_(True)
    (OB.exhaustive_minibatch_triplet_loss(a, b, **kw) * 0.37).backward()
    loss, D, d1, d2 = R.exhaustive_triplet_loss_grads(e1, e2, 0.37, rows=3, **kw)
    np.testing.assert_allclose(loss.item(), want.item(), rtol=1e-12)
    np.testing.assert_allclose(d1.numpy(), a.grad.numpy(), rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(d2.numpy(), b.grad.numpy(), rtol=1e-9, atol=1e-14)
    # distances: the oracle's ranking distances (model/cvig_baseline.py:458) and the chunked form against one broadcast
    for q in range(B):
        want_d = torch.pow(torch.sum(torch.pow(e1 - e2[q][None], 2), dim=1), 0.5)
        np.testing.assert_allclose(R.pairwise_sqdist(e1, e2, take_sqrt=True, rows=2)[:, q].numpy(), want_d.numpy(), rtol=1e-13)
    np.testing.assert_allclose(D.numpy(), ((e2[None] - e1[:, None]) ** 2).sum(2).numpy(), rtol=1e-13)
    assert R.triplet_terms(D, 0.3).shape == (2, B, B - 1)
    if not kw.get('soft_margin'):
        m = kw.get('margin', 1.)
        np.testing.assert_allclose(torch.relu(R.triplet_terms(D, m)).sum().item() / (2 * B * (B - 1)), want.item(), rtol=1e-12)


@pytest.mark.parametrize('case', [(3, 10, 12, (9, 11), 6), (2, 4, 4, (3, 3), 16), (1, 1, 2, (1, 2), 5), (3, 1, 1, (1, 1), 7)])
def test_batchnorm_restatement_against_torch_float64(case):
    B, Hp, Wp, (H, W), C = case
    g = _rng(302, C, Hp)
    a = _t(g, (B, Hp, Wp, C)) + 3.0
    gamma, beta = 1 + 0.1 * _t(g, (C,)), 0.1 * _t(g, (C,))
    rm0, rv0 = 0.5 * _t(g, (C,)), 0.5 + torch.from_numpy(g.random((C,)))
    s = R.bn_train_stats(a, (H, W), gamma, beta, rm0, rv0, eps=1e-5, momentum=0.1)
    rm, rv = rm0.clone(), rv0.clone()
    x = a[:, :H, :W].permute(0, 3, 1, 2).contiguous()
    y, save_mean, save_invstd = torch.native_batch_norm(x, gamma, beta, rm, rv, True, 0.1, 1e-5)
    for got, want in ((s.mean, save_mean), (s.invstd, save_invstd), (s.running_mean, rm), (s.running_var, rv)):
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose((a[:, :H, :W] * s.scale + s.shift).numpy(), y.permute(0, 2, 3, 1).numpy(), rtol=1e-10, atol=1e-10)
    rm2, rv2 = rm0.clone(), rv0.clone()
    y2 = F.batch_norm(F.leaky_relu(x, 0.2), rm2, rv2, gamma, beta, True, 0.1, 1e-5)
    np.testing.assert_allclose(R.bn_lrelu(a, (H, W), gamma, beta).numpy(), y2.permute(0, 2, 3, 1).numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(s.var.numpy(), x.var(dim=(0, 2, 3), unbiased=False).numpy(), rtol=1e-11)


def test_head_restatement_against_the_oracle_encoder_tail():
    """GeM (three maps into one row) and the normalisation against the tail of oracle.encoder_forward, in float64: the oracle's
    blocks 5-7 are re-run here on a random block-4 output, train-mode BatchNorm included."""
    g = _rng(303)
    B = 3
    x = _t(g, (B, 8, 30, 30))
    prm = [{'w': _t(g, (co, ci, 4, 4), 0.1), 'b': _t(g, (co,), 0.1), 'gamma': 1 + 0.1 * _t(g, (co,)), 'beta': 0.1 * _t(g, (co,)),
            'mean': torch.zeros(co, dtype=torch.float64), 'var': torch.ones(co, dtype=torch.float64)}
           for ci, co in ((8, 12), (12, 10), (10, 9))]
    feats, h = [], x
    for q in prm:                      # oracle.encoder_forward's loop body for i >= 4 with train=True (its first four blocks left out)
        z = F.conv2d(h, q['w'], q['b'], stride=2)
        a = F.leaky_relu(z, 0.2)
        h = F.batch_norm(a, q['mean'].clone(), q['var'].clone(), q['gamma'], q['beta'], training=True, momentum=0.1, eps=1e-5)
        feats.append(torch.pow(torch.mean(torch.pow(F.relu(h), 3.), [2, 3]), 1. / 3.))
        # the restatement on the same activation, NHWC inside a padded map
        vh, vw = a.shape[2:]
        ap = torch.full((B, vh + 1, vw + 2, a.shape[1]), 7.0, dtype=torch.float64)
        ap[:, :vh, :vw] = a.permute(0, 2, 3, 1)
        s = R.bn_train_stats(ap, (vh, vw), q['gamma'], q['beta'])
        np.testing.assert_allclose(R.gem_pool(ap, (vh, vw), 3., s.scale, s.shift).numpy(), feats[-1].numpy(), rtol=1e-10)
        np.testing.assert_allclose(R.gem_pool(h.permute(0, 2, 3, 1), (vh, vw), 3.).numpy(), feats[-1].numpy(), rtol=1e-12)
    f = torch.cat(feats, 1)
    want = f / torch.unsqueeze(torch.pow(torch.linalg.norm(f, dim=1), 0.5), 1)
    np.testing.assert_allclose(R.embed_normalize(f).numpy(), want.numpy(), rtol=1e-14)


def test_whole_oracle_encoder_ends_in_the_restated_head():
    """oracle.encoder_forward itself (eval mode, fp32) on one small image against its own convolutions followed by the restated
    GeM and normalisation."""
    prm = [{k: torch.from_numpy(v) for k, v in q.items()} for q in synth.baseline_params(11)]
    x = torch.from_numpy(synth.images_u8(11, 1, (1, 3, 382, 382))).float()
    with torch.no_grad():
        want = OB.encoder_forward(x, prm)
        h, feats = -1. + 2. * (x / 255.), []
        for i, q in enumerate(prm):
            h = F.batch_norm(F.leaky_relu(F.conv2d(h, q['w'], q['b'], stride=2), 0.2), q['mean'], q['var'], q['gamma'], q['beta'],
                             training=False, eps=1e-5)
            if i >= 4:
                feats.append(R.gem_pool(h.permute(0, 2, 3, 1), tuple(h.shape[2:]), 3.))
        got = R.embed_normalize(torch.cat(feats, 1))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize('case', [(2, 5, 7, (5, 7), 3, 12), (1, 6, 6, (4, 3), 2, 11), (2, 3, 3, (1, 1), 4, 16)])
def test_depth_to_space_restatement_inverts_space_to_depth(case):
    B, Hp, Wp, (H, W), C, Cp = case
    g = _rng(304, Hp, C)
    x = _t(g, (B, Hp, Wp, C))
    xv = torch.zeros((B, 2 * ((H + 1) // 2), 2 * ((W + 1) // 2), C), dtype=torch.float64)
    xv[:, :H, :W] = x[:, :H, :W]
    s2d = torch.zeros((B, (H + 1) // 2, (W + 1) // 2, Cp), dtype=torch.float64)
    s2d[..., :4 * C] = torch.cat([xv[:, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)], dim=3)      # as tests/test_baseline_gpu.py
    back = R.depth_to_space2(s2d, (Hp, Wp), (H, W), C)
    want = torch.zeros_like(x)
    want[:, :H, :W] = x[:, :H, :W]
    assert torch.equal(back, want)
    assert torch.equal(R.depth_to_space2(s2d, (Hp, Wp), (H, W), C, add=x), want * 2)
