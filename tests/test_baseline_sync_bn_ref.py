"""tests/baseline_sync_bn_ref.py on its own (no GPU): the split BatchNorm arithmetic -- partial sums per share, the shares added,
then the second entry -- is the one-shot arithmetic of the whole batch. These pin the formula the GPU tests hold the kernels to.

Bounds (float64 throughout, u = 1.1e-16): sums about a pivot 100 sigma from the mean carry terms of 1e4 sigma^2 into a variance of
sigma^2, so the variance keeps about 1e4 x n u < 1e-9 of itself at the sizes used; everything else is far below. rtol = 1e-9."""
import numpy as np
import pytest
import torch

from tests import baseline_sync_bn_ref as S

RTOL = 1e-9
CASE = (7, 6, 10, (5, 9), 8)            # B, Hp, Wp, (H, W), C: a valid region smaller than the padded one
SPLITS = [(7,), (3, 4), (1, 4, 2)]      # batch shares: whole, K = 2, K = 3 (unequal)


def _case(seed=0):
    B, Hp, Wp, (H, W), C = CASE
    g = np.random.Generator(np.random.Philox(key=[501, seed]))
    a = g.standard_normal((B, Hp, Wp, C)) * g.uniform(0.5, 2.0, (C,)) + g.uniform(-3.0, 3.0, (C,))
    a[:, H:] = 57.0
    a[:, :, W:] = 57.0
    return g, a


def _shares(x, split):
    edges = np.cumsum((0,) + tuple(split))
    return [x[lo:hi] for lo, hi in zip(edges[:-1], edges[1:])]


@pytest.mark.parametrize('pivot_kind', ['zero', 'mean_plus_100_sigma'])
@pytest.mark.parametrize('split', SPLITS)
def test_partials_summed_then_finalised_are_the_one_shot_statistics(split, pivot_kind):
    B, _Hp, _Wp, (H, W), C = CASE
    g, a = _case()
    v = a[:, :H, :W, :]
    mean, var = v.mean(axis=(0, 1, 2)), v.var(axis=(0, 1, 2))
    pivot = np.zeros(C) if pivot_kind == 'zero' else mean + 100.0 * np.sqrt(var)
    gamma, beta = 1 + 0.1 * g.standard_normal(C), 0.1 * g.standard_normal(C)
    rm0, rv0 = 0.5 * g.standard_normal(C), 0.5 + g.random(C)
    part = sum(S.partial_stats(s, (H, W), pivot) for s in _shares(a, split))
    n = B * H * W
    st = S.finalize_stats(part, pivot, n, gamma, beta, rm0, rv0, eps=1e-5, momentum=0.1)
    np.testing.assert_allclose(st.mean, mean, rtol=RTOL, atol=RTOL * float(np.abs(mean).max()))
    np.testing.assert_allclose(st.var, var, rtol=RTOL)
    np.testing.assert_allclose(st.invstd, 1.0 / np.sqrt(var + 1e-5), rtol=RTOL)
    np.testing.assert_allclose(st.scale, gamma * st.invstd, rtol=RTOL)
    np.testing.assert_allclose(st.shift, beta - mean * gamma / np.sqrt(var + 1e-5), rtol=RTOL, atol=RTOL)
    # torch's own float64 BatchNorm on the concatenation, running buffers included
    rm, rv = torch.from_numpy(rm0.copy()), torch.from_numpy(rv0.copy())
    x = torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)))
    _y, tmean, tinvstd = torch.native_batch_norm(x, torch.from_numpy(gamma), torch.from_numpy(beta), rm, rv, True, 0.1, 1e-5)
    np.testing.assert_allclose(st.mean, tmean.numpy(), rtol=RTOL, atol=RTOL * float(np.abs(mean).max()))
    np.testing.assert_allclose(st.invstd, tinvstd.numpy(), rtol=RTOL)
    np.testing.assert_allclose(st.running_mean, rm.numpy(), rtol=RTOL, atol=RTOL)
    np.testing.assert_allclose(st.running_var, rv.numpy(), rtol=RTOL)


def test_finalize_refuses_one_value_per_channel():
    with pytest.raises(ValueError):
        S.finalize_stats(np.zeros(8), np.zeros(4), 1, np.ones(4), np.zeros(4))


@pytest.mark.parametrize('split', SPLITS)
def test_backward_partials_summed_then_applied_are_autograd_of_the_whole_batch(split):
    """against torch's float64 autograd of F.batch_norm(F.leaky_relu(z, 0.2), training=True) on the concatenated batch: dz, dgamma, dbeta"""
    B, Hp, Wp, (H, W), C = CASE
    g, z = _case(1)
    dy = g.standard_normal((B, Hp, Wp, C))
    dy[:, H:] = 57.0
    dy[:, :, W:] = 57.0
    gamma, beta = 1 + 0.1 * g.standard_normal(C), 0.1 * g.standard_normal(C)
    zr = torch.from_numpy(np.ascontiguousarray(z[:, :H, :W].transpose(0, 3, 1, 2))).requires_grad_(True)
    gr, br = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
    y = torch.nn.functional.batch_norm(torch.nn.functional.leaky_relu(zr, 0.2), None, None, gr, br, True, 0.1, 1e-5)
    y.backward(torch.from_numpy(np.ascontiguousarray(dy[:, :H, :W].transpose(0, 3, 1, 2))))
    want = zr.grad.numpy().transpose(0, 2, 3, 1)

    a = np.where(z > 0, z, 0.2 * z)
    n = B * H * W
    pivot = np.zeros(C)
    st = S.finalize_stats(sum(S.partial_stats(s, (H, W), pivot) for s in _shares(a, split)), pivot, n, gamma, beta)
    sums = sum(S.bwd_partial(sa, sd, (H, W), st.mean, st.invstd) for sa, sd in zip(_shares(a, split), _shares(dy, split)))
    dz = np.concatenate([S.bwd_apply(sa, sd, (H, W), st.mean, st.invstd, gamma, sums, n, 0.2)
                         for sa, sd in zip(_shares(a, split), _shares(dy, split))])
    assert dz.shape == a.shape and float(np.abs(dz[:, H:]).max()) == 0.0 and float(np.abs(dz[:, :, W:]).max()) == 0.0
    np.testing.assert_allclose(dz[:, :H, :W], want, rtol=RTOL, atol=RTOL * float(np.abs(want).max()))
    np.testing.assert_allclose(sums[:C], br.grad.numpy(), rtol=RTOL, atol=RTOL * float(np.abs(br.grad.numpy()).max()))
    np.testing.assert_allclose(sums[C:], gr.grad.numpy(), rtol=RTOL, atol=RTOL * float(np.abs(gr.grad.numpy()).max()))
    # the space-to-depth form of dy is the same gradient, element for element
    s2d = S.space_to_depth2(dy, (H, W), 4 * C + 4)
    for h in range(H):
        for w in range(W):
            k = ((h & 1) * 2 + (w & 1)) * C
            assert np.array_equal(s2d[:, h >> 1, w >> 1, k:k + C], dy[:, h, w, :])
