"""The Adam references of tests/adam_ref.py checked on the CPU: the fp32 restatement of adam_kernel against float64 within the
derived rounding bound, the float64 formula against torch.optim.Adam in float64, and every deliberately wrong variant changing
the expected bits of every case it applies to (so the GPU tests' bit equality rules each of them out)."""
import numpy as np
import pytest
import torch

from . import adam_ref as R

HYPERS = [dict(), dict(lr=3e-4, b1=0.8, b2=0.99, eps=1e-6)]
STEPS = [1, 2, 10, 1000, 100000]
KINDS = ['normal', 'near_eps', 'carried']


def test_bias_terms_are_formed_in_double_and_rounded_once():
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    for step in STEPS:
        bc1, bc2s = R.bias_terms(0.9, 0.999, step)
        assert bc1.dtype == np.float32 and bc2s.dtype == np.float32
        assert float(bc1) == float(np.float32(1.0 - b1 ** step)) and float(bc2s) == float(np.float32((1.0 - b2 ** step) ** 0.5))
    # formed in fp32 instead, bc1 of step 1 would be 1 - fp32(0.9) either way, but bc2_sqrt differs: the double route is pinned
    assert float(R.bias_terms(0.9, 0.999, 10)[1]) != float(np.sqrt(np.float32(1) - np.float32(0.999) ** np.float32(10)))


@pytest.mark.parametrize('hyper', HYPERS)
@pytest.mark.parametrize('kind', KINDS)
def test_fp32_restatement_within_derived_bound_of_float64(kind, hyper):
    """step32 against step64 from the same fp32 state and the fp32-rounded hyper-parameters: the bound is adam_ref.step_bound's
    (2u*A on m, 3u relative on v, u|p| + 9.5u|update| + m's share on p), derived there."""
    for step in STEPS:
        p, g, m, v = R.operands(kind, 1000, 7 * step + len(kind))
        h32 = [float(x) for x in R.hyper32(hyper.get('lr', 1e-3), hyper.get('b1', 0.9), hyper.get('b2', 0.999), hyper.get('eps', 1e-8))]
        got = R.step32(p, g, m, v, step, **hyper)
        ref = R.step64(p, g, m, v, step, *h32)
        bound = R.step_bound(p, g, m, v, step, **hyper)
        for name, a, b, bd in zip('pmv', got, ref, bound):
            err = np.abs(a.astype(np.float64) - b)
            assert (err <= bd).all(), (name, kind, step, float((err / np.maximum(bd, 1e-300)).max()))


@pytest.mark.parametrize('hyper', HYPERS)
def test_float64_reference_equals_torch_adam(hyper):
    r = np.random.RandomState(3)
    n, steps = 257, 6
    p0 = r.randn(n) * 0.05
    grads = [r.randn(n) * 0.01 for _ in range(steps)]
    lr, b1, b2, eps = hyper.get('lr', 1e-3), hyper.get('b1', 0.9), hyper.get('b2', 0.999), hyper.get('eps', 1e-8)
    q = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for t, g in enumerate(grads, 1):
        q.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, m, v = R.step64(p, g, m, v, t, lr, b1, b2, eps)
        # same formula in float64; the association of the operations may differ between torch versions: a few float64 roundings
        # of the accumulated update
        tol = 16 * 2.0 ** -53 * (np.abs(p) + np.abs(p - p0))
        assert (np.abs(q.detach().numpy() - p) <= tol).all(), t
        st = opt.state[q]
        # m is a signed sum whose terms are bounded by max|g|: a few float64 roundings (2^-53 each) of that, not of m itself
        np.testing.assert_allclose(st['exp_avg'].numpy(), m, rtol=0, atol=16 * 2.0 ** -53 * max(np.abs(x).max() for x in grads))
        np.testing.assert_allclose(st['exp_avg_sq'].numpy(), v, rtol=1e-14, atol=0)


def _ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def _applies(variant, p, g, m, v, step, hyper):
    """A variant applies to a case when, with the fp32 roundings taken out (the same expressions in float64), it moves some
    element of p, m or v by more than two fp32 ulps of that element: then no rounding can bring the two back together. It does
    not apply where it computes the same numbers: both bias corrections are exactly 1 at step 100000, and with b1 = 0.8,
    b2 = 0.99 they are 1 to a part in 1e5 already at step 1000, which gradients near eps do not show."""
    with np.errstate(all='ignore'):
        good = R.step32(p, g, m, v, step, ftype=np.float64, **hyper)
        bad = R.step32(p, g, m, v, step, variant=variant, ftype=np.float64, **hyper)
        return any(bool((~(np.abs(a - b) <= 2 * _ulp32(a))).any()) for a, b in zip(good, bad))


@pytest.mark.parametrize('variant', R.VARIANTS)
def test_every_wrong_variant_changes_the_bits_of_every_case(variant):
    seen, skipped = 0, []
    for hi, hyper in enumerate(HYPERS):
        for kind in KINDS:
            for step in STEPS:
                p, g, m, v = R.operands(kind, 257, 11 * step + len(kind))
                if not _applies(variant, p, g, m, v, step, hyper):
                    skipped.append((hi, kind, step))
                    continue
                good = R.step32(p, g, m, v, step, **hyper)
                bad = R.step32(p, g, m, v, step, variant=variant, **hyper)
                same = np.ones(257, dtype=bool)
                for a, b in zip(good, bad):
                    same &= R.bits(a) == R.bits(b)
                assert not same.all(), (variant, kind, step, hyper)
                seen += 1
    # only the bias-term variants ever fail to apply, and only at step >= 1000; with the default betas only at step 100000
    bias = variant in ('bc_swapped', 'step_plus_1', 'step_minus_1', 'eps_times_sqrt_bc2')
    assert all(bias and step >= 1000 and (step == 100000 or hi == 1) for hi, _, step in skipped), (variant, skipped)
    assert seen >= len(HYPERS) * len(KINDS) * (len(STEPS) - 2)


def test_variants_that_cannot_show_at_step_100000_are_exactly_the_bias_ones():
    p, g, m, v = R.operands('normal', 64, 5)
    good = R.step32(p, g, m, v, 100000)
    for variant in R.VARIANTS:
        bad = R.step32(p, g, m, v, 100000, variant=variant)
        equal = all((R.bits(a) == R.bits(b)).all() for a, b in zip(good, bad))
        assert equal == (not _applies(variant, p, g, m, v, 100000, {})), variant


def test_zero_gradient_leaves_p_unchanged_bit_for_bit_signed_zeros_included():
    p, g, m, v = R.operands('zero', 257, 1)
    assert (R.bits(p) == R.bits(np.float32(-0.0))).any() and (R.bits(p) == 0).any()
    for step in STEPS:
        pn, mn, vn = R.step32(p, g, m, v, step)
        assert (R.bits(pn) == R.bits(p)).all() and (R.bits(mn) == 0).all() and (R.bits(vn) == 0).all()
