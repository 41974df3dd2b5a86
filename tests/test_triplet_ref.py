"""The triplet-loss reference of tests/triplet_ref.py checked on the CPU: against the oracle's triplet_loss and its float64
autograd, slabs adding up to the full form over any partition, the saturation premise of the exact cases proved in fp32, and
every deliberately wrong variant moving the expected values of every case it applies to by more than the GPU tests allow."""
import numpy as np
import pytest
import torch

from oracle import cvig_fov_oracle as O

from . import triplet_ref as T

ALPHAS = [10., 3., 0.5]
SLABS = [(2, 1, 0), (2, 1, 1), (257, 1, 256), (300, 44, 256), (513, 257, 256), (70, 35, 35)]
PARTITION = (256, 1, 200, 56)          # of 513


def _random_cases():
    for B in (2, 3, 64, 257):
        for alpha in ALPHAS:
            yield 'chord B=%d a=%g' % (B, alpha), T.random_case(B, 10 * B + int(alpha)), alpha
    for alpha in ALPHAS:
        yield 'wide B=64 a=%g' % alpha, T.random_case(64, 5, wide_alpha=alpha), alpha


def test_reference_equals_oracle_loss_and_float64_autograd():
    for name, D, alpha in _random_cases():
        for gloss in (1., -2.5, 0.):
            ref = T.full(D, alpha, gloss)
            Dt = torch.tensor(D, dtype=torch.float64, requires_grad=True)
            loss = O.triplet_loss(Dt, alpha)
            assert torch.isfinite(loss).item(), name
            (loss * gloss).backward()
            assert abs(ref['loss'] - loss.item()) <= 1e-13 * abs(loss.item()), name
            # float64 roundings of the oracle's naive log(1 + exp): relative 2^-52 exp(|x|) per term at worst when 1 + e swallows e,
            # so the gradient is compared against the size of the entries, not entry by entry
            scale = np.abs(ref['grad']).max()
            assert np.abs(Dt.grad.numpy() - ref['grad']).max() <= 1e-12 * scale + 1e-300, name


def test_sigmoid_form_stays_finite_where_autograd_gives_nan():
    """the one documented deviation: an overflowing softplus makes the loss +inf and autograd's gradient NaN (inf * 0); the
    sigmoid form the kernels implement is finite there"""
    D, _ = T.exact_case(5, 10.)
    Dt = torch.tensor(D, dtype=torch.float32, requires_grad=True)
    loss = O.triplet_loss(Dt, 10.)
    loss.backward()
    assert torch.isinf(loss).item() and torch.isnan(Dt.grad).any().item()
    assert np.isfinite(T.full(D, 10.)['grad']).all()


@pytest.mark.parametrize('alpha', ALPHAS)
def test_exact_cases_saturate_in_fp32(alpha):
    """the premise of the bit-exact GPU cases, in fp32 numpy: every alpha * (d_mm - d_ij) is 0 or at least 95.9 in magnitude,
    1 / (1 + exp(-x)) is then exactly 0.5, 1 or 0, the sigmoid sums are the counts exact_sig_sums takes from the levels alone,
    and the fp32 formula of the loss gives +inf"""
    f = np.float32
    for B in (2, 3, 64, 257, 513):
        D, L = T.exact_case(B, alpha)
        assert D.dtype == f and set(np.unique(L)) <= {0, 1, 2}
        dg = np.diagonal(D)
        sums, overflow = [], False
        for dm in (dg[:, None], dg[None, :]):
            x = f(alpha) * (dm - D)
            assert x.dtype == f and ((x == 0) | (np.abs(x) >= 95.9)).all()
            with np.errstate(over='ignore'):
                s = f(1) / (f(1) + np.exp(-x))
                sp = np.log(f(1) + np.exp(x))
            assert s.dtype == f and np.isin(s, [0., 0.5, 1.]).all()
            assert ((s == 0.5) == (x == 0)).all() and ((s == 1) == (x > 0)).all()
            assert (np.isinf(sp) == (x > 0)).all() and (sp[x <= 0] <= f(0.6931472)).all()
            sums.append(s)
            overflow = overflow or bool(np.isinf(sp).any())
        assert overflow                  # so the loss of every exact case is +inf
        rowsig, colsig, both = T.exact_sig_sums(L)
        assert (sums[0].astype(np.float64).sum(1) == rowsig).all() and (sums[1].astype(np.float64).sum(0) == colsig).all()
        assert (both == sums[0].astype(np.float64) + sums[1]).all()
        # multiples of 0.5 below 2^24: exact in fp32 whatever the order of summation
        assert (rowsig * 2 == np.round(rowsig * 2)).all() and rowsig.max() < 2 ** 23
        # and the float64 reference agrees with the counts to its own rounding (e^-96 is 2e-42)
        ref = T.full(D, alpha)
        assert np.abs(ref['rowsig'] - rowsig).max() <= 1e-38 * B and np.abs(ref['colsig'] - colsig).max() <= 1e-38 * B


def test_exact_pattern_has_the_properties_the_cases_rely_on():
    for B in (64, 257, 513):
        L = T.exact_levels(B)
        rowsig, colsig, _ = T.exact_sig_sums(L)
        assert len(set(np.diagonal(L))) == 2
        assert (rowsig != colsig).mean() >= 0.99                      # a row's sum is not its column's
        assert len(set(rowsig)) >= 0.6 * B and len(set(colsig)) >= 0.6 * B     # and few rows / columns share one
        assert not (L == L.T).all()
        if B > 256:     # every level on both sides of index 255 (and 511) in the long rows and columns: a dropped tail shows
            for lo in ([256] if B < 513 else [256, 512]):
                assert (L[:, lo:] == 0).any() and (L[lo:, :] == 0).any() and (L[:, lo:] == 1).any() and (L[lo:, :] == 1).any()
                r_head = T.exact_sig_sums(L, 0, lo)[0]
                assert (r_head != rowsig).mean() >= (0.9 if B - lo > 8 else 0.25)      # B = 257: one column past 255


def test_slabs_of_any_partition_add_up_to_the_full_form():
    for B, widths in ((513, PARTITION), (70, (35, 35)), (7, (1, 1, 1, 1, 1, 1, 1)), (64, (64,))):
        for exact in (False, True):
            D = T.exact_case(B, 3.)[0] if exact else T.random_case(B, B)
            ref = T.full(D, 3., -2.5)
            partial, rowsig, col0 = 0., np.zeros(B), 0
            grads, colsigs = [], []
            for w in widths:
                s = T.slab(D, col0, w, 3., -2.5)
                partial, rowsig, col0 = partial + s['partial'], rowsig + s['rowsig'], col0 + w
                grads.append(s['grad'])
                colsigs.append(s['colsig'])
            assert col0 == B
            if not exact:
                assert abs(partial / ref['norm'] - ref['loss']) <= 1e-13 * ref['loss']
            assert np.abs(rowsig - ref['rowsig']).max() <= 1e-12 * B
            assert np.abs(np.concatenate(colsigs) - ref['colsig']).max() <= 1e-12 * B
            assert np.abs(np.concatenate(grads, axis=1) - ref['grad']).max() <= 1e-13 * np.abs(ref['grad']).max()


def test_last_step_f32_rounds_each_operation_once():
    g = np.array([-1.5, 0., 300.5, -0.5], dtype=np.float64)
    out = T.last_step_f32(g, -2.5, 3., 513)
    assert out.dtype == np.float32
    fac = np.float32(np.float32(np.float32(-2.5) * np.float32(3.)) / np.float32(2 * 513 * 512))
    assert (out.view(np.int32) == (g.astype(np.float32) * fac).view(np.int32)).all()
    z = T.last_step_f32(g, 0., 3., 513)          # grad_loss = 0: signed zeros, as the kernel's multiply gives them
    assert (z == 0).all()
    assert np.signbit(T.last_step_f32(g, 0., 3., 513)).tolist() == np.signbit(g.astype(np.float32) * np.float32(0.)).tolist()


# which quantities a variant must move, and the cases it applies to (it computes the same numbers elsewhere)
FULL_MOVES = {
    'rows_cols_exchanged': (('rowsig', 'colsig', 'grad'), lambda B: True),
    'diag_left_out': (('loss', 'rowsig', 'colsig', 'grad'), lambda B: True),
    'norm_2B2': (('loss', 'grad'), lambda B: True),
    'norm_BBm1': (('loss', 'grad'), lambda B: True),
    'alpha_missing': (('grad',), lambda B: True),
    'diag_term_sign': (('grad',), lambda B: True),
    'dropped_past_256': (('loss', 'rowsig', 'colsig', 'grad'), lambda B: B > 256),
}
SLAB_MOVES = {
    'rows_cols_exchanged': (('rowsig', 'colsig'), lambda Bo, Bs, c0: True),
    'diag_left_out': (('partial', 'rowsig', 'colsig', 'grad'), lambda Bo, Bs, c0: True),
    'norm_2B2': (('grad',), lambda Bo, Bs, c0: True),
    'norm_BBm1': (('grad',), lambda Bo, Bs, c0: True),
    'col0_ignored_in_diag': (('partial', 'colsig', 'grad'), lambda Bo, Bs, c0: c0 > 0),
    'col0_ignored_in_eq': (('grad',), lambda Bo, Bs, c0: c0 > 0),
    'rowsig_one_slab': (('grad',), lambda Bo, Bs, c0: Bs < Bo),
    'alpha_missing': (('grad',), lambda Bo, Bs, c0: True),
    'diag_term_sign': (('grad',), lambda Bo, Bs, c0: True),
    'dropped_past_256': (('partial', 'colsig'), lambda Bo, Bs, c0: Bo > 256),
}


def _moved(good, bad, bound, exact):
    good, bad = np.asarray(good, dtype=np.float64), np.asarray(bad, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        if exact:           # the GPU test is an equality there (loss and softplus sums are +inf on both sides: not compared)
            return bool((good != bad).any())
        return bool((np.abs(good - bad) > 4 * np.asarray(bound)).any())


@pytest.mark.parametrize('variant', T.VARIANTS)
def test_every_wrong_variant_moves_every_case_it_applies_to(variant):
    gloss, seen = -2.5, 0
    if variant in FULL_MOVES:
        names, applies = FULL_MOVES[variant]
        for B in (2, 3, 64, 255, 256, 257, 513):
            if not applies(B):
                continue
            for alpha in ALPHAS:
                for exact in (False, True):
                    D = T.exact_case(B, alpha)[0] if exact else T.random_case(B, 100 + B)
                    good, bad = T.full(D, alpha, gloss), T.full(D, alpha, gloss, variant=variant)
                    bounds = T.full_bounds(good)
                    for q in names:
                        if exact and q == 'loss':
                            continue
                        assert _moved(good[q], bad[q], bounds[q], exact), (variant, q, B, alpha, exact)
                    seen += 1
    if variant in SLAB_MOVES:
        names, applies = SLAB_MOVES[variant]
        slabs = SLABS + [(513, w, sum(PARTITION[:k])) for k, w in enumerate(PARTITION)]
        for Bo, Bs, col0 in slabs:
            if not applies(Bo, Bs, col0):
                continue
            for alpha in ALPHAS:
                for exact in (False, True):
                    D = T.exact_case(Bo, alpha)[0] if exact else T.random_case(Bo, Bo + 2)
                    good, bad = T.slab(D, col0, Bs, alpha, gloss), T.slab(D, col0, Bs, alpha, gloss, variant=variant)
                    rs = T.full(D, alpha)['rowsig']
                    bounds = T.slab_bounds(good, Bo, Bs, rs, T.U * rs)
                    for q in names:
                        if exact and q == 'partial':
                            continue
                        assert _moved(good[q], bad[q], bounds[q], exact), (variant, q, (Bo, Bs, col0), alpha, exact)
                    seen += 1
    assert seen > 0
