"""The eight soft-margin triplet loss kernels of csrc/loss.hip (full form and column slabs) against tests/triplet_ref.py.

Exact cases (D = levels * 96 / alpha): every sigmoid is exactly 0, 0.5 or 1 in fp32, so ws[2B:4B], rowsig, colsig and every
gradient entry must match bit for bit. Their forward loss overflows by design: the kernel keeps the reference's naive
log(1 + exp), which gives +inf there, and autograd would give NaN gradients (inf * 0); the kernels' sigmoid form stays finite.
That is the one documented deviation from autograd, pinned here.
Random cases: every output against float64 within the rounding bound derived in tests/triplet_ref.py."""
import numpy as np
import pytest
import torch

from . import triplet_ref as T

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ALPHAS = [10., 3., 0.5]
GLOSS = [1., -2.5, 0.]
SIZES = [2, 3, 64, 255, 256, 257, 513]
SLABS = [(2, 1, 0), (2, 1, 1), (257, 1, 256), (300, 44, 256), (513, 257, 256), (70, 35, 35)]
PARTITION = (256, 1, 200, 56)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _gl(g):
    return torch.tensor([g], dtype=torch.float32, device=DEV)


def _full(D, alpha, gloss):
    from witw_amd import ops
    Dd = _dev(D)
    loss, ws = ops.triplet_loss_fwd(Dd, alpha)
    gd = ops.triplet_loss_bwd(Dd, ws, _gl(gloss), alpha)
    torch.cuda.synchronize()
    B = D.shape[0]
    w = ws.cpu().numpy()
    return dict(loss=float(loss.item()), row_sp=w[0:B], col_sp=w[B:2 * B], rowsig=w[2 * B:3 * B], colsig=w[3 * B:4 * B], grad=gd.cpu().numpy())


def _slab(D, col0, Bs, alpha, gloss, rowsig_full):
    from witw_amd import ops
    S, dg = _dev(D[:, col0:col0 + Bs]), _dev(np.diagonal(D))
    part = ops.triplet_loss_slab_fwd(S, dg, col0, alpha)
    rowsig, colsig = ops.triplet_loss_slab_sig(S, dg, col0, alpha)
    gd = ops.triplet_loss_slab_bwd(S, dg, _dev(rowsig_full), colsig, _gl(gloss), col0, alpha)
    torch.cuda.synchronize()
    return dict(partial=float(part.item()), rowsig=rowsig.cpu().numpy(), colsig=colsig.cpu().numpy(), grad=gd.cpu().numpy())


def _within(got, ref, bound, what):
    got, ref, bound = (np.asarray(x, dtype=np.float64) for x in (got, ref, bound))
    assert (np.isnan(bound) == np.isnan(ref)).all(), what
    assert (np.isnan(got) == np.isnan(ref)).all(), (what, 'NaN places differ', np.argwhere(np.isnan(got) != np.isnan(ref))[:4].tolist())
    ok = ~np.isnan(ref)
    err = np.abs(got - ref)[ok]
    print('%s: worst error / bound %.3f' % (what, float((err / np.maximum(bound[ok], 1e-300)).max()) if err.size else 0.))
    assert (err <= bound[ok]).all(), (what, float((err / np.maximum(bound[ok], 1e-300)).max()))


# ----------------------------------------------------------------------------- the measured constants
def test_term_error_of_device_softplus_and_sigmoid():
    """One term per row through the slab kernels with one column: rowsig[i] = sigmoid(x_i), and, with the column's own diagonal
    entry at -1e30 (its softplus is log(1 + 0) = 0 exactly), part[i] = softplus(x_i). 2^17 arguments over [-85, 85] (where
    sigmoid is still a normal number) plus a dense stretch around 0. The worst errors in the units of triplet_ref's K_SP / K_SG
    are printed; the constants there are twice the figures measured when the test was written (K_SP_MEASURED, K_SG_MEASURED),
    and the run must stay inside them."""
    from witw_amd import _lib
    n = 1 << 17
    r = np.random.RandomState(0)
    x = np.concatenate([r.uniform(-85, 85, n - 4096), r.uniform(-1, 1, 4096)]).astype(np.float32)
    x[0] = 0
    diag = x.copy()                 # alpha = 1, D[i,0] = 0: x_i = 1 * (diag[i] - 0), both roundings exact
    D = np.zeros((n, 1), dtype=np.float32)
    from witw_amd import ops
    rowsig, _ = ops.triplet_loss_slab_sig(_dev(D), _dev(diag), 0, 1.)
    sg = rowsig.cpu().numpy().astype(np.float64)
    # softplus: column 0's own diagonal entry is diag[0]; put row 0 far down so that term is log(1 + 0) for every row
    diag2 = diag.copy()
    diag2[0] = np.float32(-1e30)
    lib = _lib.load()
    Dd, dg, part, out = _dev(D), _dev(diag2), torch.empty(n, device=DEV), torch.empty(1, device=DEV)
    _lib.check(lib.witw_triplet_loss_slab_fwd(Dd.data_ptr(), dg.data_ptr(), n, 1, 0, 1.0, out.data_ptr(), part.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), 'witw_triplet_loss_slab_fwd')
    torch.cuda.synchronize()
    sp = part.cpu().numpy().astype(np.float64)[1:]
    x64 = x.astype(np.float64)
    k_sg = np.abs(sg - T.sigmoid(x64)) / (T.U * T.sigmoid(x64))
    k_sp = np.abs(sp - T.softplus(x64[1:])) / (T.U * (1 + T.softplus(x64[1:])))
    print('measured K_SG %.3f at x=%g, K_SP %.3f at x=%g' % (k_sg.max(), x[k_sg.argmax()], k_sp.max(), x[1:][k_sp.argmax()]))
    assert k_sg.max() <= T.K_SG and k_sp.max() <= T.K_SP


# ----------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize('alpha', ALPHAS)
def test_exact_cases_full_form_bit_for_bit(alpha):
    """Sigmoid sums and every gradient entry through an integer view. The loss is +inf, as the fp32 formula of the reference
    gives (the kept naive log(1 + exp) overflows), and the gradient is finite where autograd's would be NaN."""
    for B in SIZES:
        D, L = T.exact_case(B, alpha)
        rowsig, colsig, both = T.exact_sig_sums(L)
        # off the diagonal the kernel leaves -s1 - s2 alone: -0.0 where both sigmoids are 0, and the sign is part of the bits
        g = np.where(np.eye(B) > 0, -both + (colsig[None, :] + rowsig[:, None]), -both)
        for gloss in GLOSS:
            got = _full(D, alpha, gloss)
            assert (_bits(got['rowsig']) == _bits(rowsig)).all() and (_bits(got['colsig']) == _bits(colsig)).all(), (B, alpha)
            want = T.last_step_f32(g, gloss, alpha, B)
            bad = np.argwhere(_bits(got['grad']) != _bits(want))
            assert bad.size == 0, (B, alpha, gloss, len(bad), bad[:4].tolist())
            assert np.isfinite(got['grad']).all()
            assert got['loss'] == float('inf')
            with np.errstate(over='ignore'):
                f = np.float32
                x = f(alpha) * (np.diagonal(D)[:, None] - D)
                assert np.isinf(np.log(f(1) + np.exp(x)).sum() + np.log(f(1) + np.exp(f(alpha) * (np.diagonal(D)[None, :] - D))).sum())


@pytest.mark.parametrize('alpha', ALPHAS)
def test_exact_cases_slabs_bit_for_bit(alpha):
    slabs = SLABS + [(513, w, sum(PARTITION[:k])) for k, w in enumerate(PARTITION)]
    for Bo, Bs, col0 in slabs:
        D, L = T.exact_case(Bo, alpha)
        rowsig_full = T.exact_sig_sums(L)[0]
        rowsig, colsig, both = T.exact_sig_sums(L, col0, Bs)
        eq = np.arange(Bo)[:, None] == (np.arange(Bs)[None, :] + col0)
        g = np.where(eq, -both + (colsig[None, :] + rowsig_full[:, None]), -both)            # -0.0 kept off the diagonal
        for gloss in GLOSS:
            got = _slab(D, col0, Bs, alpha, gloss, rowsig_full)
            assert (_bits(got['rowsig']) == _bits(rowsig)).all() and (_bits(got['colsig']) == _bits(colsig)).all(), (Bo, Bs, col0)
            bad = np.argwhere(_bits(got['grad']) != _bits(T.last_step_f32(g, gloss, alpha, Bo)))
            assert bad.size == 0, (Bo, Bs, col0, alpha, gloss, len(bad), bad[:4].tolist())
            assert np.isfinite(got['grad']).all()
    # the partition of 513: partial rowsig summed over the slabs (exact, multiples of 0.5) is the full form's
    D, L = T.exact_case(513, alpha)
    full = _full(D, alpha, -2.5)
    acc, grads, col0 = np.zeros(513, dtype=np.float32), [], 0
    for w in PARTITION:
        s = _slab(D, col0, w, alpha, -2.5, T.exact_sig_sums(L)[0])
        acc, col0 = acc + s['rowsig'], col0 + w
        grads.append(s['grad'])
    assert (_bits(acc) == _bits(full['rowsig'])).all()
    assert (_bits(np.concatenate(grads, axis=1)) == _bits(full['grad'])).all()


# ----------------------------------------------------------------------------- random cases
def _random(B, alpha, wide):
    return T.random_case(B, 31 * B + int(alpha), wide_alpha=alpha if wide else None)


@pytest.mark.parametrize('wide', [False, True], ids=['chord', 'wide'])
@pytest.mark.parametrize('alpha', ALPHAS)
def test_random_cases_full_form_within_derived_bound(alpha, wide):
    for B in SIZES:
        D = _random(B, alpha, wide)
        for gloss in (GLOSS if B in (3, 257) else GLOSS[1:2]):       # grad_loss only scales the last step
            ref = T.full(D, alpha, gloss)
            bounds = T.full_bounds(ref)
            got = _full(D, alpha, gloss)
            for q in ('loss', 'row_sp', 'col_sp', 'rowsig', 'colsig', 'grad'):
                _within(got[q], ref[q], bounds[q], '%s B=%d a=%g g=%g' % (q, B, alpha, gloss))
            if wide:
                x = np.abs(ref['x_row'])
                assert np.isfinite(got['loss']) and (x.max() > 60 if B >= 64 else True) and x.max() < 80.5


@pytest.mark.parametrize('wide', [False, True], ids=['chord', 'wide'])
@pytest.mark.parametrize('alpha', ALPHAS)
def test_random_cases_slabs_within_derived_bound(alpha, wide):
    gloss = -2.5
    for Bo, Bs, col0 in SLABS:
        D = _random(Bo, alpha, wide)
        true_rowsig = T.full(D, alpha)['rowsig']
        fed = true_rowsig.astype(np.float32)                     # the summed row sums handed to the backward: one rounding
        ref = T.slab(D, col0, Bs, alpha, gloss)
        bounds = T.slab_bounds(ref, Bo, Bs, true_rowsig, T.U * true_rowsig)
        got = _slab(D, col0, Bs, alpha, gloss, fed)
        for q in ('partial', 'rowsig', 'colsig', 'grad'):
            _within(got[q], ref[q], bounds[q], '%s slab=%s a=%g' % (q, (Bo, Bs, col0), alpha))
    # an unequal partition of 513: summed partials, summed rowsig and stitched gradients reproduce the full form
    D = _random(513, alpha, wide)
    ref = T.full(D, alpha, gloss)
    fb = T.full_bounds(ref)
    parts, col0 = [], 0
    for w in PARTITION:
        r = T.slab(D, col0, w, alpha, gloss)
        parts.append((col0, w, r, T.slab_bounds(r, 513, w, ref['rowsig'], 0 * ref['rowsig'])))
        col0 += w
    dev_sig = [_slab(D, c, w, alpha, gloss, ref['rowsig']) for c, w, _, _ in parts]
    rowsig = np.zeros(513, dtype=np.float32)
    b_rowsig = np.zeros(513)
    partial, b_partial = np.float32(0), 0.
    for (c, w, r, b), s in zip(parts, dev_sig):
        rowsig = rowsig + s['rowsig']                            # fp32 adds, as the all-reduce does: one rounding each
        b_rowsig = b_rowsig + b['rowsig'] + T.U * np.abs(rowsig)
        partial = partial + np.float32(s['partial'])
        b_partial = b_partial + b['partial'] + T.U * abs(float(partial))
    _within(rowsig, ref['rowsig'], T.SECOND_ORDER * b_rowsig, 'partition rowsig a=%g' % alpha)
    _within(float(partial) / ref['norm'], ref['loss'], T.SECOND_ORDER * b_partial / ref['norm'], 'partition loss a=%g' % alpha)
    grads = []
    for c, w, r, b in parts:
        s = _slab(D, c, w, alpha, gloss, rowsig)
        bb = T.slab_bounds(r, 513, w, ref['rowsig'], T.SECOND_ORDER * b_rowsig)
        _within(s['grad'], ref['grad'][:, c:c + w], bb['grad'], 'partition grad col0=%d a=%g' % (c, alpha))
        grads.append(s['grad'])
    assert np.concatenate(grads, axis=1).shape == (513, 513)


# ----------------------------------------------------------------------------- non-finite inputs
@pytest.mark.parametrize('where', [(5, 9), (7, 7)], ids=['off_diagonal', 'diagonal'])
def test_one_nan_reaches_exactly_the_entries_the_reference_says(where):
    B, alpha, gloss = 64, 3., -2.5
    D = _random(B, alpha, False)
    D[where] = np.nan
    ref = T.full(D, alpha, gloss)
    places = np.argwhere(np.isnan(ref['grad']))
    i, j = where
    if i != j:      # (i,j) itself, the diagonal entries through rowsig_i and colsig_j, and no more: the reference decides
        assert sorted(map(tuple, places.tolist())) == sorted({(i, j), (i, i), (j, j)})
    else:           # the whole row and column read d_ii
        assert len(places) == 2 * B - 1
    got = _full(D, alpha, gloss)
    assert np.isnan(got['loss']) and np.isnan(ref['loss'])
    bounds = T.full_bounds(ref)
    for q in ('row_sp', 'col_sp', 'rowsig', 'colsig', 'grad'):
        _within(got[q], ref[q], bounds[q], '%s nan at %s' % (q, where))
    # and the slab holding column j
    col0, Bs = (j // 16) * 16, 16
    r = T.slab(D, col0, Bs, alpha, gloss)
    fed = np.where(np.isnan(ref['rowsig']), np.nan, ref['rowsig']).astype(np.float32)
    s = _slab(D, col0, Bs, alpha, gloss, fed)
    b = T.slab_bounds(r, B, Bs, ref['rowsig'], T.U * np.abs(ref['rowsig']))
    assert np.isnan(s['partial'])
    for q in ('rowsig', 'colsig', 'grad'):
        _within(s[q], r[q], b[q], 'slab %s nan at %s' % (q, where))


# ----------------------------------------------------------------------------- the autograd wrapper and argument checks
def test_autograd_wrapper_scaled_loss_and_noncontiguous_input():
    from witw_amd import cvig_fov
    B, alpha, s = 65, 3., -1.75
    D = _random(B, alpha, False)
    ref = T.full(D, alpha, s)
    bounds = T.full_bounds(ref)
    base = _dev(np.ascontiguousarray(D.T)).requires_grad_(True)
    view = base.t()                                     # a non-contiguous D
    assert not view.is_contiguous()
    loss = cvig_fov.triplet_loss(view * 1.0, alpha)
    (loss * s).backward()
    _within(loss.item(), ref['loss'], bounds['loss'], 'wrapper loss')
    _within(base.grad.t().cpu().numpy(), ref['grad'], bounds['grad'], 'wrapper grad')
    leaf = view.detach().requires_grad_(True)           # the non-contiguous tensor itself as the leaf
    (cvig_fov.triplet_loss(leaf, alpha) * s).backward()
    _within(leaf.grad.cpu().numpy(), ref['grad'], bounds['grad'], 'wrapper grad, non-contiguous leaf')


def test_entries_refuse_bad_arguments():
    from witw_amd import _lib, cvig_fov, ops
    one = torch.zeros((1, 1), device=DEV)
    with pytest.raises(_lib.WitwError):
        ops.triplet_loss_fwd(one, 10.)
    with pytest.raises(_lib.WitwError):
        ops.triplet_loss_bwd(one, torch.zeros(4, device=DEV), _gl(1.), 10.)
    with pytest.raises(_lib.WitwError):
        cvig_fov.triplet_loss(torch.zeros((3, 4), device=DEV))
    S, dg = torch.zeros((8, 3), device=DEV), torch.zeros(8, device=DEV)
    sig = (torch.zeros(8, device=DEV), torch.zeros(3, device=DEV))
    for col0 in (6, -1):                                # col0 + Bs > Bo; col0 < 0
        with pytest.raises(_lib.WitwError):
            ops.triplet_loss_slab_fwd(S, dg, col0, 10.)
        with pytest.raises(_lib.WitwError):
            ops.triplet_loss_slab_sig(S, dg, col0, 10.)
        with pytest.raises(_lib.WitwError):
            ops.triplet_loss_slab_bwd(S, dg, sig[0], sig[1], _gl(1.), col0, 10.)
    with pytest.raises(_lib.WitwError):                 # Bo = 1
        ops.triplet_loss_slab_fwd(torch.zeros((1, 1), device=DEV), torch.zeros(1, device=DEV), 0, 10.)
    torch.cuda.synchronize()
