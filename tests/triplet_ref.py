"""Float64 restatement of the soft-margin triplet loss kernels (csrc/loss.hip) for tests/test_triplet_ref.py (CPU) and
tests/test_triplet_loss_gpu.py.

Full matrix D [B,B], a = alpha, norm = 2B(B-1), both sums over the whole matrix, diagonal included:
    row_sp[i] = sum_j softplus(a(d_ii - d_ij))   (ws[0:B])      rowsig[i] = sum_j sigmoid(a(d_ii - d_ij))   (ws[2B:3B])
    col_sp[j] = sum_i softplus(a(d_jj - d_ij))   (ws[B:2B])     colsig[j] = sum_i sigmoid(a(d_jj - d_ij))   (ws[3B:4B])
    loss = (sum row_sp + sum col_sp) / norm
    dL/dD_ij = gloss * a / norm * ( -sigmoid(a(d_jj - d_ij)) - sigmoid(a(d_ii - d_ij)) + [i == j] (colsig_j + rowsig_i) )
the sigmoid form the kernels implement. It is autograd's gradient wherever the loss is finite; where softplus overflows (the
naive log(1 + exp) is kept from the reference) autograd gives inf * 0 = NaN and this form stays finite.

Column slab [Bo,Bs] = D[:, col0:col0+Bs] with the global diagonal, c = col0 + j: un-normalised partial, rowsig over the slab's
columns only (the caller sums it over the slabs), colsig complete, slab gradient with [i == c].

VARIANTS: deliberately wrong restatements, each one mistake a kernel could make.
"""
import numpy as np

f32 = np.float32
U = 2.0 ** -24

# Worst error of one device term given its fp32 argument x, in units of u = 2^-24:
#   softplus: |logf(1 + expf(x)) - softplus(x)| <= K_SP * u * (1 + softplus(x))
#   sigmoid:  |1 / (1 + expf(-x)) - sigmoid(x)| <= K_SG * u * sigmoid(x)
# Derivation: e = expf(x) carries E_e ulp (relative 2 E_e u), 1 + e rounds once (relative u of the sum, absolute <= u in the
# logarithm), logf carries E_l ulp of its result (2 E_l u softplus); the error of e enters the logarithm as sigmoid(x) * 2 E_e u.
# Softplus: u (1 + 2 E_e sigmoid + 2 E_l softplus) <= u (1 + softplus) max(1 + 2 E_e, 2 E_l). Sigmoid: the sum and the division
# round once each (2u sigmoid) and e's error enters as sigmoid (1 - sigmoid) 2 E_e u: u sigmoid (2 + 2 E_e).
# The ulp figures of device expf / logf are not stated by any header or document of the ROCm installation, so the two constants
# are MEASURED (tests/test_triplet_loss_gpu.py::test_term_error_of_device_softplus_and_sigmoid measures them again on every run,
# through the slab kernels with one column, over 2^17 arguments in [-85, 85]) and set to twice the worst figure seen:
# K_SP_MEASURED / K_SG_MEASURED below; by the derivation above they correspond to E_e, E_l below one ulp.
K_SP_MEASURED = 2.417    # worst softplus term, at x = 11.10 (MI355X, ROCm's ocml expf / logf)
K_SG_MEASURED = 2.501    # worst sigmoid term, at x = -16.74
K_SP = 2 * K_SP_MEASURED
K_SG = 2 * K_SG_MEASURED
SECOND_ORDER = 1 + 2.0 ** -10        # every product of two roundings (O(u^2 n)) folded into one factor

VARIANTS = ('rows_cols_exchanged', 'diag_left_out', 'norm_2B2', 'norm_BBm1', 'col0_ignored_in_diag', 'col0_ignored_in_eq',
            'rowsig_one_slab', 'alpha_missing', 'diag_term_sign', 'dropped_past_256')


def softplus(x):
    """log(1 + exp(x)) in float64 without overflow (NaN stays NaN)"""
    with np.errstate(all='ignore'):
        return np.where(x > 0, x, 0) + np.log1p(np.exp(-np.abs(x))) + np.where(np.isnan(x), np.nan, 0)


def sigmoid(x):
    with np.errstate(all='ignore'):
        e = np.exp(-np.abs(x))
        return np.where(x >= 0, 1 / (1 + e), e / (1 + e)) + np.where(np.isnan(x), np.nan, 0)


def _keep(n, variant):
    """weights of the summed index: elements at index 256 and above dropped under 'dropped_past_256'"""
    w = np.ones(n)
    if variant == 'dropped_past_256':
        w[256:] = 0
    return w


def _wsum(t, w, axis):
    """sum over `axis` of the terms with weight 1 (a dropped term does not take part, even when it is NaN)"""
    w = w[None, :] if axis == 1 else w[:, None]
    return np.where(w > 0, t, 0).sum(axis=axis)


def _norm(B, variant):
    return {'norm_2B2': 2.0 * B * B, 'norm_BBm1': 1.0 * B * (B - 1)}.get(variant, 2.0 * B * (B - 1))


def full(D, alpha, gloss=1.0, variant=None):
    """-> dict: loss, row_sp, col_sp, rowsig, colsig, grad (float64), and x_row / x_col, the two arguments of every entry"""
    assert variant is None or variant in VARIANTS
    D = np.asarray(D, dtype=np.float64)
    if variant == 'rows_cols_exchanged':
        D = D.T
    B = D.shape[0]
    a = float(f32(alpha))
    dg = np.diagonal(D)
    x_row = a * (dg[:, None] - D)            # a(d_ii - d_ij)
    x_col = a * (dg[None, :] - D)            # a(d_jj - d_ij)
    off = 1 - np.eye(B) if variant == 'diag_left_out' else np.ones((B, B))
    w = _keep(B, variant)
    row_sp = _wsum(np.where(off > 0, softplus(x_row), 0), w, 1)
    col_sp = _wsum(np.where(off > 0, softplus(x_col), 0), w, 0)
    rowsig = _wsum(np.where(off > 0, sigmoid(x_row), 0), w, 1)
    colsig = _wsum(np.where(off > 0, sigmoid(x_col), 0), w, 0)
    norm = _norm(B, variant)
    loss = (_wsum(row_sp[None, :], w, 1)[0] + _wsum(col_sp[None, :], w, 1)[0]) / norm
    g = -sigmoid(x_col) - sigmoid(x_row)
    sign = -1.0 if variant == 'diag_term_sign' else 1.0
    g = g + np.where(np.eye(B) > 0, sign * (colsig[None, :] + rowsig[:, None]), 0)
    factor = float(f32(gloss)) * (1.0 if variant == 'alpha_missing' else a) / norm
    grad = g * factor
    return dict(factor=factor, loss=loss, row_sp=row_sp, col_sp=col_sp, rowsig=rowsig, colsig=colsig, g=g, grad=grad, x_row=x_row, x_col=x_col,
                norm=norm)


def slab(D, col0, Bs, alpha, gloss=1.0, variant=None, rowsig_full=None):
    """the slab quantities of the columns [col0, col0+Bs) of the full matrix D -> dict: partial (un-normalised), rowsig (this
    slab's share), colsig, grad [Bo,Bs]; rowsig_full = the row sums over all slabs (default: computed from D)"""
    assert variant is None or variant in VARIANTS
    D = np.asarray(D, dtype=np.float64)
    Bo = D.shape[0]
    a = float(f32(alpha))
    S = D[:, col0:col0 + Bs]
    dg = np.diagonal(D)
    dcol = dg[0:Bs] if variant == 'col0_ignored_in_diag' else dg[col0:col0 + Bs]
    x_row = a * (dg[:, None] - S)            # a(d_ii - d_ij)
    x_col = a * (dcol[None, :] - S)          # a(d_cc - d_ij)
    if variant == 'rows_cols_exchanged':
        x_row, x_col = x_col, x_row
    eq = (np.arange(Bo)[:, None] == (np.arange(Bs)[None, :] + col0))
    off = ~eq if variant == 'diag_left_out' else np.ones((Bo, Bs), dtype=bool)
    wr, wc = _keep(Bs, variant), _keep(Bo, variant)
    part_rows = _wsum(np.where(off, softplus(x_col) + softplus(x_row), 0), wr, 1)
    partial = _wsum(part_rows[None, :], wc, 1)[0]
    rowsig = _wsum(np.where(off, sigmoid(x_row), 0), wr, 1)
    colsig = _wsum(np.where(off, sigmoid(x_col), 0), wc, 0)
    if rowsig_full is None:
        rowsig_full = full(D, alpha, variant=variant if variant in ('diag_left_out', 'rows_cols_exchanged') else None)['rowsig']
    if variant == 'rowsig_one_slab':
        rowsig_full = rowsig
    if variant == 'col0_ignored_in_eq':
        eq = (np.arange(Bo)[:, None] == np.arange(Bs)[None, :])
    g = -sigmoid(x_col) - sigmoid(x_row)
    sign = -1.0 if variant == 'diag_term_sign' else 1.0
    g = g + np.where(eq, sign * (colsig[None, :] + np.asarray(rowsig_full, dtype=np.float64)[:, None]), 0)
    norm = _norm(Bo, variant)
    factor = float(f32(gloss)) * (1.0 if variant == 'alpha_missing' else a) / norm
    grad = g * factor
    return dict(factor=factor, partial=partial, part_rows=part_rows, rowsig=rowsig, colsig=colsig, g=g, grad=grad, x_row=x_row, x_col=x_col, eq=eq,
                norm=norm)


def last_step_f32(g, gloss, alpha, B):
    """the gradient's last step as the kernels do it in fp32: g * (gloss * alpha / norm), norm = 2.f * B * (B - 1), each
    operation rounded once (g must be exactly representable, as in the exact cases)"""
    norm = f32(2) * f32(B) * f32(B - 1)
    with np.errstate(all='ignore'):
        return np.asarray(g).astype(f32) * (f32(gloss) * f32(alpha) / norm)


# ----------------------------------------------------------------------------- exact cases
def exact_levels(B):
    """Levels in {0, 1, 2}, [B,B]: a triangular pattern in a scattered order. With q(k) = (11 k + 5) mod B (11 is coprime to
    every size used) entry (i, j) is 0 where q(j) < q(i) and 2 where q(j) > q(i), except that every entry with (i + 2 j) mod 5 = 0
    is 1; the diagonal is 1, and 2 where i mod 3 = 0 (so the diagonal level of column j differs from that of column col0 + j
    at the offsets the slab cases use). Row i so holds about q(i) zeros and column j about B - 1 - q(j): the sums
    differ from row to row and from column to column, rows are no mirror of columns, and zeros, ones and twos lie on both sides
    of index 255 and of 511 in every long row and column."""
    if B == 2:          # four entries: chosen by hand so that every wrong variant shows on both one-column slabs
        return np.array([[2, 2], [1, 1]], dtype=np.int64)
    k = np.arange(B)
    q = (11 * k + 5) % B
    i, j = k[:, None], k[None, :]
    L = np.where(q[None, :] < q[:, None], 0, 2)
    L = np.where((i + 2 * j) % 5 == 0, 1, L)
    L[k, k] = np.where(k % 3 == 0, 2, 1)
    return L.astype(np.int64)


def exact_case(B, alpha):
    """-> (D fp32 [B,B] = levels * fp32(96 / alpha), levels)"""
    L = exact_levels(B)
    unit = f32(96.0 / float(f32(alpha)))
    return (L.astype(f32) * unit).astype(f32), L


def exact_sig_sums(L, col0=0, Bs=None):
    """the sigmoid sums of a saturated case from the levels alone: sigmoid is 1 where the entry's level is below the diagonal
    one, 0.5 where equal, 0 where above -> (rowsig over the columns [col0, col0+Bs), colsig of those columns, s = the two
    sigmoids of every entry of the slab added)"""
    B = L.shape[0]
    Bs = B if Bs is None else Bs
    S = L[:, col0:col0 + Bs]
    dg = np.diagonal(L)

    def sg(dm):
        return np.where(S < dm, 1.0, np.where(S == dm, 0.5, 0.0))
    s_row, s_col = sg(dg[:, None]), sg(dg[None, col0:col0 + Bs])
    return s_row.sum(1), s_col.sum(0), s_row + s_col


# ----------------------------------------------------------------------------- rounding bounds of the random cases
def _trips(n):
    return (n + 255) // 256


def sp_term_bound(x):
    """one softplus term: x = fl(a * fl(dm - d)) carries two roundings (|x| 2u, through the derivative sigmoid(x)), then the
    evaluation error K_SP u (1 + softplus)"""
    ax = np.abs(x)
    return U * (2 * ax * sigmoid(x) + K_SP * (1 + softplus(x)))


def sg_term_bound(x):
    """one sigmoid term: the two roundings of x through the derivative sigmoid (1 - sigmoid), then K_SG u sigmoid; 2^-126 covers
    the terms the device returns as 0 (expf overflowed) or as a flushed subnormal"""
    s = sigmoid(x)
    return U * (2 * np.abs(x) * s * (1 - s) + K_SG * s) + 2.0 ** -126


def sum_bound(term_bounds, terms, n, axis):
    """a block sum of n positive terms: each thread adds its ceil(n/256) strided terms in turn, 6 shuffle levels, then
    (sh0 + sh1) + (sh2 + sh3), one more for the last use: (trips + 6 + 3) u * sum of the terms, plus the terms' own errors"""
    return SECOND_ORDER * (term_bounds.sum(axis=axis) + (_trips(n) + 9) * U * np.abs(terms).sum(axis=axis))


def full_bounds(ref):
    """bounds of every output of the full form for the reference `ref` = full(D, alpha, gloss)"""
    B = ref['rowsig'].shape[0]
    b = dict(
        row_sp=sum_bound(sp_term_bound(ref['x_row']), softplus(ref['x_row']), B, 1),
        col_sp=sum_bound(sp_term_bound(ref['x_col']), softplus(ref['x_col']), B, 0),
        rowsig=sum_bound(sg_term_bound(ref['x_row']), sigmoid(ref['x_row']), B, 1),
        colsig=sum_bound(sg_term_bound(ref['x_col']), sigmoid(ref['x_col']), B, 0))
    # loss: two block sums over the B partials (their own bounds carried), one add and one division
    total = ref['row_sp'].sum() + ref['col_sp'].sum()
    b['loss'] = SECOND_ORDER * (b['row_sp'].sum() + b['col_sp'].sum() + (_trips(B) + 9 + 2) * U * total) / ref['norm']
    b['grad'] = _grad_bound(ref, b['rowsig'][:, None], b['colsig'][None, :], np.eye(B) > 0, ref['rowsig'][:, None], ref['colsig'][None, :])
    return b


def _grad_bound(ref, b_rowsig, b_colsig, eq, rowsig, colsig):
    """g = (-s1 - s2) [+ (colsig + rowsig) on the diagonal]: the terms' own errors, one rounding per add over the magnitudes
    added (1 off the diagonal, 3 on it), then g * ((gloss * a) / norm): three more roundings, relative"""
    s1, s2 = sigmoid(ref['x_col']), sigmoid(ref['x_row'])
    mag = s1 + s2 + np.where(eq, colsig + rowsig, 0)
    err = sg_term_bound(ref['x_col']) + sg_term_bound(ref['x_row']) + np.where(eq, b_rowsig + b_colsig, 0) + np.where(eq, 3, 1) * U * mag
    return SECOND_ORDER * abs(ref['factor']) * (err + 3 * U * mag)


def slab_bounds(ref, Bo, Bs, rowsig_full, b_rowsig_full):
    """bounds of the slab outputs for ref = slab(...); rowsig_full / b_rowsig_full = the summed row sums fed to the backward
    and how far they may be from the true sums"""
    both = softplus(ref['x_col']) + softplus(ref['x_row'])
    # the thread adds two terms per trip: 2 * trips adds
    b_rows = SECOND_ORDER * ((sp_term_bound(ref['x_col']) + sp_term_bound(ref['x_row'])).sum(1) + (2 * _trips(Bs) + 9) * U * both.sum(1))
    b = dict(part_rows=b_rows,
             partial=SECOND_ORDER * (b_rows.sum() + (_trips(Bo) + 9) * U * both.sum()),
             rowsig=sum_bound(sg_term_bound(ref['x_row']), sigmoid(ref['x_row']), Bs, 1),
             colsig=sum_bound(sg_term_bound(ref['x_col']), sigmoid(ref['x_col']), Bo, 0))
    b['grad'] = _grad_bound(ref, np.asarray(b_rowsig_full)[:, None], b['colsig'][None, :], ref['eq'], np.asarray(rowsig_full)[:, None],
                            ref['colsig'][None, :])
    return b


# ----------------------------------------------------------------------------- random cases
def random_case(B, seed, wide_alpha=None):
    """fp32 D: |N(0,1)| clipped to [0, 4), the range of the model's chord distances; wide_alpha: uniform in [0, 80 / alpha), so
    that alpha * delta reaches about +-80 and every exp stays finite"""
    r = np.random.RandomState(seed)
    if wide_alpha is None:
        return np.minimum(np.abs(r.randn(B, B)), np.nextafter(f32(4), f32(0))).astype(f32)
    return (r.rand(B, B) * (80.0 / wide_alpha)).astype(f32)
