"""Plain torch restatement of the batch-hard form of cvig_baseline's loss on column slabs (witw_amd/csrc/baseline_loss_hard.hip and the
mining entries of csrc/loss_hard.hip), written from the formulas in include/witw_hip.h, in the dtype of its arguments: float64 gives
the expectations of tests/test_baseline_hard_gpu.py, and CpuKernels is the op set cvig_baseline.sharded_batch_hard_loss takes
through `_kernels=` where no GPU is (tests/test_baseline_hard.py).

    T [B, b]  T[g][c] = |x_g - y_c|^2, column c = global column col0 + c;  Tm = T with the global diagonal at +inf
    rv, ri [B] = min / argmin of the rows of Tm, cv, ci [b] = of its columns (torch.min: a NaN is the minimum at the first NaN's
    index, else ties go to the lowest index); int64 global indices
    l(x) = log(1 + exp(alpha x)) or max(x + margin, 0);  l' its derivative, [x + margin > 0] for the hard margin
    loss = (sum_i l(d_i - rv_i) + sum_j l(d_j - cv_j)) / 2B
"""
import torch

from tests.baseline_slab_ref import term, term_d

INF = float('inf')


def sqdist(x, y, rows=16):
    """T [B, b] from the differences themselves, `rows` rows of x at a time (the [rows, b, n] differences are the memory)"""
    return torch.cat([((x[i:i + rows, None, :] - y[None, :, :]) ** 2).sum(2) for i in range(0, x.shape[0], rows)], 0)


def _masked(T, col0):
    B, b = T.shape
    on = torch.arange(B)[:, None] == (col0 + torch.arange(b))[None, :]
    return T.masked_fill(on, INF)


def slab_mine(T, col0):
    """-> (rv [B], ri [B]: over this slab's columns only, global column indices; the masked diagonal takes part as +inf at its own
    index, so a row whose only column here is its own diagonal has (+inf, its own index); cv [b], ci [b]: complete)"""
    Tm = _masked(T, col0)
    rv, ri = Tm.min(1)
    cv, ci = Tm.min(0)
    return rv, ri + col0, cv, ci


def merge_rows(rv_parts, ri_parts):
    """[w, B] per-slab row minima, slab order -> global (rv [B], ri [B]); parts with index -1 do not take part, an earlier slab wins
    a tie (and a NaN is the minimum, the first one's)"""
    v = rv_parts.masked_fill(ri_parts < 0, INF)
    rv, part = v.min(0)
    return rv, ri_parts.gather(0, part[None])[0]


def mine(T):
    """the whole matrix: (rv, ri, cv, ci), each [B]"""
    return slab_mine(T, 0)


def slab_loss(T, rv, cv, col0, soft_margin=False, alpha=10.0, margin=1.0):
    """un-normalised partial [1]: row terms of the anchors col0 .. col0+b-1 (rv global) + column terms of the slab's columns"""
    b = T.shape[1]
    c = torch.arange(b)
    d = T[col0 + c, c]
    return (term(d - rv[col0:col0 + b], soft_margin, alpha, margin) + term(d - cv, soft_margin, alpha, margin)).sum().reshape(1)


def pairs(diag, rv, ri, cv, ci, grad_loss, col0, soft_margin=False, alpha=10.0, margin=1.0):
    """-> (pair_g int32 [2b + B] global row, pair_c int32 local column, pair_w): the diagonal of the slab's columns, its column
    pairs, the row pairs whose mined column lies in the slab; (-1, -1, 0) elsewhere"""
    B, b = diag.numel(), cv.numel()
    sc = grad_loss.reshape(()) / (2.0 * B)
    wr = sc * term_d(diag - rv, soft_margin, alpha, margin)
    wc = sc * term_d(diag[col0:col0 + b] - cv, soft_margin, alpha, margin)
    c = torch.arange(b)
    ok_c = ci >= 0
    ok_r = (ri >= col0) & (ri < col0 + b)
    neg = torch.full((), -1, dtype=torch.int64)
    pg = torch.cat([col0 + c, torch.where(ok_c, ci, neg), torch.where(ok_r, torch.arange(B), neg)])
    pc = torch.cat([c, torch.where(ok_c, c, neg), torch.where(ok_r, ri - col0, neg)])
    zero = torch.zeros((), dtype=diag.dtype)
    pw = torch.cat([wr[col0:col0 + b] + wc, torch.where(ok_c, -wc, zero), torch.where(ok_r, -wr, zero)])
    return pg.to(torch.int32), pc.to(torch.int32), pw


def dense_grad(B, b, pg, pc, pw):
    """the pair list as the dense dL/dT [B, b]: duplicates add, entries out of range are skipped"""
    G = torch.zeros((B, b), dtype=pw.dtype)
    ok = (pg >= 0) & (pg < B) & (pc >= 0) & (pc < b)
    G.index_put_((pg[ok].long(), pc[ok].long()), pw[ok], accumulate=True)
    return G


def sqdist_pairs_bwd(x, y, pg, pc, pw, need_dx=True, need_dy=True):
    """a pair (g, c, w) adds 2w (x_g - y_c) to dx[g] and 2w (y_c - x_g) to dy[c]; rows without a pair are zero"""
    ok = (pg >= 0) & (pg < x.shape[0]) & (pc >= 0) & (pc < y.shape[0])
    g, c, w = pg[ok].long(), pc[ok].long(), pw[ok]
    t = 2.0 * w[:, None] * (x[g] - y[c])
    dx = torch.zeros_like(x).index_add_(0, g, t) if need_dx else None
    dy = torch.zeros_like(y).index_add_(0, c, -t) if need_dy else None
    return dx, dy


def loss_and_grads(x, y, grad_loss=1.0, soft_margin=False, alpha=10.0, margin=1.0):
    """the whole definition on one slab: x [B, n] (rows of T), y [B, n] (columns) -> (loss, dx, dy, (rv, ri, cv, ci), T)"""
    B = x.shape[0]
    T = sqdist(x, y)
    rv, ri, cv, ci = mine(T)
    loss = slab_loss(T, rv, cv, 0, soft_margin, alpha, margin) / (2.0 * B)
    pg, pc, pw = pairs(torch.diagonal(T), rv, ri, cv, ci, torch.as_tensor(grad_loss, dtype=x.dtype), 0, soft_margin, alpha, margin)
    dx, dy = sqdist_pairs_bwd(x, y, pg, pc, pw)
    return loss.reshape(()), dx, dy, (rv, ri, cv, ci), T


class CpuKernels(object):
    """the six calls of cvig_baseline._hard_kernels() on CPU tensors"""
    pairwise_sqdist = staticmethod(sqdist)
    batch_hard_slab_mine = staticmethod(slab_mine)
    batch_hard_merge_rows = staticmethod(merge_rows)
    hard_slab_loss = staticmethod(slab_loss)
    hard_pairs = staticmethod(pairs)
    sqdist_pairs_bwd = staticmethod(sqdist_pairs_bwd)
