"""Plain torch restatement of the column-slab form of cvig_baseline's exhaustive loss (witw_amd/csrc/baseline_loss_slab.hip), written
from the formulas in include/witw_hip.h, in the dtype of its arguments: float64 gives the expectations of
tests/test_baseline_sharded_loss_gpu.py, and CpuKernels is the op set cvig_baseline.sharded_exhaustive_loss takes through
`_kernels=` where no GPU is (tests/test_baseline_sharded_loss.py).

    T [B, b]  T[g][c] = |x_g - y_c|^2, column c = global column col0 + c;  diag [B] the global diagonal
    l(x) = log(1 + exp(alpha x)) or max(x + margin, 0);  l' its derivative
"""
import torch


def term(x, soft_margin, alpha, margin):
    return torch.log(1.0 + torch.exp(alpha * x)) if soft_margin else torch.relu(x + margin)


def term_d(x, soft_margin, alpha, margin):
    return alpha * torch.sigmoid(alpha * x) if soft_margin else (x + margin > 0).to(x.dtype)


def _args(T, diag, col0):
    """-> (x of the column anchors, x of the row anchors, mask of the off-diagonal entries), each [B, b]"""
    B, b = T.shape
    off = torch.arange(B)[:, None] != (col0 + torch.arange(b))[None, :]
    return diag[col0:col0 + b][None, :] - T, diag[:, None] - T, off


def slab_partial(T, diag, col0, soft_margin=False, alpha=10.0, margin=1.0):
    xc, xr, off = _args(T, diag, col0)
    return ((term(xc, soft_margin, alpha, margin) + term(xr, soft_margin, alpha, margin)) * off).sum().reshape(1)


def slab_sig(T, diag, col0, soft_margin=False, alpha=10.0, margin=1.0):
    """-> (rowsig [B]: this slab's part, colsig [b])"""
    xc, xr, off = _args(T, diag, col0)
    return (term_d(xr, soft_margin, alpha, margin) * off).sum(1), (term_d(xc, soft_margin, alpha, margin) * off).sum(0)


def slab_grad(T, diag, rowsig, colsig, grad_loss, col0, soft_margin=False, alpha=10.0, margin=1.0):
    """G [B, b] = dL/dT; rowsig = the row sums of ALL slabs"""
    B, b = T.shape
    xc, xr, off = _args(T, diag, col0)
    G = -(term_d(xc, soft_margin, alpha, margin) + term_d(xr, soft_margin, alpha, margin)) * off
    c = torch.arange(b)
    G[col0 + c, c] = rowsig[col0:col0 + b] + colsig
    return G * (grad_loss / (2.0 * B * (B - 1)))


def sqdist_rect_bwd(x, y, G, need_dx=True, need_dy=True):
    """dx[g] = 2 sum_c G[g][c] (x_g - y_c), dy[c] = 2 sum_g G[g][c] (y_c - x_g)"""
    dx = 2.0 * (G.sum(1)[:, None] * x - G @ y) if need_dx else None
    dy = 2.0 * (G.sum(0)[:, None] * y - G.t() @ x) if need_dy else None
    return dx, dy


class CpuKernels(object):
    """the five calls of cvig_baseline._slab_kernels() on CPU tensors"""

    @staticmethod
    def pairwise_sqdist(x, y):
        return ((x[:, None, :] - y[None, :, :]) ** 2).sum(2)

    exhaustive_loss_slab_fwd = staticmethod(slab_partial)
    exhaustive_loss_slab_sig = staticmethod(slab_sig)
    exhaustive_loss_slab_bwd = staticmethod(slab_grad)
    sqdist_rect_bwd = staticmethod(sqdist_rect_bwd)
