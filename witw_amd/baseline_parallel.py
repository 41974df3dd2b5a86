"""Host-side wrappers of csrc/baseline_loss_slab.hip: the exhaustive minibatch triplet loss on the [B, b] column slab one rank holds
of the global batch, and the backward of a rectangular squared-distance matrix. With ops.pairwise_sqdist they are the op set of
cvig_baseline.sharded_exhaustive_loss and live here, not in ops.py; their memory-contract cases are in
tests/test_baseline_sharded_loss_gpu.py. No CPU fallback."""
import torch

from . import _lib
from .ops import _dev_f32, _p, _stream


def _slab(name, T, diag, col0):
    T, diag = _dev_f32(T, 'T'), _dev_f32(diag, 'diag')
    if T.dim() != 2 or diag.dim() != 1 or diag.numel() != T.shape[0]:
        raise _lib.WitwError('%s: need a [B, b] slab and the B diagonal entries, got %s and %s' % (name, tuple(T.shape), tuple(diag.shape)))
    return T, diag, T.shape[0], T.shape[1], int(col0)


def exhaustive_loss_slab_fwd(T, diag, col0, soft_margin=False, alpha=10., margin=1.):
    """Un-normalised loss partial f32 [1] of this rank's slab T [B,b] (witw_exhaustive_loss_slab_fwd): the sum over the ranks,
    divided by 2B(B-1), is the loss."""
    T, diag, B, b, col0 = _slab('exhaustive_loss_slab_fwd', T, diag, col0)
    out = torch.empty((1,), dtype=torch.float32, device=T.device)
    ws = torch.empty((B,), dtype=torch.float32, device=T.device)
    _lib.check(_lib.load().witw_exhaustive_loss_slab_fwd(T.data_ptr(), diag.data_ptr(), B, b, col0, int(bool(soft_margin)), float(alpha),
                                                         float(margin), out.data_ptr(), ws.data_ptr(), _stream()),
               'witw_exhaustive_loss_slab_fwd')
    return out


def exhaustive_loss_slab_sig(T, diag, col0, soft_margin=False, alpha=10., margin=1.):
    """-> (rowsig [B]: this slab's part of the row sums of l', to be summed over the ranks; colsig [b]: complete)."""
    T, diag, B, b, col0 = _slab('exhaustive_loss_slab_sig', T, diag, col0)
    rowsig = torch.empty((B,), dtype=torch.float32, device=T.device)
    colsig = torch.empty((b,), dtype=torch.float32, device=T.device)
    _lib.check(_lib.load().witw_exhaustive_loss_slab_sig(T.data_ptr(), diag.data_ptr(), B, b, col0, int(bool(soft_margin)), float(alpha),
                                                         float(margin), rowsig.data_ptr(), colsig.data_ptr(), _stream()),
               'witw_exhaustive_loss_slab_sig')
    return rowsig, colsig


def exhaustive_loss_slab_bwd(T, diag, rowsig, colsig, grad_loss, col0, soft_margin=False, alpha=10., margin=1.):
    """G [B,b] = dL/dT of the slab for grad_loss of the GLOBAL loss; rowsig = the row sums summed over the ranks."""
    T, diag, B, b, col0 = _slab('exhaustive_loss_slab_bwd', T, diag, col0)
    rowsig, colsig = _dev_f32(rowsig, 'rowsig'), _dev_f32(colsig, 'colsig')
    if rowsig.numel() != B or colsig.numel() != b:
        raise _lib.WitwError('exhaustive_loss_slab_bwd: rowsig / colsig must hold one sum per row / column of the slab')
    gl = _dev_f32(grad_loss.reshape(1).contiguous(), 'grad_loss')
    G = torch.empty_like(T)
    _lib.check(_lib.load().witw_exhaustive_loss_slab_bwd(T.data_ptr(), diag.data_ptr(), rowsig.data_ptr(), colsig.data_ptr(), gl.data_ptr(),
                                                         G.data_ptr(), B, b, col0, int(bool(soft_margin)), float(alpha), float(margin),
                                                         _stream()), 'witw_exhaustive_loss_slab_bwd')
    return G


def sqdist_rect_bwd(x, y, G, need_dx=True, need_dy=True):
    """Backward of T = ops.pairwise_sqdist(x [B,n], y [b,n]) for G = dL/dT [B,b] -> (dx [B,n] or None, dy [b,n] or None)."""
    x, y, G = _dev_f32(x, 'x'), _dev_f32(y, 'y'), _dev_f32(G, 'G')
    if x.dim() != 2 or y.dim() != 2 or x.shape[1] != y.shape[1] or tuple(G.shape) != (x.shape[0], y.shape[0]):
        raise _lib.WitwError('sqdist_rect_bwd: need x [B,n], y [b,n] and G [B,b], got %s, %s and %s'
                             % (tuple(x.shape), tuple(y.shape), tuple(G.shape)))
    dx = torch.empty_like(x) if need_dx else None
    dy = torch.empty_like(y) if need_dy else None
    _lib.check(_lib.load().witw_sqdist_rect_bwd(x.data_ptr(), y.data_ptr(), G.data_ptr(), _p(dx), _p(dy), x.shape[0], y.shape[0], x.shape[1],
                                                _stream()), 'witw_sqdist_rect_bwd')
    return dx, dy
