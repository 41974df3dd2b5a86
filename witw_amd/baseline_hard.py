"""Host-side wrappers of csrc/baseline_loss_hard.hip: the batch-hard form of cvig_baseline's triplet loss on the [B, b] column slab
one rank holds of the global batch (loss partial and the gradient's pair list), and the pair-list backward of a squared-distance
matrix. With ops.pairwise_sqdist, ops.batch_hard_slab_mine and ops.batch_hard_merge_rows they are the op set of
cvig_baseline.sharded_batch_hard_loss and live here, not in ops.py; their memory-contract cases are in
tests/test_baseline_hard_gpu.py. No CPU fallback."""
import torch

from . import _lib
from .ops import _dev_f32, _p, _stream


def _dev_int(t, name, dtype, numel):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() == numel):
        raise _lib.WitwError('%s must be a contiguous %s GPU tensor of %d entries' % (name, str(dtype).replace('torch.', ''), numel))
    return t


def _cfg(soft_margin, alpha, margin):
    return int(bool(soft_margin)), float(alpha), float(margin)


def hard_slab_loss(T, rv, cv, col0, soft_margin=False, alpha=10., margin=1.):
    """Un-normalised loss partial f32 [1] of this rank's slab T [B,b] (witw_baseline_hard_slab_loss): the row terms of the anchors
    col0 .. col0+b-1 (rv [B] = the GLOBAL row minima) plus the column terms of its columns (cv [b]). The sum over the ranks, divided by
    2B, is the loss."""
    T, rv, cv = _dev_f32(T, 'T'), _dev_f32(rv, 'rv'), _dev_f32(cv, 'cv')
    if T.dim() != 2 or rv.numel() != T.shape[0] or cv.numel() != T.shape[1]:
        raise _lib.WitwError('hard_slab_loss: need a [B, b] slab, the B row minima and the b column minima, got %s, %s and %s'
                             % (tuple(T.shape), tuple(rv.shape), tuple(cv.shape)))
    out = torch.empty((1,), dtype=torch.float32, device=T.device)
    _lib.check(_lib.load().witw_baseline_hard_slab_loss(T.data_ptr(), rv.data_ptr(), cv.data_ptr(), T.shape[0], T.shape[1], int(col0),
                                                        *_cfg(soft_margin, alpha, margin), out.data_ptr(), _stream()),
               'witw_baseline_hard_slab_loss')
    return out


def hard_pairs(diag, rv, ri, cv, ci, grad_loss, col0, soft_margin=False, alpha=10., margin=1.):
    """The non-zeros of dL/dT in the columns [col0, col0+b) (b = cv.numel()) for grad_loss of the GLOBAL loss, as a pair list
    (pair_g int32 global row, pair_c int32 local column, pair_w f32) of 2b + B entries, unused ones (-1, -1, 0)."""
    diag, rv, cv = _dev_f32(diag, 'diag'), _dev_f32(rv, 'rv'), _dev_f32(cv, 'cv')
    B, b = diag.numel(), cv.numel()
    if rv.numel() != B:
        raise _lib.WitwError('hard_pairs: diag and rv must hold one entry per row of the global batch, got %d and %d' % (B, rv.numel()))
    ri, ci = _dev_int(ri, 'ri', torch.int64, B), _dev_int(ci, 'ci', torch.int64, b)
    gl = _dev_f32(grad_loss.reshape(1).contiguous(), 'grad_loss')
    P = 2 * b + B
    pg = torch.empty((P,), dtype=torch.int32, device=diag.device)
    pc = torch.empty((P,), dtype=torch.int32, device=diag.device)
    pw = torch.empty((P,), dtype=torch.float32, device=diag.device)
    _lib.check(_lib.load().witw_baseline_hard_pairs(diag.data_ptr(), rv.data_ptr(), ri.data_ptr(), cv.data_ptr(), ci.data_ptr(),
                                                    gl.data_ptr(), B, b, int(col0), *_cfg(soft_margin, alpha, margin), pg.data_ptr(),
                                                    pc.data_ptr(), pw.data_ptr(), _stream()), 'witw_baseline_hard_pairs')
    return pg, pc, pw


def sqdist_pairs_bwd(x, y, pair_g, pair_c, pair_w, need_dx=True, need_dy=True):
    """Backward of T = ops.pairwise_sqdist(x [B,n], y [b,n]) for dL/dT given as a pair list (dL/dT[g][c] = the sum of pair_w over the
    pairs (g, c); entries with an index out of range are skipped) -> (dx [B,n] or None, dy [b,n] or None), rows without a pair zero.
    Deterministic, no atomics."""
    x, y = _dev_f32(x, 'x'), _dev_f32(y, 'y')
    if x.dim() != 2 or y.dim() != 2 or x.shape[1] != y.shape[1]:
        raise _lib.WitwError('sqdist_pairs_bwd: need x [B,n] and y [b,n], got %s and %s' % (tuple(x.shape), tuple(y.shape)))
    P = pair_w.numel()
    pg, pc = _dev_int(pair_g, 'pair_g', torch.int32, P), _dev_int(pair_c, 'pair_c', torch.int32, P)
    pw = _dev_f32(pair_w, 'pair_w')
    lib = _lib.load()
    nb = lib.witw_sqdist_pairs_bwd_workspace_bytes(x.shape[0], y.shape[0], P)
    if nb < 0:
        raise _lib.WitwError('sqdist_pairs_bwd: unsupported shape B=%d b=%d with %d pairs' % (x.shape[0], y.shape[0], P))
    ws = torch.empty((nb,), dtype=torch.uint8, device=x.device) if nb else None
    dx = torch.empty_like(x) if need_dx else None
    dy = torch.empty_like(y) if need_dy else None
    _lib.check(lib.witw_sqdist_pairs_bwd(x.data_ptr(), y.data_ptr(), pg.data_ptr(), pc.data_ptr(), pw.data_ptr(), P, _p(dx), _p(dy),
                                         x.shape[0], y.shape[0], x.shape[1], _p(ws), _stream()), 'witw_sqdist_pairs_bwd')
    return dx, dy
