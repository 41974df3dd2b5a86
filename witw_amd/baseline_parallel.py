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


# ---------------------------------------------------------------------------------------------------------------- synchronised BatchNorm
# cvig_baseline's BatchNorm2d over the GLOBAL batch (SurfaceEncoder(sync_bn=True)): the split entries of csrc/baseline_bn_sync.hip
# (bn_partial_stats / bn_finalize_stats / bn_lrelu_bwd_partial / bn_lrelu_bwd_apply below: here and not in ops.py, as the slab wrappers above;
# their memory-contract cases are in tests/test_baseline_sync_bn_gpu.py) with one all-reduce of 2C floats in the seam
# of each direction. With no process group, or a world of one, the same entries run back to back without a collective.

def _bn_vec(t, name, n):
    """a per-channel operand of the split BatchNorm entries: fp32 on the device, contiguous, n entries"""
    t = _dev_f32(t.detach(), name)
    if t.numel() != n:
        raise _lib.WitwError('%s must have %d entries, got %d' % (name, n, t.numel()))
    return t


def _bn_s2d_cp(name, a, dy, valid_hw, dy_s2d):
    """the dy_s2d_cp argument: 0 for dy shaped like a, else the channel stride of the space-to-depth gradient (checked as bn_lrelu_bwd does)"""
    B, _Hp, _Wp, C = a.shape
    H, W = valid_hw
    if not dy_s2d:
        if dy.shape != a.shape:
            raise _lib.WitwError('%s: gradient %s does not match activation %s' % (name, tuple(dy.shape), tuple(a.shape)))
        return 0
    if dy.dim() != 4 or tuple(dy.shape[:3]) != (B, (H + 1) // 2, (W + 1) // 2) or dy.shape[3] < 4 * C:
        raise _lib.WitwError('%s: space-to-depth gradient %s does not match activation %s valid %s' % (name, tuple(dy.shape), tuple(a.shape), (H, W)))
    return dy.shape[3]


def bn_partial_stats(a, valid_hw, pivot):
    """This rank's share of the BatchNorm2d batch statistics over the valid region of a NHWC tensor -> part [2C]: sum (a - pivot[c])
    and sum (a - pivot[c])^2 per channel. `pivot` [C] must be the same on every rank whose parts are added (witw_bn_partial_stats)."""
    lib = _lib.load()
    a = _dev_f32(a, 'a')
    B, Hp, Wp, C = a.shape
    H, W = valid_hw
    pivot = _bn_vec(pivot, 'pivot', C)
    part = torch.empty((2 * C,), dtype=torch.float32, device=a.device)
    ws = torch.empty(lib.witw_bn_workspace_floats(B, H, W, C), dtype=torch.float32, device=a.device)
    _lib.check(lib.witw_bn_partial_stats(a.data_ptr(), B, Hp, Wp, H, W, C, pivot.data_ptr(), part.data_ptr(), ws.data_ptr(), _stream()),
               'witw_bn_partial_stats')
    return part


def bn_finalize_stats(part_sum, pivot, count, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1):
    """The parts of bn_partial_stats added over the ranks, and the values per channel behind them (`count`, the global B*H*W)
    -> (mean, invstd, scale, shift), what bn_train_stats returns for the whole batch; the running buffers are updated in place.
    `pivot` may be running_mean itself. count <= 1 is refused (witw_bn_finalize_stats)."""
    lib = _lib.load()
    C = part_sum.numel() // 2
    part_sum = _bn_vec(part_sum, 'part_sum', 2 * C)
    pivot, gamma, beta = _bn_vec(pivot, 'pivot', C), _bn_vec(gamma, 'gamma', C), _bn_vec(beta, 'beta', C)
    if (running_mean is None) != (running_var is None):
        raise _lib.WitwError('bn_finalize_stats: running_mean and running_var come together')
    if running_mean is not None:
        running_mean, running_var = _bn_vec(running_mean, 'running_mean', C), _bn_vec(running_var, 'running_var', C)
    out = [torch.empty((C,), dtype=torch.float32, device=part_sum.device) for _ in range(4)]
    _lib.check(lib.witw_bn_finalize_stats(part_sum.data_ptr(), pivot.data_ptr(), int(count), gamma.data_ptr(), beta.data_ptr(), float(eps),
                                          float(momentum), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                                          _p(running_mean), _p(running_var), C, _stream()), 'witw_bn_finalize_stats')
    return out


def bn_lrelu_bwd_partial(a, dy, valid_hw, mean, invstd, dy_s2d=False):
    """This rank's share of the two sums of bn_lrelu_bwd -> part [2C]: sum dy and sum dy * xhat per channel; dy as in bn_lrelu_bwd."""
    lib = _lib.load()
    a, dy = _dev_f32(a, 'a'), _dev_f32(dy, 'dy')
    B, Hp, Wp, C = a.shape
    H, W = valid_hw
    cp = _bn_s2d_cp('bn_lrelu_bwd_partial', a, dy, valid_hw, dy_s2d)
    mean, invstd = _bn_vec(mean, 'mean', C), _bn_vec(invstd, 'invstd', C)
    part = torch.empty((2 * C,), dtype=torch.float32, device=a.device)
    ws = torch.empty(lib.witw_bn_workspace_floats(B, H, W, C), dtype=torch.float32, device=a.device)
    _lib.check(lib.witw_bn_lrelu_bwd_partial(a.data_ptr(), dy.data_ptr(), mean.data_ptr(), invstd.data_ptr(), B, Hp, Wp, H, W, C, cp,
                                             part.data_ptr(), ws.data_ptr(), _stream()), 'witw_bn_lrelu_bwd_partial')
    return part


def bn_lrelu_bwd_apply(a, dy, valid_hw, mean, invstd, gamma, sums, count, slope=0.2, dy_s2d=False):
    """-> dz of bn_lrelu_bwd from `sums` [2C] = the parts of bn_lrelu_bwd_partial added over the ranks and the global `count` of
    values per channel. dbeta = sums[:C] and dgamma = sums[C:] are the global parameter gradients (witw_bn_lrelu_bwd_apply)."""
    lib = _lib.load()
    a, dy = _dev_f32(a, 'a'), _dev_f32(dy, 'dy')
    B, Hp, Wp, C = a.shape
    H, W = valid_hw
    cp = _bn_s2d_cp('bn_lrelu_bwd_apply', a, dy, valid_hw, dy_s2d)
    mean, invstd, gamma = _bn_vec(mean, 'mean', C), _bn_vec(invstd, 'invstd', C), _bn_vec(gamma, 'gamma', C)
    sums = _bn_vec(sums, 'sums', 2 * C)
    dz = torch.empty_like(a)
    _lib.check(lib.witw_bn_lrelu_bwd_apply(a.data_ptr(), dy.data_ptr(), dz.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                                           sums.data_ptr(), int(count), B, Hp, Wp, H, W, C, float(slope), cp, _stream()),
               'witw_bn_lrelu_bwd_apply')
    return dz


def sync_bn_global_images(b, device):
    """The images of the global batch from this rank's b: one all-reduce of a number per encoder call, so that the ranks' shares
    need not be equal (training refuses unequal shares in the loss, as without sync_bn). A host read."""
    from . import parallel
    if parallel.world() == 1:
        return int(b)
    n = torch.tensor([int(b)], dtype=torch.int64, device=device)
    with parallel.phase('bn_stats_all_reduce'):
        parallel.all_reduce_sum_(n)
    return int(n.item())


def sync_bn_train_stats(a, valid_hw, bn, images):
    """ops.bn_train_stats over the global batch of `images` images -> (mean, invstd, scale, shift), the same on every rank; bn's
    running buffers take the global statistics on every rank alike. The sums are taken about bn.running_mean as it stands before the
    call: rank-identical after parallel.broadcast_parameters / broadcast_buffers, and it stays so because every rank applies the
    same update."""
    from . import parallel
    part = bn_partial_stats(a, valid_hw, bn.running_mean)
    with parallel.phase('bn_stats_all_reduce'):
        parallel.all_reduce_sum_(part)
    return bn_finalize_stats(part, bn.running_mean, int(images) * valid_hw[0] * valid_hw[1], bn.weight, bn.bias, bn.running_mean,
                                 bn.running_var, bn.eps, bn.momentum)


def sync_bn_lrelu_bwd(a, dy, valid_hw, mean, invstd, gamma, images, slope=0.2, dy_s2d=False):
    """ops.bn_lrelu_bwd over the global batch -> (dz of this rank's images, dgamma / N, dbeta / N) on N ranks. The two sums are complete
    on every rank after their all-reduce, and so are dgamma and dbeta -- but the step's gradient all-reduce (parallel.OverlappedGradReducer
    / all_reduce_grads: SUM over the ranks of every parameter gradient, the conv gradients being per-rank shares) would then count them
    N times. Each rank therefore hands over 1/N of them and that SUM restores the global value; the reducer is unchanged and the
    BatchNorm parameters stay in its buckets. Exact for N a power of two, one rounding otherwise. Before the gradient all-reduce
    bn.weight.grad / bn.bias.grad hold 1/N of the gradient."""
    from . import parallel
    sums = bn_lrelu_bwd_partial(a, dy, valid_hw, mean, invstd, dy_s2d=dy_s2d)
    with parallel.phase('bn_grad_all_reduce'):
        parallel.all_reduce_sum_(sums)
    dz = bn_lrelu_bwd_apply(a, dy, valid_hw, mean, invstd, gamma, sums, int(images) * valid_hw[0] * valid_hw[1], slope, dy_s2d=dy_s2d)
    C = sums.numel() // 2
    if parallel.world() > 1:
        sums = sums / parallel.world()
    return dz, sums[C:], sums[:C]
