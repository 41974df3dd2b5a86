"""Host-side wrappers of csrc/baseline_retrieval.hip: row norms, the GEMM-form squared-distance matrix and the exact re-scoring of
a list of pairs. They are the op set of cvig_baseline.retrieve(method='gemm') and live here, not in ops.py; their memory-contract
cases are in tests/test_baseline_retrieval_gpu.py. No CPU fallback."""
import torch

from . import _lib
from .ops import _dev_f32, _stream


def _rows(name, *ts):
    for t in ts:
        if t.dim() != 2 or t.shape[1] != ts[0].shape[1]:
            raise _lib.WitwError('%s: need [rows, n] operands of one width, got %s' % (name, [tuple(x.shape) for x in ts]))


def row_sqnorm(x):
    """x [N,n] -> |x_i|^2 as f32 [N] (witw_row_sqnorm)."""
    x = _dev_f32(x, 'x')
    _rows('row_sqnorm', x)
    out = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().witw_row_sqnorm(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], _stream()), 'witw_row_sqnorm')
    return out


def sqdist_gemm(g, q, gn, qn):
    """g [Ng,n], q [Nq,n] and their row_sqnorm -> D [Ng,Nq] = max(0, gn_i + qn_j - 2 g_i.q_j) on the fp32 MFMA: squared distances
    known to cvig_baseline.band_eps only (the product form cancels on near pairs). Ng is not bounded by 65,535."""
    g, q, gn, qn = _dev_f32(g, 'g'), _dev_f32(q, 'q'), _dev_f32(gn, 'gn'), _dev_f32(qn, 'qn')
    _rows('sqdist_gemm', g, q)
    if gn.numel() != g.shape[0] or qn.numel() != q.shape[0]:
        raise _lib.WitwError('sqdist_gemm: gn / qn must hold one norm per row of g / q')
    D = torch.empty((g.shape[0], q.shape[0]), dtype=torch.float32, device=g.device)
    _lib.check(_lib.load().witw_sqdist_gemm(g.data_ptr(), q.data_ptr(), gn.data_ptr(), qn.data_ptr(), D.data_ptr(), g.shape[0],
                                            q.shape[0], g.shape[1], _stream()), 'witw_sqdist_gemm')
    return D


def sqdist_pairs(g, q, pair_g, pair_q, take_sqrt=False):
    """out[p] = ops.pairwise_sqdist(g, q, take_sqrt)[pair_g[p], pair_q[p]] bit for bit, without the matrix (pair_g / pair_q: int32
    [P] on the device, inside the operands' rows)."""
    g, q = _dev_f32(g, 'g'), _dev_f32(q, 'q')
    _rows('sqdist_pairs', g, q)
    for name, t in (('pair_g', pair_g), ('pair_q', pair_q)):
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1 and t.numel() == pair_g.numel()):
            raise _lib.WitwError('sqdist_pairs: %s must be a contiguous int32 GPU vector, one entry per pair' % name)
    out = torch.empty((pair_g.numel(),), dtype=torch.float32, device=g.device)
    _lib.check(_lib.load().witw_sqdist_pairs(g.data_ptr(), q.data_ptr(), pair_g.data_ptr(), pair_q.data_ptr(), out.data_ptr(),
                                             pair_g.numel(), g.shape[1], int(take_sqrt), _stream()), 'witw_sqdist_pairs')
    return out
