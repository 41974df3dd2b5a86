"""float64 reference of the match backward (csrc/match.hip: match_bwd_*_kernel; csrc/loss_hard.hip: pairs_bwd_*_kernel), written
from the closed form in the kernels' header comment, not through torch autograd:

    window[o, s][ch, k] = ov[o, ch, (k + ori[o, s]) & 63],  k < We           (ch: the 16 x 4 = 64 rows of an embedding)
    c = <window, su[s]>,  wn = |window|,  sn = |su[s]|,  d = 2 (1 - c / (wn sn))
    dd/dsu[s][ch, k]     = -2 window[ch, k] / (wn sn) + 2 c su[s][ch, k] / (wn sn^3)
    dd/dwindow[ch, k]    = -2 su[s][ch, k] / (wn sn)  + 2 c window[ch, k] / (wn^3 sn)

ori is a constant of the graph. match_bwd_ref returns the gradients of sum(gD * d): grad_su sums dd/dsu over the overheads,
grad_ov scatters dd/dwindow to the columns (k + ori) & 63 and sums over the surfaces. Each gradient comes with a per-element
scale, the same sum over the ABSOLUTE values of its terms (the window / su term and the self term alike): the error of a result
is measured against it (tests/wgrad_ref.py: err), and an element whose scale is 0 -- no term at all -- must be an exact 0.

kernel_inputs gives, in float64, what the kernels take next to the embeddings: score (= c), wn [Bo, 64] (the window norm at
EVERY shift, as witw_match_fwd leaves it in its workspace) and sn [Bs]; the tests round them to fp32.

The pair-list form (witw_match_bwd_pairs) is the same reference at gD = the pair weights scattered with accumulation; entries
with an index outside [0, Bo) x [0, Bs) are dropped. Its scale scatters |pair_w|: the kernel sums one term per list entry.

geometry restates match_bwd_splits and the launcher's cdiv (csrc/match.hip: witw_match_bwd).
"""
import numpy as np

from tests.wgrad_ref import F32_ULP, err  # noqa: F401  (the error measure of the edge tests)

W = 64          # columns of an overhead embedding = number of shifts
CH = 64         # 16 x 4 rows


def _f64(t):
    if hasattr(t, 'detach'):
        t = t.detach().cpu().double().numpy()
    return np.ascontiguousarray(np.asarray(t, dtype=np.float64))


def _i64(t):
    if hasattr(t, 'detach'):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t, dtype=np.int64))


def _operands(ov, su, ori):
    ov, su, ori = _f64(ov), _f64(su), _i64(ori)
    Bo, Bs, We = ov.shape[0], su.shape[0], su.shape[3]
    if ov.shape != (Bo, 16, 4, W) or su.shape != (Bs, 16, 4, We) or not 1 <= We <= W or ori.shape != (Bo, Bs):
        raise ValueError('ov %s, su %s, ori %s are not [Bo,16,4,64], [Bs,16,4,We], [Bo,Bs]' % (ov.shape, su.shape, ori.shape))
    if ori.min() < 0 or ori.max() >= W:
        raise ValueError('orientation outside [0, 64)')
    return ov.reshape(Bo, CH, W), su.reshape(Bs, CH, We), ori


def _columns(ori_row, We):
    """[Bs, We]: the overhead column under window position k of every surface"""
    return (np.arange(We)[None, :] + ori_row[:, None]) & (W - 1)


def kernel_inputs(ov, su, ori):
    """-> (score [Bo, Bs], wn [Bo, 64], sn [Bs]) float64"""
    ov, su, ori = _operands(ov, su, ori)
    Bo, Bs, We = ov.shape[0], su.shape[0], su.shape[2]
    col = (ov * ov).sum(axis=1)                                             # [Bo, 64] energy per column
    k = (np.arange(W)[:, None] + np.arange(We)[None, :]) & (W - 1)          # [shift, k]
    wn = np.sqrt(col[:, k].sum(axis=2))
    sn = np.sqrt((su * su).sum(axis=(1, 2)))
    score = np.empty((Bo, Bs), dtype=np.float64)
    for o in range(Bo):
        win = ov[o][:, _columns(ori[o], We)]                                # [ch, Bs, We]
        score[o] = np.einsum('csk,sck->s', win, su)
    return score, wn, sn


def match_bwd_ref(ov, su, ori, gD, gD_abs=None):
    """-> (grad_ov [Bo,16,4,64], grad_su [Bs,16,4,We], scale_ov, scale_su) float64 for the loss sum(gD * d).
    gD_abs: what the scales weigh the terms with (default |gD|; the pair form passes the scattered |pair_w|)."""
    ov, su, ori = _operands(ov, su, ori)
    Bo, Bs, We = ov.shape[0], su.shape[0], su.shape[2]
    gD = _f64(gD)
    gA = np.abs(gD) if gD_abs is None else _f64(gD_abs)
    if gD.shape != (Bo, Bs) or gA.shape != (Bo, Bs):
        raise ValueError('gD %s is not [%d, %d]' % (gD.shape, Bo, Bs))
    score, wn, sn = kernel_inputs(ov.reshape(Bo, 16, 4, W), su.reshape(Bs, 16, 4, We), ori)
    su_abs, ov_abs = np.abs(su), np.abs(ov)
    g_su, s_su = np.zeros_like(su), np.zeros_like(su)
    self_su, self_su_abs = np.zeros(Bs), np.zeros(Bs)
    g_ov, s_ov = np.zeros_like(ov), np.zeros_like(ov)
    eye = np.eye(W)
    for o in range(Bo):
        cols = _columns(ori[o], We)                                         # [Bs, We]
        wv = wn[o, ori[o]]                                                  # [Bs]
        a = -2.0 / (wv * sn)                                                # coefficient of the window / su term
        # ---- grad_su: the window term now, the self term (a multiple of su[s]) after the loop
        win = ov[o][:, cols].transpose(1, 0, 2)                             # [Bs, ch, We]
        g_su += (gD[o] * a)[:, None, None] * win
        s_su += (gA[o] * -a)[:, None, None] * np.abs(win)
        b_su = 2.0 * score[o] / (wv * sn ** 3)
        self_su += gD[o] * b_su
        self_su_abs += gA[o] * np.abs(b_su)
        # ---- grad_ov[o]: scatter su[s][ch, k] to column cols[s, k]; the self term covers the window's columns only
        onehot = eye[cols.ravel()]                                          # [Bs * We, 64]
        g_ov[o] = ((gD[o] * a)[:, None, None] * su).transpose(1, 0, 2).reshape(CH, Bs * We) @ onehot
        s_ov[o] = ((gA[o] * -a)[:, None, None] * su_abs).transpose(1, 0, 2).reshape(CH, Bs * We) @ onehot
        b_ov = 2.0 * score[o] / (wv ** 3 * sn)
        cover = onehot.reshape(Bs, We, W).sum(axis=1)                       # [Bs, 64]: 1 where the window of s covers column w
        g_ov[o] += ov[o] * ((gD[o] * b_ov) @ cover)[None, :]
        s_ov[o] += ov_abs[o] * ((gA[o] * np.abs(b_ov)) @ cover)[None, :]
    g_su += su * self_su[:, None, None]
    s_su += su_abs * self_su_abs[:, None, None]
    shape_o, shape_s = (Bo, 16, 4, W), (Bs, 16, 4, We)
    return g_ov.reshape(shape_o), g_su.reshape(shape_s), s_ov.reshape(shape_o), s_su.reshape(shape_s)


def pairs_to_dense(po, ps, pw, Bo, Bs):
    """-> (gD, gD_abs, valid) float64 [Bo, Bs] x 2 and the mask of the entries that count: pw (and |pw|) scattered with
    accumulation, entries with an index out of range dropped"""
    po, ps, pw = _i64(po), _i64(ps), _f64(pw)
    if not po.shape == ps.shape == pw.shape or po.ndim != 1:
        raise ValueError('pair list of unequal lengths')
    ok = (po >= 0) & (po < Bo) & (ps >= 0) & (ps < Bs)
    gD, gA = np.zeros((Bo, Bs)), np.zeros((Bo, Bs))
    np.add.at(gD, (po[ok], ps[ok]), pw[ok])
    np.add.at(gA, (po[ok], ps[ok]), np.abs(pw[ok]))
    return gD, gA, ok


def match_bwd_pairs_ref(ov, su, ori, po, ps, pw):
    """match_bwd_ref for a pair list -> (grad_ov, grad_su, scale_ov, scale_su)"""
    gD, gA, _ok = pairs_to_dense(po, ps, pw, _f64(ov).shape[0], _f64(su).shape[0])
    return match_bwd_ref(ov, su, ori, gD, gA)


def cdiv(a, b):
    return -(-a // b)


def splits(Bo, Bs):
    """match_bwd_splits: enough (surface, split) blocks for 768, at least 32 overheads per split"""
    return max(1, min(cdiv(768, Bs), cdiv(Bo, 32)))


def geometry(Bo, Bs):
    """(splits, overheads per split, trailing splits whose overhead range is empty) of witw_match_bwd given scratch"""
    s = splits(Bo, Bs)
    per = cdiv(Bo, s)
    return s, per, s - cdiv(Bo, per)


def scratch_floats(Bo, Bs, We):
    """witw_match_bwd_scratch_floats"""
    s = splits(Bo, Bs)
    return s * Bs * (64 * We + 1) if s > 1 else 0
