"""Writes tests/golden/loss_bits/loss_bits.npz: the exact bytes the triplet-loss kernels of both models (csrc/loss.hip, loss_hard.hip,
baseline_loss_slab.hip, baseline_loss_hard.hip, the loss and embed_normalize kernels of baseline.hip) return on fixed inputs, through
their Python wrappers. tests/test_loss_bits_gpu.py recomputes outputs() and compares byte for byte.

The inputs are a closed integer formula, multiples of 1/64 (1/256 on the diagonal), so that with margin 1 the hinge meets
x + margin == 0 exactly; positives are mostly smaller than negatives. The values depend on the toolchain's device expf / logf: run
this again, on an MI355X, when ROCm changes -- and only with a library whose kernels are known good, since what it writes becomes the
expectation.   python -m tests.golden.gen_loss_bits"""
import hashlib
import os

import numpy as np
import torch

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'loss_bits', 'loss_bits.npz')
DEV = torch.device('cuda:0')

# (B, b, col0): the smallest legal batch twice; a slab not at column 0; sizes off the wave width; the 256-stride loop of the column
# sums; the 256-stride loop of the row partials and of sum_parts
SHAPES = [(2, 2, 0), (2, 1, 1), (5, 2, 3), (67, 13, 54), (300, 41, 259), (300, 300, 0)]
FOV = [10., 1.]                                               # alpha
BASELINE = [(1, 10., 1.), (0, 10., 1.), (0, 10., 0.25)]       # (soft_margin, alpha, margin)
SPECIAL_SHAPE = (67, 13, 54)                                  # the batch-hard entries again with a NaN and with +inf entries
MAX_RAW = 4096                                                # a longer output is stored as the SHA-256 of its bytes


def grid(rows, cols, shift=0):
    i = torch.arange(rows, dtype=torch.int64)[:, None]
    j = torch.arange(cols, dtype=torch.int64)[None, :]
    return ((131 * i + 71 * j + 7 + shift) % 257).to(torch.float32) / 64


def matrix(B, special=None):
    D = grid(B, B)
    D.diagonal().mul_(0.25)
    if special == 'nan':
        D[60, 56] = float('nan')                 # off the diagonal, inside the slab: row 60's and column 56's minimum
    if special == 'inf':
        D[60, :60] = float('inf')                # anchor 60 has no finite negative among the overheads' row
        D[60, 61:] = float('inf')
        D[5, 58] = float('inf')
    return D.to(DEV)


def outputs():
    """name -> numpy array (or the 32 bytes of its SHA-256), in insertion order; needs the GPU"""
    from witw_amd import baseline_hard as BH
    from witw_amd import baseline_parallel as BP
    from witw_amd import ops
    out = {}
    gl = torch.tensor([0.7], device=DEV)

    def put(name, *tensors):
        for k, t in enumerate(tensors):
            a = t.detach().cpu().contiguous().numpy()
            if a.size > MAX_RAW:
                a = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
            out['%s.%d' % (name, k)] = a

    def hard(tag, D, b, col0):
        """the batch-hard entries of both models on the slab; rv / ri of the whole matrix stand in for the merged row minima"""
        B = D.shape[0]
        S, diag = D[:, col0:col0 + b].contiguous(), D.diagonal().contiguous()
        for alpha in FOV:
            loss, rv, ri, cv, ci = ops.batch_hard_fwd(D, alpha)
            _, _, cvs, cis = ops.batch_hard_slab_mine(S, col0)
            put('%s.fov%g.hard_fwd' % (tag, alpha), loss)
            put('%s.fov%g.hard_bwd' % (tag, alpha), ops.batch_hard_bwd(D, rv, ri, cv, ci, gl, alpha))
            put('%s.fov%g.hard_slab_loss' % (tag, alpha), ops.batch_hard_slab_loss(S, rv, cvs, col0, alpha))
            put('%s.fov%g.hard_pairs' % (tag, alpha), *ops.batch_hard_pairs(diag, rv, ri, cvs, cis, gl, col0, alpha))
        _, rv, ri, _, _ = ops.batch_hard_fwd(D, 1.)
        _, _, cvs, cis = ops.batch_hard_slab_mine(S, col0)
        for cfg in BASELINE:
            put('%s.base%d_%g_%g.hard_slab_loss' % ((tag,) + cfg), BH.hard_slab_loss(S, rv, cvs, col0, *cfg))
            put('%s.base%d_%g_%g.hard_pairs' % ((tag,) + cfg), *BH.hard_pairs(diag, rv, ri, cvs, cis, gl, col0, *cfg))

    dense_done = set()
    for B, b, col0 in SHAPES:
        tag = 'B%d_b%d_c%d' % (B, b, col0)
        D = matrix(B)
        S, diag = D[:, col0:col0 + b].contiguous(), D.diagonal().contiguous()
        for alpha in FOV:
            t = '%s.fov%g' % (tag, alpha)
            put(t + '.slab_fwd', ops.triplet_loss_slab_fwd(S, diag, col0, alpha))
            rowsig, colsig = ops.triplet_loss_slab_sig(S, diag, col0, alpha)
            put(t + '.slab_sig', rowsig, colsig)
            put(t + '.slab_bwd', ops.triplet_loss_slab_bwd(S, diag, rowsig, colsig, gl, col0, alpha))
        for cfg in BASELINE:
            t = '%s.base%d_%g_%g' % ((tag,) + cfg)
            put(t + '.slab_fwd', BP.exhaustive_loss_slab_fwd(S, diag, col0, *cfg))
            rowsig, colsig = BP.exhaustive_loss_slab_sig(S, diag, col0, *cfg)
            put(t + '.slab_sig', rowsig, colsig)
            put(t + '.slab_bwd', BP.exhaustive_loss_slab_bwd(S, diag, rowsig, colsig, gl, col0, *cfg))
        hard(tag, D, b, col0)
        if B in dense_done:
            continue
        dense_done.add(B)
        for alpha in FOV:
            loss, ws = ops.triplet_loss_fwd(D, alpha)
            put('B%d.fov%g.dense' % (B, alpha), loss, ws, ops.triplet_loss_bwd(D, ws, gl, alpha))
        e1, e2 = grid(B, 5, 3).to(DEV), grid(B, 5, 11).to(DEV)
        for cfg in BASELINE:
            put('B%d.base%d_%g_%g.dense' % ((B,) + cfg), ops.exhaustive_triplet_loss(D, *cfg).reshape(1),
                *ops.exhaustive_triplet_loss_bwd(e1, e2, D, gl, *cfg))
    B, b, col0 = SPECIAL_SHAPE
    for special in ('nan', 'inf'):
        hard('B%d_b%d_c%d.%s' % (B, b, col0, special), matrix(B, special), b, col0)
    for n in (5, 300):
        g, df = (grid(3, n, 1) + 0.5).to(DEV), (grid(3, n, 29) - 2).to(DEV)
        put('normalize.n%d' % n, ops.embed_normalize_(g.clone()), ops.embed_normalize_bwd(g, df))
    torch.cuda.synchronize()
    return out


if __name__ == '__main__':
    res = outputs()
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    np.savez_compressed(PATH, **res)
    print('%d arrays, %d bytes' % (len(res), os.path.getsize(PATH)))
