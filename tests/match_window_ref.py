"""The masked match restated on the oracle (test infrastructure; oracle/ itself is frozen).

A shift mask is one 64-bit word per query: bit k set = shift k may be chosen; a word of 0 = no prior = all 64 bits. With
sc = O.correlation_scores(ov, su) [Bo,Bs,64]:

    orientation = argmax_k(sc.masked_fill(~allowed[None], -inf))          # torch.argmax: the first maximal index wins
    distance    = l2_distance(crop_overhead(ov, orientation, We), su)      # unchanged, at the chosen shift
"""
import numpy as np
import torch

from oracle import cvig_fov_oracle as O

ALL = -1      # int64 word with all 64 bits set


def words(bit_lists):
    """[[k, ...], ...] -> int64 [Bs] mask words (bit 63 makes a word negative)."""
    out = np.zeros(len(bit_lists), dtype=np.uint64)
    for i, bits in enumerate(bit_lists):
        for k in bits:
            out[i] |= np.uint64(1) << np.uint64(k)
    return torch.from_numpy(out.view(np.int64).copy())


def window_words(starts, widths):
    """mask words allowing the `widths[s]` consecutive shifts (circular) from `starts[s]` on."""
    return words([[(int(a) + j) % 64 for j in range(int(w))] for a, w in zip(starts, widths)])


def allowed(mask):
    """int64 [Bs] -> bool [Bs,64]; a zero word allows everything."""
    m = mask.cpu().numpy().view(np.uint64)
    bits = ((m[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    bits[m == 0] = True
    return torch.from_numpy(bits)


def masked_scores(sc, mask):
    return sc.masked_fill(~allowed(mask)[None], float('-inf'))


def correlation(ov, su, mask):
    return torch.argmax(masked_scores(O.correlation_scores(ov, su), mask), -1)


def match(ov, su, mask):
    """The three lines of the definition, through the oracle's materialising crop_overhead / l2_distance."""
    ori = correlation(ov, su, mask)
    return ori, O.l2_distance(O.crop_overhead(ov, ori, su.shape[3]), su)


def scores_pair(ov, su):
    """(fp32, fp64) correlation scores: the part of match_fused that does not depend on the mask."""
    return O.correlation_scores(ov, su), O.correlation_scores(ov.double(), su.double())


def match_fused(ov, su, mask, scores=None):
    """O.match_fused with the mask: no crop tensor, fp64 accumulation (large shapes). -> (orientation from the fp32 scores as
    O.match_fused takes it, distance f32, gap = best minus second-best ALLOWED fp64 score; +inf where one shift is allowed).
    scores: scores_pair(ov, su), when several masks are tried on the same embeddings."""
    ovd, sud = ov.double(), su.double()
    we, w = su.shape[3], ov.shape[3]
    sc32, sc = scores if scores is not None else scores_pair(ov, su)
    ori = torch.argmax(masked_scores(sc32, mask), -1)
    col = (ovd * ovd).sum(dim=(1, 2))
    col2 = torch.cat((col, col[:, :we - 1]), dim=1) if we > 1 else col
    win = col2.unfold(1, we, 1)[:, :w].sum(-1)
    best = torch.gather(sc, 2, ori[:, :, None]).squeeze(-1)
    wn = torch.gather(win, 1, ori).sqrt()
    sn = sud.reshape(sud.shape[0], -1).norm(dim=1)
    top2 = masked_scores(sc, mask).topk(2, -1).values
    gap = top2[..., 0] - top2[..., 1]
    return ori, (2 * (1 - best / (wn * sn[None, :]))).float(), gap
