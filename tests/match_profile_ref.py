"""numpy restatements for the orientation-profile tests (tests/test_match_profile.py, tests/test_match_profile_gpu.py; CPU only):
the kernel form witw_match_profile reaches, the fp32 distance epilogue at every shift, the hypothesis rule of
witw_profile_hypotheses, and the derived rounding bound of a score against a float64 sum.
"""
import numpy as np

SHIFTS = 64
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def dispatch(Bo, Bs, We):
    """witw_match_profile (csrc/match.hip) restated: the match_kernel<OPW,MT,false,true> instantiation a shape reaches -- only the
    generic forms have the profile epilogue, chosen by the grid arithmetic match_fwd_launch uses for them."""
    cdiv = lambda a, b: (a + b - 1) // b
    gx = cdiv(Bs, 128)
    if gx * cdiv(Bo, 4) >= 512:
        return 'match_kernel<2,2,false,true>'
    if gx * cdiv(Bo, 2) >= 256:
        return 'match_kernel<1,2,false,true>'
    return 'match_kernel<1,1,false,true>'


def distance_all_f32(sc, n2w, n2s):
    """The profile epilogue in np.float32, one rounding per operation, at every shift: sc [Bo,Bs,64] (exact scores), n2w [Bo,64] /
    n2s [Bs] exact norm squares -> 2 * (1 - v / (sqrt(n2w[o,k]) * sqrt(n2s[s]))) as float32 [Bo,Bs,64]."""
    with np.errstate(all='ignore'):
        wn = np.sqrt(n2w.astype(np.float32))
        sn = np.sqrt(n2s.astype(np.float32))
        q = sc.astype(np.float32) / (wn[:, None, :] * sn[None, :, None])
        return np.float32(2) * (np.float32(1) - q)


def allowed_bits(words, n):
    """uint64 [n_words] (or None) -> bool [n,64]: profile p reads word p % n_words; None or a word of 0 allows every shift."""
    if words is None:
        return np.ones((n, SHIFTS), dtype=bool)
    words = np.asarray(words).view(np.uint64).reshape(-1)
    w = words[np.arange(n) % len(words)]
    bits = ((w[:, None] >> np.arange(SHIFTS, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    bits[w == 0] = True
    return bits


def hypotheses(score_all, n_hyp, min_sep, words=None):
    """The rule of witw_profile_hypotheses on finite (or infinite, not NaN) scores: score_all [...,64] -> int64 [...,n_hyp].
    Hypothesis 1: the first maximum over the allowed shifts; hypothesis j + 1: the first maximum over the allowed shifts whose
    circular distance on the ring of 64 to every earlier hypothesis is > min_sep; -1 once no shift is left."""
    sc = np.asarray(score_all, dtype=np.float64)
    lead = sc.shape[:-1]
    sc = sc.reshape(-1, SHIFTS)
    n = sc.shape[0]
    live = allowed_bits(words, n)
    out = np.full((n, n_hyp), -1, dtype=np.int64)
    ring = np.arange(SHIFTS)
    for j in range(n_hyp):                       # all profiles at once; a profile whose shifts are used up keeps -1
        has = live.any(axis=1)
        cand = np.where(live, sc, -np.inf)
        k = (live & (cand == cand.max(axis=1)[:, None])).argmax(axis=1)      # the first allowed index that holds the maximum
        out[:, j] = np.where(has, k, -1)
        d = np.abs(ring[None, :] - k[:, None])
        live &= (np.minimum(d, SHIFTS - d) > min_sep) & has[:, None]
    return out.reshape(lead + (n_hyp,))


def score_bound(ov, su, We):
    """The derived bound of |fp32 chain - exact sum| per (pair, shift): (64 * We + 2) * 2^-24 * sum |ov * su|. The chain is
    N = 64 * We fused multiply-adds with one rounding each (the pad column of an odd width multiplies an exact zero and rounds
    nothing), so its error is at most gamma_N * sum |ov * su|, gamma_N = N u / (1 - N u), u = 2^-24; with N <= 4096,
    gamma_N <= (N + N^2 u (1 + 2^-11)) u <= (N + 2) u. Nothing measured enters.
    ov [Bo,64,64], su [Bs,64,We] float64 -> float64 [Bo,Bs,64]."""
    a, b = np.abs(ov), np.abs(su)
    Bo, Bs = ov.shape[0], su.shape[0]
    out = np.zeros((Bo, Bs, SHIFTS))
    bt = b.reshape(Bs, -1).T
    for sh in range(SHIFTS):
        out[:, :, sh] = a[:, :, (np.arange(We) + sh) % 64].reshape(Bo, -1) @ bt
    return (64 * We + 2) * 2.0 ** -24 * out
