"""Orientation profiles: the match at every shift, and ranked orientation hypotheses (witw_match_profile,
witw_match_pairs_profile, witw_profile_hypotheses of include/witw_hip.h).

Host-side wrappers in the manner of ops.py: torch tensors in, C-ABI calls out, no CPU fallback. The public surface on top
of them is cvig_fov.orientation_profile / orientation_hypotheses.
"""
import torch

from . import _lib, ops

SHIFTS = 64


def _pair_list(name, pair_o, pair_s):
    """the two index tensors of a pair list, checked as the kernels read them -> their length"""
    if not isinstance(pair_o, torch.Tensor):
        raise _lib.WitwError('%s: pair_o must be a tensor, got %s' % (name, type(pair_o)))
    n = int(pair_o.numel())
    for what, t in (('pair_o', pair_o), ('pair_s', pair_s)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1
                and t.numel() == n):
            raise _lib.WitwError('%s: %s must be a contiguous int32 GPU tensor of %d entries' % (name, what, n))
    return n


def match_profile(overhead_embed, surface_embed, want_scores=True, want_distances=True, want_workspace=False):
    """The match at EVERY shift: overhead_embed [Bo,16,4,64], surface_embed [Bs,16,4,We] -> (scores, distances[, workspace]),
    each f32 [Bo,Bs,64] (None where not wanted; at least one is). scores[o,s,k] is the correlation at shift k and
    distances[o,s,k] = 2 * (1 - score / (|window(o,k)| * |su[s]|)). Per pair the 64 scores carry the bits of the chain every
    form of ops.match_fwd runs: their first arg-max is its orientation, and the two values there are its score and distance.
    workspace: the norms as match_fwd leaves them (match_pairs / match_pairs_profile take it)."""
    lib = _lib.load()
    ov, su, Bo, Bs, We = ops._match_operands('match_profile', overhead_embed, surface_embed)
    if not (want_scores or want_distances):
        raise _lib.WitwError('match_profile: nothing wanted (want_scores and want_distances are both False)')
    scores = torch.empty((Bo, Bs, SHIFTS), dtype=torch.float32, device=ov.device) if want_scores else None
    dists = torch.empty((Bo, Bs, SHIFTS), dtype=torch.float32, device=ov.device) if want_distances else None
    ws = torch.empty(lib.witw_match_workspace_floats(Bo, Bs), dtype=torch.float32, device=ov.device)
    prof = ops._prof_begin()
    _lib.check(lib.witw_match_profile(ov.data_ptr(), su.data_ptr(), Bo, Bs, We, ops._p(scores), ops._p(dists), ws.data_ptr(),
                                      ops._stream()), 'witw_match_profile')
    if prof is not None:      # the launch = two small norm kernels + the match kernel, as in match_fwd
        ops._prof_end(prof, ('match_profile', We), 2.0 * 64 * (64 * We) * Bo * Bs)
    return (scores, dists, ws) if want_workspace else (scores, dists)


def match_pairs_profile(overhead_embed, surface_embed, wn, sn, pair_o, pair_s, want_scores=True, want_distances=True):
    """match_profile for a LIST of pairs (overhead row pair_o[i], surface row pair_s[i]; int32 on the device, every index
    inside its batch -- the kernel does not check) -> (scores, distances), each f32 [n,64] or None, rows bit-identical to
    match_profile's rows of those pairs. wn / sn: the norm blocks of a match_fwd / match_profile workspace over the same
    tensors (wn = ws[:Bo * 64], sn = ws[Bo * 64:Bo * 64 + Bs])."""
    lib = _lib.load()
    ov, su, Bo, Bs, We = ops._match_operands('match_pairs_profile', overhead_embed, surface_embed)
    n = _pair_list('match_pairs_profile', pair_o, pair_s)
    if not (want_scores or want_distances):
        raise _lib.WitwError('match_pairs_profile: nothing wanted (want_scores and want_distances are both False)')
    wn, sn = ops._dev_f32(wn, 'wn'), ops._dev_f32(sn, 'sn')
    if wn.numel() != Bo * 64 or sn.numel() != Bs:
        raise _lib.WitwError('match_pairs_profile: wn / sn must hold [Bo,64] / [Bs] norms')
    scores = torch.empty((n, SHIFTS), dtype=torch.float32, device=ov.device) if want_scores else None
    dists = torch.empty((n, SHIFTS), dtype=torch.float32, device=ov.device) if want_distances else None
    if n:
        prof = ops._prof_begin()
        _lib.check(lib.witw_match_pairs_profile(ov.data_ptr(), su.data_ptr(), wn.data_ptr(), sn.data_ptr(), pair_o.data_ptr(),
                                                pair_s.data_ptr(), n, Bo, Bs, We, ops._p(scores), ops._p(dists), ops._stream()),
                   'witw_match_pairs_profile')
        if prof is not None:
            ops._prof_end(prof, ('match_pairs_profile', We), 2.0 * 64 * (64 * We) * n)
    return scores, dists


def profile_hypotheses(score_all, n_hyp, min_sep, shift_mask=None):
    """Ranked orientation hypotheses of profiles: score_all f32 [...,64] (match_profile's or match_pairs_profile's scores)
    -> shifts int64 [...,n_hyp]. Hypothesis 1 is the first maximum over the allowed shifts (match_fwd's orientation under the
    same shift_mask); hypothesis j + 1 the first maximum over the allowed shifts farther than min_sep shifts (circular) from
    every earlier one; -1 where none is left. 1 <= n_hyp <= 64, 0 <= min_sep <= 31.
    shift_mask: None, or a contiguous int64 tensor of n_words words on score_all's device; profile p (rows flattened) reads word
    p % n_words, so [Bs] words go with a dense [Bo,Bs,64] profile (the words of match_fwd), [n] words with a pair list's
    [n,64], and one word is shared by all. n_words must divide the number of profiles. A word of 0 allows all 64 shifts."""
    lib = _lib.load()
    sc = ops._dev_f32(score_all, 'score_all')
    if sc.dim() < 1 or sc.shape[-1] != SHIFTS:
        raise _lib.WitwError('profile_hypotheses: score_all must be [...,%d], got %s' % (SHIFTS, tuple(sc.shape)))
    n_hyp, min_sep = int(n_hyp), int(min_sep)
    if not 1 <= n_hyp <= SHIFTS:
        raise _lib.WitwError('profile_hypotheses: n_hyp=%d outside [1,%d]' % (n_hyp, SHIFTS))
    if not 0 <= min_sep <= 31:
        raise _lib.WitwError('profile_hypotheses: min_sep=%d outside [0,31]' % min_sep)
    n = sc.numel() // SHIFTS
    n_words = 0
    if shift_mask is not None:
        t = shift_mask
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.device == sc.device and t.dim() == 1
                and t.is_contiguous() and t.numel() >= 1):
            raise _lib.WitwError('profile_hypotheses: shift_mask must be a contiguous int64 [n_words] tensor on %s, got %s'
                                 % (sc.device, (tuple(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t)))
        n_words = int(t.numel())
        if n % n_words:
            raise _lib.WitwError('profile_hypotheses: %d mask words do not divide %d profiles' % (n_words, n))
    shifts = torch.empty(tuple(sc.shape[:-1]) + (n_hyp,), dtype=torch.int64, device=sc.device)
    if n:
        prof = ops._prof_begin()
        _lib.check(lib.witw_profile_hypotheses(sc.data_ptr(), n, ops._p(shift_mask), n_words, n_hyp, min_sep, shifts.data_ptr(),
                                               ops._stream()), 'witw_profile_hypotheses')
        if prof is not None:
            ops._prof_end(prof, ('profile_hypotheses', n_hyp), 0.0)
    return shifts
