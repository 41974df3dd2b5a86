"""Orientation profiles and ranked hypotheses, the CPU side: the numpy restatement of the hypothesis rule against hand cases,
refine_orientation, the degrees -> shifts conversion, and the refusals of the three C entries, the wrappers and heatmap.sweep --
all without a GPU. tests/test_match_profile_gpu.py holds the kernels against these restatements."""
import numpy as np
import pytest
import torch

from tests import match_profile_ref as P


def _word(*bits):
    w = np.uint64(0)
    for b in bits:
        w |= np.uint64(1) << np.uint64(b)
    return np.array([w], dtype=np.uint64)


# ----------------------------------------------------------------------------- the restatement of the hypothesis rule
def test_wraparound_suppression():
    """a winner at shift 63 with min_sep = 2 removes 61, 62, 63, 0, 1: the next best of those left is taken"""
    sc = np.zeros(64)
    sc[[63, 62, 61, 0, 1]] = [10, 9, 9, 9, 9]
    sc[[2, 60]] = [5, 4]
    assert P.hypotheses(sc, 3, 2).tolist() == [63, 2, 60]
    sc[[2, 60]] = [4, 4]                      # and of two equal ones the lower shift
    assert P.hypotheses(sc, 2, 2).tolist() == [63, 2]


def test_ties_resolve_to_the_lower_shift():
    sc = np.zeros(64)
    sc[[40, 8]] = 3.0
    assert P.hypotheses(sc, 2, 0).tolist() == [8, 40]
    assert P.hypotheses(np.zeros(64), 3, 0).tolist() == [0, 1, 2]
    assert P.hypotheses(np.zeros(64), 3, 4).tolist() == [0, 5, 10]


def test_one_bit_word_gives_one_hypothesis():
    g = np.random.Generator(np.random.Philox(key=[7, 1]))
    sc = g.standard_normal((5, 64))
    for k in (0, 17, 63):
        assert P.hypotheses(sc, 3, 4, _word(k)).tolist() == [[k, -1, -1]] * 5


def test_min_sep_31_yields_at_most_two():
    g = np.random.Generator(np.random.Philox(key=[7, 2]))
    sc = g.standard_normal((9, 64))
    h = P.hypotheses(sc, 4, 31)
    assert (h[:, 0] == sc.argmax(axis=1)).all()
    assert (h[:, 1] == (h[:, 0] + 32) % 64).all() and (h[:, 2:] == -1).all()


def test_word_0_is_all_ones_and_words_cycle():
    g = np.random.Generator(np.random.Philox(key=[7, 3]))
    sc = g.standard_normal((6, 64))
    assert np.array_equal(P.hypotheses(sc, 5, 3, np.zeros(1, np.uint64)), P.hypotheses(sc, 5, 3, np.array([P.ALL])))
    assert np.array_equal(P.hypotheses(sc, 5, 3, np.zeros(1, np.uint64)), P.hypotheses(sc, 5, 3, None))
    words = np.concatenate((_word(3, 4, 50), _word(63), np.zeros(1, np.uint64)))      # profile p reads word p % 3
    h = P.hypotheses(sc, 2, 0, words)
    assert set(h[0]) <= {3, 4, 50} and set(h[3]) <= {3, 4, 50} and h[1].tolist() == [63, -1] and h[4].tolist() == [63, -1]
    assert np.array_equal(h[[2, 5]], P.hypotheses(sc[[2, 5]], 2, 0))


def test_hypotheses_are_separated_allowed_and_ranked():
    g = np.random.Generator(np.random.Philox(key=[7, 4]))
    sc = g.standard_normal((40, 64))
    words = g.integers(1, 2 ** 63, size=40, dtype=np.uint64)
    ok = P.allowed_bits(words, 40)
    for min_sep in (0, 4, 31):
        h = P.hypotheses(sc, 64, min_sep, words)
        for p in range(40):
            got = h[p][h[p] >= 0]
            assert ok[p, got].all() and len(set(got)) == len(got)
            d = np.abs(got[:, None] - got[None, :])
            d = np.minimum(d, 64 - d) + 65 * np.eye(len(got), dtype=np.int64)
            assert d.min() > min_sep
            assert (np.diff(sc[p, got]) <= 0).all() or min_sep > 0      # without suppression the list is the sorted profile
            left = ok[p].copy()                      # nothing allowed is left un-suppressed when the list ends early
            for k in got:
                dd = np.abs(np.arange(64) - k)
                left &= np.minimum(dd, 64 - dd) > min_sep
            assert len(got) == 64 or not left.any()


def test_profile_dispatch_restated():
    assert P.dispatch(1, 1, 64) == P.dispatch(3, 200, 1) == P.dispatch(70, 5, 63) == 'match_kernel<1,1,false,true>'
    assert P.dispatch(100, 77, 33) == 'match_kernel<1,1,false,true>'
    assert P.dispatch(258, 129, 20) == P.dispatch(510, 129, 64) == P.dispatch(510, 129, 17) == 'match_kernel<1,2,false,true>'
    assert P.dispatch(1021, 129, 33) == P.dispatch(4096, 1, 12) == P.dispatch(4096, 128, 64) == 'match_kernel<2,2,false,true>'


# ----------------------------------------------------------------------------- refine_orientation
def _parabola(k, vertex_offset, curvature=-3.0, top=7.0):
    sc = np.full(64, -100.0)                      # sampled on the ring: positions k-1, k, k+1 (mod 64)
    for d in (-1, 0, 1):
        sc[(k + d) % 64] = top + curvature * (d - vertex_offset) ** 2
    return sc


def test_refine_recovers_an_exactly_sampled_parabola_and_wraps():
    from witw_amd import cvig_fov
    for k in (0, 20, 63):
        for off in (0.25, -0.25, 0.0, 0.5):
            sc = torch.from_numpy(_parabola(k, off)).reshape(1, 64)
            d = cvig_fov.refine_orientation(sc, torch.tensor([k]))
            assert d.dtype == torch.float64 and d.shape == (1,)
            assert abs(float(d[0]) - off) <= 1e-12, (k, off, float(d[0]))
    # fp32 scores are taken to float64 before anything is subtracted, and a listed shift [..., n] gives [..., n] offsets
    sc = torch.from_numpy(np.stack([_parabola(5, 0.25), _parabola(63, -0.125)])).float()
    d = cvig_fov.refine_orientation(sc, torch.tensor([[5, -1], [63, 63]]))
    assert d.shape == (2, 2) and abs(float(d[0, 0]) - 0.25) <= 1e-6 and float(d[0, 1]) == 0.0
    assert abs(float(d[1, 0]) + 0.125) <= 1e-6 and float(d[1, 1]) == float(d[1, 0])


def test_refine_is_zero_on_flat_nan_and_upward_triples_and_clamped():
    from witw_amd import cvig_fov
    flat = torch.zeros(1, 64, dtype=torch.float64)
    assert float(cvig_fov.refine_orientation(flat, torch.tensor([9]))[0]) == 0.0
    nan = torch.zeros(1, 64, dtype=torch.float64)
    nan[0, 10] = float('nan')
    for k in (9, 10, 11):
        assert float(cvig_fov.refine_orientation(nan, torch.tensor([k]))[0]) == 0.0
    inf = torch.zeros(1, 64, dtype=torch.float64)
    inf[0, 0] = float('inf')
    assert float(cvig_fov.refine_orientation(inf, torch.tensor([63]))[0]) == 0.0
    up = torch.from_numpy(_parabola(30, 0.25, curvature=2.0)).reshape(1, 64)           # denominator > 0: no maximum
    assert float(cvig_fov.refine_orientation(up, torch.tensor([30]))[0]) == 0.0
    far = torch.zeros(1, 64, dtype=torch.float64)                                       # vertex beyond the neighbour: clamped
    far[0, 29:32] = torch.tensor([0.0, 1.0, 1.9], dtype=torch.float64)
    assert float(cvig_fov.refine_orientation(far, torch.tensor([30]))[0]) == 0.5
    with pytest.raises(Exception, match='refine_orientation'):
        cvig_fov.refine_orientation(torch.zeros(2, 63), torch.tensor([0, 0]))
    with pytest.raises(Exception, match='refine_orientation'):
        cvig_fov.refine_orientation(torch.zeros(2, 64), torch.tensor([0, 0, 0]))


def test_min_separation_deg_to_shifts():
    from witw_amd import _lib, cvig_fov
    assert [cvig_fov.min_separation_shifts(d) for d in (0, 5.624, 5.625, 22.5)] == [0, 0, 1, 4]
    assert cvig_fov.min_separation_shifts(179.99) == 31
    for bad in (-1, 180, float('nan'), float('inf')):
        with pytest.raises(_lib.WitwError, match='min_separation_deg'):
            cvig_fov.min_separation_shifts(bad)


# ----------------------------------------------------------------------------- refusals without a GPU
def test_c_entries_refuse_bad_arguments_without_gpu():
    from witw_amd import _lib
    lib = _lib.load()
    err = lambda: lib.witw_last_error()
    # witw_match_profile(ov, su, Bo, Bs, We, score_all, distance_all, workspace, stream)
    assert lib.witw_match_profile(None, 1, 4, 4, 64, 1, 1, 1, None) == -1 and b'null' in err()
    assert lib.witw_match_profile(1, 1, 4, 4, 64, 1, 1, None, None) == -1 and b'null' in err()
    assert lib.witw_match_profile(1, 1, 4, 4, 64, None, None, 1, None) == -1 and b'no output' in err()
    assert lib.witw_match_profile(1, 1, 0, 4, 64, 1, 1, 1, None) == -1 and b'empty' in err()
    assert lib.witw_match_profile(1, 1, 4, 0, 64, 1, None, 1, None) == -1 and b'empty' in err()
    for we in (0, 65):
        assert lib.witw_match_profile(1, 1, 4, 4, we, 1, 1, 1, None) == -1 and b'width' in err()
    # witw_match_pairs_profile(ov, su, wn, sn, pair_o, pair_s, n_pairs, Bo, Bs, We, score_all, distance_all, stream)
    for hole in range(6):
        ptrs = [1] * 6
        ptrs[hole] = None
        assert lib.witw_match_pairs_profile(*ptrs, 3, 4, 4, 64, 1, 1, None) == -1 and b'null' in err()
    assert lib.witw_match_pairs_profile(1, 1, 1, 1, 1, 1, 3, 4, 4, 64, None, None, None) == -1 and b'no output' in err()
    assert lib.witw_match_pairs_profile(1, 1, 1, 1, 1, 1, 0, 4, 4, 64, 1, 1, None) == -1 and b'empty' in err()
    assert lib.witw_match_pairs_profile(1, 1, 1, 1, 1, 1, 3, 0, 4, 64, 1, 1, None) == -1 and b'empty' in err()
    for we in (0, 65):
        assert lib.witw_match_pairs_profile(1, 1, 1, 1, 1, 1, 3, 4, 4, we, 1, 1, None) == -1 and b'width' in err()
    # witw_profile_hypotheses(score_all, n_pairs, shift_mask, n_words, n_hyp, min_sep, shifts, stream)
    assert lib.witw_profile_hypotheses(None, 3, None, 0, 3, 4, 1, None) == -1 and b'null' in err()
    assert lib.witw_profile_hypotheses(1, 3, None, 0, 3, 4, None, None) == -1 and b'null' in err()
    assert lib.witw_profile_hypotheses(1, 0, None, 0, 3, 4, 1, None) == -1 and b'empty' in err()
    assert lib.witw_profile_hypotheses(1, 3, 1, 0, 3, 4, 1, None) == -1 and b'n_words' in err()
    for n_hyp in (0, 65):
        assert lib.witw_profile_hypotheses(1, 3, None, 0, n_hyp, 4, 1, None) == -1 and b'n_hyp' in err()
    for min_sep in (-1, 32):
        assert lib.witw_profile_hypotheses(1, 3, None, 0, 3, min_sep, 1, None) == -1 and b'min_sep' in err()
    with pytest.raises(_lib.WitwError, match='min_sep'):
        _lib.check(-1, 'witw_profile_hypotheses')


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from witw_amd import _lib, cvig_fov, match_profile
    ov, su = torch.zeros(2, 16, 4, 64), torch.zeros(3, 16, 4, 12)
    with pytest.raises(_lib.WitwError, match='CUDA'):
        match_profile.match_profile(ov, su)
    with pytest.raises(_lib.WitwError, match='CUDA'):
        match_profile.match_pairs_profile(ov, su, torch.zeros(128), torch.zeros(3), torch.zeros(2, dtype=torch.int32),
                                          torch.zeros(2, dtype=torch.int32))
    with pytest.raises(_lib.WitwError, match='CUDA'):
        match_profile.profile_hypotheses(torch.zeros(3, 64), 3, 4)
    with pytest.raises(_lib.WitwError, match='CUDA'):
        cvig_fov.orientation_profile(ov, su)
    with pytest.raises(_lib.WitwError, match='hypotheses'):
        cvig_fov.orientation_hypotheses(ov, su, n=0)
    with pytest.raises(_lib.WitwError, match='hypotheses'):
        cvig_fov.orientation_hypotheses(ov, su, n=65)
    with pytest.raises(_lib.WitwError, match='min_separation_deg'):
        cvig_fov.orientation_hypotheses(ov, su, min_separation_deg=180)
    with pytest.raises(_lib.WitwError, match='output_width_max'):
        cvig_fov.orientation_hypotheses(ov, su, output_width_max=65)
    with pytest.raises(_lib.WitwError, match='outside'):
        cvig_fov.orientation_profile(ov, su, pairs=(torch.tensor([0, 2]), torch.tensor([0, 1])))
    with pytest.raises(_lib.WitwError, match='outside'):
        cvig_fov.orientation_profile(ov, su, pairs=(torch.tensor([0, 1]), torch.tensor([-1, 1])))
    with pytest.raises(_lib.WitwError, match='pairs'):
        cvig_fov.orientation_profile(ov, su, pairs=(torch.tensor([0, 1]), torch.tensor([1])))
    with pytest.raises(_lib.WitwError, match='known_shift'):
        cvig_fov.sweep_scores(ov, su, known_shift=torch.zeros(3, dtype=torch.int64), hypotheses=2)
    with pytest.raises(_lib.WitwError, match='hypotheses'):
        cvig_fov.sweep_scores(ov, su, hypotheses=0)


def test_heatmap_sweep_refuses_bad_hypothesis_arguments(tmp_path):
    from witw_amd import heatmap
    args = (3, (0., 0., 100., 100.), 50., 50., 70, None, None, str(tmp_path / 'out.csv'))
    for bad in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match='hypotheses'):
            heatmap.sweep(*args, hypotheses=bad)
    for bad in (-1., 180.):
        with pytest.raises(ValueError, match='min_separation'):
            heatmap.sweep(*args, hypotheses=2, min_separation=bad)
    with pytest.raises(ValueError, match='trusted heading'):
        heatmap.sweep(*args, heading=90., heading_tolerance=0., hypotheses=2)
    assert heatmap.check_hypotheses(1, 22.5, (10., 0.)) == (1, 22.5)            # a trusted heading alone stays what it was
    assert heatmap.check_hypotheses(3, 10, (10., 15.)) == (3, 10.0)
    with pytest.raises(SystemExit):
        heatmap.main(['--heading', '90', '--heading-tolerance', '0', '--hypotheses', '2'])
    assert not (tmp_path / 'out.csv').exists()
