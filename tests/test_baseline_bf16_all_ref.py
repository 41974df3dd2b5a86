"""CPU side of the 'bf16_all' cvig_baseline tests: tests/baseline_bf16_all_ref.py agrees with the reference of the 'bf16' forward where
the two coincide, its exact cases tell every wrong kernel it can name from the right one, and the parts of the third precision value
that need no GPU."""
import numpy as np
import pytest
import torch

from tests import baseline_bf16_all_ref as A
from tests import baseline_bf16_ref as R


def test_slices_are_even_contiguous_and_never_empty():
    assert A.slices(3, 2) == [(0, 2), (2, 3)] and A.slices(3, 3) == [(0, 1), (1, 2), (2, 3)] and A.slices(4, 1) == [(0, 4)]
    for nkc in (1, 2, 3, 7, 128):
        for S in range(1, nkc + 1):
            sl = A.slices(nkc, S)
            n = [b - a for a, b in sl]
            assert len(sl) == S and min(n) >= 1 and max(n) - min(n) <= 1 and sl[0][0] == 0 and sl[-1][1] == nkc
            assert all(sl[i][1] == sl[i + 1][0] for i in range(S - 1))


def test_one_slice_plain_batch_is_the_bf16_conv_reference():
    """S = 1, g = 1, valid = the map: conv + finish is baseline_bf16_ref.conv_taps4 before its space-to-depth store"""
    c = A.case('tile_k32')
    x, k3, bias, scale, shift = c.data()
    y = c.expected(1)
    s2d = R.conv_taps4(x, k3, bias, c.slope, scale, shift, c.valid, out_f32=True)
    assert np.array_equal(A.s2d_mosaic(y, 1, rounding=False), s2d)


@pytest.mark.parametrize('c,S', A.CASE_SPLITS, ids=A.CASE_SPLIT_IDS)
def test_exact_cases_are_exact_and_tell_wrong_kernels_apart(c, S):
    x, k3, bias, scale, shift = c.data()
    assert set(np.unique(x)) <= {-1., 0., 1.} and set(np.unique(k3)) <= {-1., 0., 1.}
    assert R.l1_bound(x, k3, bias) <= c.NZ + 2          # no partial sum of any order, of any slice, exceeds 8
    ws = c.partials(S)
    assert ws.shape == (S, c.Bm, c.g * c.h, c.g * c.w, c.Cout) and np.abs(ws).max() <= c.NZ
    want = c.expected(S)
    assert np.array_equal(R.bf16_round(want), want)
    assert np.array_equal(want, c.expected(1))           # exact: every slicing gives the same sum
    bits = R.f32_bits(want)
    applied = 0
    for v in A.CONV_VARIANTS:
        if not c.applies(v, S):
            continue
        applied += 1
        assert not np.array_equal(R.f32_bits(c.expected(S, v)), bits), (c.name, S, v)
    assert applied >= 3
    pre = A.finish(ws, bias, None, None, None, c.n_images, c.g, c.valid)
    assert (pre > 0).mean() >= 0.25 and (pre < 0).mean() >= 0.25, ((pre > 0).mean(), (pre < 0).mean())


def test_every_variant_applies_somewhere():
    for v in A.CONV_VARIANTS:
        assert any(c.applies(v, S) for c, S in A.CASE_SPLITS), v


def test_case_list_covers_what_it_names():
    by = {c.name: c for c in A.CASES}
    assert by['k48'].ksplits == (2, 3) and [b - a for a, b in A.slices(3, 2)] == [2, 1]
    g5 = by['mosaic_g5']
    assert (g5.Bm, g5.g * g5.h, g5.Bm * 25 - g5.n_images) == (2, 15, 23)
    assert by['mosaic_g2'].g * by['mosaic_g2'].h == 14 and by['mosaic_g2'].n_images == 7
    assert (by['ragged_17x18'].h, by['ragged_17x18'].w) == (17, 18)
    assert by['cout136'].Cout == 136 and by['cout12'].Cout % 8 == 4
    assert by['k64'].ksplits == (1, 2, 3, 4)
    x = g5.data()[0]
    assert not x[1, 3:, :].any() and not x[1, :3, 6:].any() and x[1, :3, :6].any()      # cells 25, 26 hold images, the rest is zero


@pytest.mark.parametrize('B,H,W,C,g', A.RELAYOUT_SHAPES)
def test_relayout_cases_tell_wrong_relayouts_apart(B, H, W, C, g):
    y = A.relayout_data(B, H, W, C)
    want = A.s2d_mosaic(y, g)
    assert want.shape == (-(-B // (g * g)), g * ((H + 1) // 2), g * ((W + 1) // 2), 4 * C)
    R.bf16_bits(want)
    for v in A.RELAYOUT_VARIANTS:
        if v == 'cell_swapped' and g == 1:
            continue
        assert not np.array_equal(A.s2d_mosaic(y, g, v), want), v
    # the data carries ties and both neighbours of ties
    lo = np.float32(y).view(np.uint32) & 0xffff
    assert (lo == 0x8000).any() and ((lo > 0) & (lo < 0x8000)).any() and (lo > 0x8000).any()
    # nearest-even is torch's conversion
    assert np.array_equal(R.bf16_round(y), torch.from_numpy(np.float32(y)).bfloat16().double().numpy())


def test_encoder_reference_differs_from_the_bf16_one_only_by_blocks_5_to_7():
    params = R.make_params(41)
    x = np.random.RandomState(1).randint(0, 256, size=(1, 3, 382, 382)).astype(np.float64)
    full, part, none = A.encoder_forward_all(x, params), R.encoder_forward(x, params), R.encoder_forward(x, params, rounding=False)
    n = np.linalg.norm(none)
    assert 1e-6 < np.linalg.norm(full - part) / n < 1e-2 and 1e-6 < np.linalg.norm(full - none) / n < 1e-2


def test_precision_argument():
    from witw_amd import _lib
    from witw_amd import cvig_baseline as cb
    assert cb.PRECISIONS == ('fp32', 'bf16', 'bf16_all') and cb.Globals.precision == 'fp32'
    assert cb.OverheadEncoder(precision='bf16_all').precision == 'bf16_all'
    for bad in ('bf16all', 'bf16_ALL', 'all', 'fp16'):
        with pytest.raises(_lib.WitwError, match="'fp32', 'bf16' or 'bf16_all'"):
            cb.SurfaceEncoder(precision=bad)
    with pytest.raises(_lib.WitwError):                  # the library's error, not an attribute error
        cb.SurfaceEncoder(precision='bf16_all').train()(torch.zeros((1, 3, 382, 382)))


def test_cli_precision_flag(monkeypatch):
    from witw_amd import cvig_baseline as cb
    calls = []
    monkeypatch.setattr(cb._fov, 'init_distributed', lambda: None)
    monkeypatch.setattr(cb, 'test', lambda **kw: calls.append(('test', kw)))
    monkeypatch.setattr(cb, 'train', lambda **kw: calls.append(('train', kw)))
    cb.main(['--mode', 'test', '--precision', 'bf16_all'])
    assert calls == [('test', dict(dataset='cvusa', match_method=None, precision='bf16_all'))]
    for argv in (['--mode', 'train', '--precision', 'bf16_all'], ['--precision', 'bf16_all']):
        with pytest.raises(SystemExit):
            cb.main(argv)
    assert len(calls) == 1
