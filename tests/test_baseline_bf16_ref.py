"""CPU side of the bf16 cvig_baseline tests: tests/baseline_bf16_ref.py is the oracle's encoder when its rounding is switched off, its
exact cases tell every wrong kernel it can name from the right one, and the parts of the precision switch that need no GPU."""
import numpy as np
import pytest
import torch

from oracle import cvig_baseline_oracle as OB
from tests import baseline_bf16_ref as R


def test_reference_without_rounding_is_the_oracle():
    params = R.make_params(41)
    x = np.random.RandomState(1).randint(0, 256, size=(1, 3, 382, 382)).astype(np.float64)
    want = OB.encoder_forward(torch.from_numpy(x), [{k: torch.from_numpy(v).double() for k, v in q.items()} for q in params]).numpy()
    got = R.encoder_forward(x, params, rounding=False)
    assert got.shape == (1, 1536)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-14)
    rounded = R.encoder_forward(x, params)
    dev = np.linalg.norm(rounded - want) / np.linalg.norm(want)
    assert 1e-6 < dev < 1e-2, dev          # the rounding is there, and small


def test_bf16_rounding_helpers():
    t = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -16, 3.0, 0.0, 2.0 ** -20 * (1 + 2.0 ** -8)])
    assert np.array_equal(R.bf16_round(t), [1., 1 + 2.0 ** -6, -1., 1 + 2.0 ** -7, 3., 0., 2.0 ** -20])
    assert np.array_equal(R.bf16_round(t), torch.from_numpy(t).float().bfloat16().double().numpy())
    assert np.array_equal(R.bf16_half_up(t)[:3], [1 + 2.0 ** -7, 1 + 2.0 ** -6, -(1 + 2.0 ** -7)])
    assert np.array_equal(R.bf16_trunc(t)[:4], [1., 1 + 2.0 ** -7, -1., 1.])
    r = np.random.RandomState(0).normal(size=4096) * 10.0 ** np.random.RandomState(1).randint(-6, 6, size=4096)
    assert np.array_equal(R.bf16_round(np.float32(r).astype(np.float64)), torch.from_numpy(np.float32(r)).bfloat16().double().numpy())


@pytest.mark.parametrize('c', R.CASES, ids=[c.name for c in R.CASES])
def test_exact_cases_are_exact_and_tell_wrong_kernels_apart(c):
    x, k3, bias, scale, shift = c.data()
    assert R.l1_bound(x, k3, bias) <= c.NZ + 2
    want = c.expected()
    assert np.array_equal(R.bf16_round(want), want)
    bits = R.out_bits(want, c.out_f32)
    applied = 0
    for v in R.VARIANTS:
        if not c.applies(v):
            continue
        applied += 1
        assert not np.array_equal(R.out_bits(c.expected(v), c.out_f32), bits), (c.name, v)
    assert applied >= 6
    pre = R.preact(x, k3, bias)[:, :c.valid[0], :c.valid[1]]
    assert (pre > 0).mean() >= 0.25 and (pre < 0).mean() >= 0.25


def test_every_variant_applies_somewhere():
    for v in R.VARIANTS:
        if v not in ('double_round', 'trunc_filters'):
            assert any(c.applies(v) for c in R.CASES), v


def test_rounding_case_tells_the_rounding_variants():
    x, k3, bias, scale, shift, slope, valid = R.rounding_case()
    want = R.conv_taps4(x, k3, bias, slope, scale, shift, valid)
    for v in ('double_round', 'trunc_filters'):
        assert not np.array_equal(R.conv_taps4(x, k3, bias, slope, scale, shift, valid, False, v), want), v
    assert not np.array_equal(R.pack_taps4(k3, 'trunc_filters'), R.pack_taps4(k3))
    # the fp32 store keeps what bf16 would round: the case separates the two output modes
    assert not np.array_equal(R.conv_taps4(x, k3, bias, slope, scale, shift, valid, True), want)


def test_precision_argument():
    from witw_amd import _lib
    from witw_amd import cvig_baseline as cb
    assert cb.Globals.precision == 'fp32' and cb.SurfaceEncoder().precision == 'fp32'
    assert cb.OverheadEncoder(precision='bf16').precision == 'bf16'
    for bad in ('fp16', 'BF16', 16, ''):
        with pytest.raises(_lib.WitwError, match='precision'):
            cb.SurfaceEncoder(precision=bad)
    old = cb.Globals.precision
    try:
        cb.Globals.precision = 'bf16'
        assert cb.SurfaceEncoder().precision == 'bf16' and cb.SurfaceEncoder(precision='fp32').precision == 'fp32'
    finally:
        cb.Globals.precision = old
    with pytest.raises(_lib.WitwError):                  # the library's error, not an attribute error
        cb.SurfaceEncoder(precision='bf16').train()(torch.zeros((1, 3, 382, 382)))


def test_cli_precision_flag(monkeypatch):
    from witw_amd import cvig_baseline as cb
    calls = []
    monkeypatch.setattr(cb._fov, 'init_distributed', lambda: None)
    monkeypatch.setattr(cb, 'test', lambda **kw: calls.append(('test', kw)))
    monkeypatch.setattr(cb, 'train', lambda **kw: calls.append(('train', kw)))
    cb.main(['--mode', 'test', '--precision', 'bf16'])
    cb.main(['--mode', 'test'])
    cb.main(['--mode', 'train'])
    assert calls[0] == ('test', dict(dataset='cvusa', match_method=None, precision='bf16'))
    assert calls[1][1]['precision'] == 'fp32' and calls[2][0] == 'train' and 'precision' not in calls[2][1]
    for argv in (['--mode', 'train', '--precision', 'bf16'], ['--precision', 'bf16'], ['--mode', 'test', '--precision', 'fp16']):
        with pytest.raises(SystemExit):
            cb.main(argv)
    assert len(calls) == 3
