"""CPU: tests/baseline_bf16_train_ref.py (the float64 restatement the GPU tests of train_precision='bf16' compare with) held against
torch float64 autograd of Conv2d(k=4, s=2) -> LeakyReLU -> BatchNorm2d(train) with the three roundings inserted as straight-through
casts; and the public surface of the knob that needs no GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import baseline_bf16_ref as R0
from tests import baseline_bf16_train_ref as R


def _block_inputs(seed, B, vp, cp, co):
    r = np.random.RandomState(seed)
    f = lambda a: a.astype(np.float32).astype(np.float64)
    a_prev = np.zeros((B, vp[0] + 1, vp[1] + 2, cp))                 # a padded map: garbage outside the valid region must not matter
    a_prev[:] = 7.
    a_prev[:, :vp[0], :vp[1]] = f(r.normal(0., 1., (B, vp[0], vp[1], cp)))
    scale, shift = f(r.normal(1., 0.2, cp)), f(r.normal(0., 0.5, cp))
    w, b = f(r.normal(0., 0.1, (co, cp, 4, 4))), f(r.normal(0., 0.1, co))
    gamma, beta = f(r.normal(1., 0.1, co)), f(r.normal(0., 0.1, co))
    vh, vw = (vp[0] - 4) // 2 + 1, (vp[1] - 4) // 2 + 1
    dy = f(r.normal(0., 1., (B, vh, vw, co)))
    return a_prev, scale, shift, w, b, gamma, beta, dy


@pytest.mark.parametrize('rounding', [True, False])
@pytest.mark.parametrize('vp', [(10, 12), (11, 9), (4, 5)])          # even and odd valid sides; one output row
def test_block_step_equals_autograd_with_straight_through_casts(vp, rounding):
    B, cp, co = 2, 4, 8
    a_prev, scale, shift, w, b, gamma, beta, dy = _block_inputs(sum(vp), B, vp, cp, co)
    got = R.block_step(a_prev, vp, scale, shift, w, b, gamma, beta, dy, rounding=rounding)
    rf, rb = R._ste()
    ident = lambda t: t
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    ap = t(a_prev[:, :vp[0], :vp[1]].transpose(0, 3, 1, 2))
    tw, tb, tg, tbe = t(w), t(b), t(gamma), t(beta)
    xin = ap * torch.as_tensor(scale)[None, :, None, None] + torch.as_tensor(shift)[None, :, None, None]
    xin = (rf if rounding else ident)(xin)
    xin.retain_grad()
    z = F.conv2d(xin, (rf if rounding else ident)(tw), tb, stride=2)
    z = (rb if rounding else ident)(z)
    y = F.batch_norm(F.leaky_relu(z, 0.2), None, None, tg, tbe, True, 0.1, 1e-5)
    (y * torch.as_tensor(dy.transpose(0, 3, 1, 2))).sum().backward()
    np.testing.assert_allclose(got['y'], y.detach().numpy().transpose(0, 2, 3, 1), rtol=0, atol=1e-12)
    for k, ref in (('dw', tw.grad), ('db', tb.grad), ('dgamma', tg.grad), ('dbeta', tbe.grad)):
        np.testing.assert_allclose(got[k], ref.numpy(), rtol=0, atol=1e-11 * max(1., float(ref.abs().max())), err_msg=k)
    dx = R.depth_to_space2(got['dh'], cp, vp).transpose(0, 3, 1, 2)       # the gradient at the rounded input, back in image layout
    np.testing.assert_allclose(dx, xin.grad.numpy(), rtol=0, atol=1e-11)
    vh, vw = (vp[0] - 4) // 2 + 1, (vp[1] - 4) // 2 + 1
    assert not got['a'][:, vh:].any() and not got['a'][:, :, vw:].any() and not got['dz'][:, vh:].any()
    if rounding:      # rounded where it says, and only there
        for k in ('h', 'dz'):
            assert np.array_equal(R0.bf16_round(got[k]), got[k]), k
        assert not np.array_equal(R0.bf16_round(got['a']), got['a'])
        plain = R.block_step(a_prev, vp, scale, shift, w, b, gamma, beta, dy, rounding=False)
        assert 1e-5 < np.abs(plain['dw'] - got['dw']).max() / np.abs(plain['dw']).max() < 5e-2


def test_filters_and_relayouts():
    r = np.random.RandomState(1)
    k3 = r.normal(0., 1., (5, 7, 3, 3))
    wf, wt = R.fwd_filter(k3, rounding=False), R.dgrad_filter(k3, rounding=False)
    assert wf.shape == (5, 7, 2, 2) and wt.shape == (7, 5, 2, 2)
    for ty in range(2):
        for tx in range(2):
            assert np.array_equal(wf[:, :, ty, tx], k3[:, :, 1 + ty, 1 + tx])
            assert np.array_equal(wt[:, :, ty, tx], k3[:, :, 2 - ty, 2 - tx].T)
    assert np.array_equal(R.fwd_filter(k3), R0.bf16_round(wf)) and np.array_equal(R.fwd_filter(k3), R0.taps4_filter(k3))
    # the data gradient is the adjoint of the forward: <conv(x), g> == <x, conv_t(g)>
    x, g = r.normal(0., 1., (2, 5, 6, 7)), r.normal(0., 1., (2, 5, 6, 5))
    lhs = (R.conv_plain(x, wf, None, 1) * g).sum()
    rhs = (x * R.conv_plain(g, wt, None, 0)).sum()
    assert abs(lhs - rhs) <= 1e-10 * abs(lhs)
    # ... and the weight gradient its derivative in the filter
    dk3, db = R.wgrad_taps4(x, g)
    assert abs((dk3 * k3).sum() - lhs) <= 1e-10 * abs(lhs) and np.allclose(db, g.sum((0, 1, 2)))
    assert not dk3[:, :, 0].any() and not dk3[:, :, :, 0].any()
    w = r.normal(0., 1., (3, 2, 4, 4))
    assert np.array_equal(R.k3_to_conv4x4(R.conv4x4_to_k3(w), 2), w)
    a = r.normal(0., 1., (1, 5, 7, 2))
    s = R.space_to_depth2(a, (5, 6), np.ones(2), np.full(2, 3.), rounding=False)
    assert s.shape == (1, 3, 3, 8) and s[0, 0, 0, 2] == a[0, 0, 1, 0] + 3. and not s[0, 2, :, 4:].any()      # row 5 does not exist: +0, no shift
    assert np.array_equal(R.depth_to_space2(R.space_to_depth2(a, (5, 7), rounding=False), 2, (5, 7)), a)


def test_encoder_step_rounds_blocks_2_to_4_only():
    """the torch form of the whole step on a 382-pixel image would take a while on the CPU: a cut-down stack shows which blocks round"""
    rf, rb = R._ste()
    t = torch.tensor(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 0.3]), requires_grad=True)
    y = rb(rf(t) * 3.)
    y.backward(torch.tensor([1 + 2.0 ** -8, 1., 1.]))
    assert np.array_equal(rf(t).detach().numpy(), R0.bf16_round(t.detach().numpy()))
    assert np.array_equal(t.grad.numpy(), 3. * R0.bf16_round(np.array([1 + 2.0 ** -8, 1., 1.])))


# ----------------------------------------------------------------------------- surface (no GPU)
def test_knob_values_and_defaults():
    from witw_amd import _lib
    from witw_amd import cvig_baseline as cb
    assert cb.Globals.train_precision == 'fp32' and cb.TRAIN_PRECISIONS == ('fp32', 'bf16')
    assert cb.SurfaceEncoder().train_precision == 'fp32' and cb.OverheadEncoder(train_precision='bf16').train_precision == 'bf16'
    old = cb.Globals.train_precision
    try:
        cb.Globals.train_precision = 'bf16'
        assert cb.SurfaceEncoder().train_precision == 'bf16' and cb.SurfaceEncoder(train_precision='fp32').train_precision == 'fp32'
    finally:
        cb.Globals.train_precision = old
    for bad in ('fp16', 'bf16_all', '', 16):
        with pytest.raises(_lib.WitwError):
            cb.SurfaceEncoder(train_precision=bad)
        with pytest.raises(_lib.WitwError):
            cb.train(train_precision=bad)
    assert sorted(cb.SurfaceEncoder(train_precision='bf16').state_dict()) == sorted(cb.SurfaceEncoder().state_dict())


def test_cli_train_precision(monkeypatch):
    from witw_amd import cvig_baseline as cb
    calls = []
    monkeypatch.setattr(cb, 'train', lambda **kw: calls.append(('train', kw)))
    monkeypatch.setattr(cb, 'test', lambda **kw: calls.append(('test', kw)))
    monkeypatch.setattr(cb._fov, 'init_distributed', lambda: None)
    cb.main(['--mode', 'train', '--train-precision', 'bf16'])
    cb.main(['--mode', 'train', '--train-precision', 'fp32', '--loss', 'batch_hard'])
    cb.main(['--mode', 'train'])
    cb.main(['--mode', 'test'])
    assert calls[0] == ('train', {'dataset': 'cvusa', 'loss': 'exhaustive', 'train_precision': 'bf16'})
    assert calls[1] == ('train', {'dataset': 'cvusa', 'loss': 'batch_hard', 'train_precision': 'fp32'})
    assert calls[2] == ('train', {'dataset': 'cvusa', 'loss': 'exhaustive'})          # the keyword only when the flag was given
    assert calls[3][0] == 'test' and 'train_precision' not in calls[3][1]
    for argv in (['--mode', 'test', '--train-precision', 'bf16'], ['--mode', 'test', '--train-precision', 'fp32'],
                 ['--mode', 'train', '--train-precision', 'bf16_all'], ['--mode', 'train', '--precision', 'bf16', '--train-precision', 'bf16']):
        with pytest.raises(SystemExit):
            cb.main(argv)
    assert len(calls) == 4
