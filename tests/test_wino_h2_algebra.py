"""Winograd F(2,3) along H (csrc/conv3x3.hip, conv_wino_h2) restated in numpy with the kernel's operation orders, no GPU:
the transforms are exact (small integers give the direct 3x3 conv bit for bit) and the fp32 form is at least as accurate as the
direct form's sequential fma chains, measured against fp64."""
import numpy as np
import pytest


def _filter_transform(g):
    """g [3 (kh), ...] -> U [4, ...]: U0 = g0, U1 = ((g0+g1)+g2)*0.5, U2 = ((g0-g1)+g2)*0.5, U3 = g2 (pack_weights_wino_kernel)"""
    g0, g1, g2 = g[0], g[1], g[2]
    h = g.dtype.type(0.5)
    return np.stack([g0, ((g0 + g1) + g2) * h, ((g0 - g1) + g2) * h, g2])


def _input_transform(d):
    """d [4 (rows), ...] -> V [4, ...]: V0 = d0-d2, V1 = d1+d2, V2 = d2-d1, V3 = d1-d3 (conv_wino_h2's transform)"""
    return np.stack([d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]])


def _chain(pairs, dtype):
    """sequential multiply-add chain acc = fma(a, b, acc) over the pairs in order; fp32 fma = fp64 product+sum rounded once"""
    acc = np.zeros(pairs[0][0].shape[:-1], dtype=dtype)
    for a, b in pairs:
        for k in range(a.shape[-1]):
            acc = (acc.astype(np.float64) + a[..., k].astype(np.float64) * b[..., k].astype(np.float64)).astype(dtype)
    return acc


def _direct(x, w, dtype):
    """x [4 rows, 3 cols(kw), N, Cin], w [3 kh, 3 kw, Cin] -> y [2, N]: K order chunk(8) -> tap -> channel"""
    cin = x.shape[-1]
    ys = []
    for r in range(2):
        pairs = []
        for c0 in range(0, cin, 8):
            for kh in range(3):
                for kw in range(3):
                    pairs.append((x[r + kh, kw, :, c0:c0 + 8], np.broadcast_to(w[kh, kw, c0:c0 + 8], x[0, 0, :, c0:c0 + 8].shape)))
        ys.append(_chain(pairs, dtype))
    return np.stack(ys)


def _wino(x, w, dtype):
    """same outputs through F(2,3)-H: m_t chains over chunk -> kw -> channel, then y0 = (m0+m1)+m2, y1 = (m1-m2)-m3"""
    cin = x.shape[-1]
    V = _input_transform(x.astype(dtype))            # [4, 3, N, Cin]
    U = _filter_transform(w.astype(dtype))           # [4, 3, Cin]
    m = []
    for t in range(4):
        pairs = []
        for c0 in range(0, cin, 8):
            for kw in range(3):
                pairs.append((V[t, kw, :, c0:c0 + 8], np.broadcast_to(U[t, kw, c0:c0 + 8], V[t, kw, :, c0:c0 + 8].shape)))
        m.append(_chain(pairs, dtype))
    m0, m1, m2, m3 = m
    return np.stack([(m0 + m1) + m2, (m1 - m2) - m3])


def test_exact_on_small_integers():
    rng = np.random.default_rng(0)
    cin, n = 16, 64
    x = rng.integers(-4, 5, size=(4, 3, n, cin)).astype(np.float32)
    w = rng.integers(-3, 4, size=(3, 3, cin)).astype(np.float32)
    exact = np.stack([sum(x[r + kh, kw] @ w[kh, kw] for kh in range(3) for kw in range(3)) for r in range(2)])
    assert np.array_equal(_direct(x, w, np.float32), exact)
    assert np.array_equal(_wino(x, w, np.float32), exact)


@pytest.mark.parametrize('cin', [64, 512])
def test_fp32_error_within_direct_order_error(cin):
    rng = np.random.default_rng(cin)
    n = 256
    x = np.maximum(rng.standard_normal((4, 3, n, cin)), 0).astype(np.float32)          # ReLU'd activations
    w = (rng.standard_normal((3, 3, cin)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)  # He-scaled filter
    exact = _direct(x.astype(np.float64), w.astype(np.float64), np.float64)
    scale = np.abs(exact).max()
    e_dir = np.abs(_direct(x, w, np.float32) - exact)
    e_win = np.abs(_wino(x, w, np.float32) - exact)
    assert e_win.max() <= 1.5 * e_dir.max(), (e_win.max() / scale, e_dir.max() / scale)
    assert np.sqrt((e_win ** 2).mean()) <= 1.5 * np.sqrt((e_dir ** 2).mean())
    assert e_win.max() <= 3e-5 * scale
