"""tests/wgrad_ref.py (the float64 weight-gradient reference of the GPU edge tests) against float64 autograd through the
oracle's convolution, on shapes small enough to enumerate: both paddings, both strides, a single column, a single row, two rows
under stride (2,1) (one output row) and an odd height under stride (2,1). The oracle's circular padding accepts W = 1 (the one
column is its own left and right neighbour), so W = 1 stays in the circular cases here and in tests/test_wgrad_edges_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import cvig_fov_oracle as O
from tests import wgrad_ref as R

SHAPES = [  # B, Cin, Cout, H, W, stride_h
    (2, 3, 4, 5, 6, 1),
    (2, 3, 4, 4, 6, 2),
    (1, 2, 3, 4, 1, 1),        # W = 1
    (2, 2, 3, 1, 5, 1),        # H = 1
    (1, 1, 1, 1, 1, 1),
    (2, 3, 2, 2, 4, 2),        # H = 2 under stride 2: one output row
    (2, 3, 2, 1, 4, 2),
    (1, 2, 3, 7, 3, 2),        # odd H under stride 2
]


def _operands(seed, B, Cin, Cout, H, W, sh):
    g = np.random.Generator(np.random.Philox(key=[seed, 31]))
    Ho = (H - 1) // sh + 1
    return torch.from_numpy(g.standard_normal((B, Cin, H, W))), torch.from_numpy(g.standard_normal((B, Cout, Ho, W)))


def _autograd(x, dz, sh, circ):
    Cout, Cin = dz.shape[1], x.shape[1]
    w = torch.zeros((Cout, Cin, 3, 3), dtype=x.dtype, requires_grad=True)
    b = torch.zeros((Cout,), dtype=x.dtype, requires_grad=True)
    y = O.conv3x3(x, w, b, sh, circ)
    assert y.shape == dz.shape
    y.backward(dz)
    return w.grad, b.grad


@pytest.mark.parametrize('circ', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_reference_equals_float64_autograd(shape, circ):
    B, Cin, Cout, H, W, sh = shape
    x, dz = _operands(H * 16 + W, *shape)
    dw_a, db_a = _autograd(x, dz, sh, circ)
    dw, db = R.wgrad_ref(x, dz, sh, circ)
    sw, sb = R.wgrad_scale(x, dz, sh, circ)
    assert dw.dtype == np.float64 and dw.shape == (Cout, Cin, 3, 3) and db.shape == (Cout,)
    assert np.all(sw >= np.abs(dw)) and np.all(sb >= np.abs(db))
    assert R.err(dw_a, dw, sw) <= 1e-12
    assert R.err(db_a, db, sb) <= 1e-12
    # taps that only ever see padding have scale 0 (and err() has just held autograd to an exact 0 there)
    if H == 1:
        assert np.all(sw[:, :, 0, :] == 0) and np.all(sw[:, :, 2, :] == 0)
    if W == 1 and not circ:
        assert np.all(sw[:, :, :, 0] == 0) and np.all(sw[:, :, :, 2] == 0)
    if W == 1 and circ and H > 1:
        assert np.all(sw[:, :, 1, 0] > 0)          # the wrapped column is real data


def test_taps4_is_the_full_form_where_the_first_tap_row_and_column_get_no_gradient():
    """dZ is non-zero at output pixel (0, 0) only: under zero padding the taps kh = 0 / kw = 0 then multiply it by the padding
    row / column alone, so the full form's first tap row and column are exact zeros and the 2x2 sub-window form must equal it."""
    x, dz = _operands(7, 3, 5, 4, 6, 7, 1)
    keep = torch.zeros_like(dz)
    keep[:, :, 0, 0] = dz[:, :, 0, 0]
    full_w, full_b = R.wgrad_ref(x, keep, 1, False)
    t4_w, t4_b = R.wgrad_ref(x, keep, 1, False, taps4=True)
    assert np.all(full_w[:, :, 0, :] == 0) and np.all(full_w[:, :, :, 0] == 0) and np.any(full_w[:, :, 1:, 1:] != 0)
    assert np.array_equal(full_w, t4_w) and np.array_equal(full_b, t4_b)
    # on ordinary operands: the live taps of the full form, exact zeros elsewhere; the scale says the same
    full_w, _ = R.wgrad_ref(x, dz, 1, False)
    t4_w, _ = R.wgrad_ref(x, dz, 1, False, taps4=True)
    t4_s, _ = R.wgrad_scale(x, dz, 1, False, taps4=True)
    assert np.array_equal(t4_w[:, :, 1:, 1:], full_w[:, :, 1:, 1:])
    for t in (t4_w, t4_s):
        assert np.all(t[:, :, 0, :] == 0) and np.all(t[:, :, :, 0] == 0)
    assert np.all(t4_s[:, :, 1:, 1:] > 0)


def test_err_measure():
    ref = np.array([1.0, -2.0, 0.0])
    scale = np.array([4.0, 2.0, 0.0])
    assert R.err(np.array([1.0, -2.0, 0.0]), ref, scale) == 0.0
    assert R.err(np.array([1.5, -2.0, 0.0]), ref, scale) == 0.125
    with pytest.raises(AssertionError):
        R.err(np.array([1.0, -2.0, 1e-30]), ref, scale)          # scale 0: an exact zero or nothing
    with pytest.raises(AssertionError):
        R.err(np.array([1.0, float('nan'), 0.0]), ref, scale)
    with pytest.raises(ValueError):
        R.wgrad_ref(np.zeros((1, 1, 4, 4)), np.zeros((1, 1, 4, 4)), 2, False)      # stride 2 halves the rows
