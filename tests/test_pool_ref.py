"""tests/pool_ref.py (the float64 reference of tests/test_pool_codes_gpu.py) against torch on the CPU: the convolution against the
oracle's, codes against F.max_pool2d(return_indices=True), the routed gradient against autograd of max_pool2d(relu(z)) at z, the
bit-level scatter against the routed gradient -- and, for EVERY case the GPU file runs, the conditions without which its exact
comparison would prove little: enough windows with a positive maximum (the others are gated by the ReLU and not compared), enough of
those with the maximum at two or more positions (the tie-break rule), and each of the four codes the answer often enough."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cvig_fov_oracle as O
from tests import pool_ref as R

SHAPES = [  # B, Cin, Cout, H, W
    (2, 3, 4, 6, 8),
    (2, 2, 3, 7, 9),          # odd H and W: a last row and column outside every window
    (1, 1, 2, 2, 2),          # one window
    (1, 2, 2, 3, 2),
    (2, 8, 5, 5, 11),
]


def _torch_side(z, gy):
    zt = torch.from_numpy(z.copy()).requires_grad_(True)
    pooled, idx = F.max_pool2d(torch.relu(zt), 2, 2, return_indices=True)
    pooled.backward(torch.from_numpy(gy.copy()))
    return pooled.detach().numpy(), idx.numpy(), zt.grad.numpy()


@pytest.mark.parametrize('circ', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_reference_equals_torch_on_the_cpu(shape, circ):
    B, Cin, Cout, H, W = shape
    x, w, b = R.exact_operands(H * 16 + W, B, Cin, Cout, H, W, px=0.5, terms=4.0)
    z = R.conv3x3_exact(x, w, b, circ)
    zo = O.conv3x3(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), 1, circ).numpy()
    assert z.dtype == np.float64 and np.array_equal(z, zo)
    pooled, code, m = R.pool_ref(z)
    gy = R.grad_ints(5, pooled.shape)
    dz = R.route_ref(z, gy)
    t_pooled, t_idx, t_dz = _torch_side(z, gy)
    assert pooled.shape == code.shape == m.shape == (B, Cout, H // 2, W // 2) and code.dtype == np.uint8
    assert np.array_equal(pooled, t_pooled) and not np.any(np.signbit(pooled))
    # torch's index is the flat position h * W + w of the first maximum of relu(z): the same position wherever the maximum is > 0
    hh, ww = np.meshgrid(np.arange(H // 2), np.arange(W // 2), indexing='ij')
    t_code = ((t_idx // W - 2 * hh) * 2 + (t_idx % W - 2 * ww)).astype(np.uint8)
    pos = m > 0
    assert np.array_equal(code[pos], t_code[pos])
    assert np.array_equal(dz, t_dz) and not np.any(np.signbit(dz) & (dz == 0))          # the zeros are +0.0
    if H % 2:
        assert np.all(dz[:, :, -1, :] == 0)
    if W % 2:
        assert np.all(dz[:, :, :, -1] == 0)
    # the scatter on bit patterns, given the gated gradient, is the routed gradient
    gated = np.where(pos, gy, 0.0).astype(np.float32).transpose(0, 2, 3, 1)
    bits = R.scatter_ref(np.ascontiguousarray(gated).view(np.int32), code.transpose(0, 2, 3, 1), H, W)
    assert np.array_equal(bits, np.ascontiguousarray(dz.astype(np.float32).transpose(0, 2, 3, 1)).view(np.int32))


def test_ties_take_the_first_position_in_scan_order():
    z = np.zeros((1, 1, 2, 8))
    z[0, 0, :, 0:2] = [[1, 1], [1, 1]]         # all four: (0,0)
    z[0, 0, :, 2:4] = [[0, 2], [2, 2]]         # (0,1) before (1,0) and (1,1)
    z[0, 0, :, 4:6] = [[-1, 0], [3, 3]]        # (1,0) before (1,1)
    z[0, 0, :, 6:8] = [[-3, -1], [-2, -1]]     # negative maximum: first of the two -1, gated
    pooled, code, m = R.pool_ref(z)
    assert code[0, 0, 0].tolist() == [0, 1, 2, 1] and m[0, 0, 0].tolist() == [1, 2, 3, -1] and pooled[0, 0, 0].tolist() == [1, 2, 3, 0]
    dz = R.route_ref(z, np.full((1, 1, 1, 4), 5.0))
    want = np.zeros_like(z)
    want[0, 0, 0, 0] = want[0, 0, 0, 3] = want[0, 0, 1, 4] = 5.0
    assert np.array_equal(dz, want)
    s = R.shares(z)
    assert s['positive'] == 0.75 and s['tied'] == 1.0 and s['codes'] == [1 / 3, 1 / 3, 1 / 3, 0.0]


def test_scatter_reference_moves_bits():
    dy = np.array([0x80000000, 0x7fc12345, 0x00000001, 0xff800000], dtype=np.uint32).reshape(1, 1, 2, 2)     # -0, NaN, subnormal, -inf
    code = np.array([[3, 0], [1, 2]], dtype=np.uint8).reshape(1, 1, 2, 2)
    out = R.scatter_ref(dy, code, 3, 5)
    assert out.shape == (1, 3, 5, 2) and out.dtype == np.uint32
    want = np.zeros((1, 3, 5, 2), dtype=np.uint32)
    want[0, 1, 1, 0], want[0, 0, 0, 1], want[0, 0, 3, 0], want[0, 1, 2, 1] = 0x80000000, 0x7fc12345, 0x00000001, 0xff800000
    assert np.array_equal(out, want)
    with pytest.raises(AssertionError):
        R.scatter_ref(dy, code, 1, 5)


def test_exactness_guard():
    x, w, b = R.exact_operands(3, 1, 8, 4, 4, 4)
    with pytest.raises(AssertionError):
        R.conv3x3_exact(x * 0.5, w, b, False)                         # not integers
    with pytest.raises(AssertionError):
        R.conv3x3_exact(np.ones((1, 8, 4, 4)), np.ones((4, 8, 3, 3)), b * 0 + 100, False)      # 72 + 100 > 128


CASES = R.all_cases()


@pytest.mark.parametrize('label', [c[0] for c in CASES])
def test_every_gpu_case_exercises_the_rule(label):
    """Conditions, not measurements: a case that misses one gets another sparsity or seed in tests/pool_ref.py, never a lower bar."""
    case = dict(CASES)[label]()
    assert float(np.abs(case.z).max()) <= R.MAX_ABS_Z
    s = R.shares(case.z)
    assert s['positive'] >= 0.30, s
    assert s['tied'] >= 0.10, s
    assert min(s['codes']) >= 0.05, s
    # the answers belong together, and the odd last row / column of the routed gradient is zero
    assert np.array_equal(case.dz, R.route_ref(case.z, case.gy)) and np.all(case.gy != 0)
    H, W = case.z.shape[2:]
    assert np.all(case.dz[:, :, 2 * (H // 2):, :] == 0) and np.all(case.dz[:, :, :, 2 * (W // 2):] == 0)
