"""Known-orientation matching without a GPU: orientation_shift against orientation_mask(c, 0), the refusals of the `known_shift=`
keyword, and the host algebra of cvig_fov.sharded_match_loss(..., known_shift=) for both losses -- a CPU op set whose
match_fwd_fixed takes the given shift (float64 distance of tests/test_batch_hard.py at that orientation) on the in-process
threaded group: 2 ranks must give the one-rank loss and gradients."""
import numpy as np
import pytest
import torch

from witw_amd import _lib, cvig_fov, synth

from .test_batch_hard import BatchHardCpuKernels, dist64
from .threaded_world import run_ranks


def _as_u64(t):
    return t.numpy().view(np.uint64)


@pytest.mark.parametrize('width', [64, 48, 7, 1])
def test_orientation_shift_is_the_one_bit_mask(width):
    step = 360. / width
    centres = np.concatenate([np.linspace(-540., 540., 433), [-180., 180., 179.999, -179.999, 0.],
                              np.arange(width) * step - 180. + step / 2.,            # half-way between two shifts: the lower one
                              np.arange(width) * step - 180.])
    sh = cvig_fov.orientation_shift(centres, width)
    assert sh.dtype == torch.int64 and tuple(sh.shape) == (len(centres),)
    assert int(sh.min()) >= 0 and int(sh.max()) < width
    words = _as_u64(cvig_fov.orientation_mask(centres, 0, width))
    assert np.array_equal(np.uint64(1) << sh.numpy().astype(np.uint64), words)
    one = cvig_fov.orientation_shift(-180., width)
    assert tuple(one.shape) == (1,) and int(one) == 0
    if width == 64:
        assert int(cvig_fov.orientation_shift(180.)) == 0 and int(cvig_fov.orientation_shift(0.)) == 32
        assert int(cvig_fov.orientation_shift(-180. + 360. / 64 / 2)) == 0          # equally near 0 and 1: the lower
    with pytest.raises(_lib.WitwError):
        cvig_fov.orientation_shift(0., 65)


def _emb(bo=3, bs=4, we=8):
    return torch.from_numpy(synth.embeddings(5, 1, (bo, 16, 4, 64))), torch.from_numpy(synth.embeddings(5, 2, (bs, 16, 4, we)))


def test_known_shift_excludes_shift_mask():
    ov, su = _emb()
    sh, m = torch.zeros(4, dtype=torch.int64), torch.ones(4, dtype=torch.int64)
    for call in (lambda: cvig_fov.match(ov, su, shift_mask=m, known_shift=sh),
                 lambda: cvig_fov.correlation(ov, su, shift_mask=m, known_shift=sh),
                 lambda: cvig_fov.ranks(ov, su, shift_mask=m, known_shift=sh),
                 lambda: cvig_fov.sharded_ranks(ov, su, 0, shift_mask=m, known_shift=sh),
                 lambda: cvig_fov.evaluation_ranks(ov, su, shift_mask=m, known_shift=sh),
                 lambda: cvig_fov.retrieve(ov, su, k=2, shift_mask=m, known_shift=sh),
                 lambda: cvig_fov.retrieve_topk(ov, su, k=2, shift_mask=m, known_shift=sh),
                 lambda: cvig_fov.sweep_scores(ov, su, shift_mask=m, known_shift=sh)):
        with pytest.raises(_lib.WitwError, match='mutually exclusive'):
            call()
    with pytest.raises(_lib.WitwError, match='one shift per query'):
        cvig_fov.match(ov, su, known_shift=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(_lib.WitwError):           # no CPU fall-back: the fixed forward wants device tensors
        cvig_fov.match(ov, su, known_shift=sh)


@pytest.mark.parametrize('method', ['dft', 'dft_masked'])
def test_known_shift_is_refused_by_the_spectral_methods(method):
    ov, su = _emb()
    sh = torch.zeros(4, dtype=torch.int64)
    for call in (lambda: cvig_fov.retrieve(ov, su, k=2, method=method, known_shift=sh),
                 lambda: cvig_fov.retrieve_topk(ov, su, k=2, method=method, known_shift=sh),
                 lambda: cvig_fov.evaluation_ranks(ov, su, method=method, known_shift=sh)):
        with pytest.raises(_lib.WitwError, match="'fixed'"):
            call()


def test_method_fixed_requires_known_shift():
    ov, su = _emb()
    for call in (lambda: cvig_fov.retrieve(ov, su, k=2, method='fixed'),
                 lambda: cvig_fov.retrieve_topk(ov, su, k=2, method='fixed'),
                 lambda: cvig_fov.evaluation_ranks(ov, su, method='fixed')):
        with pytest.raises(_lib.WitwError, match='requires known_shift'):
            call()


def test_cli_exclusions():
    for argv in (['--mode', 'test', '--known-orientation', '0', '--orientation-window', '0,0'],
                 ['--mode', 'test', '--match-method', 'fixed']):
        with pytest.raises(SystemExit):
            cvig_fov.main(argv)


# ----------------------------------------------------------------------------- the sharded algebra under known shifts
class FixedCpuKernels(BatchHardCpuKernels):
    """BatchHardCpuKernels with the fixed forward: the orientation is the given shift & 63 broadcast over the overheads, the
    distance the float64 one at that orientation; match_bwd differentiates that distance at the saved orientation. match_fwd
    must not be reached when known_shift is given."""

    @staticmethod
    def match_fwd(*a, **k):
        raise AssertionError('sharded_match_loss(known_shift=) called match_fwd')

    @staticmethod
    def match_fwd_fixed(ov, su, shift, want_score=False, want_workspace=False, want_orientation=True):
        with torch.no_grad():
            ori = (shift & 63)[None, :].expand(ov.shape[0], -1).contiguous()
            d = dist64(ov.double(), su.double(), ori).float()
        if want_workspace:
            return ori, d, torch.zeros(1), torch.zeros(1)
        return ori, d

    @staticmethod
    def match_bwd(ov, su, ori, score, ws, g_dist, need_ov=True, need_su=True):
        with torch.enable_grad():
            ov64 = ov.detach().double().requires_grad_(True)
            su64 = su.detach().double().requires_grad_(True)
            dist64(ov64, su64, ori).backward(g_dist.double())
        return ov64.grad.float(), su64.grad.float()

    # the soft-margin slab formulas of CpuKernels in float64, rounded once: the sums over a slab and the cancellation on the
    # diagonal then do not depend on how the columns are sharded beyond fp32 rounding of the results
    @staticmethod
    def triplet_loss_slab_fwd(dist, diag, col0, alpha):
        return BatchHardCpuKernels.triplet_loss_slab_fwd(dist.double(), diag.double(), col0, alpha)

    @staticmethod
    def triplet_loss_slab_sig(dist, diag, col0, alpha):
        return BatchHardCpuKernels.triplet_loss_slab_sig(dist.double(), diag.double(), col0, alpha)

    @staticmethod
    def triplet_loss_slab_bwd(dist, diag, rowsig, colsig, g_loss, col0, alpha):
        return BatchHardCpuKernels.triplet_loss_slab_bwd(dist.double(), diag.double(), rowsig, colsig, g_loss.double(), col0, alpha)


FX_B, FX_b, FX_WE = 12, 6, 8


def _fixed_inputs():
    ov = torch.from_numpy(synth.embeddings(11, 1, (FX_B, 16, 4, 64)))
    shift = (7 * torch.arange(FX_B) + 3) % 64
    shift[0], shift[1] = 0, 63
    col = (torch.arange(FX_WE)[None, :] + shift[:, None]) % 64
    su = torch.gather(ov, 3, col[:, None, None, :].expand(-1, 16, 4, -1)) + \
        2.0 * torch.from_numpy(synth.embeddings(11, 2, (FX_B, 16, 4, FX_WE)))
    return ov.contiguous(), su.contiguous(), shift + 64 * (torch.arange(FX_B) % 3)      # & 63 is part of the contract


def _loss_rank(ov, su, shift, rank, b, loss):
    sl = slice(rank * b, (rank + 1) * b)
    ov_l, su_l = ov[sl].clone().requires_grad_(True), su[sl].clone().requires_grad_(True)
    out = cvig_fov.sharded_match_loss(ov_l, su_l, loss=loss, _kernels=FixedCpuKernels, known_shift=shift[sl].clone())
    assert torch.equal(out[1], (shift[sl] & 63)[None, :].expand(ov.shape[0], -1))
    out[0].backward()
    return out[0].item(), ov_l.grad.clone(), su_l.grad.clone()


@pytest.mark.parametrize('loss', ['soft_margin', 'batch_hard'])
def test_sharded_loss_with_known_shift_two_ranks_equal_one(loss):
    ov, su, shift = _fixed_inputs()
    one = run_ranks(1, lambda r: _loss_rank(ov, su, shift, r, FX_B, loss))[0]
    two = run_ranks(2, lambda r: _loss_rank(ov, su, shift, r, FX_b, loss))
    assert np.isfinite(one[0]) and float(one[1].abs().max()) > 0
    for rank, (l, g_ov, g_su) in enumerate(two):
        sl = slice(rank * FX_b, (rank + 1) * FX_b)
        assert abs(l - one[0]) <= 1e-6 * abs(one[0]), (rank, l, one[0])
        np.testing.assert_allclose(g_ov.numpy(), one[1][sl].numpy(), rtol=0, atol=2e-6 * float(one[1].abs().max()))
        np.testing.assert_allclose(g_su.numpy(), one[2][sl].numpy(), rtol=0, atol=2e-6 * float(one[2].abs().max()))
    # and the value is the loss of the distances at the known orientations, restated
    D = dist64(ov.double(), su.double(), (shift & 63)[None, :].expand(FX_B, -1)).float()
    if loss == 'soft_margin':
        d = D.diagonal()
        want = (torch.log(1 + torch.exp(10. * (d[None, :] - D))) + torch.log(1 + torch.exp(10. * (d[:, None] - D)))).double().sum() \
            / (2. * FX_B * (FX_B - 1))
    else:
        from .test_batch_hard import restated_loss
        want = restated_loss(D)[0]
    assert abs(one[0] - float(want)) <= 1e-5 * abs(float(want))
