"""Known-orientation matching on the GPU (witw_match_fwd_fixed, `known_shift=`): every result is compared with the existing
masked path under the one-bit words shift_mask = 1 << (shift & 63), bit for bit -- forward, norms, backward, the sharded losses,
retrieval, the heat-map scores and the CLI -- and the distances with the fp64 CPU restatement of tests/match_window_ref.py."""
import numpy as np
import pytest
import torch

from witw_amd import synth

from . import match_window_ref as R
from .test_drivers_gpu import _write_dataset
from .threaded_world import run_ranks

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _onebit(shift):
    k = shift & 63
    return torch.where(k == 63, torch.full_like(k, -2 ** 63), torch.ones_like(k) << k.clamp(max=62))


def _embeddings(Bo, Bs, We, seed):
    return (torch.from_numpy(synth.embeddings(seed, 1, (Bo, 16, 4, 64))), torch.from_numpy(synth.embeddings(seed, 2, (Bs, 16, 4, We))))


def _shifts(Bs, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'same':
        return torch.full((Bs,), 37, dtype=torch.int64)
    if kind == 'groups64':      # all 64 groups, of unequal size (group k has 1 + k % 4 members), interleaved
        sh = torch.cat([torch.full((1 + k % 4,), k, dtype=torch.int64) for k in range(64)])
        return sh[torch.randperm(len(sh), generator=g)]
    sh = torch.randint(0, 64, (Bs,), generator=g)
    sh[0], sh[-1] = 0, 63
    return sh


CASES = [(4, 4, 64, 'random'), (37, 29, 12, 'random'), (37, 29, 11, 'random'), (130, 70, 64, 'random'), (3, 200, 1, 'random'),
         (130, 70, 64, 'same'), (37, 160, 12, 'groups64')]


def _fixed_and_masked(ov, su, sh):
    from witw_amd import ops
    m = ops.match_fwd(ov, su, want_score=True, want_workspace=True, shift_mask=_onebit(sh))
    f = ops.match_fwd_fixed(ov, su, sh, want_score=True, want_workspace=True)
    assert ops.last_kernel_variant().startswith('match_fixed_kernel<'), ops.last_kernel_variant()
    return f, m


@pytest.mark.parametrize('Bo,Bs,We,kind', CASES)
def test_fixed_forward_carries_the_bits_of_the_one_bit_mask(Bo, Bs, We, kind):
    ov, su = _embeddings(Bo, Bs, We, 7)
    sh = _shifts(Bs, kind, 3)
    assert len(sh) == Bs
    (ori, d, sc, ws), (ori_m, d_m, sc_m, ws_m) = _fixed_and_masked(ov.to(DEV), su.to(DEV), sh.to(DEV))
    assert torch.equal(ori.cpu(), sh[None, :].expand(Bo, -1))
    assert torch.equal(ori, ori_m)
    assert torch.equal(d, d_m) and torch.equal(sc, sc_m)
    assert torch.equal(ws[:Bo * 64 + Bs], ws_m[:Bo * 64 + Bs])           # window norms + surface norms
    _, d_ref, _ = R.match_fused(ov, su, _onebit(sh))
    print('max |d - oracle| = %.3g' % float((d.cpu() - d_ref).abs().max()))
    np.testing.assert_allclose(d.cpu().numpy(), d_ref.numpy(), rtol=0, atol=1e-5)


def test_shifts_outside_0_63_are_taken_mod_64():
    from witw_amd import ops
    ov, su = _embeddings(37, 29, 12, 9)
    sh = _shifts(29, 'random', 5)
    wild = sh + 64 * (torch.arange(29) % 5 - 2)                          # negative and >= 64, the same value & 63
    assert int(wild.min()) < 0 and int(wild.max()) > 63 and torch.equal(wild & 63, sh)
    a = ops.match_fwd_fixed(ov.to(DEV), su.to(DEV), sh.to(DEV), want_score=True)
    b = ops.match_fwd_fixed(ov.to(DEV), su.to(DEV), wild.to(DEV), want_score=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(b[0].cpu(), sh[None, :].expand(37, -1))
    d_only = ops.match_fwd_fixed(ov.to(DEV), su.to(DEV), sh.to(DEV), want_orientation=False)
    assert d_only[0] is None and torch.equal(d_only[1], a[1])


@pytest.mark.parametrize('Bo,Bs,We', [(37, 29, 12), (130, 70, 64)])
def test_backward_carries_the_bits_of_the_masked_backward(Bo, Bs, We):
    from witw_amd import cvig_fov
    ov, su = _embeddings(Bo, Bs, We, 21)
    sh = _shifts(Bs, 'random', 8)
    w = torch.from_numpy(synth.embeddings(21, 3, (Bo, Bs))).to(DEV)
    grads = []
    for prior in ({'known_shift': sh}, {'shift_mask': _onebit(sh)}):
        o, s = ov.to(DEV).requires_grad_(True), su.to(DEV).requires_grad_(True)
        ori, d = cvig_fov.match(o, s, **prior)
        (d * w).sum().backward()
        grads.append((ori, d.detach(), o.grad, s.grad))
    for x, y in zip(*grads):
        assert torch.equal(x, y)
    assert float(grads[0][2].abs().max()) > 0 and float(grads[0][3].abs().max()) > 0


@pytest.mark.parametrize('loss', ['soft_margin', 'batch_hard'])
def test_sharded_loss_one_rank_equals_the_masked_composition(loss):
    from witw_amd import cvig_fov
    B, We = 37, 12
    ov, su = _embeddings(B, B, We, 31)
    sh = _shifts(B, 'random', 2)
    o, s = ov.to(DEV).requires_grad_(True), su.to(DEV).requires_grad_(True)
    l, ori, d = cvig_fov.sharded_match_loss(o, s, loss=loss, known_shift=sh)
    l.backward()
    o2, s2 = ov.to(DEV).requires_grad_(True), su.to(DEV).requires_grad_(True)
    ori2, d2 = cvig_fov.match(o2, s2, shift_mask=_onebit(sh))
    l2 = cvig_fov.triplet_loss(d2) if loss == 'soft_margin' else cvig_fov.batch_hard_triplet_loss(d2)
    l2.backward()
    assert torch.equal(ori, ori2) and torch.equal(d, d2.detach())
    if loss == 'soft_margin':      # the same functions in the same order
        assert torch.equal(l, l2) and torch.equal(o.grad, o2.grad) and torch.equal(s.grad, s2.grad)
    else:                          # fused pair-list backward against the dense one: tests/test_batch_hard_gpu.py's bound
        assert abs(l.item() - l2.item()) <= 1e-6 * abs(l2.item())
        for got, one in ((o.grad, o2.grad), (s.grad, s2.grad)):
            assert float((got.double() - one.double()).norm()) <= 1e-4 * float(one.double().norm()) + 1e-30


@pytest.mark.parametrize('loss', ['soft_margin', 'batch_hard'])
def test_sharded_loss_over_8_rank_threads_equals_full_matrix(loss):
    from witw_amd import cvig_fov
    B, b, We = 256, 32, 12
    ov, su = _embeddings(B, B, We, 41)
    sh = _shifts(B, 'random', 6)
    ov_d, su_d, sh_d = ov.to(DEV), su.to(DEV), sh.to(DEV)

    def fn(rank):
        torch.cuda.set_device(DEV)
        sl = slice(rank * b, (rank + 1) * b)
        ov_l, su_l = ov_d[sl].clone().requires_grad_(True), su_d[sl].clone().requires_grad_(True)
        l, ori, d = cvig_fov.sharded_match_loss(ov_l, su_l, loss=loss, known_shift=sh_d[sl].clone())
        l.backward()
        torch.cuda.synchronize()
        return l.item(), ov_l.grad.cpu(), su_l.grad.cpu(), ori.cpu(), d.cpu()
    res = run_ranks(8, fn)
    o1, s1 = ov_d.clone().requires_grad_(True), su_d.clone().requires_grad_(True)
    l1, ori1, d1 = cvig_fov.sharded_match_loss(o1, s1, loss=loss, known_shift=sh_d)
    l1.backward()
    for rank, (l, g_ov, g_su, ori, d) in enumerate(res):
        sl = slice(rank * b, (rank + 1) * b)
        assert torch.equal(ori, ori1[:, sl].cpu()) and torch.equal(d, d1[:, sl].cpu()), rank
        assert abs(l - l1.item()) <= 1e-6 * abs(l1.item()), (rank, l, l1.item())
        for got, one in ((g_ov, o1.grad[sl].cpu()), (g_su, s1.grad[sl].cpu())):
            assert float((got.double() - one.double()).norm()) <= 1e-5 * float(one.double().norm()), rank


def _planted(n_g, n_q, We, seed):
    ov = torch.from_numpy(synth.embeddings(seed, 1, (n_g, 16, 4, 64)))
    sh = _shifts(n_q, 'random', seed)
    col = (torch.arange(We)[None, :] + sh[:, None]) % 64
    su = torch.gather(ov[:n_q], 3, col[:, None, None, :].expand(-1, 16, 4, -1)) + \
        1.5 * torch.from_numpy(synth.embeddings(seed, 2, (n_q, 16, 4, We)))
    return ov.contiguous(), su.contiguous(), sh


@pytest.mark.parametrize('n_g,n_q,We,chunk', [(300, 70, 12, 32), (1100, 40, 64, 16)])
def test_retrieval_fixed_equals_direct_under_one_bit_masks(n_g, n_q, We, chunk):
    from witw_amd import cvig_fov
    ov, su, sh = _planted(n_g, n_q, We, 51)
    ov_d, su_d = ov.to(DEV), su.to(DEV)
    r0, v0, i0 = cvig_fov.retrieve(ov_d, su_d, k=10, query_chunk=chunk, method='direct', shift_mask=_onebit(sh))
    r1, v1, i1 = cvig_fov.retrieve(ov_d, su_d, k=10, query_chunk=chunk, method='fixed', known_shift=sh)
    assert np.array_equal(r0, r1) and torch.equal(v0, v1) and torch.equal(i0, i1)
    assert (r1 == 1).mean() > 0.5                                        # the planted matches rank first
    v2, i2 = cvig_fov.retrieve_topk(ov_d, su_d, k=10, query_chunk=chunk, method='fixed', known_shift=sh)
    assert torch.equal(v2, v0) and torch.equal(i2, i0)
    assert np.array_equal(cvig_fov.evaluation_ranks(ov_d[:n_q], su_d, method='fixed', known_shift=sh),
                          cvig_fov.evaluation_ranks(ov_d[:n_q], su_d, method='direct', shift_mask=_onebit(sh)))
    assert np.array_equal(cvig_fov.ranks(ov_d, su_d, known_shift=sh), r0)
    assert np.array_equal(cvig_fov.sharded_ranks(ov_d, su_d, 0, query_chunk=chunk, known_shift=sh), r0)
    # a gallery sharded over two ranks, emulated by two calls: the counts add up to the same ranks
    half = n_g // 2 + 3
    ra = cvig_fov.retrieve(ov_d[:half], su_d, k=10, shard_begin=0, query_chunk=chunk, method='fixed', known_shift=sh)[0]
    rb = cvig_fov.retrieve(ov_d[half:], su_d, k=10, shard_begin=half, query_chunk=chunk, method='fixed', known_shift=sh)[0]
    assert np.array_equal(ra + rb, r0)


def test_sweep_scores_known_shift_equals_one_bit_mask():
    from witw_amd import cvig_fov
    ov, su = _embeddings(200, 1, 12, 61)
    sh = cvig_fov.orientation_shift(35.)
    a = cvig_fov.sweep_scores(ov.to(DEV), su.to(DEV), known_shift=sh)
    b = cvig_fov.sweep_scores(ov.to(DEV), su.to(DEV), shift_mask=cvig_fov.orientation_mask(35., 0))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(cvig_fov.correlation(ov.to(DEV), su.to(DEV), known_shift=sh).cpu(), sh[None, :].expand(200, -1))


def test_cli_known_orientation_gives_the_recall_table_of_the_zero_width_window(tmp_path, monkeypatch, capsys):
    from witw_amd import cvig_fov, ops
    csv = _write_dataset(str(tmp_path), 6)
    monkeypatch.chdir(tmp_path)
    for name in ('match_method', 'precision', 'vgg16_weights', 'loss'):      # main() writes them: restored after the test
        monkeypatch.setattr(cvig_fov.Globals, name, getattr(cvig_fov.Globals, name, None), raising=False)
    monkeypatch.setattr(cvig_fov.Globals, 'test_random_orientation', False, raising=False)
    # train mode under the known orientation (training and validation loss), leaving the checkpoints test mode loads
    best = cvig_fov.train(dataset='cvusa', fov=70, val_quantity=2, batch_size=2, num_workers=0, num_epochs=1, csv_path=csv,
                          known_orientation=0.)
    assert best is not None and np.isfinite(best)
    real, tables = cvig_fov.test, []
    monkeypatch.setattr(cvig_fov, 'test', lambda **k: tables.append(real(batch_size=4, num_workers=0, csv_path=csv, **k)))
    cvig_fov.main(['--mode', 'test', '--dataset', 'cvusa', '--fov', '70', '--known-orientation', '0', '--match-method', 'fixed'])
    assert ops.last_kernel_variant().startswith('match_fixed_kernel<'), ops.last_kernel_variant()
    cvig_fov.main(['--mode', 'test', '--dataset', 'cvusa', '--fov', '70', '--orientation-window', '0,0', '--match-method', 'direct'])
    out = capsys.readouterr().out
    assert out.count('Locations: 6') == 2
    assert tables[0] == tables[1] and 0 <= tables[0]['top_1'] <= 100
