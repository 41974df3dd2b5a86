"""adam_kernel, adam_multi_kernel (csrc/conv3x3_wgrad.hip) and cvig_fov.Adam against tests/adam_ref.py: the device must give the
bits of the operation-for-operation fp32 restatement in p, m and v (the build has -ffp-contract=off and no fast-math; device
sqrtf and division are correctly rounded), which tests/test_adam_ref.py shows no listed mistake can do. cvig_fov.Adam is held to
torch.optim.Adam in float64 within the derived rounding bound."""
import numpy as np
import pytest
import torch

from . import adam_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
HYPERS = [dict(), dict(lr=3e-4, b1=0.8, b2=0.99, eps=1e-6)]
SIZES = [1, 255, 256, 257, 1000]
STEPS = [1, 2, 10, 1000, 100000]


def _kw(h):
    return dict(lr=h.get('lr', 1e-3), beta1=h.get('b1', 0.9), beta2=h.get('b2', 0.999), eps=h.get('eps', 1e-8))


def _run_single(p, g, m, v, step, hyper):
    from witw_amd import ops
    t = [torch.from_numpy(a.copy()).to(DEV) for a in (p, g, m, v)]
    ops.adam_step(t[0], t[1], t[2], t[3], step, **_kw(hyper))
    torch.cuda.synchronize()
    assert torch.equal(t[1].cpu().view(torch.int32), torch.from_numpy(g).view(torch.int32))        # the gradient is only read
    return [x.cpu().numpy() for x in (t[0], t[2], t[3])]


def _assert_bits(got, want, what):
    for name, a, b in zip('pmv', got, want):
        bad = np.nonzero((R.bits(a) != R.bits(b)) & ~(np.isnan(a) & np.isnan(b)))[0]         # a NaN's payload is not part of the contract
        assert bad.size == 0, (what, name, int(bad.size), int(bad[0]), float(a[bad[0]]), float(b[bad[0]]))


@pytest.mark.parametrize('hyper', HYPERS, ids=['default', 'other'])
@pytest.mark.parametrize('kind', ['normal', 'near_eps', 'carried', 'zero'])
def test_adam_step_equals_fp32_restatement_bit_for_bit(kind, hyper):
    for n in SIZES:
        for step in STEPS:
            p, g, m, v = R.operands(kind, n, 1000 * n + step)
            got = _run_single(p, g, m, v, step, hyper)
            _assert_bits(got, R.step32(p, g, m, v, step, **hyper), (kind, n, step))
            if kind == 'zero':          # p unchanged bit for bit, -0.0 included
                assert (R.bits(got[0]) == R.bits(p)).all()


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
def test_adam_step_nonfinite_gradient_touches_only_its_element(bad):
    for n, k in ((257, 256), (1000, 255), (1, 0)):
        p, g, m, v = R.operands('carried', n, n)
        clean = _run_single(p, g, m, v, 2, {})
        g2 = g.copy()
        g2[k] = bad
        got = _run_single(p, g2, m, v, 2, {})
        _assert_bits(got, R.step32(p, g2, m, v, 2), ('nonfinite', n, k))
        keep = np.arange(n) != k
        for a, b in zip(got, clean):
            assert (R.bits(a)[keep] == R.bits(b)[keep]).all()
        assert not np.isfinite(got[2][k]) and np.isnan(got[0][k])       # v = inf or NaN; inf / inf = NaN reaches p


def test_adam_step_subnormal_squares_follow_ieee():
    """gradients whose square, or whose square times (1 - b2), is subnormal: the expectation stays the IEEE restatement (the
    build does not flush fp32 denormals)"""
    n = 257
    r = np.random.RandomState(4)
    g = (10.0 ** r.uniform(-21.5, -18.5, n) * r.choice([-1.0, 1.0], n)).astype(np.float32)
    p = (r.randn(n) * 0.05).astype(np.float32)
    z = np.zeros(n, np.float32)
    want = R.step32(p, g, z, z, 1)
    assert ((want[2] > 0) & (want[2] < np.float32(2.0 ** -126))).any()         # subnormal second moments are really there
    _assert_bits(_run_single(p, g, z, z, 1, {}), want, 'subnormal')


def _flat_case(sizes, seed, guard=3):
    """tensors laid out back to back in one buffer per role, `guard` untouched elements (a NaN pattern) around each"""
    r = np.random.RandomState(seed)
    canary = np.array([0x7FC5A3E1], dtype=np.uint32).view(np.float32)[0]
    total = guard + sum(s + guard for s in sizes)
    bufs = [np.full(total, canary, dtype=np.float32) for _ in range(4)]
    spans, off = [], guard
    for k, s in enumerate(sizes):
        kind = ('normal', 'carried', 'near_eps')[k % 3]
        for b, a in zip(bufs, R.operands(kind, s, seed + k)):
            b[off:off + s] = a
        spans.append((off, s))
        off += s + guard
    steps = [int(x) for x in r.choice([1, 2, 3, 10, 1000, 100000], len(sizes))]
    return bufs, spans, steps


@pytest.mark.parametrize('count', [1, 48, 49, 96, 97])
@pytest.mark.parametrize('hyper', HYPERS, ids=['default', 'other'])
def test_adam_step_multi_equals_restatement_and_leaves_guards(count, hyper):
    from witw_amd import ops
    pool = [1, 255, 256, 257, 4099]
    sizes = [pool[(3 * k + count) % 5] for k in range(count)]
    if count >= 48:
        sizes[5:45] = [1] * 40                  # a run of one-element tensors: the workgroup -> tensor search crosses many entries
        sizes[45] = 4099
    bufs, spans, steps = _flat_case(sizes, 50 + count)
    dev = [torch.from_numpy(b.copy()).to(DEV) for b in bufs]
    views = [[d[o:o + s] for o, s in spans] for d in dev]
    ops.adam_step_multi(views[0], views[1], views[2], views[3], steps, **_kw(hyper))
    torch.cuda.synchronize()
    out = [d.cpu().numpy() for d in dev]
    assert (R.bits(out[1]) == R.bits(bufs[1])).all()                    # gradients only read
    inside = np.zeros(bufs[0].size, dtype=bool)
    for k, (o, s) in enumerate(spans):
        sl = slice(o, o + s)
        inside[sl] = True
        want = R.step32(bufs[0][sl], bufs[1][sl], bufs[2][sl], bufs[3][sl], steps[k], **hyper)
        _assert_bits([out[0][sl], out[2][sl], out[3][sl]], want, ('multi', count, k, s, steps[k]))
    for a, b in zip(out, bufs):                                          # guard elements between the tensors untouched
        assert (R.bits(a)[~inside] == R.bits(b)[~inside]).all()


def test_adam_class_against_torch_float64():
    """Three steps on four parameters: one never receives a gradient, one first at step 2 (its own step counter), one has a
    non-contiguous gradient. Reference: torch.optim.Adam in float64 with the hyper-parameters the C entry receives (floats).
    Bound per step from adam_ref.step_bound with the roundings of the earlier steps carried, summed over the steps."""
    from witw_amd import cvig_fov
    r = np.random.RandomState(9)
    shapes = [(300,), (17, 31), (64, 5), (257,)]
    init = [(r.randn(*s) * 0.05).astype(np.float32) for s in shapes]
    lr = 1e-3
    h32 = [float(x) for x in R.hyper32(lr, 0.9, 0.999, 1e-8)]
    pg = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV)) for a in init]
    pr = [torch.nn.Parameter(torch.from_numpy(a.copy()).double()) for a in init]
    mine = cvig_fov.Adam(pg, lr=lr)
    ref = torch.optim.Adam(pr, lr=h32[0], betas=(h32[1], h32[2]), eps=h32[3])
    bound = [np.zeros(s) for s in shapes]
    m_abs = [np.zeros(s) for s in shapes]
    own = [0, 0, 0, 0]
    for t in (1, 2, 3):
        mine.zero_grad()
        ref.zero_grad(set_to_none=True)
        for k in range(4):
            if k == 0 or (k == 1 and t < 2):
                continue                        # 0: never a gradient; 1: first gradient at step 2
            g = (r.randn(*shapes[k]) * 0.01).astype(np.float32)
            if k == 2:                          # non-contiguous gradient: a transposed view
                pg[k].grad = torch.from_numpy(np.ascontiguousarray(g.T)).to(DEV).t()
                assert not pg[k].grad.is_contiguous()
            else:
                pg[k].grad = torch.from_numpy(g).to(DEV)
            pr[k].grad = torch.from_numpy(g).double()
            own[k] += 1
            st = ref.state.get(pr[k], {})
            m0 = st['exp_avg'].numpy().copy() if st else np.zeros(shapes[k])
            v0 = st['exp_avg_sq'].numpy().copy() if st else np.zeros(shapes[k])
            bp, _, _ = R.step_bound(pr[k].detach().numpy(), g, m0, v0, own[k], lr, carried=own[k] - 1, m_abs=m_abs[k])
            bound[k] += bp
            m_abs[k] = h32[1] * m_abs[k] + (1 - h32[1]) * np.abs(g)
        versions = [getattr(q, '_witw_version', 0) for q in pg]
        mine.step()
        ref.step()
        torch.cuda.synchronize()
        moved = [k for k in range(4) if not (k == 0 or (k == 1 and t < 2))]
        for k in range(4):
            assert getattr(pg[k], '_witw_version', 0) == versions[k] + (1 if k in moved else 0), (t, k)
    assert pg[0] not in mine.state and torch.equal(pg[0].detach().cpu().view(torch.int32), torch.from_numpy(init[0]).view(torch.int32))
    assert [mine.state[pg[k]]['step'] for k in (1, 2, 3)] == [2, 3, 3]
    for k in (1, 2, 3):
        err = np.abs(pg[k].detach().cpu().double().numpy() - pr[k].detach().numpy())
        assert (err <= bound[k]).all(), (k, float((err / bound[k]).max()))
        assert (np.abs(pr[k].detach().numpy() - init[k]) > 100 * bound[k]).mean() > 0.9       # the bound is far below the movement
