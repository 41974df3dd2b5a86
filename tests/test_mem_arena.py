"""The detector of tests/mem_arena.py, proven on CPU tensors with plain Python writers: an overrun by one element on either
side and an unwritten ragged corner are reported with where they are; a writer that stays inside passes."""
import pytest
import torch

from tests.mem_arena import ALT_BAND_BYTE, Arena, ArenaError, ArenaTorch, band_bytes, canary_int


def _flat_around(arena, t):
    """the flat element view of t's whole buffer and the element index of t[0] in it (how a stray writer reaches the bands)"""
    a = [x for x in arena.live if x.tensor.data_ptr() == t.data_ptr()][0]
    es = t.element_size()
    lead = a.off % es
    flat = a.buf[lead:lead + (a.buf.numel() - lead) // es * es].view(t.dtype)
    return flat, (a.off - lead) // es


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.int64, torch.uint8])
def test_one_element_before_the_payload_is_reported(dtype):
    arena = Arena('cpu')
    y = arena.empty((5, 7), dtype)
    flat, i0 = _flat_around(arena, y)
    y.fill_(1)
    flat[i0 - 1] = 1
    with pytest.raises(ArenaError) as e:
        arena.check(y)
    (f,) = e.value.findings
    es = y.element_size()
    assert (f['kind'], f['side']) == ('band', 'before')
    assert -es <= f['first'] <= f['last'] <= -1, f
    assert 'before the payload' in str(e.value)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.int32])
def test_one_element_after_the_payload_is_reported(dtype):
    arena = Arena('cpu')
    y = arena.empty((3, 11), dtype)
    flat, i0 = _flat_around(arena, y)
    y.fill_(2)
    flat[i0 + y.numel()] = 2
    with pytest.raises(ArenaError) as e:
        arena.check((y,))
    (f,) = e.value.findings
    es = y.element_size()
    assert (f['kind'], f['side']) == ('band', 'after')
    assert 0 <= f['first'] <= f['last'] <= es - 1, f
    assert 'after the payload' in str(e.value)


def test_an_overrun_of_a_workspace_and_of_an_input_is_reported_too():
    arena = Arena('cpu')
    ws = arena.empty((16,), torch.float32)          # not returned: bands only
    x = arena.place(torch.arange(6, dtype=torch.float32).reshape(2, 3))
    y = arena.empty((2, 3), torch.float32)
    y.copy_(x)
    arena.check(y)                                  # clean; a partly written workspace is no finding
    ws = arena.empty((16,), torch.float32)
    x = arena.place(torch.arange(6, dtype=torch.float32))
    for t in (ws, x):
        flat, i0 = _flat_around(arena, t)
        flat[i0 + t.numel() + 3] = 0.
    with pytest.raises(ArenaError) as e:
        arena.check(None)
    assert [(f['alloc'], f['side'], f['first'], f['last']) for f in e.value.findings] == [(0, 'after', 12, 15), (1, 'after', 12, 15)]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16, torch.int64, torch.int32, torch.uint8])
def test_an_unwritten_ragged_corner_is_reported_with_its_index_box(dtype):
    arena = Arena('cpu')
    y = arena.empty((2, 9, 13), dtype)
    y[0] = 1
    y[1, :8] = 1
    y[1, 8, :10] = 1            # the last row's last three columns stay unwritten
    with pytest.raises(ArenaError) as e:
        arena.check(y)
    (f,) = e.value.findings
    assert f['kind'] == 'uncovered' and f['count'] == 3 and f['lo'] == (1, 8, 10) and f['hi'] == (1, 8, 12), f
    assert bool(f['mask'][1, 8, 10:].all()) and int(f['mask'].sum()) == 3


def test_a_writer_inside_its_payload_passes_whatever_finite_value_it_stores():
    arena = Arena('cpu')
    y = arena.empty((4, 5), torch.float32)
    x = arena.place(torch.randn(4, 5))
    y.copy_(x * 0)
    c = arena.empty((4, 5), torch.uint8)
    c.copy_(torch.arange(20).reshape(4, 5) % 4)
    o = arena.empty((7,), torch.int64)
    o.fill_(-1)
    arena.check((y, c, o))
    assert arena.live == []


def test_zeros_allocations_are_zero_and_not_subject_to_coverage():
    arena = Arena('cpu')
    z = arena.zeros((3, 5), torch.float32)
    assert bool((z == 0).all())
    z[0, 0] += 1.               # a launch that accumulates into part of it
    arena.check(z)
    zl = arena.zeros_like(torch.empty(4, dtype=torch.int32))
    assert zl.dtype == torch.int32 and bool((zl == 0).all())
    arena.check(zl)


def test_a_returned_tuple_and_nested_list_are_walked():
    arena = Arena('cpu')
    a = arena.empty((4,), torch.float32)
    b = arena.empty((4,), torch.int64)
    a.fill_(0)
    b[:3] = 5
    with pytest.raises(ArenaError) as e:
        arena.check((a, [None, b], 17))
    (f,) = e.value.findings
    assert f['kind'] == 'uncovered' and f['alloc'] == 1 and f['lo'] == (3,) and f['hi'] == (3,)
    # the same tensors not returned (workspaces) are not subject to coverage
    b = arena.empty((4,), torch.int64)
    arena.check(None)


def test_a_returned_leading_slice_is_checked_over_its_own_extent():
    arena = Arena('cpu')
    p = arena.empty((64,), torch.int32)
    p[:5] = 3
    arena.check(p[:5])
    p = arena.empty((64,), torch.int32)
    p[:4] = 3
    with pytest.raises(ArenaError):
        arena.check(p[:5])


def test_empty_interiors_hold_the_canary_and_inputs_sit_in_nan_bands():
    arena = Arena('cpu')
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        y = arena.empty((33,), dtype)
        assert bool(torch.isnan(y.float()).all())
        assert bool((y.view({2: torch.int16, 4: torch.int32}[y.element_size()]) == canary_int(dtype)).all())
    assert canary_int(torch.float32) == 0x7FC5A3E1
    i = arena.empty((9,), torch.int64)
    assert bool((i.view(torch.uint8) == 0xA5).all())
    assert bool((Arena('cpu', int_fill=ALT_BAND_BYTE).empty((9,), torch.uint8) == 0x5A).all())
    for dtype in (torch.float32, torch.bfloat16):
        x = arena.place(torch.ones(10, dtype=dtype))
        flat, i0 = _flat_around(arena, x)
        assert bool((flat[i0:i0 + 10] == 1).all())
        assert bool(torch.isnan(flat[:i0].float()).all()) and bool(torch.isnan(flat[i0 + 10:].float()).all())
    arena.check(None)           # an untouched NaN band is clean


def test_band_size():
    assert band_bytes(1) == 4096 and band_bytes(4097) == 4352 and band_bytes(5 << 20) == 1 << 20


def test_interior_alignment():
    for _ in range(8):          # whatever the allocator returns
        t = Arena('cpu').empty((1000,), torch.float32)
        assert t.data_ptr() % 256 == 0 and t.data_ptr() % 512 != 0
        s = Arena('cpu', skew_bytes=16).empty((1000,), torch.float32)
        assert s.data_ptr() % 16 == 0 and s.data_ptr() % 32 != 0
        p = Arena('cpu', skew_bytes=16).place(torch.zeros(7, dtype=torch.int64))
        assert p.data_ptr() % 16 == 0 and p.data_ptr() % 32 != 0 and p.is_contiguous()


def test_arena_torch_forwards_everything_else():
    at = ArenaTorch(Arena('cpu'))
    assert at.float32 is torch.float32 and at.cuda is torch.cuda and at.Tensor is torch.Tensor
    assert at.cat is torch.cat and at.from_numpy is torch.from_numpy
    assert isinstance(torch.ones(1), at.Tensor)
    # CPU allocations pass through, in every call form ops.py uses
    for t in (at.empty((2, 3), dtype=torch.float32), at.empty(5, dtype=torch.int32, device='cpu'), at.zeros((4,), dtype=torch.uint8),
              at.empty_like(torch.ones(3)), at.zeros_like(torch.ones(3))):
        assert t.device.type == 'cpu'
    assert at.empty(2, 3).shape == (2, 3) and at._arena.live == []


def test_arena_torch_sends_device_allocations_to_the_arena(monkeypatch):
    arena = Arena('cpu')
    at = ArenaTorch(arena)
    monkeypatch.setattr(at, '_on_device', lambda device: device is not None)
    e = at.empty((3, 4), dtype=torch.float32, device='cpu')
    z = at.zeros(6, dtype=torch.int32, device=torch.device('cpu'))
    el = at.empty_like(torch.ones(5, dtype=torch.bfloat16))
    zl = at.zeros_like(torch.ones(2, 2))
    assert [a.kind for a in arena.live] == ['empty', 'zeros', 'empty', 'zeros']
    assert e.shape == (3, 4) and bool(torch.isnan(e).all()) and z.dtype == torch.int32 and bool((z == 0).all())
    assert el.dtype == torch.bfloat16 and el.shape == (5,) and zl.shape == (2, 2)
    assert at.empty((2,), dtype=torch.float32).data_ptr() not in [a.tensor.data_ptr() for a in arena.live]    # no device: torch's
