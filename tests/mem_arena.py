"""Guard-banded allocations for memory-contract tests (tests/test_memory_contract_gpu.py, tests/test_mem_arena.py).

An Arena hands out tensors that are interior views of larger flat byte buffers: a guard band on each side of the payload,
filled with a known byte, and -- for `empty` -- a payload pre-filled with a canary no kernel fed finite data can produce.
`Arena.check` then tells a store outside the payload (a dirty band) and an output element that was never stored (a canary left
in a returned tensor) from a correct launch, neither of which a value comparison of the returned tensor sees.

ArenaTorch is a stand-in for the `torch` module inside ONE module (`monkeypatch.setattr(ops, 'torch', ArenaTorch(arena))`):
device `empty` / `zeros` / `empty_like` / `zeros_like` go to the arena, everything else is torch's own. torch itself is not
patched. Works on CPU tensors too (that is how the detector itself is tested).
"""
import torch

BAND_BYTE = 0xA5
ALT_BAND_BYTE = 0x5A            # a second fill for telling "stored the canary's value" from "not stored" (see Arena.int_fill)
BAND_MIN = 4096
BAND_MAX = 1 << 20

# quiet NaNs with a fixed payload; as signed integers of the element's width
CANARY_BITS = {
    torch.float32: 0x7FC5A3E1,
    torch.bfloat16: 0x7FE5,
    torch.float16: 0x7E5A,
}
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _signed(bits, nbytes):
    if nbytes == 1:
        return bits             # viewed as uint8
    return bits - (1 << (8 * nbytes)) if bits >= 1 << (8 * nbytes - 1) else bits


def canary_int(dtype, int_fill=BAND_BYTE):
    """the canary of `dtype` as the integer its elements compare equal to when viewed as _INT_VIEW[element size]"""
    size = torch.empty((), dtype=dtype).element_size()
    if dtype in CANARY_BITS:
        return _signed(CANARY_BITS[dtype], size)
    return _signed(int.from_bytes(bytes([int_fill]) * size, 'little'), size)


def band_bytes(payload_bytes):
    """guard band per side: the payload rounded up to 256, within [4 KiB, 1 MiB] -- an overrun by a whole tile row stays inside"""
    return min(BAND_MAX, max(BAND_MIN, (payload_bytes + 255) // 256 * 256))


class ArenaError(AssertionError):
    """findings: list of dicts (kind 'band' or 'uncovered'); the message lists them"""

    def __init__(self, findings):
        self.findings = findings
        AssertionError.__init__(self, '\n'.join(f['text'] for f in findings))


class _Alloc(object):
    __slots__ = ('buf', 'off', 'nbytes', 'band', 'band_fill', 'tensor', 'kind', 'canary', 'label')


class Arena(object):
    """device: where the buffers live. skew_bytes: added to the interior's address (16: a 16-byte-aligned pointer that is not
    32-byte aligned). int_fill: the canary byte of integer `empty` payloads (BAND_BYTE; ALT_BAND_BYTE for a second run that
    settles whether an integer element equal to the canary was stored or skipped)."""

    def __init__(self, device, skew_bytes=0, int_fill=BAND_BYTE):
        self.device = torch.device(device)
        self.skew = int(skew_bytes)
        self.int_fill = int(int_fill)
        self.live = []          # allocations since the last check

    # ------------------------------------------------------------------ allocation
    def _alloc(self, shape, dtype, kind, band_canary=None, label=None):
        shape = tuple(int(s) for s in shape)
        esize = torch.empty((), dtype=dtype).element_size()
        n = 1
        for s in shape:
            n *= s
        nbytes = n * esize
        band = band_bytes(nbytes)
        buf = torch.empty(nbytes + 2 * band + 1024 + self.skew, dtype=torch.uint8, device=self.device)
        # interior = 256 bytes past a 512-byte boundary (+ skew): 256-aligned, deliberately not 512-aligned
        off = band + (256 - (buf.data_ptr() + band)) % 512 + self.skew
        a = _Alloc()
        a.buf, a.off, a.nbytes, a.band, a.kind, a.label = buf, off, nbytes, band, kind, label
        if band_canary is None:
            buf.fill_(BAND_BYTE)
            a.band_fill = None
        else:       # input bands: the NaN canary of band_canary's width, so a stray read that is multiplied poisons the result
            w = torch.empty((), dtype=band_canary).element_size()
            pat = torch.tensor([canary_int(band_canary)], dtype=_INT_VIEW[w]).view(torch.uint8).to(self.device)
            phase = (off - (off // w) * w)      # keep the pattern aligned to the payload's elements
            rep = pat.repeat(buf.numel() // w + 2)
            buf.copy_(rep[(w - phase) % w:(w - phase) % w + buf.numel()])
            a.band_fill = buf.clone()
        t = buf[off:off + nbytes].view(dtype).view(shape)
        a.canary = None
        if kind == 'empty':
            a.canary = canary_int(dtype, self.int_fill)
            if n:
                t.view(_INT_VIEW[esize]).fill_(a.canary)
        elif kind == 'zeros':
            t.zero_()
        a.tensor = t
        self.live.append(a)
        return t

    def empty(self, shape, dtype=torch.float32):
        return self._alloc(shape, dtype, 'empty')

    def zeros(self, shape, dtype=torch.float32):
        return self._alloc(shape, dtype, 'zeros')

    def empty_like(self, t):
        return self._alloc(t.shape, t.dtype, 'empty')

    def zeros_like(self, t):
        return self._alloc(t.shape, t.dtype, 'zeros')

    def place(self, t, label=None):
        """a copy of `t` (contiguous) inside NaN-canary bands"""
        t = t.detach()
        nan_dtype = t.dtype if t.dtype in CANARY_BITS else torch.float32
        out = self._alloc(t.shape, t.dtype, 'place', band_canary=nan_dtype, label=label)
        out.copy_(t)
        return out

    # ------------------------------------------------------------------ checking
    @staticmethod
    def _returned_ptrs(returned, acc):
        if isinstance(returned, torch.Tensor):
            acc.append(returned)
        elif isinstance(returned, (tuple, list)):
            for r in returned:
                Arena._returned_ptrs(r, acc)
        elif returned is not None and hasattr(returned, 'data') and isinstance(getattr(returned, 'data'), torch.Tensor):
            acc.append(returned.data)           # ops.Spectra
        return acc

    def check(self, returned=None):
        """(a) every band of every allocation since the last check still holds its fill; (b) every returned tensor that starts
        an `empty` allocation of this arena holds no canary element. Raises ArenaError listing every finding; the allocations
        are then forgotten either way."""
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)
        live, self.live = self.live, []
        findings = []
        for i, a in enumerate(live):
            for side, lo, hi in (('before', 0, a.off), ('after', a.off + a.nbytes, a.buf.numel())):
                got = a.buf[lo:hi]
                bad = (got != BAND_BYTE) if a.band_fill is None else (got != a.band_fill[lo:hi])
                if bool(bad.any()):
                    idx = bad.nonzero().flatten()
                    first, last = int(idx[0]) + lo - a.off, int(idx[-1]) + lo - a.off
                    if side == 'after':
                        first, last = first - a.nbytes, last - a.nbytes
                    findings.append({
                        'kind': 'band', 'alloc': i, 'side': side, 'first': first, 'last': last, 'count': int(idx.numel()),
                        'text': 'allocation %d (%s %s %s%s): %d byte(s) written %s the payload, byte offsets %d..%d relative to the '
                                'payload\'s %s' % (i, a.kind, tuple(a.tensor.shape), a.tensor.dtype, ', ' + a.label if a.label else '',
                                                  int(idx.numel()), side, first, last, 'start' if side == 'before' else 'end')})
        by_ptr = {a.tensor.data_ptr(): (i, a) for i, a in enumerate(live) if a.kind == 'empty' and a.nbytes}
        for k, r in enumerate(self._returned_ptrs(returned, [])):
            hit = by_ptr.get(r.data_ptr()) if r.numel() else None
            if hit is None:
                continue
            i, a = hit
            # the returned tensor's own elements (a leading slice of the allocation where the entry returns one)
            esize = r.element_size()
            mask = r.contiguous().view(_INT_VIEW[esize]) == a.canary
            if bool(mask.any()):
                idx = mask.reshape(r.shape).nonzero()
                lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
                findings.append({
                    'kind': 'uncovered', 'alloc': i, 'ret': k, 'count': int(idx.shape[0]), 'lo': tuple(lo), 'hi': tuple(hi),
                    'mask': mask.reshape(r.shape), 'dtype': r.dtype,
                    'text': 'allocation %d (returned %s %s): %d element(s) never written, index box %s..%s'
                            % (i, tuple(r.shape), r.dtype, int(idx.shape[0]), tuple(lo), tuple(hi))})
        if findings:
            raise ArenaError(findings)


class ArenaTorch(object):
    """`torch` for one module: device empty / zeros / empty_like / zeros_like come from the arena, the rest is torch's."""

    def __init__(self, arena):
        self._arena = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    def _on_device(self, device):
        return device is not None and torch.device(device).type == self._arena.device.type and self._arena.device.type != 'cpu'

    def _new(self, kind, size, kw):
        dtype = kw.pop('dtype', None) or torch.get_default_dtype()
        device = kw.pop('device', None)
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        if not self._on_device(device) or kw:
            if device is not None:
                kw['device'] = device
            return getattr(torch, kind)(*size, dtype=dtype, **kw)
        return getattr(self._arena, kind)(size, dtype)

    def empty(self, *size, **kw):
        return self._new('empty', size, kw)

    def zeros(self, *size, **kw):
        return self._new('zeros', size, kw)

    def _like(self, kind, t, kw):
        if kw or not self._on_device(t.device):
            return getattr(torch, kind)(t, **kw)
        return getattr(self._arena, kind)(t)

    def empty_like(self, t, **kw):
        return self._like('empty_like', t, kw)

    def zeros_like(self, t, **kw):
        return self._like('zeros_like', t, kw)
