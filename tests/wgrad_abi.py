"""The weight-gradient entries of libwitw_hip.so called through ctypes with the arguments witw_amd.ops does not expose:
`accumulate`, a caller-supplied workspace and `db = NULL` (tests/test_wgrad_edges_gpu.py, tools/wgrad_edge_ratios.py).

dw, db and the workspace come from a tests/mem_arena.Arena (guard bands around each); the workspace is filled with NaN before
every call. Operands are built with the layout helpers of witw_amd.ops. No ops signature is involved.
"""
import torch

from witw_amd import _lib, ops

ENTRIES = ('f32', 'taps4', 'bf16_octet', 'bf16_nhwc', 'f16x3')
_WS = {'f32': 'witw_conv3x3_wgrad_workspace_floats', 'taps4': 'witw_conv3x3_wgrad_workspace_floats',
       'bf16_octet': 'witw_conv3x3_wgrad_bf16_workspace_floats', 'bf16_nhwc': 'witw_conv3x3_wgrad_bf16_nhwc_workspace_floats',
       'f16x3': 'witw_conv3x3_wgrad_f16x3_workspace_floats'}


def out_rows(H, stride_h):
    return (H + 2 - 3) // stride_h + 1


def _cdiv(a, b):
    return -(-a // b)


def workspace_floats(entry, B, H, W, Cin, Cout, stride_h):
    return int(getattr(_lib.load(), _WS[entry])(B, H, W, Cin, Cout, stride_h))


def f16x3_bias_parts(B, H, W, stride_h):
    """partial sums of the f16x3 bias gradient (csrc/wgrad_f16x3.hip: hx_bias_rows, ~96 blocks of at least 32 pixels)"""
    npix = B * out_rows(H, stride_h) * W
    rows = max(32, _cdiv(npix, 96))
    return _cdiv(npix, rows)


def lib_splits(entry, B, H, W, Cin, Cout, stride_h):
    """the K-split count the launcher will use, from what the library exports: witw_conv3x3_wgrad_splits for the fp32 entries,
    the workspace size for the others (splits x (9 Cin Cout + Cout) floats; f16x3: two partials per split, then the bias partials)"""
    ws = workspace_floats(entry, B, H, W, Cin, Cout, stride_h)
    n = 9 * Cin * Cout
    if entry in ('f32', 'taps4'):
        s = int(_lib.load().witw_conv3x3_wgrad_splits(B, out_rows(H, stride_h), W, Cin, Cout))
        assert ws == s * (n + Cout), (ws, s)
        return s
    if entry == 'f16x3':
        s, rest = divmod(ws - f16x3_bias_parts(B, H, W, stride_h) * Cout, 2 * n)
    else:
        s, rest = divmod(ws, n + Cout)
    assert rest == 0 and s >= 1, (entry, ws, s, rest)
    return s


def _nhwc_bf16(t_nchw, C):
    assert C % 16 == 0, 'ops.nchw_to_nhwc_bf16 lays channels out in 16s: bf16 cases use multiples of 16 (C = %d)' % C
    return ops.nchw_to_nhwc_bf16(t_nchw, cpad=C)


def operands(entry, x_nchw, dz_nchw):
    """device operands of `entry` for x [B,Cin,H,W] and dz [B,Cout,Ho,W] (fp32, any device): the tensors whose pointers the entry
    takes, in its argument order. Every one of x's Cin channels is kept -- cin_real is the call's business."""
    dev = torch.device('cuda:0')
    x, dz = x_nchw.to(dev).float().contiguous(), dz_nchw.to(dev).float().contiguous()
    Cin, Cout = x.shape[1], dz.shape[1]
    if entry in ('f32', 'taps4'):
        return ops.nchw_to_nhwc(x, Cin), ops.nchw_to_nhwc(dz, Cout)
    if entry == 'bf16_nhwc':
        return _nhwc_bf16(x, Cin), _nhwc_bf16(dz, Cout)
    if entry == 'bf16_octet':
        return ops.nhwc_bf16_to_octet(_nhwc_bf16(x, Cin)), ops.nhwc_bf16_to_octet(_nhwc_bf16(dz, Cout))
    if entry == 'f16x3':
        dz_split = ops.nchw_to_split_f16(dz, Cout)
        return ops.split_f16_to_octet(ops.nchw_to_split_f16(x, Cin)), ops.split_f16_to_octet(dz_split), dz_split
    raise ValueError(entry)


def call(entry, opnd, dims, cin_real, circular, arena, accumulate=0, dw_init=None, db_init=None, want_db=True, dw_shape=None,
         ws_floats=None):
    """One launch. dims = (B, H, W, Cin, Cout, stride_h). dw / db / workspace are fresh arena allocations (NaN canaries; the
    workspace NaN-filled once more, explicitly); dw_init / db_init are copied in first (accumulate). Returns (rc, dw, db, ws)
    without synchronising or checking anything: the caller runs arena.check."""
    B, H, W, Cin, Cout, sh = dims
    lib = _lib.load()
    ws = arena.empty((ws_floats if ws_floats is not None else workspace_floats(entry, B, H, W, Cin, Cout, sh),))
    ws.fill_(float('nan'))
    dw = arena.empty(dw_shape or (Cout, cin_real, 3, 3))
    db = arena.empty((Cout,)) if want_db else None
    if dw_init is not None:
        dw.copy_(dw_init)
    if db_init is not None and db is not None:
        db.copy_(db_init)
    ptrs = [t.data_ptr() for t in opnd]
    pdb = db.data_ptr() if db is not None else None
    st = ops._stream()
    if entry == 'f32':
        rc = lib.witw_conv3x3_wgrad(ptrs[0], ptrs[1], dw.data_ptr(), pdb, ws.data_ptr(), B, H, W, Cin, cin_real, Cout, sh,
                                    int(circular), int(accumulate), st)
    elif entry == 'taps4':
        assert sh == 1 and not circular
        rc = lib.witw_conv3x3_wgrad_taps4(ptrs[0], ptrs[1], dw.data_ptr(), pdb, ws.data_ptr(), B, H, W, Cin, cin_real, Cout,
                                          int(accumulate), st)
    elif entry == 'bf16_octet':
        rc = lib.witw_conv3x3_wgrad_bf16(ptrs[0], ptrs[1], dw.data_ptr(), pdb, ws.data_ptr(), B, H, W, Cin, cin_real, Cout, sh,
                                         int(circular), int(accumulate), st)
    elif entry == 'bf16_nhwc':
        rc = lib.witw_conv3x3_wgrad_bf16_nhwc(ptrs[0], ptrs[1], dw.data_ptr(), pdb, ws.data_ptr(), B, H, W, Cin, cin_real, Cout, sh,
                                              int(circular), int(accumulate), st)
    elif entry == 'f16x3':
        rc = lib.witw_conv3x3_wgrad_f16x3(ptrs[0], ptrs[1], ptrs[2], dw.data_ptr(), pdb, ws.data_ptr(), B, H, W, Cin, cin_real, Cout,
                                          sh, int(circular), int(accumulate), st)
    else:
        raise ValueError(entry)
    return rc, dw, db, ws


def run(entry, opnd, dims, cin_real, circular, arena, **kw):
    """call() that must succeed: raises on an error code, then on a touched guard band or an element of dw / db left unwritten.
    -> (dw, db)"""
    rc, dw, db, _ws = call(entry, opnd, dims, cin_real, circular, arena, **kw)
    _lib.check(rc, 'wgrad entry %r' % entry)
    arena.check((dw, db))
    return dw, db


def last_error():
    msg = _lib.load().witw_last_error()
    return msg.decode() if msg else ''
