"""float64 reference of the 3x3 convolution's weight / bias gradient, and the error measure the weight-gradient tests use.

Written from the defining sum (csrc/conv3x3_wgrad.hip), not through torch.nn.functional.conv2d:

    dW[co, ci, kh, kw] = sum_{b, h, w} dZ[b, co, h, w] * Xpad[b, ci, h * SH + kh - 1, w + kw - 1]
    db[co]             = sum_{b, h, w} dZ[b, co, h, w]

Xpad is x with one zero row above and below and one column left and right: zeros, or (circular) the opposite edge column of the
same row -- rows are always zero-padded, as in oracle.cvig_fov_oracle.conv3x3. Tensors are NCHW, as torch hands them over.

The error of a result is measured against the MAGNITUDE of each element's own sum (wgrad_scale: the same sum over |dZ| |Xpad|),
not against the tensor's largest entry: one dropped pixel moves an element by about 1 / (number of pixels) of its scale whatever
the element's size next to the others, and an element whose scale is 0 (a tap that only ever sees padding, a dead tap of the
2x2 sub-window form) must be an exact 0.
"""
import numpy as np

F32_ULP = 2.0 ** -23          # spacing of fp32 numbers in [1, 2): one ulp of the scale, as a fraction of the scale


def _f64(t):
    if hasattr(t, 'detach'):
        t = t.detach().cpu().double().numpy()
    return np.ascontiguousarray(np.asarray(t, dtype=np.float64))


def _pad(x, circular):
    B, C, H, W = x.shape
    xp = np.zeros((B, C, H + 2, W + 2), dtype=np.float64)
    xp[:, :, 1:-1, 1:-1] = x
    if circular:
        xp[:, :, 1:-1, 0] = x[:, :, :, -1]
        xp[:, :, 1:-1, -1] = x[:, :, :, 0]
    return xp


def _sums(x, dz, stride_h, circular, taps4):
    B, Cin, H, W = x.shape
    Bz, Cout, Ho, Wo = dz.shape
    if stride_h not in (1, 2) or (Bz, Ho, Wo) != (B, (H - 1) // stride_h + 1, W):
        raise ValueError('dz %s does not belong to x %s under stride (%d, 1)' % (dz.shape, x.shape, stride_h))
    xp = _pad(x, circular)
    dw = np.zeros((Cout, Cin, 3, 3), dtype=np.float64)
    for kh in range(3):
        for kw in range(3):
            if taps4 and (kh == 0 or kw == 0):
                continue
            win = xp[:, :, kh:kh + (Ho - 1) * stride_h + 1:stride_h, kw:kw + W]       # Xpad[b, ci, h*SH + kh - 1, w + kw - 1]
            dw[:, :, kh, kw] = np.einsum('bohw,bihw->oi', dz, win, optimize=True)
    return dw, dz.sum(axis=(0, 2, 3))


def wgrad_ref(x_nchw, dz_nchw, stride_h, circular, taps4=False):
    """-> (dW [Cout, Cin, 3, 3], db [Cout]) float64. taps4: the taps (kh, kw) in {1,2}^2 only, exact zeros elsewhere."""
    return _sums(_f64(x_nchw), _f64(dz_nchw), stride_h, bool(circular), taps4)


def wgrad_scale(x_nchw, dz_nchw, stride_h, circular, taps4=False):
    """the same sums over |dZ| |Xpad| (and sum |dZ| for the bias): what a relative error of each element is relative to"""
    return _sums(np.abs(_f64(x_nchw)), np.abs(_f64(dz_nchw)), stride_h, bool(circular), taps4)


def err(got, ref, scale):
    """max over elements of |got - ref| / scale. Elements whose scale is 0 must be exactly 0 (AssertionError otherwise)."""
    got = _f64(got)
    if got.shape != ref.shape or ref.shape != scale.shape:
        raise AssertionError('shapes differ: got %s, reference %s, scale %s' % (got.shape, ref.shape, scale.shape))
    if not np.all(np.isfinite(got)):
        raise AssertionError('%d non-finite element(s)' % int((~np.isfinite(got)).sum()))
    dead = scale == 0
    if np.any(got[dead] != 0):
        bad = np.argwhere(dead & (got != 0))
        raise AssertionError('%d element(s) whose sum has no non-zero term are not exact zeros, first at %s = %r'
                             % (len(bad), tuple(bad[0]), float(got[tuple(bad[0])])))
    live = ~dead
    if not np.any(live):
        return 0.0
    return float((np.abs(got - ref)[live] / scale[live]).max())
