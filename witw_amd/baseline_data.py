"""Host-side wrappers of csrc/baseline_prep.hip: cvig_baseline's SyncedRotation + SurfaceResize('cvusa') for a whole batch of
individually stored images in one launch per side, over the descriptor table of ops.resize_batched. They are the op set of
cvig_baseline.GpuPreprocess's packed path and live here, not in ops.py; their memory-contract cases are in
tests/test_baseline_prep_gpu.py. No CPU fallback."""
import torch

from . import _lib, ops
from .ops import _stream


def roll_start(angle_deg, W):
    """The left roll in columns that cvig_baseline.horizontal_shift(img, angle_deg, 'degrees') applies to a panorama W columns wide,
    reduced to [0, W): round(angle * W / 360) with Python's half-to-even round on a double, as there."""
    return round(angle_deg * W / 360.) % int(W)


def _table(name, desc, batch):
    if not (isinstance(desc, torch.Tensor) and desc.is_cuda and desc.dtype == torch.int64 and desc.is_contiguous()
            and tuple(desc.shape) == (batch, 5)):
        raise _lib.WitwError('%s: desc must be a contiguous int64 GPU tensor [%d,5]' % (name, batch))


def rotate_batched(desc, angles_deg, batch, channels, size, kind=1, theta=None):
    """ops.rotate_nearest of every image of a descriptor table (int64 GPU [B,5] = {device address, H, W, -, channels stored per
    pixel}; kind 0 = float32 CHW sources, 1 = uint8 HWC), all of size = (H, W): -> fp32 [B,channels,H,W], bit for bit what
    ops.rotate_nearest gives on the images converted to float CHW. angles_deg: one angle per image (counter-clockwise), or None
    with theta = ops.rotation_theta(angles, H, W) already on the device."""
    _table('rotate_batched', desc, batch)
    H, W = int(size[0]), int(size[1])
    if theta is None:
        if len(angles_deg) != batch:
            raise _lib.WitwError('rotate_batched: %d angles for %d images' % (len(angles_deg), batch))
        theta = ops.rotation_theta(angles_deg, H, W).to(desc.device)
    if not (theta.is_cuda and theta.dtype == torch.float32 and theta.is_contiguous() and theta.numel() == 6 * batch):
        raise _lib.WitwError('rotate_batched: theta must be a contiguous float32 GPU tensor of %d x 6 entries' % batch)
    y = torch.empty((batch, channels, H, W), dtype=torch.float32, device=desc.device)
    _lib.check(_lib.load().witw_baseline_rotate_batched(desc.data_ptr(), theta.data_ptr(), y.data_ptr(), batch, channels, H, W, int(kind),
                                                        _stream()), 'witw_baseline_rotate_batched')
    return y


def roll_rows_batched(desc, batch, channels, size, rep=1, kind=1):
    """y[b,c,oy,ox] = image_b[c, oy // rep, (ox + start_b) % W] for a descriptor table as in rotate_batched, column 3 = start_b in
    [0, W): torch.roll(-start_b, -1) then repeat_interleave(rep, -2), exactly. size = (Ho, Wo) = (rep * H, W) of every image.
    -> fp32 [B,channels,Ho,Wo]."""
    _table('roll_rows_batched', desc, batch)
    Ho, Wo = int(size[0]), int(size[1])
    y = torch.empty((batch, channels, Ho, Wo), dtype=torch.float32, device=desc.device)
    _lib.check(_lib.load().witw_baseline_roll_rows_batched(desc.data_ptr(), y.data_ptr(), batch, channels, Ho, Wo, int(rep), int(kind),
                                                           _stream()), 'witw_baseline_roll_rows_batched')
    return y
