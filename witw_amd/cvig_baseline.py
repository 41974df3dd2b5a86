#!/usr/bin/env python
"""MI355X-native drop-in for the hot path of the reference's model/cvig_baseline.py (Liu & Li CVPR'19-style
baseline): 7 x [Conv2d(4,2,0) -> LeakyReLU(0.2) -> BatchNorm2d] encoders with GeM-like
multi-scale pooling, exhaustive minibatch triplet loss on squared Euclidean distances, Euclidean ranking.
Inference (BatchNorm running statistics folded into the conv epilogue) and training (batch statistics, full backward
through BatchNorm / LeakyReLU / the 4x4 convolutions / GeM pooling / the exhaustive loss) run on the HIP kernels.
"""
import math

import torch
import torch.nn as nn

from . import _lib, baseline_bf16, baseline_parallel, ops, parallel, retrieval, slab_loss
from . import cvig_fov as _fov
from .cvig_fov import Adam, recall_table  # noqa: F401  (same table, model/cvig_baseline.py:461-466)

device = _fov.device      # model/cvig_baseline.py:20 (cuda:0); under torch.distributed.run every process takes the GPU of its LOCAL_RANK
device_parallel = False
device_ids = None


class Globals:
    """model/cvig_baseline.py:24-48"""
    dataset_paths = {
        'cvusa': {'train': './data/train-19zl.csv', 'test': './data/val-19zl.csv'},
        'witw': {'train': './data2/train.csv', 'test': './data2/test.csv'},
    }
    path_formats = {
        'cvusa': {'path_columns': [0, 1], 'path_names': ['overhead', 'surface'], 'header': None, 'panorama': True},
        'witw': {'path_columns': [15, 16], 'path_names': ['surface', 'overhead'], 'header': 0, 'panorama': False},
    }
    precision = 'fp32'       # arithmetic of the encoders' eval forward: 'fp32', 'bf16' (blocks 1-4 on the bf16 MFMA) or 'bf16_all' (all seven); bf16 is inference only


    train_precision = 'fp32'  # arithmetic of the training step: 'fp32', or 'bf16' (forward, data and weight gradient of blocks 2-4 on the bf16 MFMA)
    sync_bn = False           # training on N ranks: BatchNorm statistics of the global batch (True) or of every rank's own share (False, nn.DataParallel)
    # not in the reference: how train() / test() bring images to the encoders. 'reference' = workers decode into float32 CHW tensors,
    # GpuPreprocess turns them sample by sample; 'packed' = the data path of cvig_fov: workers only parse / entropy-decode, each side
    # of a batch crosses PCIe as one byte block, the GPU finishes the decode and GpuPreprocess runs two launches per batch (same bits)
    data_path = 'reference'
    device_jpeg = True        # 'packed': as cvig_fov.Globals.device_jpeg / jpeg_progressive / jpeg_440
    jpeg_progressive = None
    jpeg_440 = None


PRECISIONS = ('fp32', 'bf16', 'bf16_all')
TRAIN_PRECISIONS = ('fp32', 'bf16')
DATA_PATHS = ('reference', 'packed')


# how many units make one full turn of the panorama, per first letter of the unit name; None: the shift already is in pixels
_FULL_TURN = {'p': None, 'f': 1., 'd': 360., 'r': 2 * math.pi}
_UNIT_NAMES = {first + rest + plural for first, rest in (('p', 'ixel'), ('f', 'raction'), ('d', 'egree'), ('r', 'adian'))
               for plural in ('', 's')} | set(_FULL_TURN)


def horizontal_shift(img, shift, unit='pixels'):
    """Turn a 360-degree panorama by `shift` (the viewer turning clockwise = the columns moving left), behaviour of
    model/cvig_baseline.py:97-113: units pixel(s)/p, fraction(s)/f, degree(s)/d, radian(s)/r in any case, the column count
    rounded half-to-even, anything else raises. Pinned by tests/golden/augment.npz."""
    name = unit.lower()
    if name not in _UNIT_NAMES:
        raise Exception('! Invalid unit in horizontal_shift()')
    turn = _FULL_TURN[name[0]]
    columns = shift if turn is None else shift * img.size(-1) / turn
    return img.roll(-round(columns), -1)


def quantized_rotation(img, factor):
    """Quarter turns counter-clockwise (model/cvig_baseline.py:116-128); any integer factor, a view where torch allows."""
    return torch.rot90(img, factor % 4, (-1, -2))


class ImagePairDataset(_fov.ImagePairDataset):
    """model/cvig_baseline.py:51-94: {'surface','overhead'} CPU float32 CHW tensors (no 'idx')."""
    _with_idx = False

    @classmethod
    def _globals(cls):
        return Globals


def _on_device(t):
    if not t.is_cuda:
        if device.type != 'cuda':
            raise _lib.WitwError('no gfx950 device: the WITW transforms run on the GPU only')
        t = t.to(device)
    return t


class SyncedRotation(object):
    """model/cvig_baseline.py:130-144: rotate the overhead image by a random angle; a panoramic surface image is
    rolled by the same angle. `angle` can be injected (tests)."""

    def __init__(self, dataset):
        self.dataset = dataset

    def __call__(self, data, angle=None):
        if angle is None:
            angle = torch.rand(()).item() * 360.
        if Globals.path_formats[self.dataset]['panorama']:
            data['surface'] = horizontal_shift(data['surface'], angle, unit='degrees')
        o = _on_device(data['overhead'])
        squeeze = o.dim() == 3
        o = ops.rotate_nearest(o.unsqueeze(0) if squeeze else o, [angle] * (1 if squeeze else o.shape[0]))
        data['overhead'] = o.squeeze(0) if squeeze else o
        return data


class QuantizedSyncedRotation(object):
    """model/cvig_baseline.py:147-160: multiples of 90 degrees (exact transposes / flips)."""

    def __init__(self, dataset):
        self.dataset = dataset

    def __call__(self, data, factor=None):
        if factor is None:
            factor = torch.randint(4, ()).item()
        if Globals.path_formats[self.dataset]['panorama']:
            data['surface'] = horizontal_shift(data['surface'], factor * 90, unit='degrees')
        data['overhead'] = quantized_rotation(data['overhead'], factor)
        return data


class GpuPreprocess(_fov.GpuPreprocess):
    """Compose[SyncedRotation, SurfaceResize] (model/cvig_baseline.py:324-328) over a batch of raw images, on the
    GPU: -> {'surface' [B,3,Hs,Ws], 'overhead' [B,3,Ho,Wo]} (values stay 0..255, the encoders rescale).
    A collate_raw batch of tensors takes the reference's route sample by sample (SyncedRotation, SurfaceResize: 2-3 launches and a
    copy per sample). Everything else -- a collate_packed batch (ring-backed or not) or a list of such parts, raw lists of uint8 HWC
    arrays / JpegCoef / JpegFile objects, a StagedBatch -- is staged as cvig_fov.GpuPreprocess stages it (one copy per side, the
    device JPEG decode, descriptor tables) and preprocessed in TWO launches whatever the batch size: baseline_data.roll_rows_batched
    (cvusa: roll + row doubling) or ops.resize_batched (witw: 500 x 500) on the surface side, baseline_data.rotate_batched on the
    overhead side. Both routes give the same bits for the same angles. One angle per sample, in sample order, from
    torch.rand(()).item() * 360. (what SyncedRotation draws), or `angles`."""

    def __init__(self, dataset, device=None, ring=None):
        # cvig_fov.GpuPreprocess.__init__ is NOT run (its Resize / ImageNormalization / PolarTransform are cvig_fov's model). What is
        # inherited is its staging -- stage(), _copy_side, _table_side, _stage_side -- which reads only `channels`, `ring`, _dev() and
        # _stage_tail() of the object: a base-class stage() that starts to read anything else must be given it here
        self.dataset = dataset
        self.rotation = SyncedRotation(dataset)
        self.resize = SurfaceResize(dataset)
        self.panorama = Globals.path_formats[dataset]['panorama']
        self.device = device      # where host images go; None = cvig_baseline.device
        self.ring = ring          # ring.PinnedRing the loader's collate_packed builds its batch blocks in (None: ordinary blocks)

    def _dev(self):      # as the base class, with THIS module's default device
        dev = self.device if self.device is not None else device
        if dev.type != 'cuda':
            raise _lib.WitwError('no gfx950 device: the WITW transforms run on the GPU only')
        return dev

    @staticmethod
    def _one_size(tab, what):
        """(H, W) shared by every row of a host table, else a WitwError naming two sizes that differ"""
        hw = tab[:, 1:3]
        odd = (hw != hw[0]).any(dim=1).nonzero()
        if odd.numel():
            h, w = hw[int(odd[0])].tolist()
            raise _lib.WitwError('the %s images of a batch differ in size: %dx%d and %dx%d' % (what, int(hw[0, 0]), int(hw[0, 1]), h, w))
        return int(hw[0, 0]), int(hw[0, 1])

    def _stage_tail(self, st, s_tab, o_tab, angles):
        """the rotation angles of the batch: theta of the overhead side, the roll starts of a panoramic surface side (column 3)"""
        from . import baseline_data
        s_tab = s_tab.cpu() if s_tab.is_cuda else s_tab
        o_tab = o_tab.cpu() if o_tab.is_cuda else o_tab
        few = int(min(s_tab[:, 4].min(), o_tab[:, 4].min()))
        if few < self.channels:
            raise _lib.WitwError('an image of the batch has %d channels, the model takes %d' % (few, self.channels))
        if angles is None:
            angles = [torch.rand(()).item() * 360. for _ in range(st.n)]
        angles = [float(a) for a in angles]
        if len(angles) != st.n:
            raise _lib.WitwError('GpuPreprocess: %d angles for a batch of %d' % (len(angles), st.n))
        st.angles = angles
        st.o_size = self._one_size(o_tab, 'overhead')
        st.s_size = None
        if self.panorama:
            st.s_size = self._one_size(s_tab, 'surface')
            s_tab[:, 3] = torch.tensor([baseline_data.roll_start(a, st.s_size[1]) for a in angles], dtype=torch.int64)
        theta = ops.rotation_theta(angles, *st.o_size).reshape(st.n, 6)
        st.theta = theta.pin_memory().to(self._dev(), non_blocking=True)
        st.keep.append(st.theta)
        return s_tab, o_tab

    def stage(self, batch, angles=None):
        """cvig_fov.GpuPreprocess.stage plus the draws of _stage_tail; an empty collate_raw batch (a rank's empty share) gives a
        StagedBatch with n == 0. A StagedBatch comes back as it is: its angles were drawn when it was staged, so `angles` with one
        is refused"""
        if isinstance(batch, _fov.StagedBatch):
            if angles is not None:
                raise _lib.WitwError('GpuPreprocess: a StagedBatch carries the angles it was staged with; pass `angles` to stage()')
            return batch
        if isinstance(batch, dict) and not batch.get('packed') and not batch['surface']:
            return _fov.StagedBatch()
        return _fov.GpuPreprocess.stage(self, batch, angles)

    def _per_sample(self, batch, angles):
        s, o = [], []
        for i, (su, ov) in enumerate(zip(batch['surface'], batch['overhead'])):
            data = {'surface': _on_device(su[:3]), 'overhead': ov[:3]}
            d = self.resize(self.rotation(data) if angles is None else self.rotation(data, angles[i]))
            s.append(d['surface'])
            o.append(d['overhead'])
        return {'surface': torch.stack(s), 'overhead': torch.stack(o)}

    def __call__(self, batch, angles=None):
        from . import baseline_data
        if isinstance(batch, dict) and not batch.get('packed') and all(isinstance(t, torch.Tensor) for t in batch['surface'] + batch['overhead']):
            return self._per_sample(batch, angles)
        st = self.stage(batch, angles)
        if st.n == 0:
            raise _lib.WitwError('GpuPreprocess: an empty batch')
        st.wait()
        c = self.channels
        if self.dataset == 'cvusa':
            surface = baseline_data.roll_rows_batched(st.s_desc, st.n, c, (2 * st.s_size[0], st.s_size[1]), rep=2, kind=st.s_kind)
        elif self.dataset == 'witw':
            surface = ops.resize_batched(st.s_desc, st.n, c, (500, 500), kind=st.s_kind)
        else:
            raise Exception('! Invalid dataset type in ' + type(self).__name__ + '().')
        overhead = baseline_data.rotate_batched(st.o_desc, None, st.n, c, st.o_size, kind=st.o_kind, theta=st.theta)
        return {'surface': surface, 'overhead': overhead}


def collate_packed(samples, ring=None):
    """cvig_fov.collate_packed for the 'packed' data path; an empty sample list (GlobalBatchShares: more ranks than rows) stays
    collate_raw's empty batch, which _embed_share and GpuPreprocess.stage know"""
    if not samples:
        return {'surface': [], 'overhead': []}
    return _fov.collate_packed(samples, ring)


class SurfaceResize(object):
    """model/cvig_baseline.py:208-225 on the GPU."""

    def __init__(self, dataset):
        self.dataset = dataset

    def __call__(self, data):
        s = data['surface']
        if self.dataset == 'cvusa':
            data['surface'] = torch.repeat_interleave(s, 2, dim=-2)
        elif self.dataset == 'witw':
            x = s.to(device) if not s.is_cuda else s
            squeeze = x.dim() == 3
            x = ops.resize_bilinear((x.unsqueeze(0) if squeeze else x).contiguous(), (500, 500))
            data['surface'] = x.squeeze(0) if squeeze else x
        else:
            raise Exception('! Invalid dataset type in ' + type(self).__name__ + '().')
        return data


class SurfaceEncoder(nn.Module):
    """model/cvig_baseline.py:228-279; parameters live in nn.Conv2d / nn.BatchNorm2d children named
    conv1..7 / bn1..7 (same state-dict keys), the forward runs on the HIP kernels."""

    def __init__(self, orientation=False, bands=3, p=3., precision=None, train_precision=None, sync_bn=None):
        """precision: None = Globals.precision; 'fp32', or 'bf16' = the eval forward runs blocks 1-4 with bf16 operands and fp32
        accumulation (bf16 activations between them, fp32 into block 5; the filters are rounded from the fp32 master weights, the
        BatchNorm fold, blocks 5-7, pooling and normalisation stay fp32); 'bf16_all' = blocks 5-7 as well: block 4 stores bf16, blocks
        5-7 run the bf16 split-K convolution over bf16 mosaics (baseline_bf16.conv_taps4_splitk_bf16), their fp32 outputs are pooled
        unrounded and rounded once on the way into the next block. `precision` never changes the training step.
        train_precision: None = Globals.train_precision; 'fp32', or 'bf16' = the training step runs the three convolutions of blocks 2-4
        (forward, data gradient, weight gradient) with bf16 operands and fp32 accumulation. Rounded once, nearest-even: the filters (from
        the fp32 master weights, per weight version), a block's input and a block's output gradient. Master weights, gradients, BatchNorm
        statistics, LeakyReLU gates, blocks 1 and 5-7, pooling and the loss stay fp32. At most 5 input channels, as precision='bf16'.
        sync_bn: None = Globals.sync_bn; False = under a process group every rank normalises with the statistics of its own images (an
        nn.DataParallel replica). True = the training step's seven BatchNorm layers take mean and variance over the GLOBAL batch: per layer
        one all-reduce of 2C floats in the forward and one in the backward (baseline_parallel.sync_bn_train_stats / sync_bn_lrelu_bwd), the
        running buffers are then the same on every rank, and the N-rank step is the one-process step on the concatenated batch up to
        summation order. With no process group the same kernels run without a collective. Works under either train_precision (BatchNorm
        is fp32 in both). Before the step's gradient all-reduce bnK.weight.grad / bnK.bias.grad hold 1/N of the gradient (see
        sync_bn_lrelu_bwd). Never changes the eval forward."""
        super().__init__()
        self.sync_bn = bool(Globals.sync_bn if sync_bn is None else sync_bn)
        self.precision = Globals.precision if precision is None else precision
        if self.precision not in PRECISIONS:
            raise _lib.WitwError("cvig_baseline encoder: precision must be 'fp32', 'bf16' or 'bf16_all', got %r" % (self.precision,))
        self.train_precision = Globals.train_precision if train_precision is None else train_precision
        if self.train_precision not in TRAIN_PRECISIONS:
            raise _lib.WitwError("cvig_baseline encoder: train_precision must be 'fp32' or 'bf16', got %r" % (self.train_precision,))
        self.orientation, self.bands, self.p = orientation, bands, p
        self.inputs = self.bands + 2 * self.orientation
        widths = [self.inputs, 64, 128, 256, 512, 512, 512, 512]
        for i in range(1, 8):
            conv = nn.Conv2d(widths[i - 1], widths[i], kernel_size=4, stride=2, padding=0)
            bn = nn.BatchNorm2d(widths[i], momentum=0.1, affine=True, track_running_stats=True)
            torch.nn.init.normal_(conv.weight, mean=0.0, std=0.02)     # :255-262
            torch.nn.init.normal_(conv.bias, mean=0.0, std=0.02)
            torch.nn.init.normal_(bn.weight, mean=1.0, std=0.02)
            torch.nn.init.normal_(bn.bias, mean=0.0, std=0.02)
            setattr(self, 'conv%d' % i, conv)
            setattr(self, 'bn%d' % i, bn)
        self._packed = {}
        self.fused_first = True       # eval forward: block 1 by witw_conv4x4s2_first_fwd (False: space-to-depth pass + 2x2-tap conv)

    def _layer(self, i, fold=True, pack=True):
        """-> (packed 2x2-tap filter, eval-mode BatchNorm scale, shift, padded input channels). fold=False (the training forward:
        batch statistics) skips the scale / shift of the running statistics. pack=False (blocks 1-4 of the 'bf16' forward and every block of the 'bf16_all' one, which never
        launch the fp32 image) skips the fp32 packing: the first element is then whatever image there is, possibly None."""
        conv, bn = getattr(self, 'conv%d' % i), getattr(self, 'bn%d' % i)
        # torch's version counters see in-place torch ops; the C-ABI Adam bumps _witw_version instead
        wkey = tuple(t._version for t in (conv.weight, conv.bias)) + tuple(getattr(t, '_witw_version', 0) for t in (conv.weight, conv.bias)) + \
            (conv.weight.data_ptr(),)
        hit = self._packed.get(i)
        if hit is None or hit[0] != wkey:
            with torch.no_grad():
                co, ci = conv.weight.shape[:2]
                cpad = (4 * ci + 7) // 8 * 8
                # 4x4/s2 filter -> 3x3 filter over space-to-depth channels (dy*2+dx)*ci+c; tap (kh,kw) in {1,2}^2 holds
                # W[:, :, 2(kh-1)+dy, 2(kw-1)+dx], row / column 0 of the taps stay zero (witw_conv4x4_to_k3: one launch)
                k3 = ops.conv4x4_to_k3(conv.weight, cpad)
            hit = [wkey, None, cpad, k3, None, (hit[1] or hit[5]) if hit else None]      # [5]: a stale fp32 image to overwrite in place
            self._packed[i] = hit
        if pack and hit[1] is None:
            with torch.no_grad():
                hit[1] = ops.PackedConv(hit[3], conv.bias, taps4=True, reuse=hit[5])      # only the 2x2 live taps
            hit[5] = None
        if not fold:
            return hit[1], None, None, hit[2]
        bkey = tuple(t._version for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)) + \
            tuple(getattr(t, '_witw_version', 0) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
        if hit[4] is None or hit[4][0] != bkey:
            with torch.no_grad():
                scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)               # eval-mode BatchNorm2d
                shift = bn.bias - bn.running_mean * scale
            hit[4] = (bkey, scale.contiguous(), shift.contiguous())
        return hit[1], hit[4][1], hit[4][2], hit[2]

    def _layer_bf16(self, i):
        """the bf16 2x2-tap filter of block i, re-packed in place when the weights have changed (the key of _layer)"""
        self._layer(i, fold=False, pack=False)
        wkey, k3 = self._packed[i][0], self._packed[i][3]
        hit = self._packed.get(('bf16', i))
        if hit is None or hit[0] != wkey:
            conv = getattr(self, 'conv%d' % i)
            hit = (wkey, baseline_bf16.PackedConvBf16Taps4(k3, conv.bias, reuse=hit[1] if hit else None))
            self._packed[('bf16', i)] = hit
        return hit[1]

    def _layer_bf16_t(self, i):
        """the bf16 data-gradient filter of block i (_layer_t's, rounded once), re-packed in place when the weights have changed"""
        self._layer(i, fold=False, pack=False)
        wkey, k3 = self._packed[i][0], self._packed[i][3]
        hit = self._packed.get(('bf16_t', i))
        if hit is None or hit[0] != wkey:
            hit = (wkey, baseline_bf16.PackedConvBf16Taps4(k3, None, reuse=hit[1] if hit else None, transpose_flip=True))
            self._packed[('bf16_t', i)] = hit
        return hit[1]

    def _layer_k3(self, i, pack=True):
        self._layer(i, fold=False, pack=pack)
        return self._packed[i][3]

    def _layer_t(self, i):
        """the data-gradient filter of block i (transposed, taps rotated), re-packed in place when the weights have changed"""
        self._layer(i, fold=False)
        wkey, k3 = self._packed[i][0], self._packed[i][3]
        hit = self._packed.get(('t', i))
        if hit is None or hit[0] != wkey:
            hit = (wkey, ops.PackedConv(k3, None, transpose_flip=True, taps4=True, reuse=hit[1] if hit else None))
            self._packed[('t', i)] = hit
        return hit[1]

    def train_params(self):
        out = []
        for i in range(1, 8):
            conv, bn = getattr(self, 'conv%d' % i), getattr(self, 'bn%d' % i)
            out += [conv.weight, conv.bias, bn.weight, bn.bias]
        return out

    def forward(self, x, lrelu_acts=None):
        """model/cvig_baseline.py:264-284. Parity hook (train mode): `lrelu_acts` {block i: NHWC tensor} replaces, in the
        BACKWARD's LeakyReLU gate only, the activation this forward recorded (its sign is the gate); the dict is read when
        the backward runs, so it may be filled after the forward (tests/test_baseline_gpu.py: a conv output within rounding of
        zero can fall on the other side of the kink than it did on the CPU reference)."""
        if not x.is_cuda:
            raise _lib.WitwError('SurfaceEncoder.forward needs a GPU tensor (no CPU fallback)')
        B, _c, H, W = x.shape
        if min(H, W) < 382:
            raise _lib.WitwError('cvig_baseline encoder needs sides >= 382 px, got %dx%d' % (H, W))
        bf16 = self.precision in ('bf16', 'bf16_all')
        bf16_all = self.precision == 'bf16_all'
        bf16_train = self.training and self.train_precision == 'bf16'
        if bf16 and self.training and not bf16_train:
            raise _lib.WitwError("cvig_baseline encoder: precision='%s' is inference only -- fp32 is the only training arithmetic" % self.precision)
        if bf16_train and self.inputs > 5:
            raise _lib.WitwError("cvig_baseline encoder: train_precision='bf16' takes at most 5 input channels, got %d" % self.inputs)
        if bf16 and self.inputs > 5:
            raise _lib.WitwError("cvig_baseline encoder: precision='%s' needs the fused first block (at most 5 input channels, got %d)"
                                 % (self.precision, self.inputs))
        if self.training:
            self._bwd_override = {} if lrelu_acts is None else lrelu_acts
            return _BaselineEncoderFn.apply(x, self, *self.train_params())
        with torch.no_grad():
            f = torch.empty((B, 1536), dtype=torch.float32, device=x.device)
            vh, vw = H, W
            g = 1                  # images per mosaic side of the current layer input h
            # block 1 straight from the raw image (normalisation :265-266, conv1, LeakyReLU, bn1 in one launch) when the second
            # block reads exactly its 4 x 64 space-to-depth channels; otherwise the re-layout pass + the generic 2x2-tap form
            fused_first = bf16 or (self.fused_first and self._layer(2)[3] == 256 and self.inputs <= 5)
            h = None if fused_first else ops.space_to_depth2(x.contiguous(), in_nchw=True, normalize=True, cpad=self._layer(1)[3])
            for i in range(1, 8):
                packed, scale, shift, _cp = self._layer(i, pack=not (bf16_all or (bf16 and i < 5)))
                vh, vw = (vh - 4) // 2 + 1, (vw - 4) // 2 + 1
                if i == 1 and fused_first:
                    h = ops.conv4x4s2_first(x.contiguous(), self.conv1.weight, self.conv1.bias, scale, shift, normalize=True, lrelu_slope=0.2,
                                            out_bf16=bf16)
                    continue
                if bf16 and i < 5:
                    # blocks 2-4 on the bf16 MFMA: bf16 activations between them, block 4 hands fp32 to the fp32 split-K blocks
                    # ('bf16') or bf16 to the bf16 ones ('bf16_all')
                    h = baseline_bf16.conv_taps4_s2d_bf16(h, self._layer_bf16(i), (vh, vw), lrelu_slope=0.2, post_scale=scale, post_shift=shift,
                                                out_f32=(i == 4 and not bf16_all))
                    continue
                if bf16_all:
                    # blocks 5-7 on the bf16 MFMA: split-K over a bf16 mosaic, fp32 out: pooled unrounded, rounded once into the next block
                    y = baseline_bf16.conv_taps4_splitk_bf16(h, self._layer_bf16(i), B, g, (vh, vw), lrelu_slope=0.2, post_scale=scale,
                                                             post_shift=shift)
                    ops.gem_pool(y, (vh, vw), f, 512 * (i - 5), self.p)
                    if i < 7:
                        nh, nw = (vh + 1) // 2, (vw + 1) // 2
                        g = max(1, min(16 // nh, 16 // nw))
                        h = baseline_bf16.space_to_depth2_mosaic_bf16(y, g)
                    continue
                if i < 5 and 4 * packed.cout == self._layer(i + 1)[3]:
                    # blocks 1-4: the epilogue writes the next block's space-to-depth input directly
                    h = ops.conv_taps4_s2d(h, packed, (vh, vw), lrelu_slope=0.2, post_scale=scale, post_shift=shift)
                    continue
                # blocks 5-7 (maps of 16x16 and below, K = 4 x 2048): split-K over a mosaic that fills the 16x16 tile
                y = ops.conv_taps4_splitk(h, packed, B, g, (vh, vw), lrelu_slope=0.2, post_scale=scale, post_shift=shift)
                if i >= 5:
                    ops.gem_pool(y, (vh, vw), f, 512 * (i - 5), self.p)                                      # :276-282
                if i < 7:
                    nh, nw = (vh + 1) // 2, (vw + 1) // 2
                    g = max(1, min(16 // nh, 16 // nw))
                    h = ops.space_to_depth2_mosaic(y, g)
            return ops.embed_normalize_(f)                                                                 # :283-284


class OverheadEncoder(SurfaceEncoder):
    pass


def _mosaic_g(x):
    """images per mosaic side for an NHWC batch of small maps: as many cells as fit a 16 x 16 tile"""
    return max(1, min(16 // x.shape[1], 16 // x.shape[2]))


def _to_mosaic(x, g):
    """[B,h,w,C] -> [ceil(B/g^2), g*h, g*w, C]: g x g images side by side (missing images zero); pure data movement on maps of at
    most 16 x 16 (the layout ops.space_to_depth2_mosaic writes directly on the eval path)"""
    if g == 1:
        return x
    B, h, w, C = x.shape
    Bm = (B + g * g - 1) // (g * g)
    if Bm * g * g != B:
        x = torch.cat((x, x.new_zeros((Bm * g * g - B, h, w, C))), 0)
    return x.reshape(Bm, g, g, h, w, C).permute(0, 1, 3, 2, 4, 5).reshape(Bm, g * h, g * w, C).contiguous()


def _pad_hw(y, H, W):
    """[B,vh,vw,C] -> [B,H,W,C], zeros outside (the layout conv3x3_fwd gives an activation: its input's spatial size)"""
    if y.shape[1] == H and y.shape[2] == W:
        return y
    return torch.nn.functional.pad(y, (0, 0, 0, W - y.shape[2], 0, H - y.shape[1]))


class _BaselineEncoderFn(torch.autograd.Function):
    """Train-mode forward (BatchNorm2d batch statistics, running-stat update) and backward of one encoder call.
    enc.train_precision == 'bf16': blocks 2-4 keep their input h as bf16 only (rounded once, behind the producer's BatchNorm affine) and
    run forward, data gradient and weight gradient through baseline_bf16; their activations a, the statistics and the gates stay fp32."""

    @staticmethod
    def forward(ctx, x, enc, *params):
        B, _c, H, W = x.shape
        with torch.no_grad():
            h = ops.space_to_depth2(x.contiguous(), in_nchw=True, normalize=True, cpad=enc._layer(1, fold=False)[3])
            g = torch.empty((B, 1536), dtype=torch.float32, device=x.device)
            vh, vw = H, W
            saved = []
            bf = enc.train_precision == 'bf16'
            if enc.sync_bn:      # BatchNorm over the global batch: its image count once per call, two sums per channel and layer
                images = baseline_parallel.sync_bn_global_images(B, x.device)
            for i in range(1, 8):
                on_bf16 = bf and 2 <= i <= 4
                packed, _es, _et, _cp = enc._layer(i, fold=False, pack=not on_bf16)
                bn = getattr(enc, 'bn%d' % i)
                vh, vw = (vh - 4) // 2 + 1, (vw - 4) // 2 + 1
                if i >= 5:      # maps of 16 x 16 and below: split-K over a mosaic of g x g images, as the eval path (15 of 16 lanes of
                    gm = _mosaic_g(h)                     # the narrow-geometry kernel idle otherwise); zero-padded to the input's size
                    a = _pad_hw(ops.conv_taps4_splitk(_to_mosaic(h, gm), packed, B, gm, (vh, vw), lrelu_slope=0.2), h.shape[1], h.shape[2])
                elif on_bf16:
                    a = baseline_bf16.conv_taps4_plain_bf16(h, enc._layer_bf16(i), (vh, vw), lrelu_slope=0.2)
                else:
                    a = ops.conv3x3_fwd(h, packed, relu=False, lrelu_slope=0.2)              # LeakyReLU(conv), :267-275
                if enc.sync_bn:
                    mean, invstd, scale, shift = baseline_parallel.sync_bn_train_stats(a, (vh, vw), bn, images)
                else:
                    mean, invstd, scale, shift = ops.bn_train_stats(a, (vh, vw), bn.weight, bn.bias, bn.running_mean,
                                                                    bn.running_var, bn.eps, bn.momentum)
                bn.num_batches_tracked += 1
                for t in (bn.running_mean, bn.running_var):      # updated through the C-ABI: invalidate the eval fold
                    t._witw_version = getattr(t, '_witw_version', 0) + 1
                saved.append((h, a, (vh, vw), mean, invstd, scale, shift))
                if i >= 5:
                    ops.gem_pool(a, (vh, vw), g, 512 * (i - 5), enc.p, scale, shift)
                if bf and 1 <= i <= 3:      # the input of a bf16 block: the same affine in fp32, one rounding at the store
                    h = baseline_bf16.space_to_depth2_bf16(a, valid_hw=(vh, vw), scale=scale, shift=shift)
                elif i < 7:
                    h = ops.space_to_depth2(a, valid_hw=(vh, vw), cpad=enc._layer(i + 1, fold=False)[3], scale=scale, shift=shift)
            f = ops.embed_normalize_(g.clone())
        ctx.enc, ctx.saved, ctx.g, ctx.bf = enc, saved, g, bf
        ctx.sync_images = images if enc.sync_bn else None
        ctx.override = getattr(enc, '_bwd_override', {})
        enc._bwd_override = {}
        enc._last_saved = saved if getattr(enc, 'keep_activations', False) else None     # diagnostics / parity tests
        return f

    @staticmethod
    def backward(ctx, df):
        enc, saved, g = ctx.enc, ctx.saved, ctx.g
        dg = ops.embed_normalize_bwd(g, df.contiguous())
        grads = [None] * 28
        dx_s2d = None
        for i in range(7, 0, -1):
            h, a, valid, mean, invstd, scale, shift = saved[i - 1]
            conv, bn = getattr(enc, 'conv%d' % i), getattr(enc, 'bn%d' % i)
            s2d_grad = False
            if i == 7:
                dy = ops.gem_pool_bwd(a, scale, shift, g, dg, valid, 1024, enc.p)
            elif i >= 5:
                dy = ops.depth_to_space2(dx_s2d, a, valid)
                ops.gem_pool_bwd(a, scale, shift, g, dg, valid, 512 * (i - 5), enc.p, out=dy)
            else:       # blocks 1-4 (the large maps): the BatchNorm backward reads the space-to-depth gradient in place
                dy, s2d_grad = dx_s2d, True
            if ctx.sync_images is not None:
                dz, dgamma, dbeta = baseline_parallel.sync_bn_lrelu_bwd(ctx.override.get(i, a), dy, valid, mean, invstd, bn.weight,
                                                                        ctx.sync_images, 0.2, dy_s2d=s2d_grad)
            else:
                dz, dgamma, dbeta = ops.bn_lrelu_bwd(ctx.override.get(i, a), dy, valid, mean, invstd, bn.weight, 0.2, dy_s2d=s2d_grad)
            on_bf16 = ctx.bf and 2 <= i <= 4
            k3 = enc._layer_k3(i, pack=not on_bf16)
            if on_bf16:
                dz = baseline_bf16.to_bf16(dz)      # the block's output gradient: rounded once, read by both gradients
                dk3, dbias = baseline_bf16.conv3x3_wgrad_bf16_taps4(h, dz, k3.shape[1])
            else:
                dk3, dbias = ops.conv3x3_wgrad(h, dz, k3.shape[1], stride_h=1, circular=False, taps4=True)
            # tap (ta+1, tb+1) of the 3x3 filter holds W[:, :, 2ta+dy, 2tb+dx] as channel (dy,dx,c): gathered back in one launch
            dw = ops.k3_to_conv4x4(dk3, conv.weight.shape[1])
            grads[4 * (i - 1):4 * i] = [dw, dbias, dgamma, dbeta]
            if on_bf16:
                dx_s2d = baseline_bf16.conv_taps4_plain_bf16(dz, enc._layer_bf16_t(i))
            elif i > 1:
                pk_t = enc._layer_t(i)
                if i >= 5:      # the same small maps in the data gradient: mosaic + split-K (dz is zero outside its valid region,
                    gm = _mosaic_g(dz)                    # so the last row / column of every cell is the zero border a window may touch)
                    dx_s2d = ops.conv_taps4_splitk(_to_mosaic(dz, gm), pk_t, dz.shape[0], gm, (dz.shape[1], dz.shape[2]))
                else:
                    dx_s2d = ops.conv3x3_fwd(dz, pk_t, relu=False)
        ctx.saved = ctx.g = None
        return (None, None) + tuple(grads)


class _ExhaustiveLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e1, e2, soft_margin, alpha, margin):
        e1, e2 = e1.contiguous(), e2.contiguous()
        D = ops.pairwise_sqdist(e1, e2)
        ctx.save_for_backward(e1, e2, D)
        ctx.cfg = (soft_margin, alpha, margin)
        return ops.exhaustive_triplet_loss(D, soft_margin, alpha, margin)

    @staticmethod
    def backward(ctx, gl):
        e1, e2, D = ctx.saved_tensors
        de1, de2 = ops.exhaustive_triplet_loss_bwd(e1, e2, D, gl.contiguous(), *ctx.cfg)
        return de1, de2, None, None, None


def exhaustive_minibatch_triplet_loss(embed1, embed2, soft_margin=False, alpha=10., margin=1.):
    """model/cvig_baseline.py:286-315 (all valid (a,p,n) combinations of the minibatch); differentiable."""
    if torch.is_grad_enabled() and (embed1.requires_grad or embed2.requires_grad):
        return _ExhaustiveLossFn.apply(embed1, embed2, bool(soft_margin), float(alpha), float(margin))
    D = ops.pairwise_sqdist(embed1.contiguous(), embed2.contiguous())
    return ops.exhaustive_triplet_loss(D, soft_margin, alpha, margin)


def _slab_kernels():
    from types import SimpleNamespace
    from . import baseline_parallel as bp
    return SimpleNamespace(pairwise_sqdist=ops.pairwise_sqdist, exhaustive_loss_slab_fwd=bp.exhaustive_loss_slab_fwd,
                           exhaustive_loss_slab_sig=bp.exhaustive_loss_slab_sig, exhaustive_loss_slab_bwd=bp.exhaustive_loss_slab_bwd,
                           sqdist_rect_bwd=bp.sqdist_rect_bwd)


class _ShardedExhaustiveLossFn(torch.autograd.Function):
    """exhaustive_minibatch_triplet_loss over the GLOBAL batch with the distance matrix sharded by COLUMNS over the ranks, on the
    column-slab protocol of witw_amd.slab_loss: rank r evaluates all B overhead embeddings against its own b surface embeddings (a [B,b]
    slab of squared distances; the loss is symmetric in its two arguments, so which side is gathered is free). Exchanges:
    forward = all-gather of the overhead embeddings and of the diagonal (B floats), all-reduce of the loss partial; backward =
    all-reduce of the row sums of l' (B floats), reduce-scatter of the overhead-embedding gradients (every rank holds the part
    that flows through ITS surfaces). The surface gradients are complete locally. One rank runs the same kernels on the one slab
    b = B, col0 = 0, without a collective."""

    @staticmethod
    def forward(ctx, surface_local, overhead_local, soft_margin, alpha, margin, k):
        x, y, b, col0, B, world = slab_loss.open_slab(overhead_local, surface_local, who='sharded_exhaustive_loss')
        with parallel.phase('slab_distances'):
            T = k.pairwise_sqdist(x, y)
        diag = slab_loss.gather_diagonal(T, col0, b, world > 1)
        part = slab_loss.sum_partial(lambda: k.exhaustive_loss_slab_fwd(T, diag, col0, soft_margin, alpha, margin), True)
        ctx.save_for_backward(x, y, T, diag)
        ctx.cfg = (col0, b, soft_margin, alpha, margin, k)
        return (part / (2. * B * (B - 1))).reshape(())

    @staticmethod
    def backward(ctx, g_loss):
        x, y, T, diag = ctx.saved_tensors
        col0, b, soft_margin, alpha, margin, k = ctx.cfg
        with parallel.phase('row_sums_all_reduce'):
            rowsig, colsig = k.exhaustive_loss_slab_sig(T, diag, col0, soft_margin, alpha, margin)
            parallel.all_reduce_sum_(rowsig)
        with parallel.phase('slab_backward'):
            G = k.exhaustive_loss_slab_bwd(T, diag, rowsig, colsig, g_loss.contiguous(), col0, soft_margin, alpha, margin)
            dx, dy = k.sqdist_rect_bwd(x, y, G, ctx.needs_input_grad[1], ctx.needs_input_grad[0])
        return dy, slab_loss.scatter_overhead_grad(dx, b, True), None, None, None, None


def sharded_exhaustive_loss(surface_local, overhead_local, soft_margin=False, alpha=10., margin=1., _kernels=None):
    """exhaustive_minibatch_triplet_loss (model/cvig_baseline.py:286-315) of the GLOBAL batch from this rank's b pairs: what the
    reference computes on the embeddings gathered from its nn.DataParallel replicas (:339-343), normaliser 2B(B-1) with the global
    B. Every rank must call it with the same b (else a WitwError, on every rank). Differentiable; identical on every rank. With no
    process group it is the same slab path at b = B. `_kernels` swaps the op set (CPU tests of the collective algebra)."""
    return _ShardedExhaustiveLossFn.apply(surface_local, overhead_local, bool(soft_margin), float(alpha), float(margin),
                                          _kernels or _slab_kernels())


LOSSES = ('exhaustive', 'batch_hard')      # train(loss=...) / --loss


def _hard_kernels():
    from types import SimpleNamespace
    from . import baseline_hard as bh
    return SimpleNamespace(pairwise_sqdist=ops.pairwise_sqdist, batch_hard_slab_mine=ops.batch_hard_slab_mine,
                           batch_hard_merge_rows=ops.batch_hard_merge_rows, hard_slab_loss=bh.hard_slab_loss, hard_pairs=bh.hard_pairs,
                           sqdist_pairs_bwd=bh.sqdist_pairs_bwd)


class _ShardedBatchHardLossFn(torch.autograd.Function):
    """The batch-hard form of the loss over the GLOBAL batch on the column-slab protocol of witw_amd.slab_loss: every anchor against
    its hardest negative only (minimum of its row / column of T with the diagonal masked; the mined indices are constants for the
    gradient). Exchanges: forward = all-gather of the overhead embeddings, of the diagonal (B floats) and of the per-rank row minima
    ([w,B] values + global column indices, merged in rank order: the lowest index wins a tie), all-reduce of the loss partial (each
    rank: the row terms of the anchors it owns + the column terms of its columns); backward = the at most 3b + B non-zeros of dL/dT in
    this rank's columns as a pair list through the pair-list backward of the distances (no dense [B,b] gradient), then the
    reduce-scatter of the overhead-embedding gradients. The surface gradients are complete locally. One rank runs the same kernels
    on the one slab b = B, col0 = 0, without a collective.
    Outputs: loss, and the mined (rv [B], ri [B]) of every overhead anchor and (cv [b], ci [b]) of this rank's surface anchors."""

    @staticmethod
    def forward(ctx, surface_local, overhead_local, soft_margin, alpha, margin, k, sharded):
        x, y, b, col0, B, world = slab_loss.open_slab(overhead_local, surface_local, who='sharded_batch_hard_loss', sharded=sharded)
        if B < 2:
            raise _lib.WitwError('sharded_batch_hard_loss: batch %d < 2 (every anchor needs a negative)' % B)
        with parallel.phase('slab_distances'):
            T = k.pairwise_sqdist(x, y)
        diag = slab_loss.gather_diagonal(T, col0, b, world > 1)
        rv, ri, cv, ci = slab_loss.mine_global(k, T, col0, world > 1)
        part = slab_loss.sum_partial(lambda: k.hard_slab_loss(T, rv, cv, col0, soft_margin, alpha, margin), world > 1)
        ctx.save_for_backward(x, y, diag, rv, ri, cv, ci)
        ctx.cfg = (col0, b, world, soft_margin, alpha, margin, k)
        ctx.mark_non_differentiable(rv, ri, cv, ci)
        ctx.set_materialize_grads(False)      # no zero gradients for the four non-differentiable outputs
        return (part / (2. * B)).reshape(()), rv, ri, cv, ci

    @staticmethod
    def backward(ctx, g_loss, *_g):
        if g_loss is None:
            return None, None, None, None, None, None, None
        x, y, diag, rv, ri, cv, ci = ctx.saved_tensors
        col0, b, world, soft_margin, alpha, margin, k = ctx.cfg
        with parallel.phase('slab_backward'):
            pg, pc, pw = k.hard_pairs(diag, rv, ri, cv, ci, g_loss.contiguous(), col0, soft_margin, alpha, margin)
            dx, dy = k.sqdist_pairs_bwd(x, y, pg, pc, pw, ctx.needs_input_grad[1], ctx.needs_input_grad[0])
        return dy, slab_loss.scatter_overhead_grad(dx, b, world > 1), None, None, None, None, None


def sharded_batch_hard_loss(surface_local, overhead_local, soft_margin=False, alpha=10., margin=1., mined=False, _kernels=None):
    """The batch-hard triplet loss of the GLOBAL batch from this rank's b pairs (not in the reference; Hermans et al. 2017 on the
    baseline's squared distances and its two margin forms): (sum_i l(d_i - min_{j != i} T_ij) + sum_j l(d_j - min_{i != j} T_ij)) / 2B
    with the global B >= 2, l as in exhaustive_minibatch_triplet_loss. Every rank must call it with the same b (else a WitwError, on
    every rank). Differentiable; identical on every rank. With no process group it is the same slab path at b = B. mined=True
    appends the mined (rv [B], ri [B], cv [b], ci [b]) of the global rows and this rank's columns (global int64 indices; a NaN is
    the minimum at the first NaN's index, else ties go to the lowest index). `_kernels` swaps the op set (CPU tests of the
    collective algebra)."""
    out = _ShardedBatchHardLossFn.apply(surface_local, overhead_local, bool(soft_margin), float(alpha), float(margin),
                                        _kernels or _hard_kernels(), True)
    return out if mined else out[0]


def batch_hard_triplet_loss(embed1, embed2, soft_margin=False, alpha=10., margin=1.):
    """exhaustive_minibatch_triplet_loss with every anchor against its hardest negative of the minibatch only, on one rank:
    the kernels of sharded_batch_hard_loss on the one slab b = B, whatever process group there is. Differentiable in both arguments."""
    return _ShardedBatchHardLossFn.apply(embed1, embed2, bool(soft_margin), float(alpha), float(margin), _hard_kernels(), False)[0]


def ranks(overhead_embed, surface_embed):
    """model/cvig_baseline.py:454-460: Euclidean distances, rank = #{gallery : d <= d_true}."""
    D = ops.pairwise_sqdist(overhead_embed.contiguous(), surface_embed.contiguous(), take_sqrt=True)   # [gallery, query]
    return ops.rank_count(D, 0).cpu().numpy().astype('int64')


# ----------------------------------------------------------------------------- gallery retrieval
DIRECT_ROWS = 65535      # gallery rows per ops.pairwise_sqdist call (its row index is gridDim.y)
GEMM_MARGIN = 32         # candidates kept beyond place k by the GEMM pass's top-k: one more slice of ops.topk_smallest
GEMM_FROM = _fov.SPECTRAL_FROM      # 'auto' is 'gemm' from this many queries on (measured against 'direct')

last_retrieve_stats = retrieval.last_retrieve_stats


def band_eps(n, gn_max, qn_max):
    """Half-width of the band around a squared threshold inside which a witw_sqdist_gemm value decides nothing. Worst case, not
    an observation; u = 2^-24, gamma_m = m u / (1 - m u), S = |g|^2 + |q|^2, s = |g - q|^2 <= 2 S:
      * the dot product, in any summation order:      |fl(g.q) - g.q| <= gamma_n |g||q| <= gamma_n S / 2, doubled: gamma_n S
      * the two norms, in any order:                  |gn + qn - S| <= gamma_n S
      * the epilogue's two additions (2 x dot exact): u (gn + qn) + u |result| <= 3 u S (1 + gamma_n)
        so |D - s| <= (2 gamma_n + 3 u (1 + gamma_n)) S; max(0, .) only moves D towards s >= 0
      * the exact kernel (difference, square, n/4 - 1 + 2 additions):  |s_x - s| <= gamma_(n/4+5) s <= 2 gamma_(n/4+5) S
      * the threshold fl(d_true^2), d_true = sqrtf(s_x):               within 3 u (1 + 3 u) of s_x <= 2 S (1 + gamma): 6.1 u S
      * two squares that sqrtf must not merge or swap (the comparison is on the rooted values, roots on the host may be an ulp
        off the kernel's):                                            4 u s <= 8 u S
    in all (2.5 n + 28) u S (1 + O(n u)) with S <= (gn_max + qn_max) / (1 - gamma_n) in the COMPUTED norms; for every n <= 12288
    that is below 3 gamma_(n+16) (gn_max + qn_max), which leaves the float32 rounding of eps and of the band kernel's own
    threshold - eps room as well."""
    m = (n + 16) * 2.0 ** -24
    return 3.0 * (m / (1.0 - m)) * (float(gn_max) + float(qn_max))


def _default_kernels():
    from types import SimpleNamespace
    from . import baseline_retrieval as br
    return SimpleNamespace(pairwise_sqdist=ops.pairwise_sqdist, rank_count_thresh=ops.rank_count_thresh, rank_count_band=ops.rank_count_band,
                           topk_smallest=ops.topk_smallest, row_sqnorm=br.row_sqnorm, sqdist_gemm=br.sqdist_gemm, sqdist_pairs=br.sqdist_pairs)


def _direct(kn, gallery, surface_all, shard_begin, query_chunk, k, want_ranks):
    return retrieval.sqdist_direct_pass(kn, DIRECT_ROWS, gallery, surface_all, _fov._NO_PRIOR, shard_begin, query_chunk, k, want_ranks)


def retrieve_topk(overhead_shard, surface_all, k=10, shard_begin=0, query_chunk=4096, method='gemm', _kernels=None):
    """The k nearest gallery rows of every query by Euclidean distance, ordered by (distance, gallery index): -> (distances f32
    [N,k], gallery indices int64 [N,k]) on the device, identical on every rank; see retrieve()."""
    return retrieve(overhead_shard, surface_all, k, shard_begin, query_chunk, method, _kernels, _want_ranks=False)[1:]


def retrieve(overhead_shard, surface_all, k=10, shard_begin=0, query_chunk=4096, method='gemm', _kernels=None, _want_ranks=True,
             _want_lists=True):
    """Ranks and top-k lists of cvig_baseline embeddings from ONE distance pass per query chunk, on the exchanges and re-scorings
    of witw_amd.retrieval that cvig_fov.retrieve runs its orientation search on: this rank holds overhead_shard = gallery rows [shard_begin, shard_begin + n)
    (any number per rank, including none), surface_all [N, E] is replicated, query q's true row is gallery row q.
    -> (ranks int64 [N] on the host = #{rows : d <= d_true}, distances f32 [N,k], gallery indices int64 [N,k] on the device,
    ordered by (distance, index)), identical on every rank. Distances are Euclidean, as ranks() returns them. 1 <= k <=
    ops.TOPK_MAX; places beyond the rows present are (+inf, -1).
    method='direct': ops.pairwise_sqdist (the difference form) over gallery blocks of at most DIRECT_ROWS rows feeding
    ops.rank_count_thresh / ops.topk_smallest (retrieval.sqdist_direct_pass); the shards' lists are merged by retrieval._merge_topk.
    method='gemm': |g|^2 + |q|^2 - 2 g.q on the fp32 MFMA (witw_sqdist_gemm), known to band_eps only; every decision inside that
    band is re-made on witw_sqdist_pairs, whose values are the direct kernel's bit for bit: rows within eps of d_true^2 are
    re-scored and compared as rooted values; ALL k + GEMM_MARGIN candidates per shard and query are re-scored and ordered
    exactly, and a query whose exact k-th distance is not strictly below sqrt(best squared distance outside the lists - eps)
    takes the direct pass. Ranks, indices AND listed distances equal method='direct' exactly. Lists of more than TOPK_MAX -
    GEMM_MARGIN places come from the direct pass, the ranks still from the GEMM pass.
    method='auto': 'gemm' from GEMM_FROM queries on. `_kernels` swaps the op set (CPU tests of the host pass)."""
    kn = _kernels or _default_kernels()
    retrieval.check_k(k)
    if method not in ('auto', 'direct', 'gemm'):
        raise _lib.WitwError("retrieve: method must be 'auto', 'direct' or 'gemm', got %r" % (method,))
    if overhead_shard.dim() != 2 or surface_all.dim() != 2 or overhead_shard.shape[1] != surface_all.shape[1]:
        raise _lib.WitwError('retrieve: need [rows, E] embeddings of one width, got %s and %s' % (tuple(overhead_shard.shape), tuple(surface_all.shape)))
    k = int(k)
    if method == 'auto':
        method = 'gemm' if surface_all.shape[0] >= GEMM_FROM else 'direct'
    gallery, surface_all = overhead_shard.contiguous(), surface_all.contiguous()
    ranks_out = v = i = None
    if method == 'gemm':
        lists = _want_lists and k + GEMM_MARGIN <= ops.TOPK_MAX
        done = _retrieve_gemm(kn, gallery, surface_all, k if lists else None, shard_begin, query_chunk, _want_ranks)
        if done is not None:
            ranks_out, v, i = done
            _want_ranks = False
            _want_lists = _want_lists and not lists
        # else: norms that are not finite admit no band -- the whole call is the direct pass
    if _want_ranks or _want_lists:
        counts, dv, di = _direct(kn, gallery, surface_all, shard_begin, query_chunk, k if _want_lists else None, _want_ranks)
        if _want_ranks:
            ranks_out = retrieval.host_ranks(counts)
        if _want_lists:
            v, i = dv, di
    return ranks_out, v, i


def _retrieve_gemm(kn, gallery, surface_all, k, shard_begin, query_chunk, want_ranks):
    """retrieve() on the GEMM pass (see there). k None: no lists. -> (ranks or None, values, indices), or None when some norm is
    not finite (decided on all-reduced data: the same on every rank)."""
    import torch.distributed as dist_
    dev = surface_all.device
    n_q, n_g, n = surface_all.shape[0], gallery.shape[0], surface_all.shape[1]
    if not want_ranks and k is None:
        return None, None, None
    gn = kn.row_sqnorm(gallery) if n_g else None
    qn_all = kn.row_sqnorm(surface_all) if n_q else torch.zeros((0,), dtype=torch.float32, device=dev)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    worst = torch.stack((gn.max() if n_g else zero, qn_all.max() if n_q else zero))
    if parallel.world() > 1:
        dist_.all_reduce(worst, op=dist_.ReduceOp.MAX)
    worst = worst.tolist()
    eps = getattr(kn, 'BAND_EPS', None)                  # an injected op set states the error of its own GEMM form
    eps = band_eps(n, worst[0], worst[1]) if eps is None else float(eps)
    if not (math.isfinite(worst[0]) and math.isfinite(worst[1]) and math.isfinite(eps)):
        return None
    kc = None if k is None else k + GEMM_MARGIN
    stats = {'method': 'gemm', 'pairs': float(n_g) * n_q, 'rescored_true': 0, 'rescored_rank': 0, 'rescored_topk': 0, 'fallback_queries': 0,
             'eps': eps}
    counts = torch.zeros((n_q,), dtype=torch.int32, device=dev)
    vals, idxs = [], []
    for q0 in range(0, n_q, query_chunk):
        q1 = min(n_q, q0 + query_chunk)
        nq = q1 - q0
        su = surface_all[q0:q1]
        D = kn.sqdist_gemm(gallery, su, gn, qn_all[q0:q1]) if n_g else None          # [n_g, nq], squared
        if want_ranks:
            exact = _exact_pairs(kn, gallery, su)
            d_true = retrieval.true_distances(exact, q0, q1, shard_begin, n_g, dev, stats)
            if n_g:   # squared thresholds; compared as ranks() compares: on the rooted exact values (sqrtf can merge neighbouring squares)
                counts[q0:q1] = retrieval.band_rescore(kn, D, (d_true * d_true).contiguous(), eps, exact, d_true, stats)
        if kc is not None:
            cv, ci = kn.topk_smallest(D, kc, shard_begin) if n_g else retrieval._empty_topk(nq, kc, dev)
            vals.append(cv)
            idxs.append(ci)
    ranks_out = v = i = None
    if want_ranks:
        parallel.all_reduce_sum_(counts)
        ranks_out = retrieval.host_ranks(counts)
    if kc is not None:
        if n_q:
            v, i = _settle_lists(kn, gallery, surface_all, k, shard_begin, query_chunk, eps, torch.cat(vals), torch.cat(idxs), stats)
        else:
            v, i = retrieval._empty_topk(0, k, dev)
    retrieval.publish_stats(retrieve, stats)
    return ranks_out, v, i


def _exact_pairs(kn, gallery, su):
    """witw_amd.retrieval's `exact_pairs` of the GEMM pass: the rooted distances of the pairs (pg, pq) of (gallery, su) through
    kn.sqdist_pairs -- the direct kernel's bits"""
    return lambda pg, pq: kn.sqdist_pairs(gallery, su, pg, pq, take_sqrt=True)


def _settle_lists(kn, gallery, surface_all, k, shard_begin, query_chunk, eps, v, i, stats):
    """The shards' candidate lists (v, i: [N, kc] by GEMM-form squared distance) -> the first k places as the direct pass lists
    them. Every gathered candidate is re-scored exactly (N kc pairs per shard: nothing next to the pass) and ordered by (exact
    distance, index). No row outside the lists has a GEMM-form value below `outsider`, the smallest last place of a full list, so
    its exact squared distance is >= outsider - eps and its rooted one >= sqrt(outsider - eps): a query whose exact k-th distance is
    strictly below that is settled, any other takes the direct pass."""
    _v, i, outsider = retrieval.gather_candidates(v, i, want_values=False)
    ev, ei = retrieval.rescore_candidates(_exact_pairs(kn, gallery, surface_all), i, None, shard_begin, gallery.shape[0], stats)
    beyond = torch.sqrt((outsider - eps).clamp(min=0))
    safe = (ev[:, min(k, ev.shape[1]) - 1] < beyond) | torch.isinf(outsider)
    ev, ei = ev[:, :k].contiguous(), ei[:, :k].contiguous()
    retrieval.fall_back(lambda q: _direct(kn, gallery, surface_all[q].contiguous(), shard_begin, query_chunk, k, False)[1:],
                        torch.nonzero(~safe).squeeze(1), ev, ei, k, stats)
    return ev, ei


def evaluation_ranks(overhead_embed, surface_embed, shard_begin=0, world=1, method='auto'):
    """The ranks test() tabulates, int64 [N] on the host, identical on every rank. `overhead_embed` / `surface_embed` are THIS
    rank's rows (world > 1: the queries are gathered, the gallery rows stay sharded from shard_begin on). method: 'direct',
    'gemm' (the same ranks, see retrieve) or 'auto' = 'gemm' from GEMM_FROM queries on. Unlike ranks() neither is bounded by
    65,535 gallery rows."""
    if method not in ('auto', 'direct', 'gemm'):         # refused before the gather
        raise _lib.WitwError("evaluation_ranks: method must be 'auto', 'direct' or 'gemm', got %r" % (method,))
    surface_all = parallel.all_gather_ragged(surface_embed) if world > 1 else surface_embed
    return retrieve(overhead_embed, surface_all, k=1, shard_begin=shard_begin, method=method, _want_lists=False)[0]


# ----------------------------------------------------------------------------- drivers
class GlobalBatchShares(object):
    """batch_sampler of the sharded validation phase: the n items go in order into global batches of `batch_size` (the last one
    ragged), exactly the batches of DataLoader(shuffle=False, drop_last=False), and this rank takes its contiguous
    parallel.shard_range share of each -- possibly none. parallel.all_gather_ragged of the ranks' shares is the global batch, in
    order; no item is padded in or repeated, as a DistributedSampler would."""

    def __init__(self, n, batch_size, rank, world):
        self.n, self.batch_size, self.rank, self.world = int(n), int(batch_size), int(rank), int(world)

    def __iter__(self):
        from . import parallel
        for i0 in range(0, self.n, self.batch_size):
            lo, hi = parallel.shard_range(min(self.batch_size, self.n - i0), self.rank, self.world)
            yield list(range(i0 + lo, i0 + hi))

    def __len__(self):
        return (self.n + self.batch_size - 1) // self.batch_size


def _embed_share(prep, surface_encoder, overhead_encoder, raw):
    """eval-mode embeddings of this rank's share of a batch; an empty share gives [0, 1536] tensors"""
    if (raw.n == 0) if isinstance(raw, _fov.StagedBatch) else (not raw.get('packed') and not raw['surface']):
        return torch.zeros((0, 1536), dtype=torch.float32, device=device), torch.zeros((0, 1536), dtype=torch.float32, device=device)
    data = prep(raw)
    with torch.no_grad():
        return surface_encoder(data['surface']), overhead_encoder(data['overhead'])


def _bn_modules(*encoders):
    return [getattr(e, 'bn%d' % i) for e in encoders for i in range(1, 8)]


def _data_path(who, data_path):
    data_path = Globals.data_path if data_path is None else data_path
    if data_path not in DATA_PATHS:
        raise _lib.WitwError("%s: data_path must be 'reference' or 'packed', got %r" % (who, data_path))
    return data_path


def _open_dataset(dataset, csv_path, packed):
    """'reference': the reference's float32 CHW tensors; 'packed': entropy-decoded JPEG files (Globals.device_jpeg) or the decoder's bytes"""
    if not packed:
        return ImagePairDataset(dataset=dataset, csv_path=csv_path)
    return ImagePairDataset(dataset=dataset, csv_path=csv_path, raw='jpeg' if Globals.device_jpeg else True,
                            jpeg_progressive=Globals.jpeg_progressive, jpeg_440=Globals.jpeg_440)


def _staging(dataset, data_set, loader_batch, num_workers, packed, n_loaders=1):
    """-> (GpuPreprocess, the DataLoaders' collate / pinning keywords, feed: loader -> what the driver iterates). 'packed': batches
    are built by collate_packed, in a pinned ring when there are workers (cvig_fov.make_staging), and staged one batch ahead on a
    copy stream (cvig_fov.DevicePrefetcher)"""
    if not packed:
        return GpuPreprocess(dataset), {'collate_fn': _fov.collate_raw}, lambda loader: loader
    import functools
    ring, _collate, pin = _fov.make_staging(data_set, loader_batch, num_workers, n_loaders=n_loaders)
    prep = GpuPreprocess(dataset, device=device, ring=ring)
    return prep, {'collate_fn': functools.partial(collate_packed, ring=ring), 'pin_memory': pin}, lambda loader: _fov.DevicePrefetcher(loader, prep)


def train(dataset='cvusa', val_quantity=1000, batch_size=16, num_workers=4, num_epochs=999999, csv_path=None, seed=0, loss='exhaustive',
          train_precision=None, sync_bn=None, data_path=None):
    """model/cvig_baseline.py:318-404 on the HIP kernels: same flow, prints and checkpoint names; Adam with torch's
    defaults (lr 1e-3) over every encoder parameter.
    Under an initialised process group (N ranks, one per GPU) it is the reference's nn.DataParallel run (:339-343) with a rank in
    the place of each replica: `batch_size` stays the GLOBAL batch (N must divide it), every rank draws batch_size / N pairs of each
    step from a DistributedSampler and normalises them with its OWN batch statistics, as a replica does; the loss couples the
    global batch (sharded_exhaustive_loss), the weight gradients are summed (parallel.OverlappedGradReducer). The running
    statistics that count are rank 0's (parallel.broadcast_buffers before every validation phase and before saving). Validation
    embeds each global batch in contiguous shares and evaluates the dense loss on the gathered batch, so its numbers are those of
    the one-process loop on the same split. Rank 0 prints and saves. `seed` fixes the train / validation split, which every rank
    must draw alike; it is not used on one rank. loss='batch_hard' (not in the reference) trains on every anchor's hardest negative
    of the global batch instead (batch_hard_triplet_loss / sharded_batch_hard_loss), and validation then evaluates that loss, so
    that "best" is judged by the loss that is trained. train_precision: None = Globals.train_precision; 'fp32', or 'bf16' = the training
    step runs blocks 2-4 on the bf16 MFMA (SurfaceEncoder(train_precision='bf16')) and the validation phase runs the encoders' eval forward
    with precision='bf16'. The same under N ranks; checkpoints are the fp32 master weights in either case. sync_bn: None = Globals.sync_bn;
    True = the BatchNorm layers of the training step normalise with the statistics of the GLOBAL batch instead (SurfaceEncoder(sync_bn=True):
    two all-reduces of 2C floats per layer and direction), so that the N-rank step is the one-process step at the same batch_size; the
    running statistics are then the same on every rank and "rank 0's are kept" holds trivially. On one rank it changes the summation
    order only. data_path: None = Globals.data_path; 'reference', or 'packed' = the loaders hand over packed byte blocks (device JPEG decode,
    pinned ring, DevicePrefetcher one batch ahead) and GpuPreprocess runs two launches per batch; the same images for the same torch seed."""
    import pathlib
    import time
    from . import parallel
    if loss not in LOSSES:
        raise _lib.WitwError("train: loss must be 'exhaustive' or 'batch_hard', got %r" % (loss,))
    train_precision = Globals.train_precision if train_precision is None else train_precision
    if train_precision not in TRAIN_PRECISIONS:
        raise _lib.WitwError("train: train_precision must be 'fp32' or 'bf16', got %r" % (train_precision,))
    sync_bn = bool(Globals.sync_bn if sync_bn is None else sync_bn)
    packed = _data_path('train', data_path) == 'packed'
    world, rank = parallel.world(), parallel.rank()
    if world > 1 and batch_size % world:
        raise _lib.WitwError('train: the global batch_size %d is not a multiple of the %d ranks' % (batch_size, world))
    if world > 1 and device.type == 'cuda':
        torch.cuda.set_device(device)
    pathlib.Path('./weights').mkdir(parents=True, exist_ok=True)
    csv_path = csv_path or Globals.dataset_paths[dataset]['train']
    trainval_set = _open_dataset(dataset, csv_path, packed)
    prep, loader_kw, feed = _staging(dataset, trainval_set, -(-batch_size // world), num_workers, packed, n_loaders=2)
    train_loader = val_loader = loader = None
    try:
        split_gen = torch.Generator().manual_seed(seed) if world > 1 else None      # every rank must draw the same split
        train_set, val_set = torch.utils.data.random_split(trainval_set, [len(trainval_set) - val_quantity, val_quantity],
                                                           generator=split_gen)
        if world > 1:
            train_sampler = torch.utils.data.distributed.DistributedSampler(train_set, shuffle=True, drop_last=True)
            train_loader = torch.utils.data.DataLoader(train_set, batch_size=batch_size // world, sampler=train_sampler, drop_last=True,
                                                       num_workers=num_workers, **loader_kw)
            val_loader = torch.utils.data.DataLoader(val_set, batch_sampler=GlobalBatchShares(len(val_set), batch_size, rank, world),
                                                     num_workers=num_workers, **loader_kw)
        else:
            train_sampler = None
            train_loader = torch.utils.data.DataLoader(train_set, batch_size=batch_size, shuffle=True, drop_last=True,
                                                       num_workers=num_workers, **loader_kw)
            val_loader = torch.utils.data.DataLoader(val_set, batch_size=batch_size, shuffle=False, drop_last=False,
                                                     num_workers=num_workers, **loader_kw)
        enc_kw = {'precision': 'bf16', 'train_precision': 'bf16'} if train_precision == 'bf16' else {'train_precision': 'fp32'}
        enc_kw['sync_bn'] = sync_bn
        surface_encoder = SurfaceEncoder(**enc_kw).to(device)
        overhead_encoder = OverheadEncoder(**enc_kw).to(device)
        encoders = [surface_encoder, overhead_encoder]
        parallel.broadcast_parameters(encoders)
        dense_loss, sharded_loss = {'exhaustive': (exhaustive_minibatch_triplet_loss, sharded_exhaustive_loss),
                                    'batch_hard': (batch_hard_triplet_loss, sharded_batch_hard_loss)}[loss]
        loss_func = sharded_loss if world > 1 else dense_loss
        optimizer = Adam(list(surface_encoder.parameters()) + list(overhead_encoder.parameters()))
        reducer = parallel.OverlappedGradReducer(encoders) if world > 1 else None      # SUM: the loss is normalised by the global batch

        def say(*a):
            if rank == 0:
                print(*a)

        best_loss = None
        for epoch in range(num_epochs):
            say('Epoch %d, %s' % (epoch + 1, time.ctime(time.time())))
            if train_sampler is not None:
                train_sampler.set_epoch(epoch)
            for phase in ['train', 'val']:
                running_count = 0
                running_loss = 0.
                loader = train_loader if phase == 'train' else val_loader
                surface_encoder.train(phase == 'train')
                overhead_encoder.train(phase == 'train')
                if phase == 'val':
                    parallel.broadcast_buffers(_bn_modules(*encoders))      # the first replica's running statistics
                for batch, raw in enumerate(feed(loader)):
                    if phase == 'val' and world > 1:
                        su, ov = _embed_share(prep, surface_encoder, overhead_encoder, raw)
                        surface_embed, overhead_embed = parallel.all_gather_ragged(su), parallel.all_gather_ragged(ov)
                        with torch.no_grad():
                            loss = dense_loss(surface_embed, overhead_embed)
                        count = surface_embed.size(0)
                    else:
                        data = prep(raw)
                        with torch.set_grad_enabled(phase == 'train'):
                            surface_embed = surface_encoder(data['surface'])
                            overhead_embed = overhead_encoder(data['overhead'])
                            loss = loss_func(surface_embed, overhead_embed)
                            if phase == 'train':
                                optimizer.zero_grad()
                                loss.backward()
                                if reducer is not None:
                                    reducer.wait()
                                optimizer.step()
                        count = surface_embed.size(0) * (world if phase == 'train' else 1)
                    running_count += count
                    running_loss += loss.item() * count
                    say('epoch = {} {}, iter = {}, count = {}, loss = {:.4f}'.format(epoch + 1, phase, batch, running_count,
                                                                                    loss.item()))
                say('  %5s: avg loss = %f' % (phase, running_loss / max(1, running_count)))
            if running_count and (best_loss is None or running_loss / running_count < best_loss):
                say('-------> new best')
                best_loss = running_loss / running_count
                if rank == 0:      # the running statistics are rank 0's own: nothing has trained since the broadcast before validation
                    torch.save(surface_encoder.state_dict(), './weights/surface_best.pth')
                    torch.save(overhead_encoder.state_dict(), './weights/overhead_best.pth')
        if reducer is not None:
            reducer.close()
        return best_loss
    finally:
        if prep.ring is not None:      # also when the loop raises: the workers go before the ring they build their batches in
            train_loader = val_loader = loader = None
            prep.ring.close()


def test(dataset='cvusa', batch_size=16, num_workers=4, csv_path=None, match_method=None, precision=None, data_path=None):
    """model/cvig_baseline.py:405-475: embed the test set (SyncedRotation stays on, as in the reference :410-414),
    rank every query against the whole gallery on the GPU, print the recall table. match_method: None = ranks() (one dense
    matrix, at most 65,535 pairs); 'direct', 'gemm' or 'auto' = evaluation_ranks(method=...): the same ranks from the chunked
    pass, 'gemm' at GEMM cost with exact re-scoring (retrieve). precision: the encoders' arithmetic ('fp32', 'bf16' or 'bf16_all'; None =
    Globals.precision), see SurfaceEncoder.
    Under an initialised process group every rank embeds a contiguous share of the test set and keeps its gallery rows; the
    queries are gathered and the rank counts summed inside evaluation_ranks, rank 0 prints. None then means 'auto': the dense
    ranks() cannot be sharded. data_path: as in train()."""
    from . import parallel
    packed = _data_path('test', data_path) == 'packed'
    world, rank = parallel.world(), parallel.rank()
    if world > 1 and device.type == 'cuda':
        torch.cuda.set_device(device)
    csv_path = csv_path or Globals.dataset_paths[dataset]['test']
    test_set = _open_dataset(dataset, csv_path, packed)
    prep, loader_kw, feed = _staging(dataset, test_set, batch_size, num_workers, packed)
    test_loader = None
    try:
        shard_begin, shard_end = parallel.shard_range(len(test_set))
        shard = torch.utils.data.Subset(test_set, range(shard_begin, shard_end)) if world > 1 else test_set
        test_loader = torch.utils.data.DataLoader(shard, batch_size=batch_size, shuffle=False, drop_last=False,
                                                  num_workers=num_workers, **loader_kw)
        surface_encoder = SurfaceEncoder(precision=precision).to(device)
        overhead_encoder = OverheadEncoder(precision=precision).to(device)
        surface_encoder.load_state_dict(torch.load('./weights/surface_best.pth', map_location='cpu'))
        overhead_encoder.load_state_dict(torch.load('./weights/overhead_best.pth', map_location='cpu'))
        surface_encoder.eval()
        overhead_encoder.eval()
        su_parts, ov_parts = [], []
        for raw in feed(test_loader):
            su, ov = _embed_share(prep, surface_encoder, overhead_encoder, raw)
            su_parts.append(su)
            ov_parts.append(ov)
    finally:
        if prep.ring is not None:      # also when the loop raises
            test_loader = None
            prep.ring.close()
    if world > 1 and not su_parts:      # a rank without rows (more ranks than items) still joins the collectives
        su, ov = _embed_share(prep, surface_encoder, overhead_encoder, {'surface': []})
        su_parts.append(su)
        ov_parts.append(ov)
    ov_all, su_all = torch.cat(ov_parts, dim=0), torch.cat(su_parts, dim=0)
    if world > 1:
        rk = evaluation_ranks(ov_all, su_all, shard_begin, world, method=match_method or 'auto')
    else:
        rk = ranks(ov_all, su_all) if match_method is None else evaluation_ranks(ov_all, su_all, method=match_method)
    t = recall_table(rk)
    if rank != 0:
        return t
    print('Top  1: {:.2f}%'.format(t['top_1']))
    print('Top  5: {:.2f}%'.format(t['top_5']))
    print('Top 10: {:.2f}%'.format(t['top_10']))
    print('Top 1%: {:.2f}%'.format(t['top_1pct']))
    print('Avg. Rank: {:.2f}'.format(t['mean']))
    print('Med. Rank: {:.2f}'.format(t['median']))
    print('Locations: {}'.format(len(rk)))
    return t


def main(argv=None):
    """CLI of model/cvig_baseline.py:478-492."""
    import argparse
    parser = argparse.ArgumentParser()
    parser.add_argument('--mode', default='train', choices=['train', 'test'], help='Run mode. [Default = train]')
    parser.add_argument('--dataset', default='cvusa', choices=['cvusa', 'witw'], help='Dataset to use. [Default = cvusa]')
    parser.add_argument('--match-method', default=None, choices=['direct', 'gemm', 'auto'],
                        help="Test mode: rank through evaluation_ranks -- 'direct' = the chunked difference-form pass, 'gemm' = the fp32 MFMA "
                             "distance GEMM with exact re-scoring (the same ranks), 'auto' = 'gemm' for large test sets. [Default = one dense "
                             "matrix, at most 65,535 pairs]")
    parser.add_argument('--loss', default='exhaustive', choices=list(LOSSES),
                        help='Train mode: exhaustive = every valid (anchor, positive, negative) of the global batch; batch_hard = every '
                             'anchor against its hardest negative of the global batch only. [Default = exhaustive]')
    parser.add_argument('--precision', default='fp32', choices=list(PRECISIONS),
                        help='Test mode: arithmetic of the encoders. fp32 = fp32 MFMA throughout (within 2e-5 of fp64); bf16 = blocks 1-4 '
                             '(86 %% of the multiply-adds) with bf16 operands and fp32 accumulation on the bf16 MFMA, blocks 5-7 and the '
                             'head in fp32 (embedding within 1e-2 of fp64, relative to its norm); bf16_all = the convolutions of blocks 5-7 on the '
                             'bf16 MFMA as well (split-K, fp32 sums; same bound). Not the training arithmetic: see --train-precision. '
                             '[Default = fp32]')
    parser.add_argument('--train-precision', default=None, choices=list(TRAIN_PRECISIONS),
                        help='Train mode: arithmetic of the training step. fp32 = fp32 MFMA throughout; bf16 = forward, data gradient and '
                             'weight gradient of blocks 2-4 with bf16 operands and fp32 accumulation (fp32 master weights, statistics and '
                             'gradients), validation with the bf16 eval forward. [Default = fp32]')
    parser.add_argument('--sync-bn', action='store_true',
                        help='Train mode on N ranks: BatchNorm statistics of the global batch (two small all-reduces per layer and '
                             'direction) instead of every rank normalising its own share as an nn.DataParallel replica does. '
                             '[Default = off]')
    parser.add_argument('--data-path', default=None, choices=list(DATA_PATHS),
                        help='How images reach the encoders: reference = workers decode into float32 tensors, one rotation per sample; '
                             'packed = workers only parse / entropy-decode, one byte block per side crosses PCIe, the GPU finishes the '
                             'decode and rotates / rolls the batch in two launches (the same images). [Default = reference]')
    args = parser.parse_args(argv)
    if args.mode != 'train' and args.train_precision is not None:
        parser.error("--train-precision belongs to --mode train")
    if args.mode != 'train' and args.sync_bn:
        parser.error("--sync-bn belongs to --mode train")
    if args.mode == 'train' and args.precision != 'fp32':
        parser.error("--precision %s is inference only: --mode train runs in fp32 (use it with --mode test)" % args.precision)
    _fov.init_distributed()       # under `python -m torch.distributed.run --nproc-per-node N`: one process per GPU; else nothing
    path = {} if args.data_path is None else {'data_path': args.data_path}      # only when the flag was given
    if args.mode == 'train':
        extra = {} if args.train_precision is None else {'train_precision': args.train_precision}      # only when the flag was given
        if args.sync_bn:
            extra['sync_bn'] = True
        train(dataset=args.dataset, loss=args.loss, **extra, **path)
    elif args.mode == 'test':
        test(dataset=args.dataset, match_method=args.match_method, precision=args.precision, **path)


if __name__ == '__main__':
    main()
