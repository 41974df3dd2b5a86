"""On-device JPEG decode for the data path: the reference decodes inside its DataLoader workers
(skimage.io.imread -> PIL -> libjpeg, model/cvig_fov.py:88-89, :402). Here a worker only ENTROPY-decodes
(libwitw_jpeg.so, csrc_host/jpeg_coef.cpp: Huffman decoding into quantised DCT coefficient blocks, about 40 % of libjpeg's
decode time); the coefficient blocks of a batch cross PCIe as one block and the GPU does the rest (csrc/jpeg.hip:
dequantisation, integer inverse DCT, fancy chroma upsampling, YCbCr -> RGB) into the same interleaved uint8 image Pillow
produces, byte for byte. Files this decoder leaves alone (progressive, arithmetic-coded, CMYK, 12-bit, unusual sampling) are
decoded by Pillow in the worker as before and travel as bytes in the same batch. Opt-in (PROGRESSIVE below): progressive
files are entropy-decoded by the worker too -- all their scans, into the blocks a sequential file would hold -- and take the same
route through the GPU; or (PROGRESSIVE_DEVICE below) the worker only writes a scan plan and the GPU decodes the scans itself, stage by
stage. Opt-in too (SAMPLING_440 below): 4:4:0 files (h1v2, e.g. a losslessly rotated 4:2:2 file) take every
route a 4:2:2 file takes.

Nothing here touches the GPU at import or in a worker: libwitw_jpeg.so is host-only C++."""
import ctypes
import os

import numpy as np
import torch

from . import build as _build

_HOST = None
KIND_JPEG = 2          # packed-batch kind: coefficient blocks (+ raw uint8 images for the files left to Pillow)
# The packed descriptor, one int64 row per image (pack() writes it, decode_tables / decode_packed_multi read it):
#   COL_OFFSET     0       byte offset of the entry in the block: coefficient blocks, FILE BYTES (COL_ON_DEVICE) or raw pixels (COL_RAW)
#   COL_QT         1       byte offset of the quantisation tables (64 uint16 per component)
#   COL_INFO       2..23   the INFO_INTS ints of witw_jpeg_info_ex (INFO_* below); a raw entry fills COL_H and COL_W only
#   COL_RAW        24      1: uint8 HWC pixels of a file left to Pillow
#   COL_CHANNELS   25      ... and their channels
#   COL_ON_DEVICE  26      1: entropy decoding on the device, the file bytes travelled; 2: the same for a PROGRESSIVE file (scan plan)
#   COL_PLAN       27      ... byte offset of the entropy plan (2: of the scan plan)
#   COL_FILE_LEN   28      ... file length
#   COL_INTERVALS  29      ... restart intervals (grid sizing of the device decoder); 2: what sizes the stage launches, in one int64:
#                          the largest segment count of a scan | scans << 32 | stages << 40 (prog_launch_sizes)
COL_OFFSET, COL_QT, COL_INFO = 0, 1, 2
COL_RAW, COL_CHANNELS, COL_ON_DEVICE, COL_PLAN, COL_FILE_LEN, COL_INTERVALS = 24, 25, 26, 27, 28, 29
DESC_COLS = 30
# the info ints and the plan header as csrc/jpeg_layout.h names them (WITW_JPEG_INFO_* / WITW_JPEG_PLAN_*: tests/test_jpeg.py compares)
INFO_H, INFO_W, INFO_NCOMP, INFO_HMAX, INFO_VMAX, INFO_BLOCKS = 0, 1, 2, 3, 4, 5
INFO_COMP, INFO_COMP_STRIDE = 6, 4            # component c: INFO_COMP + INFO_COMP_STRIDE * c + ...
INFO_COMP_H, INFO_COMP_V, INFO_COMP_BW, INFO_COMP_BH = 0, 1, 2, 3
INFO_INTS = 22
PLAN_INTERVALS = 1
# ... and of the scan plan of a progressive file ('JPW2'): header ints
PLAN_PROG_MAGIC = 0x3257504A
PLAN_PROG_SCANS, PLAN_PROG_SEGMENTS, PLAN_PROG_STAGES, PLAN_PROG_MAX_SEGMENTS, PLAN_PROG_BLOCKS, PLAN_PROG_BYTES = 1, 2, 27, 28, 29, 30
PLAN_PROG_MAX_SCANS, PLAN_PROG_MAX_STAGES = 64, 14
COL_H, COL_W = COL_INFO + INFO_H, COL_INFO + INFO_W
# Baseline / extended-sequential Huffman files are entropy-decoded ON THE DEVICE (round 6; csrc/jpeg.hip): with restart markers one GPU
# thread per restart interval (jpeg_huffman_kernel), without them a self-synchronising decode, one workgroup per file
# (jpeg_selfsync_kernel). The worker only parses the header and scans for markers; the file bytes cross PCIe instead of the
# coefficient blocks, and every launch covers all the files of a batch side (decode_packed_multi).
# Modes: 'all' (default) = every such file; disk -> embeddings with the bf16 encoders and FOUR loader workers: 16.1-16.4 k pairs/s on files
# with a restart marker every 1-2 MCUs, 14.9 k on ordinary files without markers -- 16 workers with host Huffman decoding reach 14.8 k on
# that box (11.5-15.0 k by box), the encoders alone 16.1-16.2 k; fp32 encoders 1,867 against 1,865 (profiles/r06_e2e_device_entropy_dev.json). 'restart' = only files with restart markers go to
# the device decoder, the others are Huffman-decoded in the worker; 'off' / False = host Huffman decoding for all.
# WITW_JPEG_DEVICE_ENTROPY = 0 | off | restart | 1 | all.
_mode = os.environ.get('WITW_JPEG_DEVICE_ENTROPY', 'all').lower()
DEVICE_ENTROPY = False if _mode in ('0', 'off', 'false') else 'restart' if _mode in ('restart', '1') else 'all'
# Progressive files (SOF2): off = left to Pillow in the worker (pixels cross PCIe); on = the worker decodes their scans into coefficient
# blocks (witw_jpeg_decode_coef_ex) and the GPU finishes them like any other file -- by the host-coefficient route, whatever
# DEVICE_ENTROPY says: the sequential device decoders do not apply to scans that refine one another. A file whose scans stop short of
# full precision stays Pillow's (libjpeg smooths it). WITW_JPEG_PROGRESSIVE = 1 | on | true; open_file / read_coef(progressive=...) override it.
PROGRESSIVE = os.environ.get('WITW_JPEG_PROGRESSIVE', '').lower() in ('1', 'on', 'true')
# Opt-in on top of that (implies taking progressive files): their scans are Huffman-decoded ON THE DEVICE too. A scan depends only on the
# earlier scans that coded the same (component, coefficient) cells, so the worker writes a scan plan (JpegFile.scan_plan: a byte scan,
# stages of mutually independent scans), the FILE BYTES travel, and one launch per stage decodes every progressive file of a batch side
# (csrc/jpeg_progressive.hip: a workgroup per scan, a thread per restart interval). Needs DEVICE_ENTROPY on; a file without a plan
# (more than 64 scans, illegal or incomplete scans) takes the host-coefficient route above, and through it Pillow.
# WITW_JPEG_PROGRESSIVE_DEVICE = 1 | on | true; open_file / read_coef(progressive='device') override it. What was measured: DESIGN.md §4.7.
PROGRESSIVE_DEVICE = os.environ.get('WITW_JPEG_PROGRESSIVE_DEVICE', '').lower() in ('1', 'on', 'true')
ACCEPT_PROGRESSIVE = 1     # flag bit 0 of witw_jpeg_info_ex / witw_jpeg_decode_coef_ex
# 4:4:0 files (h1v2: luma 1x2, chroma 1x1 -- a portrait photo turned losslessly from a 4:2:2 file): off = left to Pillow in the worker; on =
# taken like a 4:2:2 file, through whichever entropy route DEVICE_ENTROPY picks (the MCU is Y, Y below it, Cb, Cr; the plan tells the
# device decoders) and upsampling mode 5 of the back end (decode_tables). A progressive 4:4:0 file is taken only when PROGRESSIVE is on
# as well. WITW_JPEG_440 = 1 | on | true; open_file / read_coef(h1v2=...) override it.
SAMPLING_440 = os.environ.get('WITW_JPEG_440', '').lower() in ('1', 'on', 'true')
ACCEPT_H1V2 = 2            # flag bit 1 of the _ex entries of libwitw_jpeg.so
CHECK_ERRORS = True    # decode_packed(host_buf=...) re-decodes files the device flagged as damaged with Pillow (as the host path does)
REPAIRED = [0]         # how many files that happened to
SELFSYNC_MIN_BLOCKS = 96   # a marker-less file of at most this many blocks is decoded by ONE thread of the interval kernel (a 1024-thread
#                            workgroup would find nothing to split)
SELFSYNC_WIDE_BYTES = 48 * 1024   # a launch of the self-synchronising kernel that holds a file this large runs 1024 threads per file, else 512
_ERRORS = []           # error flags (device int32 tensors) of the last batches decoded on the device: entropy_errors() sums them


def host_lib():
    global _HOST
    if _HOST is None:
        path = _build.build_host(verbose=False)
        lib = ctypes.CDLL(path)
        ptr, size = ctypes.c_void_p, ctypes.c_size_t
        # every entry has an _ex twin that takes the flags (ACCEPT_*) as one more int; this module calls the twins only
        for name, res, args in (('witw_jpeg_info', ctypes.c_int, [ptr, size, ptr]),
                                ('witw_jpeg_decode_coef', ctypes.c_int, [ptr, size, ptr, ptr]),
                                ('witw_jpeg_entropy_plan_bytes', ctypes.c_longlong, [ptr, size]),
                                ('witw_jpeg_entropy_plan', ctypes.c_longlong, [ptr, size, ptr, size, ptr])):
            for fn, a in ((getattr(lib, name), args), (getattr(lib, name + '_ex'), args + [ctypes.c_int])):
                fn.restype, fn.argtypes = res, a
        # (the scan plan of a progressive file has the _ex form only)
        lib.witw_jpeg_scan_plan_bytes_ex.restype, lib.witw_jpeg_scan_plan_bytes_ex.argtypes = ctypes.c_longlong, [ptr, size, ctypes.c_int]
        lib.witw_jpeg_scan_plan_ex.restype, lib.witw_jpeg_scan_plan_ex.argtypes = ctypes.c_longlong, [ptr, size, ptr, size, ptr, ctypes.c_int]
        _HOST = lib
    return _HOST


class JpegCoef(object):
    """The entropy-decoded form of one JPEG file: info (the 22 ints of witw_jpeg_info), coef int16 [blocks, 64] (natural
    order, components one after another), qt uint16 [components, 64]."""
    __slots__ = ('info', 'coef', 'qt')

    def __init__(self, info, coef, qt):
        self.info, self.coef, self.qt = info, coef, qt

    @property
    def shape(self):          # of the decoded image, HWC
        return (int(self.info[INFO_H]), int(self.info[INFO_W]), int(self.info[INFO_NCOMP]))


class JpegFile(JpegCoef):
    """A JPEG file whose header has been parsed (info) but whose entropy-coded data is still to be decoded: pack() decodes it
    straight into its place in the batch block (no array of its own, no copy). `coef` / `qt` decode on demand. progressive: a
    progressive file (open_file(progressive=True)): all its scans are decoded on the host -- unless device_scans (a progressive file
    opened with progressive='device'): pack() then sends it to the device with a scan plan when it has one. flags: what the file
    was opened under (ACCEPT_PROGRESSIVE | ACCEPT_H1V2): the _ex entries take it again when the file is decoded or planned."""
    __slots__ = ('data', 'progressive', 'flags', 'device_scans')

    def __init__(self, info, data, progressive=False, flags=0, device_scans=False):
        self.info, self.data, self.progressive, self.flags = info, data, progressive, flags
        self.device_scans = bool(device_scans and progressive)

    def decode_into(self, coef, qt):
        """coef int16 [blocks, 64], qt uint16 [components, 64]: views of the destination. -> False if the entropy data is bad (or,
        progressive, its scans are illegal or stop short of full precision)."""
        return host_lib().witw_jpeg_decode_coef_ex(self.data.ctypes.data, self.data.size, coef.ctypes.data, qt.ctypes.data, self.flags) == 0

    def entropy_plan(self):
        """What the DEVICE needs to entropy-decode this file itself (csrc_host/jpeg_coef.cpp witw_jpeg_entropy_plan: header fields,
        Huffman tables, the byte offset of every restart interval) -> (plan uint8 array, qt uint16 [components, 64]), or None for a
        file without restart markers (or one this scheme leaves to the host: more than two tables of a kind, markers out of
        sequence, a progressive file). A byte scan of the file, no Huffman decoding."""
        if self.progressive:
            return None
        lib = host_lib()
        n = int(lib.witw_jpeg_entropy_plan_bytes_ex(self.data.ctypes.data, self.data.size, self.flags))
        if n <= 0:
            return None
        plan = np.empty((n,), dtype=np.uint8)
        qt = np.empty((int(self.info[INFO_NCOMP]), 64), dtype=np.uint16)
        if lib.witw_jpeg_entropy_plan_ex(self.data.ctypes.data, self.data.size, plan.ctypes.data, n, qt.ctypes.data, self.flags) != n:
            return None
        return plan, qt

    def scan_plan(self):
        """What the DEVICE needs to decode the scans of this PROGRESSIVE file itself (csrc_host/jpeg_coef.cpp witw_jpeg_scan_plan_ex:
        frame geometry, a record per scan with its stage, the Huffman tables in force at each scan, a record per restart interval of
        each scan) -> (plan uint8 array, qt uint16 [components, 64]), or None: not a progressive file, or one the plan writer leaves
        to the host route (more than PLAN_PROG_MAX_SCANS scans, illegal scan parameters or scan order, restart markers out of
        sequence, no EOI, scans that stop short of bit 0). A byte scan of the file, no Huffman decoding."""
        if not self.progressive:
            return None
        lib = host_lib()
        n = int(lib.witw_jpeg_scan_plan_bytes_ex(self.data.ctypes.data, self.data.size, self.flags))
        if n <= 0:
            return None
        plan = np.empty((n,), dtype=np.uint8)
        qt = np.empty((int(self.info[INFO_NCOMP]), 64), dtype=np.uint16)
        if lib.witw_jpeg_scan_plan_ex(self.data.ctypes.data, self.data.size, plan.ctypes.data, n, qt.ctypes.data, self.flags) != n:
            return None
        return plan, qt

    def pillow(self):
        """The host decoder's opinion of the file (what the reference's imread returns, model/cvig_fov.py:88-89): uint8 HWC.
        pack() takes it when the entropy data does not decode cleanly here -- libjpeg reads many damaged files with a warning."""
        import io
        from PIL import Image
        a = np.asarray(Image.open(io.BytesIO(self.data.tobytes())))
        return a[:, :, None] if a.ndim == 2 else a

    def _decoded(self):
        coef = np.empty((int(self.info[INFO_BLOCKS]), 64), dtype=np.int16)
        qt = np.empty((int(self.info[INFO_NCOMP]), 64), dtype=np.uint16)
        if not self.decode_into(coef, qt):
            raise ValueError('corrupt JPEG entropy data')
        return coef, qt

    coef = property(lambda self: self._decoded()[0])
    qt = property(lambda self: self._decoded()[1])


def open_file(src, progressive=None, h1v2=None):
    """src: a path or the bytes of a JPEG file -> JpegFile (header parsed, entropy decoding deferred to pack()), or None when the
    file is left to the host decoder. progressive: take progressive files too -- True: their scans are decoded in pack(), on the host;
    'device': on the device where the file has a scan plan (None: 'device' under the module flag PROGRESSIVE_DEVICE, else the module
    flag PROGRESSIVE); h1v2: take 4:4:0 files too (None: the module flag SAMPLING_440)."""
    data = np.fromfile(src, dtype=np.uint8) if isinstance(src, (str, os.PathLike)) else np.frombuffer(src, dtype=np.uint8)
    info = np.zeros(INFO_INTS, dtype=np.int32)
    if progressive is None:
        progressive = 'device' if PROGRESSIVE_DEVICE else PROGRESSIVE
    flags = (ACCEPT_PROGRESSIVE if progressive else 0) | (ACCEPT_H1V2 if (SAMPLING_440 if h1v2 is None else h1v2) else 0)
    rc = host_lib().witw_jpeg_info_ex(data.ctypes.data, data.size, info.ctypes.data, flags)      # (1: a progressive file, only under its flag)
    return JpegFile(info, data, progressive=rc == 1, flags=flags, device_scans=progressive == 'device') if rc in (0, 1) else None


def read_coef(src, progressive=None, h1v2=None):
    """src: a path or the bytes of a JPEG file -> JpegCoef, or None when the file is left to the host decoder. progressive, h1v2: as
    open_file."""
    f = open_file(src, progressive, h1v2)
    if f is None:
        return None
    coef = np.empty((int(f.info[INFO_BLOCKS]), 64), dtype=np.int16)
    qt = np.empty((int(f.info[INFO_NCOMP]), 64), dtype=np.uint16)
    if not f.decode_into(coef, qt):
        return None               # truncated / corrupt entropy data: let the host decoder say what it thinks of the file
    return JpegCoef(f.info, coef, qt)


def plan_intervals(plan):
    """The restart intervals of an entropy plan (uint8 array, JpegFile.entropy_plan): header int PLAN_INTERVALS; 1 = a file without
    restart markers."""
    return int(plan[4 * PLAN_INTERVALS:4 * PLAN_INTERVALS + 4].view(np.int32)[0])


def prog_launch_sizes(plan):
    """What sizes the stage launches of a progressive file, from its scan plan (uint8 array, JpegFile.scan_plan), as ONE int64 (the
    descriptor's COL_INTERVALS of such a file): the largest segment count of a scan | scans << 32 | stages << 40."""
    h = plan[:128].view(np.int32)
    return int(h[PLAN_PROG_MAX_SEGMENTS]) | (int(h[PLAN_PROG_SCANS]) << 32) | (int(h[PLAN_PROG_STAGES]) << 40)


def _shared_bytes(n):
    """n bytes of shared memory as a uint8 tensor: a DataLoader worker's batch block is built in place where the parent process
    will read it (torch would otherwise copy every tensor of a batch into shared memory when it pickles it)."""
    return torch.empty((n,), dtype=torch.uint8).share_memory_() if n else torch.empty((0,), dtype=torch.uint8)


def pack(images, shared=False, alloc=None):
    """A list of JpegCoef / JpegFile (and, for files left to Pillow, uint8 HWC arrays) -> (uint8 tensor, int64 [B, DESC_COLS],
    KIND_JPEG): one contiguous block for the pinned copy, images 128-byte aligned, the quantisation tables behind the coefficient
    data. JpegFile entries are entropy-decoded HERE, straight into the block. shared: allocate the block in shared memory;
    alloc(nbytes) -> (offset, uint8 numpy view) or None: build the block in caller-provided memory (ring.PinnedRing), in which
    case the first result is (offset, nbytes) instead of a tensor."""
    desc, off, spans = np.zeros((len(images), DESC_COLS), dtype=np.int64), 0, []
    plans, prog = {}, set()
    for i, a in enumerate(images):
        if DEVICE_ENTROPY and isinstance(a, JpegFile):
            if a.progressive:
                # opened for the device (open_file(progressive='device')) and planned: the stage launches; else the host decodes its scans below
                pl = a.scan_plan() if a.device_scans else None
                if pl is not None:
                    plans[i] = pl
                    prog.add(i)
            else:
                pl = a.entropy_plan()
                # (a plan of ONE interval = a file without restart markers: the self-synchronising kernel, mode 'all' only)
                if pl is not None and (DEVICE_ENTROPY in ('all', True) or plan_intervals(pl[0]) > 1):
                    plans[i] = pl
        if i in plans:
            # entropy decoding on the device: the FILE BYTES travel (24 readable bytes behind the end: the kernel reads aligned 8-byte
            # words one ahead of the one it decodes)
            nbytes = int(a.data.size) + 24
            desc[i, COL_INFO:COL_RAW] = a.info
            desc[i, COL_ON_DEVICE], desc[i, COL_FILE_LEN] = 2 if i in prog else 1, int(a.data.size)
            desc[i, COL_INTERVALS] = prog_launch_sizes(plans[i][0]) if i in prog else plan_intervals(plans[i][0])
        elif isinstance(a, JpegCoef):
            nbytes = int(a.info[INFO_BLOCKS]) * 128
            desc[i, COL_INFO:COL_RAW] = a.info
        else:
            a = np.ascontiguousarray(a)
            if a.dtype != np.uint8 or a.ndim != 3:
                raise ValueError('jpeg.pack takes JpegCoef / JpegFile objects and uint8 HWC arrays')
            nbytes = a.size
            desc[i, COL_H], desc[i, COL_W], desc[i, COL_RAW], desc[i, COL_CHANNELS] = a.shape[0], a.shape[1], 1, a.shape[2]
        desc[i, COL_OFFSET] = off
        spans.append((off, nbytes))
        # every entry starts on a 128-byte boundary: the device back end addresses coefficient data in 128-byte BLOCKS from the start
        # of the buffer (decode_tables: first block = offset // 128), so a raw image of a file left to Pillow in front of a JPEG
        # entry must not push it off that grid (round 4: it did -- 16-byte alignment -- and such a batch decoded its later JPEG
        # entries from up to 112 bytes too early)
        off += (nbytes + 127) // 128 * 128
    for i, a in enumerate(images):
        if isinstance(a, JpegCoef):
            desc[i, COL_QT] = off
            off += (int(a.info[INFO_NCOMP]) * 128 + 15) // 16 * 16
    for i in plans:
        desc[i, COL_PLAN] = off
        off += (plans[i][0].size + 15) // 16 * 16
    if alloc is not None:
        got = alloc(off)
        if got is None:
            return None
        t, buf = (got[0], off), got[1]
    else:
        t = _shared_bytes(off) if shared else torch.empty((off,), dtype=torch.uint8)
        buf = t.numpy()
    for i, a in enumerate(images):
        o, nbytes = spans[i]
        qt_at = int(desc[i, COL_QT])
        if i in plans:
            plan, qt = plans[i]
            buf[o:o + a.data.size] = a.data
            buf[o + a.data.size:o + nbytes] = 0
            buf[int(desc[i, COL_PLAN]):int(desc[i, COL_PLAN]) + plan.size] = plan
            buf[qt_at:qt_at + qt.size * 2] = qt.reshape(-1).view(np.uint8)
        elif isinstance(a, JpegFile):
            coef = buf[o:o + nbytes].view(np.int16).reshape(-1, 64)
            qt = buf[qt_at:qt_at + int(a.info[INFO_NCOMP]) * 128].view(np.uint16).reshape(-1, 64)
            if not a.decode_into(coef, qt):
                # damaged entropy data: the file goes to Pillow after all (as the reference and raw=True read it) and rides in the
                # same span as a raw uint8 image -- the coefficient blocks of an image are never smaller than its pixels
                px = np.ascontiguousarray(a.pillow())
                if px.dtype != np.uint8 or px.size > nbytes:
                    raise ValueError('image %d of the batch: JPEG entropy data is corrupt and the host decoder returned %s %s'
                                     % (i, px.dtype, px.shape))
                buf[o:o + px.size] = px.reshape(-1)
                desc[i, COL_INFO:COL_RAW] = 0
                desc[i, COL_H], desc[i, COL_W], desc[i, COL_RAW], desc[i, COL_CHANNELS] = px.shape[0], px.shape[1], 1, px.shape[2]
        elif isinstance(a, JpegCoef):
            buf[o:o + nbytes] = a.coef.reshape(-1).view(np.uint8)
            buf[qt_at:qt_at + a.qt.size * 2] = a.qt.reshape(-1).view(np.uint8)
        else:
            buf[o:o + nbytes] = np.ascontiguousarray(a).reshape(-1)
    return t, torch.from_numpy(desc), KIND_JPEG


def decode_tables(d):
    """The launch tables of the device back end from the host descriptor rows of the JPEG entries of a batch (d: int64 [n, DESC_COLS],
    none of them raw) -> (planes int64 [P, 6] = {first coefficient block, quantisation table index, byte offset of the plane in the
    component buffer, blocks wide, blocks high, first block of the plane in the launch}, images int64 [n, 12] = {H, W, components,
    upsampling mode (0 none, 1 h2v1, 2 h2v2, 3 / 4 those two replicated, 5 h1v2 = 4:4:0), luma plane offset, luma pitch, Cb offset, Cr offset, chroma pitch, chroma rows, chroma columns, output byte
    offset}, blocks in all, component bytes, output bytes, byte offset of the first quantisation table). Whole-array numpy: a
    per-image Python loop here cost 8 ms per 128 pairs, as much as the bf16 encoders take for them."""
    n = d.shape[0]
    if (d[:, COL_OFFSET] % 128).any():
        raise ValueError('jpeg: a coefficient entry does not start on a 128-byte boundary of the packed block')
    H, W, ncomp, hmax, vmax = (d[:, COL_INFO + k] for k in (INFO_H, INFO_W, INFO_NCOMP, INFO_HMAX, INFO_VMAX))
    qt_base = int(d[:, COL_QT].min())
    comp = COL_INFO + INFO_COMP + INFO_COMP_STRIDE * np.arange(3)      # first column of each component's record
    bw, bh = d[:, comp + INFO_COMP_BW], d[:, comp + INFO_COMP_BH]
    valid = np.arange(3)[None, :] < ncomp[:, None]
    nb = bw * bh * valid                                                  # blocks per (image, component)
    cb = (d[:, COL_OFFSET] // 128)[:, None] + np.cumsum(nb, axis=1) - nb             # coefficient blocks are 128 bytes
    flat = nb[valid]
    blk_off = np.cumsum(flat) - flat                                      # image-major, component-minor
    plane_first = np.zeros((n, 3), dtype=np.int64)
    plane_first[valid] = blk_off
    qti = ((d[:, COL_QT] - qt_base) // 128)[:, None] + np.arange(3)[None, :]
    planes = np.stack([cb[valid], qti[valid], blk_off * 64, bw[valid], bh[valid], blk_off], axis=1).astype(np.int64)
    # (1, 2) = 4:4:0, taken only as the host parser describes such a file -- the luma component itself sampled 1 x 2 (its INFO_COMP_H, INFO_COMP_V); a row
    # that claims the sampling without it was not written by witw_jpeg_info_ex
    is_440 = (hmax == 1) & (vmax == 2) & (d[:, comp[0] + INFO_COMP_H] == 1) & (d[:, comp[0] + INFO_COMP_V] == 2)
    mode = np.where((hmax == 1) & (vmax == 1), 0, np.where((hmax == 2) & (vmax == 1), 1, np.where((hmax == 2) & (vmax == 2), 2,
                                                                                                  np.where(is_440, 5, -1))))
    if (mode < 0).any():
        i = int(np.nonzero(mode < 0)[0][0])
        raise ValueError('jpeg: sampling %dx%d reached the device path' % (int(hmax[i]), int(vmax[i])))
    cw, ch = -(-W // hmax), -(-H // vmax)
    # libjpeg replicates chroma planes of at most two columns instead of filtering them -- where it would filter HORIZONTALLY: the
    # vertical-only h1v2 filter runs on planes of any size (jdsample.c jinit_upsampler)
    mode = mode + 2 * ((mode > 0) & (mode < 3) & (cw <= 2))
    images = np.zeros((n, 12), dtype=np.int64)
    images[:, 0], images[:, 1], images[:, 2], images[:, 3] = H, W, ncomp, mode
    images[:, 4], images[:, 5] = plane_first[:, 0] * 64, bw[:, 0] * 8
    c3 = ncomp == 3
    images[c3, 6], images[c3, 7], images[c3, 8] = plane_first[c3, 1] * 64, plane_first[c3, 2] * 64, bw[c3, 1] * 8
    images[c3, 9], images[c3, 10] = ch[c3], cw[c3]
    ob = (H * W * ncomp + 15) // 16 * 16
    images[:, 11] = np.cumsum(ob) - ob
    return planes, images, int(flat.sum()), int(flat.sum()) * 64, int(ob.sum()), qt_base


def _decode_group(dev, d, coef_ptr, qt_ptr):
    """dequantisation + inverse DCT + upsampling + colour conversion of the JPEG entries d (descriptor rows whose COL_OFFSET is the
    byte offset of their coefficient blocks from coef_ptr, COL_QT that of their quantisation tables from qt_ptr) -> (tensors to keep
    alive, device address of every decoded image, components per image). Two launches."""
    from . import _lib, ops
    try:
        planes, images, blk, pbytes, obytes, qt_base = decode_tables(d)
    except ValueError as e:
        raise _lib.WitwError(str(e))
    plane_t = torch.from_numpy(planes).pin_memory().to(dev, non_blocking=True)
    image_t = torch.from_numpy(images).pin_memory().to(dev, non_blocking=True)
    comp = torch.empty((pbytes,), dtype=torch.uint8, device=dev)
    rgb = torch.empty((obytes,), dtype=torch.uint8, device=dev)
    lib = _lib.load()
    st = ops._stream()
    _lib.check(lib.witw_jpeg_idct(coef_ptr, qt_ptr + qt_base, plane_t.data_ptr(), planes.shape[0], blk, comp.data_ptr(), st), 'witw_jpeg_idct')
    _lib.check(lib.witw_jpeg_to_rgb(comp.data_ptr(), image_t.data_ptr(), int(d.shape[0]), int((images[:, 0] * images[:, 1]).max()),
                                    rgb.data_ptr(), st), 'witw_jpeg_to_rgb')
    return [plane_t, image_t, comp, rgb], rgb.data_ptr() + images[:, 11], images[:, 2]


def _rebase(parts):
    """The descriptor rows of all parts as one table whose byte offsets (COL_OFFSET, COL_QT, COL_PLAN) count from the LOWEST block
    (allocations are 512-byte aligned) -> (address of that block, rows int64 [sum B, DESC_COLS], part of each row, each row's
    COL_OFFSET within its own part)."""
    from . import _lib
    ref = min(int(p[0].data_ptr()) for p in parts)
    ds, part_of, off0 = [], [], []
    for k, (dbuf, desc, _hb) in enumerate(parts):
        dk = np.array(desc.numpy() if isinstance(desc, torch.Tensor) else desc, dtype=np.int64, copy=True)
        delta = int(dbuf.data_ptr()) - ref
        if delta % 128:
            # the back end addresses coefficient blocks and quantisation tables on a 128-byte grid from the lowest block
            # (decode_tables): a part off that grid would decode with another file's tables
            raise _lib.WitwError('jpeg: part %d of the batch sits %d bytes from the lowest, not a multiple of 128' % (k, delta))
        off0.append(dk[:, COL_OFFSET].copy())
        for c in (COL_OFFSET, COL_QT, COL_PLAN):
            dk[:, c] += delta
        ds.append(dk)
        part_of.append(np.full((dk.shape[0],), k, dtype=np.int64))
    return ref, np.concatenate(ds), np.concatenate(part_of), np.concatenate(off0)


def _entropy_launch(dev, rows, launch, errors, at, keep):
    """One launch of a device entropy decoder: rows (int64, one per file) go up through pinned memory, launch(address of the row table,
    files, address of their int32 damage flags) runs the kernel, and the flags land at positions `at` of `errors` -- written there
    directly when the launch holds every file of `errors`."""
    files_t = torch.from_numpy(np.ascontiguousarray(rows)).pin_memory().to(dev, non_blocking=True)
    e = errors if at.size == errors.numel() else torch.zeros((int(at.size),), dtype=torch.int32, device=dev)
    launch(files_t.data_ptr(), int(at.size), e.data_ptr())
    if e is not errors:
        errors[torch.from_numpy(at).to(dev)] = e
    keep += [files_t, e]


def _entropy_decode(dev, d, ref, keep):
    """Entropy decoding on the device of the entries d that travelled as file bytes (offsets from ref) -> (coef int16: the files'
    coefficient blocks one after another, first block of each file, errors int32 per file). Files with restart markers: one thread
    per interval; files without (ONE interval of more than SELFSYNC_MIN_BLOCKS blocks): the self-synchronising kernel, one workgroup
    per file; progressive files (COL_ON_DEVICE 2): one launch per stage of their scan plans. All write into the one zero-filled
    coefficient buffer and the one flag per file."""
    from . import _lib, ops
    lib, st = _lib.load(), ops._stream()
    blocks = d[:, COL_INFO + INFO_BLOCKS]
    first = np.cumsum(blocks) - blocks
    coef = torch.zeros((int(blocks.sum()) * 64,), dtype=torch.int16, device=dev)
    errors = torch.zeros((d.shape[0],), dtype=torch.int32, device=dev)
    prog = d[:, COL_ON_DEVICE] == 2
    sync = ~prog & (d[:, COL_INTERVALS] == 1) & (blocks > SELFSYNC_MIN_BLOCKS)
    rows = np.stack([ref + d[:, COL_OFFSET], ref + d[:, COL_PLAN], coef.data_ptr() + first * 128, d[:, COL_FILE_LEN]], axis=1).astype(np.int64)
    ir, isy, ipg = np.nonzero(~sync & ~prog)[0], np.nonzero(sync)[0], np.nonzero(prog)[0]
    if ipg.size:
        # progressive files: one launch per stage over all of them, in order on the stream -- the only synchronisation between stages
        sizes = d[ipg, COL_INTERVALS]
        segs, scans, stages = int((sizes & 0xffffffff).max()), int(((sizes >> 32) & 0xff).max()), int(((sizes >> 40) & 0xff).max())

        def launch(files, n, err):
            for stage in range(stages):
                _lib.check(lib.witw_jpeg_progressive_stage(files, n, stage, scans, segs, err, st), 'witw_jpeg_progressive_stage')
        _entropy_launch(dev, rows[ipg], launch, errors, ipg, keep)
    if ir.size:
        most = int(d[ir, COL_INTERVALS].max())
        _entropy_launch(dev, rows[ir], lambda files, n, err: _lib.check(lib.witw_jpeg_huffman(files, n, most, err, st), 'witw_jpeg_huffman'),
                        errors, ir, keep)
    if isy.size:
        sizes = (d[isy, COL_FILE_LEN] + 32 + 7) // 8 * 8
        soff = np.cumsum(sizes) - sizes
        scratch = torch.empty((int(sizes.sum()),), dtype=torch.uint8, device=dev)
        srows = np.concatenate([rows[isy], (scratch.data_ptr() + soff)[:, None], np.zeros((isy.size, 1), np.int64)], axis=1).astype(np.int64)
        # threads per file: 1024 when the launch holds a large file (shorter subsequences: 113 KB files 1.3 against 1.4 ms per 128 at
        # 512 threads), 512 otherwise (22 KB files: 0.76 against 0.89 ms -- more rounds than the shorter subsequences save)
        env_t = os.environ.get('WITW_SELFSYNC_THREADS')
        threads = (1024 if int(env_t) >= 1024 else 512 if int(env_t) >= 512 else 256) if env_t else \
            (1024 if int(d[isy, COL_FILE_LEN].max()) >= SELFSYNC_WIDE_BYTES else 512)
        _entropy_launch(dev, srows, lambda files, n, err: _lib.check(lib.witw_jpeg_huffman_selfsync_threads(files, n, threads, err, st),
                                                                     'witw_jpeg_huffman_selfsync_threads'), errors, isy, keep)
        keep.append(scratch)
    return coef, first, errors


def _deferred_repair(dev, parts, d, part_of, off0, dv, errors, table, keep):
    """A file whose entropy-coded data is damaged is read by the reference through libjpeg, which recovers what it can (with a
    warning); the host path hands such a file to Pillow inside pack(). On the device the damage shows only once the kernel has run:
    queue a copy of the flags (4 bytes per file; it waits for THIS stream's staging work, which the drivers run on the copy stream one
    batch ahead of the encoders) -> finish(): waits for it -- the one host wait -- and lets Pillow decode the flagged files from the
    bytes that are still in the host block -- the same image, by the same decoder, as on the host path -- patching `table` in place."""
    flags_host = torch.empty((int(dv.size),), dtype=torch.int32).pin_memory()
    flags_host.copy_(errors, non_blocking=True)
    flags_ready = torch.cuda.Event()
    flags_ready.record(torch.cuda.current_stream(dev))

    def finish():
        flags_ready.synchronize()
        for j in np.nonzero(flags_host.numpy())[0]:
            i = int(dv[j])
            hb = parts[int(part_of[i])][2]
            if hb is None:
                continue
            hb = hb.numpy() if isinstance(hb, torch.Tensor) else np.asarray(hb)
            px = np.array(JpegFile(None, hb[int(off0[i]):int(off0[i]) + int(d[i, COL_FILE_LEN])]).pillow())      # a writable copy (from_numpy warns on Pillow's read-only view)
            t = torch.from_numpy(px).to(dev)
            keep.append(t)
            table[i] = (t.data_ptr(), px.shape[0], px.shape[1], 0, px.shape[2])
            REPAIRED[0] += 1
    return finish


def decode_packed_multi(parts, defer=False):
    """parts: [(dbuf, desc, host_buf or None), ...] = the packed blocks of ONE side of a batch, each on the GPU with its HOST descriptor
    table (a batch arrives in pieces when the loader hands out quarter batches: DevicePrefetcher(group=4)) -> (tensors to keep alive,
    int64 host table [sum B, 5] = {device address, H, W, 0, channels} of the decoded uint8 HWC images in part order: the descriptor
    rows of witw_resize_bilinear_normalize_batched / witw_polar_from_raw, kind 1, finish).
    EVERY LAUNCH COVERS THE FILES OF ALL PARTS (the descriptor rows carry addresses, so the blocks need not be one allocation): two
    launches for the entries whose coefficient blocks came from the host; for the entries that travelled as file bytes (DEVICE_ENTROPY)
    one or two more in front entropy-decode them into a coefficient buffer on the device -- a thread's chain of symbols bounds
    jpeg_huffman_kernel, so four launches over 32 files each take four times as long as one over 128.
    finish: None, or (defer=True, some part came with its host block) a callable that reads the damage flags of the device decoder --
    the one host wait of the call -- and lets Pillow re-decode flagged files, patching `table` in place; with defer=False that has
    happened on return."""
    dev = parts[0][0].device
    ref, d, part_of, off0 = _rebase(parts)
    table = np.zeros((d.shape[0], 5), dtype=np.int64)
    keep, finish = [], None
    is_raw = d[:, COL_RAW] != 0
    on_dev = (d[:, COL_ON_DEVICE] != 0) & ~is_raw
    table[:, 1], table[:, 2] = d[:, COL_H], d[:, COL_W]
    table[is_raw, 0] = ref + d[is_raw, COL_OFFSET]
    table[is_raw, 4] = d[is_raw, COL_CHANNELS]
    jp = np.nonzero(~is_raw & ~on_dev)[0]
    if jp.size:
        k, addr, ncomp = _decode_group(dev, d[jp], ref, ref)
        keep += k
        table[jp, 0], table[jp, 4] = addr, ncomp
    dv = np.nonzero(on_dev)[0]
    if dv.size:
        dd = d[dv]
        coef, first, errors = _entropy_decode(dev, dd, ref, keep)
        dd[:, COL_OFFSET] = first * 128                          # where each file's coefficient blocks sit in `coef`
        k, addr, ncomp = _decode_group(dev, dd, coef.data_ptr(), ref)
        keep += k + [coef, errors]
        table[dv, 0], table[dv, 4] = addr, ncomp
        _ERRORS.append(errors)
        del _ERRORS[:-64]
        if CHECK_ERRORS and any(p[2] is not None for p in parts):
            finish = _deferred_repair(dev, parts, d, part_of, off0, dv, errors, table, keep)
    if finish is not None and not defer:
        finish()
        finish = None
    return keep, torch.from_numpy(table), finish


def decode_packed(dbuf, desc, host_buf=None):
    """One packed block: decode_packed_multi([(dbuf, desc, host_buf)]) -> (tensors to keep alive, table); damaged files repaired on
    return."""
    keep, table, _f = decode_packed_multi([(dbuf, desc, host_buf)])
    return keep, table


def entropy_errors():
    """Files of the last (up to 64) device-entropy-decoded batches whose entropy-coded data was damaged (the host path hands such a
    file to Pillow; on the device it decodes with zeros from the damage on and is counted here). Synchronises."""
    n = sum(int((e != 0).sum().item()) for e in _ERRORS)
    return n


def decode(images, device):
    """Decode a list of JpegCoef (or uint8 HWC arrays, passed through) on `device` -> list of uint8 HWC tensors (tests and
    one-off use; the data path goes through pack / decode_packed inside GpuPreprocess)."""
    buf, desc, _k = pack(images)
    dbuf = buf.to(device)
    keep, table = decode_packed(dbuf, desc, host_buf=buf)      # files the device flags as damaged: Pillow, as on the data path
    torch.cuda.synchronize(device)
    out = []
    for i in range(len(images)):
        H, W, C = int(table[i, 1]), int(table[i, 2]), int(table[i, 4])
        src = next(t for t in [dbuf] + keep if t.dtype == torch.uint8 and t.data_ptr() <= int(table[i, 0]) < t.data_ptr() + max(1, t.numel())
                   and int(table[i, 0]) + H * W * C <= t.data_ptr() + t.numel() and (t is dbuf) == bool(desc[i, COL_RAW]))
        o = int(table[i, 0]) - src.data_ptr()
        out.append(src.reshape(-1)[o:o + H * W * C].reshape(H, W, C).clone())      # (a repaired image is an H x W x C tensor)
    return out
