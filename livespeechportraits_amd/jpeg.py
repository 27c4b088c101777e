"""The JPEG writer of demo.py's frame loop on the device (demo.py:268-272 -> util/visualizer.py:120-136 save_images ->
util/util.py:70-72 ``Image.fromarray(img).save(path)`` with a ``.jpg`` name).

``JpegEncoder`` encodes batches of uint8 device frames with ``lspjpeg_encode`` (include/lspjpeg.h) and hands back complete
files as ``bytes``: for the same pixels they are the bytes Pillow writes with its defaults (quality 75, baseline, 4:2:0,
standard Huffman tables, JFIF header).  Only the compressed bytes cross PCIe: the per-frame sizes are copied first, then
each frame's bytes.  There is no CPU path.

``JpegOptions`` carries Pillow's other two baseline switches, byte for byte Pillow's as well: ``optimize`` (per-frame optimal Huffman
tables, about a tenth fewer bytes) and ``restart_rows`` / ``restart_blocks`` (restart intervals, which ``JpegDecoder`` decodes in
parallel), and ``subsampling`` (Pillow's ``subsampling=``: 4:4:4, 4:2:2 or 4:2:0, and with it frames of ANY size, padded as libjpeg pads
them).  No default uses them.

The way back is ``JpegDecoder`` (include/lspjpegdec.h): baseline files -- the candidate images of demo.py:88-95, the frames of an
``AviWriter`` recording, anything Pillow writes by default -- decoded on the device to the pixels Pillow returns, bit for bit.  The
host does the marker parsing and the batch layout (``DecodePlan``, no device needed); the compressed bytes cross PCIe once, in one
block with the tables.  ``probe`` reports a file's geometry and whether it can be decoded.  With ``progressive=True`` (``probe``,
``DecodePlan``, ``JpegDecoder``) complete progressive files are taken as well, scan by scan, to the same pixels; off by default.
With ``parallel=True`` (``DecodePlan``, ``JpegDecoder``) the entropy decode runs in parallel inside a restart interval, which for a file
without restart markers means inside the file; same pixels and statuses; off by default.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, NamedTuple, Optional, Sequence, Union

import numpy as np

import torch

from . import _native as N
from . import imagedec
from .imagedec import FORM_GRAY8, FORM_PLANAR_F32, FORM_RGB8, MAX_SIDE, DecodeError, _aligned, _info  # noqa: F401  (the decoder half's shared names)


def _header_of(lib, h) -> bytes:
    n = lib.lspjpeg_header(h, None, 0)
    if n < 0:
        N.check_jpeg(n)
    buf = (ctypes.c_ubyte * n)()
    N.check_jpeg(min(int(lib.lspjpeg_header(h, buf, n)), 0))
    return bytes(buf)


class JpegOptions(NamedTuple):
    """What Pillow's ``Image.save(f, "JPEG", quality=, optimize=, restart_marker_rows=, restart_marker_blocks=)`` takes, as one value:
    accepted wherever a JPEG quality is (``render_frames(jpeg_quality=)``, ``LivePortraitPool.tick(jpeg_quality=)``, ``record_quality=``,
    ``VideoSink``).  ``optimize``: per-frame optimal Huffman tables; ``restart_rows`` MCU rows or ``restart_blocks`` MCUs per restart
    interval (not both; 0 = none).  ``subsampling``: None is the 4:2:0 encoder for frames whose sides are multiples of 16 (grey: 8);
    ``"4:4:4"`` / ``"4:2:2"`` / ``"4:2:0"`` (or Pillow's 0 / 1 / 2) is Pillow's ``subsampling=`` for frames of any size.  Grey frames have no
    chroma: any value but None selects the any-size route, and the value itself is ignored, as Pillow ignores it."""
    quality: int = 75
    optimize: bool = False
    restart_rows: int = 0
    restart_blocks: int = 0
    subsampling: Optional[str] = None

    @classmethod
    def of(cls, value) -> "JpegOptions":
        """an int (a quality, today's form) or a JpegOptions -> JpegOptions with plain types; the restart keywords are checked here, the
        quality where it always was (lspjpeg_create: LspjpegError; the pools: ValueError)"""
        o = value if isinstance(value, cls) else cls(quality=value)
        sub = o.subsampling
        if sub is not None:
            if isinstance(sub, bool) or sub not in _SUBSAMPLING:
                raise ValueError("subsampling must be None, '4:4:4', '4:2:2', '4:2:0' or Pillow's 0, 1, 2 (got %r)" % (sub, ))
            sub = _SUBSAMPLING[sub]
        o = cls(int(o.quality), bool(o.optimize), int(o.restart_rows), int(o.restart_blocks), sub)
        if o.restart_rows < 0 or o.restart_blocks < 0:
            raise ValueError("restart_rows and restart_blocks must be >= 0")
        if o.restart_rows and o.restart_blocks:
            raise ValueError("give restart_rows or restart_blocks, not both")
        return o

    def luma_factors(self, channels: int):
        """(h, v) sampling factors of the luma component: the MCU is 8h x 8v pixels"""
        if channels != 3:
            return 1, 1
        return _FACTORS[_SUBSAMPLING[self.subsampling]] if self.subsampling is not None else (2, 2)

    def restart_interval(self, width: int, channels: int) -> int:
        """MCUs per restart interval: jcmaster.c jinit_c_master_control's rows * MCUs per row capped at 65535 (on the grid of the chosen
        subsampling: ceil(width / 8h) MCUs per row); blocks as given"""
        if self.restart_rows:
            m = 8 * self.luma_factors(channels)[0]
            return min(self.restart_rows * ((int(width) + m - 1) // m if self.subsampling is not None else int(width) // m), 65535)
        return self.restart_blocks


_FACTORS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
_SUBSAMPLING = {"4:4:4": "4:4:4", "4:2:2": "4:2:2", "4:2:0": "4:2:0", 0: "4:4:4", 1: "4:2:2", 2: "4:2:0"}


def _create(lib, width: int, height: int, channels: int, o: JpegOptions) -> ctypes.c_void_p:
    """lspjpeg_create for plain options (the same handle, the parent's kernels), lspjpeg_create_opts with optimize or restart intervals,
    lspjpeg_create_format with a subsampling (any size; the geometry of the other two gives their handle)"""
    h = ctypes.c_void_p()
    if o.subsampling is not None:
        hs, vs = o.luma_factors(channels)
        c = N.JpegEncFormat(N.JPEG_FORMAT_ABI_VERSION, int(width), int(height), int(channels), o.quality, int(o.optimize), o.restart_interval(width, channels), hs, vs)
        N.check_jpeg(lib.lspjpeg_create_format(ctypes.byref(c), ctypes.byref(h)))
    elif not o.optimize and not o.restart_rows and not o.restart_blocks:
        N.check_jpeg(lib.lspjpeg_create(int(width), int(height), int(channels), o.quality, ctypes.byref(h)))
    else:
        c = N.JpegEncOptions(N.JPEG_ABI_VERSION, int(width), int(height), int(channels), o.quality, int(o.optimize), o.restart_interval(width, channels))
        N.check_jpeg(lib.lspjpeg_create_opts(ctypes.byref(c), ctypes.byref(h)))
    return h


def file_header(width: int, height: int, channels: int = 3, quality: Union[int, JpegOptions] = 75, optimize: bool = False, restart_rows: int = 0,
                restart_blocks: int = 0, subsampling=None) -> bytes:
    """The bytes every file of that geometry and those options starts with, built on the host: no device needed.  SOI .. SOS; with
    ``optimize`` SOI .. SOF0 (the tables, DRI and SOS are then each frame's own)."""
    lib = N.load()
    o = quality if isinstance(quality, JpegOptions) else JpegOptions(quality, optimize, restart_rows, restart_blocks, subsampling)
    h = _create(lib, width, height, channels, JpegOptions.of(o))
    try:
        return _header_of(lib, h)
    finally:
        lib.lspjpeg_destroy(h)


class JpegEncoder:
    """Baseline JPEG of ``[B, H, W, 3]`` uint8 RGB frames (``Engine.forward_image``; H, W multiples of 16) or ``[B, H, W]``
    uint8 grayscale frames (``FeatureMapRasteriser.rasterise(..., as_uint8=True)``; multiples of 8), B <= ``max_batch``; with a
    ``subsampling`` (``JpegOptions``) frames of any size, in 4:4:4, 4:2:2 or 4:2:0.
    ``size`` is the side of square frames or (H, W).  The device buffers (output at the documented worst-case bound per
    frame, sizes, workspace) are allocated once, here.  ``quality`` may be a ``JpegOptions``; ``optimize`` / ``restart_rows`` /
    ``restart_blocks`` are Pillow's ``optimize`` / ``restart_marker_rows`` / ``restart_marker_blocks``, and the files Pillow's with them."""

    _encode_symbol, _destroy_symbol, _check_rc = "lspjpeg_encode", "lspjpeg_destroy", staticmethod(N.check_jpeg)      # (png.PngEncoder: its own)

    def __init__(self, size: Union[int, Sequence[int]], channels: int = 3, quality: Union[int, JpegOptions] = 75, device="cuda:0", max_batch: int = 8,
                 optimize: bool = False, restart_rows: int = 0, restart_blocks: int = 0, subsampling=None):
        self.lib = N.load()
        self.height, self.width = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        if isinstance(quality, JpegOptions):
            if optimize or restart_rows or restart_blocks or subsampling is not None:
                raise ValueError("give a JpegOptions or the keywords, not both")
            self.options = JpegOptions.of(quality)
        else:
            self.options = JpegOptions.of(JpegOptions(quality, optimize, restart_rows, restart_blocks, subsampling))
        self.channels, self.quality, self.max_batch = int(channels), self.options.quality, int(max_batch)
        if self.max_batch < 1:
            raise ValueError("max_batch must be >= 1")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the JPEG encoder runs on the MI355X only (no CPU path); the reference's host path is Pillow's Image.save")
        h = _create(self.lib, self.width, self.height, self.channels, self.options)
        self._h = h
        self.header = _header_of(self.lib, h)
        self._allocate(int(self.lib.lspjpeg_capacity_bytes(h)), int(self.lib.lspjpeg_workspace_bytes(h, self.max_batch)))

    def _allocate(self, capacity: int, ws_bytes: int) -> None:
        self.capacity, self._ws_bytes = capacity, ws_bytes
        self._dst = torch.empty((self.max_batch, self.capacity), dtype=torch.uint8, device=self.device)
        self._sizes = torch.empty(self.max_batch, dtype=torch.int32, device=self.device)
        self._ws = torch.empty(self._ws_bytes, dtype=torch.uint8, device=self.device)
        self._sizes_host = torch.empty(self.max_batch, dtype=torch.int32, pin_memory=True)
        self._host = torch.empty(0, dtype=torch.uint8)
        self._pending = None                                    # (batch, stream) of a submit() not yet collected

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self.lib, self._destroy_symbol)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, frames: torch.Tensor) -> int:
        """shape, dtype, device and layout are checked HERE: the library receives bare pointers (as Engine._check_out)"""
        tail = (self.height, self.width, 3) if self.channels == 3 else (self.height, self.width)
        ok = isinstance(frames, torch.Tensor) and frames.dim() == len(tail) + 1 and tuple(frames.shape[1:]) == tail \
            and frames.dtype == torch.uint8 and frames.device == self.device and frames.is_contiguous()
        if not ok:
            raise ValueError("frames must be a contiguous uint8 tensor of shape [B, %s] on %s (got %s %s on %s, contiguous=%s)" % (
                ", ".join(map(str, tail)), self.device, getattr(frames, "dtype", type(frames)), tuple(getattr(frames, "shape", ())),
                getattr(frames, "device", "?"), getattr(frames, "is_contiguous", lambda: "?")()))
        b = frames.shape[0]
        if not 1 <= b <= self.max_batch:
            raise ValueError("batch %d outside 1..max_batch=%d" % (b, self.max_batch))
        # (a format handle reads bytes unless its geometry is that of lspjpeg_create; the library then states the rule itself)
        if self._aligned_src() and frames.data_ptr() % 16:
            raise ValueError("frames must start on a 16-byte boundary (a view with a storage offset does not)")
        return b

    def _aligned_src(self) -> bool:
        return self.options.subsampling is None

    def _launch(self, frames: torch.Tensor, b: int, stream) -> None:
        self._check_rc(getattr(self.lib, self._encode_symbol)(self._h, ctypes.c_void_p(frames.data_ptr()), b, ctypes.c_void_p(self._dst.data_ptr()),
                                                              ctypes.c_void_p(self._sizes.data_ptr()), ctypes.c_void_p(self._ws.data_ptr()), self._ws_bytes,
                                                              ctypes.c_void_p(stream.cuda_stream)))

    def submit(self, frames: torch.Tensor) -> None:
        """Enqueue the encode and the copy of the byte counts on the current stream; collect() hands out the files."""
        if self._pending is not None:
            raise RuntimeError("collect() the previous batch first: the encoder's buffers are still in use")
        b = self._check(frames)
        stream = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            self._launch(frames, b, stream)
            self._sizes_host[:b].copy_(self._sizes[:b], non_blocking=True)
        self._pending = (b, stream)

    @property
    def slab(self):
        """(output ``[max_batch, capacity]`` uint8, byte counts ``[max_batch]`` int32): what lspjpeg_encode leaves on the device, for a
        consumer that stays there (video.DeviceMuxer).  Read-only: the encoder writes them."""
        return self._dst, self._sizes

    def enqueue(self, frames: torch.Tensor) -> int:
        """The encode alone on the current stream, into ``slab``: no copy to the host, nothing for collect() to hand out.  Returns the batch."""
        if self._pending is not None:
            raise RuntimeError("collect() the previous batch first: the encoder's buffers are still in use")
        b = self._check(frames)
        stream = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            self._launch(frames, b, stream)
        return b

    def collect(self) -> List[bytes]:
        """Wait for the submitted batch, copy exactly its compressed bytes to pinned memory, return one file per frame."""
        if self._pending is None:
            raise RuntimeError("nothing submitted")
        b, stream = self._pending
        stream.synchronize()
        sizes = [int(v) for v in self._sizes_host[:b].tolist()]
        if any(not 2 <= n <= self.capacity for n in sizes):
            self._pending = None
            raise RuntimeError("%s returned byte counts %s outside 2..%d" % (self._encode_symbol, sizes, self.capacity))
        total = sum(sizes)
        if self._host.numel() < total:
            self._host = torch.empty(max(total, 2 * self._host.numel()), dtype=torch.uint8, pin_memory=True)
        offs = [sum(sizes[:k]) for k in range(b)]
        with torch.cuda.stream(stream):
            for k in range(b):
                self._host[offs[k]:offs[k] + sizes[k]].copy_(self._dst[k, :sizes[k]], non_blocking=True)
        stream.synchronize()
        self._pending = None
        host = self._host.numpy()
        return [self.header + host[offs[k]:offs[k] + sizes[k]].tobytes() for k in range(b)]

    def encode(self, frames: torch.Tensor) -> List[bytes]:
        """frames [B, H, W, 3] or [B, H, W] uint8 on the device -> B complete JPEG files"""
        self.submit(frames)
        return self.collect()


def save_images(save_root: str, jpegs: Sequence[bytes], index0: int = 0, prefix: str = "pred") -> List[str]:
    """Write encoded frames under the names Visualizer.save_images gives them (util/visualizer.py:120-136 with
    image_path = str(ind + 1), demo.py:271): ``<save_root>/<prefix>_<ind + 1>.jpg`` for ind = index0, index0 + 1, ..."""
    os.makedirs(save_root, exist_ok=True)
    paths = []
    for k, data in enumerate(jpegs):
        path = os.path.join(save_root, "%s_%d.jpg" % (prefix, index0 + k + 1))
        with open(path, "wb") as f:
            f.write(data)
        paths.append(path)
    return paths


# ---- decode -------------------------------------------------------------------------------------------------------------------------
UNSUPPORTED, CORRUPT, RANGE = 1, 2, 3                          # the per-file status words of include/lspjpegdec.h
STATUS_NAMES = {0: "OK", UNSUPPORTED: "UNSUPPORTED", CORRUPT: "CORRUPT", RANGE: "RANGE"}
FLAG_PROGRESSIVE = 1                                           # LSPJPEG_DEC_FLAG_PROGRESSIVE
FLAG_PARALLEL = 2                                              # LSPJPEG_DEC_FLAG_PARALLEL


class JpegError(DecodeError):
    """``code`` is UNSUPPORTED / CORRUPT / RANGE"""
    kind, names = "JPEG", STATUS_NAMES


class JpegInfo(NamedTuple):
    status: int                 # 0, UNSUPPORTED or CORRUPT: the header and the marker structure of the scan
    width: int
    height: int
    components: int
    hsamp: int                  # luma sampling factors: (1, 1) 4:4:4 or grey, (2, 1) 4:2:2, (2, 2) 4:2:0
    vsamp: int
    restart_interval: int       # MCUs per restart interval, 0 = none
    mcus: int
    segments: int               # restart intervals: the waves stage 1 gives the file
    default_tables: int         # bit (2 * id + class): that Huffman table is Annex K's because the file carries none
    scan_offset: int
    scan_bytes: int


class JpegScan(NamedTuple):
    """one scan of a progressive file, as the planner recorded it (lspjpeg_dec_scan)"""
    components: tuple           # indices in frame order: one, or all of the frame's
    dc_tables: tuple            # the table ids the SOS names, per scan component
    ac_tables: tuple
    ss: int
    se: int
    ah: int
    al: int
    restart_interval: int       # the DRI in force, in units; 0 = none
    units: int                  # interleaved MCUs, or the one component's own blocks
    segments: int
    begin: int                  # inside the block: the first entropy-coded byte, the marker that ends the scan
    end: int


def probe(data: bytes, progressive: bool = False) -> JpegInfo:
    """Geometry, sampling, restart interval and whether ``JpegDecoder`` takes the file (``status == 0``); host only.  ``progressive``: the
    answer of a decoder made with ``progressive=True`` (complete SOF2 files are taken; include/lspjpegdec.h says what the fields then mean)."""
    lib = N.load()
    data = bytes(data)
    info = N.JpegDecInfo()
    N.check_jpeg_dec(lib.lspjpeg_dec_probe_flags(ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), len(data), FLAG_PROGRESSIVE if progressive else 0,
                                                 ctypes.byref(info)))
    return _info(JpegInfo, info)


class DecodePlan(imagedec.DecodePlan):
    """The descriptor block of a batch (``lspjpeg_dec_plan``): per-file tables and output descriptions, the entropy-coded bytes, one
    entry per restart interval.  ``file(i).scan_offset`` is the offset of the file's data inside the block.
    ``progressive``: complete progressive files are planned too, scan by scan (``scans(i)``); without it they are UNSUPPORTED.
    ``parallel``: stage 1 of the baseline files decodes inside a restart interval in parallel (``parallel_segment(k)`` says how interval k is
    cut); same statuses, same coefficients, and ``host_coefficients`` then runs that route's code with the lanes as loops."""
    check = staticmethod(N.check_jpeg_dec)
    plan_symbol, summary_symbol, file_symbol = "lspjpeg_dec_plan_flags", "lspjpeg_dec_summary_of", "lspjpeg_dec_plan_file"
    info_struct, summary_struct, info_type = N.JpegDecInfo, N.JpegDecSummary, JpegInfo

    def __init__(self, files: Sequence[bytes], max_side: int = MAX_SIDE, outputs=None, buffer=None, progressive: bool = False, parallel: bool = False):
        super().__init__(files, max_side, outputs, buffer, ((FLAG_PROGRESSIVE if progressive else 0) | (FLAG_PARALLEL if parallel else 0), ))

    def qtable(self, i: int, c: int) -> np.ndarray:
        out = np.zeros(64, np.uint16)
        N.check_jpeg_dec(self.lib.lspjpeg_dec_plan_qtable(self.ptr, int(i), int(c), ctypes.c_void_p(out.ctypes.data)))
        return out

    def segment(self, k: int):
        """(file, first MCU, MCUs, begin, end) of restart interval k; begin / end are offsets inside the block"""
        f, m0, nm = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        b, e = ctypes.c_uint64(), ctypes.c_uint64()
        N.check_jpeg_dec(self.lib.lspjpeg_dec_plan_segment(self.ptr, int(k), ctypes.byref(f), ctypes.byref(m0), ctypes.byref(nm), ctypes.byref(b), ctypes.byref(e)))
        return f.value, m0.value, nm.value, b.value, e.value

    def parallel_segment(self, k: int):
        """(bytes of one subsequence, subsequences) of restart interval k of a plan made with ``parallel=True``; raises on any other plan"""
        size, count = ctypes.c_uint32(), ctypes.c_uint32()
        N.check_jpeg_dec(self.lib.lspjpeg_dec_plan_parallel(self.ptr, int(k), ctypes.byref(size), ctypes.byref(count)))
        return size.value, count.value

    def parallel_stats(self):
        """(most rounds the fixed point took in any chunk, true entry states inside a block) of the last ``host_coefficients`` call on this
        thread; (0, 0) unless that plan was made with ``parallel=True``"""
        rounds, mid = ctypes.c_uint32(), ctypes.c_uint32()
        N.check_jpeg_dec(self.lib.lspjpeg_dec_host_parallel_stats(ctypes.byref(rounds), ctypes.byref(mid)))
        return rounds.value, mid.value

    def scans(self, i: int) -> List[JpegScan]:
        """the scans of file i in file order; empty for a file that was not planned as a progressive one"""
        out = []
        for k in range(N.check_jpeg_dec(self.lib.lspjpeg_dec_plan_scans(self.ptr, int(i)))):
            s = N.JpegDecScan()
            N.check_jpeg_dec(self.lib.lspjpeg_dec_plan_scan(self.ptr, int(i), k, ctypes.byref(s)))
            nc = int(s.components)
            out.append(JpegScan(tuple(s.component[:nc]), tuple(s.dc_table[:nc]), tuple(s.ac_table[:nc]), int(s.ss), int(s.se), int(s.ah), int(s.al),
                                int(s.restart_interval), int(s.units), int(s.segments), int(s.begin), int(s.end)))
        return out

    def host_coefficients(self, i: int):
        """stage 1 of file i on the host, with the code the kernel runs: (status, int16 [blocks, 64] or None)"""
        info = self.file(i)
        if info.status:
            return info.status, None
        bpm = 1 if info.components == 1 else info.hsamp * info.vsamp + 2
        out = np.zeros((info.mcus * bpm, 64), np.int16)
        st = N.check_jpeg_dec(self.lib.lspjpeg_dec_host_coefficients(self.ptr, int(i), ctypes.c_void_p(out.ctypes.data), out.size))
        return st, (out if st == 0 else None)


class JpegDecoder(imagedec.Decoder):
    """Baseline JPEG files -> pixels on the device, equal to Pillow's (include/lspjpegdec.h states the arithmetic and what is refused).
    One call takes files of different sizes and kinds; batches above ``max_batch`` are split.  ``max_side`` bounds width and height
    (larger files are UNSUPPORTED).  The device buffers grow to the largest batch seen and are kept.  ``progressive=True`` also takes complete
    progressive files (SOF2), mixed freely with baseline ones: one more launch per call that holds any, one wave per such file.
    ``parallel=True`` decodes inside every restart interval of the baseline files in parallel (one workgroup per interval instead of one lane of
    one wave: the route for files without restart markers, Pillow's default and the encoder's own); same pixels, same statuses, same number of
    launches; off by default."""
    kind, error, decode_symbol, check = "JPEG", JpegError, "lspjpeg_dec_decode", staticmethod(N.check_jpeg_dec)

    def __init__(self, device="cuda:0", max_side: int = 1024, max_batch: int = 64, progressive: bool = False, parallel: bool = False):
        super().__init__(device, max_side, max_batch)
        self.progressive, self.parallel = bool(progressive), bool(parallel)

    def probe(self, data: bytes) -> JpegInfo:
        return probe(data, self.progressive)

    def plan(self, files: Sequence[bytes], outputs) -> DecodePlan:
        return DecodePlan(files, self.max_side, outputs, self._buffer, self.progressive, self.parallel)
