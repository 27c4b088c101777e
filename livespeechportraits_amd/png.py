"""PNG files -> pixels on the device, equal to Pillow's (include/lsppng.h states what is decoded, the arithmetic and every refusal): the lossless
sibling of jpeg.py's decoder half, with the same three output forms, the same argument checks, one synchronisation per call and growing buffers.
``probe`` and ``DecodePlan`` are host code; ``DecodePlan.host_scanlines`` / ``host_pixels`` run the kernels' code with the lanes as loops."""
from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _native as N

UNSUPPORTED, CORRUPT = 1, 2                                    # the per-file status words of include/lsppng.h
STATUS_NAMES = {0: "OK", UNSUPPORTED: "UNSUPPORTED", CORRUPT: "CORRUPT"}
MAX_SIDE = 8192                                                # LSPPNG_MAX_SIDE
FORM_RGB8, FORM_GRAY8, FORM_PLANAR_F32 = 0, 1, 2
SIGNATURE = b"\x89PNG\r\n\x1a\n"


class PngError(ValueError):
    """A file of a batch was refused: ``index`` and ``code`` (UNSUPPORTED / CORRUPT) of the first one, ``statuses`` of all.
    The outputs of the refused files were left untouched; the others are complete."""

    def __init__(self, statuses: Sequence[int]):
        self.statuses = [int(v) for v in statuses]
        self.index = next(i for i, v in enumerate(self.statuses) if v)
        self.code = self.statuses[self.index]
        bad = ["%d: %s" % (i, STATUS_NAMES.get(v, str(v))) for i, v in enumerate(self.statuses) if v]
        super().__init__("PNG file %d of the batch is %s (refused files: %s)" % (self.index, STATUS_NAMES.get(self.code, str(self.code)), ", ".join(bad)))


class PngInfo(NamedTuple):
    status: int                 # 0, UNSUPPORTED or CORRUPT: the container and the zlib header
    width: int
    height: int
    color_type: int             # 0 grey, 2 RGB, 3 palette, 4 grey + alpha, 6 RGBA
    depth: int
    components: int             # of the output: 3 or 1
    idat_bytes: int             # the concatenated IDAT payload
    raw_bytes: int              # height * (1 + rowbytes): the filtered scanlines


def _info(i: "N.PngDecInfo") -> PngInfo:
    return PngInfo(*(int(getattr(i, name)) for name in PngInfo._fields))


def probe(data: bytes) -> PngInfo:
    """Geometry, colour type, depth and whether ``PngDecoder`` takes the file (``status == 0``); host only."""
    lib = N.load()
    data = bytes(data)
    info = N.PngDecInfo()
    N.check_png_dec(lib.lsppng_dec_probe(ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), len(data), ctypes.byref(info)))
    return _info(info)


def _aligned(nbytes: int) -> np.ndarray:
    raw = np.zeros(nbytes + 16, np.uint8)
    at = (-raw.ctypes.data) % 16
    return raw[at:at + nbytes]


class DecodePlan:
    """The descriptor block of a batch (``lsppng_dec_plan``): per file the geometry, the output description, the palette and the concatenated
    IDAT payload.  Host only.  ``outputs`` is a list of ``(ptr, table_ptr, plane_stride, form)`` per file (device pointers), or None to plan
    for the host alone.  ``buffer(nbytes)`` supplies the memory (a pinned tensor's numpy view, say)."""

    def __init__(self, files: Sequence[bytes], max_side: int = MAX_SIDE, outputs=None, buffer=None):
        self.lib = N.load()
        self.files = [bytes(f) for f in files]
        n = len(self.files)
        if n < 1:
            raise ValueError("no files")
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(f), ctypes.c_void_p) for f in self.files])
        lens = (ctypes.c_size_t * n)(*[len(f) for f in self.files])
        outs = None
        if outputs is not None:
            outs = (N.JpegDecOutput * n)()
            for o, spec in zip(outs, outputs):
                if spec is not None:
                    o.ptr, o.table, o.plane_stride, o.form = spec[0], spec[1] or None, int(spec[2]), int(spec[3])
        need = N.check_png_dec(self.lib.lsppng_dec_plan(ptrs, lens, outs, n, int(max_side), None, 0))
        self.blob = buffer(need) if buffer is not None else _aligned(need)
        if self.blob.dtype != np.uint8 or self.blob.size < need or self.blob.ctypes.data % 16:
            raise ValueError("the plan needs a 16-byte aligned uint8 buffer of %d bytes" % need)
        self.ptr = ctypes.c_void_p(self.blob.ctypes.data)
        self.bytes = N.check_png_dec(self.lib.lsppng_dec_plan(ptrs, lens, outs, n, int(max_side), self.ptr, self.blob.size))
        self.summary = N.PngDecSummary()
        N.check_png_dec(self.lib.lsppng_dec_summary_of(self.ptr, ctypes.byref(self.summary)))

    def file(self, i: int) -> PngInfo:
        """what the planner recorded for file i"""
        info = N.PngDecInfo()
        N.check_png_dec(self.lib.lsppng_dec_plan_file(self.ptr, int(i), ctypes.byref(info)))
        return _info(info)

    def statuses(self) -> List[int]:
        at = int(self.summary.status_offset)
        return [int(v) for v in self.blob[at:at + 4 * len(self.files)].view(np.uint32)]

    def host_scanlines(self, i: int):
        """launch 1 of file i on the host, with the code the kernel runs: (status, the filtered scanlines uint8 [H, 1 + rowbytes] or None)"""
        info = self.file(i)
        if info.status:
            return info.status, None
        out = np.zeros(info.raw_bytes, np.uint8)
        st = N.check_png_dec(self.lib.lsppng_dec_host_scanlines(self.ptr, int(i), ctypes.c_void_p(out.ctypes.data), out.size))
        return st, (out.reshape(info.height, -1) if st == 0 else None)

    def host_pixels(self, i: int):
        """all three launches of file i on the host: (status, uint8 [H, W, 3] or [H, W], or None)"""
        info = self.file(i)
        if info.status:
            return info.status, None
        shape = (info.height, info.width, 3) if info.components == 3 else (info.height, info.width)
        out = np.zeros(shape, np.uint8)
        st = N.check_png_dec(self.lib.lsppng_dec_host_pixels(self.ptr, int(i), ctypes.c_void_p(out.ctypes.data), out.size))
        return st, (out if st == 0 else None)


class PngDecoder:
    """PNG files -> pixels on the device, equal to Pillow's ``convert("RGB")`` / ``convert("L")`` (include/lsppng.h).  One call takes files of
    different sizes and kinds; batches above ``max_batch`` are split.  ``max_side`` bounds width and height (larger files are UNSUPPORTED).
    The device buffers grow to the largest batch seen and are kept."""

    def __init__(self, device="cuda:0", max_side: int = 1024, max_batch: int = 64):
        self.lib = N.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the PNG decoder runs on the MI355X only (no CPU path); the reference's host path is cv2.imread / Pillow")
        if not 1 <= int(max_side) <= MAX_SIDE or int(max_batch) < 1:
            raise ValueError("max_side must be in 1..%d and max_batch >= 1" % MAX_SIDE)
        self.max_side, self.max_batch = int(max_side), int(max_batch)
        self._host = torch.empty(0, dtype=torch.uint8)
        self._dev = torch.empty(0, dtype=torch.uint8, device=self.device)
        self._ws = torch.empty(0, dtype=torch.uint8, device=self.device)
        self.last_status: List[int] = []

    def _buffer(self, nbytes: int) -> np.ndarray:
        if self._host.numel() < nbytes:
            self._host = torch.empty(max(nbytes, 2 * self._host.numel()), dtype=torch.uint8, pin_memory=True)
        return self._host.numpy()

    def _run(self, files: Sequence[bytes], outputs) -> List[int]:
        """plan, upload, the three launches, and the status words back: the one synchronisation of a call"""
        plan = DecodePlan(files, self.max_side, outputs, self._buffer)
        if all(plan.statuses()):
            return plan.statuses()                             # nothing to decode: the planner refused every file
        n, ws = int(plan.bytes), int(plan.summary.workspace_bytes)
        if self._dev.numel() < n:
            self._dev = torch.empty(max(n, 2 * self._dev.numel()), dtype=torch.uint8, device=self.device)
        if self._ws.numel() < ws:
            self._ws = torch.empty(max(ws, 2 * self._ws.numel()), dtype=torch.uint8, device=self.device)
        stream = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            self._dev[:n].copy_(self._host[:n], non_blocking=True)
            N.check_png_dec(self.lib.lsppng_dec_decode(plan.ptr, ctypes.c_void_p(self._dev.data_ptr()), ctypes.c_void_p(self._ws.data_ptr()),
                                                       self._ws.numel(), ctypes.c_void_p(stream.cuda_stream)))
            at = int(plan.summary.status_offset)
            status = self._dev[at:at + 4 * len(files)].cpu()
        return [int(v) for v in status.numpy().view(np.uint32)]

    def _infos(self, files: Sequence[bytes]) -> List[PngInfo]:
        infos = [probe(f) for f in files]
        for i in infos:
            if i.status == 0 and max(i.width, i.height) > self.max_side:
                raise ValueError("a %dx%d file: this decoder was made with max_side=%d" % (i.width, i.height, self.max_side))
        return infos

    def decode(self, files: Sequence[bytes], strict: bool = True, outs: Optional[Sequence[torch.Tensor]] = None) -> List[Optional[torch.Tensor]]:
        """One uint8 tensor per file, ``[H, W, 3]`` (colour types 2, 3, 6) or ``[H, W]`` (0, 4).  A refused file raises ``PngError``; with
        ``strict=False`` it gives None in the list instead and ``last_status`` holds the status words.  ``outs`` supplies the tensors
        (contiguous, right shape); a refused file's tensor is left untouched."""
        files = [bytes(f) for f in files]
        infos = self._infos(files)
        result: List[Optional[torch.Tensor]] = []
        for k, i in enumerate(infos):
            shape = (i.height, i.width, 3) if i.components == 3 else (i.height, i.width)
            if i.status:
                result.append(None)
                continue
            t = outs[k] if outs is not None else torch.empty(shape, dtype=torch.uint8, device=self.device)
            if tuple(t.shape) != shape or t.dtype != torch.uint8 or t.device != self.device or not t.is_contiguous():
                raise ValueError("outs[%d] must be a contiguous uint8 tensor of shape %s on %s" % (k, shape, self.device))
            result.append(t)
        specs = [None if t is None else (t.data_ptr(), 0, 0, FORM_RGB8 if t.dim() == 3 else FORM_GRAY8) for t in result]
        self.last_status = []
        for at in range(0, len(files), self.max_batch):
            self.last_status += self._run(files[at:at + self.max_batch], specs[at:at + self.max_batch])
        if any(self.last_status):
            if strict:
                raise PngError(self.last_status)
            result = [None if s else t for s, t in zip(self.last_status, result)]
        return result

    def decode_into(self, files: Sequence[bytes], out: torch.Tensor, channel0: int, table: torch.Tensor) -> None:
        """``table[pixel]`` of every file as float32 planes of ``out`` ([C, H, W], contiguous): file j's channels follow file j - 1's,
        the first at ``channel0``.  ``table`` is 256 float32 on the device.  Every file must be H x W.  Raises ``PngError`` when a file
        is refused; the channels of the others are complete, its own untouched."""
        files = [bytes(f) for f in files]
        if not (isinstance(out, torch.Tensor) and out.dim() == 3 and out.dtype == torch.float32 and out.device == self.device and out.is_contiguous()):
            raise ValueError("out must be a contiguous float32 [C, H, W] tensor on %s" % self.device)
        if not (isinstance(table, torch.Tensor) and tuple(table.shape) == (256,) and table.dtype == torch.float32 and table.device == self.device
                and table.is_contiguous()):
            raise ValueError("table must be 256 contiguous float32 values on %s" % self.device)
        c, h, w = out.shape
        specs, ch = [], int(channel0)
        for k, i in enumerate(self._infos(files)):
            if i.status:
                specs.append(None)
                continue
            if (i.height, i.width) != (h, w):
                raise ValueError("file %d is %dx%d, out is %dx%d" % (k, i.width, i.height, w, h))
            if ch < 0 or ch + i.components > c:
                raise ValueError("file %d would land at channels %d..%d of %d" % (k, ch, ch + i.components - 1, c))
            specs.append((out.data_ptr() + 4 * ch * h * w, table.data_ptr(), h * w, FORM_PLANAR_F32))
            ch += i.components
        self.last_status = []
        for at in range(0, len(files), self.max_batch):
            self.last_status += self._run(files[at:at + self.max_batch], specs[at:at + self.max_batch])
        if any(self.last_status):
            raise PngError(self.last_status)
