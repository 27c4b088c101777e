"""The front end the image decoders share (jpeg.JpegDecoder, png.PngDecoder): the error a refused file raises, the descriptor block of a batch
(``DecodePlan``) and the decoder that plans, uploads, launches and reads the status words back (``Decoder``).  A format supplies what differs: its
``kind``, its status names, its probe, the symbols of its library half (include/lspjpegdec.h, include/lsppng.h) and, for JPEG, the two plan flags.
The three output forms are the library's (csrc/decode_out.h): the same words in both C headers."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _native as N

MAX_SIDE = 8192                                                # LSPJPEG_MAX_SIDE, LSPPNG_MAX_SIDE
FORM_RGB8, FORM_GRAY8, FORM_PLANAR_F32 = 0, 1, 2


class DecodeError(ValueError):
    """A file of a batch was refused: ``index`` and ``code`` (a status word of the format) of the first one, ``statuses`` of all.
    The outputs of the refused files were left untouched; the others are complete."""
    kind = "image"
    names = {0: "OK"}                                           # the format's STATUS_NAMES

    def __init__(self, statuses: Sequence[int]):
        self.statuses = [int(v) for v in statuses]
        self.index = next(i for i, v in enumerate(self.statuses) if v)
        self.code = self.statuses[self.index]
        bad = ["%d: %s" % (i, self.names.get(v, str(v))) for i, v in enumerate(self.statuses) if v]
        super().__init__("%s file %d of the batch is %s (refused files: %s)" % (self.kind, self.index, self.names.get(self.code, str(self.code)), ", ".join(bad)))


def _info(cls, struct):
    """a library info struct as the NamedTuple ``cls`` of the same field names"""
    return cls(*(int(getattr(struct, name)) for name in cls._fields))


def _aligned(nbytes: int) -> np.ndarray:
    raw = np.zeros(nbytes + 16, np.uint8)
    at = (-raw.ctypes.data) % 16
    return raw[at:at + nbytes]


class DecodePlan:
    """The descriptor block of a batch.  Host only.  ``outputs`` is a list of ``(ptr, table_ptr, plane_stride, form)`` per file (device
    pointers), or None to plan for the host alone.  ``buffer(nbytes)`` supplies the memory (a pinned tensor's numpy view, say).  A subclass names
    the library's symbols and structs; ``plan_args`` are the arguments its planner takes between ``max_side`` and the block."""
    check = plan_symbol = summary_symbol = file_symbol = info_struct = summary_struct = info_type = None

    def __init__(self, files: Sequence[bytes], max_side: int = MAX_SIDE, outputs=None, buffer=None, plan_args=()):
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
        plan = getattr(self.lib, self.plan_symbol)
        need = self.check(plan(ptrs, lens, outs, n, int(max_side), *plan_args, None, 0))   # the size first, then the content
        self.blob = buffer(need) if buffer is not None else _aligned(need)
        if self.blob.dtype != np.uint8 or self.blob.size < need or self.blob.ctypes.data % 16:
            raise ValueError("the plan needs a 16-byte aligned uint8 buffer of %d bytes" % need)
        self.ptr = ctypes.c_void_p(self.blob.ctypes.data)
        self.bytes = self.check(plan(ptrs, lens, outs, n, int(max_side), *plan_args, self.ptr, self.blob.size))
        self.summary = self.summary_struct()
        self.check(getattr(self.lib, self.summary_symbol)(self.ptr, ctypes.byref(self.summary)))

    def file(self, i: int):
        """what the planner recorded for file i"""
        info = self.info_struct()
        self.check(getattr(self.lib, self.file_symbol)(self.ptr, int(i), ctypes.byref(info)))
        return _info(self.info_type, info)

    def statuses(self) -> List[int]:
        at = int(self.summary.status_offset)
        return [int(v) for v in self.blob[at:at + 4 * len(self.files)].view(np.uint32)]


class Decoder:
    """Files -> pixels on the device.  One call takes files of different sizes and kinds; batches above ``max_batch`` are split.  ``max_side``
    bounds width and height (larger files are UNSUPPORTED).  The device buffers grow to the largest batch seen and are kept.  A subclass gives
    ``kind``, ``error`` (its DecodeError), ``decode_symbol``, ``probe(data)`` and ``plan(files, outputs)``."""
    kind = error = decode_symbol = None
    check = None

    def __init__(self, device="cuda:0", max_side: int = 1024, max_batch: int = 64):
        self.lib = N.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the %s decoder runs on the MI355X only (no CPU path); the reference's host path is cv2.imread / Pillow" % self.kind)
        if not 1 <= int(max_side) <= MAX_SIDE or int(max_batch) < 1:
            raise ValueError("max_side must be in 1..%d and max_batch >= 1" % MAX_SIDE)
        self.max_side, self.max_batch = int(max_side), int(max_batch)
        self._host = torch.empty(0, dtype=torch.uint8)
        self._dev = torch.empty(0, dtype=torch.uint8, device=self.device)
        self._ws = torch.empty(0, dtype=torch.uint8, device=self.device)
        self.last_status: List[int] = []

    def probe(self, data: bytes):
        raise NotImplementedError

    def plan(self, files: Sequence[bytes], outputs) -> DecodePlan:
        raise NotImplementedError

    def _buffer(self, nbytes: int) -> np.ndarray:
        if self._host.numel() < nbytes:
            self._host = torch.empty(max(nbytes, 2 * self._host.numel()), dtype=torch.uint8, pin_memory=True)
        return self._host.numpy()

    def _run(self, files: Sequence[bytes], outputs) -> List[int]:
        """plan, upload, the launches, and the status words back: the one synchronisation of a call"""
        plan = self.plan(files, outputs)
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
            self.check(getattr(self.lib, self.decode_symbol)(plan.ptr, ctypes.c_void_p(self._dev.data_ptr()), ctypes.c_void_p(self._ws.data_ptr()),
                                                             self._ws.numel(), ctypes.c_void_p(stream.cuda_stream)))
            at = int(plan.summary.status_offset)
            status = self._dev[at:at + 4 * len(files)].cpu()
        return [int(v) for v in status.numpy().view(np.uint32)]

    def _infos(self, files: Sequence[bytes]) -> list:
        infos = [self.probe(f) for f in files]
        for i in infos:
            if i.status == 0 and max(i.width, i.height) > self.max_side:
                raise ValueError("a %dx%d file: this decoder was made with max_side=%d" % (i.width, i.height, self.max_side))
        return infos

    def _decode(self, files: Sequence[bytes], specs) -> None:
        self.last_status = []
        for at in range(0, len(files), self.max_batch):
            self.last_status += self._run(files[at:at + self.max_batch], specs[at:at + self.max_batch])

    def decode(self, files: Sequence[bytes], strict: bool = True, outs: Optional[Sequence[torch.Tensor]] = None) -> List[Optional[torch.Tensor]]:
        """One uint8 tensor per file, ``[H, W, 3]`` (three components) or ``[H, W]`` (one).  A refused file raises the format's error
        (``JpegError``, ``PngError``); with ``strict=False`` it gives None in the list instead and ``last_status`` holds the status words.
        ``outs`` supplies the tensors (contiguous, right shape); a refused file's tensor is left untouched."""
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
        self._decode(files, [None if t is None else (t.data_ptr(), 0, 0, FORM_RGB8 if t.dim() == 3 else FORM_GRAY8) for t in result])
        if any(self.last_status):
            if strict:
                raise self.error(self.last_status)
            result = [None if s else t for s, t in zip(self.last_status, result)]
        return result

    def decode_into(self, files: Sequence[bytes], out: torch.Tensor, channel0: int, table: torch.Tensor) -> None:
        """``table[pixel]`` of every file as float32 planes of ``out`` ([C, H, W], contiguous): file j's channels follow file j - 1's,
        the first at ``channel0``.  ``table`` is 256 float32 on the device.  Every file must be H x W.  Raises the format's error when a file
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
        self._decode(files, specs)
        if any(self.last_status):
            raise self.error(self.last_status)
