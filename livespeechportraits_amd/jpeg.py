"""The JPEG writer of demo.py's frame loop on the device (demo.py:268-272 -> util/visualizer.py:120-136 save_images ->
util/util.py:70-72 ``Image.fromarray(img).save(path)`` with a ``.jpg`` name).

``JpegEncoder`` encodes batches of uint8 device frames with ``lspjpeg_encode`` (include/lspjpeg.h) and hands back complete
files as ``bytes``: for the same pixels they are the bytes Pillow writes with its defaults (quality 75, baseline, 4:2:0,
standard Huffman tables, JFIF header).  Only the compressed bytes cross PCIe: the per-frame sizes are copied first, then
each frame's bytes.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence, Union

import torch

from . import _native as N


def _header_of(lib, h) -> bytes:
    n = lib.lspjpeg_header(h, None, 0)
    if n < 0:
        N.check_jpeg(n)
    buf = (ctypes.c_ubyte * n)()
    N.check_jpeg(min(int(lib.lspjpeg_header(h, buf, n)), 0))
    return bytes(buf)


def file_header(width: int, height: int, channels: int = 3, quality: int = 75) -> bytes:
    """The bytes every file of that geometry and quality starts with (SOI .. SOS), built on the host: no device needed."""
    lib = N.load()
    h = ctypes.c_void_p()
    N.check_jpeg(lib.lspjpeg_create(int(width), int(height), int(channels), int(quality), ctypes.byref(h)))
    try:
        return _header_of(lib, h)
    finally:
        lib.lspjpeg_destroy(h)


class JpegEncoder:
    """Baseline JPEG of ``[B, H, W, 3]`` uint8 RGB frames (``Engine.forward_image``; H, W multiples of 16) or ``[B, H, W]``
    uint8 grayscale frames (``FeatureMapRasteriser.rasterise(..., as_uint8=True)``; multiples of 8), B <= ``max_batch``.
    ``size`` is the side of square frames or (H, W).  The device buffers (output at the documented worst-case bound per
    frame, sizes, workspace) are allocated once, here."""

    def __init__(self, size: Union[int, Sequence[int]], channels: int = 3, quality: int = 75, device="cuda:0", max_batch: int = 8):
        self.lib = N.load()
        self.height, self.width = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        self.channels, self.quality, self.max_batch = int(channels), int(quality), int(max_batch)
        if self.max_batch < 1:
            raise ValueError("max_batch must be >= 1")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the JPEG encoder runs on the MI355X only (no CPU path); the reference's host path is Pillow's Image.save")
        h = ctypes.c_void_p()
        N.check_jpeg(self.lib.lspjpeg_create(self.width, self.height, self.channels, self.quality, ctypes.byref(h)))
        self._h = h
        self.header = _header_of(self.lib, h)
        self.capacity = int(self.lib.lspjpeg_capacity_bytes(h))
        self._ws_bytes = int(self.lib.lspjpeg_workspace_bytes(h, self.max_batch))
        self._dst = torch.empty((self.max_batch, self.capacity), dtype=torch.uint8, device=self.device)
        self._sizes = torch.empty(self.max_batch, dtype=torch.int32, device=self.device)
        self._ws = torch.empty(self._ws_bytes, dtype=torch.uint8, device=self.device)
        self._sizes_host = torch.empty(self.max_batch, dtype=torch.int32, pin_memory=True)
        self._host = torch.empty(0, dtype=torch.uint8)
        self._pending = None                                    # (batch, stream) of a submit() not yet collected

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.lspjpeg_destroy(self._h)
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
        if frames.data_ptr() % 16:
            raise ValueError("frames must start on a 16-byte boundary (a view with a storage offset does not)")
        return b

    def submit(self, frames: torch.Tensor) -> None:
        """Enqueue the encode and the copy of the byte counts on the current stream; collect() hands out the files."""
        if self._pending is not None:
            raise RuntimeError("collect() the previous batch first: the encoder's buffers are still in use")
        b = self._check(frames)
        stream = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            N.check_jpeg(self.lib.lspjpeg_encode(self._h, ctypes.c_void_p(frames.data_ptr()), b, ctypes.c_void_p(self._dst.data_ptr()),
                                                 ctypes.c_void_p(self._sizes.data_ptr()), ctypes.c_void_p(self._ws.data_ptr()), self._ws_bytes,
                                                 ctypes.c_void_p(stream.cuda_stream)))
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
            N.check_jpeg(self.lib.lspjpeg_encode(self._h, ctypes.c_void_p(frames.data_ptr()), b, ctypes.c_void_p(self._dst.data_ptr()),
                                                 ctypes.c_void_p(self._sizes.data_ptr()), ctypes.c_void_p(self._ws.data_ptr()), self._ws_bytes,
                                                 ctypes.c_void_p(stream.cuda_stream)))
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
            raise RuntimeError("lspjpeg_encode returned byte counts %s outside 2..%d" % (sizes, self.capacity))
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
