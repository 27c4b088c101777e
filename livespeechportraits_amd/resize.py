"""``PIL.Image.resize`` for 8-bit grey and RGB images on the device, bit for bit (include/lspresize.h states the arithmetic).

``Resizer.resize(u8, size, resample)`` takes uint8 frames that are already on the device -- the generator's, a decoded photograph -- and
returns them at another size without a pixel crossing PCIe; ``resize_planes`` writes them as normalised float planes through a 256-entry
table instead (candidates.load_candidates).  ``ResizePlan`` is the host half (Pillow's coefficients in double, then fixed point): it needs
the library and no device.

Offered: BOX, BILINEAR, HAMMING, BICUBIC (the default, as Pillow's ``resize``) and LANCZOS; 1 or 3 channels; sides of 1 .. 8192.
NOT offered, refused with ValueError: NEAREST (another code path in Pillow), ``box=``, ``reducing_gap=``, other modes and dtypes.
There is no CPU path: the reference's host path is Pillow itself.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native as N

FILTERS = tuple(N.RSZ_FILTERS)
MAX_SIDE = N.RSZ_MAX_SIDE
Size = Union[int, Sequence[int]]


def check_filter(resample) -> str:
    """the filter's name, or ValueError naming what is not offered"""
    name = resample.lower() if isinstance(resample, str) else resample
    if name == "nearest" or resample == 0 and not isinstance(resample, str):
        raise ValueError("resample NEAREST is not offered: it is another code path in Pillow (offered: %s)" % ", ".join(FILTERS))
    if name not in N.RSZ_FILTERS:
        raise ValueError("resample %r is not offered: give one of %s by name" % (resample, ", ".join(FILTERS)))
    return name


def check_size(size: Size) -> Tuple[int, int]:
    """(width, height) of an int or a (width, height) pair, as Pillow's ``size``; ValueError for a side of 0 or above 8192"""
    if isinstance(size, (int, np.integer)):
        w = h = int(size)
    else:
        try:
            w, h = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError("size must be an int or (width, height), got %r" % (size,))
    if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
        raise ValueError("size %dx%d: a side of 0 or above %d is not offered" % (w, h, MAX_SIDE))
    return w, h


def _aligned(nbytes: int) -> np.ndarray:
    raw = np.zeros(nbytes + 16, np.uint8)
    at = (-raw.ctypes.data) % 16
    return raw[at:at + nbytes]


class ResizePlan:
    """The descriptor block of one geometry and filter (``lsprsz_plan``): per pass the bounds and the int32 coefficients, the row window
    of the horizontal pass, and which kernel path each pass takes.  Host only."""

    def __init__(self, in_size: Size, out_size: Size, resample: str = "bicubic"):
        self.lib = N.load()
        self.filter = check_filter(resample)
        (self.in_w, self.in_h), (self.out_w, self.out_h) = check_size(in_size), check_size(out_size)
        geom = (self.in_w, self.in_h, self.out_w, self.out_h, N.RSZ_FILTERS[self.filter])
        try:
            need = N.check_rsz(self.lib.lsprsz_plan(*geom, None, 0))
            self.blob = _aligned(need)
            self.ptr = ctypes.c_void_p(self.blob.ctypes.data)
            self.bytes = N.check_rsz(self.lib.lsprsz_plan(*geom, self.ptr, self.blob.size))
        except N.LsprszError as e:
            raise ValueError(str(e)) from e
        self.info = N.RszInfo()
        N.check_rsz(self.lib.lsprsz_plan_info(self.ptr, ctypes.byref(self.info)))

    @property
    def paths(self) -> Tuple[Optional[str], Optional[str]]:
        """(horizontal, vertical): "tile", "general" or None where the pass does not run (a copy runs through the vertical kernel)"""
        return N.RSZ_PATHS[self.info.path_h], N.RSZ_PATHS[self.info.path_v]

    @property
    def launches(self) -> int:
        return int(self.info.launches)

    def axis(self, axis: int):
        """(bounds int32 [out, 2], coefficients int32 [out, ksize]) of the horizontal (0) or vertical (1) pass, None where it does not run"""
        ksize = int(self.info.ksize_v if axis else self.info.ksize_h)
        n = int(self.out_h if axis else self.out_w)
        if not (self.info.need_v if axis else self.info.need_h):
            return None
        b, k = np.zeros((n, 2), np.int32), np.zeros((n, ksize), np.int32)
        got = N.check_rsz(self.lib.lsprsz_plan_axis(self.ptr, int(axis), ctypes.c_void_p(b.ctypes.data), b.size, ctypes.c_void_p(k.ctypes.data), k.size))
        assert got == n
        return b, k

    def workspace_bytes(self, n: int, channels: int) -> int:
        return N.check_rsz(self.lib.lsprsz_workspace_bytes(self.ptr, int(n), int(channels)))


class Resizer:
    """Resizes batches of uint8 images on ``device``.  Plans (host block and device copy) are kept per (input size, output size, filter);
    the workspace grows to the largest call seen and is kept.  ``max_batch`` bounds the images of one call."""

    def __init__(self, device="cuda:0", max_batch: int = 8):
        self.lib = N.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the resampler runs on the MI355X only (no CPU path); the reference's host path is Pillow's Image.resize")
        if int(max_batch) < 1:
            raise ValueError("max_batch must be >= 1")
        self.max_batch = int(max_batch)
        self._plans: Dict[tuple, Tuple[ResizePlan, torch.Tensor]] = {}
        self._ws = torch.empty(0, dtype=torch.uint8, device=self.device)

    def plan(self, in_size: Size, out_size: Size, resample: str = "bicubic") -> ResizePlan:
        return self._plan(check_size(in_size), check_size(out_size), check_filter(resample))[0]

    def _plan(self, in_size, out_size, filt):
        key = (in_size, out_size, filt)
        if key not in self._plans:
            p = ResizePlan(in_size, out_size, filt)
            self._plans[key] = (p, torch.from_numpy(p.blob[:p.bytes]).to(self.device))
        return self._plans[key]

    @property
    def workspace(self) -> torch.Tensor:
        """the workspace as it stands (uint8); its content on entry to a call is irrelevant"""
        return self._ws

    def _images(self, u8, channels: Optional[int] = None) -> Tuple[torch.Tensor, bool, int]:
        """[n, H, W, C] view of the argument, whether it was a single image, and C.  Without ``channels`` a 4-dimensional tensor is an RGB
        batch, a 3-dimensional one whose last side is 3 ONE RGB image and any other a grey batch, a 2-dimensional one a grey image;
        ``channels`` (1 or 3) says it outright."""
        if not isinstance(u8, torch.Tensor):
            raise ValueError("images must be a torch tensor on %s, got %s" % (self.device, type(u8).__name__))
        if u8.dtype != torch.uint8:
            raise ValueError("images must be uint8, got %s: modes other than 8-bit grey and RGB are not offered" % u8.dtype)
        if u8.device != self.device:
            raise ValueError("images are on %s, this Resizer on %s" % (u8.device, self.device))
        if channels not in (None, 1, 3):
            raise ValueError("%r channels are not offered (1 for grey, 3 for RGB)" % (channels,))
        if channels is None:
            channels = 3 if u8.dim() == 4 or (u8.dim() == 3 and u8.shape[2] == 3) else 1
        if channels == 3:
            if u8.dim() not in (3, 4):
                raise ValueError("RGB images must be [n, H, W, 3] or [H, W, 3], got %s" % (tuple(u8.shape),))
            if u8.shape[-1] != 3:
                raise ValueError("%s: %d channels are not offered (3 for RGB; grey is [n, H, W])" % (tuple(u8.shape), u8.shape[-1]))
            x, single, ch = (u8, False, 3) if u8.dim() == 4 else (u8.unsqueeze(0), True, 3)
        else:
            if u8.dim() not in (2, 3):
                raise ValueError("grey images must be [n, H, W] or [H, W], got %s" % (tuple(u8.shape),))
            x, single, ch = (u8.unsqueeze(3), False, 1) if u8.dim() == 3 else (u8.unsqueeze(0).unsqueeze(3), True, 1)
        n, h, w = x.shape[:3]
        if not 1 <= n <= self.max_batch:
            raise ValueError("batch %d outside 1..max_batch=%d" % (n, self.max_batch))
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise ValueError("images of %dx%d: a side of 0 or above %d is not offered" % (w, h, MAX_SIDE))
        if x.stride()[1:] != (w * ch, ch, 1) or (n > 1 and x.stride(0) < h * w * ch):
            raise ValueError("every image must be contiguous (only the stride between images is free), got strides %s" % (tuple(u8.stride()),))
        return x, single, ch

    def _run(self, x: torch.Tensor, ch: int, size, filt: str, out: N.RszOutput) -> None:
        n, h, w = x.shape[:3]
        plan, dev = self._plan((w, h), size, filt)
        need = plan.workspace_bytes(n, ch)
        if self._ws.numel() < need:
            self._ws = torch.empty(max(need, 2 * self._ws.numel()), dtype=torch.uint8, device=self.device)
        stream = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            N.check_rsz(self.lib.lsprsz_resize(plan.ptr, ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(x.data_ptr()), int(x.stride(0)) if n > 1 else h * w * ch,
                                               n, ch, ctypes.byref(out), ctypes.c_void_p(self._ws.data_ptr()) if need else None, self._ws.numel(),
                                               ctypes.c_void_p(stream.cuda_stream)))

    def resize(self, u8: torch.Tensor, size: Size, resample: str = "bicubic", out: Optional[torch.Tensor] = None, channels: Optional[int] = None,
               box=None, reducing_gap=None) -> torch.Tensor:
        """uint8 ``[n, H, W, 3]``, ``[n, H, W]`` or a single ``[H, W, 3]`` / ``[H, W]`` image on the device -> the same form at ``size`` (an int or
        ``(width, height)``), enqueued on the current stream; ``out`` (same form, images contiguous) receives it.  A 3-dimensional tensor whose
        last side is 3 is ONE RGB image unless ``channels=1`` says it is a grey batch (``channels``: 1 or 3, None = by shape)."""
        if box is not None or reducing_gap is not None:
            raise ValueError("box= and reducing_gap= are not offered")
        filt, size = check_filter(resample), check_size(size)
        x, single, ch = self._images(u8, channels)
        n = x.shape[0]
        shape = (n, size[1], size[0], ch)
        if out is None:
            res = torch.empty(shape, dtype=torch.uint8, device=self.device)
            o4 = res
        else:
            o4, o_single, o_ch = self._images(out, ch)
            if tuple(o4.shape) != shape or o_single != single:
                raise ValueError("out must have the form of the images at %dx%d, got %s" % (size[0], size[1], tuple(out.shape)))
            res = o4
        spec = N.RszOutput(o4.data_ptr(), None, int(o4.stride(0)) if n > 1 else shape[1] * shape[2] * ch, 0, N.RSZ_FORM_U8, 0)
        self._run(x, ch, size, filt, spec)
        if out is not None:
            return out
        res = res if ch == 3 else res.squeeze(3)
        return res[0] if single else res

    def resize_planes(self, u8: torch.Tensor, size: Size, table: torch.Tensor, out: torch.Tensor, resample: str = "bicubic",
                      channels: Optional[int] = None) -> torch.Tensor:
        """``table[pixel]`` of the resized images as float32 planes: ``out`` is ``[n, C, height, width]`` (or ``[C, height, width]`` for a single
        image) with contiguous planes; ``table`` 256 float32 on the device.  No uint8 image of the output size is formed in between."""
        filt, size = check_filter(resample), check_size(size)
        x, single, ch = self._images(u8, channels)
        n = x.shape[0]
        if not (isinstance(table, torch.Tensor) and tuple(table.shape) == (256,) and table.dtype == torch.float32 and table.device == self.device and table.is_contiguous()):
            raise ValueError("table must be 256 contiguous float32 values on %s" % self.device)
        o = out.unsqueeze(0) if isinstance(out, torch.Tensor) and single and out.dim() == 3 else out
        if not (isinstance(o, torch.Tensor) and o.dtype == torch.float32 and o.device == self.device and tuple(o.shape) == (n, ch, size[1], size[0])
                and o.stride()[2:] == (size[0], 1) and o.stride(1) >= size[0] * size[1] and (n == 1 or o.stride(0) >= ch * o.stride(1))):
            raise ValueError("out must be float32 [%d, %d, %d, %d] on %s with contiguous planes" % (n, ch, size[1], size[0], self.device))
        spec = N.RszOutput(o.data_ptr(), table.data_ptr(), int(o.stride(0)) if n > 1 else ch * int(o.stride(1)), int(o.stride(1)), N.RSZ_FORM_PLANAR_F32, 0)
        self._run(x, ch, size, filt, spec)
        return out
