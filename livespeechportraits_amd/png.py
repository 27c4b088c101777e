"""PNG files -> pixels on the device, equal to Pillow's (include/lsppng.h states what is decoded, the arithmetic and every refusal): the lossless
sibling of jpeg.py's decoder half.  The front end is imagedec's (the output forms, the argument checks, one synchronisation per call, growing
buffers); here are ``PngInfo``, ``probe`` and the plan's two host twins, ``host_scanlines`` / ``host_pixels``: the kernels' code with the lanes as loops."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Sequence

import numpy as np

from . import _native as N
from . import imagedec
from .imagedec import FORM_GRAY8, FORM_PLANAR_F32, FORM_RGB8, MAX_SIDE, DecodeError, _aligned, _info  # noqa: F401  (the front end's shared names)

UNSUPPORTED, CORRUPT = 1, 2                                    # the per-file status words of include/lsppng.h
STATUS_NAMES = {0: "OK", UNSUPPORTED: "UNSUPPORTED", CORRUPT: "CORRUPT"}
SIGNATURE = b"\x89PNG\r\n\x1a\n"


class PngError(DecodeError):
    """``code`` is UNSUPPORTED / CORRUPT"""
    kind, names = "PNG", STATUS_NAMES


class PngInfo(NamedTuple):
    status: int                 # 0, UNSUPPORTED or CORRUPT: the container and the zlib header
    width: int
    height: int
    color_type: int             # 0 grey, 2 RGB, 3 palette, 4 grey + alpha, 6 RGBA
    depth: int
    components: int             # of the output: 3 or 1
    idat_bytes: int             # the concatenated IDAT payload
    raw_bytes: int              # height * (1 + rowbytes): the filtered scanlines


def probe(data: bytes) -> PngInfo:
    """Geometry, colour type, depth and whether ``PngDecoder`` takes the file (``status == 0``); host only."""
    lib = N.load()
    data = bytes(data)
    info = N.PngDecInfo()
    N.check_png_dec(lib.lsppng_dec_probe(ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), len(data), ctypes.byref(info)))
    return _info(PngInfo, info)


class DecodePlan(imagedec.DecodePlan):
    """The descriptor block of a batch (``lsppng_dec_plan``): per file the geometry, the output description, the palette and the concatenated
    IDAT payload."""
    check = staticmethod(N.check_png_dec)
    plan_symbol, summary_symbol, file_symbol = "lsppng_dec_plan", "lsppng_dec_summary_of", "lsppng_dec_plan_file"
    info_struct, summary_struct, info_type = N.PngDecInfo, N.PngDecSummary, PngInfo

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


class PngDecoder(imagedec.Decoder):
    """PNG files -> pixels on the device, equal to Pillow's ``convert("RGB")`` / ``convert("L")`` (include/lsppng.h): ``[H, W, 3]`` for colour
    types 2, 3, 6 and ``[H, W]`` for 0, 4."""
    kind, error, decode_symbol, check = "PNG", PngError, "lsppng_dec_decode", staticmethod(N.check_png_dec)

    def probe(self, data: bytes) -> PngInfo:
        return probe(data)

    def plan(self, files: Sequence[bytes], outputs) -> DecodePlan:
        return DecodePlan(files, self.max_side, outputs, self._buffer)
