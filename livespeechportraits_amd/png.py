"""PNG files -> pixels on the device, equal to Pillow's (include/lsppng.h states what is decoded, the arithmetic and every refusal): the lossless
sibling of jpeg.py's decoder half.  The front end is imagedec's (the output forms, the argument checks, one synchronisation per call, growing
buffers); here are ``PngInfo``, ``probe`` and the plan's two host twins, ``host_scanlines`` / ``host_pixels``: the kernels' code with the lanes as loops.

And the way out: ``PngEncoder`` (include/lsppngenc.h) writes uint8 device frames, RGB or grey and of any size, as complete PNG files, losslessly:
Pillow and ``PngDecoder`` return exactly the pixels that went in.  The bytes are not Pillow's (its zlib is serial); they are a pure function of the
pixels and the options, and ``host_file`` makes the same file on the host with the kernels' code.  The front end is ``jpeg.JpegEncoder``'s."""
from __future__ import annotations

import ctypes
import os
from typing import List, NamedTuple, Optional, Sequence, Union

import numpy as np

from . import _native as N
from . import imagedec
from .jpeg import JpegEncoder
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


# ---- encode -------------------------------------------------------------------------------------------------------------------------
CHUNK = N.PNGENC_CHUNK                                         # bytes of the filtered scanlines per independently compressed piece
FILTERS = {None: -1, "none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, 0: 0, 1: 1, 2: 2, 3: 3, 4: 4}


class PngOptions(NamedTuple):
    """``level``: 1 = matcher + Huffman coding (default), 0 = stored blocks only.  ``filter``: None = the PNG specification's per-row heuristic,
    0..4 (or "none" / "sub" / "up" / "average" / "paeth") = that filter for all rows.  Accepted wherever ``png=`` is."""
    level: int = 1
    filter: Optional[Union[int, str]] = None

    @classmethod
    def of(cls, value) -> "PngOptions":
        """True or a PngOptions -> PngOptions with plain types"""
        o = cls() if value is True else value
        if not isinstance(o, cls):
            raise ValueError("png must be True or a PngOptions (got %r)" % (value, ))
        if isinstance(o.filter, bool) or o.filter not in FILTERS:
            raise ValueError("filter must be None, 0..4 or one of 'none', 'sub', 'up', 'average', 'paeth' (got %r)" % (o.filter, ))
        if isinstance(o.level, bool) or o.level not in (0, 1):
            raise ValueError("level must be 0 or 1 (got %r)" % (o.level, ))
        f = FILTERS[o.filter]
        return cls(int(o.level), None if f < 0 else f)


def _create(lib, width: int, height: int, channels: int, o: PngOptions) -> ctypes.c_void_p:
    h = ctypes.c_void_p()
    c = N.PngEncOptions(N.PNGENC_ABI_VERSION, o.level, -1 if o.filter is None else o.filter)
    N.check_png_enc(lib.lsppng_enc_create(int(width), int(height), int(channels), ctypes.byref(c), ctypes.byref(h)))
    return h


def _header_of(lib, h) -> bytes:
    buf = (ctypes.c_ubyte * N.PNGENC_HEADER_BYTES)()
    N.check_png_enc(lib.lsppng_enc_header(h, buf, N.PNGENC_HEADER_BYTES))
    return bytes(buf)


def capacity_bytes(width: int, height: int, channels: int = 3) -> int:
    """the bound of include/lsppngenc.h on a frame's bytes behind the 33-byte header: raw + 22 * chunks + 30; a level 0 file has exactly that many"""
    raw = int(height) * (1 + int(width) * int(channels))
    return raw + 22 * ((raw + CHUNK - 1) // CHUNK) + 30


def host_file(pixels: np.ndarray, level: int = 1, filter=None, stats: bool = False):
    """One frame (uint8 ``[H, W, 3]`` or ``[H, W]``) -> the complete PNG file on the host, with the code the kernels run (the lanes as loops): the
    file ``PngEncoder`` makes of the same pixels, bit for bit.  With ``stats`` also (chunks per block form [stored, fixed, dynamic], rows per
    filter [5]).  No device needed."""
    lib = N.load()
    px = np.ascontiguousarray(pixels)
    if px.dtype != np.uint8 or px.ndim not in (2, 3) or (px.ndim == 3 and px.shape[2] != 3):
        raise ValueError("pixels must be uint8 [H, W, 3] or [H, W] (got %s %s)" % (px.dtype, px.shape))
    channels = 3 if px.ndim == 3 else 1
    o = PngOptions.of(PngOptions(level, filter))
    h = _create(lib, px.shape[1], px.shape[0], channels, o)
    try:
        cap = N.PNGENC_HEADER_BYTES + int(lib.lsppng_enc_capacity_bytes(h))
        out = np.empty(cap, np.uint8)
        forms, rows = np.zeros(3, np.uint32), np.zeros(5, np.uint32)
        n = N.check_png_enc(lib.lsppng_enc_host_file(h, ctypes.c_void_p(px.ctypes.data), ctypes.c_void_p(out.ctypes.data), cap,
                                                     ctypes.c_void_p(forms.ctypes.data), ctypes.c_void_p(rows.ctypes.data)))
    finally:
        lib.lsppng_enc_destroy(h)
    data = out[:n].tobytes()
    return (data, forms.tolist(), rows.tolist()) if stats else data


def host_code_lengths(freq: Sequence[int], limit: int = 15) -> List[int]:
    """the encoder's length-limited code builder on the host (``lsppng_enc_host_code_lengths``): a length per symbol, 0 for an unused one"""
    lib = N.load()
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    out = np.zeros(f.size, np.uint8)
    N.check_png_enc(lib.lsppng_enc_host_code_lengths(ctypes.c_void_p(f.ctypes.data), int(f.size), int(limit), ctypes.c_void_p(out.ctypes.data)))
    return out.tolist()


class PngEncoder(JpegEncoder):
    """PNG of ``[B, H, W, 3]`` uint8 RGB frames (``Engine.forward_image``) or ``[B, H, W]`` uint8 grey frames (the edge maps of
    ``FeatureMapRasteriser.rasterise(..., as_uint8=True)``) of any size, B <= ``max_batch``: ``submit`` / ``enqueue`` / ``collect`` / ``encode``,
    ``slab`` and ``close`` are ``JpegEncoder``'s, the files lossless (include/lsppngenc.h).  ``level`` and ``filter``: ``PngOptions``."""
    _encode_symbol, _destroy_symbol, _check_rc = "lsppng_enc_encode", "lsppng_enc_destroy", staticmethod(N.check_png_enc)

    def __init__(self, size: Union[int, Sequence[int]], channels: int = 3, device="cuda:0", max_batch: int = 8, level: int = 1, filter=None):
        import torch
        self.lib = N.load()
        self.height, self.width = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        self.options = PngOptions.of(level if isinstance(level, PngOptions) else PngOptions(level, filter))
        self.channels, self.max_batch = int(channels), int(max_batch)
        if self.max_batch < 1:
            raise ValueError("max_batch must be >= 1")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the PNG encoder runs on the MI355X only (no CPU path); the reference's host path is Pillow's Image.save")
        self._h = _create(self.lib, self.width, self.height, self.channels, self.options)
        self.header = _header_of(self.lib, self._h)
        self._allocate(int(self.lib.lsppng_enc_capacity_bytes(self._h)), int(self.lib.lsppng_enc_workspace_bytes(self._h, self.max_batch)))

    def _aligned_src(self) -> bool:
        return False                                            # the filter kernel reads bytes


def save_images(save_root: str, files: Sequence[bytes], index0: int = 0, prefix: str = "pred") -> List[str]:
    """Write encoded frames as ``<save_root>/<prefix>_<ind + 1>.png`` for ind = index0, index0 + 1, ... (the names of jpeg.save_images)"""
    os.makedirs(save_root, exist_ok=True)
    paths = []
    for k, data in enumerate(files):
        path = os.path.join(save_root, "%s_%d.png" % (prefix, index0 + k + 1))
        with open(path, "wb") as f:
            f.write(data)
        paths.append(path)
    return paths
