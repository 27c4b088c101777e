"""Pillow 12's Resample.c for 8 bits per channel (modes L and RGB), restated in numpy: the model the device resampler (include/lspresize.h) and
its host planner are held to.  Not imported by the product.

    coefficients(in, out, filter)   precompute_coeffs + normalize_coeffs_8bpc of one axis: (ksize, bounds [out, 2], k int32 [out, ksize])
    resample(img, bounds, k, axis)  one pass: clamp((2^21 + sum pixel * k) >> 22, 0, 255)
    resize(img, (width, height), filter)   Image.resize: horizontal first (only when the width changes, only the rows the vertical pass
                                    reads, rounded to uint8), then vertical (only when the height changes)

The filters are evaluated with ``math.sin`` / ``math.cos`` (libm, what Pillow's C calls), one value at a time, and summed in index order.
"""
from __future__ import annotations

import functools
import hashlib
import math

import numpy as np

FILTERS = ("box", "bilinear", "hamming", "bicubic", "lanczos")          # the library's filter ids are the indices
SUPPORT = {"box": 0.5, "bilinear": 1.0, "hamming": 1.0, "bicubic": 2.0, "lanczos": 3.0}
PRECISION_BITS = 32 - 8 - 2
_C054, _C046 = float(np.float32(0.54)), float(np.float32(0.46))           # Resample.c writes 0.54f and 0.46f: float literals widened to double


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (_C054 + _C046 * math.cos(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FUNCTIONS = {"box": _box, "bilinear": _bilinear, "hamming": _hamming, "bicubic": _bicubic, "lanczos": _lanczos}


@functools.lru_cache(maxsize=None)
def coefficients(n_in: int, n_out: int, filt: str):
    f, scale = FUNCTIONS[filt], n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[filt] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        kk[xx, :xmax] = [int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5) for v in w]
        bounds[xx] = (xmin, xmax)
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return ksize, bounds, kk


def resample(img: np.ndarray, bounds: np.ndarray, kk: np.ndarray, axis: int, first: int = 0) -> np.ndarray:
    """one pass along ``axis`` (0: vertical, 1: horizontal) of uint8 [H, W] or [H, W, C]; ``first`` is the index ``img``'s first row / column has"""
    # float64 holds every product and partial sum exactly (integers below 2^31), so BLAS may do the sums
    src = np.moveaxis(img, axis, 0).astype(np.float64)
    out = np.empty((len(bounds),) + src.shape[1:], np.uint8)
    for i, (lo, n) in enumerate(np.asarray(bounds).tolist()):
        k = np.asarray(kk[i, :n], np.float64)
        assert np.abs(k).sum() * 255 + (1 << (PRECISION_BITS - 1)) < 2 ** 31, "the int32 accumulator of Resample.c could overflow"
        acc = np.tensordot(k, src[lo - first:lo - first + n], 1).astype(np.int64) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def check_arguments(img: np.ndarray, size, filt: str):
    if filt not in FILTERS:
        raise ValueError("filter %r is not offered" % (filt,))
    if img.dtype != np.uint8 or not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)):
        raise ValueError("uint8 [H, W] or [H, W, 3]")
    w, h = (size, size) if isinstance(size, int) else size
    return int(w), int(h)


def resize(img: np.ndarray, size, filt: str = "bicubic") -> np.ndarray:
    """``np.asarray(Image.fromarray(img).resize(size, filter))`` for uint8 [H, W] / [H, W, 3]; ``size`` is an int or (width, height)"""
    w, h = check_arguments(img, size, filt)
    H, W = img.shape[:2]
    need_h, need_v = w != W, h != H
    if need_v:
        _, vb, vk = coefficients(H, h, filt)
        row0, rows = int(vb[0, 0]), int(vb[-1, 0] + vb[-1, 1] - vb[0, 0])
    else:
        row0, rows = 0, H
    out = img
    if need_h:
        _, hb, hk = coefficients(W, w, filt)
        out = resample(img[row0:row0 + rows], hb, hk, 1)
    if need_v:
        out = resample(out, vb, vk, 0, first=row0 if need_h else 0)
    return out.copy() if out is img else out


def resize_with(img: np.ndarray, axes) -> np.ndarray:
    """the two passes with GIVEN coefficients: ``axes`` = (horizontal, vertical), each None or (bounds, k) -- the library planner's, say"""
    hor, ver = axes
    row0, rows = (int(ver[0][0, 0]), int(ver[0][-1, 0] + ver[0][-1, 1] - ver[0][0, 0])) if ver is not None else (0, img.shape[0])
    out = img
    if hor is not None:
        out = resample(img[row0:row0 + rows], hor[0], hor[1], 1)
    if ver is not None:
        out = resample(out, ver[0], ver[1], 0, first=row0 if hor is not None else 0)
    return out.copy() if out is img else out


def digest(bounds_k_pairs) -> int:
    """rszcore::plan_digest: FNV-1a 64 over (ksize, bounds, coefficients) of the horizontal axis, then the vertical one (those that run)"""
    h = 1469598103934665603
    for ksize, bounds, kk in bounds_k_pairs:
        data = np.int32(ksize).tobytes() + np.ascontiguousarray(bounds, "<i4").tobytes() + np.ascontiguousarray(kk, "<i4").tobytes()
        for b in data:
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def sha256(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the cases of the tests and of tools/make_golden_resize.py ------------------------------------------------------------------------
# (in_h, in_w, out_h, out_w, kind): the smallest shapes at which the kernels can still go wrong
GEOMETRIES = [
    (1, 1, 1, 1, "noise"), (64, 64, 64, 64, "noise"),                                     # copy
    (64, 64, 64, 32, "noise"), (64, 64, 32, 64, "noise"),                                 # one pass only, each way
    (2, 2, 31, 29, "noise"),                                                              # upscale, every window clipped at an edge
    (17, 1, 3, 40, "noise"),                                                              # a side of 1
    (5, 7, 16, 16, "binary"),                                                             # only 0 and 255: BICUBIC / LANCZOS overshoot into the clamp
    (37, 53, 64, 48, "noise"),                                                            # up on one axis, down on the other; widths no multiple of 4
    (100, 60, 33, 200, "smooth"),                                                         # non-integer ratios
    (257, 255, 64, 64, "noise"),                                                          # windows that straddle tile edges; odd sizes
    (1080, 1920, 512, 512, "smooth"),                                                     # 25 taps
    (512, 512, 256, 256, "smooth"), (512, 512, 384, 384, "smooth"), (512, 512, 171, 171, "smooth"), (512, 512, 360, 640, "smooth"),   # the product's own sizes
    (2100, 1500, 5, 20, "noise"),                                                         # tap counts past the LDS budget: the general path of both passes
]
# geometries the planner is also held to (no pixels): (in, out) of one axis
PLANNER_AXES = [(8192, 3), (8192, 4096), (8192, 1), (1, 8192), (8192, 8191)]
BATCH = 3
CANDIDATE_SIZES = [(64, 48), (96, 96), (33, 70), (128, 100)]           # (width, height) of the JPEG files of the load_candidates test


def make_image(recipe: dict) -> np.ndarray:
    """jpeg_model.make_image, plus kind "binary": its noise thresholded to 0 / 255"""
    from jpeg_model import make_image as base
    if recipe["kind"] == "binary":
        return np.where(base(dict(recipe, kind="noise")) >= 128, 255, 0).astype(np.uint8)
    return base(recipe)


def cases():
    """every case: a dict with the input recipe of image 0 (image i of the batch has seed + i), the output size and the filter"""
    out = []
    for g, (ih, iw, oh, ow, kind) in enumerate(GEOMETRIES):
        for ch in (1, 3):
            for filt in FILTERS:
                out.append({"name": "%dx%d_%dx%d_c%d_%s" % (ih, iw, oh, ow, ch, filt), "kind": kind, "h": ih, "w": iw, "channels": ch, "seed": 1000 + 10 * g + ch,
                            "out_h": oh, "out_w": ow, "filter": filt})
    return out


@functools.lru_cache(maxsize=None)
def _batch(kind, h, w, channels, seed):
    a = np.stack([make_image({"kind": kind, "h": h, "w": w, "channels": channels, "seed": seed + i}) for i in range(BATCH)])
    a.setflags(write=False)
    return a


def batch_of(case: dict) -> np.ndarray:
    """uint8 [BATCH, h, w(, 3)]: three DIFFERENT images (read-only, shared between the tests)"""
    return _batch(case["kind"], case["h"], case["w"], case["channels"], case["seed"])
