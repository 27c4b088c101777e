"""The cases of the PNG encoder's tests (include/lsppngenc.h), made from seeds: shared by tests/test_png_encode_cpu.py and tests/test_gpu_png_encode.py.
A case is (name, pixels uint8 [H, W] or [H, W, 3], level, filter); filter None is the per-row heuristic.  Test infrastructure."""
import functools
import random

import numpy as np

CHUNK = 16384                                                   # LSPPNG_ENC_CHUNK
HEADER = 33


def smooth(h, w, channels, seed):
    """a gradient with a little noise: Sub / Up / Average / Paeth all have something to win, and the filtered stream has matches"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = [(x * (3 + c) + y * (5 - c) + rng.integers(0, 3, (h, w))) % 256 for c in range(channels)]
    px = np.stack(planes, -1).astype(np.uint8)
    return px if channels == 3 else px[..., 0]


def noise(h, w, channels, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3) if channels == 3 else (h, w), dtype=np.uint8)


def periodic_rows(h, w, period, seed):
    """grey noise rows repeating every ``period`` rows: with filter 0 the stream repeats every period * (1 + w) bytes and nowhere sooner"""
    rows = noise(period, w, 1, seed)
    return np.ascontiguousarray(rows[np.arange(h) % period])


def line_drawing(size=512, lines=90, seed=5):
    """a binary edge map: ``lines`` two-pixel lines from a seeded generator"""
    from PIL import Image, ImageDraw
    rnd = random.Random(seed)
    im = Image.new("L", (size, size), 0)
    draw = ImageDraw.Draw(im)
    for _ in range(lines):
        draw.line([rnd.randrange(size) for _ in range(4)], fill=255, width=2)
    return np.asarray(im).copy()


# (width, height) of grey images whose filtered stream is CHUNK - 1, CHUNK, CHUNK + 1 and 2 * CHUNK + 1 bytes
STREAM_EDGES = [(128, 127), (127, 128), (144, 113), (330, 99)]
assert [h * (1 + w) for w, h in STREAM_EDGES] == [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
TINY = [(1, 1), (2, 1), (1, 3), (3, 2), (17, 5)]                # (width, height)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for w, h in TINY:
        for ch in (1, 3):
            for level in (0, 1):
                out.append(("tiny_%dx%d_c%d_l%d" % (w, h, ch, level), smooth(h, w, ch, 10 + w + h), level, None))
    for ch in (1, 3):
        for f in range(5):
            for level in (0, 1):
                out.append(("fixed_filter%d_c%d_l%d" % (f, ch, level), smooth(40, 37, ch, 20 + f), level, f))
    for k, (w, h) in enumerate(STREAM_EDGES):
        out.append(("stream_edge_%d" % (h * (1 + w)), smooth(h, w, 1, 30 + k), 1, None))
        out.append(("stream_edge_%d_stored" % (h * (1 + w)), noise(h, w, 1, 40 + k), 1, None))
    out.append(("match_across_chunks", periodic_rows(256, 127, 16, 50), 1, 0))      # the period is 2048 bytes: chunk 1 can only copy from chunk 0
    out.append(("constant_64", np.full((64, 64), 7, np.uint8), 1, None))
    out.append(("five_filters", noise(64, 64, 1, 60), 1, None))
    out.append(("noise_rgb_128", noise(128, 128, 3, 61), 1, None))
    out.append(("noise_rgb_128_l0", noise(128, 128, 3, 61), 0, None))
    out.append(("smooth_rgb_96x80", smooth(80, 96, 3, 62), 1, None))
    out.append(("lines_128", line_drawing(128, 12, 63), 1, None))
    return out


@functools.lru_cache(maxsize=None)
def wide_cases():
    """the two geometries at LSPPNG_MAX_SIDE (host tests only: the GPU tests stop at 512 x 512)"""
    row = noise(1, 8192, 3, 70)
    return [("wide_8192x2", np.ascontiguousarray(np.concatenate([row, row])), 1, 0),       # row 1 copies row 0 from 24 577 bytes back
            ("tall_2x8192", smooth(8192, 2, 3, 71), 1, None)]


def capacity(px):
    raw = px.shape[0] * (1 + px.shape[1] * (3 if px.ndim == 3 else 1))
    return raw + 22 * ((raw + CHUNK - 1) // CHUNK) + 30
