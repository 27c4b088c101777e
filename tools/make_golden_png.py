#!/usr/bin/env python
"""Writes the fixtures of the PNG decoder's tests: tests/golden/png_dec.json + png_dec.npz (small files of every decoded kind with the pixels Pillow
returns for them) and png_dec_512.npz (four 512 x 512 candidate images; the json holds the SHA-256 of Pillow's pixels for them).  Run on the CPU with Pillow and the standard library's zlib:

    python tools/make_golden_png.py

The files are written with the tests' own PNG / deflate writer (tests/png_writer.py), because Pillow chooses its own filters and writes one dynamic
block: the fixtures need every filter, every block kind, chosen IDAT cuts and matches zlib never emits (distance 32768).  Every file is checked here
against Pillow AND against the model (tests/png_decode_model.py) before it is written.  Content is synthetic and seeded; the 512 x 512 images are
smooth so that the files stay small.
"""
import hashlib
import io
import json
import os
import struct
import sys
import zlib

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import png_decode_model as D  # noqa: E402
import png_writer as W  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CYCLE = [0, 1, 2, 3, 4]


def noise(shape, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.uint8)


def smooth(h, w, ch, seed):
    y, x = np.mgrid[:h, :w]
    planes = [((x * (2 + c) + y * (3 - c) + seed * 29) // 3 + ((x * y) >> 7) + 60 * c) & 255 for c in range(ch)]
    return np.stack(planes, 2).astype(np.uint8) if ch > 1 else planes[0].astype(np.uint8)


def rows_of(img, color_type, depth):
    if color_type == 3:
        return W.pack_indices(img, depth)
    return [img[y].tobytes() for y in range(img.shape[0])]


def deflate(raw, how):
    """the zlib stream of the filtered scanlines; `how` names the deflate variant"""
    kind = how[0]
    if kind == "zlib":
        _, level, strategy = how
        c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
        return c.compress(raw) + c.flush()
    if kind == "stored":                                       # level 0, with a zero-length stored block (a sync flush) in the middle
        c = zlib.compressobj(0)
        half = len(raw) // 2
        z = c.compress(raw[:half]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(raw[half:]) + c.flush()
        assert b"\x00\x00\xff\xff" in z
        return z
    if kind == "flushrows":                                    # a full flush after every row: many blocks
        _, stride = how
        c = zlib.compressobj(6)
        z = b"".join(c.compress(raw[k:k + stride]) + c.flush(zlib.Z_FULL_FLUSH) for k in range(0, len(raw), stride))
        return z + c.flush()
    w = W.BitWriter()
    if kind == "fixed_tokens":
        W.fixed_block(w, W.tokens_of(raw, how[1]))
    elif kind == "single_distance":                            # a dynamic block whose distance code is ONE code of one bit
        tokens = W.tokens_of(raw, [1])
        assert any(t[0] == "match" for t in tokens)
        W.dynamic_block(w, tokens, dist_lengths=[1])
    elif kind == "mixed":                                      # stored, fixed, dynamic and an empty fixed block in one stream
        a, b = len(raw) // 3, 2 * len(raw) // 3
        W.stored_block(w, raw[:a], final=False)
        W.fixed_block(w, [("lit", v) for v in raw[a:b]], final=False)
        W.fixed_block(w, [], final=False)
        W.dynamic_block(w, W.tokens_of(raw[b:], [1, 2, 3, 4, 6, 8]))
    else:
        raise ValueError(kind)
    return W.zlib_stream(w.done(), raw)


def build(img, color_type, depth, filters, how=("zlib", 6, zlib.Z_DEFAULT_STRATEGY), palette=None, raw=None, **container):
    """(file bytes, raw scanlines); `raw` overrides the filtered scanlines (files whose STREAM is the point)"""
    h, w = img.shape[:2]
    channels = {0: 1, 3: 1, 4: 2, 2: 3, 6: 4}[color_type]
    if raw is None:
        raw = W.filter_rows(rows_of(img, color_type, depth), max(1, channels * depth // 8), filters)
    return W.png(w, h, depth, color_type, deflate(raw, how), palette=palette, **container), raw


def pillow_pixels(data, color_type):
    return np.asarray(Image.open(io.BytesIO(data)).convert("L" if color_type in (0, 4) else "RGB"))


def raw_grey(h, w, fill):
    """filtered scanlines of a grey file given directly: fill(y) -> (filter byte, the w bytes behind it)"""
    out = bytearray()
    for y in range(h):
        ft, row = fill(y)
        assert 0 <= ft <= 4 and len(row) == w
        out.append(ft)
        out += bytes(row)
    return bytes(out)


def small_cases():
    """[(name, file, color_type, depth, note)]"""
    out = []

    def add(name, note, img, ct, depth, filters, **kw):
        data, _ = build(img, ct, depth, filters, **kw)
        out.append((name, data, ct, depth, note))

    Z = zlib.Z_DEFAULT_STRATEGY
    add("rgb_1x1", "the smallest file", noise((1, 1, 3), 1), 2, 8, [0])
    add("grey_w1_h70", "width 1, more rows than one band", noise((70, 1), 2), 0, 8, CYCLE)
    add("rgb_w3_h70", "width 3, more rows than one band", noise((70, 3, 3), 3), 2, 8, CYCLE, how=("zlib", 9, Z))
    add("rgba_65x5", "RGBA, alpha dropped", noise((5, 65, 4), 4), 6, 8, CYCLE, how=("zlib", 1, Z))
    add("ga_21x67", "grey + alpha, alpha dropped", noise((67, 21, 2), 5), 4, 8, CYCLE)
    add("grey_20x20", "grey", smooth(20, 20, 1, 6), 0, 8, CYCLE)
    add("rgb_64x64", "one band exactly", noise((64, 64, 3), 7), 2, 8, CYCLE)
    add("rgb_65x65", "one row into the second band", smooth(65, 65, 3, 8), 2, 8, CYCLE, how=("zlib", 9, Z))
    add("p1_13x9", "palette depth 1, partial last byte", noise((9, 13), 9, 0, 2), 3, 1, CYCLE, palette=noise(6, 10))
    add("p2_10x7", "palette depth 2, three entries used of three", noise((7, 10), 11, 0, 3), 3, 2, CYCLE, palette=noise(9, 12))
    add("p4_3x11", "palette depth 4 at width 3, partial last byte", noise((11, 3), 13, 0, 11), 3, 4, CYCLE, palette=noise(33, 14))
    add("p8_17x6", "palette depth 8, 200 entries", noise((6, 17), 15, 0, 200), 3, 8, CYCLE, palette=noise(600, 16))
    for ft in range(5):
        add("rgb_19x23_f%d" % ft, "every row filter %d" % ft, noise((23, 19, 3), 20 + ft) if ft < 3 else smooth(23, 19, 3, 20 + ft), 2, 8, [ft])
    img = smooth(17, 31, 3, 30) ^ (noise((17, 31, 3), 31) & 3)
    add("rgb_31x17_stored", "level 0: stored blocks, a zero-length one included", img, 2, 8, CYCLE, how=("stored",))
    add("rgb_31x17_fixed", "Z_FIXED", img, 2, 8, CYCLE, how=("zlib", 6, zlib.Z_FIXED))
    for level in (1, 6, 9):
        add("rgb_31x17_l%d" % level, "level %d" % level, img, 2, 8, CYCLE, how=("zlib", level, Z))
    add("rgb_31x17_flushrows", "a full flush after every row: many blocks", img, 2, 8, CYCLE, how=("flushrows", 1 + 31 * 3))
    add("rgb_31x17_mixed", "stored, fixed, empty fixed and dynamic blocks in one stream", img, 2, 8, CYCLE, how=("mixed",))

    # files whose stream is the point: the filtered scanlines are given, the picture is whatever they reconstruct to
    rng = np.random.default_rng(40)
    raw = raw_grey(6, 40, lambda y: (y % 5, [int(rng.integers(256))] * 20 + [int(rng.integers(256))] * 20))
    data, _ = build(np.zeros((6, 40), np.uint8), 0, 8, None, how=("single_distance",), raw=raw)
    out.append(("grey_40x6_single_distance", data, 0, 8, "a dynamic block whose distance code is a single code of one bit"))
    raw = raw_grey(2, 300, lambda y: (0, [0] * 300))
    tokens = W.tokens_of(raw, [1])
    assert ("match", 258, 1) in tokens
    data, _ = build(np.zeros((2, 300), np.uint8), 0, 8, None, how=("fixed_tokens", [1]), raw=raw)
    out.append(("grey_300x2_run258", data, 0, 8, "a run at distance 1 of length 258"))
    periods = (2, 3, 63, 64, 65)
    raw = raw_grey(5, 200, lambda y: (y % 5, [(k % periods[y]) * 3 + 5 + y for k in range(200)]))
    tokens = W.tokens_of(raw, periods)
    for d in periods:
        assert any(t[0] == "match" and t[2] == d and t[1] > d for t in tokens), d          # overlapping: longer than its distance
    data, _ = build(np.zeros((5, 200), np.uint8), 0, 8, None, how=("fixed_tokens", periods), raw=raw)
    out.append(("grey_200x5_overlaps", data, 0, 8, "overlapping matches at distances 2, 3, 63, 64 and 65"))

    # 128 x 128 RGB: 49280 bytes of scanlines, past the 32 KiB window; noise, so every match is one placed here
    stride = 1 + 128 * 3
    lines = bytearray(W.filter_rows([noise(384, 50 + y).tobytes() for y in range(128)], 3, [0]))
    at = 2 * stride + 1 + 32768                                # a match at distance exactly 32768: row 2's first bytes again
    assert at // stride == 87 and at % stride + 200 < stride
    lines[at:at + 200] = lines[at - 32768:at - 32768 + 200]
    lines[32750:32790] = lines[32750 - 3 * stride:32790 - 3 * stride]      # a match written across the ring's wrap (position 32768)
    lines[32760 + stride:32795 + stride] = lines[32760:32795]              # and one read across it
    raw = bytes(lines)
    tokens = W.tokens_of(raw, [32768, 3 * stride, stride], min_len=20)
    assert ("match", 200, 32768) in tokens and ("match", 40, 3 * stride) in tokens and ("match", 35, stride) in tokens
    w = W.BitWriter()
    W.fixed_block(w, tokens)
    data = W.png(128, 128, 8, 2, W.zlib_stream(w.done(), raw))
    out.append(("rgb_128x128_window", data, 2, 8, "scanlines past 32 KiB: a match at distance 32768, one written and one read across the ring's wrap"))

    img = noise((9, 9, 3), 60)
    add("rgb_9x9_idat1", "IDAT cut after every byte, an empty IDAT in between", img, 2, 8, CYCLE, every=1, empty_between=True)
    add("rgb_9x9_idat17", "IDAT cut every 17 bytes, an empty IDAT in between", img, 2, 8, CYCLE, every=17, empty_between=True)
    add("rgb_64x64_idat8192", "IDAT cut every 8192 bytes, an empty IDAT in between", noise((64, 64, 3), 61), 2, 8, CYCLE, every=8192, empty_between=True)
    before = [W.chunk(b"gAMA", struct.pack(">I", 45455)), W.chunk(b"pHYs", struct.pack(">IIB", 2835, 2835, 1)), W.chunk(b"tEXt", b"Comment\0a fixture"),
              W.chunk(b"tRNS", struct.pack(">HHH", 1, 2, 3))]
    after = [W.chunk(b"tEXt", b"Comment\0behind the data"), W.chunk(b"tIME", struct.pack(">HBBBBB", 2026, 10, 21, 0, 0, 0))]
    add("rgb_12x10_ancillary", "gAMA, pHYs, tEXt, tRNS before IDAT; tEXt, tIME after", noise((10, 12, 3), 62), 2, 8, CYCLE, before=before, after=after)
    data, _ = build(noise((5, 7), 63, 0, 4), 3, 2, CYCLE, palette=noise(12, 64))
    chunks = W.chunks_of(data)
    k = next(i for i, c in enumerate(chunks) if c[0] == b"IDAT")
    data = W.rebuild(chunks[:k] + [(b"tRNS", bytes([0, 128, 255]))] + chunks[k:])
    out.append(("p2_7x5_trns", data, 3, 2, "a palette file with tRNS: the palette colours, no alpha"))
    return out


def candidates():
    """four 512 x 512 files that give 3 components: RGB, RGBA, palettised, and one saved by Pillow itself with optimize=True"""
    out = []
    data, _ = build(smooth(512, 512, 3, 70), 2, 8, CYCLE, how=("zlib", 9, zlib.Z_DEFAULT_STRATEGY), every=8192)
    out.append(("cand_rgb", data))
    data, _ = build(smooth(512, 512, 4, 71), 6, 8, [4])
    out.append(("cand_rgba", data))
    idx = ((smooth(512, 512, 1, 72).astype(np.int32) * 200) >> 8).astype(np.uint8)
    data, _ = build(idx, 3, 8, [0, 2], palette=smooth(1, 200, 3, 73).reshape(-1))
    out.append(("cand_palette", data))
    b = io.BytesIO()
    Image.fromarray(smooth(512, 512, 3, 74)).save(b, "PNG", optimize=True)
    out.append(("cand_pillow_optimize", b.getvalue()))
    return out


def main():
    meta, files, arrays = {"pillow": Image.__version__, "cases": [], "candidates": []}, {}, {}
    for name, data, ct, depth, note in small_cases():
        px = pillow_pixels(data, ct)
        assert np.array_equal(D.decode(data), px), name
        f = D.parse(data)
        meta["cases"].append({"name": name, "width": f["width"], "height": f["height"], "color_type": ct, "depth": depth, "note": note,
                              "idat_bytes": len(f["idat"]), "pixels_sha256": hashlib.sha256(px.tobytes()).hexdigest()})
        arrays[name + ".png"] = np.frombuffer(data, np.uint8)
        arrays[name + ".px"] = px
    np.savez_compressed(os.path.join(GOLDEN, "png_dec.npz"), **arrays)
    big = {}
    for name, data in candidates():
        px = pillow_pixels(data, 2)
        assert px.shape == (512, 512, 3) and np.array_equal(D.decode(data), px), name
        meta["candidates"].append({"name": name, "bytes": len(data), "color_type": D.parse(data)["color_type"],
                                   "pixels_sha256": hashlib.sha256(px.tobytes()).hexdigest()})
        big[name + ".png"] = np.frombuffer(data, np.uint8)
    np.savez_compressed(os.path.join(GOLDEN, "png_dec_512.npz"), **big)
    with open(os.path.join(GOLDEN, "png_dec.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    for n in ("png_dec.json", "png_dec.npz", "png_dec_512.npz"):
        print(n, os.path.getsize(os.path.join(GOLDEN, n)))


if __name__ == "__main__":
    main()
