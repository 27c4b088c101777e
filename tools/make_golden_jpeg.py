#!/usr/bin/env python3
"""Writes tests/golden/jpeg_pil.{json,npz}: what Pillow writes for `Image.fromarray(img).save(f, "JPEG", quality=q)` on deterministic
images (recipes of tests/jpeg_model.make_image, pixels from synth's counter hash), so that a machine without Pillow still compares
against Pillow's bytes.  Small images keep the whole file (npz), frames of 512^2 and up its length and sha256.  Records the Pillow and
libjpeg-turbo versions.   python tools/make_golden_jpeg.py"""
import hashlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_model as M  # noqa: E402
from PIL import Image, features  # noqa: E402

QUALITIES = (1, 10, 50, 75, 90, 95, 100)


def pil(img, q):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=q)
    return b.getvalue()


def cases():
    out = []

    def add(name, q, **r):
        out.append({"name": name, "quality": q, "recipe": r})

    for q in QUALITIES:
        add("gradient_c_48x64_q%d" % q, q, kind="gradient", h=48, w=64, channels=3)
        add("noise_c_32x32_q%d" % q, q, kind="noise", h=32, w=32, channels=3, seed=11)
        add("edges_g_64x64_q%d" % q, q, kind="edges", h=64, w=64, channels=1, seed=12, segments=6)
        add("noise_g_24x40_q%d" % q, q, kind="noise", h=24, w=40, channels=1, seed=13)
    add("flat_c_32x32_q75", 75, kind="flat", h=32, w=32, channels=3, value=128)
    add("flat_c_32x32_q100", 100, kind="flat", h=32, w=32, channels=3, value=37)
    add("flat_g_16x16_q75", 75, kind="flat", h=16, w=16, channels=1, value=200)
    for q in (1, 75, 100):
        add("primaries_c_32x48_q%d" % q, q, kind="primaries", h=32, w=48, channels=3)
    for q in (1, 100):
        add("extremes_c_64x64_q%d" % q, q, kind="extremes", h=64, w=64, channels=3)
    add("extremes_g_64x64_q100", 100, kind="extremes", h=64, w=64, channels=1)
    for q in (50, 75, 90):
        add("sparse_c_64x64_q%d" % q, q, kind="sparse", h=64, w=64, channels=3)
    add("sparse_g_64x64_q75", 75, kind="sparse", h=64, w=64, channels=1)
    add("noise_c_64x64_q100", 100, kind="noise", h=64, w=64, channels=3, seed=14)
    # the final, padded byte of the scan is 0xFF (so it is stuffed too): the first seed that gives one
    for seed in range(1000, 5000):
        r = dict(kind="noise", h=16, w=16, channels=1, seed=seed)
        img = M.make_image(r)
        data, bits = M.entropy_code(*M.coefficients(img, 75), with_bits=True)
        if bits % 8 and data.endswith(b"\xff\x00"):
            add("final_ff_g_16x16_q75", 75, **r)
            break
    # frames (length + sha256 only)
    for q in QUALITIES:
        add("golden_normal_512_q%d" % q, q, kind="golden", case="normal_512", h=512, w=512, channels=3)
        add("edges_g_512_q%d" % q, q, kind="edges", h=512, w=512, channels=1, seed=21, segments=60)
    add("golden_large_512_q75", 75, kind="golden", case="large_512", h=512, w=512, channels=3)
    for k in range(8):                                       # eight different frames of each kind: the slots of a batch
        add("smooth_c_512_s%d_q75" % k, 75, kind="smooth", h=512, w=512, channels=3, seed=100 + k)
        add("edges_g_512_s%d_q75" % k, 75, kind="edges", h=512, w=512, channels=1, seed=200 + k, segments=40)
    for s in (768, 1024):
        add("smooth_c_%d_q75" % s, 75, kind="smooth", h=s, w=s, channels=3, seed=300 + s)
        add("edges_g_%d_q75" % s, 75, kind="edges", h=s, w=s, channels=1, seed=400 + s, segments=40)
    add("noise_c_1024_q100", 100, kind="noise", h=1024, w=1024, channels=3, seed=500)
    return out


def main():
    meta = {"pillow": Image.__version__, "libjpeg_turbo": features.version("libjpeg_turbo"), "libjpeg": features.version("jpg"),
            "writer": "Image.fromarray(img).save(f, 'JPEG', quality=q)", "cases": []}
    arrays = {}
    for c in cases():
        img = M.make_image(c["recipe"])
        data = pil(img, c["quality"])
        assert M.encode(img, c["quality"]) == data, "the model disagrees with Pillow on %s" % c["name"]
        c = dict(c, length=len(data), sha256=hashlib.sha256(data).hexdigest())
        if img.shape[0] * img.shape[1] < 512 * 512:
            arrays[c["name"]] = np.frombuffer(data, np.uint8)
        meta["cases"].append(c)
        print("%-28s %7d bytes" % (c["name"], len(data)), flush=True)
    g = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(g, "jpeg_pil.npz"), **arrays)
    with open(os.path.join(g, "jpeg_pil.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
