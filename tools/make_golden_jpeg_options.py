#!/usr/bin/env python3
"""Writes tests/golden/jpeg_options.{json,npz}: what Pillow writes for `Image.fromarray(img).save(f, "JPEG", quality=q, optimize=...,
restart_marker_rows=..., restart_marker_blocks=...)` on deterministic images (recipes of tests/jpeg_model.make_image and the limiter
picture of tests/jpeg_options_model), whole files, so that a machine without Pillow still compares against Pillow's bytes.  Records the
Pillow and libjpeg-turbo versions.   python tools/make_golden_jpeg_options.py"""
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_model as M  # noqa: E402
import jpeg_options_model as O  # noqa: E402
from PIL import Image, features  # noqa: E402

# (optimize, restart_rows, restart_blocks)
ALL_SETS = [(o, r, b) for o in (0, 1) for (r, b) in ((0, 0), (1, 0), (2, 0), (0, 1), (0, 3))]
FEW_SETS = [(0, 1, 0), (1, 0, 0), (1, 0, 3), (1, 2, 0), (0, 0, 1)]


def pil(img, q, optimize, rows, blocks):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=q, optimize=bool(optimize), restart_marker_rows=rows, restart_marker_blocks=blocks)
    return b.getvalue()


def cases():
    out = []

    def add(name, q, sets, **r):
        for (o, rows, blocks) in sets:
            out.append({"name": "%s_q%d_o%d_r%d_b%d" % (name, q, o, rows, blocks), "image": name, "quality": q, "optimize": o,
                        "restart_rows": rows, "restart_blocks": blocks, "recipe": r})

    small = [("noise_c_16x16", dict(kind="noise", h=16, w=16, channels=3, seed=21)),
             ("smooth_c_48x48", dict(kind="smooth", h=48, w=48, channels=3, seed=22)),       # 9 MCUs: restart_blocks=1 wraps RSTn
             ("noise_g_8x8", dict(kind="noise", h=8, w=8, channels=1, seed=23)),
             ("edges_g_24x40", dict(kind="edges", h=24, w=40, channels=1, seed=24, segments=4)),
             ("batch0_c_32x48", dict(kind="smooth", h=32, w=48, channels=3, seed=25)),       # a batch of three whose frames get different tables
             ("batch1_c_32x48", dict(kind="noise", h=32, w=48, channels=3, seed=26)),
             ("batch2_c_32x48", dict(kind="flat", h=32, w=48, channels=3, value=90))]
    for name, r in small:
        add(name, 75, ALL_SETS, **r)
    for q in (1, 50, 95, 100):
        add("smooth_c_48x48", q, FEW_SETS, **small[1][1])
        add("edges_g_24x40", q, FEW_SETS, **small[3][1])
    add("flat_g_16x16", 75, [(1, 0, 0), (1, 0, 1)], kind="flat", h=16, w=16, channels=1, value=200)     # the AC table holds EOB alone
    # a restart interval (not the last) whose padded byte is 0xFF and gets stuffed: the first seed that gives one
    for seed in range(3000, 9000):
        r = dict(kind="noise", h=16, w=16, channels=1, seed=seed)
        info = {}
        O.encode(M.make_image(r), 75, False, 1, info)
        if any(info["stuffed_pad"][:-1]):
            add("pad_ff_g_16x16", 75, [(0, 0, 1), (1, 0, 1)], **r)
            break
    else:
        raise SystemExit("no seed gives a stuffed padding byte")
    # a table that goes through the 16-bit limit (tests/jpeg_options_model.limiter_image)
    add("limiter_g_848x512", 25, [(1, 0, 0), (1, 1, 0)], kind="limiter", h=848, w=512, channels=1, quality=25, nsym=17)
    return out


def main():
    arrays, meta = {}, []
    for c in cases():
        img = O.make_image(c["recipe"])
        data = pil(img, c["quality"], c["optimize"], c["restart_rows"], c["restart_blocks"])
        r = O.restart_interval(img.shape[1], c["recipe"]["channels"], c["restart_rows"], c["restart_blocks"])
        assert O.encode(img, c["quality"], bool(c["optimize"]), r) == data, c["name"]
        arrays[c["name"]] = np.frombuffer(data, np.uint8)
        meta.append(c)
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "jpeg_options.npz"), **arrays)
    with open(os.path.join(gold, "jpeg_options.json"), "w") as f:
        json.dump({"pillow": Image.__version__ if hasattr(Image, "__version__") else __import__("PIL").__version__,
                   "libjpeg_turbo": features.version("jpg"), "cases": meta}, f, indent=1)
    print("%d cases, %d bytes of files" % (len(meta), sum(a.size for a in arrays.values())))


if __name__ == "__main__":
    main()
