#!/usr/bin/env python3
"""Writes tests/golden/jpeg_geometry.{json,npz}: what Pillow writes for `Image.fromarray(img).save(f, "JPEG", quality=q, subsampling=s,
optimize=..., restart_marker_rows=..., restart_marker_blocks=...)` on deterministic pictures of sizes that are no multiple of the MCU
(recipes of tests/jpeg_model.make_image), whole files, so that a machine without Pillow still compares against Pillow's bytes.  Records the
Pillow and libjpeg-turbo versions.   python tools/make_golden_jpeg_geometry.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_geometry_model as G  # noqa: E402
from PIL import Image, features  # noqa: E402

# (H, W): no padding at all; one block or less; even H with a dummy row under 4:2:0; odd H and W; a dummy column only; dummy combinations
SIZES = [(16, 16), (64, 36), (1, 1), (7, 5), (8, 8), (24, 24), (24, 40), (40, 24), (50, 34), (9, 23), (33, 47), (17, 33), (16, 24), (100, 75), (36, 64)]
# every geometry is a batch of three different pictures per quality; noise at q95 fills the 200 KB of the fixture on the five large sizes alone, so
# those take a flat picture in its place there (noise at q75 and smooth at q95 cover every size)
PICTURES = ["noise", "smooth", "gradient"]
PICTURES_LARGE_Q95 = ["flat", "smooth", "gradient"]
# (optimize, restart_rows, restart_blocks) on a few geometries, the smooth picture alone
OPTION_SETS = [(1, 0, 0), (0, 1, 0), (0, 0, 3), (1, 1, 0)]
OPTION_SIZES = [(33, 47), (50, 34), (7, 5)]


def cases():
    out = []
    for (h, w) in SIZES:
        for fmt in G.FORMATS:
            ch = 1 if fmt == "grey" else 3
            for q in (75, 95):
                sets = [(0, 0, 0)] + (OPTION_SETS if (h, w) in OPTION_SIZES and q == 75 else [])
                for (o, rows, blocks) in sets:
                    for kind in ((PICTURES_LARGE_Q95 if q == 95 and h * w > 1100 else PICTURES) if not (o or rows or blocks) else PICTURES[1:2]):
                        out.append([h, w, fmt, q, o, rows, blocks, kind])
    return out


def main():
    files, meta = [], cases()
    for row in meta:
        c = G.fixture_case(row)
        img = G.make_image(c["recipe"])
        data = G.pillow_bytes(Image, img, c["quality"], c["format"], c["optimize"], c["restart_rows"], c["restart_blocks"])
        assert G.encode(img, c["quality"], c["format"], bool(c["optimize"]), c["restart_rows"], c["restart_blocks"]) == data, c["name"]
        files.append(data)
    gold = os.path.join(ROOT, "tests", "golden")
    # one array of all files, in the order of the cases, and where each ends: the files share their tables, which compress away only side by side
    np.savez_compressed(os.path.join(gold, "jpeg_geometry.npz"), data=np.frombuffer(b"".join(files), np.uint8), ends=np.cumsum([len(f) for f in files]).astype(np.int64))
    with open(os.path.join(gold, "jpeg_geometry.json"), "w") as f:
        json.dump({"pillow": __import__("PIL").__version__, "libjpeg_turbo": features.version("jpg"),
                   "columns": ["h", "w", "format", "quality", "optimize", "restart_rows", "restart_blocks", "kind"], "cases": meta}, f, separators=(",", ":"))
    print("%d cases, %d bytes of files" % (len(meta), sum(len(f) for f in files)))


if __name__ == "__main__":
    main()
