#!/usr/bin/env python3
"""Writes tests/golden/jpeg_prog.{json,npz} and tests/golden/jpeg_prog_512.npz: progressive JPEG files written by Pillow (``save(progressive=True)``), the pixels
``numpy.asarray(Image.open(f))`` returns for them, and each file's baseline twin (same image, same keywords, no ``progressive``), which the
baseline decoder reads: a second oracle beside Pillow, because a complete progressive file holds the twin's coefficients.

  small cases   (jpeg_prog.npz) "<name>.jpg" the progressive file, "<name>.twin" the baseline twin, "<name>.px" the pixels.  Sizes (h x w) and samplings are the
                smallest that can go wrong: 1x1, 2x3, 9x2 (one block, fewer blocks than an MCU), 17x33 and 31x18 in 4:2:0 and 4:2:2 (partial
                MCUs: a component's own extent is narrower than the MCU grid), 8x24 in 4:4:4, 40x72 and 64x64 in each sampling and grey; each
                plain, with restart_marker_rows=1 and with restart_marker_blocks 1 / 3, with optimize off and on; kinds noise / smooth / extremes
                and qualities 1 / 30 / 75 / 95 / 100 rotate through them;
  constant_512  (jpeg_prog_512.npz, like the next) one constant 512^2 colour frame: end-of-band runs of thousands of blocks (the 12-to-14-bit EOBn symbols) in a file of a few
                hundred bytes; the file and its twin are stored, of the pixels the sha256;
  candidates    four 512^2 `smooth` files at quality 95, progressive: the recipes of candidate_{j}_512_q95 in tests/golden/jpeg_dec_512.npz, which
                are their baseline twins (the twins' pixel sha256 there must equal the one recorded here); the files are stored, of the pixels
                the sha256.

Every file is checked against tests/jpeg_progressive_model.py, and its coefficients against the twin's from tests/jpeg_decode_model.py, before
it is written.   python tools/make_golden_jpeg_progressive.py"""
import hashlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_decode_model as D  # noqa: E402
import jpeg_model as M  # noqa: E402
import jpeg_progressive_model as P  # noqa: E402
from PIL import Image, features  # noqa: E402

MODES = {"420": (3, {"subsampling": 2}), "422": (3, {"subsampling": 1}), "444": (3, {"subsampling": 0}), "grey": (1, {})}
GEOMETRIES = ([((h, w), m) for h, w in ((1, 1), (2, 3), (9, 2)) for m in ("420", "grey")] + [((h, w), m) for h, w in ((17, 33), (31, 18)) for m in ("420", "422")]
              + [((8, 24), "444")] + [((h, w), m) for h, w in ((40, 72), (64, 64)) for m in ("444", "422", "420", "grey")])
RESTARTS = (("plain", {}), ("rstr", {"restart_marker_rows": 1}), ("rstb1", {"restart_marker_blocks": 1}), ("rstb3", {"restart_marker_blocks": 3}))
QUALITIES = (1, 30, 75, 95, 100)
KINDS = ("noise", "smooth", "extremes")


def pil_bytes(img, **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", **kw)
    return b.getvalue()


def pil_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)))


def small_cases():
    out, k = [], 0
    for (h, w), mode in GEOMETRIES:
        ch, kw = MODES[mode]
        for rname, rkw in RESTARTS:
            for opt in (False, True):
                kind = "noise" if ch == 1 else KINDS[k % 3]
                q = QUALITIES[(k // 3 + k) % 5]
                save = dict(kw, **rkw)
                if opt:
                    save["optimize"] = True
                out.append({"name": "%s_%s_%s%s_%dx%d_q%d" % (kind, mode, rname, "_opt" if opt else "", h, w, q), "quality": q, "save": save,
                            "recipe": {"kind": kind, "h": h, "w": w, "channels": ch, "seed": 1300 + k}})
                k += 1
    return out


def checked(name, img, quality, save):
    """(progressive file, twin, pixels): the model gives Pillow's pixels, Pillow gives the twin's pixels, the coefficients are the twin's"""
    prog, twin = pil_bytes(img, quality=quality, progressive=True, **save), pil_bytes(img, quality=quality, **save)
    px = pil_pixels(prog)
    assert D.status_of(prog) == D.UNSUPPORTED and np.array_equal(pil_pixels(twin), px), name
    f = P.parse(prog)
    coef = P.coefficients(prog, f)
    assert np.array_equal(D.pixels_from(coef, P.as_baseline(f)), px), "the model disagrees with Pillow on %s" % name
    assert np.array_equal(coef, D.coefficients(twin)), "%s: not the twin's coefficients" % name
    return prog, twin, px


def main():
    meta = {"pillow": Image.__version__, "libjpeg_turbo": features.version("libjpeg_turbo"), "reader": "numpy.asarray(Image.open(f))", "cases": [], "frames": []}
    z, big = {}, {}
    for c in small_cases():
        prog, twin, px = checked(c["name"], M.make_image(c["recipe"]), c["quality"], c["save"])
        z[c["name"] + ".jpg"], z[c["name"] + ".twin"], z[c["name"] + ".px"] = np.frombuffer(prog, np.uint8), np.frombuffer(twin, np.uint8), px
        meta["cases"].append(dict(c, length=len(prog), scans=len(P.parse(prog)["scans"])))
    sha = lambda px: hashlib.sha256(np.ascontiguousarray(px).tobytes()).hexdigest()
    img = np.empty((512, 512, 3), np.uint8)
    img[:] = (37, 150, 201)
    prog, twin, px = checked("constant_512", img, 75, {})
    big["constant_512.jpg"], big["constant_512.twin"] = np.frombuffer(prog, np.uint8), np.frombuffer(twin, np.uint8)
    meta["frames"].append({"name": "constant_512", "quality": 75, "colour": [37, 150, 201], "length": len(prog), "shape": list(px.shape), "pixels_sha256": sha(px)})
    dec = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "jpeg_dec.json")))["frames"]}
    twins = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_dec_512.npz"))
    for j in range(4):
        name, of = "candidate_%d_512_q95_prog" % j, "candidate_%d_512_q95" % j
        prog, twin, px = checked(name, M.make_image(dec[of]["recipe"]), 95, {})
        assert twin == twins[of + ".jpg"].tobytes() and sha(px) == dec[of]["pixels_sha256"], "%s is not the twin of %s" % (of, name)
        big[name + ".jpg"] = np.frombuffer(prog, np.uint8)
        meta["frames"].append({"name": name, "quality": 95, "recipe": dec[of]["recipe"], "twin": of, "length": len(prog), "shape": list(px.shape),
                               "pixels_sha256": sha(px)})
        print("%-28s %7d bytes" % (name, len(prog)), flush=True)
    g = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(g, "jpeg_prog.npz"), **z)
    np.savez_compressed(os.path.join(g, "jpeg_prog_512.npz"), **big)
    with open(os.path.join(g, "jpeg_prog.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
        fh.write("\n")
    for n in ("jpeg_prog.npz", "jpeg_prog_512.npz", "jpeg_prog.json"):
        print(n, os.path.getsize(os.path.join(g, n)), "bytes")


if __name__ == "__main__":
    main()
