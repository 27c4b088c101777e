#!/usr/bin/env python3
"""Writes tests/golden/jpeg_dec.{json,npz} and tests/golden/jpeg_dec_512.npz: JPEG files written by Pillow and the pixels
``numpy.asarray(Image.open(f))`` returns for them, so that a machine without Pillow still compares the decoder against Pillow's pixels.

  small cases (jpeg_dec.npz)   "<name>.jpg" the file, "<name>.px" the pixels: every listed size (the ones whose chroma is at most 2 samples
                               wide among them) x {4:2:0, 4:4:4, 4:2:2, optimised tables, restart_marker_blocks=3, restart_marker_rows=1,
                               grey, grey with restart rows}, image kinds and qualities 1 / 30 / 75 / 95 / 100 rotating through them;
  four 64^2 `smooth` files     at quality 95: candidate images at the size of the golden case normal_s64_b3;
  two files without DHT        the decoder then uses Annex K's tables;
  refused files                progressive, CMYK, and files edited into each refusal of include/lspjpegdec.h are made by the tests from
                               these bytes; the two that need Pillow (progressive, CMYK) are stored here;
  corrupt files                three files for the device test: a changed byte in the scan (CORRUPT in stage 1), a quantisation table of
                               255s (RANGE in stage 2), a file cut inside its scan (CORRUPT in the planner);
  512^2 (jpeg_dec_512.npz)     four `smooth` colour files at quality 95 (stand-ins for candidate images) and the eight `smooth` quality-75
                               frames of tests/golden/jpeg_pil.json (same recipes, same bytes: their sha256 is checked against that file);
                               the files are stored, of the pixels only the sha256.

Every file is checked against tests/jpeg_decode_model.py before it is written.   python tools/make_golden_jpeg_decode.py"""
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
from PIL import Image, features  # noqa: E402

SIZES = ((7, 1), (1, 7), (47, 33), (1, 17), (17, 1), (3, 9), (9, 3), (4, 9), (9, 4), (2, 5), (5, 2), (40, 72), (16, 16), (8, 24))     # (h, w)
QUALITIES = (1, 30, 75, 95, 100)
KINDS = ("noise", "smooth", "extremes", "primaries", "sparse")
MODES = (("420", 3, {}), ("444", 3, {"subsampling": 0}), ("422", 3, {"subsampling": 1}), ("opt", 3, {"optimize": True}),
         ("rstb", 3, {"restart_marker_blocks": 3}), ("rstr", 3, {"restart_marker_rows": 1}), ("grey", 1, {}), ("greyrst", 1, {"restart_marker_rows": 1}))


def pil_bytes(img, quality, **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=quality, **kw)
    return b.getvalue()


def pil_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)))


def small_cases():
    out, k = [], 0
    for h, w in SIZES:
        for mode, ch, kw in MODES:
            kind = "noise" if ch == 1 else KINDS[k % len(KINDS)]
            q = QUALITIES[(k // len(KINDS) + k) % len(QUALITIES)]
            out.append({"name": "%s_%s_%dx%d_q%d" % (kind, mode, h, w, q), "quality": q, "save": kw,
                        "recipe": {"kind": kind, "h": h, "w": w, "channels": ch, "seed": 700 + k}})
            k += 1
    return out


def main():
    meta = {"pillow": Image.__version__, "libjpeg_turbo": features.version("libjpeg_turbo"),
            "reader": "numpy.asarray(Image.open(f))", "cases": [], "refused": [], "corrupt": [], "frames": []}
    small, big = {}, {}
    for c in small_cases():
        img = M.make_image(c["recipe"])
        data = pil_bytes(img, c["quality"], **c["save"])
        px = pil_pixels(data)
        assert np.array_equal(D.decode(data), px), "the model disagrees with Pillow on %s" % c["name"]
        small[c["name"] + ".jpg"], small[c["name"] + ".px"] = np.frombuffer(data, np.uint8), px
        meta["cases"].append(dict(c, length=len(data)))
    # four 64^2 stand-ins for candidate images: the size of the golden case the device test feeds them to
    for j in range(4):
        c = {"name": "candidate_%d_64x64_q95" % j, "quality": 95, "save": {}, "recipe": {"kind": "smooth", "h": 64, "w": 64, "channels": 3, "seed": 950 + j}}
        data = pil_bytes(M.make_image(c["recipe"]), 95)
        px = pil_pixels(data)
        assert np.array_equal(D.decode(data), px)
        small[c["name"] + ".jpg"], small[c["name"] + ".px"] = np.frombuffer(data, np.uint8), px
        meta["cases"].append(dict(c, length=len(data)))
    # without DHT: same pixels in Pillow, Annex K's tables in the decoder
    find = lambda part: next(c["name"] for c in meta["cases"] if part in c["name"])
    for part in ("_420_47x33_", "_grey_40x72_"):
        src = find(part)
        data = D.strip_dht(small[src + ".jpg"].tobytes())
        assert np.array_equal(pil_pixels(data), small[src + ".px"]) and np.array_equal(D.decode(data), small[src + ".px"])
        small[src + "_nodht.jpg"], small[src + "_nodht.px"] = np.frombuffer(data, np.uint8), small[src + ".px"]
        meta["cases"].append({"name": src + "_nodht", "derived_from": src, "edit": "DHT segments removed", "length": len(data)})
    # the two refusals only Pillow can write
    img = M.make_image({"kind": "smooth", "h": 24, "w": 24, "channels": 3, "seed": 9})
    for name, data in (("progressive", pil_bytes(img, 75, progressive=True)), ("cmyk", pil_bytes_cmyk(img))):
        assert D.status_of(data) == D.UNSUPPORTED
        small["refused_%s.jpg" % name] = np.frombuffer(data, np.uint8)
        meta["refused"].append({"name": "refused_" + name, "status": D.UNSUPPORTED})
    # three corrupt files for the device test (each goes through the stand-alone host check first: tests/test_jpeg_decode_cpu.py)
    src = find("_420_40x72_")
    good = small[src + ".jpg"].tobytes()
    f = D.parse(good)
    for at in range(f["scan_begin"], f["scan_end"]):           # the first byte of the scan whose change passes the planner and fails stage 1
        bad = bytearray(good)
        bad[at] ^= 0x5A
        if 0xFF in (good[at - 1], good[at], bad[at]):
            continue                                           # the marker structure stays as it is
        D.parse(bytes(bad))
        if D.status_of(bytes(bad)) == D.CORRUPT:
            break
    else:
        raise AssertionError("no byte of the scan makes stage 1 fail")
    corrupt = [("corrupt_scan_byte", bytes(bad), "byte %d of %s changed" % (at, src))]
    src2 = "extremes 16x16 at quality 100"
    ext = bytearray(pil_bytes(M.make_image({"kind": "extremes", "h": 16, "w": 16, "channels": 3}), 100))
    i = bytes(ext).index(b"\xff\xdb")
    ext[i + 5:i + 4 + 65] = b"\xff" * 64                       # every luma step 255: DC * 255 leaves int16
    corrupt.append(("corrupt_range", bytes(ext), "luma quantisation table of %s set to 255" % src2))
    corrupt.append(("corrupt_cut", good[:f["scan_begin"] + 40], "%s cut 40 bytes into its scan" % src))
    for name, data, how in corrupt:
        st = D.status_of(data)
        assert st in (D.CORRUPT, D.RANGE), (name, st)
        small[name + ".jpg"] = np.frombuffer(data, np.uint8)
        meta["corrupt"].append({"name": name, "status": st, "edit": how})
    assert meta["corrupt"][1]["status"] == D.RANGE
    # 512^2: candidates at q95 and the encoder fixtures' frames at q75
    pil_meta = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "jpeg_pil.json")))["cases"]}
    frames = [("candidate_%d_512_q95" % j, 95, {"kind": "smooth", "h": 512, "w": 512, "channels": 3, "seed": 900 + j}, None) for j in range(4)]
    frames += [("smooth_c_512_s%d_q75" % k, 75, pil_meta["smooth_c_512_s%d_q75" % k]["recipe"], pil_meta["smooth_c_512_s%d_q75" % k]["sha256"]) for k in range(8)]
    for name, q, recipe, sha in frames:
        data = pil_bytes(M.make_image(recipe), q)
        assert sha is None or hashlib.sha256(data).hexdigest() == sha, "%s is not the file of jpeg_pil.json" % name
        px = pil_pixels(data)
        assert np.array_equal(D.decode(data), px), "the model disagrees with Pillow on %s" % name
        big[name + ".jpg"] = np.frombuffer(data, np.uint8)
        meta["frames"].append({"name": name, "quality": q, "recipe": recipe, "length": len(data), "shape": list(px.shape),
                               "pixels_sha256": hashlib.sha256(np.ascontiguousarray(px).tobytes()).hexdigest()})
        print("%-28s %7d bytes" % (name, len(data)), flush=True)
    g = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(g, "jpeg_dec.npz"), **small)
    np.savez_compressed(os.path.join(g, "jpeg_dec_512.npz"), **big)
    with open(os.path.join(g, "jpeg_dec.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
        fh.write("\n")
    for n in ("jpeg_dec.npz", "jpeg_dec_512.npz", "jpeg_dec.json"):
        print(n, os.path.getsize(os.path.join(g, n)), "bytes")


def pil_bytes_cmyk(img):
    b = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(b, "JPEG", quality=75)
    return b.getvalue()


if __name__ == "__main__":
    main()
