#!/usr/bin/env python3
"""Writes tests/golden/resize.json and tests/golden/resize.npz from LIVE Pillow: the fixtures of tests/test_resize_cpu.py and
tests/test_gpu_resize.py.  Needs Pillow (the fixtures were written with the version recorded in the JSON); no device.

Every case of tests/resize_model.py cases() -- an input recipe for jpeg_model.make_image (kind, h, w, channels, seed; image i of the batch of
three has seed + i), the output size and the filter -- is resized with ``Image.fromarray(img).resize((out_w, out_h), filter)``.  A batch
whose three outputs take at most 64 * 64 * 3 bytes is stored whole (npz, key = the case's name, uint8 [3, out_h, out_w(, 3)]); a larger one
as the SHA-256 of those bytes.  The npz also holds four small JPEG files of different geometries (``candidate_0`` .. ``candidate_3``, Pillow's
encoder at quality 90): the photographs of the ``load_candidates(resize=)`` test, which no encoder of the project could write (33 x 70).

    python tools/make_golden_resize.py            # rewrite the fixtures
    python tools/make_golden_resize.py --check    # compare live Pillow with the stored fixtures, write nothing
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
WHOLE_BYTES = 64 * 64 * 3


def pillow_batch(case, batch):
    from PIL import Image
    flt = getattr(Image.Resampling, case["filter"].upper())
    return np.stack([np.asarray(Image.fromarray(img).resize((case["out_w"], case["out_h"]), flt)) for img in batch])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import PIL
    import resize_model as M
    golden = os.path.join(ROOT, "tests", "golden")
    meta = {"pillow": PIL.__version__, "batch": M.BATCH, "cases": []}
    arrays = {}
    for case in M.cases():
        out = pillow_batch(case, M.batch_of(case))
        entry = dict(case)
        if out.nbytes <= WHOLE_BYTES:
            arrays[case["name"]] = out
        entry["sha256"] = M.sha256(out)
        meta["cases"].append(entry)
    from PIL import Image
    import io
    for j, (w, h) in enumerate(M.CANDIDATE_SIZES):
        b = io.BytesIO()
        Image.fromarray(M.make_image({"kind": "smooth", "h": h, "w": w, "channels": 3, "seed": 300 + j})).save(b, "JPEG", quality=90)
        arrays["candidate_%d" % j] = np.frombuffer(b.getvalue(), np.uint8)
    if args.check:
        old = json.load(open(os.path.join(golden, "resize.json")))
        bad = [a["name"] for a, b in zip(meta["cases"], old["cases"]) if a != b]
        print("Pillow %s against fixtures of Pillow %s: %d cases, %d differ %s" % (PIL.__version__, old["pillow"], len(meta["cases"]), len(bad), bad[:5]))
        return 1 if bad or len(meta["cases"]) != len(old["cases"]) else 0
    with open(os.path.join(golden, "resize.json"), "w") as f:
        json.dump(meta, f, indent=0, sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(golden, "resize.npz"), **arrays)
    print("%d cases, %d stored whole, %d candidate files" % (len(meta["cases"]), len(arrays) - len(M.CANDIDATE_SIZES), len(M.CANDIDATE_SIZES)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
