#!/usr/bin/env python3
"""Cost of the device PNG decoder (include/lsppng.h, png.PngDecoder), recorded to profiles/png_decode_time.txt.

    python tools/png_decode_time.py [output directory, default profiles/]

runs every GPU step as a process of its own under `timeout`, one after the other, and stops at the first that fails:
  1..4  `rocprofv3 --kernel-trace --stats -- python tools/png_decode_time.py --trace CASE REPS`, in the order png4, jpeg4, png4, jpeg4: device time
        per launch (no counters in these runs), read from the run's database;
  5     `--e2e`: call to pixels on the device (plan on the host, one upload, three launches, status words back), A-B-A-B against Pillow on this
        host with 1 and 16 threads plus the upload of its pixels, and against jpeg.JpegDecoder on quality-95 JPEG files of the same images (made
        here with Pillow) in the same session.  Without Pillow here that is recorded and those legs are left out.

Cases: `png4` the four 512^2 candidate files of tests/golden/png_dec_512.npz in one call (RGB, RGBA, palette, one saved by Pillow with
optimize=True); `jpeg4` the same four images as quality-95 JPEG files through JpegDecoder.  No speed is promised: one wave walks a file's symbols."""
import glob
import io
import json
import os
import re
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
ORDER = ("png4", "jpeg4", "png4", "jpeg4")


def png_files():
    meta = json.load(open(os.path.join(GOLDEN, "png_dec.json")))
    z = np.load(os.path.join(GOLDEN, "png_dec_512.npz"))
    return [z[c["name"] + ".png"].tobytes() for c in meta["candidates"]]


def jpeg_files():
    """quality-95 JPEG files of the same four images; None without Pillow"""
    try:
        from PIL import Image
    except ImportError:
        return None
    out = []
    for data in png_files():
        b = io.BytesIO()
        Image.open(io.BytesIO(data)).convert("RGB").save(b, "JPEG", quality=95)
        out.append(b.getvalue())
    return out


def trace(case, reps):
    import torch
    from livespeechportraits_amd.jpeg import JpegDecoder
    from livespeechportraits_amd.png import PngDecoder
    files = png_files() if case == "png4" else jpeg_files()
    if files is None:
        raise SystemExit("jpeg4 needs Pillow to make the JPEG files")
    dec = (PngDecoder if case == "png4" else JpegDecoder)("cuda:0", max_side=512, max_batch=4)
    for _ in range(reps + 2):
        dec.decode(files)
    torch.cuda.synchronize()


def e2e(out_path):
    import torch
    from livespeechportraits_amd.jpeg import JpegDecoder
    from livespeechportraits_amd.png import PngDecoder
    try:
        from PIL import Image
    except ImportError:
        Image = None
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "pillow": None if Image is None else Image.__version__}
    pngs, jpegs = png_files(), jpeg_files()

    def pil_one(data):
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))

    def pil_batch(pool):
        px = list(pool.map(pil_one, pngs)) if pool else [pil_one(f) for f in pngs]
        out = [torch.from_numpy(p).to(dev, non_blocking=True) for p in px]
        torch.cuda.synchronize()
        return out

    def ms(fn, reps):
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t))

    from concurrent.futures import ThreadPoolExecutor
    pdec = PngDecoder(dev, max_side=512, max_batch=4)
    legs = {"png_device": lambda: pdec.decode(pngs)}
    if Image is not None:
        pool = ThreadPoolExecutor(16)
        jdec = JpegDecoder(dev, max_side=512, max_batch=4)
        legs["pillow_1_thread_plus_upload"] = lambda: pil_batch(None)
        legs["pillow_16_threads_plus_upload"] = lambda: pil_batch(pool)
        legs["jpeg_q95_device"] = lambda: jdec.decode(jpegs)
    for fn in legs.values():
        fn()                                                   # warm: buffers, page faults, thread start
    rounds = {k: [] for k in legs}
    for _ in range(2):                                         # A-B-A-B: every leg twice, interleaved
        for k, fn in legs.items():
            rounds[k].append(ms(fn, 20))
    rec["files"] = len(pngs)
    rec["png_bytes"] = sum(map(len, pngs))
    rec["jpeg_bytes"] = None if jpegs is None else sum(map(len, jpegs))
    rec["median_ms_per_call"] = rounds
    print(json.dumps(rec), flush=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


def launch_times(db):
    cur = sqlite3.connect(db).cursor()
    rows = cur.execute("select name, count(*), sum(end-start) from kernels where name like '%pngdec_%' or name like '%jpegdec_%' group by name").fetchall()
    return {re.search(r"(png|jpeg)dec_\w+", n).group(0): (c, t / 1e3 / c) for n, c, t in rows}


def main():
    out_dir = next((a for a in sys.argv[1:] if not a.startswith("--")), os.path.join(ROOT, "profiles"))
    work = tempfile.mkdtemp(prefix="png_decode_time_")          # the traces' databases and the e2e record: read here, not kept
    lines = ["# tools/png_decode_time.py: device PNG decoder, four 512^2 candidate files in one call; launch times from rocprofv3 --kernel-trace (average per launch, us)"]
    reps = 20
    for run, case in enumerate(ORDER):
        tag = "%s_%d" % (case, run)
        cmd = ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "-d", work, "-o", tag, "--", sys.executable, os.path.abspath(__file__),
               "--trace", case, str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            lines.append("%s: the trace run ended with status %d; nothing after it was run\n%s" % (case, r.returncode, r.stderr[-800:]))
            break
        db = sorted(glob.glob(os.path.join(work, "**", tag + "_results.db"), recursive=True))
        st = launch_times(db[-1]) if db else {}
        lines.append("%-6s %s   sum %.1f us" % (case, "  ".join("%s %.1f us" % (k, v[1]) for k, v in sorted(st.items())), sum(v[1] for v in st.values())))
        print(lines[-1], file=sys.stderr, flush=True)
    else:
        path = os.path.join(work, "e2e.json")
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--e2e", path], capture_output=True, text=True)
        if r.returncode != 0:
            lines.append("e2e: ended with status %d\n%s" % (r.returncode, r.stderr[-800:]))
        else:
            rec = json.load(open(path))
            lines.append("# call to pixels, median ms per call, two rounds each (A-B-A-B); %s; Pillow on this host: %s" % (rec["device"], rec["pillow"] or "not installed"))
            lines.append("%d files, %d bytes as PNG, %s bytes as quality-95 JPEG" % (rec["files"], rec["png_bytes"], rec["jpeg_bytes"]))
            for k, t in rec["median_ms_per_call"].items():
                lines.append("%-32s %s" % (k, " / ".join("%.2f" % x for x in t)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "png_decode_time.txt"), "w") as f:
        f.write(text)
    return 0 if "ended with status" not in text else 1


if __name__ == "__main__":
    if "--trace" in sys.argv:
        i = sys.argv.index("--trace")
        trace(sys.argv[i + 1], int(sys.argv[i + 2]))
    elif "--e2e" in sys.argv:
        e2e(sys.argv[sys.argv.index("--e2e") + 1])
    else:
        sys.exit(main())
