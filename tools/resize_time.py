#!/usr/bin/env python3
"""Cost of the device resampler (include/lspresize.h, resize.Resizer), recorded to profiles/resize_time.txt.

    python tools/resize_time.py [output directory, default profiles/]

runs every GPU step as a process of its own under `timeout`, one after the other, and stops at the first that fails:
  1  `rocprofv3 --kernel-trace --stats -- python tools/resize_time.py --trace REPS`: device time per kernel (no counters in this run), read from
     the run's database, for
       8 frames of 512^2 -> 256^2 and -> 384^2, BICUBIC and LANCZOS (the `normal` generator's own uint8 frames);
       four 1080p candidates -> 512^2 (one call per candidate, float planes through the normalisation table), BICUBIC and LANCZOS;
       the colour JPEG encode of the same 8 frames at q75 -- the YARDSTICK: the stage that stands next to the resize on a lane;
  2  `--loop`: render_frames on the `normal` bf16 batch-8 plan with jpeg_quality=75, without and with out_size=256, A-B-A-B, frames/s with the spread;
  3  `--host`: Pillow on this host for the same frames, 1 and 16 threads, plus the upload of its pixels (recorded as absent without Pillow).
"""
import glob
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
B, S = 8, 512
FRAME_CASES = [(256, "bicubic"), (256, "lanczos"), (384, "bicubic"), (384, "lanczos")]
CAND_FILTERS = ("bicubic", "lanczos")


def frames_of(dev):
    """8 uint8 frames of 512^2: the `normal` bf16 generator's own output on synthetic inputs"""
    import torch
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.engine import Engine
    from livespeechportraits_amd.topology import build_topology
    eng = Engine("normal", size=S, max_batch=B, dtype="bf16")
    eng.load_state_dict(synth.make_state_dict(build_topology("normal"), 1234))
    eng.bind(eng.pack(), dev)
    feats, cand = synth.make_inputs(B, S, seed=5, cand_batch=1)
    u8 = torch.empty((B, S, S, 3), dtype=torch.uint8, device=dev)
    eng.forward_image(torch.from_numpy(feats).to(dev), torch.from_numpy(cand).to(dev), out_u8=u8)
    torch.cuda.synchronize()
    return u8


def photographs():
    """four 1080 x 1920 uint8 RGB pictures (smooth with a little noise)"""
    rng = np.random.default_rng(11)
    y, x = np.meshgrid(np.arange(1080), np.arange(1920), indexing="ij")
    out = []
    for j in range(4):
        base = np.stack([128 + 90 * np.sin(x / (37.0 + j) + j) * np.cos(y / 53.0), 128 + 90 * np.cos((x + y) / 41.0 + j), 128 - 90 * np.sin(x / 61.0) * np.cos(y / (29.0 + j))], -1)
        out.append(np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8))
    return out


def trace(reps):
    """every case `reps` times, one case after the other: the summary tells the cases apart by the order of their launches (ORDER, on stdout)"""
    import torch
    from livespeechportraits_amd.candidates import normalisation_table
    from livespeechportraits_amd.jpeg import JpegEncoder
    from livespeechportraits_amd.resize import Resizer
    dev = torch.device("cuda:0")
    u8 = frames_of(dev)
    rs = Resizer(dev, max_batch=B)
    order = []
    for size, filt in FRAME_CASES:
        out = torch.empty((B, size, size, 3), dtype=torch.uint8, device=dev)
        for _ in range(reps):
            rs.resize(u8, size, filt, out=out)
        order.append(("frames8_512_to_%d_%s" % (size, filt), reps, rs.plan(S, size, filt).launches))
    table = torch.from_numpy(normalisation_table()).to(dev)
    photos = [torch.from_numpy(p).to(dev) for p in photographs()]
    planes = torch.empty((12, S, S), dtype=torch.float32, device=dev)
    for filt in CAND_FILTERS:
        for _ in range(reps):
            for j, p in enumerate(photos):
                rs.resize_planes(p, S, table, planes[3 * j:3 * j + 3], filt)
        order.append(("candidates4_1080p_to_512_%s" % filt, reps, 4 * rs.plan((1920, 1080), S, filt).launches))
    enc = JpegEncoder(S, 3, 75, dev, max_batch=B)
    for _ in range(reps):
        enc.enqueue(u8)
    torch.cuda.synchronize()
    print("ORDER " + json.dumps(order), flush=True)


def kernel_rows(db):
    cur = sqlite3.connect(db).cursor()
    return cur.execute("select name, start, end from kernels order by start").fetchall()


def summarise(rows, order):
    """per case: microseconds per call, split by kernel; the resize kernels appear in launch order, the encoder's after them"""
    rs = [(n, e - s) for n, s, e in rows if "resize_" in n]
    jp = [(n, e - s) for n, s, e in rows if re.search(r"jpeg(?!dec)", n) and "resize_" not in n]
    out, at = [], 0
    for name, reps, per_call in order:
        part = rs[at:at + reps * per_call]
        at += reps * per_call
        hor = sum(t for n, t in part if "horizontal" in n) / 1e3 / reps
        ver = sum(t for n, t in part if "vertical" in n) / 1e3 / reps
        out.append("%-38s %7.1f us per call (horizontal %.1f, vertical %.1f; %d launches)" % (name, hor + ver, hor, ver, per_call))
    reps = order[0][1]
    if jp:
        out.append("%-38s %7.1f us per call (the yardstick: lspjpeg_encode of the same 8 frames, %d kernels per call)" % (
            "jpeg_colour_q75_frames8_512", sum(t for _, t in jp) / 1e3 / reps, len(jp) // reps))
    if at != len(rs):
        out.append("(%d resize launches in the trace, %d accounted for)" % (len(rs), at))
    return out


def loop(out_path):
    import argparse
    import torch
    import livespeechportraits_amd as L
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.render_loop import render_frames
    from livespeechportraits_amd.topology import build_topology
    dev = torch.device("cuda:0")
    sd = synth.make_state_dict(build_topology("normal"), 1234)
    feats, cand = synth.make_inputs(B, S, seed=5, cand_batch=1)
    cd = torch.from_numpy(cand).to(dev)
    opt = argparse.Namespace(model="feature2face", gpu_ids=[0], isTrain=False, size="normal", ngf=64, n_downsample_G=8, fp16=0, checkpoints_dir=tempfile.mkdtemp(),
                             name="t", load_epoch="none", verbose=False)
    model = L.create_model(opt)
    model._g().netG.dtype = "bf16"                             # the bf16 storage plan before the first engine is built
    model._g().load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    model.eval()
    nframes = 256
    maps = [torch.from_numpy(feats[i % B]).pin_memory() for i in range(nframes)]
    rec = {"device": torch.cuda.get_device_name(0), "jpeg75_fps": [], "jpeg75_out256_fps": []}
    for arm in ("jpeg75", "jpeg75_out256") * 3:
        kw = {"jpeg_quality": 75, **({"out_size": 256} if arm.endswith("256") else {})}
        render_frames(model, iter(maps[:4 * B]), cd, batch=B, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        render_frames(model, iter(maps), cd, batch=B, **kw)
        rec[arm + "_fps"].append(round(nframes / (time.perf_counter() - t0), 1))
    with open(out_path, "w") as f:
        json.dump(rec, f)


def host(out_path):
    import torch
    try:
        from PIL import Image
    except ImportError:
        json.dump({"pillow": None}, open(out_path, "w"))
        return
    from concurrent.futures import ThreadPoolExecutor
    dev = torch.device("cuda:0")
    frames = frames_of(dev).cpu().numpy()
    photos = photographs()
    pool = ThreadPoolExecutor(16)

    def run(images, size, filt, workers):
        one = lambda im: np.asarray(Image.fromarray(im).resize((size, size), getattr(Image.Resampling, filt.upper())))
        px = list(pool.map(one, images)) if workers else [one(im) for im in images]
        torch.from_numpy(np.stack(px)).to(dev)
        torch.cuda.synchronize()

    def ms(fn, reps=10):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(t)), 3)

    rec = {"pillow": Image.__version__, "cases": {}}
    jobs = [("frames8_512_to_%d_%s" % (s, f), frames, s, f) for s, f in FRAME_CASES] + [("candidates4_1080p_to_512_%s" % f, photos, S, f) for f in CAND_FILTERS]
    for name, images, size, filt in jobs:
        rounds = {"1_thread_plus_upload_ms": [], "16_threads_plus_upload_ms": []}
        for _ in range(2):                                         # A-B-A-B
            rounds["1_thread_plus_upload_ms"].append(ms(lambda: run(images, size, filt, False)))
            rounds["16_threads_plus_upload_ms"].append(ms(lambda: run(images, size, filt, True)))
        rec["cases"][name] = rounds
    json.dump(rec, open(out_path, "w"))


def main():
    out_dir = next((a for a in sys.argv[1:] if not a.startswith("--")), os.path.join(ROOT, "profiles"))
    work = tempfile.mkdtemp(prefix="resize_time_")
    me, reps = os.path.abspath(__file__), 20
    lines = ["# tools/resize_time.py: device resampler (two launches: horizontal into the workspace, vertical out of it); device time from rocprofv3 --kernel-trace,",
             "# average per call over %d calls; 8 frames = the `normal` bf16 generator's uint8 output" % reps]
    r = subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", work, "-o", "resize", "--", sys.executable, me, "--trace", str(reps)],
                       capture_output=True, text=True)
    order = re.search(r"^ORDER (.*)$", r.stdout, re.M)
    db = sorted(glob.glob(os.path.join(work, "**", "resize_results.db"), recursive=True))
    if r.returncode != 0 or not order or not db:
        lines.append("trace: the run ended with status %d; nothing after it was run\n%s" % (r.returncode, r.stderr[-800:]))
    else:
        lines += summarise(kernel_rows(db[-1]), json.loads(order.group(1)))
        steps = (("--loop", "loop.json", 420), ("--host", "host.json", 300))
        for flag, name, limit in steps:
            path = os.path.join(work, name)
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, me, flag, path], capture_output=True, text=True)
            if r.returncode != 0:
                lines.append("%s: ended with status %d; nothing after it was run\n%s" % (flag, r.returncode, r.stderr[-800:]))
                break
            rec = json.load(open(path))
            if flag == "--loop":
                lines.append("# render_frames, `normal` bf16, batch 8, 256 frames, jpeg_quality=75, frames/s, A-B-A-B-A-B on %s" % rec["device"])
                for k in ("jpeg75_fps", "jpeg75_out256_fps"):
                    lines.append("%-38s %s   (min %.1f, max %.1f)" % (k, " / ".join("%.1f" % v for v in rec[k]), min(rec[k]), max(rec[k])))
            elif rec["pillow"] is None:
                lines.append("# Pillow is not installed on this host: no host figure")
            else:
                lines.append("# Pillow %s on this host, Image.resize of the same pictures + upload of the result, median ms per call, two rounds each" % rec["pillow"])
                for name, v in rec["cases"].items():
                    lines.append("%-38s %s" % (name, "; ".join("%s %s" % (k, " / ".join("%.2f" % x for x in t)) for k, t in v.items())))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "resize_time.txt"), "w") as f:
        f.write(text)
    return 0 if "ended with status" not in text else 1


if __name__ == "__main__":
    if "--trace" in sys.argv:
        trace(int(sys.argv[sys.argv.index("--trace") + 1]))
    elif "--loop" in sys.argv:
        loop(sys.argv[sys.argv.index("--loop") + 1])
    elif "--host" in sys.argv:
        host(sys.argv[sys.argv.index("--host") + 1])
    else:
        sys.exit(main())
