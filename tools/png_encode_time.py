#!/usr/bin/env python3
"""Cost of the device PNG encoder (include/lsppngenc.h, png.PngEncoder), recorded to profiles/png_encode_time.txt.

    python tools/png_encode_time.py [output directory, default profiles/]

runs every GPU step as a process of its own under `timeout`, one after the other, and stops at the first that fails:
  1..4  `rocprofv3 --kernel-trace --stats -- python tools/png_encode_time.py --trace CASE REPS`, in the order colour, gray, colour, gray: device time
        per launch (no counters in these runs), read from the run's database.  Inside a run the PNG and the JPEG (q75) encoder take turns on the same
        8 frames, A-B-A-B;
  5     `--e2e`: host clock, A-B-A-B: PngEncoder.encode and JpegEncoder.encode (launches + the files' bytes to the host), Pillow save(..., "PNG") of
        the same frames on this host with 1 and 16 threads plus the copy of the raw frames to the host that it needs, the files' sizes, and
        render_frames `normal` bf16 batch 8 without and with png=True.

Cases: `colour` 8 frames of 512^2 from the `normal` bf16 generator itself, `gray` 8 edge maps of 512^2 from the rasteriser.  No speed is promised."""
import argparse
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
ORDER = ("colour", "gray", "colour", "gray")
B, S = 8, 512


def frames(case):
    """(the 8 frames on the device, the engine or None)"""
    import torch
    from livespeechportraits_amd import synth
    dev = torch.device("cuda:0")
    if case == "gray":
        from livespeechportraits_amd.feature_map import FeatureMapRasteriser
        rng = np.random.default_rng(5)
        lm = 256 + rng.normal(0, 60, (B, 73, 2))
        sh = np.stack([np.linspace(0, 512, 18), np.full(18, 470.0)], 1)[None].repeat(B, 0)
        return FeatureMapRasteriser(S, 18, dev).rasterise(lm, sh, as_uint8=True).contiguous()
    from livespeechportraits_amd.engine import Engine
    from livespeechportraits_amd.topology import build_topology
    eng = Engine("normal", size=S, max_batch=B, dtype="bf16")
    eng.load_state_dict(synth.make_state_dict(build_topology("normal"), 1234))
    eng.bind(eng.pack(), dev)
    feats, cand = synth.make_inputs(B, S, seed=5, cand_batch=1)
    u8 = torch.empty((B, S, S, 3), dtype=torch.uint8, device=dev)
    eng.forward_image(torch.from_numpy(feats).to(dev), torch.from_numpy(cand).to(dev), out_u8=u8)
    torch.cuda.synchronize()
    eng.close()
    return u8


def encoders(case):
    from livespeechportraits_amd.jpeg import JpegEncoder
    from livespeechportraits_amd.png import PngEncoder
    ch = 3 if case == "colour" else 1
    return PngEncoder(S, ch, "cuda:0", max_batch=B), JpegEncoder(S, ch, 75, "cuda:0", max_batch=B)


def trace(case, reps):
    import torch
    x = frames(case)
    penc, jenc = encoders(case)
    for _ in range(2):                                         # A-B-A-B
        for enc in (penc, jenc):
            for _ in range(reps):
                enc.enqueue(x)
            torch.cuda.synchronize()


def e2e(out_path):
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    import livespeechportraits_amd as L
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.render_loop import render_frames
    from livespeechportraits_amd.topology import build_topology
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "pillow": Image.__version__, "cases": {}}

    def ms(fn, reps=10):
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(t)), 3)

    def pil(img):
        b = io.BytesIO()
        Image.fromarray(img).save(b, "PNG")
        return b.getvalue()

    pool = ThreadPoolExecutor(16)
    for case in ("colour", "gray"):
        x = frames(case)
        penc, jenc = encoders(case)
        host = x.cpu().numpy()
        legs = {"png_device_encode_and_fetch": lambda: penc.encode(x), "jpeg75_device_encode_and_fetch": lambda: jenc.encode(x),
                "raw_frames_to_host": lambda: x.cpu(),
                "pillow_png_1_thread": lambda: [pil(f) for f in host], "pillow_png_16_threads": lambda: list(pool.map(pil, list(host)))}
        for fn in legs.values():
            fn()
        rounds = {k: [] for k in legs}
        for _ in range(2):                                     # A-B-A-B: every leg twice, interleaved
            for k, fn in legs.items():
                rounds[k].append(ms(fn))
        files = penc.encode(x)
        assert all(np.array_equal(np.asarray(Image.open(io.BytesIO(f))), h) for f, h in zip(files, host))
        rec["cases"][case] = {"median_ms_per_batch": rounds, "raw_bytes": int(host[0].nbytes), "png_device_bytes": int(np.mean([len(f) for f in files])),
                              "png_pillow_bytes": int(np.mean([len(pil(f)) for f in host])), "jpeg75_bytes": int(np.mean([len(f) for f in jenc.encode(x)]))}
    opt = argparse.Namespace(model="feature2face", gpu_ids=[0], isTrain=False, size="normal", ngf=64, n_downsample_G=8, fp16=0, checkpoints_dir=tempfile.mkdtemp(),
                             name="t", load_epoch="none", verbose=False)
    model = L.create_model(opt)
    model._g().netG.dtype = "bf16"                             # the bf16 storage plan before the first engine is built
    model._g().load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.make_state_dict(build_topology("normal"), 1234).items()})
    model.eval()
    feats, cand = synth.make_inputs(B, S, seed=5, cand_batch=1)
    cd = torch.from_numpy(cand).to(dev)
    maps = [torch.from_numpy(feats[i % B]).pin_memory() for i in range(128)]
    rec["render_frames_fps"] = {"plain": [], "png": []}
    for arm in ("plain", "png", "plain", "png"):
        kw = {"png": True} if arm == "png" else {}
        render_frames(model, iter(maps[:2 * B]), cd, batch=B, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        render_frames(model, iter(maps), cd, batch=B, **kw)
        rec["render_frames_fps"][arm].append(round(len(maps) / (time.perf_counter() - t0), 1))
    print(json.dumps(rec), flush=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


def launch_times(db):
    cur = sqlite3.connect(db).cursor()
    rows = cur.execute("select name, count(*), sum(end-start) from kernels where name like '%pngenc_%' or name like '%jpeg_%' group by name").fetchall()
    out = {}
    for n, c, t in rows:
        key = re.search(r"(pngenc|jpeg)_\w+", n).group(0)
        cc, tt = out.get(key, (0, 0.0))
        out[key] = (cc + c, tt + t / 1e3)
    return {k: (c, t / c) for k, (c, t) in out.items()}


def main():
    out_dir = next((a for a in sys.argv[1:] if not a.startswith("--")), os.path.join(ROOT, "profiles"))
    work = tempfile.mkdtemp(prefix="png_encode_time_")          # the traces' databases and the e2e record: read here, not kept
    lines = ["# tools/png_encode_time.py: device PNG encoder (4 launches) beside the JPEG encoder (q75, 4 launches), 8 frames of 512^2 per call; launch times from "
             "rocprofv3 --kernel-trace (average per launch, us)"]
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
        for kind in ("pngenc", "jpeg"):
            mine = {k: v for k, v in sorted(st.items()) if k.startswith(kind + "_")}
            lines.append("%-6s %-6s %s   sum %.1f us" % (case, kind, "  ".join("%s %.1f us" % (k, v[1]) for k, v in mine.items()), sum(v[1] for v in mine.values())))
            print(lines[-1], file=sys.stderr, flush=True)
    else:
        path = os.path.join(work, "e2e.json")
        r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--e2e", path], capture_output=True, text=True)
        if r.returncode != 0:
            lines.append("e2e: ended with status %d\n%s" % (r.returncode, r.stderr[-800:]))
        else:
            rec = json.load(open(path))
            lines.append("# host clock, median ms per batch of 8, two rounds each (A-B-A-B); %s; Pillow %s on this host" % (rec["device"], rec["pillow"]))
            for case, c in rec["cases"].items():
                lines.append("%s: bytes per frame: raw %d, PNG device %d, PNG Pillow %d (x%.2f), JPEG q75 %d" % (
                    case, c["raw_bytes"], c["png_device_bytes"], c["png_pillow_bytes"], c["png_device_bytes"] / c["png_pillow_bytes"], c["jpeg75_bytes"]))
                for k, t in c["median_ms_per_batch"].items():
                    lines.append("  %-34s %s" % (k, " / ".join("%.2f" % x for x in t)))
            lines.append("render_frames normal bf16 batch 8, frames/s: plain %s, png=True %s" % (rec["render_frames_fps"]["plain"], rec["render_frames_fps"]["png"]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "png_encode_time.txt"), "w") as f:
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
