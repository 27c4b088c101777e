#!/usr/bin/env python3
"""Cost of the device JPEG encoder (include/lspjpeg.h) in one session on the GPU, recorded to profiles/<name>.json (+ .txt):
  (a) device time of lspjpeg_encode for 8 frames of 512^2 at q75: the `normal` bf16 generator's own uint8 frames (colour) and the rasteriser's
      uint8 edge maps (grayscale), with the bf16 batch-8 forward timed the same way for the 10 % bar;
  (b) Pillow (Image.fromarray(img).save(f, "JPEG", quality=75)) on the same frames with 1 and 16 threads, on this host, if Pillow is installed;
  (c) render_frames frames/s, `normal` bf16, batch 8, without and with jpeg_quality=75, run A-B-A-B.
    python tools/jpeg_time.py [name] [output directory, default profiles/]
With --options instead (default name jpeg_options_time), the encoder's options as arms {default, restart_rows=1, optimize, both}, A-B-A-B:
  (d) device time of lspjpeg_encode for the same 8 + 8 frames per arm (the default arm runs the kernels of a handle without options), and
      the bytes per frame of each arm on the generator's own frames;
  (e) JpegDecoder.decode of 64 such files per arm (host clock, plan + upload + three stages + status): the decoder gives a wave to every
      restart interval.
    python tools/jpeg_time.py --options [name] [output directory]
With --geometry instead (default name jpeg_geometry_time), the format handles (lspjpeg_create_format) against the plain handle, A-B-A-B:
  (f) device time of lspjpeg_encode for 8 colour frames at q75: the plain 512^2 4:2:0 handle (the baseline: its kernels are untouched), 512^2
      in 4:4:4 and 4:2:2, and 500 x 500 in 4:2:0 (the generator's frames cropped), and the bytes per frame of each subsampling on the
      generator's own 512^2 frames.
    python tools/jpeg_time.py --geometry [name] [output directory]"""
import argparse
import ctypes
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import livespeechportraits_amd as L  # noqa: E402
from livespeechportraits_amd import _native as N, synth  # noqa: E402
from livespeechportraits_amd.engine import Engine  # noqa: E402
from livespeechportraits_amd.feature_map import FeatureMapRasteriser  # noqa: E402
from livespeechportraits_amd.jpeg import JpegEncoder  # noqa: E402
from livespeechportraits_amd.render_loop import render_frames  # noqa: E402
from livespeechportraits_amd.topology import build_topology  # noqa: E402

OPTIONS, GEOMETRY = "--options" in sys.argv, "--geometry" in sys.argv
argv = [a for a in sys.argv[1:] if a not in ("--options", "--geometry")]
name = argv[0] if len(argv) > 0 else ("jpeg_options_time" if OPTIONS else "jpeg_geometry_time" if GEOMETRY else "jpeg_time")
out_dir = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles")
dev = torch.device("cuda:0")
B, S, Q = 8, 512, 75
rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "batch": B, "size": S, "quality": Q}
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def device_us(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


# ---- the frames: the normal bf16 generator's own output and the rasteriser's edge maps ------------------------------------------
topo = build_topology("normal")
sd = synth.make_state_dict(topo, 1234)
eng = Engine("normal", size=S, max_batch=B, dtype="bf16")
eng.load_state_dict(sd)
eng.bind(eng.pack(), dev)
feats, cand = synth.make_inputs(B, S, seed=5, cand_batch=1)
fd, cd = torch.from_numpy(feats).to(dev), torch.from_numpy(cand).to(dev)
u8 = torch.empty((B, S, S, 3), dtype=torch.uint8, device=dev)
eng.forward_image(fd, cd, out_u8=u8)
rng = np.random.default_rng(5)
lm = 256 + rng.normal(0, 60, (B, 73, 2))
sh = np.stack([np.linspace(0, 512, 18), np.full(18, 470.0)], 1)[None].repeat(B, 0)
edges = FeatureMapRasteriser(S, 18, dev).rasterise(lm, sh, as_uint8=True)
torch.cuda.synchronize()

encs = {"colour": (JpegEncoder(S, 3, Q, dev, max_batch=B), u8), "gray": (JpegEncoder(S, 1, Q, dev, max_batch=B), edges)}
st = torch.cuda.current_stream(dev)


def launch(enc, x):
    N.check_jpeg(enc.lib.lspjpeg_encode(enc._h, ctypes.c_void_p(x.data_ptr()), B, ctypes.c_void_p(enc._dst.data_ptr()), ctypes.c_void_p(enc._sizes.data_ptr()),
                                        ctypes.c_void_p(enc._ws.data_ptr()), enc._ws_bytes, ctypes.c_void_p(st.cuda_stream)))


def finish():
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, name + ".json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    with open(os.path.join(out_dir, name + ".txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if OPTIONS:
    from livespeechportraits_amd.jpeg import JpegDecoder, probe
    arms = {"default": {}, "restart_rows=1": dict(restart_rows=1), "optimize": dict(optimize=True), "both": dict(optimize=True, restart_rows=1)}
    made = {a: {"colour": (JpegEncoder(S, 3, Q, dev, max_batch=B, **kw), u8), "gray": (JpegEncoder(S, 1, Q, dev, max_batch=B, **kw), edges)} for a, kw in arms.items()}
    rec["d"] = {a: {"colour_us": [], "gray_us": []} for a in arms}
    for rnd in range(2):                                   # A-B-A-B over the arms
        for a in arms:
            for k, (enc, x) in made[a].items():
                rec["d"][a][k + "_us"].append(round(device_us(lambda: launch(enc, x)), 2))
    files = {a: {k: enc.encode(x) for k, (enc, x) in made[a].items()} for a in arms}
    for a in arms:
        rec["d"][a]["bytes_per_frame"] = {k: int(np.mean([len(f) for f in v])) for k, v in files[a].items()}
        rec["d"][a]["segments"] = probe(files[a]["colour"][0]).segments
        say("(d) lspjpeg_encode, %d frames %d^2 q%d, %-14s: colour %s us, gray %s us; mean file: colour %d B, gray %d B; %d restart intervals per colour file" % (
            B, S, Q, a, rec["d"][a]["colour_us"], rec["d"][a]["gray_us"], rec["d"][a]["bytes_per_frame"]["colour"], rec["d"][a]["bytes_per_frame"]["gray"],
            rec["d"][a]["segments"]))
    base = rec["d"]["default"]["bytes_per_frame"]
    say("(d) bytes against the default arm: " + ", ".join("%s colour %+.1f %% gray %+.1f %%" % (
        a, 100.0 * (rec["d"][a]["bytes_per_frame"]["colour"] / base["colour"] - 1), 100.0 * (rec["d"][a]["bytes_per_frame"]["gray"] / base["gray"] - 1))
        for a in arms if a != "default"))
    dec = JpegDecoder(dev, max_side=S, max_batch=64)
    want = dec.decode(files["default"]["colour"] * 8)
    rec["e"] = {a: [] for a in arms}
    for rnd in range(2):
        for a in arms:
            batch = files[a]["colour"] * 8                 # 64 recorded frames
            got = dec.decode(batch)
            assert all(torch.equal(g, w) for g, w in zip(got, want)), a
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                dec.decode(batch)
            torch.cuda.synchronize()
            rec["e"][a].append(round((time.perf_counter() - t0) / 10 * 1e3, 3))
    for a in arms:
        say("(e) JpegDecoder.decode of 64 colour files %d^2, %-14s: %s ms per call (host clock; the pixels equal the default arm's)" % (S, a, rec["e"][a]))
    eng.close()
    finish()
    sys.exit(0)


if GEOMETRY:
    from livespeechportraits_amd.jpeg import JpegOptions
    crop = u8[:, :500, :500].contiguous()
    arms = {"plain 512^2 4:2:0": (JpegEncoder(S, 3, Q, dev, max_batch=B), u8),
            "512^2 4:2:0 via subsampling=": (JpegEncoder(S, 3, JpegOptions(Q, subsampling="4:2:0"), dev, max_batch=B), u8),
            "512^2 4:2:2": (JpegEncoder(S, 3, JpegOptions(Q, subsampling="4:2:2"), dev, max_batch=B), u8),
            "512^2 4:4:4": (JpegEncoder(S, 3, JpegOptions(Q, subsampling="4:4:4"), dev, max_batch=B), u8),
            "500x500 4:2:0": (JpegEncoder(500, 3, JpegOptions(Q, subsampling="4:2:0"), dev, max_batch=B), crop)}
    rec["f"] = {a: {"us": []} for a in arms}
    for rnd in range(2):                                   # A-B-A-B over the arms
        for a, (enc, x) in arms.items():
            rec["f"][a]["us"].append(round(device_us(lambda: launch(enc, x)), 2))
    for a, (enc, x) in arms.items():
        rec["f"][a]["bytes_per_frame"] = int(np.mean([len(f) for f in enc.encode(x)]))
        say("(f) lspjpeg_encode, %d colour frames q%d, %-28s: %s us; mean file %d B" % (B, Q, a, rec["f"][a]["us"], rec["f"][a]["bytes_per_frame"]))
    base = rec["f"]["plain 512^2 4:2:0"]
    say("(f) against the plain handle: " + ", ".join("%s x%.2f time, %+.1f %% bytes" % (a, min(v["us"]) / min(base["us"]), 100.0 * (v["bytes_per_frame"] / base["bytes_per_frame"] - 1))
                                                      for a, v in rec["f"].items() if a != "plain 512^2 4:2:0"))
    eng.close()
    finish()
    sys.exit(0)


rec["a"] = {}
fwd = []
for rep in range(2):                                       # A-B: forward, colour, gray, both
    fwd.append(device_us(lambda: eng.forward_image(fd, cd, out_u8=u8)))
    for k, (enc, x) in encs.items():
        rec["a"].setdefault(k + "_us", []).append(round(device_us(lambda: launch(enc, x)), 2))
    rec["a"].setdefault("colour_plus_gray_us", []).append(round(device_us(lambda: (launch(*encs["colour"]), launch(*encs["gray"]))), 2))
rec["a"]["bf16_forward_b8_us"] = [round(v, 1) for v in fwd]
files = {k: enc.encode(x) for k, (enc, x) in encs.items()}
rec["a"]["bytes_per_frame"] = {k: int(np.mean([len(f) for f in v])) for k, v in files.items()}
both, f = min(rec["a"]["colour_plus_gray_us"]), min(fwd)
rec["a"]["encode_over_forward"] = round(both / f, 4)
say("(a) device, %d frames %d^2 q%d: colour %s us, gray %s us, colour+gray %s us; bf16 forward_image batch %d: %s us -> encode / forward = %.1f %% (bar 10 %%); "
    "mean file: colour %d B, gray %d B" % (B, S, Q, rec["a"]["colour_us"], rec["a"]["gray_us"], rec["a"]["colour_plus_gray_us"], B, rec["a"]["bf16_forward_b8_us"],
                                           100 * both / f, rec["a"]["bytes_per_frame"]["colour"], rec["a"]["bytes_per_frame"]["gray"]))
# with the copy of the compressed bytes to pinned host memory (what render_frames pays per batch)
rec["a"]["encode_and_fetch_ms"] = {}
for k, (enc, x) in encs.items():
    enc.encode(x)
    t0 = time.perf_counter()
    for _ in range(20):
        enc.encode(x)
    rec["a"]["encode_and_fetch_ms"][k] = round((time.perf_counter() - t0) / 20 * 1e3, 3)
say("(a') encode + sizes + bytes to pinned host memory, host clock: %s ms per batch of %d" % (rec["a"]["encode_and_fetch_ms"], B))

# ---- (b) Pillow on this host -------------------------------------------------------------------------------------------------
host = {"colour": u8.cpu().numpy(), "gray": edges.cpu().numpy()}
try:
    from PIL import Image, features
    from concurrent.futures import ThreadPoolExecutor

    def pil(img):
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", quality=Q)
        return b.getvalue()
    rec["b"] = {"where": "the host CPU of the machine that holds the GPU", "pillow": Image.__version__,
                "libjpeg_turbo": features.version("libjpeg_turbo")}
    for k, frames in host.items():
        same = [pil(frames[i]) for i in range(B)] == files[k]
        t0 = time.perf_counter()
        for _ in range(5):
            for i in range(B):
                pil(frames[i])
        one = (time.perf_counter() - t0) / 5
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(pil, list(frames)))
            t0 = time.perf_counter()
            for _ in range(5):
                list(ex.map(pil, list(frames)))
            sixteen = (time.perf_counter() - t0) / 5
        rec["b"][k] = {"1_thread_ms_per_batch": round(one * 1e3, 3), "16_threads_ms_per_batch": round(sixteen * 1e3, 3), "device_bytes_equal_pillow": same}
    say("(b) Pillow %s (libjpeg-turbo %s) on the GPU host, %d frames: %s" % (rec["b"]["pillow"], rec["b"]["libjpeg_turbo"], B,
                                                                          {k: rec["b"][k] for k in host}))
except ImportError:
    rec["b"] = {"where": "not installed on the GPU host: see the build-machine figures in README"}
    say("(b) Pillow is not installed on this host")

# ---- (c) render_frames frames/s, normal bf16, batch 8, A-B-A-B ------------------------------------------------------------------
opt = argparse.Namespace(model="feature2face", gpu_ids=[0], isTrain=False, size="normal", ngf=64, n_downsample_G=8, fp16=0, checkpoints_dir=tempfile.mkdtemp(), name="t",
                         load_epoch="none", verbose=False)
model = L.create_model(opt)
model._g().netG.dtype = "bf16"                             # the bf16 storage plan (bench.py's configs[2]) before the first engine is built
model._g().load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
model.eval()
nframes = 256
maps = [torch.from_numpy(feats[i % B]).pin_memory() for i in range(nframes)]
rec["c"] = {"plain_fps": [], "jpeg75_fps": []}
for arm in ("plain", "jpeg75", "plain", "jpeg75", "plain", "jpeg75"):
    kw = {"jpeg_quality": 75} if arm == "jpeg75" else {}
    render_frames(model, iter(maps[:4 * B]), cd, batch=B, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = render_frames(model, iter(maps), cd, batch=B, **kw)
    dt = time.perf_counter() - t0
    rec["c"][arm + "_fps"].append(round(nframes / dt, 1))
    say("(c) render_frames normal bf16 batch %d, %s: %.1f frames/s (%d frames in %.3f s)" % (B, arm, nframes / dt, nframes, dt))
eng.close()
finish()
