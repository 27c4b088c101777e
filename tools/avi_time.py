#!/usr/bin/env python3
"""Cost of writing the Motion-JPEG AVI (livespeechportraits_amd/video.py) in one session on the GPU, A-B-A-B in a fresh process, recorded to
profiles/<name>.json (+ .txt).  8 frames of 512^2 at q75 behind the `normal` bf16 batch-8 forward (the setting of profiles/jpeg_time_normal_b8.txt),
audio f32:
  (A) the host route: JpegEncoder.submit / collect (sizes, one copy per frame, header + bytes per frame) and AviWriter.append_jpegs;
  (B) the device route: DeviceMuxer.submit / collect (lspavi_pack, one copy per batch) and AviWriter.append_fragment;
  per batch on the host clock (forward + encode + fetch + append), and as render_frames frames/s with video=, both routes.
The default of the render loops (video.DEFAULT_VIDEO_ROUTE) is (B) only if (B) is not slower than (A) by more than the A-A spread of this session.
    python tools/avi_time.py [name] [output directory, default profiles/]
    python tools/avi_time.py --kernels      the device route alone, 20 batches: run under `rocprofv3 --kernel-trace --stats --` for the device time of
                                            avi_layout and avi_gather"""
import argparse
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
from livespeechportraits_amd import synth  # noqa: E402
from livespeechportraits_amd.engine import Engine  # noqa: E402
from livespeechportraits_amd.render_loop import render_frames  # noqa: E402
from livespeechportraits_amd.topology import build_topology  # noqa: E402
from livespeechportraits_amd.video import AviWriter, VideoSink, clip_audio  # noqa: E402

kernels_only = "--kernels" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
name = args[0] if args else "avi_time"
out_dir = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles")
dev = torch.device("cuda:0")
B, S, Q = 8, 512, 75
rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "batch": B, "size": S, "quality": Q, "audio": "f32"}
lines = []
tmp = tempfile.mkdtemp()


def say(s):
    print(s, flush=True)
    lines.append(s)


topo = build_topology("normal")
sd = synth.make_state_dict(topo, 1234)
eng = Engine("normal", size=S, max_batch=B, dtype="bf16")
eng.load_state_dict(sd)
eng.bind(eng.pack(), dev)
feats, cand = synth.make_inputs(B, S, seed=5, cand_batch=1)
fd, cd = torch.from_numpy(feats).to(dev), torch.from_numpy(cand).to(dev)
u8 = torch.empty((B, S, S, 3), dtype=torch.uint8, device=dev)
wave = (np.random.default_rng(7).standard_normal(16000 * 40) * 0.3).astype(np.float32)


def per_batch_ms(route, reps):
    """forward_image, then the route, then the append: host clock per batch of 8, the file on disk growing as it would"""
    with AviWriter(os.path.join(tmp, "t.avi"), S, S) as w:
        sink = VideoSink(w, S, Q, dev, B, *clip_audio(w, wave, dev), route=route)
        for _ in range(5):
            eng.forward_image(fd, cd, out_u8=u8)
            sink.submit(u8, w.nframes)
            sink.collect()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            eng.forward_image(fd, cd, out_u8=u8)
            sink.submit(u8, w.nframes)
            sink.collect()
        dt = time.perf_counter() - t0
        nbytes = w._movi / w.nframes
    return dt / reps * 1e3, nbytes


if kernels_only:
    per_batch_ms("device", 20)
    sys.exit(0)

rec["per_batch_ms"] = {"host": [], "device": []}
for route in ("host", "device", "host", "device", "host", "device"):
    ms, nbytes = per_batch_ms(route, 100)
    rec["per_batch_ms"][route].append(round(ms, 4))
    say("per batch of %d (forward + encode + fetch + append), route %s: %.4f ms (%.0f file bytes per frame)" % (B, route, ms, nbytes))

# ---- render_frames frames/s with video=, normal bf16, batch 8 ------------------------------------------------------------------
opt = argparse.Namespace(model="feature2face", gpu_ids=[0], isTrain=False, size="normal", ngf=64, n_downsample_G=8, fp16=0, checkpoints_dir=tmp, name="t",
                         load_epoch="none", verbose=False)
model = L.create_model(opt)
model._g().netG.dtype = "bf16"
model._g().load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
model.eval()
nframes = 512
maps = [torch.from_numpy(feats[i % B]).pin_memory() for i in range(nframes)]
rec["render_frames_fps"] = {"host": [], "device": []}
for route in ("host", "device"):                            # both routes warm (lanes, encoders, graphs) before the first timed arm
    with AviWriter(os.path.join(tmp, "w.avi"), S, S) as w:
        render_frames(model, iter(maps[:8 * B]), cd, batch=B, video=w, audio=wave, video_route=route)
for route in ("host", "device") * 5:
    with AviWriter(os.path.join(tmp, "w.avi"), S, S) as w:
        render_frames(model, iter(maps[:4 * B]), cd, batch=B, video=w, audio=wave, video_route=route)
    torch.cuda.synchronize()
    with AviWriter(os.path.join(tmp, "r.avi"), S, S) as w:
        t0 = time.perf_counter()
        render_frames(model, iter(maps), cd, batch=B, video=w, audio=wave, video_route=route)
        dt = time.perf_counter() - t0
    rec["render_frames_fps"][route].append(round(nframes / dt, 1))
    say("render_frames normal bf16 batch %d with video, route %s: %.1f frames/s (%d frames in %.3f s)" % (B, route, nframes / dt, nframes, dt))

a, b = rec["per_batch_ms"]["host"], rec["per_batch_ms"]["device"]
spread = max(a) - min(a)
fa, fb = rec["render_frames_fps"]["host"], rec["render_frames_fps"]["device"]
fspread = max(fa) - min(fa)
rec["verdict"] = {"host_ms_median": float(np.median(a)), "device_ms_median": float(np.median(b)), "host_spread_ms": round(spread, 4),
                  "device_not_slower_per_batch": bool(np.median(b) <= np.median(a) + spread),
                  "host_fps_median": float(np.median(fa)), "device_fps_median": float(np.median(fb)), "host_spread_fps": round(fspread, 1),
                  "device_not_slower_in_render_frames": bool(np.median(fb) >= np.median(fa) - fspread)}
say("verdict, one batch at a time: host median %.4f ms, device median %.4f ms, host A-A spread %.4f ms -> device route %s" % (
    np.median(a), np.median(b), spread, "is not slower" if rec["verdict"]["device_not_slower_per_batch"] else "is slower"))
say("verdict, render_frames on two lanes: host median %.1f frames/s, device median %.1f frames/s, host A-A spread %.1f -> device route %s" % (
    np.median(fa), np.median(fb), fspread, "is not slower" if rec["verdict"]["device_not_slower_in_render_frames"] else "is slower"))
eng.close()
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, name + ".json"), "w") as fh:
    json.dump(rec, fh, indent=1)
with open(os.path.join(out_dir, name + ".txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
