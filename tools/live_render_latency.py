#!/usr/bin/env python3
"""Latency of the live render pool (livespeechportraits_amd/live_render.py), recorded to profiles/<name>.txt (+ .json).  Set-up as
tools/live_pool_latency.py (synthetic weights, 30 000-row database) with the `normal` fp32 generator at 512 x 512 and the invented avatar
of tests/golden/landmarks_may (its AMPs scaled so that the synthetic audio models' rows stay in view).
  (a) per tick p50 / p99 / max, call to frames of all sessions on the host, for S in {1, 4, 16} sessions that each push one frame of audio
      per tick (opened two ticks apart), without and with JPEG (quality 75).  The percentiles are over the steady ticks: those in which
      every session pushes AND gets a frame back (S frames rendered per tick).
  (b) for comparison, the numpy restatement of the reference's post-processing (tests/landmark_model.py) on one session's rows on this
      host: the whole clip at once, which is the only form the reference has.
  (c) 60 fps portraits one process sustains = S / (60 x p50 tick) at the best S.
`--trace S TICKS`: no timing, only 2 (S - 1) + 120 + TICKS ticks of S sessions, for a `rocprofv3 --kernel-trace --stats` run of its own
(own process after `--`, no counters in it); `--kernel-time <results.db> [<results.db> ...]` then prints the landmark launch's time.
Every GPU step runs under its own time limit and the steps are chained, so that nothing starts after one has failed:
    timeout -k 10 420 python tools/live_render_latency.py [name, default live_render_latency] [output directory, default profiles/] && \
    timeout -k 10 200 rocprofv3 --kernel-trace --stats -d <dir> -o s16 -- python tools/live_render_latency.py --trace 16 100 && \
    python tools/live_render_latency.py --kernel-time <dir>/*/s16_results.db        (reads the trace; no GPU)"""
import argparse
import json
import os
import sys
import tempfile
import time

if "--kernel-time" in sys.argv:
    import sqlite3
    for db in sys.argv[sys.argv.index("--kernel-time") + 1:]:
        cur = sqlite3.connect(db).cursor()
        q = "select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels where name like '%lmk_frames%' group by name"
        for n, c, avg, lo, hi in cur.execute(q):
            print("%s: %s  launches %d  mean %.2f us  min %.2f us  max %.2f us" % (os.path.basename(db), n.split("(")[0].replace("void ", ""), c, avg / 1e3, lo / 1e3, hi / 1e3))
    sys.exit(0)

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import landmark_model as M  # noqa: E402
from livespeechportraits_amd import synth  # noqa: E402
from livespeechportraits_amd.apc import APC_encoder  # noqa: E402
from livespeechportraits_amd.landmarks import LandmarkStage  # noqa: E402
from livespeechportraits_amd.live_pool import LiveSessionPool  # noqa: E402
from livespeechportraits_amd.live_render import LivePortraitPool  # noqa: E402
from livespeechportraits_amd.models import create_model  # noqa: E402
from livespeechportraits_amd.topology import build_topology  # noqa: E402

trace = int(sys.argv[sys.argv.index("--trace") + 1]) if "--trace" in sys.argv else 0
TRACE_TICKS = int(sys.argv[sys.argv.index("--trace") + 2]) if trace else 0
args = [a for a in sys.argv[1:] if not a.startswith("--")] if not trace else []
name = args[0] if len(args) > 0 else "live_render_latency"
out_dir = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles")
dev = torch.device("cuda:0")
NFRAME = 360
NSAMP = int(NFRAME / 60 * 16000)
tmp = tempfile.mkdtemp()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


apc = APC_encoder(80, 512, 3, False)
apc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_apc_state_dict().items()})
apc = apc.to(dev).eval()
ck = os.path.join(tmp, "Audio2Feature.pkl")
torch.save({"module." + k: torch.from_numpy(v) for k, v in synth.make_a2f_state_dict().items()}, ck)
fopt = argparse.Namespace(model="audio2feature", gpu_ids=[0], isTrain=False, checkpoints_dir=tmp, name="a2f", load_epoch=ck, verbose=False,
                          feature_decoder="LSTM", loss="L2", A2L_GMM_ndim=75, A2L_GMM_ncenter=1, predict_length=1, APC_hidden_size=512, frame_future=18)
a2f = create_model(fopt)
a2f.setup(fopt)
a2f.eval()
ch = os.path.join(tmp, "Audio2Headpose.pkl")
torch.save({"module." + k: torch.from_numpy(v) for k, v in synth.make_a2h_state_dict(dict(synth.A2H_DEFAULTS)).items()}, ch)
hopt = argparse.Namespace(
    model="audio2headpose", gpu_ids=[0], isTrain=False, checkpoints_dir=tmp, name="x", load_epoch=ch, verbose=False,
    feature_decoder="WaveNet", loss="GMM", A2H_GMM_ndim=12, A2H_GMM_ncenter=1, APC_hidden_size=512,
    A2H_wavenet_residual_layers=7, A2H_wavenet_residual_blocks=2, A2H_wavenet_residual_channels=128,
    A2H_wavenet_dilation_channels=128, A2H_wavenet_skip_channels=256, A2H_wavenet_kernel_size=2, time_frame_length=1,
    A2H_wavenet_use_bias=True, A2H_wavenet_input_channels=12, A2H_wavenet_cond_channels=512, frame_future=15)
a2h = create_model(hopt)
a2h.setup(hopt)
a2h.eval()
db_np = synth.make_feature_database(30000, 8, 512, 24)[0]
topo = build_topology("normal", ngf=64, num_downs=8, size=512)
gopt = argparse.Namespace(model="feature2face", gpu_ids=[0], isTrain=False, size="normal", ngf=64, n_downsample_G=8, fp16=0, checkpoints_dir=tmp,
                          name="t", load_epoch="none", verbose=False)
f2f = create_model(gopt)
f2f._g().load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.make_state_dict(topo, 3).items()})
f2f.eval()
cand = torch.from_numpy(synth.make_inputs(1, 512, seed=5, cand_batch=1)[1]).to(dev)
av = dict(np.load(os.path.join(ROOT, "tests", "golden", "landmarks_may.npz")))
SET = dict(mouth_sigma=1.5, head_sigma=[5, 10], amp_method="XYZ", amp=[0.004, 0.004, 0.004], rot_amp=0.5, trans_amp=0.002, shoulder_amp=0.5)
wave = (0.1 * np.random.default_rng(1).standard_normal(NSAMP)).astype(np.float32)
pre = np.zeros(12, np.float32)

pieces, pos, k = [], 0, 0
while pos < NSAMP:
    nxt = min(int((k + 1) * 16000 / 60), NSAMP)
    pieces.append(nxt - pos)
    pos, k = nxt, k + 1
starts = np.concatenate([[0], np.cumsum(pieces)])
piece = lambda k: wave[starts[k]:starts[k + 1]]


def new_stage(S):
    return LandmarkStage(av["mean_pts3d"], av["std_mean_pts3d"], av["candidate_eye_brow"], av["mean_translation"], av["camera_intrinsic"], av["scale"][()],
                         av["shoulder3D"], av["ref_trans"], shoulder_AMP=SET["shoulder_amp"], AMP_method=SET["amp_method"], Feat_AMPs=SET["amp"],
                         rot_AMP=SET["rot_amp"], trans_AMP=SET["trans_amp"], Feat_smooth_sigma=SET["mouth_sigma"], Head_smooth_sigma=SET["head_sigma"],
                         image_pad=[int(v) for v in av["image_pad"]], device=dev, max_sessions=S)


def new_pool(S):
    audio = LiveSessionPool(apc, a2f, a2h, db_np, True, 10, 1.0, sigma_scale=0.3, device=dev, max_sessions=S, feature_opt=fopt, headpose_opt=hopt)
    return LivePortraitPool(audio, new_stage(S), f2f, cand, max_batch=8)


def serve(S, jpeg, ticks=None):
    """tick t: session j (opened at tick 2j) pushes its piece t - 2j; -> (wall time, frames handed out) per tick"""
    pool = new_pool(S)
    ts, nf, live = [], [], {}
    for t in range(ticks if ticks is not None else len(pieces) + 2 * (S - 1)):
        if t % 2 == 0 and t // 2 < S:
            live[t // 2] = pool.open(pre)
        work = [(j, t - 2 * j) for j in sorted(live) if 0 <= t - 2 * j < len(pieces)]
        fin = [live[j] for j, k in work if k == len(pieces) - 1]
        t0 = time.perf_counter()
        out = pool.tick({live[j]: piece(k) for j, k in work}, finish=fin, host=True, jpeg_quality=75 if jpeg else None)
        ts.append(time.perf_counter() - t0)
        nf.append(sum(len(f) for _, f in out.values()) if len(work) == S and not fin else -1)
        for j, k in work:
            if k == len(pieces) - 1:
                live.pop(j)
    return np.array(ts), np.array(nf)


if trace:
    serve(trace, False, ticks=2 * (trace - 1) + 120 + TRACE_TICKS)
    torch.cuda.synchronize()
    print("traced: %d sessions, %d ticks in all" % (trace, 2 * (trace - 1) + 120 + TRACE_TICKS))
    sys.exit(0)

rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "clip_frames": NFRAME, "database_rows": 30000, "generator": "normal f32 512", "a": {}}
serve(2, True, ticks=150)                                        # warm-up: engines, graphs, kernels, allocator, the JPEG encoder
serve(2, False, ticks=150)
stat = lambda ts: {"p50_ms": round(float(np.percentile(ts, 50)) * 1e3, 3), "p99_ms": round(float(np.percentile(ts, 99)) * 1e3, 3),
                   "max_ms": round(float(ts.max()) * 1e3, 3), "ticks": int(len(ts))}
fmt = lambda d: "p50 %.3f ms, p99 %.3f ms, max %.3f ms over %d ticks" % (d["p50_ms"], d["p99_ms"], d["max_ms"], d["ticks"])
say("(a) one frame of audio per session and tick, sessions opened two ticks apart; call -> frames of all sessions on the host; steady ticks (S frames out)")
best = None
for S in (1, 4, 16):
    rec["a"][S] = {}
    for jpeg in (False, True, False, True):                      # alternated, so that box noise shows
        ts, nf = serve(S, jpeg)
        d = stat(ts[nf == S])
        rec["a"][S].setdefault("jpeg" if jpeg else "uint8", []).append(d)
        say("    S = %2d  %-22s %s" % (S, "JPEG files (q 75)" if jpeg else "uint8 frames", fmt(d)))
    p50 = min(d["p50_ms"] for d in rec["a"][S]["uint8"])
    if best is None or S / p50 > best[0] / best[1]:
        best = (S, p50)
# (b) the host restatement on one session's rows
audio = LiveSessionPool(apc, a2f, a2h, db_np, True, 10, 1.0, sigma_scale=0.3, device=dev, max_sessions=1, feature_opt=fopt, headpose_opt=hopt)
sid = audio.open(pre)
mouth, poses = [], []
for k in range(len(pieces)):
    o = audio.tick({sid: piece(k)}, finish=[sid] if k == len(pieces) - 1 else [], host=True)[sid]
    mouth.append(o.mouth)
    poses.append(o.poses)
mouth, poses = np.concatenate(mouth).reshape(-1, 75), np.concatenate(poses).reshape(-1, 12)
cfg = dict(SET, **{k: av[k] for k in ("mean_pts3d", "std_mean_pts3d", "candidate_eye_brow", "mean_translation", "ref_trans", "camera_intrinsic",
                                      "relative_rotation", "relative_translation", "shoulder3D")}, scale=av["scale"][()], image_pad=[int(v) for v in av["image_pad"]])
host_ms = []
for _ in range(3):
    t0 = time.perf_counter()
    M.clip(mouth, poses, cfg, True)
    host_ms.append((time.perf_counter() - t0) * 1e3)
n = min(len(mouth), len(poses))
rec["b"] = {"frames": n, "whole_clip_ms": round(min(host_ms), 2), "per_frame_ms": round(min(host_ms) / n, 4)}
say("(b) numpy restatement of the reference's post-processing on this host, one session, whole clip of %d frames: %.2f ms (%.4f ms per frame; x S per tick"
    " for S sessions, and only once the clip is over)" % (n, min(host_ms), min(host_ms) / n))
rec["c"] = {"best_S": best[0], "portraits_60fps": round(best[0] * 1e3 / (60 * best[1]), 2)}
say("(c) 60 fps portraits one process sustains, S / (60 x p50 tick): %.2f (S = %d, uint8 frames)" % (rec["c"]["portraits_60fps"], best[0]))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, name + ".json"), "w") as fh:
    json.dump(rec, fh, indent=1)
with open(os.path.join(out_dir, name + ".txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
