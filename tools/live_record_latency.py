#!/usr/bin/env python3
"""Cost of recording live sessions inside LivePortraitPool.tick (livespeechportraits_amd/live_render.py), recorded to
profiles/<name>.txt (+ .json).  Set-up as tools/live_render_latency.py: synthetic weights, the `normal` fp32 generator at 512 x 512, the
invented avatar of tests/golden/landmarks_may; the clip is 687 frames (the demo clip's length).
  S in {1, 4, 16} sessions, opened two ticks apart, each pushes one frame of audio per tick and is recorded from open() into its own
  AviWriter (float audio).  Per S, alternated: the unrecorded tick (frames to the host, the figure of profiles/live_render_latency.txt),
  then A-B-A-B with A = record_route "host" (JpegEncoder + append_jpegs per session: what the API offered before) and B = "device"
  (one lspavi_pack_multi per group of frames).  The time is from the call to tick() to its return, when every byte has been handed to the
  files; p50 / p99 / max over the steady ticks (every session pushes and gets a frame back).
`--trace S TICKS`: no timing, only 2 (S - 1) + 120 + TICKS ticks of S recorded sessions on the device route, for a
`rocprofv3 --kernel-trace --stats` run of its own (own process after `--`, no counters in it); `--kernel-time <results.db> ...` then prints
the muxer's launches.  Every GPU step runs under its own time limit and the steps are chained:
    timeout -k 10 500 python tools/live_record_latency.py [name, default live_record_latency] [output directory, default profiles/] && \\
    timeout -k 10 200 rocprofv3 --kernel-trace --stats -d <dir> -o s16 -- python tools/live_record_latency.py --trace 16 100 && \\
    python tools/live_record_latency.py --kernel-time <dir>/*/s16_results.db        (reads the trace; no GPU)"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

if "--kernel-time" in sys.argv:
    import sqlite3
    for db in sys.argv[sys.argv.index("--kernel-time") + 1:]:
        cur = sqlite3.connect(db).cursor()
        q = "select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels where name like '%avi_%' group by name"
        for n, c, avg, lo, hi in cur.execute(q):
            print("%s: %s  launches %d  mean %.2f us  min %.2f us  max %.2f us" % (os.path.basename(db), n.split("(")[0].replace("void ", ""), c, avg / 1e3, lo / 1e3, hi / 1e3))
    sys.exit(0)

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from livespeechportraits_amd import synth  # noqa: E402
from livespeechportraits_amd.apc import APC_encoder  # noqa: E402
from livespeechportraits_amd.landmarks import LandmarkStage  # noqa: E402
from livespeechportraits_amd.live_pool import LiveSessionPool  # noqa: E402
from livespeechportraits_amd.live_render import LivePortraitPool  # noqa: E402
from livespeechportraits_amd.models import create_model  # noqa: E402
from livespeechportraits_amd.topology import build_topology  # noqa: E402
from livespeechportraits_amd.video import AviWriter  # noqa: E402

trace = int(sys.argv[sys.argv.index("--trace") + 1]) if "--trace" in sys.argv else 0
TRACE_TICKS = int(sys.argv[sys.argv.index("--trace") + 2]) if trace else 0
args = [a for a in sys.argv[1:] if not a.startswith("--")] if not trace else []
name = args[0] if len(args) > 0 else "live_record_latency"
out_dir = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles")
dev = torch.device("cuda:0")
NFRAME = 687
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


def new_pool(S, route):
    audio = LiveSessionPool(apc, a2f, a2h, db_np, True, 10, 1.0, sigma_scale=0.3, device=dev, max_sessions=S, feature_opt=fopt, headpose_opt=hopt)
    return LivePortraitPool(audio, new_stage(S), f2f, cand, max_batch=8, **(dict(record_quality=75, record_route=route) if route else {}))


def serve(S, route, ticks=None):
    """tick t: session j (opened at tick 2j) pushes its piece t - 2j; route None: unrecorded, frames to the host.
    -> (wall time, frames handed out, bytes written) per tick"""
    pool = new_pool(S, route)
    where = tempfile.mkdtemp(dir=tmp)
    ts, nf, live, writers = [], [], {}, {}
    for t in range(ticks if ticks is not None else len(pieces) + 2 * (S - 1)):
        if t % 2 == 0 and t // 2 < S:
            j = t // 2
            if route:
                writers[j] = AviWriter(os.path.join(where, "%d.avi" % j), 512, 512)
            live[j] = pool.open(pre, video=writers.get(j))
        work = [(j, t - 2 * j) for j in sorted(live) if 0 <= t - 2 * j < len(pieces)]
        fin = [live[j] for j, k in work if k == len(pieces) - 1]
        t0 = time.perf_counter()
        out = pool.tick({live[j]: piece(k) for j, k in work}, finish=fin, host=route is None)
        ts.append(time.perf_counter() - t0)
        nf.append(sum(len(f) for _, f in out.values()) if len(work) == S and not fin else -1)
        for j, k in work:
            if k == len(pieces) - 1:
                live.pop(j)
    torch.cuda.synchronize()
    frames = sum(w.nframes for w in writers.values())
    for w in writers.values():
        w.close()
    nbytes = sum(os.path.getsize(w.path) for w in writers.values())
    shutil.rmtree(where)
    return np.array(ts), np.array(nf), frames, nbytes


if trace:
    serve(trace, "device", ticks=2 * (trace - 1) + 120 + TRACE_TICKS)
    print("traced: %d recorded sessions, %d ticks in all" % (trace, 2 * (trace - 1) + 120 + TRACE_TICKS))
    shutil.rmtree(tmp)
    sys.exit(0)

rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "clip_frames": NFRAME, "generator": "normal f32 512", "S": {}}
for route in ("host", "device", None):                           # warm-up: engines, kernels, allocator, both encoders' buffers
    serve(2, route, ticks=150)
stat = lambda ts: {"p50_ms": round(float(np.percentile(ts, 50)) * 1e3, 3), "p99_ms": round(float(np.percentile(ts, 99)) * 1e3, 3),
                   "max_ms": round(float(ts.max()) * 1e3, 3), "ticks": int(len(ts))}
fmt = lambda d: "p50 %.3f ms, p99 %.3f ms, max %.3f ms over %d ticks" % (d["p50_ms"], d["p99_ms"], d["max_ms"], d["ticks"])
say("one frame of audio per session and tick over the %d-frame clip, sessions opened two ticks apart, every session recorded from open() (q 75, f32 audio);" % NFRAME)
say("call -> return of tick(), steady ticks (S frames out).  unrecorded: uint8 frames copied to the host instead")
for S in (1, 4, 16):
    rec["S"][S] = {}
    for route in (None, "host", "device", "host", "device"):
        ts, nf, frames, nbytes = serve(S, route)
        d = dict(stat(ts[nf == S]), frames_written=frames, bytes_written=nbytes)
        rec["S"][S].setdefault(route or "unrecorded", []).append(d)
        say("    S = %2d  %-26s %s%s" % (S, "(%s) record_route=%s" % ("A" if route == "host" else "B", route) if route else "unrecorded, host=True", fmt(d),
                                       "  [%d frames, %.1f MB in %d files]" % (frames, nbytes / 1e6, S) if route else ""))
    a, b = [d["p50_ms"] for d in rec["S"][S]["host"]], [d["p50_ms"] for d in rec["S"][S]["device"]]
    say("    S = %2d  p50: A %.3f / %.3f ms (A-A spread %.3f), B %.3f / %.3f ms; B - A = %+.3f ms" % (S, a[0], a[1], abs(a[0] - a[1]), b[0], b[1], np.mean(b) - np.mean(a)))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, name + ".json"), "w") as fh:
    json.dump(rec, fh, indent=1)
with open(os.path.join(out_dir, name + ".txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
shutil.rmtree(tmp)
