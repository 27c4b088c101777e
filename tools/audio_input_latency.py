#!/usr/bin/env python3
"""Cost of the audio input stage (livespeechportraits_amd/audio_input.py), recorded to profiles/<name>.txt (+ .json).
Set-up as tools/live_record_latency.py: synthetic weights, the `normal` fp32 generator at 512 x 512, the invented avatar of
tests/golden/landmarks_may; the clip is 300 frames.
  Host side: S in {1, 4, 16} sessions, opened two ticks apart, each pushes one frame of audio per tick.  A-B-A-B per S, with
  A = the path without the stage (the pool is fed the pre-resampled 16 kHz float32 clip, 266 / 267 samples per tick) and B = 48 kHz int16
  sessions through the stage (800 raw samples per tick).  The time is from the call to tick() to its return (frames stay on the device);
  p50 / p99 over the steady ticks (every session pushes and gets a frame back).
  The comparator a user would otherwise run on the host: scipy.signal.resample_poly(x, 1, 3) for the same 16 x 800 samples, 1 thread and
  16 threads, plus the upload of the result.
`--trace S TICKS`: no timing, only the stage alone: S sessions (48 kHz int16 and 44.1 kHz float32 alternating) push one frame per tick
(800 / 735 samples) for TICKS ticks, for a `rocprofv3 --kernel-trace --stats` run of its own (own process after `--`, no counters in it);
`--kernel-time <results.db> ...` then prints the stage's launches.  Every GPU step runs under its own time limit and the steps are chained:
    timeout -k 10 500 python tools/audio_input_latency.py [name, default audio_input_latency] [output directory, default profiles/] && \\
    timeout -k 10 120 rocprofv3 --kernel-trace --stats -d <dir> -o s16 -- python tools/audio_input_latency.py --trace 16 200 && \\
    python tools/audio_input_latency.py --kernel-time <dir>/s16_results.db        (reads the trace; no GPU)"""
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
        q = "select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels where name like '%rs_outputs%' group by name"
        for n, c, avg, lo, hi in cur.execute(q):
            print("%s: %s  launches %d  mean %.2f us  min %.2f us  max %.2f us" % (os.path.basename(db), n.split("(")[0].replace("void ", ""), c, avg / 1e3, lo / 1e3, hi / 1e3))
    sys.exit(0)

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from livespeechportraits_amd.audio_input import AudioInputStage  # noqa: E402

dev = torch.device("cuda:0")
trace = int(sys.argv[sys.argv.index("--trace") + 1]) if "--trace" in sys.argv else 0
if trace:
    ticks = int(sys.argv[sys.argv.index("--trace") + 2])
    st = AudioInputStage([48000, 44100], dev, max_sessions=trace, max_push=1600)
    rng = np.random.default_rng(2)
    spec = [(48000, "s16", 800) if j % 2 == 0 else (44100, "f32", 735) for j in range(trace)]
    sids = [st.open(r, f) for r, f, _ in spec]
    frames = [rng.integers(-8000, 8000, n).astype(np.int16) if f == "s16" else rng.normal(0, 0.2, n).astype(np.float32) for _, f, n in spec]
    for _ in range(ticks):
        st.tick(dict(zip(sids, frames)))
    torch.cuda.synchronize()
    print("traced: %d sessions, %d ticks, %d launches" % (trace, ticks, st.launches))
    sys.exit(0)

from livespeechportraits_amd import synth  # noqa: E402
from livespeechportraits_amd.apc import APC_encoder  # noqa: E402
from livespeechportraits_amd.landmarks import LandmarkStage  # noqa: E402
from livespeechportraits_amd.live_pool import LiveSessionPool  # noqa: E402
from livespeechportraits_amd.live_render import LivePortraitPool  # noqa: E402
from livespeechportraits_amd.models import create_model  # noqa: E402
from livespeechportraits_amd.topology import build_topology  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
name = args[0] if len(args) > 0 else "audio_input_latency"
out_dir = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles")
NFRAME = 300
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
pre = np.zeros(12, np.float32)

raw = np.clip(np.rint(0.1 * np.random.default_rng(1).standard_normal(NFRAME * 800) * 32768), -32768, 32767).astype(np.int16)
clip16 = AudioInputStage([48000], dev, max_sessions=1).resample_clip(raw, 48000).cpu().numpy()       # what path A is fed: resampled beforehand
cuts16 = [k * 16000 // 60 for k in range(NFRAME + 1)]


def new_pool(S, staged):
    audio = LiveSessionPool(apc, a2f, a2h, db_np, True, 10, 1.0, sigma_scale=0.3, device=dev, max_sessions=S, feature_opt=fopt, headpose_opt=hopt)
    stage = LandmarkStage(av["mean_pts3d"], av["std_mean_pts3d"], av["candidate_eye_brow"], av["mean_translation"], av["camera_intrinsic"], av["scale"][()],
                          av["shoulder3D"], av["ref_trans"], shoulder_AMP=SET["shoulder_amp"], AMP_method=SET["amp_method"], Feat_AMPs=SET["amp"],
                          rot_AMP=SET["rot_amp"], trans_AMP=SET["trans_amp"], Feat_smooth_sigma=SET["mouth_sigma"], Head_smooth_sigma=SET["head_sigma"],
                          image_pad=[int(v) for v in av["image_pad"]], device=dev, max_sessions=S)
    return LivePortraitPool(audio, stage, f2f, cand, max_batch=8, audio_input=AudioInputStage([48000], dev, max_sessions=S, max_push=1600) if staged else None)


def serve(S, staged, ticks=None):
    """tick t: session j (opened at tick 2j) pushes its frame t - 2j -> wall time per tick and whether the tick was steady"""
    pool = new_pool(S, staged)
    ts, steady, live = [], [], {}
    for t in range(ticks if ticks is not None else NFRAME + 2 * (S - 1)):
        if t % 2 == 0 and t // 2 < S:
            live[t // 2] = pool.open(pre, **(dict(input_rate=48000, input_format="s16") if staged else {}))
        work = [(j, t - 2 * j) for j in sorted(live) if 0 <= t - 2 * j < NFRAME]
        fin = [live[j] for j, k in work if k == NFRAME - 1]
        push = {live[j]: raw[800 * k:800 * k + 800] if staged else clip16[cuts16[k]:cuts16[k + 1]] for j, k in work}
        t0 = time.perf_counter()
        out = pool.tick(push, finish=fin)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        steady.append(len(work) == S and not fin and sum(len(f) for _, f in out.values()) == S)
        for j, k in work:
            if k == NFRAME - 1:
                live.pop(j)
    return np.array(ts)[np.array(steady)]


rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "clip_frames": NFRAME, "generator": "normal f32 512", "S": {}, "host": {}}
for staged in (False, True):                                         # warm-up: engines, kernels, allocator
    serve(2, staged, ticks=120)
stat = lambda ts: {"p50_ms": round(float(np.percentile(ts, 50)) * 1e3, 3), "p99_ms": round(float(np.percentile(ts, 99)) * 1e3, 3), "ticks": int(len(ts))}
say("one frame of audio per session and tick over a %d-frame clip, sessions opened two ticks apart; call -> return of tick() + synchronize, steady ticks" % NFRAME)
say("A: 16 kHz float32 pushed (resampled beforehand: the pool without the stage)   B: 48 kHz int16 pushed, resampled by the stage inside the tick")
for S in (1, 4, 16):
    rec["S"][S] = {"A": [], "B": []}
    for staged in (False, True, False, True):
        d = stat(serve(S, staged))
        rec["S"][S]["B" if staged else "A"].append(d)
        say("    S = %2d  (%s)  p50 %.3f ms, p99 %.3f ms over %d ticks" % (S, "B" if staged else "A", d["p50_ms"], d["p99_ms"], d["ticks"]))
    a, b = [d["p50_ms"] for d in rec["S"][S]["A"]], [d["p50_ms"] for d in rec["S"][S]["B"]]
    say("    S = %2d  p50: A %.3f / %.3f ms (A-A spread %.3f), B %.3f / %.3f ms; B - A = %+.3f ms" % (S, a[0], a[1], abs(a[0] - a[1]), b[0], b[1], np.mean(b) - np.mean(a)))

# the host resampler a user of the 16 kHz-only pool would run instead: scipy's polyphase filter with its default window, then one upload
from concurrent.futures import ThreadPoolExecutor  # noqa: E402
from scipy.signal import resample_poly  # noqa: E402
frames = [raw[800 * k:800 * k + 800].astype(np.float32) / 32768 for k in range(16)]


def host_once(pool):
    t0 = time.perf_counter()
    ys = list(pool.map(lambda x: resample_poly(x, 1, 3).astype(np.float32), frames)) if pool else [resample_poly(x, 1, 3).astype(np.float32) for x in frames]
    torch.from_numpy(np.concatenate(ys)).to(dev)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


for label, pool in (("1 thread", None), ("16 threads", ThreadPoolExecutor(16))):
    for _ in range(20):
        host_once(pool)
    d = stat(np.array([host_once(pool) for _ in range(300)]))
    rec["host"][label] = d
    say("    host: scipy.signal.resample_poly(x, 1, 3) of 16 x 800 samples + one upload, %-10s p50 %.3f ms, p99 %.3f ms (no session state: each frame filtered alone)" % (label + ":", d["p50_ms"], d["p99_ms"]))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, name + ".json"), "w") as fh:
    json.dump(rec, fh, indent=1)
with open(os.path.join(out_dir, name + ".txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
shutil.rmtree(tmp)
