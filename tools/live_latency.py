#!/usr/bin/env python3
"""Latency of the live audio front-end (livespeechportraits_amd/live.py: LiveAudioFrontEnd, a LiveSessionPool of one) on the GPU,
recorded to profiles/<name>.json (+ .txt).
Synthetic weights and stand-in data from `synth`, as bench.py's pipeline_extra uses them (APC 3x GRU-512, Audio2Feature, the default
head-pose WaveNet, a 30 000-row feature database, a 687-frame = 183 200-sample clip):
  (a) per-push wall time, from the call to the returned frames being on the host, for pushes of exactly one frame of audio (alternating
      266 and 267 samples) over the whole clip: p50, p99, max; and the total time of that stream (pushes + finish);
  (b) the whole-clip audio stages (all the audio at once) in the same session: mel.compute_mel -> APC_encoder -> manifold.project ->
      Audio2FeatureModel / Audio2HeadposeModel.generate_sequences, median of 3 after a warm-up.
    python tools/live_latency.py [name, default live_latency] [output directory, default profiles/]"""
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
from livespeechportraits_amd import manifold, mel, synth  # noqa: E402
from livespeechportraits_amd.apc import APC_encoder  # noqa: E402
from livespeechportraits_amd.live import LiveAudioFrontEnd  # noqa: E402
from livespeechportraits_amd.models import create_model  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "live_latency"
out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
dev = torch.device("cuda:0")
NFRAME, NSAMP = 687, 183200
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
db = torch.from_numpy(db_np).to(dev)
wave = (0.1 * np.random.default_rng(1).standard_normal(NSAMP)).astype(np.float32)
pre = np.zeros(12, np.float32)
rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "clip_frames": NFRAME, "clip_samples": NSAMP, "database_rows": 30000}

pieces, pos, k = [], 0, 0
while pos < NSAMP:
    nxt = min(int((k + 1) * 16000 / 60), NSAMP)
    pieces.append(nxt - pos)
    pos, k = nxt, k + 1


def live_run():
    s = LiveAudioFrontEnd(apc, a2f, a2h, db_np, True, 10, 1.0, pre, 0.3, device=dev, feature_opt=fopt, headpose_opt=hopt)
    torch.cuda.synchronize()
    ts, pos = [], 0
    t_all = time.perf_counter()
    for k in pieces:
        t0 = time.perf_counter()
        s.push(wave[pos:pos + k], host=True)
        ts.append(time.perf_counter() - t0)
        pos += k
    s.finish(host=True)
    return np.array(ts), time.perf_counter() - t_all


live_run()                                                   # warm-up: engines, kernels, allocator
ts, total = live_run()
rec["a"] = {"pushes": len(ts), "push_sizes": sorted(set(pieces)), "p50_ms": round(float(np.percentile(ts, 50)) * 1e3, 3),
            "p99_ms": round(float(np.percentile(ts, 99)) * 1e3, 3), "max_ms": round(float(ts.max()) * 1e3, 3),
            "stream_total_s": round(total, 4), "budget_ms_at_60fps": round(1e3 / 60, 3)}
say("(a) live, one frame of audio per push (%s samples), %d pushes: p50 %.3f ms, p99 %.3f ms, max %.3f ms (budget %.3f ms at 60 fps); "
    "whole stream incl. finish(): %.3f s" % (rec["a"]["push_sizes"], len(ts), rec["a"]["p50_ms"], rec["a"]["p99_ms"], rec["a"]["max_ms"],
                                             rec["a"]["budget_ms_at_60fps"], total))


def whole():
    mels = mel.compute_mel(torch.from_numpy(wave).to(dev)).unsqueeze(0)
    feats = apc.forward(mels, torch.Tensor([mels.shape[1]]))[0]
    feats = manifold.project(feats.contiguous(), db, 10, 1.0).cpu().numpy()
    a2f.generate_sequences(feats, 16000, 60, fill_zero=True, opt=fopt)
    a2h.generate_sequences(feats, pre, fill_zero=True, sigma_scale=0.3, opt=hopt)


whole()
wt = []
for _ in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    whole()
    wt.append(time.perf_counter() - t0)
rec["b"] = {"whole_clip_s": sorted(round(v, 4) for v in wt)}
say("(b) whole clip at once (compute_mel -> APC_encoder -> manifold.project -> generate_sequences x2): %s s (median %.3f s)"
    % (rec["b"]["whole_clip_s"], sorted(wt)[1]))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, name + ".json"), "w") as fh:
    json.dump(rec, fh, indent=1)
with open(os.path.join(out_dir, name + ".txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
