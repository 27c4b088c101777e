#!/usr/bin/env python3
"""Latency of the live session pool (livespeechportraits_amd/live_pool.py) against serving every stream from a pool of one, recorded to
profiles/<name>.txt (+ .json).  Set-up as tools/live_latency.py (synthetic weights, 30 000-row database, the 687-frame clip).
  (a) per tick p50 / p99 / max, call to frames of all sessions on the host, for S in {1, 2, 4, 8, 16} sessions that each push one frame of
      audio per tick, opened two ticks apart; and the same S served by S pools of one (LiveAudioFrontEnd objects) pushed one after
      another, alternated pool - objects - pool - objects per S so that box noise shows.  The percentiles are over the
      ticks in which all S sessions push.
  (b) the max tick of one session with prime_steps_per_tick 16 against 254 (priming in one go).
  (c) 60 fps streams one process sustains = 1 / (60 x p50 tick / S) at the best S, beside the pools-of-one figure from (a) at S = 1.
`--trace S TICKS`: no timing, only 2 (S - 1) + 40 + TICKS ticks of S sessions, for a `rocprofv3 --kernel-trace --stats` run of its own (own
process after `--`, no counters in it).  Two such runs that differ only in TICKS differ by TICKS steady-state ticks (every session past its
priming), so `--diff A_results.db B_results.db TICKS` prints launches and device time per steady tick, per kernel:
    rocprofv3 --kernel-trace --stats -d <dir> -o s16_200 -- python tools/live_pool_latency.py --trace 16 200
    python tools/live_pool_latency.py [name, default live_pool_latency] [output directory, default profiles/]"""
import argparse
import json
import os
import sys
import tempfile
import time

if "--diff" in sys.argv:
    import sqlite3
    a, b, ticks = sys.argv[sys.argv.index("--diff") + 1: sys.argv.index("--diff") + 4]
    q = "select name, count(*), sum(end - start) from kernels group by name"
    ka = {r[0]: r[1:] for r in sqlite3.connect(a).cursor().execute(q)}
    kb = {r[0]: r[1:] for r in sqlite3.connect(b).cursor().execute(q)}
    ticks = int(ticks)
    rows = sorted(((n, (kb[n][0] - ka.get(n, (0, 0))[0]) / ticks, (kb[n][1] - ka.get(n, (0, 0))[1]) / 1e3 / ticks) for n in kb), key=lambda r: -r[2])
    print("%-72s %12s %12s" % ("kernel, per steady-state tick", "launches", "device us"))
    for n, c, us in rows:
        if c > 0:
            print("%-72s %12.2f %12.2f" % (n.replace("void ", "")[:72], c, us))
    print("%-72s %12.2f %12.2f" % ("all kernels", sum(r[1] for r in rows), sum(r[2] for r in rows)))
    sys.exit(0)

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from livespeechportraits_amd import synth  # noqa: E402
from livespeechportraits_amd.apc import APC_encoder  # noqa: E402
from livespeechportraits_amd.live import LiveAudioFrontEnd  # noqa: E402
from livespeechportraits_amd.live_pool import LiveSessionPool  # noqa: E402
from livespeechportraits_amd.models import create_model  # noqa: E402

trace = int(sys.argv[sys.argv.index("--trace") + 1]) if "--trace" in sys.argv else 0
TRACE_TICKS = int(sys.argv[sys.argv.index("--trace") + 2]) if trace else 0
args = [a for a in sys.argv[1:] if not a.startswith("--")] if not trace else []
name = args[0] if len(args) > 0 else "live_pool_latency"
out_dir = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles")
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
wave = (0.1 * np.random.default_rng(1).standard_normal(NSAMP)).astype(np.float32)
pre = np.zeros(12, np.float32)

pieces, pos, k = [], 0, 0
while pos < NSAMP:
    nxt = min(int((k + 1) * 16000 / 60), NSAMP)
    pieces.append(nxt - pos)
    pos, k = nxt, k + 1
starts = np.concatenate([[0], np.cumsum(pieces)])
piece = lambda k: wave[starts[k]:starts[k + 1]]


def new_pool(S, **kw):
    return LiveSessionPool(apc, a2f, a2h, db_np, True, 10, 1.0, sigma_scale=0.3, device=dev, max_sessions=S, feature_opt=fopt, headpose_opt=hopt, **kw)


def serve(S, push_all, open_one, finish_one, ticks=None):
    """tick t: session j (opened at tick 2j) pushes its piece t - 2j; -> per-tick wall time"""
    ts, live = [], {}
    for t in range(ticks if ticks is not None else len(pieces) + 2 * (S - 1)):
        if t % 2 == 0 and t // 2 < S:
            live[t // 2] = open_one()
        work = [(j, t - 2 * j) for j in sorted(live) if 0 <= t - 2 * j < len(pieces)]
        t0 = time.perf_counter()
        push_all([(live[j], k) for j, k in work])
        ts.append(time.perf_counter() - t0)
        for j, k in work:
            if k == len(pieces) - 1:
                finish_one(live.pop(j))
    return np.array(ts)


def run_pool(S, ticks=None, **kw):
    pool = new_pool(S, **kw)
    return serve(S, lambda work: pool.tick({sid: piece(k) for sid, k in work}, host=True), lambda: pool.open(pre), lambda sid: pool.tick(finish=[sid]), ticks)


def run_objects(S):
    return serve(S, lambda work: [fe.push(piece(k), host=True) for fe, k in work],
                 lambda: LiveAudioFrontEnd(apc, a2f, a2h, db_np, True, 10, 1.0, pre, 0.3, device=dev, feature_opt=fopt, headpose_opt=hopt),
                 lambda fe: fe.finish())


if trace:
    run_pool(trace, ticks=2 * (trace - 1) + 40 + TRACE_TICKS)
    torch.cuda.synchronize()
    print("traced: %d sessions, %d ticks in all, of which the last %d with every session past its priming" % (trace, 2 * (trace - 1) + 40 + TRACE_TICKS, TRACE_TICKS))
    sys.exit(0)

rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "clip_frames": NFRAME, "database_rows": 30000, "a": {}}
run_pool(2, ticks=60)                                           # warm-up: engines, kernels, allocator
run_objects(1)
stat = lambda ts: {"p50_ms": round(float(np.percentile(ts, 50)) * 1e3, 3), "p99_ms": round(float(np.percentile(ts, 99)) * 1e3, 3),
                   "max_ms": round(float(ts.max()) * 1e3, 3)}
fmt = lambda d: "p50 %.3f ms, p99 %.3f ms, max %.3f ms" % (d["p50_ms"], d["p99_ms"], d["max_ms"])
say("(a) one frame of audio per session and tick, sessions opened two ticks apart; percentiles over the ticks in which all S sessions push")
best = None
for S in (1, 2, 4, 8, 16):
    full = slice(2 * (S - 1), len(pieces))
    runs = [("pool", run_pool(S)), ("objects", run_objects(S)), ("pool", run_pool(S)), ("objects", run_objects(S))]
    rec["a"][S] = [(kind, stat(ts[full])) for kind, ts in runs]
    for kind, ts in runs:
        say("    S = %2d  %-28s %s" % (S, "LiveSessionPool.tick" if kind == "pool" else "S pools of one, .push", fmt(stat(ts[full]))))
    p50 = min(d["p50_ms"] for kind, d in rec["a"][S] if kind == "pool")
    if best is None or p50 / S < best[1] / best[0]:
        best = (S, p50)
say("(b) one session, max tick over the whole clip: prime_steps_per_tick 16: %.3f ms; 254 (priming in one go): %.3f ms"
    % (run_pool(1, prime_steps_per_tick=16).max() * 1e3, run_pool(1, prime_steps_per_tick=254).max() * 1e3))
single = min(d["p50_ms"] for kind, d in rec["a"][1] if kind == "objects")
rec["c"] = {"best_S": best[0], "pool_streams_60fps": round(1e3 / (60 * best[1] / best[0]), 1), "pools_of_one_streams_60fps": round(1e3 / (60 * single), 1)}
say("(c) 60 fps streams one process sustains, 1 / (60 x p50 tick / S): pool %.1f (S = %d); S separate pools of one (LiveAudioFrontEnd) %.1f"
    % (rec["c"]["pool_streams_60fps"], best[0], rec["c"]["pools_of_one_streams_60fps"]))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, name + ".json"), "w") as fh:
    json.dump(rec, fh, indent=1)
with open(os.path.join(out_dir, name + ".txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
