#!/usr/bin/env python3
"""Cost of the device JPEG decoder (include/lspjpegdec.h, jpeg.JpegDecoder), recorded to profiles/jpeg_decode_time.txt.

    python tools/jpeg_decode_time.py [output directory, default profiles/]

runs every GPU step as a process of its own under `timeout`, one after the other, and stops at the first that fails:
  1..4  `rocprofv3 --kernel-trace --stats -- python tools/jpeg_decode_time.py --trace CASE REPS` for the cases below: device time per stage
        (no counters in these runs), read from the run's database with tools/rocprof_summary.py's query;
  5     `--e2e`: call to pixels on the device (plan on the host, one upload, three launches, status words back), A-B-A-B against Pillow on this
        host with 1 and 16 threads plus the upload of its pixels.  Without Pillow here that is recorded, and the host figure has to come from
        another machine, labelled as such.

Cases: `cand4` the four 512^2 quality-95 candidate files in one call; `rec8` / `rec64` 8 / 64 frames of 512^2 at quality 75 (the encoder
fixtures' files, as a recording holds them: no restart markers, one wave per frame); `rst64` the same 64 frames re-encoded with
restart_marker_rows=1 (32 waves per frame), to show what restart intervals buy -- needs Pillow for the re-encode, or the files as
`--restart-npz FILE` (arrays named like the frames).

    python tools/jpeg_decode_time.py --progressive [output directory]

is the progressive leg, recorded to profiles/jpeg_progressive_time.txt: `prog4`, the four 512^2 quality-95 candidates as progressive files
(tests/golden/jpeg_prog_512.npz) through JpegDecoder(progressive=True), beside `cand4`, their baseline twins through the existing path, in the
same session: the traces run prog4, cand4, prog4, cand4 (device time of jpegdec_progressive and of the whole call's kernels), then `--e2e` times
both calls A-B-A-B against Pillow decoding the same progressive files on this host with 1 and 16 threads plus the upload.

    python tools/jpeg_decode_time.py --parallel [output directory]

is the leg of the parallel route (JpegDecoder(parallel=True): decode inside a file in parallel), recorded to profiles/jpeg_parallel_time.txt:
`cand4`, `rec8` and `rec64` without and with the flag (`CASE+par`) in the same session.  The traces run CASE, CASE+par, CASE, CASE+par for each
case (device time of jpegdec_entropy against jpegdec_entropy_parallel; no counters), then `--e2e` times both calls A-B-A-B against Pillow on
this host with 1 and 16 threads plus the upload.  The file ends with the ratios and the A-A spread."""
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
CASES = ("cand4", "rec8", "rec64", "rst64")
PAR_CASES = ("cand4", "rec8", "rec64")


def restart_npz():
    return sys.argv[sys.argv.index("--restart-npz") + 1] if "--restart-npz" in sys.argv else None


def files_of(case):
    case = case.split("+")[0]
    if case == "prog4":
        z = np.load(os.path.join(GOLDEN, "jpeg_prog_512.npz"))
        return [z[k].tobytes() for k in sorted(z.files) if k.startswith("candidate_")]
    z = np.load(os.path.join(GOLDEN, "jpeg_dec_512.npz"))
    cand = [z[k].tobytes() for k in sorted(z.files) if k.startswith("candidate_")]
    rec = [z[k].tobytes() for k in sorted(z.files) if k.startswith("smooth_")]
    if case == "cand4":
        return cand
    if case in ("rec8", "rec64"):
        return rec * (1 if case == "rec8" else 8)
    if restart_npz():
        r = np.load(restart_npz())
        return [r[k].tobytes() for k in sorted(r.files)] * 8
    from PIL import Image
    out = []
    for data in rec:
        b = io.BytesIO()
        Image.open(io.BytesIO(data)).save(b, "JPEG", quality=75, restart_marker_rows=1)
        out.append(b.getvalue())
    return out * 8


def trace(case, reps):
    import torch
    from livespeechportraits_amd.jpeg import JpegDecoder
    files = files_of(case)
    dec = JpegDecoder("cuda:0", max_side=512, max_batch=64, progressive=case == "prog4", parallel=case.endswith("+par"))
    for _ in range(reps + 2):
        dec.decode(files)
    torch.cuda.synchronize()


def e2e(out_path, cases=CASES):
    import torch
    from livespeechportraits_amd.jpeg import JpegDecoder
    try:
        from PIL import Image
    except ImportError:
        Image = None
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "pillow": None if Image is None else Image.__version__, "cases": {}}

    def pil_one(data):
        return np.asarray(Image.open(io.BytesIO(data)))

    def pil_batch(files, pool):
        px = list(pool.map(pil_one, files)) if pool else [pil_one(f) for f in files]
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
    pool = ThreadPoolExecutor(16) if Image is not None else None
    for case in cases:
        if case == "rst64" and Image is None and not restart_npz():
            rec["cases"][case] = "skipped: the re-encode with restart markers needs Pillow or --restart-npz"
            continue
        files = files_of(case)
        dec = JpegDecoder(dev, max_side=512, max_batch=64, progressive=case == "prog4")
        legs = {"device": lambda: dec.decode(files)}
        if cases is PAR_CASES:
            par = JpegDecoder(dev, max_side=512, max_batch=64, parallel=True)
            legs["device_parallel"] = lambda: par.decode(files)
        if Image is not None and (cases is CASES or cases is PAR_CASES or case == "prog4"):
            legs["pillow_1_thread_plus_upload"] = lambda: pil_batch(files, None)
            legs["pillow_16_threads_plus_upload"] = lambda: pil_batch(files, pool)
        for fn in legs.values():
            fn()                                                   # warm: buffers, page faults, thread start
        reps = 10 if len(files) > 8 else 30
        rounds = {k: [] for k in legs}
        for _ in range(2):                                         # A-B-A-B: every leg twice, interleaved
            for k, fn in legs.items():
                rounds[k].append(ms(fn, reps))
        rec["cases"][case] = {"files": len(files), "bytes": sum(map(len, files)), "median_ms_per_call": rounds}
        print(case, json.dumps(rec["cases"][case]), flush=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


def stage_times(db, calls):
    cur = sqlite3.connect(db).cursor()
    rows = cur.execute("select name, count(*), sum(end-start) from kernels where name like '%jpegdec_%' group by name").fetchall()
    return {re.search(r"jpegdec_\w+", n).group(0): (c, t / 1e3 / c) for n, c, t in rows}


def main():
    progressive, parallel = "--progressive" in sys.argv, "--parallel" in sys.argv
    out_dir = next((a for a in sys.argv[1:] if not a.startswith("--") and a != restart_npz()), os.path.join(ROOT, "profiles"))
    work = tempfile.mkdtemp(prefix="jpeg_decode_time_")              # the traces' databases and the e2e record: read here, not kept
    extra = ["--restart-npz", restart_npz()] if restart_npz() else []
    lines = ["# tools/jpeg_decode_time.py%s: device JPEG decoder, 512^2 files; stage times from rocprofv3 --kernel-trace (average per launch, us)"
             % (" --progressive" if progressive else " --parallel" if parallel else "")]
    reps = 10 if parallel else 20
    stage1 = {}                                                      # --parallel: case -> the stage-1 times of its runs, in order
    order = [c + s for c in PAR_CASES for s in ("", "+par", "", "+par")] if parallel else ("prog4", "cand4", "prog4", "cand4") if progressive else CASES
    for run, case in enumerate(order):
        tag = "%s_%d" % (case, run)
        cmd = ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "-d", work, "-o", tag, "--", sys.executable, os.path.abspath(__file__),
               "--trace", case, str(reps)] + extra
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            lines.append("%s: the trace run ended with status %d; nothing after it was run\n%s" % (case, r.returncode, r.stderr[-800:]))
            break
        db = sorted(glob.glob(os.path.join(work, "**", tag + "_results.db"), recursive=True))
        st = stage_times(db[-1], reps + 2) if db else {}
        lines.append("%-9s %s   sum %.1f us" % (case, "  ".join("%s %.1f us" % (k, v[1]) for k, v in sorted(st.items())), sum(v[1] for v in st.values())))
        print(lines[-1], file=sys.stderr, flush=True)                 # progress: a session of many traces is long
        one = st.get("jpegdec_entropy_parallel" if case.endswith("+par") else "jpegdec_entropy")
        if one:
            stage1.setdefault(case, []).append(one[1])
    else:
        path = os.path.join(work, "e2e.json")
        r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--e2e", path] + (["--progressive"] if progressive else []) +
                           (["--parallel"] if parallel else []) + extra,
                           capture_output=True, text=True)
        if r.returncode != 0:
            lines.append("e2e: ended with status %d\n%s" % (r.returncode, r.stderr[-800:]))
        else:
            rec = json.load(open(path))
            lines.append("# call to pixels on the device, median ms per call, two rounds each (A-B-A-B); %s; Pillow on this host: %s" % (rec["device"], rec["pillow"] or "not installed"))
            for case, v in rec["cases"].items():
                lines.append("%-6s %s" % (case, v if isinstance(v, str) else "%d files, %d bytes: " % (v["files"], v["bytes"]) + "; ".join(
                    "%s %s" % (k, " / ".join("%.2f" % x for x in t)) for k, t in v["median_ms_per_call"].items())))
            if parallel:
                lines.append("# stage 1, unflagged over flagged (means of the two runs), and the A-A spread of each (|a1 - a2| / mean); call to pixels the same way,"
                             " and Pillow's best over the flagged call")
                spread = lambda t: abs(t[0] - t[1]) / (sum(t) / 2) if len(t) == 2 else float("nan")
                mean = lambda t: sum(t) / len(t)
                for case in PAR_CASES:
                    a, b = stage1.get(case, []), stage1.get(case + "+par", [])
                    v = rec["cases"].get(case)
                    if not a or not b or not isinstance(v, dict):
                        continue
                    t = v["median_ms_per_call"]
                    text = "%-6s stage 1 %.1f / %.1f us = %.1fx (spread %.1f%% / %.1f%%)" % (case, mean(a), mean(b), mean(a) / mean(b), 100 * spread(a), 100 * spread(b))
                    text += "; call %.2f / %.2f ms = %.1fx (spread %.1f%% / %.1f%%)" % (mean(t["device"]), mean(t["device_parallel"]), mean(t["device"]) / mean(t["device_parallel"]),
                                                                                      100 * spread(t["device"]), 100 * spread(t["device_parallel"]))
                    for k in ("pillow_1_thread_plus_upload", "pillow_16_threads_plus_upload"):
                        if k in t:
                            text += "; %s %.2f ms = %.2fx the flagged call" % (k, mean(t[k]), mean(t[k]) / mean(t["device_parallel"]))
                    lines.append(text)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "jpeg_progressive_time.txt" if progressive else "jpeg_parallel_time.txt" if parallel else "jpeg_decode_time.txt"), "w") as f:
        f.write(text)
    return 0 if "ended with status" not in text else 1


if __name__ == "__main__":
    if "--trace" in sys.argv:
        i = sys.argv.index("--trace")
        trace(sys.argv[i + 1], int(sys.argv[i + 2]))
    elif "--e2e" in sys.argv:
        e2e(sys.argv[sys.argv.index("--e2e") + 1], ("prog4", "cand4") if "--progressive" in sys.argv else PAR_CASES if "--parallel" in sys.argv else CASES)
    else:
        sys.exit(main())
