#!/usr/bin/env python3
"""Pins the audio input stage on REAL librosa the moment librosa and resampy are importable (neither is in this image: the resampler is
PARITY-UNPINNED against librosa until this script has run somewhere and its fixture is committed).

  python tools/pin_resample_fixture.py [--out tests/golden]

Calls what the reference calls -- demo.py:179: librosa.load(path, sr=16000), which for a 44.1 kHz file is
librosa.resample(y, 44100, 16000, res_type='kaiser_best') (librosa 0.7: resampy.resample + fix_length to ceil(n * 16000 / 44100)) -- on
1 500 samples of N(0, 0.3) noise, reports the float64 model of tests/resample_model.py against it, and writes
tests/golden/resample_librosa.npz (x, rate, y) + .json.  tests/test_audio_input_cpu.py::test_resampler_matches_real_librosa compares the
model with the fixture when it exists and reports "unpinned" (xfail) when it does not.  If librosa or resampy is missing the script says
so, writes nothing and exits 2."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    try:
        import librosa
        import resampy
    except ImportError as e:
        print("pin_resample_fixture: %s -- nothing written; the resampler stays parity-unpinned against librosa "
              "(requirements.txt of the reference pins librosa==0.7.0, which resamples through resampy)" % e, file=sys.stderr)
        return 2
    import resample_model as RM
    rate = 44100
    x = np.random.default_rng(rate).normal(0, 0.3, 1500).astype(np.float32)
    try:
        y = librosa.resample(x, rate, 16000, res_type="kaiser_best")                # librosa 0.7's positional form
    except TypeError:
        y = librosa.resample(x, orig_sr=rate, target_sr=16000, res_type="kaiser_best")
    y = np.asarray(y, np.float32)
    ours = RM.resample64(x.astype(np.float64), rate)
    err = float(np.abs(ours[:-1] - y[:-1]).max()) if ours.shape == y.shape else float("nan")
    print("tests/resample_model.resample64 vs librosa %s / resampy %s: %d outputs, max-abs %.3e without the last sample (librosa pads it)"
          % (librosa.__version__, resampy.__version__, len(y), err))
    os.makedirs(a.out, exist_ok=True)
    np.savez_compressed(os.path.join(a.out, "resample_librosa.npz"), x=x, rate=np.int64(rate), y=y)
    json.dump({"librosa_version": librosa.__version__, "resampy_version": resampy.__version__, "model_max_abs": err,
               "generator": "tools/pin_resample_fixture.py: librosa.resample(x, 44100, 16000, res_type='kaiser_best'), demo.py:179"},
              open(os.path.join(a.out, "resample_librosa.json"), "w"), indent=1)
    return 0 if err <= 1e-4 else 1


if __name__ == "__main__":
    sys.exit(main())
