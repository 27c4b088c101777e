"""The JPEG decoder without a device: the numpy restatement against Pillow's pixels, the library's host half (probe, planner, stage 1 run on
the host) against the restatement, every refusal, truncations and corruptions, the sanitizer-built stand-alone checker, AviReader against the
tests' own AVI parser, and the candidates' normalisation table.  The device half is tests/test_gpu_jpeg_decode.py."""
import hashlib
import io
import os
import shutil
import struct
import subprocess
import warnings

import numpy as np
import pytest

import avi_parser
import jpeg_decode_cases as K
import jpeg_decode_model as D
import jpeg_model as M
from conftest import ROOT

CSRC = os.path.join(ROOT, "livespeechportraits_amd", "csrc")


def _pillow():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


def _pil_pixels(data):
    """Pillow's pixels, or None when it does not open the file"""
    Image = _pillow()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return np.asarray(Image.open(io.BytesIO(data)))
    except Exception:
        return None


def _stage1(data):
    """(status, coefficients) of the model up to the end of stage 1"""
    try:
        f = D.parse(data)
        return 0, D.coefficients(data, f)
    except D.Refused as e:
        return e.status, None


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_the_model_gives_pillows_pixels_on_every_small_fixture():
    meta, files, pixels = K.fixtures()
    assert len(meta["cases"]) >= 100
    for name in K.small_names():
        got = D.decode(files[name])
        assert got.dtype == np.uint8 and got.shape == pixels[name].shape and np.array_equal(got, pixels[name]), name


def test_the_model_gives_pillows_pixels_on_the_512_frames():
    meta = K.fixtures()[0]
    files = K.frames_512()
    assert len(meta["frames"]) == 12
    for c in meta["frames"]:
        got = D.decode(files[c["name"]])
        assert list(got.shape) == c["shape"] and hashlib.sha256(got.tobytes()).hexdigest() == c["pixels_sha256"], c["name"]


def test_the_model_gives_pillows_pixels_on_a_fresh_pillow_run():
    Image = _pillow()
    if Image is None:
        pytest.skip("Pillow is not installed: the frozen fixtures stand in for it")
    n = 0
    for k, (h, w) in enumerate(((1, 1), (2, 3), (3, 4), (31, 18), (24, 56), (9, 2))):
        for ch, kw in ((3, {}), (3, {"subsampling": 0}), (3, {"subsampling": 1}), (3, {"optimize": True}), (3, {"restart_marker_blocks": 2}),
                       (3, {"restart_marker_rows": 1}), (1, {}), (1, {"restart_marker_blocks": 1})):
            img = M.make_image({"kind": ("noise", "extremes", "smooth")[(k + n) % 3] if ch == 3 else "noise", "h": h, "w": w, "channels": ch, "seed": 40 + n})
            b = io.BytesIO()
            Image.fromarray(img).save(b, "JPEG", quality=(1, 30, 75, 95, 100)[n % 5], **kw)
            assert np.array_equal(D.decode(b.getvalue()), np.asarray(Image.open(io.BytesIO(b.getvalue())))), (h, w, ch, kw)
            n += 1


def test_a_file_without_dht_uses_annex_k():
    meta, files, pixels = K.fixtures()
    names = [n for n in K.small_names() if n.endswith("_nodht")]
    assert len(names) == 2
    for n in names:
        assert b"\xff\xc4" not in files[n][:D.parse(files[n])["scan_begin"]]
        assert np.array_equal(D.decode(files[n]), pixels[n[:-6]])


# ---- the library's host half ------------------------------------------------------------------------------------------------------------
def test_probe_and_planner_agree_with_the_model():
    """geometry, quantisation tables, restart intervals and their offsets, and the coefficients of stage 1, for all small fixtures planned as
    ONE batch (files of every geometry side by side)"""
    from livespeechportraits_amd import jpeg as J
    _, files, _ = K.fixtures()
    names = K.small_names()
    plan = J.DecodePlan([files[n] for n in names])
    assert plan.summary.files == len(names) and plan.statuses() == [0] * len(names)
    seg = 0
    for i, n in enumerate(names):
        f = D.parse(files[n])
        hs, vs = f["comps"][0][1], f["comps"][0][2]
        want = (0, f["width"], f["height"], len(f["comps"]), hs, vs, f["restart"], f["mcux"] * f["mcuy"], len(f["segments"]))
        info = J.probe(files[n])
        assert tuple(info[:9]) == want, n
        assert (info.scan_offset, info.scan_bytes) == (f["scan_begin"], f["scan_end"] - f["scan_begin"]), n
        assert info.default_tables == (15 if n.endswith("_nodht") and len(f["comps"]) == 3 else 3 if n.endswith("_nodht") else 0), n
        planned = plan.file(i)
        assert tuple(planned[:9]) == want and planned.scan_bytes == info.scan_bytes, n
        data_at = planned.scan_offset
        assert bytes(plan.blob[data_at:data_at + info.scan_bytes]) == files[n][f["scan_begin"]:f["scan_end"]], n
        for c in range(len(f["comps"])):
            assert np.array_equal(plan.qtable(i, c), f["q"][f["comps"][c][3]]), (n, c)
        for begin, end, mcu0, nmcu in f["segments"]:
            assert plan.segment(seg) == (i, mcu0, nmcu, begin - f["scan_begin"] + data_at, end - f["scan_begin"] + data_at), (n, seg)
            seg += 1
        status, coef = plan.host_coefficients(i)
        assert status == 0 and np.array_equal(coef, D.coefficients(files[n], f)), n
    assert seg == plan.summary.segments


def test_a_512_frame_through_the_host_half():
    from livespeechportraits_amd import jpeg as J
    name, data = sorted(K.frames_512().items())[0]
    plan = J.DecodePlan([data])
    status, coef = plan.host_coefficients(0)
    assert status == 0 and np.array_equal(coef, D.coefficients(data)), name


@pytest.mark.parametrize("k", range(len(K.refusals())))
def test_every_refusal_returns_its_code(k):
    from livespeechportraits_amd import jpeg as J
    what, data, want = K.refusals()[k]
    model, _ = _stage1(data)
    assert model == want, "%s: the model says %d" % (what, model)
    plan = J.DecodePlan([data])
    status = plan.statuses()[0] or plan.host_coefficients(0)[0]
    assert status == want, "%s: the library says %d" % (what, status)
    if want == D.UNSUPPORTED or plan.statuses()[0]:
        assert J.probe(data).status == want, what        # what the parser and the scan walker see, probe reports


def test_the_range_fixture_passes_stage_1_and_is_range_in_the_model():
    from livespeechportraits_amd import jpeg as J
    data = K.fixtures()[1]["corrupt_range"]
    assert J.DecodePlan([data]).host_coefficients(0)[0] == 0             # the device finds it in stage 2 (tests/test_gpu_jpeg_decode.py)
    assert D.status_of(data) == D.RANGE


def _changed(files, names):
    """every truncation of three files, and single-byte changes at a fixed seed"""
    rng = np.random.default_rng(20261018)
    for n in names[:3]:
        for length in range(len(files[n])):
            yield n, files[n][:length]
    for n in names:
        for _ in range(25):
            b = bytearray(files[n])
            b[int(rng.integers(len(b)))] ^= int(rng.integers(1, 256))
            yield n, bytes(b)


def test_truncations_and_corruptions_give_an_error_or_pillows_pixels():
    """A changed file is refused, or it decodes to what Pillow returns for it: the library's stage 1 equals the model's (status and
    coefficients), and the model's pixels equal Pillow's wherever both decode.  Nothing crashes."""
    from livespeechportraits_amd import jpeg as J
    _, files, _ = K.fixtures()
    names = [K.find(p) for p in ("_420_9x3_", "_greyrst_5x2_", "_rstb_4x9_", "_422_40x72_", "_opt_16x16_", "_444_8x24_", "_grey_16x16_", "_rstr_40x72_")]
    counts = {"refused": 0, "decoded": 0, "pillow agrees": 0}
    batch = list(_changed(files, names))
    for at in range(0, len(batch), 64):
        part = batch[at:at + 64]
        plan = J.DecodePlan([d for _, d in part])
        for i, (n, data) in enumerate(part):
            status, coef = plan.host_coefficients(i)
            want, wcoef = _stage1(data)
            assert status == want and (want != 0 or np.array_equal(coef, wcoef)), (n, len(data), status, want)
            if want:
                counts["refused"] += 1
                continue
            try:
                px = D.pixels_from(wcoef, D.parse(data))
            except D.Refused as e:
                assert e.status == D.RANGE
                counts["refused"] += 1
                continue
            counts["decoded"] += 1
            ref = _pil_pixels(data) if _pillow() else None
            if ref is not None:
                assert ref.shape == px.shape and np.array_equal(ref, px), "%s changed: decoded, but not to Pillow's pixels" % n
                counts["pillow agrees"] += 1
    print(counts)
    assert counts["refused"] > 300 and counts["decoded"] > 20


def _sanitizer_works(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    cxx = os.environ.get("HOSTCXX", "c++")
    if shutil.which(cxx) is None:
        return "no host C++ compiler (%s)" % cxx
    r = subprocess.run([cxx, "-fsanitize=address,undefined", str(src), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        return "the host compiler has no sanitizer runtime: " + r.stderr.strip().split("\n")[-1]
    return None


def test_the_sanitizer_built_checker_runs_clean(tmp_path):
    """csrc/jpegdec_check.cpp (the parser, the planner and the segment decoder as host code under ASan + UBSan, with its own main) over all
    small fixtures, the refusals and the three corrupt files, every truncation of three files and 40 single-byte changes of each."""
    why = _sanitizer_works(tmp_path)
    if why:
        pytest.skip(why)
    subprocess.run(["make", "-C", CSRC, "-s", "check-jpegdec"], check=True)
    exe = os.path.join(CSRC, "build", "jpegdec_check")
    meta, files, _ = K.fixtures()
    entries = [files[n] for n in (K.find("_420_9x3_"), K.find("_rstr_40x72_"), K.find("_grey_16x16_"))]
    entries += [files[n] for n in K.small_names()] + [files[c["name"]] for c in meta["corrupt"]] + [d for _, d, _ in K.refusals()]
    bundle = bytearray(b"LSDB" + struct.pack("<I", len(entries)))
    for data in entries:
        status, coef = _stage1(data)
        coef = np.zeros(0, np.int16) if coef is None else np.ascontiguousarray(coef, "<i2").reshape(-1)
        bundle += struct.pack("<III", len(data), status, coef.size) + data + coef.tobytes()
    path = tmp_path / "bundle.bin"
    path.write_bytes(bytes(bundle))
    r = subprocess.run([str(exe), str(path), "20261018", "3", "40"], capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "0 failures" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr


# ---- AviReader ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("audio_format", ["f32", "s16", None])
def test_avi_reader_finds_what_the_parser_finds(tmp_path, audio_format):
    from livespeechportraits_amd import video as V
    _, files, _ = K.fixtures()
    name = K.find("_420_16x16_")
    jpegs = [files[name], D.strip_dht(files[name]), files[name]] * 3                 # chunks with and without DHT
    wave = (np.sin(np.arange(4000) / 7.0) * 0.5).astype(np.float32)
    path = str(tmp_path / "clip.avi")
    V.write_avi(path, jpegs, None if audio_format is None else wave, fps=30, audio_rate=8000, audio_format=audio_format or "f32")
    ref = avi_parser.parse(open(path, "rb").read())
    r = V.AviReader(path)
    assert (r.width, r.height, r.fps, r.nframes, r.channels) == (16, 16, 30, len(jpegs), 3)
    assert [r.jpeg(i) for i in range(r.nframes)] == ref["video"] == [bytes(j) for j in jpegs]
    if audio_format is None:
        assert r.audio_rate is None and r.audio_format is None and r.audio() is None
    else:
        assert (r.audio_rate, r.audio_format) == (8000, audio_format)
        assert r.audio().dtype == ref["audio"].dtype and np.array_equal(r.audio(), ref["audio"])
        n = len(jpegs) * 8000 // 30
        assert np.array_equal(r.audio(), wave[:n] if audio_format == "f32" else V.pcm16(wave[:n]))


def test_avi_reader_refuses_what_it_does_not_read(tmp_path):
    from livespeechportraits_amd import video as V
    _, files, _ = K.fixtures()
    path = str(tmp_path / "clip.avi")
    V.write_avi(path, [files[K.find("_420_16x16_")]] * 2, None)
    good = open(path, "rb").read()
    for what, data in (("not RIFF", b"JUNK" + good[4:]), ("truncated", good[:-20]), ("another codec", good.replace(b"MJPG", b"DIVX")),
                       ("no index", good[:good.rindex(b"idx1")] ), ("an index entry that points elsewhere", good[:-8] + struct.pack("<II", 999999, 5))):
        p = str(tmp_path / "bad.avi")
        with open(p, "wb") as f:
            f.write(data)
        with pytest.raises(V.AviError):
            V.AviReader(p)


# ---- candidates ----------------------------------------------------------------------------------------------------------------------------
def test_the_normalisation_table_is_the_formula_for_all_256_values():
    """albumentations' ToTensor(normalize=...) is img / 255.0 (float64 -> float32 tensor) then (t - mean) / std in float32; albumentations is
    not installed, so the table is pinned on that formula: parity-unpinned against albumentations"""
    from livespeechportraits_amd.candidates import candidate_paths, normalisation_table
    t = normalisation_table()
    assert t.dtype == np.float32 and t.shape == (256,)
    for v in range(256):
        want = (np.float32(np.float64(v) / 255.0) - np.float32(0.5)) / np.float32(0.5)
        assert t[v] == want and type(want) is np.float32, v
    assert t[0] == -1.0 and t[255] == 1.0
    assert candidate_paths("/data/May") == ["/data/May/candidates/normalized_full_%d.jpg" % j for j in range(4)]
