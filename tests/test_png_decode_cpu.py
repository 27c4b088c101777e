"""The PNG decoder without a device: the Python restatement (its own inflate) against Pillow's pixels, the library's host half (probe, planner, the
three stages run on the host with the kernels' code) against the restatement, every refusal, raw and re-sealed changes, the sanitizer-built
stand-alone checker, and load_candidates' unchanged refusals.  The device half is tests/test_gpu_png_decode.py."""
import io
import os
import shutil
import struct
import subprocess
import warnings

import numpy as np
import pytest

import png_decode_cases as K
import png_decode_model as D
from conftest import ROOT

CSRC = os.path.join(ROOT, "livespeechportraits_amd", "csrc")
SEED = 20261021
# the files whose changes are tried: every block kind, palette and alpha files among them; all small, so that the model's inflate stays quick
CHANGED = ("rgb_31x17_l6", "rgb_31x17_fixed", "rgb_31x17_stored", "rgb_31x17_mixed", "p4_3x11", "ga_21x67", "grey_200x5_overlaps", "grey_40x6_single_distance")
TRUNCATED = ("rgb_1x1", "p1_13x9", "grey_20x20")


def _pillow():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


def _pil_pixels(data, components):
    """Pillow's pixels, or None when it does not open the file"""
    Image = _pillow()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return np.asarray(Image.open(io.BytesIO(data)).convert("RGB" if components == 3 else "L"))
    except Exception:
        return None


def _model(data):
    """(status, filtered scanlines or None, pixels or None) of the model"""
    try:
        f, raw = D.scanlines(data)
        return 0, raw, D.pixels(f, D.unfilter(f, raw))
    except D.Refused as e:
        return e.status, None, None


def _library(plan, i):
    """(status after all three stages, scanlines, pixels) of the library's host half"""
    st, lines = plan.host_scanlines(i)
    if st:
        return st, None, None
    st, px = plan.host_pixels(i)
    return (st, None, None) if st else (0, lines.tobytes(), px)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_the_model_gives_pillows_pixels_on_every_fixture():
    meta, files, pixels = K.fixtures()
    assert len(meta["cases"]) >= 30 and {(c["color_type"], c["depth"]) for c in meta["cases"]} == {(2, 8), (6, 8), (0, 8), (4, 8), (3, 1), (3, 2), (3, 4), (3, 8)}
    for name in K.small_names():
        got = D.decode(files[name])
        assert got.dtype == np.uint8 and got.shape == pixels[name].shape and np.array_equal(got, pixels[name]), name
    assert len(K.candidate_pixels()) == 4                        # hashes them against what Pillow returned when they were written


def test_the_model_gives_pillows_pixels_on_a_fresh_pillow_save():
    Image = _pillow()
    if Image is None:
        pytest.skip("Pillow is not installed: the frozen fixtures stand in for it")
    rng = np.random.default_rng(7)
    for mode, shape in (("RGB", (23, 31, 3)), ("RGBA", (9, 70, 4)), ("L", (66, 5)), ("LA", (12, 12, 2)), ("P", (20, 33)), ("1", (11, 13))):
        for kw in ({}, {"optimize": True}, {"compress_level": 1}):
            img = rng.integers(0, 256, shape).astype(np.uint8)
            if mode == "1":
                im = Image.fromarray(img > 127).convert("P")     # a palette file of depth 1
            elif mode == "P":
                im = Image.fromarray(img % 37, "P")
                im.putpalette([int(v) for v in rng.integers(0, 256, 37 * 3)])
            else:
                im = Image.fromarray(img, mode)
            b = io.BytesIO()
            im.save(b, "PNG", **kw)
            data = b.getvalue()
            assert np.array_equal(D.decode(data), _pil_pixels(data, D.parse(data)["ncomp"])), (mode, kw)


# ---- the library's host half ------------------------------------------------------------------------------------------------------------
def test_probe_planner_and_host_twins_agree_with_the_model():
    """geometry, the IDAT payload's size, the filtered scanlines of stage 1 and the pixels of stages 2 and 3, for all small fixtures planned as ONE
    batch (files of every geometry side by side)"""
    from livespeechportraits_amd import png as P
    _, files, pixels = K.fixtures()
    names = K.small_names()
    plan = P.DecodePlan([files[n] for n in names])
    assert plan.summary.files == len(names) and plan.statuses() == [0] * len(names)
    for i, n in enumerate(names):
        f, raw = D.scanlines(files[n])
        want = (0, f["width"], f["height"], f["color_type"], f["depth"], f["ncomp"], len(f["idat"]), f["raw_bytes"])
        assert tuple(P.probe(files[n])) == want and tuple(plan.file(i)) == want, n
        st, lines = plan.host_scanlines(i)
        assert st == 0 and lines.shape == (f["height"], 1 + f["rowbytes"]) and lines.tobytes() == raw, n
        st, px = plan.host_pixels(i)
        assert st == 0 and px.shape == pixels[n].shape and np.array_equal(px, pixels[n]), n


def test_the_512_candidates_through_the_host_half():
    from livespeechportraits_amd import png as P
    plan = P.DecodePlan([data for _, data in K.candidates()])
    for i, (name, _) in enumerate(K.candidates()):
        st, px = plan.host_pixels(i)
        assert st == 0 and np.array_equal(px, K.candidate_pixels()[name]), name


@pytest.mark.parametrize("k", range(len(K.refusals())))
def test_every_refusal_returns_its_code(k):
    from livespeechportraits_amd import png as P
    what, data, want = K.refusals()[k]
    assert _model(data)[0] == want, "%s: the model says %d" % (what, _model(data)[0])
    plan = P.DecodePlan([data])
    status = plan.statuses()[0] or _library(plan, 0)[0]
    assert status == want, "%s: the library says %d" % (what, status)
    if plan.statuses()[0]:
        assert P.probe(data).status == want, what              # what the planner sees, probe reports
    else:
        assert P.probe(data).status == 0, what                 # found in the stream: by the code the kernels run


def test_what_stands_next_to_a_refusal_is_decoded():
    from livespeechportraits_amd import png as P
    for what, data in K.admitted():
        st, _, px = _model(data)
        got = _library(P.DecodePlan([data]), 0)
        assert st == 0 and got[0] == 0 and np.array_equal(got[2], px), what
        if _pillow():
            assert np.array_equal(px, _pil_pixels(data, 3)), what


def test_raw_truncations_and_changes_are_all_refused():
    """every truncation of three small files, and 40 seeded single-byte changes of each of eight: every byte of a PNG is under a CRC or is a length,
    so all of them are refused, by the library and by the model alike"""
    from livespeechportraits_amd import png as P
    _, files, _ = K.fixtures()
    rng = np.random.default_rng(SEED)
    batch = [files[n][:length] for n in TRUNCATED for length in range(len(files[n]))]
    for n in CHANGED:
        for _ in range(40):
            b = bytearray(files[n])
            b[int(rng.integers(len(b)))] ^= int(rng.integers(1, 256))
            batch.append(bytes(b))
    assert len(batch) > 8 * 40 + 300
    for at in range(0, len(batch), 64):
        part = batch[at:at + 64]
        plan = P.DecodePlan(part)
        for i, data in enumerate(part):
            status = plan.statuses()[0 + i] or _library(plan, i)[0]
            want = _model(data)[0]
            assert status == want and want != 0, (at + i, len(data), status, want)


def _resealed():
    _, files, _ = K.fixtures()
    rng = np.random.default_rng(SEED)
    return [(n, K.resealed(files[n], rng)) for n in CHANGED for _ in range(60)]


def test_resealed_changes_give_an_error_or_pillows_pixels():
    """One byte of the deflate body flipped, Adler-32 and CRCs made right again: the changes that reach the stream-level code.  The library's status
    equals the model's; where it is 0 the scanlines and the pixels are equal too, and the pixels are Pillow's wherever Pillow also decodes.  At
    least a fifth of the changed files must decode and at least a third must be refused, so neither side passes by doing nothing."""
    from livespeechportraits_amd import png as P
    counts = {"decoded": 0, "refused": 0, "pillow agrees": 0, "pillow decodes what is refused": 0}
    batch = _resealed()
    assert len(batch) == 480
    for at in range(0, len(batch), 64):
        part = batch[at:at + 64]
        plan = P.DecodePlan([d for _, d in part])
        for i, (n, data) in enumerate(part):
            want, wraw, wpx = _model(data)
            status, raw, px = _library(plan, i)
            assert status == want, (n, at + i, status, want)
            ref = _pil_pixels(data, D.parse(data)["ncomp"]) if _pillow() else None
            if want:
                counts["refused"] += 1
                counts["pillow decodes what is refused"] += ref is not None
                continue
            counts["decoded"] += 1
            assert raw == wraw and np.array_equal(px, wpx), (n, at + i)
            if ref is not None:
                assert ref.shape == px.shape and np.array_equal(ref, px), "%s changed: decoded, but not to Pillow's pixels" % n
                counts["pillow agrees"] += 1
    print(counts)
    assert counts["decoded"] >= 480 // 5 and counts["refused"] >= 480 // 3, counts


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
    """csrc/pngdec_check.cpp (the chunk walker, the planner and the three stages as host code under ASan + UBSan, with its own main) over all small
    fixtures, one 512 x 512 candidate, every refusal, the re-sealed changes, every truncation of three files and 40 single-byte changes of each
    small file that decodes."""
    why = _sanitizer_works(tmp_path)
    if why:
        pytest.skip(why)
    subprocess.run(["make", "-C", CSRC, "-s", "check-pngdec"], check=True)
    exe = os.path.join(CSRC, "build", "pngdec_check")
    _, files, _ = K.fixtures()
    entries = [files[n] for n in TRUNCATED] + [files[n] for n in K.small_names()] + [K.candidates()[3][1]]
    entries += [d for _, d, _ in K.refusals()] + [d for _, d in K.admitted()] + [d for _, d in _resealed()]
    bundle = bytearray(b"LSPB" + struct.pack("<I", len(entries)))
    for data in entries:
        status, raw, _ = _model(data)
        raw = raw if status == 0 else b""
        bundle += struct.pack("<III", len(data), status, len(raw)) + data + raw
    path = tmp_path / "bundle.bin"
    path.write_bytes(bytes(bundle))
    r = subprocess.run([str(exe), str(path), str(SEED), "3", "40"], capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "0 failures" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr


# ---- candidates ----------------------------------------------------------------------------------------------------------------------------
def test_load_candidates_without_png_refuses_what_it_refused():
    """png=False is the default and every line of the earlier behaviour: a PNG file is CORRUPT to jpeg.probe and goes where a broken JPEG goes; the
    checks in front of the decoder are the same for both settings"""
    from livespeechportraits_amd import jpeg as J
    from livespeechportraits_amd.candidates import load_candidates
    pngs = [data for _, data in K.candidates()]
    assert all(J.probe(d).status == J.CORRUPT for d in pngs)
    for kw in ({}, {"png": False}, {"png": True}):
        with pytest.raises(ValueError, match="3 candidate images"):
            load_candidates(pngs[:3], device="cpu", **kw)
    for kw in ({}, {"png": False}):
        with pytest.raises(RuntimeError, match="JPEG decoder runs on the MI355X only"):
            load_candidates(pngs, device="cpu", **kw)
    with pytest.raises(RuntimeError, match="PNG decoder runs on the MI355X only"):
        load_candidates(pngs, device="cpu", png=True)
    small = K.fixtures()[1]["rgb_64x64"]
    with pytest.raises(ValueError, match="candidate 1 is 64x64 with 3 components"):
        load_candidates([pngs[0], small, pngs[2], pngs[3]], device="cpu", png=True)
    grey = K.fixtures()[1]["grey_20x20"]
    with pytest.raises(ValueError, match="with 1 components"):
        load_candidates([pngs[0], grey, pngs[2], pngs[3]], device="cpu", png=True, resize="bicubic")
    with pytest.raises(ValueError):
        load_candidates(pngs, device="cpu", png=True, resize="nearest")
