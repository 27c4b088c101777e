"""Progressive JPEG (LSPJPEG_DEC_FLAG_PROGRESSIVE) without a device: the numpy restatement (tests/jpeg_progressive_model.py) against Pillow's
pixels and against the baseline twins' coefficients, the library's host half (probe, planner, scan list, stage 1 run on the host) against the
restatement, every new refusal, truncations and corruptions, and the sanitizer-built stand-alone checker over the flagged bundle kind.  The
device half is tests/test_gpu_jpeg_progressive.py.  Every test here fails on the parent commit, where the flag does not exist."""
import hashlib
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_decode_cases as K
import jpeg_decode_model as D
import jpeg_model as M
import jpeg_progressive_cases as KP
import jpeg_progressive_model as P
from conftest import ROOT
from test_jpeg_decode_cpu import _pil_pixels, _pillow, _sanitizer_works

CSRC = os.path.join(ROOT, "livespeechportraits_amd", "csrc")


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_the_model_gives_pillows_pixels_and_the_twins_coefficients_on_every_small_fixture():
    """pixels: Pillow's, frozen.  Coefficients: the baseline twin's from the existing model, padding blocks outside a component's extent
    included (libjpeg's edge rule gives the encoder the same padding in both files)"""
    meta, files, twins, pixels = KP.fixtures()
    assert len(meta["cases"]) == 19 * 8
    for n in KP.small_names():
        f = P.parse(files[n])
        coef = P.coefficients(files[n], f)
        got = D.pixels_from(coef, P.as_baseline(f))
        assert got.dtype == np.uint8 and got.shape == pixels[n].shape and np.array_equal(got, pixels[n]), n
        assert np.array_equal(coef, D.coefficients(twins[n])), n
        assert D.status_of(files[n]) == D.UNSUPPORTED, n                    # the existing model still refuses SOF2


def test_the_model_gives_pillows_pixels_on_the_512_frames():
    meta = KP.fixtures()[0]
    files, twins = KP.frames_512()
    assert [c["name"] for c in meta["frames"]] == ["constant_512"] + ["candidate_%d_512_q95_prog" % j for j in range(4)]
    for c in meta["frames"]:
        f = P.parse(files[c["name"]])
        coef = P.coefficients(files[c["name"]], f)
        got = D.pixels_from(coef, P.as_baseline(f))
        assert list(got.shape) == c["shape"] and hashlib.sha256(got.tobytes()).hexdigest() == c["pixels_sha256"], c["name"]
        assert np.array_equal(coef, D.coefficients(twins[c["name"]])), c["name"]
    assert len(files["constant_512"]) < 2500                               # tables, and end-of-band runs of thousands of blocks
    assert max(s["units"] for s in P.parse(files["constant_512"])["scans"]) == 4096


def test_the_model_gives_pillows_pixels_on_a_fresh_pillow_run():
    Image = _pillow()
    if Image is None:
        pytest.skip("Pillow is not installed: the frozen fixtures stand in for it")
    n = 0
    for k, (h, w) in enumerate(((1, 1), (2, 3), (3, 4), (31, 18), (24, 56), (9, 2), (17, 33))):
        for ch, kw in ((3, {}), (3, {"subsampling": 0}), (3, {"subsampling": 1}), (3, {"optimize": True}), (3, {"restart_marker_blocks": 2}),
                       (3, {"restart_marker_rows": 1, "subsampling": 1}), (1, {}), (1, {"restart_marker_blocks": 1})):
            img = M.make_image({"kind": ("noise", "extremes", "smooth")[(k + n) % 3] if ch == 3 else "noise", "h": h, "w": w, "channels": ch, "seed": 70 + n})
            b, t = io.BytesIO(), io.BytesIO()
            Image.fromarray(img).save(b, "JPEG", quality=(1, 30, 75, 95, 100)[n % 5], progressive=True, **kw)
            Image.fromarray(img).save(t, "JPEG", quality=(1, 30, 75, 95, 100)[n % 5], **kw)
            assert np.array_equal(P.decode(b.getvalue()), np.asarray(Image.open(io.BytesIO(b.getvalue())))), (h, w, ch, kw)
            assert np.array_equal(P.coefficients(b.getvalue()), D.coefficients(t.getvalue())), (h, w, ch, kw)
            n += 1


# ---- the library's host half ------------------------------------------------------------------------------------------------------------
def _check_file(J, plan, i, name, data):
    """probe, the planner's record, the scan list with intervals and offsets, and stage 1 on the host against the model"""
    f = P.parse(data)
    hs, vs = f["comps"][0][1], f["comps"][0][2]
    nseg = sum(len(s["segments"]) for s in f["scans"])
    want = (0, f["width"], f["height"], len(f["comps"]), hs, vs, f["restart"], f["mcux"] * f["mcuy"], nseg)
    info = J.probe(data, progressive=True)
    assert tuple(info[:9]) == want and info.default_tables == 0, name
    assert (info.scan_offset, info.scan_bytes) == (f["data_begin"], f["data_end"] - f["data_begin"]), name
    planned = plan.file(i)
    assert tuple(planned[:9]) == want and planned.scan_bytes == info.scan_bytes, name
    at = planned.scan_offset - f["data_begin"]                             # file offset -> offset inside the block
    assert bytes(plan.blob[planned.scan_offset:planned.scan_offset + info.scan_bytes]) == data[f["data_begin"]:f["data_end"]], name
    for c in range(len(f["comps"])):
        assert np.array_equal(plan.qtable(i, c), f["q"][f["comps"][c][3]]), (name, c)
    scans = plan.scans(i)
    assert len(scans) == len(f["scans"]), name
    for got, s in zip(scans, f["scans"]):
        assert got == J.JpegScan(tuple(s["comps"]), tuple(s["td"]), tuple(s["ta"]), s["ss"], s["se"], s["ah"], s["al"], s["restart"], s["units"], len(s["segments"]),
                                 s["begin"] + at, s["end"] + at), (name, got)
    status, coef = plan.host_coefficients(i)
    assert status == 0 and np.array_equal(coef, P.coefficients(data, f)), name


def test_probe_planner_and_host_coefficients_agree_with_the_model():
    """all progressive fixtures and the existing baseline small fixtures planned as ONE batch, interleaved"""
    from livespeechportraits_amd import jpeg as J
    _, files, _, _ = KP.fixtures()
    _, base, _ = K.fixtures()
    pn, bn = KP.small_names(), K.small_names()
    order = []
    for k in range(max(len(pn), len(bn))):
        order += [("p", n) for n in pn[k:k + 1]] + [("b", n) for n in bn[k:k + 1]]
    order.append(("p", "constant_512"))
    big = KP.frames_512()[0]
    data = [files[n] if n in files else big[n] if kind == "p" else base[n] for kind, n in order]
    plan = J.DecodePlan(data, progressive=True)
    assert plan.summary.files == len(order) and plan.statuses() == [0] * len(order)
    seg = 0
    for i, (kind, n) in enumerate(order):
        if kind == "p":
            _check_file(J, plan, i, n, data[i])
            continue
        f = D.parse(data[i])                                               # a baseline file beside them: as without the flag
        assert plan.scans(i) == [] and J.probe(data[i], progressive=True) == J.probe(data[i]), n
        for begin, end, mcu0, nmcu in f["segments"]:
            got = plan.segment(seg)
            assert got[:3] == (i, mcu0, nmcu) and got[4] - got[3] == end - begin, (n, seg)
            seg += 1
        status, coef = plan.host_coefficients(i)
        assert status == 0 and np.array_equal(coef, D.coefficients(data[i], f)), n
    assert seg == plan.summary.segments                                    # the progressive files' intervals are not in the baseline list


def test_a_512_candidate_through_the_host_half():
    from livespeechportraits_amd import jpeg as J
    files, twins = KP.frames_512()
    name = "candidate_0_512_q95_prog"
    plan = J.DecodePlan([files[name], twins[name]], progressive=True)
    (sa, a), (sb, b) = plan.host_coefficients(0), plan.host_coefficients(1)
    assert sa == 0 and sb == 0 and np.array_equal(a, b)                    # the progressive file holds its baseline twin's coefficients
    assert len(plan.scans(0)) == 10 and plan.scans(1) == []


def test_without_the_flag_the_same_files_are_unsupported():
    from livespeechportraits_amd import jpeg as J
    _, files, _, _ = KP.fixtures()
    names = KP.small_names()
    data = [files[n] for n in names] + list(KP.frames_512()[0].values())
    plan = J.DecodePlan(data)
    assert plan.statuses() == [J.UNSUPPORTED] * len(data) and plan.summary.segments == 0 and plan.summary.total_blocks == 0
    for d in data[::7]:
        assert J.probe(d).status == J.UNSUPPORTED and J.probe(d, progressive=False).status == J.UNSUPPORTED
    assert all(plan.scans(i) == [] and plan.host_coefficients(i) == (J.UNSUPPORTED, None) for i in range(0, len(data), 7))


@pytest.mark.parametrize("k", range(10))
def test_every_new_refusal_returns_its_code(k):
    from livespeechportraits_amd import jpeg as J
    cases = KP.refusals()
    assert len(cases) == 10
    what, data, want = cases[k]
    model, coef, f = P.stage1(data)
    assert model == want, "%s: the model says %d" % (what, model)
    plan = J.DecodePlan([data], progressive=True)
    status, got = plan.host_coefficients(0)
    assert status == want, "%s: the library says %d" % (what, status)
    if want == D.UNSUPPORTED or plan.statuses()[0]:
        assert J.probe(data, progressive=True).status == want, what
    assert J.DecodePlan([data]).statuses() == [J.UNSUPPORTED], what        # without the flag the parser stops at the SOF2 marker (or at SOF0's first SOS)
    if want == 0:                                                          # the control: the pixels of the file it was made from
        assert np.array_equal(got, coef)
        assert np.array_equal(D.pixels_from(coef, f), KP.fixtures()[3][KP.find("_420_plain_40x72_")])
        ref = _pil_pixels(data) if _pillow() else None
        assert ref is None or np.array_equal(ref, D.pixels_from(coef, f))


def _changed(files, names):
    """every truncation of three files, and single-byte changes at a fixed seed"""
    rng = np.random.default_rng(20261020)
    for n in names[:3]:
        for length in range(len(files[n])):
            yield n, files[n][:length]
    for n in names:
        for _ in range(25):
            b = bytearray(files[n])
            b[int(rng.integers(len(b)))] ^= int(rng.integers(1, 256))
            yield n, bytes(b)


CHANGED = ("_420_plain_2x3_", "_grey_rstb1_9x2_", "_420_rstr_opt_1x1_", "_422_rstb3_17x33_", "_420_plain_opt_31x18_", "_444_rstr_8x24_", "_grey_plain_40x72_",
           "_420_rstb3_opt_17x33_")


def test_truncations_and_corruptions_give_an_error_or_pillows_pixels():
    """A changed file is refused, or it decodes to what Pillow returns for it: the library's status and coefficients equal the model's, and
    the model's pixels equal Pillow's wherever both decode.  Nothing crashes."""
    from livespeechportraits_amd import jpeg as J
    _, files, _, _ = KP.fixtures()
    names = [KP.find(p) for p in CHANGED]
    counts = {"refused": 0, "decoded": 0, "pillow agrees": 0, "pillow refuses": 0}
    batch = list(_changed(files, names))
    for at in range(0, len(batch), 64):
        part = batch[at:at + 64]
        plan = J.DecodePlan([d for _, d in part], progressive=True)
        for i, (n, data) in enumerate(part):
            status, coef = plan.host_coefficients(i)
            want, wcoef, f = P.stage1(data)
            assert status == want and (want != 0 or np.array_equal(coef, wcoef)), (n, len(data), status, want)
            if want:
                counts["refused"] += 1
                continue
            try:
                px = D.pixels_from(wcoef, f)
            except D.Refused as e:
                assert e.status == D.RANGE
                counts["refused"] += 1
                continue
            counts["decoded"] += 1
            ref = _pil_pixels(data) if _pillow() else None
            if ref is not None:
                assert ref.shape == px.shape and np.array_equal(ref, px), "%s changed: decoded, but not to Pillow's pixels" % n
                counts["pillow agrees"] += 1
            elif _pillow():
                counts["pillow refuses"] += 1
    print(counts)
    assert counts["refused"] > 0 and counts["decoded"] > 0
    assert _pillow() is None or counts["pillow agrees"] > 0


def test_the_sanitizer_built_checker_runs_clean_over_the_flagged_bundle(tmp_path):
    """csrc/jpegdec_check.cpp (host code under ASan + UBSan, with its own main) over a bundle of the flagged kind ("LSDP": every entry is planned
    with LSPJPEG_DEC_FLAG_PROGRESSIVE): progressive fixtures of every geometry and restart option beside baseline ones, the constant 512^2 frame,
    the new refusals; every truncation of three files and 40 single-byte changes of each."""
    why = _sanitizer_works(tmp_path)
    if why:
        pytest.skip(why)
    subprocess.run(["make", "-C", CSRC, "-s", "check-jpegdec"], check=True)
    exe = os.path.join(CSRC, "build", "jpegdec_check")
    _, files, _, _ = KP.fixtures()
    _, base, _ = K.fixtures()
    entries = [files[KP.find(p)] for p in CHANGED[:3]]
    entries += [files[n] for n in KP.small_names()[::3]] + [base[n] for n in K.small_names()[::9]] + [KP.frames_512()[0]["constant_512"]]
    entries += [d for _, d, _ in KP.refusals()]
    bundle = bytearray(b"LSDP" + struct.pack("<I", len(entries)))
    for data in entries:
        status, coef, _ = P.stage1(data)
        coef = np.zeros(0, np.int16) if coef is None else np.ascontiguousarray(coef, "<i2").reshape(-1)
        bundle += struct.pack("<III", len(data), status, coef.size) + data + coef.tobytes()
    path = tmp_path / "bundle.bin"
    path.write_bytes(bytes(bundle))
    r = subprocess.run([str(exe), str(path), "20261020", "3", "40"], capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "0 failures" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
