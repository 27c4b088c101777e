"""The resampler without a device: the numpy restatement of Pillow's Resample.c (tests/resize_model.py) against Pillow's frozen pixels and live
Pillow, the library's host planner (include/lspresize.h lsprsz_plan) against the model integer for integer and against Pillow's pixels, the
sanitizer-built planner (csrc/resize_check.cpp), what is refused, and that the new arguments are off by default."""
import json
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import resize_model as M
from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "livespeechportraits_amd", "csrc")
CASES = M.cases()
# (in_w, in_h, out_w, out_h) the planner is held to: the geometry list, and the long axes
PLAN_GEOMS = [(g[1], g[0], g[3], g[2]) for g in M.GEOMETRIES] + [(8192, 8192, 3, 4096), (8192, 1, 1, 8192), (8192, 8192, 8191, 1)]


@pytest.fixture(scope="module")
def fixtures():
    meta = json.load(open(os.path.join(GOLDEN, "resize.json")))
    whole = {k: v for k, v in np.load(os.path.join(GOLDEN, "resize.npz")).items() if not k.startswith("candidate_")}
    assert [c["name"] for c in meta["cases"]] == [c["name"] for c in CASES], "tests/golden/resize.json is not of this case list: run tools/make_golden_resize.py"
    assert 40 <= len(whole) < len(CASES)
    return meta["cases"], whole


def _agrees(got, case, whole):
    if case["name"] in whole:
        assert np.array_equal(got, whole[case["name"]]), case["name"]
    assert M.sha256(got) == case["sha256"], case["name"]


def test_the_model_gives_pillows_pixels_on_every_fixture(fixtures):
    frozen, whole = fixtures
    for case in frozen:
        _agrees(np.stack([M.resize(im, (case["out_w"], case["out_h"]), case["filter"]) for im in M.batch_of(case)]), case, whole)


def test_the_model_gives_live_pillows_pixels():
    """a fresh Pillow run over the geometry list x {L, RGB} x the five filters (image 0 of every batch); without Pillow the fixtures stand in"""
    Image = pytest.importorskip("PIL.Image")
    for case in CASES:
        img = M.batch_of(case)[0]
        want = np.asarray(Image.fromarray(img).resize((case["out_w"], case["out_h"]), getattr(Image.Resampling, case["filter"].upper())))
        assert np.array_equal(M.resize(img, (case["out_w"], case["out_h"]), case["filter"]), want), case["name"]


@pytest.fixture(scope="module")
def plans():
    from livespeechportraits_amd.resize import ResizePlan
    return {(g, f): ResizePlan(g[:2], g[2:], f) for g in PLAN_GEOMS for f in M.FILTERS}


def test_the_planner_equals_the_model_integer_for_integer(plans):
    for (g, filt), plan in plans.items():
        iw, ih, ow, oh = g
        for axis, (n_in, n_out) in enumerate(((iw, ow), (ih, oh))):
            got = plan.axis(axis)
            if n_in == n_out:
                assert got is None, (g, filt, axis)
                continue
            ksize, bounds, kk = M.coefficients(n_in, n_out, filt)
            assert got[1].shape == (n_out, ksize) and np.array_equal(got[0], bounds) and np.array_equal(got[1], kk), (g, filt, axis)
        info = plan.info
        if ih != oh:
            _, vb, _ = M.coefficients(ih, oh, filt)
            assert (info.row0, info.rows) == (vb[0, 0], vb[-1, 0] + vb[-1, 1] - vb[0, 0]), (g, filt)
        else:
            assert (info.row0, info.rows) == (0, ih)
        assert plan.launches == (2 if iw != ow and ih != oh else 1) and plan.bytes <= 4 << 20


def test_the_longest_axes_are_planned_not_refused_and_the_switch_over_rule_holds(plans):
    """8192 -> 1 LANCZOS has 49153 taps: planned, on the general path; the rule of include/lspresize.h for every plan"""
    from livespeechportraits_amd.resize import ResizePlan
    p = ResizePlan((8192, 8192), (1, 1), "lanczos")
    assert p.info.ksize_h == p.info.ksize_v == 49153 and p.paths == ("general", "general") and p.bytes < 1 << 20
    assert int(np.abs(p.axis(0)[1].astype(np.int64)).sum()) * 255 < 2 ** 31
    for (g, filt), plan in plans.items():
        i = plan.info
        if i.need_h:
            hb = plan.axis(0)[0].astype(np.int64)
            span = max(int((hb[x0:x0 + 64, 0] + hb[x0:x0 + 64, 1]).max() - hb[x0:x0 + 64, 0].min()) for x0 in range(0, g[2], 64))
            lds = 64 * (i.ksize_h + 2) * 4 + 8 * ((3 * span + 6) // 4 * 4 + 4)
            assert plan.paths[0] == ("tile" if lds <= 48 * 1024 else "general") and i.lds_h == (lds if lds <= 48 * 1024 else 0), (g, filt)
        else:
            assert plan.paths[0] is None
        if i.need_v:
            lds = 8 * (i.ksize_v + 2) * 4
            assert plan.paths[1] == ("tile" if lds <= 48 * 1024 else "general") and i.lds_v == (lds if lds <= 48 * 1024 else 0), (g, filt)
    assert {p.paths for p in plans.values()} >= {("tile", "tile"), ("general", "general"), ("general", "tile"), ("tile", None), (None, "tile")}


def test_the_planners_coefficients_give_pillows_pixels_on_every_fixture(fixtures, plans):
    """the host core pinned on Pillow, not on the model alone: numpy runs the two integer passes with the LIBRARY's coefficients"""
    frozen, whole = fixtures
    for case in frozen:
        plan = plans[((case["w"], case["h"], case["out_w"], case["out_h"]), case["filter"])]
        axes = (plan.axis(0), plan.axis(1))
        _agrees(np.stack([M.resize_with(im, axes) for im in M.batch_of(case)]), case, whole)


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


def test_the_sanitizer_built_planner_runs_clean_and_agrees(tmp_path, plans):
    """csrc/resize_check.cpp (resize_core.h as host code under ASan + UBSan, with its own main) over the same list, the longest axes and the
    refused geometries, on stdin: one digest per plan, equal to the digest of the model's coefficients and to the library's paths"""
    why = _sanitizer_works(tmp_path)
    if why:
        pytest.skip(why)
    subprocess.run(["make", "-C", CSRC, "-s", "check-resize"], check=True)
    exe = os.path.join(CSRC, "build", "resize_check")
    jobs = [(g, f) for g in PLAN_GEOMS + [(8192, 8192, 1, 1)] for f in range(5)]
    refused = [((0, 5, 5, 5), 3), ((5, 5, 5, 0), 3), ((8193, 5, 5, 5), 3), ((5, 5, 5, 8193), 1), ((5, 5, 4, 4), 5), ((5, 5, 4, 4), -1), ((-3, 5, 4, 4), 0)]
    text = "\n".join("%d %d %d %d %d" % (g + (f,)) for g, f in jobs + refused) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(jobs) + len(refused)
    paths = {None: 0, "tile": 1, "general": 2}
    for (g, f), line in zip(jobs, lines):
        words = line.split()
        assert words[:6] == [str(v) for v in g + (f,)] + ["ok"], line
        filt = M.FILTERS[f]
        axes = [(n_in, n_out) for n_in, n_out in ((g[0], g[2]), (g[1], g[3])) if n_in != n_out]
        assert int(words[7], 16) == M.digest([M.coefficients(n_in, n_out, filt) for n_in, n_out in axes]), line
        if (g, filt) in plans:
            p = plans[(g, filt)]
            assert [int(w) for w in words[8:12]] == [paths[p.paths[0]], paths[p.paths[1]], p.info.row0, p.info.rows] and int(words[6]) == p.bytes, line
    for line in lines[len(jobs):]:
        assert line.split()[5] == "refused", line


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _hostless_resizer():
    """a Resizer whose argument checks can run without a device: every refusal below is raised before anything is enqueued"""
    from livespeechportraits_amd.resize import Resizer
    r = Resizer.__new__(Resizer)
    r.device, r.max_batch = torch.device("cpu"), 8
    return r


@pytest.mark.parametrize("kwargs, words", [
    ({"resample": "nearest"}, "NEAREST"), ({"resample": 0}, "NEAREST"), ({"resample": "area"}, "not offered"),
    ({"box": (0, 0, 4, 4)}, "box="), ({"reducing_gap": 2.0}, "reducing_gap"),
    ({"size": 0}, "side of 0"), ({"size": (16, 0)}, "side of 0"), ({"size": 8193}, "above 8192"), ({"size": (8, 8, 8)}, "(width, height)"),
    ({"images": torch.zeros((2, 8, 8, 2), dtype=torch.uint8)}, "2 channels"), ({"images": torch.zeros((2, 8, 8, 4), dtype=torch.uint8)}, "4 channels"),
    ({"images": torch.zeros((8, 8, 4), dtype=torch.uint8), "channels": 3}, "4 channels"), ({"channels": 2}, "2 channels"), ({"images": torch.zeros((2, 8, 8, 3), dtype=torch.float32)}, "uint8"),
    ({"images": torch.zeros((2, 0, 8, 3), dtype=torch.uint8)}, "side of 0"), ({"images": torch.zeros((9, 8, 8, 3), dtype=torch.uint8)}, "max_batch"),
    ({"images": torch.zeros((2, 8, 16, 3), dtype=torch.uint8)[:, :, ::2]}, "contiguous"), ({"images": np.zeros((2, 8, 8, 3), np.uint8)}, "torch tensor"),
])
def test_what_is_not_offered_is_refused_with_its_reason(kwargs, words):
    kw = dict(kwargs)
    images, size = kw.pop("images", torch.zeros((2, 8, 8, 3), dtype=torch.uint8)), kw.pop("size", 4)
    with pytest.raises(ValueError, match=words.replace("(", r"\(").replace(")", r"\)")):
        _hostless_resizer().resize(images, size, **kw)


def test_the_planner_and_the_device_class_refuse_cleanly():
    from livespeechportraits_amd import _native as N
    from livespeechportraits_amd.resize import ResizePlan, Resizer
    lib = N.load()
    for geom, code in (((5, 5, 4, 4, 5), -1), ((5, 5, 4, 4, -1), -1), ((0, 5, 4, 4, 3), -1), ((5, 8193, 4, 4, 3), -1), ((5, 5, 4, 8193, 3), -1)):
        assert lib.lsprsz_plan(*geom, None, 0) == code and lib.lsprsz_last_error()
    need = lib.lsprsz_plan(5, 5, 4, 4, 3, None, 0)
    buf = np.zeros(need + 32, np.uint8)
    at = (-buf.ctypes.data) % 16
    assert lib.lsprsz_plan(5, 5, 4, 4, 3, buf.ctypes.data + at, need - 1) == -1            # a cap below the need
    assert lib.lsprsz_plan(5, 5, 4, 4, 3, buf.ctypes.data + at + 4, need) == -1           # an unaligned block
    assert lib.lsprsz_plan(5, 5, 4, 4, 3, buf.ctypes.data + at, need) == need
    assert lib.lsprsz_workspace_bytes(buf.ctypes.data + at, 2, 2) == -1 and lib.lsprsz_workspace_bytes(buf.ctypes.data + at, 2, 3) == 2 * 5 * 16
    assert lib.lsprsz_plan_info(buf.ctypes.data + at + 16, N.RszInfo()) == -1              # not a plan block
    with pytest.raises(ValueError, match="8192"):
        ResizePlan((8193, 5), (4, 4))
    with pytest.raises(ValueError, match="NEAREST"):
        ResizePlan((8, 8), (4, 4), "nearest")
    with pytest.raises(RuntimeError, match="no CPU path"):
        Resizer("cpu")


# ---- defaults are off -------------------------------------------------------------------------------------------------------------------
class _Constructed(Exception):
    pass


@pytest.fixture
def no_resizer(monkeypatch):
    """constructing a Resizer is an error for the length of the test"""
    from livespeechportraits_amd import resize

    def refuse(*a, **k):
        raise _Constructed("a Resizer was constructed")
    monkeypatch.setattr(resize, "Resizer", refuse)


class _HostModel:
    def inference_image(self, maps, cand):
        return torch.full((maps.shape[0], 16, 16, 3), 9, dtype=torch.uint8)


def test_render_frames_leaves_the_resampler_alone_by_default(no_resizer):
    from livespeechportraits_amd.render_loop import render_frames, render_frames_from_landmarks
    maps = [torch.zeros((1, 16, 16)) for _ in range(3)]
    frames = render_frames(_HostModel(), maps, torch.zeros((1, 12, 16, 16)), batch=2)
    assert len(frames) == 3 and frames[0].shape == (16, 16, 3)
    for fn, args in ((render_frames, (_HostModel(), maps, torch.zeros((1, 12, 16, 16)))), (render_frames_from_landmarks, (_HostModel(), [], [], torch.zeros((1, 12, 16, 16))))):
        with pytest.raises(ValueError, match="device only"):
            fn(*args, out_size=8)                                  # a model on the host: refused before anything runs
        with pytest.raises(ValueError, match="NEAREST"):
            fn(*args, out_size=8, resample="nearest")
        with pytest.raises(ValueError, match="above 8192"):
            fn(*args, out_size=(8, 9000))


def test_load_candidates_refuses_a_wrong_sized_file_as_ever_by_default(no_resizer):
    import jpeg_decode_cases as K
    from livespeechportraits_amd.candidates import load_candidates
    _, files, _ = K.fixtures()
    small = files[K.find("_420_9x3_")]
    with pytest.raises(ValueError, match="candidate 0 is 3x9 with 3 components, the generator takes 512x512 RGB"):
        load_candidates([small] * 4, device="cpu")
    with pytest.raises(ValueError, match="NEAREST"):
        load_candidates([small] * 4, device="cpu", resize="nearest")
    grey = files[K.find("_grey_16x16_")]
    with pytest.raises(ValueError, match="candidate 1 is 16x16 with 1 components"):
        load_candidates([small, grey, small, small], device="cpu", resize="bicubic")     # a grey file is not a candidate at any size


def _pool_parts(monkeypatch):
    from livespeechportraits_amd import feature_map
    monkeypatch.setattr(feature_map, "FeatureMapRasteriser", lambda *a, **k: object())
    cpu = torch.device("cpu")
    audio = types.SimpleNamespace(device=cpu, max_sessions=2, ff_mouth=18, ff_head=18)
    stage = types.SimpleNamespace(device=cpu, max_sessions=2, max_push=64, future=(5, 3, 3), radii=(10, 6, 6))
    cand = types.SimpleNamespace(device=types.SimpleNamespace(type="cuda", index=None))
    return audio, stage, object(), cand


def test_the_live_pool_leaves_the_resampler_alone_by_default(no_resizer, monkeypatch):
    from livespeechportraits_amd.live_render import LivePortraitPool
    from livespeechportraits_amd.video import AviWriter
    parts = _pool_parts(monkeypatch)
    pool = LivePortraitPool(*parts, load_size=64, max_batch=4, raster_chunk=1)
    assert pool.out_size is None and pool._resizer is None and (pool.frame_width, pool.frame_height) == (64, 64)
    with pytest.raises(_Constructed):                              # the hook is on the path: with out_size the pool makes its Resizer
        LivePortraitPool(*parts, load_size=64, max_batch=4, raster_chunk=1, out_size=32)
    for bad, words in ((0, "side of 0"), ((32, 9000), "above 8192")):
        with pytest.raises(ValueError, match=words):
            LivePortraitPool(*parts, load_size=64, max_batch=4, raster_chunk=1, out_size=bad)
    with pytest.raises(ValueError, match="NEAREST"):
        LivePortraitPool(*parts, load_size=64, max_batch=4, raster_chunk=1, out_size=32, resample="nearest")


def test_the_live_pool_holds_video_writers_to_out_size(monkeypatch, tmp_path):
    """_check_writer: ``video`` is compared with out_size, ``video_input`` (the edge maps) with load_size"""
    from livespeechportraits_amd import resize
    from livespeechportraits_amd.live_render import LivePortraitPool
    from livespeechportraits_amd.video import AviWriter
    monkeypatch.setattr(resize, "Resizer", lambda *a, **k: object())
    pool = LivePortraitPool(*_pool_parts(monkeypatch), load_size=64, max_batch=4, raster_chunk=1, out_size=(48, 32))
    assert (pool.frame_width, pool.frame_height) == (48, 32)

    def writer(name, w, h, ch):
        return AviWriter(str(tmp_path / name), w, h, fps=60, channels=ch, audio_rate=None)
    ok, full, grey, small_grey = writer("a.avi", 48, 32, 3), writer("b.avi", 64, 64, 3), writer("c.avi", 64, 64, 1), writer("d.avi", 48, 32, 1)
    try:
        pool._check_writer(ok, "video")
        pool._check_writer(grey, "video_input")
        with pytest.raises(ValueError, match="video must be an AviWriter of 48x32"):
            pool._check_writer(full, "video")
        with pytest.raises(ValueError, match="video_input must be an AviWriter of 64x64"):
            pool._check_writer(small_grey, "video_input")
    finally:
        for w in (ok, full, grey, small_grey):
            w.close()
