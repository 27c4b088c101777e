"""The device JPEG encoder's contract on the host (no GPU): tests/jpeg_model.py restates the file Pillow writes with
`Image.fromarray(img).save(f, "JPEG", quality=q)` (demo.py:271 -> util/util.py:70-72) step by step, and must give Pillow's bytes;
the library's host-built header (lspjpeg_header) must be the prefix of those files up to the end of SOS.

Pillow's bytes are frozen in tests/golden/jpeg_pil.{json,npz} by tools/make_golden_jpeg.py (whole files for small images,
length + sha256 for frames of 512^2 and up), so the GPU suite compares against Pillow where Pillow is not installed."""
import hashlib
import io
import json
import os

import numpy as np
import pytest

import jpeg_model as M
from conftest import GOLDEN

QUALITIES = (1, 10, 50, 75, 90, 95, 100)


def _fixtures():
    meta = json.load(open(os.path.join(GOLDEN, "jpeg_pil.json")))
    return meta, dict(np.load(os.path.join(GOLDEN, "jpeg_pil.npz")))


def _pillow():
    try:
        from PIL import Image, features
    except ImportError:
        pytest.skip("Pillow is not installed here: the live comparison is skipped (the frozen fixtures are still checked)")
    return Image, features


def _pil_bytes(img, q):
    Image, _ = _pillow()
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=q)
    return b.getvalue()


def _same(data, case, arrays):
    if case["name"] in arrays:
        return data == arrays[case["name"]].tobytes()
    return len(data) == case["length"] and hashlib.sha256(data).hexdigest() == case["sha256"]


def test_fixtures_cover_the_cases_the_encoder_must_get_right():
    meta, arrays = _fixtures()
    names = [c["name"] for c in meta["cases"]]
    assert meta["pillow"] and meta["libjpeg_turbo"], "the fixture must say which Pillow / libjpeg-turbo wrote it"
    for kind in ("gradient", "noise", "flat", "primaries", "extremes", "sparse", "edges", "golden", "smooth"):
        assert any(c["recipe"]["kind"] == kind for c in meta["cases"]), kind
    assert {c["quality"] for c in meta["cases"]} >= set(QUALITIES)
    assert {"golden_normal_512_q75", "golden_large_512_q75", "final_ff_g_16x16_q75"} <= set(names)
    assert {(c["recipe"]["h"], c["recipe"]["channels"]) for c in meta["cases"]} >= {(512, 3), (512, 1), (768, 3), (768, 1), (1024, 3), (1024, 1)}
    assert all(c["name"] in arrays for c in meta["cases"] if c["recipe"]["h"] * c["recipe"]["w"] < 512 * 512)
    sz = sum(os.path.getsize(os.path.join(GOLDEN, "jpeg_pil." + e)) for e in ("json", "npz"))
    assert sz < 1 << 20, sz


def test_fixture_recipes_reach_the_extremes_of_the_code():
    """DC differences of 11 bits and AC values of 10 bits (q100 extremes), runs of 16+ zeros (ZRL), all-EOB blocks, dense 0xFF
    stuffing, and a final padded byte that is 0xFF"""
    r = lambda **k: M.make_image(dict(k))
    coef, comp = M.coefficients(r(kind="extremes", h=64, w=64, channels=3), 100)
    dc = coef[comp == 0, 0]
    assert np.abs(np.diff(dc)).max() >= 1024                                                    # category 11
    assert np.abs(coef[:, 1:]).max() >= 512                                                     # category 10
    coef, _ = M.coefficients(r(kind="sparse", h=64, w=64, channels=3), 75)
    nz = [np.nonzero(b[1:])[0] for b in coef]
    assert any(len(p) and p[0] >= 16 for p in nz), "no run of 16 zeros"
    coef, _ = M.coefficients(r(kind="flat", h=32, w=32, channels=3, value=128), 75)
    assert not coef[:, 1:].any()
    scan = M.scan(M.encode(r(kind="noise", h=64, w=64, channels=3, seed=14), 100))
    assert scan.count(b"\xff\x00") > 40
    meta, _ = _fixtures()
    rec = next(c for c in meta["cases"] if c["name"] == "final_ff_g_16x16_q75")["recipe"]
    data, bits = M.entropy_code(*M.coefficients(M.make_image(rec), 75), with_bits=True)
    assert bits % 8 and data.endswith(b"\xff\x00")


def test_model_reproduces_every_pillow_fixture():
    meta, arrays = _fixtures()
    bad = [c["name"] for c in meta["cases"] if not _same(M.encode(M.make_image(c["recipe"]), c["quality"]), c, arrays)]
    assert not bad, bad


def test_model_matches_the_installed_pillow():
    Image, features = _pillow()
    meta, _ = _fixtures()
    for c in meta["cases"]:
        r = c["recipe"]
        if r["h"] * r["w"] >= 512 * 512 and r["kind"] != "golden":
            continue                                                                            # (the frames: the fixture check above)
        img = M.make_image(r)
        assert M.encode(img, c["quality"]) == _pil_bytes(img, c["quality"]), c["name"]
    rng = np.random.default_rng(7)
    for q in QUALITIES:
        img = rng.integers(0, 256, (32, 48, 3), np.uint8)
        assert M.encode(img, q) == _pil_bytes(img, q), q


def test_model_quantisation_tables_are_pillows_for_every_quality():
    _pillow()
    for q in range(1, 101):
        for ch in (3, 1):
            img = np.zeros((16, 16, 3) if ch == 3 else (16, 16), np.uint8)
            hdr = M.header(16, 16, ch, q)
            assert _pil_bytes(img, q)[:len(hdr)] == hdr, (q, ch)


def test_library_header_is_the_prefix_of_pillows_files():
    """lspjpeg_create + lspjpeg_header are host calls (no device): SOI .. SOS in Pillow's layout"""
    from livespeechportraits_amd.jpeg import file_header
    meta, arrays = _fixtures()
    for c in meta["cases"]:
        r = c["recipe"]
        hdr = file_header(r["w"], r["h"], r["channels"], c["quality"])
        full = arrays[c["name"]].tobytes() if c["name"] in arrays else None
        if full is not None:
            assert full[:len(hdr)] == hdr and M.scan(full) == full[len(hdr):], c["name"]
        assert hdr == M.header(r["w"], r["h"], r["channels"], c["quality"]), c["name"]
    for q in range(1, 101):
        for (h, w, ch) in ((512, 512, 3), (768, 1024, 3), (512, 512, 1), (24, 40, 1)):
            assert file_header(w, h, ch, q) == M.header(w, h, ch, q), (h, w, ch, q)


def test_library_header_against_live_pillow():
    _pillow()
    from livespeechportraits_amd.jpeg import file_header
    for q in QUALITIES:
        for (h, w, ch) in ((512, 512, 3), (16, 48, 3), (512, 512, 1), (8, 24, 1)):
            hdr = file_header(w, h, ch, q)
            img = np.full((h, w, 3) if ch == 3 else (h, w), 90, np.uint8)
            assert _pil_bytes(img, q)[:len(hdr)] == hdr, (h, w, ch, q)
    # SOF0 of a colour file: 4:2:0 (Y 2x2, Cb / Cr 1x1), as Pillow writes it
    hdr = file_header(512, 512, 3, 75)
    assert bytes.fromhex("012200021101031101") in hdr[hdr.index(b"\xff\xc0"):]


def test_library_capacity_and_refusals_on_the_host():
    """the documented worst-case bound per frame, and the refusals of lspjpeg_create (before any device work)"""
    import ctypes
    from livespeechportraits_amd import _native as N
    lib = N.load()
    h = ctypes.c_void_p()
    for (w, hh, ch) in ((512, 512, 3), (1024, 768, 3), (512, 512, 1), (16, 16, 3), (8, 8, 1)):
        N.check_jpeg(lib.lspjpeg_create(w, hh, ch, 75, ctypes.byref(h)))
        blocks = w * hh // 64 * (3 if ch == 3 else 2) // 2
        assert lib.lspjpeg_capacity_bytes(h) == 2 * ((blocks * 1660 + 7) // 8) + 2
        assert lib.lspjpeg_workspace_bytes(h, 8) > lib.lspjpeg_workspace_bytes(h, 1) > 0
        lib.lspjpeg_destroy(h)
    for args in ((520, 512, 3, 75), (512, 520, 3, 75), (36, 40, 1, 75), (512, 512, 2, 75), (512, 512, 4, 75), (512, 512, 3, 0),
                 (512, 512, 3, 101), (0, 512, 3, 75), (16384, 16, 3, 75)):
        rc = lib.lspjpeg_create(*args, ctypes.byref(h))
        assert rc < 0 and not h.value, args
        assert lib.lspjpeg_last_error()
    # a colour frame's H, W must be multiples of 16 (one 4:2:0 MCU); grayscale multiples of 8
    from livespeechportraits_amd.jpeg import file_header
    with pytest.raises(N.LspjpegError):
        file_header(24, 24, 3, 75)
    assert file_header(24, 24, 1, 75)


def test_render_loop_refuses_jpeg_for_a_host_model():
    """there is no host encoder: a model that renders on the host together with jpeg_quality raises (the keyword exists)"""
    import torch
    from livespeechportraits_amd.render_loop import render_frames

    class Host:
        def inference_image(self, maps, cand):
            return torch.zeros((maps.shape[0], 16, 16, 3), dtype=torch.uint8)
    maps = [torch.zeros(1, 16, 16) for _ in range(3)]
    with pytest.raises(ValueError, match="jpeg_quality"):
        render_frames(Host(), iter(maps), torch.zeros(1, 12, 16, 16), batch=2, jpeg_quality=75)
    assert len(render_frames(Host(), iter(maps), torch.zeros(1, 12, 16, 16), batch=2)) == 3
