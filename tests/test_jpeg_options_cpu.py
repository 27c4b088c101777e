"""The JPEG encoder's options on the host (no GPU): tests/jpeg_options_model.py restates what Pillow writes with `optimize=True`,
`restart_marker_rows=` and `restart_marker_blocks=` and must give Pillow's bytes; the library's host calls (lspjpeg_create_opts,
lspjpeg_header, lspjpeg_capacity_bytes, lspjpeg_host_optimal_table) must agree with it; csrc/jpegenc_core.h runs as a stand-alone
program under the sanitizers.

Pillow's bytes are frozen in tests/golden/jpeg_options.{json,npz} by tools/make_golden_jpeg_options.py."""
import ctypes
import functools
import io
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_model as M
import jpeg_options_model as O
from conftest import GOLDEN

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "livespeechportraits_amd", "csrc")
QUALITIES = (1, 50, 75, 95, 100)
SETS = [(o, r, b) for o in (0, 1) for (r, b) in ((0, 0), (1, 0), (2, 0), (0, 1), (0, 3))]           # (optimize, restart_rows, restart_blocks)


@functools.lru_cache(None)
def _fixtures():
    meta = json.load(open(os.path.join(GOLDEN, "jpeg_options.json")))
    return meta, dict(np.load(os.path.join(GOLDEN, "jpeg_options.npz")))


def _restart(c):
    r = c["recipe"]
    return O.restart_interval(r["w"], r["channels"], c["restart_rows"], c["restart_blocks"])


@functools.lru_cache(None)
def _modelled(name):
    """(the model's file, its info) of a fixture: computed once, shared by the tests"""
    meta, _ = _fixtures()
    c = next(c for c in meta["cases"] if c["name"] == name)
    info = {}
    data = O.encode(O.make_image(c["recipe"]), c["quality"], bool(c["optimize"]), _restart(c), info)
    return data, info


def _pillow():
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("Pillow is not installed here: the live comparison is skipped (the frozen fixtures are still checked)")
    return Image


def _pil_bytes(img, q, o, rows, blocks):
    b = io.BytesIO()
    _pillow().fromarray(img).save(b, "JPEG", quality=q, optimize=bool(o), restart_marker_rows=rows, restart_marker_blocks=blocks)
    return b.getvalue()


def _host_table(freq):
    from livespeechportraits_amd import _native as N
    f = (ctypes.c_uint32 * 256)(*[int(v) for v in freq])
    bits, vals, n = (ctypes.c_ubyte * 17)(), (ctypes.c_ubyte * 256)(), ctypes.c_int()
    N.check_jpeg(N.load().lspjpeg_host_optimal_table(f, bits, vals, ctypes.byref(n)))
    return list(bits), bytes(vals[:n.value])


def _fibonacci(n, a=1, b=2):
    out = [a, b]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


def _synthetic():
    """histograms no picture gives: one symbol, all equal, counts whose unlimited codes pass 16 and 32 bits, counts near 2^32"""
    single = [0] * 256
    single[0x21] = 9
    return {"single": single, "equal": [1] * 256, "equal_large": [4294967295] * 256, "fib_20": _fibonacci(20) + [0] * 236,
            "fib_40_descending": [0] * 100 + _fibonacci(40)[::-1] + [0] * 116, "fib_ties": [0] * 7 + _fibonacci(24, 1, 1) + [0] * 225,
            "near_2_32": [4294967295 - 3 * i for i in range(256)], "empty": [0] * 256,
            "two": [0] * 254 + [4294967295, 1]}


# ---- 1. the model is Pillow --------------------------------------------------------------------------------------------------------------
def test_fixtures_record_their_origin_and_cover_the_option_grid():
    meta, arrays = _fixtures()
    assert meta["pillow"] and meta["libjpeg_turbo"], "the fixture must say which Pillow / libjpeg-turbo wrote it"
    cases = meta["cases"]
    assert {c["quality"] for c in cases} >= set(QUALITIES)
    assert {(c["optimize"], c["restart_rows"], c["restart_blocks"]) for c in cases} >= set(SETS[1:])
    assert {(c["recipe"]["h"], c["recipe"]["w"], c["recipe"]["channels"]) for c in cases} >= {(16, 16, 3), (48, 48, 3), (8, 8, 1), (24, 40, 1), (32, 48, 3)}
    assert all(c["name"] in arrays for c in cases)
    sz = sum(os.path.getsize(os.path.join(GOLDEN, "jpeg_options." + e)) for e in ("json", "npz"))
    assert sz < 1 << 19, sz


def test_model_reproduces_every_pillow_fixture():
    meta, arrays = _fixtures()
    bad = [c["name"] for c in meta["cases"] if _modelled(c["name"])[0] != arrays[c["name"]].tobytes()]
    assert not bad, bad


def test_model_matches_the_installed_pillow():
    _pillow()
    rng = np.random.default_rng(11)
    for q in QUALITIES:
        for shape in ((48, 48, 3), (24, 40), (16, 16, 3), (8, 8)):
            ch = 3 if len(shape) == 3 else 1
            img = rng.integers(0, 256, shape, np.uint8) if q != 50 else M.make_image(dict(kind="smooth", h=shape[0], w=shape[1], channels=ch, seed=q))
            for (o, rows, blocks) in SETS:
                got = O.encode(img, q, bool(o), O.restart_interval(shape[1], ch, rows, blocks))
                assert got == _pil_bytes(img, q, o, rows, blocks), (q, shape, o, rows, blocks)


# ---- 2. the recipes reach what the code can get wrong ----------------------------------------------------------------------------------------
def test_fixture_recipes_reach_the_cases_the_code_can_get_wrong():
    meta, arrays = _fixtures()
    info = lambda name: _modelled(name)[1]
    # more than 8 intervals in a frame: RST7 is followed by RST0
    data, i = _modelled("smooth_c_48x48_q75_o0_r0_b1")
    assert len(i["bits"]) == 9 and O.segments(data)[-2][0] == 0xDD
    scan = M.scan(data)
    marks = [scan[k + 1] for k in range(len(scan) - 1) if scan[k] == 0xFF and 0xD0 <= scan[k + 1] <= 0xD7]
    assert marks == [0xD0 + (k & 7) for k in range(8)] and marks[-1] == 0xD7
    assert len(info("smooth_c_48x48_q75_o1_r0_b1")["bits"]) == 9
    scan = M.scan(_modelled("edges_g_24x40_q75_o0_r0_b1")[0])                                   # 15 intervals: RST0 .. RST7, RST0 .. RST5
    assert [scan[k + 1] for k in range(len(scan) - 1) if scan[k] == 0xFF and 0xD0 <= scan[k + 1] <= 0xD7] == [0xD0 + (k & 7) for k in range(14)]
    # the padded byte of an interval that is not the last is 0xFF and gets stuffed, in front of the marker
    for name in ("pad_ff_g_16x16_q75_o0_r0_b1", ):
        data, i = _modelled(name)
        k = i["stuffed_pad"][:-1].index(True)
        assert bytes([0xFF, 0x00, 0xFF, 0xD0 + (k & 7)]) in M.scan(data)
    # an interval that ends on a byte boundary (no padding), and one that does not
    bits = [b for c in meta["cases"] if c["restart_blocks"] or c["restart_rows"] for b in info(c["name"])["bits"][:-1]]
    assert any(b % 8 == 0 for b in bits) and any(b % 8 for b in bits)
    # an interval longer than the frame, and an interval length that does not divide the MCU count
    c = next(c for c in meta["cases"] if c["name"] == "noise_c_16x16_q75_o0_r0_b3")
    assert len(info(c["name"])["bits"]) == 1                                                    # an interval longer than the frame: DRI, no marker
    c = next(c for c in meta["cases"] if c["name"] == "smooth_c_48x48_q75_o1_r2_b0")
    assert _restart(c) == 6 and len(info(c["name"])["bits"]) == 2 and 9 % 6                     # 9 MCUs in intervals of 6: 6 + 3
    # a frame whose optimised AC table holds EOB alone
    for name in ("flat_g_16x16_q75_o1_r0_b0", "flat_g_16x16_q75_o1_r0_b1"):
        bits, vals = info(name)["tables"][0][1]
        assert vals == b"\x00" and sum(bits) == 1
    # the frames of the batch get different tables
    tabs = [json.dumps([[list(t[0]), list(t[1])] for pair in info("batch%d_c_32x48_q75_o1_r0_b0" % k)["tables"] for t in pair]) for k in range(3)]
    assert len(set(tabs)) == 3
    # a table that went through the 16-bit limit, in a file Pillow wrote
    for name in ("limiter_g_848x512_q25_o1_r0_b0", "limiter_g_848x512_q25_o1_r1_b0"):
        freq = info(name)["freq"][0][1]
        assert max(O.code_sizes(freq)) > 16
        bits, vals = O.parse_dht(arrays[name].tobytes())[(1, 0)]
        assert bits[16] > 0 and (bits, vals) == tuple(O.gen_optimal_table(freq))


# ---- 3. the library's table builder -------------------------------------------------------------------------------------------------------
def _all_histograms():
    meta, _ = _fixtures()
    out = []
    for c in meta["cases"]:
        if c["optimize"]:
            out += [(c["name"], f) for pair in _modelled(c["name"])[1]["freq"] for f in pair]
    return out


def test_host_optimal_table_equals_the_restated_algorithm():
    hists = _all_histograms()
    assert len(hists) > 100
    for name, freq in hists + list(_synthetic().items()):
        assert _host_table(freq) == tuple(O.gen_optimal_table(freq)), name
    s = _synthetic()
    assert _host_table(s["single"]) == ([0, 1] + [0] * 15, b"\x21")
    assert max(O.code_sizes(s["fib_20"])) > 16 and max(O.code_sizes(s["fib_40_descending"])) > 32
    assert _host_table(s["equal"])[0] == [0] * 8 + [255, 1] + [0] * 7                            # 257 leaves: 255 of 8 bits, 2 of 9, one the pseudo-symbol's


def test_host_optimal_table_equals_the_tables_in_pillows_files():
    """the DHT segments libjpeg itself wrote, for the histograms the model counts"""
    meta, arrays = _fixtures()
    n = 0
    for c in meta["cases"]:
        if not c["optimize"]:
            continue
        tables = O.parse_dht(arrays[c["name"]].tobytes())
        freq = _modelled(c["name"])[1]["freq"]
        assert len(tables) == 2 * len(freq), c["name"]
        for t, pair in enumerate(freq):
            for cls in (0, 1):
                assert _host_table(pair[cls]) == tables[(cls, t)], (c["name"], cls, t)
                n += 1
    assert n > 100


# ---- 5. headers ------------------------------------------------------------------------------------------------------------------------------
def test_library_header_is_the_prefix_of_pillows_files():
    from livespeechportraits_amd.jpeg import JpegOptions, file_header
    meta, arrays = _fixtures()
    for c in meta["cases"]:
        r = c["recipe"]
        hdr = file_header(r["w"], r["h"], r["channels"], c["quality"], bool(c["optimize"]), c["restart_rows"], c["restart_blocks"])
        full = arrays[c["name"]].tobytes()
        assert full[:len(hdr)] == hdr, c["name"]
        assert hdr == O.file_header(r["w"], r["h"], r["channels"], c["quality"], bool(c["optimize"]), _restart(c)), c["name"]
        assert hdr == file_header(r["w"], r["h"], r["channels"], JpegOptions(c["quality"], bool(c["optimize"]), c["restart_rows"], c["restart_blocks"]))
        last = O.segments(hdr + (b"" if not c["optimize"] else full[len(hdr):]))[-1]
        assert hdr.endswith(b"\x00\x3f\x00") != bool(c["optimize"]) and last[0] == 0xDA


def test_library_header_against_live_pillow():
    _pillow()
    from livespeechportraits_amd.jpeg import file_header
    for q in (1, 75, 100):
        for (h, w, ch) in ((512, 512, 3), (16, 48, 3), (512, 512, 1), (8, 24, 1)):
            img = np.full((h, w, 3) if ch == 3 else (h, w), 90, np.uint8)
            for (o, rows, blocks) in SETS:
                hdr = file_header(w, h, ch, q, bool(o), rows, blocks)
                assert _pil_bytes(img, q, o, rows, blocks)[:len(hdr)] == hdr, (h, w, ch, q, o, rows, blocks)
    # rows * MCUs per row is capped at 65535, as jinit_c_master_control caps it: 8192 x 16 with 200 rows of 512 MCUs
    img = np.zeros((16, 8192, 3), np.uint8)
    pil = _pil_bytes(img, 75, 0, 200, 0)
    hdr = file_header(8192, 16, 3, 75, restart_rows=200)
    assert pil[:len(hdr)] == hdr and b"\xff\xdd\x00\x04\xff\xff\xff\xda" in hdr
    assert file_header(8192, 16, 3, 75, restart_rows=200) == O.file_header(8192, 16, 3, 75, False, 65535)


# ---- 6. capacity and refusals ----------------------------------------------------------------------------------------------------------------
def _create(width, height, comps, quality, optimize, restart, abi=None):
    from livespeechportraits_amd import _native as N
    o = N.JpegEncOptions(N.JPEG_ABI_VERSION if abi is None else abi, width, height, comps, quality, optimize, restart)
    h = ctypes.c_void_p()
    return N.load().lspjpeg_create_opts(ctypes.byref(o), ctypes.byref(h)), h


def test_capacity_holds_every_fixture_and_is_todays_without_options():
    from livespeechportraits_amd import _native as N
    lib = N.load()
    meta, arrays = _fixtures()
    for c in meta["cases"]:
        r = c["recipe"]
        rc, h = _create(r["w"], r["h"], r["channels"], c["quality"], c["optimize"], _restart(c))
        assert rc == 0, c["name"]
        hdr = lib.lspjpeg_header(h, None, 0)
        assert 0 < len(_modelled(c["name"])[0]) - hdr <= lib.lspjpeg_capacity_bytes(h), c["name"]
        assert lib.lspjpeg_workspace_bytes(h, 3) > lib.lspjpeg_workspace_bytes(h, 1) > 0
        lib.lspjpeg_destroy(h)
    for (w, hh, ch) in ((512, 512, 3), (1024, 768, 3), (512, 512, 1), (16, 16, 3), (8, 8, 1)):
        blocks = w * hh // 64 * (3 if ch == 3 else 2) // 2
        today = 2 * ((blocks * 1660 + 7) // 8) + 2
        rc, h = _create(w, hh, ch, 75, 0, 0)
        plain = ctypes.c_void_p()
        N.check_jpeg(lib.lspjpeg_create(w, hh, ch, 75, ctypes.byref(plain)))
        assert rc == 0 and lib.lspjpeg_capacity_bytes(h) == lib.lspjpeg_capacity_bytes(plain) == today
        assert lib.lspjpeg_workspace_bytes(h, 8) == lib.lspjpeg_workspace_bytes(plain, 8)
        lib.lspjpeg_destroy(plain)
        lib.lspjpeg_destroy(h)
        # the stated bound: 27 + 63 * 26 bits per block with optimised tables, a byte of padding per interval, all of it stuffed, 2 bytes per
        # marker, EOI, and the tables (452 bytes)
        mcus = blocks // (6 if ch == 3 else 1)
        for optimize, restart in ((1, 0), (0, 1), (1, 7), (0, 65535)):
            rc, h = _create(w, hh, ch, 75, optimize, restart)
            nint = -(-mcus // restart) if restart else 1
            want = 2 * ((blocks * (1665 if optimize else 1660) + 7) // 8 + nint) + 2 * (nint - 1) + 2 + (452 if optimize else 0)
            assert rc == 0 and lib.lspjpeg_capacity_bytes(h) == want, (w, hh, ch, optimize, restart)
            lib.lspjpeg_destroy(h)


def test_refusals_touch_no_device():
    from livespeechportraits_amd import _native as N
    from livespeechportraits_amd.jpeg import JpegEncoder, JpegOptions, file_header
    for kw in (dict(restart=-1), dict(restart=65536), dict(optimize=2), dict(optimize=-1), dict(abi=0), dict(abi=2)):
        args = dict(optimize=0, restart=0, abi=None)
        args.update(kw)
        rc, h = _create(512, 512, 3, 75, args["optimize"], args["restart"], args["abi"])
        assert rc < 0 and not h.value and N.load().lspjpeg_last_error(), kw
    assert _create(520, 512, 3, 75, 1, 0)[0] < 0 and _create(512, 512, 3, 0, 1, 0)[0] < 0          # the geometry and quality rules of lspjpeg_create
    assert _create(512, 512, 3, 75, 1, 65535)[0] == 0
    with pytest.raises(ValueError, match="not both"):
        JpegEncoder(512, 3, 75, "cuda:0", optimize=True, restart_rows=1, restart_blocks=2)
    with pytest.raises(ValueError, match="not both"):
        file_header(512, 512, 3, 75, restart_rows=1, restart_blocks=2)
    with pytest.raises(ValueError, match="not both"):
        JpegOptions.of(JpegOptions(75, False, 1, 1))
    with pytest.raises(N.LspjpegError):
        file_header(512, 512, 3, 75, restart_blocks=65536)
    assert JpegOptions.of(90) == JpegOptions(90, False, 0, 0)
    for q in (0, 101):                                                                          # the quality is refused where it always was, with the same error
        for kw in ({}, dict(optimize=True), dict(restart_rows=1)):
            with pytest.raises(N.LspjpegError):
                file_header(512, 512, 3, q, **kw)
    assert JpegOptions(75, restart_rows=200).restart_interval(8192, 3) == 65535


# ---- 7. the core header under the sanitizers ---------------------------------------------------------------------------------------------------
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
    """csrc/jpegenc_check.cpp (the table builder and the interval bookkeeping of jpegenc_core.h as host code under ASan + UBSan, with its
    own main) over the histograms of every fixture and the synthetic ones, against the Python restatement's tables"""
    why = _sanitizer_works(tmp_path)
    if why:
        pytest.skip(why)
    subprocess.run(["make", "-C", CSRC, "-s", "check-jpegenc"], check=True)
    hists = [f for _, f in _all_histograms()] + list(_synthetic().values())
    bundle = bytearray(b"LSEH" + struct.pack("<I", len(hists)))
    for freq in hists:
        bits, vals = O.gen_optimal_table(freq)
        bundle += struct.pack("<256I", *freq) + bytes(bits) + struct.pack("<I", len(vals)) + vals
    path = tmp_path / "histograms.bin"
    path.write_bytes(bytes(bundle))
    r = subprocess.run([os.path.join(CSRC, "build", "jpegenc_check"), str(path)], capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "%d histograms" % len(hists) in r.stdout and " 0 failures" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
