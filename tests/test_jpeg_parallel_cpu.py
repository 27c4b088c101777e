"""The parallel route of the JPEG decoder's stage 1 (LSPJPEG_DEC_FLAG_PARALLEL) without a device.  On a plan made with ``parallel=True``
``host_coefficients`` runs the kernel's subsequence decoder, fixed point and write pass with the lanes as loops; the yardstick is the serial
host decoder on the same bytes: same status for every file, same coefficients wherever the status is 0.  Also here: a plan made without the flag
is byte for byte what the parent commit's library wrote, the coverage the fixtures give the route, and the sanitizer-built stand-alone checker
(csrc/jpegdec_par_check.cpp).  The device half is tests/test_gpu_jpeg_parallel.py."""
import hashlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_decode_cases as K
import jpeg_decode_model as D
import jpeg_model as M
from conftest import ROOT

CSRC = os.path.join(ROOT, "livespeechportraits_amd", "csrc")


def _both(files):
    """[(status, coefficients)] of the serial and of the parallel route for one batch"""
    from livespeechportraits_amd import jpeg as J
    serial, parallel = J.DecodePlan(files), J.DecodePlan(files, parallel=True)
    return [serial.host_coefficients(i) for i in range(len(files))], [parallel.host_coefficients(i) for i in range(len(files))]


def _same(a, b):
    return a[0] == b[0] and (a[0] != 0 or np.array_equal(a[1], b[1]))


def test_every_fixture_decodes_to_the_serial_coefficients():
    _, files, _ = K.fixtures()
    everything = dict(files)
    everything.update(K.frames_512())
    assert len(K.small_names()) >= 100 and len(K.frames_512()) == 12
    for name in K.small_names() + sorted(K.frames_512()):
        serial, parallel = _both([everything[name]])
        assert serial[0][0] == 0 and _same(serial[0], parallel[0]), name


def test_all_fixtures_in_one_batch():
    _, files, _ = K.fixtures()
    names = sorted(files)                                       # the small fixtures, their twins without DHT, the corrupt and the refused files
    serial, parallel = _both([files[n] for n in names])
    for n, s, p in zip(names, serial, parallel):
        assert _same(s, p), (n, s[0], p[0])
    assert sum(1 for s in serial if s[0] == 0) >= 100


@pytest.mark.parametrize("k", range(len(K.refusals())))
def test_every_refusal_keeps_its_code(k):
    what, data, want = K.refusals()[k]
    serial, parallel = _both([data])
    assert serial[0][0] == want and _same(serial[0], parallel[0]), what


def _changed(files, names):
    """tests/test_jpeg_decode_cpu.py's inputs: every truncation of three files, and 25 single-byte changes of eight at the same seed"""
    rng = np.random.default_rng(20261018)
    for n in names[:3]:
        for length in range(len(files[n])):
            yield n, files[n][:length]
    for n in names:
        for _ in range(25):
            b = bytearray(files[n])
            b[int(rng.integers(len(b)))] ^= int(rng.integers(1, 256))
            yield n, bytes(b)


def test_truncations_and_corruptions_keep_status_and_coefficients():
    _, files, _ = K.fixtures()
    names = [K.find(p) for p in ("_420_9x3_", "_greyrst_5x2_", "_rstb_4x9_", "_422_40x72_", "_opt_16x16_", "_444_8x24_", "_grey_16x16_", "_rstr_40x72_")]
    batch = list(_changed(files, names))
    counts = {0: 0, 1: 0, 2: 0, 3: 0}
    for at in range(0, len(batch), 64):
        part = batch[at:at + 64]
        serial, parallel = _both([d for _, d in part])
        for (n, data), s, p in zip(part, serial, parallel):
            assert _same(s, p), (n, len(data), s[0], p[0])
            counts[s[0]] += 1
    print(counts)
    assert counts[2] > 300 and counts[0] > 20                   # the inputs do reach stage 1 both ways


def _grey_row(blocks, symbols):
    """a grey file of `blocks` 8x8 blocks in one row on Annex K's tables, its scan written here (as jpeg_decode_cases.refusals() does)"""
    _, files, _ = K.fixtures()
    grey_nodht = files[K.find("_grey_40x72_") + "_nodht"]
    sof = K.segment(grey_nodht, 0xC0)[1]
    head = K.patched(grey_nodht, sof + 5, b"\x00\x08" + (8 * blocks).to_bytes(2, "big"))[:D.parse(grey_nodht)["scan_begin"]]
    return head + K.pack_bits(symbols) + b"\xff\xd9"


def test_two_failures_in_one_interval_report_the_first():
    """Blocks of DC difference +2047 and nothing else: the prediction leaves int16 at the 17th (RANGE).  A code that is in no table (sixteen
    1-bits where a DC code is due) stands behind it in one file and in front of it in the other.  Every block is 3 bytes, so the two failures lie
    in different subsequences, and the serial walk's answer -- the first in stream order -- has to come out of the lanes' answers."""
    from livespeechportraits_amd import jpeg as J
    dco, dsi = M._CODES["dc0"]
    aco, asi = M._CODES["ac0"]
    block = [(int(dco[11]), int(dsi[11])), (2047, 11), (int(aco[0]), int(asi[0]))]       # DC size 11, +2047, EOB
    bad = [(0xFFFF, 16)]
    n = 40
    control = _grey_row(16, block * 16)                         # sixteen such blocks stay inside int16
    range_first = _grey_row(n, block * 30 + bad + block * 9)
    corrupt_first = _grey_row(n, block * 5 + bad + block * 34)
    for what, data, want in (("control", control, 0), ("RANGE before CORRUPT", range_first, J.RANGE), ("CORRUPT before RANGE", corrupt_first, J.CORRUPT)):
        serial, parallel = _both([data])
        assert serial[0][0] == want, (what, serial[0][0])
        assert _same(serial[0], parallel[0]), (what, parallel[0][0])
        plan = J.DecodePlan([data], parallel=True)
        assert plan.parallel_segment(0)[1] >= 4, what
    assert _both([control])[1][0][1][15, 0] == 16 * 2047


# sha256 of the whole descriptor block of DecodePlan([file]) as the parent commit's library wrote it (flags = 0)
PARENT_PLANS = {
    "_420_40x72_": "b4c3bb1fbea705378a522599bd0a4a3519f2c8263c88439ed0f194aa1852a7dd",
    "_rstr_40x72_": "0b0b7d11c4f89458bb38c98cbb91c48ab1d9ac18b4c6ea73fb6f4aec544e329e",
    "_grey_16x16_": "2dfa0ba86cb08c443814212b6892df6b9445c05423182dfe8ab9fa4d683bd595",
}


def test_a_plan_without_the_flag_is_the_parent_commits():
    from livespeechportraits_amd import jpeg as J
    _, files, _ = K.fixtures()
    for part, want in PARENT_PLANS.items():
        data = files[K.find(part)]
        plan = J.DecodePlan([data])
        assert hashlib.sha256(bytes(plan.blob[:plan.bytes])).hexdigest() == want, part
        # and the flag changes one word of the header, nothing else: no area moves, the workspace does not grow
        flagged = J.DecodePlan([data], parallel=True)
        a, b = np.asarray(plan.blob[:plan.bytes]), np.asarray(flagged.blob[:flagged.bytes])
        assert plan.bytes == flagged.bytes and list(np.nonzero(a != b)[0]) == [24]
        assert plan.summary.workspace_bytes == flagged.summary.workspace_bytes
    prog = files["refused_progressive"]
    a, b = J.DecodePlan([prog, data], progressive=True), J.DecodePlan([prog, data], progressive=True, parallel=True)
    assert a.statuses() == [0, 0] and list(np.nonzero(np.asarray(a.blob[:a.bytes]) != np.asarray(b.blob[:b.bytes]))[0]) == [24]


def test_the_probe_takes_the_flag_and_ignores_it():
    from livespeechportraits_amd import _native as N
    import ctypes
    data = K.fixtures()[1][K.find("_420_40x72_")]
    lib = N.load()
    infos = []
    for flags in (0, 2, 1, 3):
        info = N.JpegDecInfo()
        assert lib.lspjpeg_dec_probe_flags(ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), len(data), flags, ctypes.byref(info)) == 0
        infos.append(bytes(info))
    assert len(set(infos)) == 1
    assert lib.lspjpeg_dec_probe_flags(ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), len(data), 4, ctypes.byref(N.JpegDecInfo())) < 0


def test_parallel_segment_needs_the_flag():
    from livespeechportraits_amd import jpeg as J
    from livespeechportraits_amd import _native as N
    data = K.fixtures()[1][K.find("_rstr_40x72_")]
    with pytest.raises(N.LspjpegError):
        J.DecodePlan([data]).parallel_segment(0)
    plan = J.DecodePlan([data], parallel=True)
    for k in range(plan.summary.segments):
        _, _, _, begin, end = plan.segment(k)
        size, count = plan.parallel_segment(k)
        assert size >= 1 and count == max(1, -(-(end - begin) // size)), k
    with pytest.raises(N.LspjpegError):
        plan.parallel_segment(plan.summary.segments)


def test_the_fixtures_cover_the_route():
    """A condition, not a measurement: the many-lane path, a fixed point of more than one round and an entry state inside a block all occur on
    the small fixtures (the 512^2 frames have thousands of subsequences each, but a test of the small ones alone must not pass on one lane)."""
    from livespeechportraits_amd import jpeg as J
    _, files, _ = K.fixtures()
    four = rounds2 = midblock = 0
    for n in K.small_names():
        plan = J.DecodePlan([files[n]], parallel=True)
        four += any(plan.parallel_segment(k)[1] >= 4 for k in range(plan.summary.segments))
        assert plan.host_coefficients(0)[0] == 0
        rounds, mid = plan.parallel_stats()
        rounds2 += rounds >= 2
        midblock += mid > 0
    print(len(K.small_names()), four, rounds2, midblock)
    assert 2 * four >= len(K.small_names()) and rounds2 >= 1 and midblock >= 1
    assert J.DecodePlan([files[K.small_names()[0]]]).host_coefficients(0)[0] == 0 and plan.parallel_stats() == (0, 0)     # the serial route counts nothing
    big = J.DecodePlan([sorted(K.frames_512().items())[0][1]], parallel=True)
    assert big.parallel_segment(0)[1] > 4096 and big.host_coefficients(0)[0] == 0 and big.parallel_stats()[0] >= 2       # more than one chunk


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
    """csrc/jpegdec_par_check.cpp (both routes as host code under ASan + UBSan, with its own main) over all small fixtures, one 512^2 frame, the
    refusals and the corrupt files, every truncation of three files and 25 single-byte changes of each: same status, same coefficients."""
    why = _sanitizer_works(tmp_path)
    if why:
        pytest.skip(why)
    subprocess.run(["make", "-C", CSRC, "-s", "check-jpegdec-par"], check=True)
    exe = os.path.join(CSRC, "build", "jpegdec_par_check")
    meta, files, _ = K.fixtures()
    entries = [files[n] for n in (K.find("_420_9x3_"), K.find("_rstr_40x72_"), K.find("_grey_16x16_"))]
    entries += [files[n] for n in K.small_names()] + [files[c["name"]] for c in meta["corrupt"]] + [d for _, d, _ in K.refusals()]
    entries.append(sorted(K.frames_512().items())[4][1])
    bundle = bytearray(b"LSDB" + struct.pack("<I", len(entries)))
    for data in entries:
        bundle += struct.pack("<III", len(data), 0, 0) + data             # the checker compares the two routes: no expectations travel
    path = tmp_path / "bundle.bin"
    path.write_bytes(bytes(bundle))
    r = subprocess.run([str(exe), str(path), "20261018", "3", "25"], capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "0 failures" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
