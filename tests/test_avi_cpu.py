"""The AVI container of livespeechportraits_amd/video.py on the host: files written by AviWriter, read back by the independent strict
parser tests/avi_parser.py and decoded chunk by chunk with Pillow.  The frames come from tests/jpeg_model.py (pinned to Pillow by
tests/test_jpeg_cpu.py).  No player or demuxer is involved: the container is player-unpinned."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

import avi_parser as P
import jpeg_model as M
from livespeechportraits_amd.video import AviFull, AviWriter, write_avi

GEOMETRIES = {"c16": (16, 16, 3), "c32x48": (32, 48, 3), "g8": (8, 8, 1)}        # (H, W, channels)
SPECIAL = np.array([np.nan, 1.5, -1.5, 1.0, -1.0, 0.0, -0.0, np.inf, -np.inf, 0.5 / 32767, 1.5 / 32767, 2.5 / 32767, -0.5 / 32767, 0.99999,
                    3.0517578e-05, 1e-30], np.float32)


def make_files(geom, n=8):
    h, w, ch = GEOMETRIES[geom]
    shape = (h, w, 3) if ch == 3 else (h, w)
    return [M.encode(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8), 75) for seed in range(n)]


def make_wave(n, seed=100):
    x = (np.random.default_rng(seed).standard_normal(n) * 0.4).astype(np.float32)
    x[:SPECIAL.size] = SPECIAL                                   # NaN, +-1.5, +-1.0, infinities, ties of the rounding
    x[266 - 3:266 + 3] = SPECIAL[:6]                             # and across the first chunk boundary
    return x


def pcm16_rule(x):
    """rintf(x * 32767.0f) clamped to +-32767, NaN as 0 -- stated in numpy, not taken from video.py"""
    v = np.rint(x.astype(np.float32) * np.float32(32767.0))
    out = np.zeros(x.shape, np.int16)
    ok = ~np.isnan(v)
    out[ok] = np.minimum(np.maximum(v[ok], -32767.0), 32767.0).astype(np.int16)
    return out


def write(path, geom, files, fmt, wave=None, **kw):
    h, w, ch = GEOMETRIES[geom]
    with AviWriter(str(path), w, h, ch, audio_rate=None if fmt is None else 16000, audio_format=fmt or "f32", **kw) as out:
        a, b = out.span(0, len(files))
        out.append_jpegs(files, None if fmt is None else wave[a:b])
    return open(path, "rb").read()


@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_both_size_parities_occur(geom):
    files = make_files(geom)
    assert {len(f) & 1 for f in files} == {0, 1}, [len(f) for f in files]
    h, w, ch = GEOMETRIES[geom]
    assert all(f.startswith(M.header(w, h, ch, 75)) for f in files)
    assert len(M.header(16, 16, 3, 75)) == 623 and len(M.header(8, 8, 1, 75)) == 328


@pytest.mark.parametrize("fmt", [None, "f32", "s16"])
@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_written_files_parse_and_decode(tmp_path, geom, fmt):
    files, wave = make_files(geom), make_wave(4000)
    h, w, ch = GEOMETRIES[geom]
    data = write(tmp_path / "a.avi", geom, files, fmt, wave)
    r = P.parse(data)
    assert r["first_chunk"] == (224 if fmt is None else 326)
    assert r["video"] == files
    for chunk, f in zip(r["video"], files):
        got, want = Image.open(io.BytesIO(chunk)), Image.open(io.BytesIO(f))
        assert got.size == (w, h) and got.mode == ("RGB" if ch == 3 else "L")
        assert np.array_equal(np.asarray(got), np.asarray(want))
    if fmt is None:
        assert r["audio"] is None and len(r["streams"]) == 1
        return
    n = 8 * 16000 // 60
    assert r["audio_counts"] == [(k + 1) * 16000 // 60 - k * 16000 // 60 for k in range(8)] and set(r["audio_counts"]) == {266, 267}
    assert r["audio"].shape == (n,)
    if fmt == "f32":
        assert r["audio"].dtype == np.float32 and r["audio"].tobytes() == wave[:n].tobytes()        # bit for bit, NaN included
    else:
        assert r["audio"].dtype == np.int16 and np.array_equal(r["audio"], pcm16_rule(wave[:n]))
        assert list(r["audio"][:5]) == [0, 32767, -32767, 32767, -32767]


def test_sample_split_of_a_whole_clip(tmp_path):
    """687 frames (the reference's demo clip): 266 / 267 samples per frame in the k * 16000 // 60 pattern, 183 200 in all, which is
    np.int32(nframe * sr / FPS) of demo.py:278"""
    files = make_files("g8", 2)
    wave = make_wave(183200 + 5)
    with AviWriter(str(tmp_path / "a.avi"), 8, 8, 1) as out:
        for k in range(0, 687, 64):
            n = min(64, 687 - k)
            a, b = out.span(k, n)
            out.append_jpegs([files[(k + j) & 1] for j in range(n)], wave[a:b])
    r = P.parse(open(tmp_path / "a.avi", "rb").read())
    assert r["audio_counts"] == [(k + 1) * 16000 // 60 - k * 16000 // 60 for k in range(687)]
    assert sum(r["audio_counts"]) == 183200 == int(np.int32(687 * 16000 / 60)) and r["audio"].tobytes() == wave[:183200].tobytes()
    assert r["avih"]["dwTotalFrames"] == 687


@pytest.mark.parametrize("fmt", [None, "f32", "s16"])
def test_header_fields(tmp_path, fmt):
    files, wave = make_files("c32x48"), make_wave(4000)
    data = write(tmp_path / "a.avi", "c32x48", files, fmt, wave)
    r = P.parse(data)
    movi = sum(8 + len(p) + (len(p) & 1) for _, _, p in r["chunks"])
    largest_v = max(len(f) for f in files)
    bps = {None: 0, "f32": 4, "s16": 2}[fmt]
    largest_a = 267 * bps
    a = r["avih"]
    assert a == {"dwMicroSecPerFrame": 16667, "dwMaxBytesPerSec": -(-movi * 60 // 8), "dwPaddingGranularity": 0, "dwFlags": 0x110, "dwTotalFrames": 8,
                 "dwInitialFrames": 0, "dwStreams": 1 if fmt is None else 2, "dwSuggestedBufferSize": max(largest_v, largest_a), "dwWidth": 48,
                 "dwHeight": 32, "dwReserved": [0, 0, 0, 0]}
    v = r["streams"][0]
    assert v["strh"] == {"fccType": b"vids", "fccHandler": b"MJPG", "dwFlags": 0, "wPriority": 0, "wLanguage": 0, "dwInitialFrames": 0, "dwScale": 1,
                         "dwRate": 60, "dwStart": 0, "dwLength": 8, "dwSuggestedBufferSize": largest_v, "dwQuality": 0xFFFFFFFF, "dwSampleSize": 0,
                         "rcFrame": (0, 0, 48, 32)}
    assert v["strf"] == {"biSize": 40, "biWidth": 48, "biHeight": 32, "biPlanes": 1, "biBitCount": 24, "biCompression": b"MJPG",
                         "biSizeImage": 48 * 32 * 3, "biXPelsPerMeter": 0, "biYPelsPerMeter": 0, "biClrUsed": 0, "biClrImportant": 0}
    if fmt is not None:
        s = r["streams"][1]
        assert s["strh"]["fccType"] == b"auds" and s["strh"]["fccHandler"] == b"\0\0\0\0"
        assert (s["strh"]["dwScale"], s["strh"]["dwRate"], s["strh"]["dwLength"], s["strh"]["dwSampleSize"]) == (1, 16000, 8 * 16000 // 60, bps)
        assert s["strh"]["dwSuggestedBufferSize"] == largest_a
        assert s["strf"] == {"wFormatTag": 3 if fmt == "f32" else 1, "nChannels": 1, "nSamplesPerSec": 16000, "nAvgBytesPerSec": 16000 * bps,
                             "nBlockAlign": bps, "wBitsPerSample": 8 * bps, "cbSize": 0}
    assert all(e[1] == 0x10 for e in r["index"]) and r["index"][0][2] == 4
    # grayscale: 8 bits
    g = P.parse(write(tmp_path / "g.avi", "g8", make_files("g8"), None))
    assert g["streams"][0]["strf"]["biBitCount"] == 8 and g["streams"][0]["strf"]["biSizeImage"] == 64


@pytest.mark.parametrize("rate", [None, 16000])
def test_empty_file_and_double_close(tmp_path, rate):
    w = AviWriter(str(tmp_path / "e.avi"), 16, 16, audio_rate=rate)
    w.close()
    first = open(tmp_path / "e.avi", "rb").read()
    w.close()
    assert open(tmp_path / "e.avi", "rb").read() == first
    r = P.parse(first)
    assert r["chunks"] == [] and r["index"] == [] and r["avih"]["dwTotalFrames"] == 0 and r["avih"]["dwMaxBytesPerSec"] == 0
    assert len(first) == (224 if rate is None else 326) + 8
    with pytest.raises(ValueError):
        w.append_jpegs(make_files("c16", 1), np.zeros(266, np.float32) if rate else None)


def test_append_jpegs_refusals(tmp_path):
    files, wave = make_files("c16"), make_wave(4000)
    w = AviWriter(str(tmp_path / "r.avi"), 16, 16)
    w.append_jpegs(files[:2], wave[:533])
    for bad in (wave[533:533 + 266], wave[533:533 + 268], None):                   # frame 2 carries 267 samples
        with pytest.raises(ValueError):
            w.append_jpegs(files[2:3], bad)
    ok = wave[533:800]
    for bad in (files[2][2:], files[2][:-2], files[2][:-1] + b"\0", b""):             # no SOI, no EOI
        with pytest.raises(ValueError):
            w.append_jpegs([files[3], bad], wave[533:1066])
    with pytest.raises(ValueError):
        w.append_jpegs(make_files("c32x48", 1), ok)                               # SOF0 says 48 x 32
    with pytest.raises(ValueError):
        w.append_jpegs(make_files("g8", 1), ok)
    assert w.nframes == 2
    w.append_jpegs(files[2:3], ok)
    w.close()
    r = P.parse(open(tmp_path / "r.avi", "rb").read())
    assert r["video"] == files[:3] and r["audio"].tobytes() == wave[:800].tobytes()
    silent = AviWriter(str(tmp_path / "s.avi"), 16, 16, audio_rate=None)
    with pytest.raises(ValueError):
        silent.append_jpegs(files[:1], wave[:266])
    silent.close()


def test_avi_full_is_raised_before_anything_is_written(tmp_path):
    files, wave = make_files("c16"), make_wave(4000)
    path = tmp_path / "f.avi"
    w = AviWriter(str(path), 16, 16, max_bytes=6000)
    w.append_jpegs(files[:2], wave[:533])                                         # 2 x (8 + 1064 + 8 + ~780): fits
    w._f.flush()
    size = path.stat().st_size
    with pytest.raises(AviFull):
        w.append_jpegs(files[2:5], wave[533:1333])
    w._f.flush()
    assert path.stat().st_size == size and w.nframes == 2 and w.nsamples == 533
    w.close()
    data = open(path, "rb").read()
    r = P.parse(data)
    assert r["video"] == files[:2] and len(data) - 8 <= 6000
    # the limit counts the index the close will write: a file that fits exactly is accepted, one byte less is not
    exact = len(data) - 8
    for limit, fits in ((exact, True), (exact - 1, False)):
        w = AviWriter(str(tmp_path / "g.avi"), 16, 16, max_bytes=limit)
        if fits:
            w.append_jpegs(files[:2], wave[:533])
        else:
            with pytest.raises(AviFull):
                w.append_jpegs(files[:2], wave[:533])
        w.close()
        assert (open(tmp_path / "g.avi", "rb").read() == data) == fits
    with pytest.raises(ValueError):
        AviWriter(str(tmp_path / "h.avi"), 16, 16, max_bytes=2 ** 31)


@pytest.mark.parametrize("fmt", [None, "f32", "s16"])
def test_fragments_of_a_second_writer_give_the_identical_file(tmp_path, fmt):
    """append_fragment's position arithmetic: fragments built by another writer's append_jpegs in batches of 1, 3, 8 and 2 frames, appended
    to a writer that only ever sees fragments, give the file one append_jpegs call gives"""
    files = make_files("c16", 8) + make_files("c16", 6)[::-1]
    wave = make_wave(4000)
    whole = write(tmp_path / "whole.avi", "c16", files, fmt, wave)
    kw = dict(audio_rate=None if fmt is None else 16000, audio_format=fmt or "f32")
    src, dst = AviWriter(str(tmp_path / "src.avi"), 16, 16, **kw), AviWriter(str(tmp_path / "dst.avi"), 16, 16, **kw)
    at = 0
    for n in (1, 3, 8, 2):
        a, b = src.span(at, n)
        data, index, nframes, nsamples, lv, la = src.append_jpegs(files[at:at + n], None if fmt is None else wave[a:b])
        assert nframes == n and nsamples == (b - a) and int(index[0, 2]) == 0 and index.shape == (n * (1 if fmt is None else 2), 4)
        dst.append_fragment(np.frombuffer(data, np.uint8), index, nframes, nsamples, lv, la)
        at += n
    src.close()
    dst.close()
    assert open(tmp_path / "dst.avi", "rb").read() == whole == open(tmp_path / "src.avi", "rb").read()
    P.parse(whole)
    with pytest.raises(ValueError):
        dst.append_fragment(data, index, nframes, nsamples, lv, la)                  # closed


def test_write_avi(tmp_path):
    files, wave = make_files("c32x48"), make_wave(4000)
    assert write_avi(str(tmp_path / "w.avi"), files, wave, batch=3) == 8
    assert open(tmp_path / "w.avi", "rb").read() == write(tmp_path / "a.avi", "c32x48", files, "f32", wave)
    assert write_avi(str(tmp_path / "n.avi"), files) == 8
    assert P.parse(open(tmp_path / "n.avi", "rb").read())["audio"] is None
    with pytest.raises(ValueError):
        write_avi(str(tmp_path / "x.avi"), files, wave[:2132])                    # 8 frames carry 2133 samples


def test_the_parser_is_strict(tmp_path):
    """the parser itself: every inconsistency it promises to catch, provoked on a good file"""
    files, wave = make_files("c16", 4), make_wave(4000)
    good = bytearray(write(tmp_path / "a.avi", "c16", files, "f32", wave))
    r = P.parse(good)

    def broken(edit):
        b = bytearray(good)
        edit(b)
        with pytest.raises(P.AviError):
            P.parse(b)

    def put(at, value):
        return lambda b: b.__setitem__(slice(at, at + 4), struct.pack("<I", value))

    first = r["first_chunk"]
    odd = next(k for k, (cc, off, p) in enumerate(r["chunks"]) if len(p) & 1)
    pad_at = first - 4 + r["chunks"][odd][1] + 8 + len(r["chunks"][odd][2])
    idx = len(good) - 16 * len(r["index"])
    broken(lambda b: b.append(0))                                                 # trailing bytes
    broken(put(4, len(good) - 8 + 2))                                             # RIFF size
    broken(put(16, struct.unpack_from("<I", good, 16)[0] + 2))                    # LIST hdrl size
    broken(put(first - 8, struct.unpack_from("<I", good, first - 8)[0] - 2))      # LIST movi size
    broken(lambda b: b.__setitem__(pad_at, 1))                                    # nonzero pad byte
    broken(put(idx + 8, 6))                                                       # index offset off a fourcc
    broken(put(idx + 12, 1060))                                                   # index length
    broken(lambda b: b.__setitem__(slice(idx, idx + 4), b"00dc"))                 # index ckid
    broken(lambda b: b.__delitem__(slice(len(b) - 16, len(b))))                   # an index entry gone (and the sizes with it)
    broken(put(32 + 16, 5))                                                       # dwTotalFrames
    broken(put(32 + 28, 100))                                                     # avih dwSuggestedBufferSize
    vstrh = 12 + 12 + 64 + 12 + 8
    broken(put(vstrh + 32, 3))                                                    # video dwLength
    broken(put(vstrh + 36, 100))                                                  # video dwSuggestedBufferSize
    astrh = vstrh + 56 + 48 + 12 + 8
    broken(put(astrh + 32, 1065))                                                 # audio dwLength
    broken(put(28, 52))                                                           # avih size
    assert good[24:28] == b"avih" and good[vstrh - 8:vstrh - 4] == b"strh" and good[astrh - 8:astrh - 4] == b"strh"
    assert good[vstrh:vstrh + 4] == b"vids" and good[astrh:astrh + 4] == b"auds"
