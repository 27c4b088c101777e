"""The device muxer (include/lspavi.h, livespeechportraits_amd/video.py DeviceMuxer) against AviWriter's host fragment builder, which
tests/test_avi_cpu.py pins on the strict parser and on Pillow: whole fragment and index, byte for byte.  The frames' bytes are those of
tests/jpeg_model.py.  Nothing here has a tolerance."""
import argparse

import numpy as np
import pytest
import torch

import avi_parser as P
import jpeg_model as M
from conftest import golden_problem
from test_avi_cpu import GEOMETRIES, SPECIAL, pcm16_rule

pytestmark = pytest.mark.gpu


def images(geom, n):
    h, w, ch = GEOMETRIES[geom]
    return np.stack([np.random.default_rng(seed).integers(0, 256, (h, w, 3) if ch == 3 else (h, w), dtype=np.uint8) for seed in range(n)])


def wave_of(n, seed=3):
    x = (np.random.default_rng(seed).standard_normal(n) * 0.4).astype(np.float32)
    for at in range(0, n - SPECIAL.size, 131):                  # NaN, +-1.5, +-1.0, infinities and rounding ties in every chunk, at every phase of a 16-byte piece
        x[at:at + SPECIAL.size] = SPECIAL
    return x


def host_fragment(tmp_path, geom, files, fmt, wave, frame0, rate=16000, fps=60):
    """the fragment of frames frame0 .. of a file that already holds frame0 frames, built on the host"""
    from livespeechportraits_amd.video import AviWriter
    h, w, ch = GEOMETRIES[geom]
    out = AviWriter(str(tmp_path / "host.avi"), w, h, ch, fps=fps, audio_rate=None if fmt is None else rate, audio_format=fmt or "f32")
    if frame0:
        a, b = out.span(0, frame0)
        out.append_jpegs([files[0]] * frame0, None if fmt is None else wave[a:b])
    a, b = out.span(frame0, len(files))
    frag = out.build_fragment(files, None if fmt is None else wave[a:b])
    out.close()
    return frag


@pytest.mark.parametrize("fmt", [None, "f32", "s16"])
@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_device_fragment_equals_the_host_fragment(gpu_device, tmp_path, geom, fmt):
    from livespeechportraits_amd.jpeg import JpegEncoder
    from livespeechportraits_amd.video import DeviceMuxer
    h, w, ch = GEOMETRIES[geom]
    batches = (1, 3, 8, 64) if geom == "c16" else (1, 3, 8)
    pixels = images(geom, max(batches))
    files = [M.encode(p, 75) for p in pixels]
    assert {len(f) & 1 for f in files[:8]} == {0, 1}
    wave = wave_of(20000)
    wave_dev = torch.from_numpy(wave).to(gpu_device)
    frames_dev = torch.from_numpy(pixels).to(gpu_device)
    for batch in batches:
        enc = JpegEncoder((h, w), ch, 75, gpu_device, max_batch=batch)
        mux = DeviceMuxer(enc, fmt)
        for frame0 in (0, 7):                                    # frame 0 carries 266 samples, frame 7 carries 267
            want = host_fragment(tmp_path, geom, files[:batch], fmt, wave, frame0)
            mux._out.fill_(0xA5)
            got = []
            for _ in range(2):                                  # twice into the same buffer, not refilled: no dependence on prior content
                mux.submit(frames_dev[:batch], frame0, None if fmt is None else wave_dev)
                data, index, nframes, nsamples, lv, la = mux.collect()
                got.append((data.tobytes(), index.tobytes(), nframes, nsamples, lv, la))
            where = (geom, fmt, batch, frame0)
            assert got[0] == got[1], where
            assert got[0][2:] == want[2:], where
            assert got[0][1] == want[1].tobytes(), where
            assert got[0][0] == want[0], where
            total = len(want[0])
            tail = mux._out[total:].cpu().numpy()
            assert tail.size >= 16 and (tail == 0xA5).all(), where           # bytes at or above the total are never touched
            assert mux._out[:total].cpu().numpy().tobytes() == want[0], where
        if fmt == "s16" and batch == 8:
            a = 7 * 16000 // 60
            pcm = b"".join(want[0][int(o) + 8:int(o) + 8 + int(n)] for ck, _, o, n in want[1] if ck == 0x62773130)
            assert np.array_equal(np.frombuffer(pcm, "<i2"), pcm16_rule(wave[a:a + len(pcm) // 2]))
        enc.close()


def test_a_waveform_one_sample_short_is_refused(gpu_device, tmp_path):
    """frames 7, 8, 9 end at sample 10 * 16000 // 60: a waveform one sample shorter is refused on the host side of the call, on both routes;
    nothing is enqueued for collect() and nothing is appended"""
    from livespeechportraits_amd import _native as N
    from livespeechportraits_amd.video import AviWriter, VideoSink, clip_audio
    frames_dev = torch.from_numpy(images("c16", 3)).to(gpu_device)
    need = 10 * 16000 // 60
    out = AviWriter(str(tmp_path / "a.avi"), 16, 16)
    for route in ("device", "host"):
        dev, host = clip_audio(out, wave_of(need)[:need - 1], gpu_device)
        sink = VideoSink(out, 16, 75, gpu_device, 3, dev, host, route)
        with pytest.raises((ValueError, N.LspaviError), match="samples"):
            sink.submit(frames_dev, 7)
        with pytest.raises(RuntimeError, match="nothing submitted"):
            (sink.mux if route == "device" else sink.enc).collect()
    dev, _ = clip_audio(out, wave_of(need), gpu_device)                       # exactly enough: accepted
    sink = VideoSink(out, 16, 75, gpu_device, 3, dev, None, "device")
    sink.mux.submit(frames_dev, 7, dev)
    assert sink.mux.collect()[2:4] == (3, need - 7 * 16000 // 60)
    assert out.nframes == 0 and out.nsamples == 0
    out.close()
    assert P.parse(open(tmp_path / "a.avi", "rb").read())["chunks"] == []


def _c16_batch(gpu_device, batch=3):
    """(device frames, their files) of ``batch`` 16x16x3 images"""
    pixels = images("c16", batch)
    return torch.from_numpy(pixels).to(gpu_device), [M.encode(p, 75) for p in pixels]


def _pack_and_compare(gpu_device, tmp_path, fmt, frame0, wave, rate=16000, fps=60):
    """one batch of 3 through DeviceMuxer with exactly ``wave`` as the clip's waveform: fragment, index and counts equal the host's"""
    from livespeechportraits_amd.jpeg import JpegEncoder
    from livespeechportraits_amd.video import DeviceMuxer
    frames_dev, files = _c16_batch(gpu_device)
    enc = JpegEncoder((16, 16), 3, 75, gpu_device, max_batch=3)
    mux = DeviceMuxer(enc, fmt, rate=rate, fps=fps)
    want = host_fragment(tmp_path, "c16", files, fmt, wave, frame0, rate, fps)
    mux._out.fill_(0xA5)
    mux.submit(frames_dev, frame0, torch.from_numpy(wave).to(gpu_device))
    data, index, *rest = mux.collect()
    where = (fmt, frame0, rate, fps)
    assert tuple(rest) == tuple(want[2:]), where
    assert index.tobytes() == want[1].tobytes(), where
    assert data.tobytes() == want[0], where
    tail = mux._out[len(want[0]):].cpu().numpy()
    assert tail.size >= 16 and (tail == 0xA5).all(), where
    enc.close()
    return want


@pytest.mark.parametrize("frame0", [0, 7])
@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_a_waveform_that_ends_where_the_batch_ends(gpu_device, tmp_path, fmt, frame0):
    """wave_samples == s(frame0 + 3): the batch's last sample is the waveform's last, so the one run's ring is full to its last sample"""
    n = (frame0 + 3) * 16000 // 60
    want = _pack_and_compare(gpu_device, tmp_path, fmt, frame0, wave_of(n)[:n])
    assert want[3] == n - frame0 * 16000 // 60


@pytest.mark.parametrize("frame0,n", [(0, 1), (1, 2)])
@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_fewer_samples_than_frames(gpu_device, tmp_path, fmt, frame0, n):
    """30 samples/s at 60 frames/s: frames carry 0, 1, 0, 1 .. samples, so every other '01wb' chunk is empty and a 16-byte piece can span
    three chunks; the waveform holds exactly the ``n`` samples frames frame0 .. frame0 + 2 end at"""
    wave = np.array([0.25, -1.5], np.float32)[:n]
    want = _pack_and_compare(gpu_device, tmp_path, fmt, frame0, wave, rate=30, fps=60)
    lengths = [int(n_) for ck, _, _, n_ in want[1] if ck == 0x62773130]
    bps = 4 if fmt == "f32" else 2
    assert lengths == [bps * ((frame0 + k) & 1) for k in range(3)]


@pytest.mark.parametrize("fmt", [None, "f32"])
def test_lspavi_pack_writes_what_its_header_says_and_no_more(gpu_device, tmp_path, fmt):
    """The library called directly, batch 3, every buffer longer than include/lspavi.h asks for and prefilled with 0xA5: status is 4
    words, the index `chunk count` rows, the workspace lspavi_workspace_bytes(3) bytes, the output the fragment's length.  A refused call
    (the waveform one sample short) leaves all four exactly as they were."""
    import ctypes
    from livespeechportraits_amd import _native as N
    from livespeechportraits_amd.jpeg import JpegEncoder
    frames_dev, files = _c16_batch(gpu_device)
    enc = JpegEncoder((16, 16), 3, 75, gpu_device, max_batch=3)
    lib, c = N.load(), ctypes.c_void_p
    frame0 = 7 if fmt else 0
    need = (frame0 + 3) * 16000 // 60
    wave = wave_of(need + 40)
    wave_dev = torch.from_numpy(wave).to(gpu_device)
    want = host_fragment(tmp_path, "c16", files, fmt, wave, frame0)
    total, nch = len(want[0]), len(want[1])
    assert nch == (6 if fmt else 3)
    code = N.AVI_AUDIO_FORMATS[fmt]
    capacity = int(lib.lspavi_capacity_bytes(len(enc.header), enc.capacity, 3, code, 16000, 60))
    ws_bytes = int(lib.lspavi_workspace_bytes(3))
    assert capacity >= total + 16 and ws_bytes > 0
    header = torch.frombuffer(bytearray(enc.header + b"\0" * (-len(enc.header) % 4)), dtype=torch.uint8).to(gpu_device)
    status = torch.full((16,), -1515870811, dtype=torch.int32, device=gpu_device)          # 0xA5A5A5A5
    index = torch.full((2 * 3 + 4, 4), -1515870811, dtype=torch.int32, device=gpu_device)
    ws = torch.full((ws_bytes + 256,), 0xA5, dtype=torch.uint8, device=gpu_device)
    out = torch.full((capacity,), 0xA5, dtype=torch.uint8, device=gpu_device)
    assert enc.enqueue(frames_dev) == 3
    dst, sizes = enc.slab
    stream = torch.cuda.current_stream(gpu_device)

    def pack(nwave):
        rc = lib.lspavi_pack(c(header.data_ptr()), len(enc.header), c(dst.data_ptr()), enc.capacity, c(sizes.data_ptr()), 3,
                             c(wave_dev.data_ptr() if fmt else None), nwave if fmt else 0, frame0, 16000, 60, code, c(out.data_ptr()), capacity,
                             c(index.data_ptr()), c(status.data_ptr()), c(ws.data_ptr()), ws_bytes, c(stream.cuda_stream))
        torch.cuda.synchronize()
        return rc, [t.cpu().numpy().copy() for t in (status, index, ws, out)]

    if fmt:
        rc, got = pack(need - 1)
        assert rc == -1 and "need %d samples, the waveform has %d" % (need, need - 1) in lib.lspavi_last_error().decode()
        assert all((g.view(np.uint8) == 0xA5).all() for g in got), "a refused call wrote to a device buffer"
    rc, (st, ix, w, o) = pack(need)
    assert rc == 0, lib.lspavi_last_error().decode()
    st, ix = st.view(np.uint32), ix.view(np.uint32)
    assert st[:4].tolist() == [total, nch, want[4], want[5]]
    assert (st[4:] == 0xA5A5A5A5).all()
    assert ix[:nch].tobytes() == want[1].tobytes()
    assert (ix[nch:] == 0xA5A5A5A5).all()
    assert (w[ws_bytes:] == 0xA5).all()
    assert o[:total].tobytes() == want[0]
    assert (o[total:] == 0xA5).all()
    enc.close()


def _model(tmp_path, case="normal_s64_b3"):
    import livespeechportraits_amd as L
    meta, _, topo, sd, _, cand = golden_problem(case)
    opt = argparse.Namespace(model="feature2face", gpu_ids=[0], isTrain=False, size=meta["variant"], ngf=meta["ngf"],
                             n_downsample_G=meta["num_downs"], fp16=0, checkpoints_dir=str(tmp_path), name="t", load_epoch="none", verbose=False)
    model = L.create_model(opt)
    model._g().load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    model.eval()
    return model, topo, cand


def _check_clip(data, files, wave, nframes=5):
    r = P.parse(data)
    assert len(r["video"]) == nframes and r["video"] == files                   # in order, and the very files the loop hands out
    n = nframes * 16000 // 60
    assert r["audio"].dtype == np.float32 and r["audio"].tobytes() == wave[:n].tobytes()
    assert r["audio_counts"] == [(k + 1) * 16000 // 60 - k * 16000 // 60 for k in range(nframes)]
    return r


def test_render_loops_write_the_clip(gpu_device, tmp_path):
    """5 frames at batch 2 (ragged last batch) from landmarks and from feature maps (two lanes, one lane, both routes): the file parses,
    holds the frames in order, each chunk is the file the same call returns with jpeg_quality=75 and no video, the audio is the clip's"""
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.render_loop import render_frames, render_frames_from_landmarks
    from livespeechportraits_amd.video import AviWriter
    model, topo, cand = _model(tmp_path)
    assert model.supports_replicas()
    S = topo.size
    rng = np.random.default_rng(4)
    lms = [S / 2 + rng.normal(0, S / 8, (73, 2)) for _ in range(5)]
    shs = [np.stack([np.linspace(0, S, 18), np.full(18, S - 10.0)], 1) for _ in range(5)]
    c = torch.from_numpy(cand[:1]).to(gpu_device)               # the golden case stores one candidate stack per frame
    wave = wave_of(5 * 16000 // 60 + 40)
    kw = dict(pad=(1, 0, 0, 2), load_size=S, batch=2)

    files = render_frames_from_landmarks(model, lms, shs, c, jpeg_quality=75, **kw)
    assert len(files) == 5 and len(set(files)) == 5
    seen = []
    with AviWriter(str(tmp_path / "lm.avi"), S, S) as w:
        assert render_frames_from_landmarks(model, lms, shs, c, video=w, audio=torch.from_numpy(wave), on_frame=lambda i, f: seen.append((i, f)), **kw) == []
    assert seen == [(i, None) for i in range(5)]
    lm_file = open(tmp_path / "lm.avi", "rb").read()
    _check_clip(lm_file, files, wave)
    with AviWriter(str(tmp_path / "lm_host.avi"), S, S) as w:
        assert render_frames_from_landmarks(model, lms, shs, c, video=w, audio=wave, video_route="host", **kw) == []
    assert open(tmp_path / "lm_host.avi", "rb").read() == lm_file

    # the edge maps' file next to it
    pairs = render_frames_from_landmarks(model, lms, shs, c, jpeg_quality=75, save_input=True, **kw)
    with AviWriter(str(tmp_path / "p.avi"), S, S) as w, AviWriter(str(tmp_path / "i.avi"), S, S, channels=1, audio_rate=None) as wi:
        render_frames_from_landmarks(model, lms, shs, c, video=w, audio=wave, video_input=wi, save_input=True, **kw)
    assert open(tmp_path / "p.avi", "rb").read() == lm_file
    assert P.parse(open(tmp_path / "i.avi", "rb").read())["video"] == [i for _, i in pairs]

    # feature maps: two lanes, one lane, the host route -- one file
    feats, _ = synth.make_inputs(5, S, seed=23, cand_batch=1)
    maps = lambda: (torch.from_numpy(f) for f in feats)
    files = render_frames(model, maps(), c, batch=2, jpeg_quality=75)
    got = {}
    for name, extra in (("two", {}), ("one", {"streams": 1}), ("host", {"video_route": "host"})):
        with AviWriter(str(tmp_path / (name + ".avi")), S, S) as w:
            assert render_frames(model, maps(), c, batch=2, video=w, audio=wave, **extra) == []
        got[name] = open(tmp_path / (name + ".avi"), "rb").read()
    _check_clip(got["two"], files, wave)
    assert got["one"] == got["two"] == got["host"]

    # one sample short for the last batch: raises, and the file holds what came before, nothing of that batch
    w = AviWriter(str(tmp_path / "short.avi"), S, S)
    with pytest.raises(Exception) as e:
        render_frames_from_landmarks(model, lms, shs, c, video=w, audio=wave[:5 * 16000 // 60 - 1], **kw)
    assert "samples" in str(e.value) and w.nframes == 4
    w.close()
    torch.cuda.synchronize()
    r = P.parse(open(tmp_path / "short.avi", "rb").read())
    assert len(r["video"]) == 4 and r["audio"].tobytes() == wave[:4 * 16000 // 60].tobytes()
