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


def host_fragment(tmp_path, geom, files, fmt, wave, frame0):
    """the fragment of frames frame0 .. of a file that already holds frame0 frames, built on the host"""
    from livespeechportraits_amd.video import AviWriter
    h, w, ch = GEOMETRIES[geom]
    out = AviWriter(str(tmp_path / "host.avi"), w, h, ch, audio_rate=None if fmt is None else 16000, audio_format=fmt or "f32")
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
