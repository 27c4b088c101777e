"""Recording inside LivePortraitPool.tick (livespeechportraits_amd/live_render.py): every recorded session's frames and their audio go to
the session's own AviWriter, muxed on the device from the audio rings (lspavi_pack_multi) or, on the "host" route, with JpegEncoder +
append_jpegs.  Nothing here has a tolerance: every file passes the strict parser, every video chunk is the file JpegEncoder gives for the
frame the same tick returned, every audio stream is the pushed samples bit for bit, and the two routes write identical files."""
import numpy as np
import pytest
import torch

import avi_parser as P
from test_avi_cpu import pcm16_rule
from test_gpu_landmarks import make_stage
from test_gpu_live import DEV, models, wave_of  # noqa: F401  (models: the module-scoped fixture)
from test_gpu_live_pool import pool_of
from test_gpu_live_render import _avatar, _pieces, generators  # noqa: F401  (generators: the module-scoped fixture)

pytestmark = pytest.mark.gpu

s = lambda f: f * 16000 // 60
nsamp = lambda frames: int(frames * 16000 / 60) + 1


def scenario(route, root, models, generators, reference):
    """Four sessions, opened some ticks apart, pushed unevenly:
      0  recorded from open(), with the edge maps' file as well; small pushes, so many ticks emit nothing for it
      1  recording starts mid-stream, 16-bit audio
      2  a frame of audio per tick; its first file holds one worst-case frame, so it fills at once and on_full hands out the second
      3  as 2, without an audio stream and without on_full: its recording stops when the file is full, the session goes on
    -> what was written and what was pushed; with ``reference`` also the JPEG files of every frame the ticks returned."""
    from livespeechportraits_amd.feature_map import FeatureMapRasteriser
    from livespeechportraits_amd.jpeg import JpegEncoder
    from livespeechportraits_amd.live_render import LivePortraitPool
    from livespeechportraits_amd.video import AviFull, AviWriter
    gens, cand = generators
    meta, cfg = _avatar()
    root.mkdir()
    pool = LivePortraitPool(pool_of(models, max_sessions=4), make_stage(cfg, meta, DEV, max_sessions=4), gens["f32"], cand, max_batch=4,
                            record_quality=75, record_route=route)
    assert pool.record_route == route and pool.ring_samples == pool.max_tick_samples + (18 + 40 + 4) * 267
    enc, enc_gray = JpegEncoder(512, 3, 75, DEV, max_batch=4), JpegEncoder(512, 1, 75, DEV, max_batch=4)
    raster = FeatureMapRasteriser(512, 18, torch.device(DEV))
    one_frame = 8 + len(enc.header) + enc.capacity + 1                  # a worst-case video chunk
    clips = {0: wave_of(nsamp(95), seed=41), 1: wave_of(nsamp(110), seed=42), 2: wave_of(nsamp(85), seed=43), 3: wave_of(nsamp(80), seed=44)}
    pieces = {0: _pieces(len(clips[0]), 200, top=400), 1: _pieces(len(clips[1]), 201, top=1500), 2: [267] * (len(clips[2]) // 267) + [len(clips[2]) % 267],
              3: [267] * (len(clips[3]) // 267) + [len(clips[3]) % 267]}
    start_tick = {0: 0, 1: 0, 2: 2, 3: 3}
    writers = {k: [] for k in ("0", "0i", "1", "2", "3")}

    def writer(name, **kw):
        w = AviWriter(str(root / ("%s_%d.avi" % (name, len(writers[name])))), 512, 512, **kw)
        writers[name].append(w)
        return w

    asked = []

    def on_full(sid, which):
        asked.append((sid, which))
        return writer("2")

    sids, pos, nframes = {}, {k: 0 for k in clips}, {k: 0 for k in clips}
    files = {k: [] for k in clips}
    gray = []
    record_from = None
    quiet = {k: 0 for k in clips}
    tick = 0
    while any(pieces.values()) or len(sids) < len(clips):
        for k in clips:
            if k not in sids and start_tick[k] <= tick:
                g = torch.Generator().manual_seed(60 + k)
                if k == 0:
                    sids[k] = pool.open(np.zeros(12, np.float32), g, video=writer("0"), video_input=writer("0i", channels=1, audio_rate=None))
                elif k == 2:
                    sids[k] = pool.open(np.zeros(12, np.float32), g, video=writer("2", max_bytes=326 + 8 + one_frame + 8 + 267 * 4 + 32 + 2048),
                                        on_full=on_full)
                elif k == 3:
                    sids[k] = pool.open(np.zeros(12, np.float32), g, video=writer("3", audio_rate=None, max_bytes=224 + 8 + one_frame + 16 + 2048))
                else:
                    sids[k] = pool.open(np.zeros(12, np.float32), g)
        if record_from is None and nframes[1] >= 12:                    # mid-stream: the file starts at the session's next emitted frame
            record_from = nframes[1]
            pool.record(sids[1], writer("1", audio_format="s16"))
        push, fin = {}, []
        for k in clips:
            if k in sids and pieces[k]:
                n = pieces[k].pop(0)
                push[sids[k]] = clips[k][pos[k]:pos[k] + n]
                pos[k] += n
                if not pieces[k]:
                    fin.append(sids[k])
        out = pool.tick(push, finish=fin)
        assert set(out) == set(push)
        by = {sid: k for k, sid in sids.items()}
        at = 0
        for sid in sorted(out):
            start, frames = out[sid]
            k = by[sid]
            assert start == nframes[k] and frames.is_cuda
            quiet[k] += nframes[k] > 0 and len(frames) == 0 and not fin
            if reference:
                for g0 in range(0, len(frames), 4):
                    files[k] += enc.encode(frames[g0:g0 + 4].contiguous())
                if k == 0 and len(frames):
                    maps = raster.rasterise_points(pool.last_points[at:at + len(frames)].contiguous(), as_uint8=True)
                    for g0 in range(0, len(frames), 4):
                        gray += enc_gray.encode(maps[g0:g0 + 4])
            at += len(frames)
            nframes[k] += len(frames)
        tick += 1
    assert not pool.open_sessions and not pool._rec
    assert quiet[0] >= 10, quiet                                        # a recorded session that emitted nothing in some ticks
    assert asked == [(sids[2], "video")]
    assert set(pool.recording_stopped) == {sids[3]} and isinstance(pool.recording_stopped[sids[3]], AviFull)
    for ws in writers.values():
        for w in ws:
            w.close()
    data = {name: [open(w.path, "rb").read() for w in ws] for name, ws in writers.items()}
    return dict(data=data, clips=clips, nframes=nframes, files=files, gray=gray, record_from=record_from)


@pytest.fixture(scope="module")
def runs(models, generators, tmp_path_factory):
    root = tmp_path_factory.mktemp("record")
    return {route: scenario(route, root / route, models, generators, reference=route == "device") for route in ("device", "host")}


def test_every_file_holds_the_ticks_own_frames_and_the_pushed_audio(runs):
    r = runs["device"]
    clips, files, total = r["clips"], r["files"], r["nframes"]
    assert min(total.values()) >= 60 and all(len(files[k]) == total[k] for k in files)
    parsed = {name: [P.parse(d) for d in ds] for name, ds in r["data"].items()}             # the strict parser: raises on anything out of place
    assert [len(v) for v in parsed.values()] == [1, 1, 1, 2, 1]

    def audio_is(p, clip, first, n, fmt="f32"):
        want = clip[first:first + s(n)]
        assert len(p["video"]) == n and p["audio_counts"] == [s(k + 1) - s(k) for k in range(n)]
        if fmt == "f32":
            assert p["audio"].dtype == np.float32 and p["audio"].tobytes() == want.tobytes()
        else:
            assert np.array_equal(p["audio"], pcm16_rule(want))

    # 0: from open(), every frame; the edge maps beside it
    p = parsed["0"][0]
    assert p["video"] == files[0]
    audio_is(p, clips[0], 0, total[0])
    assert parsed["0i"][0]["video"] == r["gray"] and len(r["gray"]) == total[0] and parsed["0i"][0]["audio"] is None
    # 1: from the frame that was next when record() was called; sample0 = s(that frame)
    F = r["record_from"]
    p = parsed["1"][0]
    assert 12 <= F < total[1] - 40 and p["video"] == files[1][F:]
    audio_is(p, clips[1], s(F), total[1] - F, "s16")
    # 2: the first file took what fitted, the second starts at the next frame with sample0 = s(that frame)
    a, b = parsed["2"]
    n1 = len(a["video"])
    assert 1 <= n1 <= 4 and a["video"] + b["video"] == files[2]
    audio_is(a, clips[2], 0, n1)
    audio_is(b, clips[2], s(n1), total[2] - n1)
    # 3: stopped when its file was full; what it holds is the session's first frames
    p = parsed["3"][0]
    assert 1 <= len(p["video"]) <= 4 and p["video"] == files[3][:len(p["video"])] and p["audio"] is None


def test_both_routes_write_identical_files(runs):
    assert runs["device"]["nframes"] == runs["host"]["nframes"]
    for name, ds in runs["device"]["data"].items():
        assert ds == runs["host"]["data"][name], name


def test_recording_refusals(models, generators, tmp_path):
    from livespeechportraits_amd.live_render import LivePortraitPool
    from livespeechportraits_amd.video import AviWriter
    gens, cand = generators
    meta, cfg = _avatar()
    stage = lambda: make_stage(cfg, meta, DEV, max_sessions=1)
    with pytest.raises(ValueError, match="record_route"):
        LivePortraitPool(pool_of(models, max_sessions=1), stage(), gens["f32"], cand, record_route="device")
    with pytest.raises(ValueError, match="record_route"):
        LivePortraitPool(pool_of(models, max_sessions=1), stage(), gens["f32"], cand, record_quality=75, record_route="disk")
    plain = LivePortraitPool(pool_of(models, max_sessions=1), stage(), gens["f32"], cand)
    assert plain.record_quality is None and not hasattr(plain, "_ring")                    # the defaults allocate nothing
    ok = AviWriter(str(tmp_path / "ok.avi"), 512, 512)
    with pytest.raises(ValueError, match="record_quality"):
        plain.open(np.zeros(12, np.float32), video=ok)
    assert not plain.open_sessions
    pool = LivePortraitPool(pool_of(models, max_sessions=1), stage(), gens["f32"], cand, record_quality=75)
    assert pool.record_route in ("device", "host")
    bad = {"size": AviWriter(str(tmp_path / "a.avi"), 256, 256), "gray": AviWriter(str(tmp_path / "b.avi"), 512, 512, channels=1),
           "fps": AviWriter(str(tmp_path / "c.avi"), 512, 512, fps=30), "rate": AviWriter(str(tmp_path / "d.avi"), 512, 512, audio_rate=22050)}
    for name, w in bad.items():
        with pytest.raises(ValueError, match="video"):
            pool.open(np.zeros(12, np.float32), video=w)
        assert not pool.open_sessions, name
    with pytest.raises(ValueError, match="video_input"):
        pool.open(np.zeros(12, np.float32), video=ok, video_input=AviWriter(str(tmp_path / "e.avi"), 512, 512))
    with pytest.raises(ValueError, match="go with video"):
        pool.open(np.zeros(12, np.float32), video_input=ok)
    sid = pool.open(np.zeros(12, np.float32), video=ok)
    with pytest.raises(ValueError, match="already"):
        pool.record(sid, AviWriter(str(tmp_path / "f.avi"), 512, 512))
    pool.stop_recording(sid)
    pool.record(sid, ok)
    with pytest.raises(KeyError):
        pool.record(sid + 7, ok)
    out = pool.tick({sid: np.zeros(300, np.float32)})
    assert tuple(out[sid][1].shape) == (0, 512, 512, 3) and ok.nframes == 0
    pool.close(sid)
    assert not pool._rec and not pool._book
