"""The device JPEG encoder with options (optimised Huffman tables, restart intervals: include/lspjpeg.h lspjpeg_create_opts) against
Pillow's bytes: the frozen fixtures of tests/golden/jpeg_options.{json,npz} (tools/make_golden_jpeg_options.py), live Pillow on the
product's own frame sizes (the model of tests/jpeg_options_model.py, pinned to Pillow by tests/test_jpeg_options_cpu.py, where Pillow is
not installed), the device decoder on our own files, and the AVI and live paths with options set.  Every comparison is byte for byte."""
import io
import json
import os

import numpy as np
import pytest
import torch

import jpeg_model as M
import jpeg_options_model as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SETS = [(o, r, b) for o in (0, 1) for (r, b) in ((0, 0), (1, 0), (2, 0), (0, 1), (0, 3))][1:]         # (optimize, restart_rows, restart_blocks)


def _fixtures():
    meta = json.load(open(os.path.join(GOLDEN, "jpeg_options.json")))
    return meta["cases"], dict(np.load(os.path.join(GOLDEN, "jpeg_options.npz")))


def _options(c):
    from livespeechportraits_amd.jpeg import JpegOptions
    return JpegOptions(c["quality"], bool(c["optimize"]), c["restart_rows"], c["restart_blocks"])


def _pillow_bytes(img, q, o, rows, blocks):
    try:
        from PIL import Image
    except ImportError:
        return O.encode(img, q, bool(o), O.restart_interval(img.shape[1], 1 if img.ndim == 2 else 3, rows, blocks))
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=q, optimize=bool(o), restart_marker_rows=rows, restart_marker_blocks=blocks)
    return b.getvalue()


def test_every_fixture_encodes_to_pillows_bytes(gpu_device):
    """every frozen file; the three batch*_c_32x48 pictures go through one call, so that every frame of the batch builds tables of its own"""
    from livespeechportraits_amd.jpeg import JpegEncoder
    cases, arrays = _fixtures()
    groups = {}
    for c in cases:
        r = c["recipe"]
        groups.setdefault((r["h"], r["w"], r["channels"], _options(c)), []).append(c)
    bad, batched = [], 0
    for (h, w, ch, opts), group in groups.items():
        enc = JpegEncoder((h, w), ch, opts, gpu_device, max_batch=len(group))
        got = enc.encode(torch.from_numpy(np.stack([O.make_image(c["recipe"]) for c in group])).to(gpu_device))
        bad += [c["name"] for c, g in zip(group, got) if g != arrays[c["name"]].tobytes()]
        batched += len(group) == 3
        enc.close()
    assert not bad, bad
    assert batched >= 9


@pytest.mark.parametrize("channels", [3, 1])
def test_product_frames_against_pillow(gpu_device, channels):
    """512 x 512, what the renderer (colour) and the rasteriser (edge map) hand over, for every option set at quality 75"""
    from livespeechportraits_amd.jpeg import JpegEncoder
    r = dict(kind="smooth", h=512, w=512, channels=3, seed=31) if channels == 3 else dict(kind="edges", h=512, w=512, channels=1, seed=32)
    img = M.make_image(r)
    x = torch.from_numpy(img[None]).to(gpu_device)
    for (o, rows, blocks) in SETS:
        enc = JpegEncoder(512, channels, 75, gpu_device, max_batch=1, optimize=bool(o), restart_rows=rows, restart_blocks=blocks)
        assert enc.encode(x)[0] == _pillow_bytes(img, 75, o, rows, blocks), (o, rows, blocks)
        enc.close()


@pytest.mark.parametrize("o,rows,blocks", [(1, 1, 0), (0, 0, 3), (1, 0, 0)])
def test_the_workspace_content_on_entry_is_irrelevant(gpu_device, o, rows, blocks):
    """two different batches back to back through one handle, the workspace filled with 0xFF in between: the files of the first run again"""
    from livespeechportraits_amd.jpeg import JpegEncoder
    a = np.stack([M.make_image(dict(kind="smooth", h=32, w=48, channels=3, seed=s)) for s in (41, 42, 43)])
    b = np.stack([M.make_image(dict(kind="noise", h=32, w=48, channels=3, seed=s)) for s in (44, 45)])
    enc = JpegEncoder((32, 48), 3, 75, gpu_device, max_batch=3, optimize=bool(o), restart_rows=rows, restart_blocks=blocks)
    xa, xb = torch.from_numpy(a).to(gpu_device), torch.from_numpy(b).to(gpu_device)
    first = (enc.encode(xa), enc.encode(xb))
    assert first[0] == [_pillow_bytes(i, 75, o, rows, blocks) for i in a] and first[1] == [_pillow_bytes(i, 75, o, rows, blocks) for i in b]
    enc._ws.fill_(0xFF)
    enc._dst.fill_(0xFF)
    again = (enc.encode(xa), enc.encode(xb))
    assert again == first


def test_the_decoder_gets_a_wave_per_mcu_row_and_the_same_pixels(gpu_device):
    """our restart_rows=1 file of a 512 x 512 frame has 32 restart intervals for the device decoder, and it and the optimize file decode to
    the pixels of the default file bit for bit (entropy coding does not change pixels)"""
    from livespeechportraits_amd.jpeg import JpegDecoder, JpegEncoder, probe
    img = M.make_image(dict(kind="smooth", h=512, w=512, channels=3, seed=33))
    x = torch.from_numpy(img[None]).to(gpu_device)
    files = {}
    for name, kw in (("default", {}), ("rows", dict(restart_rows=1)), ("optimize", dict(optimize=True)), ("both", dict(optimize=True, restart_rows=1))):
        files[name] = JpegEncoder(512, 3, 75, gpu_device, max_batch=1, **kw).encode(x)[0]
    assert probe(files["default"]).segments == 1 and probe(files["optimize"]).segments == 1
    assert probe(files["rows"]).segments == 32 and probe(files["both"]).segments == 32 and probe(files["rows"]).restart_interval == 32
    assert len(files["optimize"]) < len(files["default"]) < len(files["rows"])
    dec = JpegDecoder(gpu_device, max_side=512)
    want = dec.decode([files["default"]])[0]
    for name in ("rows", "optimize", "both"):
        assert torch.equal(dec.decode([files[name]])[0], want), name


# ---- AVI ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o,rows,blocks", [(1, 1, 0), (0, 0, 3)])
def test_avi_muxers_and_routes_with_options(gpu_device, tmp_path, o, rows, blocks):
    """3 frames of 32 x 32 with audio: lspavi_pack and lspavi_pack_multi build the fragment the host builds from Pillow's files (a constant
    header plus a slab of per-frame bytes, whatever the frame bytes start with), and both routes of VideoSink write one and the same file,
    which the strict parser takes and whose chunks are Pillow's files"""
    import avi_parser as P
    from livespeechportraits_amd.jpeg import JpegEncoder, JpegOptions
    from livespeechportraits_amd.video import AviWriter, DeviceMultiMuxer, DeviceMuxer, VideoSink
    opts = JpegOptions(75, bool(o), rows, blocks)
    pixels = np.stack([M.make_image(dict(kind=k, h=32, w=32, channels=3, seed=50 + i)) for i, k in enumerate(("smooth", "noise", "smooth"))])
    files = [_pillow_bytes(p, 75, o, rows, blocks) for p in pixels]
    wave = (np.sin(np.arange(4000) / 5.0) * 0.5).astype(np.float32)
    wave_dev, frames = torch.from_numpy(wave).to(gpu_device), torch.from_numpy(pixels).to(gpu_device)
    host = AviWriter(str(tmp_path / "frag.avi"), 32, 32, 3, fps=60, audio_rate=16000, audio_format="f32")
    a, b = host.span(0, 3)
    want = host.build_fragment(files, wave[a:b])
    host.close()
    enc = JpegEncoder(32, 3, opts, gpu_device, max_batch=3)
    assert enc.encode(frames) == files
    mux = DeviceMuxer(enc, "f32")
    mux.submit(frames, 0, wave_dev)
    data, index, *rest = mux.collect()
    assert data.tobytes() == want[0] and index.tobytes() == want[1].tobytes() and tuple(rest) == tuple(want[2:])
    multi = DeviceMultiMuxer(enc)
    (data, index, *rest), = multi.pack(frames, [(3, 0, "f32", wave_dev, 0, 0, wave.shape[0])])
    assert data.tobytes() == want[0] and index.tobytes() == want[1].tobytes() and tuple(rest) == tuple(want[2:])
    written = {}
    for route in ("device", "host"):
        path = str(tmp_path / (route + ".avi"))
        with AviWriter(path, 32, 32, 3, fps=60, audio_rate=16000, audio_format="f32") as out:
            sink = VideoSink(out, 32, opts, gpu_device, 3, wave_dev, wave, route)
            sink.submit(frames, 0)
            sink.collect()
        written[route] = open(path, "rb").read()
    assert written["device"] == written["host"]
    parsed = P.parse(written["device"])                                 # the strict parser: raises on anything out of place
    assert parsed["video"] == files and parsed["audio"].tobytes() == wave[a:b].tobytes()


# ---- live ---------------------------------------------------------------------------------------------------------------------------------
from test_gpu_landmarks import make_stage  # noqa: E402
from test_gpu_live import DEV, models, wave_of  # noqa: E402,F401  (models: the module-scoped fixture)
from test_gpu_live_pool import pool_of  # noqa: E402
from test_gpu_live_render import _avatar, generators  # noqa: E402,F401  (generators: the module-scoped fixture)


def test_live_ticks_and_recordings_with_options(models, generators, tmp_path):
    """One session per pool, the smallest pool the live-render tests use.  Pool A records on the device route with options and hands out
    the frames: its file's chunks are JpegEncoder.encode (same options) of those frames.  Pool B, the same session again on the host
    route, hands out files from tick(jpeg_quality=options): the files of A's frames; and it writes the file A wrote."""
    import avi_parser as P
    from livespeechportraits_amd.jpeg import JpegEncoder, JpegOptions
    from livespeechportraits_amd.live_render import LivePortraitPool
    from livespeechportraits_amd.video import AviWriter
    gens, cand = generators
    meta, cfg = _avatar()
    opts = JpegOptions(75, True, restart_rows=1)
    clip = wave_of(30 * 267, seed=71)
    enc = JpegEncoder(512, 3, opts, DEV, max_batch=4)

    def run(route, as_files):
        pool = LivePortraitPool(pool_of(models, max_sessions=1), make_stage(cfg, meta, DEV, max_sessions=1), gens["f32"], cand, max_batch=4,
                                record_quality=opts, record_route=route)
        assert pool.record_quality == opts
        path = str(tmp_path / (route + ".avi"))
        writer = AviWriter(path, 512, 512)
        sid = pool.open(np.zeros(12, np.float32), torch.Generator().manual_seed(72), video=writer)
        got, step = [], 1500
        for at in range(0, len(clip), step):
            last = at + step >= len(clip)
            start, out = pool.tick({sid: clip[at:at + step]}, finish=[sid] if last else (), jpeg_quality=opts if as_files else None)[sid]
            assert start == len(got)
            if as_files:
                got += out
            else:
                for g0 in range(0, len(out), 4):
                    got += enc.encode(out[g0:g0 + 4].contiguous())
        assert len(pool._jpeg) == (1 if as_files else 0)                # one encoder for the whole option set, however often it is named
        writer.close()
        return got, open(path, "rb").read()

    files_a, avi_a = run("device", False)
    files_b, avi_b = run("host", True)
    assert len(files_a) > 4 and files_a == files_b and avi_a == avi_b                         # more frames than one group of max_batch
    parsed = P.parse(avi_a)
    assert parsed["video"] == files_a
    from livespeechportraits_amd.jpeg import probe
    assert probe(files_a[0]).segments == 32 and probe(files_a[0]).default_tables == 0
