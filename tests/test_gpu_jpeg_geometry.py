"""The device JPEG encoder's format handles (frames of any size in 4:4:4, 4:2:2, 4:2:0 or grey: include/lspjpeg.h lspjpeg_create_format)
against Pillow's bytes: the frozen fixtures of tests/golden/jpeg_geometry.{json,npz} (tools/make_golden_jpeg_geometry.py), live Pillow where a
picture is not frozen (the model of tests/jpeg_geometry_model.py, pinned to Pillow by tests/test_jpeg_geometry_cpu.py, where Pillow is not
installed), the device decoder on our own files, and the render loops, the AVI route and the live pool at sizes that are no multiple of 16.
Every comparison is byte for byte."""
import functools
import io

import numpy as np
import pytest
import torch

import jpeg_decode_model as D
import jpeg_geometry_model as G
import jpeg_model as M
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def _fixtures():
    return G.load_fixtures(GOLDEN)


def _options(c):
    from livespeechportraits_amd.jpeg import JpegOptions
    return JpegOptions(c["quality"], bool(c["optimize"]), c["restart_rows"], c["restart_blocks"], "4:2:2" if c["format"] == "grey" else c["format"])


def _pillow_bytes(img, q, fmt, o=0, rows=0, blocks=0):
    try:
        from PIL import Image
    except ImportError:
        return G.encode(img, q, fmt, bool(o), rows, blocks)
    return G.pillow_bytes(Image, img, q, fmt, o, rows, blocks)


def _pillow_pixels(data):
    try:
        from PIL import Image
    except ImportError:
        return D.decode(data)
    return np.asarray(Image.open(io.BytesIO(data)))


@pytest.mark.parametrize("fmt", G.FORMATS)
def test_every_fixture_encodes_to_pillows_bytes(gpu_device, fmt):
    """every frozen file of the layout.  The three pictures of a geometry go through one call (with an odd width frames 1 and 2 of the batch start
    at odd addresses) and then one by one through the same handle"""
    from livespeechportraits_amd.jpeg import JpegEncoder
    _, cases, files = _fixtures()
    groups = {}
    for c in cases:
        if c["format"] == fmt:
            r = c["recipe"]
            groups.setdefault((r["h"], r["w"], r["channels"], _options(c)), []).append(c)
    bad, batched = [], 0
    for (h, w, ch, opts), group in groups.items():
        enc = JpegEncoder((h, w), ch, opts, gpu_device, max_batch=len(group))
        x = torch.from_numpy(np.stack([G.make_image(c["recipe"]) for c in group])).to(gpu_device)
        got = enc.encode(x)
        bad += [c["name"] for c, g in zip(group, got) if g != files[c["name"]]]
        if len(group) == 3:
            batched += 1
            bad += [c["name"] + " (alone)" for k, c in enumerate(group) if enc.encode(x[k:k + 1])[0] != files[c["name"]]]
        enc.close()
    assert not bad, bad
    assert batched == 30                                                                         # 15 sizes at two qualities


@pytest.mark.parametrize("h,w", [(100, 75), (64, 36), (36, 64), (50, 34), (33, 47)])
def test_noise_at_quality_95_on_the_large_sizes(gpu_device, h, w):
    """the pictures the fixture has no room for (every coefficient coded, dense stuffing), against the installed Pillow or the model"""
    from livespeechportraits_amd.jpeg import JpegEncoder, JpegOptions
    for fmt in G.FORMATS:
        ch = 1 if fmt == "grey" else 3
        imgs = np.stack([G.make_image(dict(kind="noise", h=h, w=w, channels=ch, seed=900 + k)) for k in range(3)])
        enc = JpegEncoder((h, w), ch, JpegOptions(95, subsampling="4:4:4" if ch == 1 else fmt), gpu_device, max_batch=3)
        assert enc.encode(torch.from_numpy(imgs).to(gpu_device)) == [_pillow_bytes(i, 95, fmt) for i in imgs], fmt
        enc.close()


@pytest.mark.parametrize("h,w,fmt,o,rows", [(33, 47, "4:2:0", 1, 1), (50, 34, "4:2:2", 0, 0), (17, 33, "4:4:4", 1, 0)])
def test_the_workspace_and_dst_content_on_entry_is_irrelevant(gpu_device, h, w, fmt, o, rows):
    """two different batches back to back through one handle, the workspace and dst filled with 0xFF in between: the files of the first run again"""
    from livespeechportraits_amd.jpeg import JpegEncoder, JpegOptions
    a = np.stack([G.make_image(dict(kind="smooth", h=h, w=w, channels=3, seed=s)) for s in (41, 42, 43)])
    b = np.stack([G.make_image(dict(kind="noise", h=h, w=w, channels=3, seed=s)) for s in (44, 45)])
    enc = JpegEncoder((h, w), 3, JpegOptions(75, bool(o), rows, 0, fmt), gpu_device, max_batch=3)
    xa, xb = torch.from_numpy(a).to(gpu_device), torch.from_numpy(b).to(gpu_device)
    first = (enc.encode(xa), enc.encode(xb))
    assert first[0] == [_pillow_bytes(i, 75, fmt, o, rows) for i in a] and first[1] == [_pillow_bytes(i, 75, fmt, o, rows) for i in b]
    enc._ws.fill_(0xFF)
    enc._dst.fill_(0xFF)
    assert (enc.encode(xa), enc.encode(xb)) == first


def test_capacity_under_load(gpu_device):
    """q100 uniform noise in 4:4:4 at 33 x 47, a batch of 8 (the largest files: every coefficient coded, dense 0xFF stuffing): within
    lspjpeg_capacity_bytes, and Pillow's bytes"""
    from livespeechportraits_amd.jpeg import JpegEncoder, JpegOptions
    imgs = np.stack([G.make_image(dict(kind="noise", h=33, w=47, channels=3, seed=70 + k)) for k in range(8)])
    enc = JpegEncoder((33, 47), 3, JpegOptions(100, subsampling="4:4:4"), gpu_device, max_batch=8)
    assert enc.capacity == 2 * ((6 * 5 * 3 * 1660 + 7) // 8) + 2
    enc._dst.fill_(0xA5)
    got = enc.encode(torch.from_numpy(imgs).to(gpu_device))
    sizes = [len(g) - len(enc.header) for g in got]
    assert max(sizes) <= enc.capacity and min(sizes) > 33 * 47 * 3 * 0.9, sizes
    dst = enc._dst.cpu().numpy()
    for k, n in enumerate(sizes):
        assert np.all(dst[k, n:] == 0xA5), k                                                     # nothing written behind a frame's bytes
    assert got == [_pillow_bytes(i, 100, "4:4:4") for i in imgs]


def test_todays_geometry_gives_the_plain_handles_bytes(gpu_device):
    from livespeechportraits_amd.jpeg import JpegEncoder, JpegOptions
    img = M.make_image(dict(kind="smooth", h=512, w=512, channels=3, seed=31))
    x = torch.from_numpy(img[None]).to(gpu_device)
    plain = JpegEncoder(512, 3, 75, gpu_device, max_batch=1)
    routed = JpegEncoder(512, 3, JpegOptions(75, subsampling="4:2:0"), gpu_device, max_batch=1)
    assert routed.header == plain.header and routed.capacity == plain.capacity and routed.encode(x) == plain.encode(x)
    grey = torch.from_numpy(img[None, :, :, 1].copy()).to(gpu_device)
    assert JpegEncoder(512, 1, JpegOptions(75, subsampling=0), gpu_device, max_batch=1).encode(grey) == JpegEncoder(512, 1, 75, gpu_device, max_batch=1).encode(grey)
    other = JpegEncoder(512, 3, JpegOptions(75, subsampling="4:4:4"), gpu_device, max_batch=1).encode(x)[0]
    assert other == _pillow_bytes(img, 75, "4:4:4") and other != plain.encode(x)[0]


def test_the_decoder_reads_our_files_as_pillow_does(gpu_device):
    """odd sizes in every layout, encoded here, decoded by JpegDecoder: the pixels Pillow decodes from the same bytes"""
    from livespeechportraits_amd.jpeg import JpegDecoder, JpegEncoder, JpegOptions, probe
    dec = JpegDecoder(gpu_device, max_side=128)
    for (h, w) in ((33, 47), (50, 34), (9, 23), (100, 75)):
        for fmt in G.FORMATS:
            comps, hs, vs = G.factors(fmt)
            img = G.make_image(dict(kind="smooth", h=h, w=w, channels=comps, seed=h))
            data = JpegEncoder((h, w), comps, JpegOptions(90, subsampling="4:2:0" if comps == 1 else fmt), gpu_device, max_batch=1).encode(torch.from_numpy(img[None]).to(gpu_device))[0]
            info = probe(data)
            assert (info.status, info.width, info.height, info.components, info.hsamp, info.vsamp) == (0, w, h, comps, hs, vs), (h, w, fmt)
            assert np.array_equal(dec.decode([data])[0].cpu().numpy(), _pillow_pixels(data)), (h, w, fmt)


def test_wrong_frames_are_refused_before_any_launch(gpu_device):
    from livespeechportraits_amd.jpeg import JpegEncoder, JpegOptions
    enc = JpegEncoder((33, 47), 3, JpegOptions(75, subsampling="4:2:2"), gpu_device, max_batch=2)
    enc._dst.fill_(0x5A)
    good = torch.zeros((2, 33, 47, 3), dtype=torch.uint8, device=gpu_device)
    for bad in (good[:, :32], torch.zeros((2, 47, 33, 3), dtype=torch.uint8, device=gpu_device), good.float(), good[..., 0], good.cpu(),
                torch.zeros((3, 33, 47, 3), dtype=torch.uint8, device=gpu_device), good[:, :, ::2], good.permute(0, 2, 1, 3)):
        with pytest.raises(ValueError):
            enc.encode(bad)
    torch.cuda.synchronize()
    assert bool((enc._dst == 0x5A).all())
    flat = torch.zeros(2 * 33 * 47 * 3 + 1, dtype=torch.uint8, device=gpu_device)
    odd = flat[1:].view(2, 33, 47, 3)                                                          # a batch that starts at an odd address: taken
    assert odd.data_ptr() % 2 == 1 and enc.encode(odd) == enc.encode(good)


# ---- the render loops -----------------------------------------------------------------------------------------------------------------------
from test_gpu_resize import _render_problem  # noqa: E402


@pytest.mark.parametrize("fmt,rows", [("4:4:4", 0), ("4:2:0", 1)])
def test_render_loops_at_a_size_that_is_no_multiple_of_16(gpu_device, tmp_path, fmt, rows):
    """the smallest generator of the render-loop JPEG tests (64 x 64 frames), out_size (360, 270): render_frames (host maps, two lanes),
    render_frames_from_landmarks, and the AVI route hand out Pillow's encoding of the frames the same call returns without jpeg_quality"""
    import avi_parser as P
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.jpeg import JpegOptions
    from livespeechportraits_amd.render_loop import render_frames, render_frames_from_landmarks
    from livespeechportraits_amd.video import AviWriter
    model, topo, c, lms, shs = _render_problem(tmp_path, gpu_device)
    opts = JpegOptions(75, restart_rows=rows, subsampling=fmt)
    feats, _ = synth.make_inputs(5, topo.size, seed=23, cand_batch=1)
    maps = lambda: (torch.from_numpy(f) for f in feats)
    plain = render_frames(model, maps(), c, batch=3, out_size=(360, 270))
    want = [_pillow_bytes(f, 75, fmt, 0, rows) for f in plain]
    assert plain[0].shape == (270, 360, 3) and render_frames(model, maps(), c, batch=3, out_size=(360, 270), jpeg_quality=opts) == want
    path = str(tmp_path / "odd.avi")
    with AviWriter(path, 360, 270, audio_rate=None) as w:
        assert render_frames(model, maps(), c, batch=3, out_size=(360, 270), jpeg_quality=opts, video=w) == []
    assert P.parse(open(path, "rb").read())["video"] == want
    kw = dict(pad=(1, 0, 0, 2), load_size=topo.size, batch=2, out_size=(360, 270))
    plain = render_frames_from_landmarks(model, lms, shs, c, **kw)
    pairs = render_frames_from_landmarks(model, lms, shs, c, jpeg_quality=opts, save_input=True, **kw)
    assert [p for p, _ in pairs] == [_pillow_bytes(f, 75, fmt, 0, rows) for f in plain]
    assert all(i[:2] == b"\xff\xd8" for _, i in pairs)                                          # the edge maps stay load_size, with the same options


# ---- live -------------------------------------------------------------------------------------------------------------------------------------
from test_gpu_landmarks import make_stage  # noqa: E402
from test_gpu_live import DEV, models, wave_of  # noqa: E402,F401  (models: the module-scoped fixture)
from test_gpu_live_pool import pool_of  # noqa: E402
from test_gpu_live_render import _avatar, generators  # noqa: E402,F401  (generators: the module-scoped fixture)


def test_a_live_recording_at_an_odd_size_in_422(models, generators, tmp_path):
    """one session, out_size (250, 187), recorded in 4:2:2: the strict parser takes the file, its chunks are Pillow's encoding of the frames the
    ticks hand out, and AviReader.frames gives the pixels Pillow decodes from them"""
    import avi_parser as P
    from livespeechportraits_amd.jpeg import JpegDecoder, JpegOptions
    from livespeechportraits_amd.live_render import LivePortraitPool
    from livespeechportraits_amd.video import AviReader, AviWriter
    gens, cand = generators
    meta, cfg = _avatar()
    opts = JpegOptions(75, subsampling="4:2:2")
    clip = wave_of(30 * 267, seed=73)
    pool = LivePortraitPool(pool_of(models, max_sessions=1), make_stage(cfg, meta, DEV, max_sessions=1), gens["f32"], cand, max_batch=4, record_quality=opts,
                            out_size=(250, 187))
    path = str(tmp_path / "live.avi")
    writer = AviWriter(path, 250, 187)
    sid = pool.open(np.zeros(12, np.float32), torch.Generator().manual_seed(74), video=writer)
    frames, step = [], 1500
    for at in range(0, len(clip), step):
        frames += list(pool.tick({sid: clip[at:at + step]}, finish=[sid] if at + step >= len(clip) else ())[sid][1].cpu().numpy())
    writer.close()
    want = [_pillow_bytes(f, 75, "4:2:2") for f in frames]
    assert len(frames) > 4 and frames[0].shape == (187, 250, 3)
    assert P.parse(open(path, "rb").read())["video"] == want
    got = list(AviReader(path).frames(decoder=JpegDecoder(DEV, max_side=256)))
    assert len(got) == len(want) and all(np.array_equal(g.cpu().numpy(), _pillow_pixels(d)) for g, d in zip(got, want))
