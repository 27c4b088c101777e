"""The PNG encoder on the device (include/lsppngenc.h, png.PngEncoder, render_frames(png=), LivePortraitPool.tick(png=)): the device's files equal
the host twin's (lsppng_enc_host_file, pinned to Pillow's and the strict decoder's pixels by tests/test_png_encode_cpu.py) bit for bit, and what
comes back from them, through PngDecoder on the device or through Pillow, equals what went in.  No tolerance anywhere.  None of this exists on the
parent commit: the whole file fails there."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import png_decode_cases as DK
import png_encode_cases as K

pytestmark = pytest.mark.gpu


def _pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)))


@pytest.fixture(scope="module")
def twins():
    """name -> (pixels, level, filter, the host twin's file)"""
    from livespeechportraits_amd import png
    return {name: (px, level, f, png.host_file(px, level=level, filter=f)) for name, px, level, f in K.cases()}


def _encoder(px, device, level=1, f=None, max_batch=1):
    from livespeechportraits_amd.png import PngEncoder
    return PngEncoder(px.shape[:2], 3 if px.ndim == 3 else 1, device, max_batch=max_batch, level=level, filter=f)


def test_every_case_equals_the_host_twin(gpu_device, twins):
    bad = []
    for name, (px, level, f, want) in twins.items():
        enc = _encoder(px, gpu_device, level, f)
        got = enc.encode(torch.from_numpy(px[None]).to(gpu_device))
        assert int(enc._sizes_host[0]) == len(want) - K.HEADER and enc.capacity == K.capacity(px), name
        if got != [want]:
            bad.append(name)
        enc.close()
    assert not bad, bad


@pytest.mark.parametrize("batch", [1, 3, 8])
@pytest.mark.parametrize("channels", [3, 1])
def test_batches_of_different_frames_and_a_reused_handle(gpu_device, batch, channels):
    """every slot of a batch is the file of its frame alone; a second call with other frames, over a poisoned workspace, leaves nothing of the first"""
    from livespeechportraits_amd import png
    kinds = [K.smooth, K.noise, K.smooth, lambda h, w, c, s: np.zeros((h, w, 3) if c == 3 else (h, w), np.uint8)]
    frames = np.stack([kinds[k % 4](96, 150, channels, 200 + k) for k in range(8)])
    if channels == 1:
        frames[4] = K.line_drawing(150, 10, 9)[:96]
    want = [png.host_file(f) for f in frames]
    enc = _encoder(frames[0], gpu_device, max_batch=8)
    assert enc.encode(torch.from_numpy(frames[:batch]).to(gpu_device)) == want[:batch]
    for byte in (0xFF, 0xA5):
        enc._ws.fill_(byte)
        enc._dst.fill_(byte)
        enc._sizes.fill_(-1)
        rolled = np.roll(frames, 3, axis=0)[:batch]
        assert enc.encode(torch.from_numpy(rolled).to(gpu_device)) == [want[(k - 3) % 8] for k in range(batch)], byte
    alone = _encoder(frames[0], gpu_device)
    assert alone.encode(torch.from_numpy(frames[batch - 1:batch]).to(gpu_device)) == [want[batch - 1]]


@pytest.fixture(scope="module")
def big_files(gpu_device):
    """the device-made files of the four 512 x 512 RGB candidates and of a 512 x 512 edge map, with their pixels"""
    from livespeechportraits_amd import png
    rgb = np.stack([np.asarray(Image.open(io.BytesIO(data)).convert("RGB")) for _, data in DK.candidates()])
    edges = K.line_drawing()
    files = _encoder(rgb[0], gpu_device, max_batch=4).encode(torch.from_numpy(rgb).to(gpu_device))
    edge_file, = _encoder(edges, gpu_device).encode(torch.from_numpy(edges[None]).to(gpu_device))
    assert files == [png.host_file(p) for p in rgb] and edge_file == png.host_file(edges)
    return rgb, files, edges, edge_file


def test_the_device_decoder_reads_the_device_made_files(gpu_device, big_files, twins):
    from livespeechportraits_amd.png import PngDecoder
    rgb, files, edges, edge_file = big_files
    small = twins["tiny_17x5_c3_l1"]
    tiny, = _encoder(small[0], gpu_device).encode(torch.from_numpy(small[0][None]).to(gpu_device))
    dec = PngDecoder(gpu_device, max_side=512, max_batch=8)
    out = dec.decode([files[0], edge_file, tiny])
    assert dec.last_status == [0, 0, 0]
    for got, want in zip(out, (rgb[0], edges, small[0])):
        assert got.dtype == torch.uint8 and torch.equal(got, torch.from_numpy(want).to(gpu_device))


def test_load_candidates_takes_four_device_made_files(gpu_device, big_files):
    from livespeechportraits_amd.candidates import load_candidates, normalisation_table
    rgb, files, _, _ = big_files
    got = load_candidates(files, gpu_device, png=True)
    want = np.concatenate([normalisation_table()[p].transpose(2, 0, 1) for p in rgb])
    assert got.shape == (1, 12, 512, 512) and np.array_equal(got[0].cpu().numpy(), want)


# ---- the render loops ----------------------------------------------------------------------------------------------------------------------
from test_gpu_jpeg import _model  # noqa: E402


@pytest.mark.parametrize("out_size", [None, 256])
def test_render_frames_hands_out_lossless_files(gpu_device, tmp_path, out_size):
    """render_frames(png=True) over 11 maps (batches 4, 4, 3): Pillow's decode of every file is the frame the same call returns without png"""
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.png import PngOptions, save_images
    from livespeechportraits_amd.render_loop import render_frames
    model, topo, cand = _model(tmp_path, "normal_s64_b3")
    feats, _ = synth.make_inputs(11, topo.size, seed=23, cand_batch=1)
    c = torch.from_numpy(cand[:1]).to(gpu_device)
    kw = dict(batch=4, out_size=out_size)
    plain = render_frames(model, (torch.from_numpy(f) for f in feats), c, **kw)
    files = render_frames(model, (torch.from_numpy(f) for f in feats), c, png=True, **kw)
    assert len(files) == 11 and all(isinstance(f, bytes) for f in files)
    for k in range(11):
        assert np.array_equal(_pillow(files[k]), plain[k]), k
    seen = []
    render_frames(model, (torch.from_numpy(f) for f in feats), c, png=PngOptions(1, None), on_frame=lambda i, b: seen.append((i, b)), **kw)
    assert [i for i, _ in seen] == list(range(11)) and [b for _, b in seen] == files
    stored = render_frames(model, (torch.from_numpy(f) for f in feats[:2]), c, png=PngOptions(level=0), **kw)
    assert all(np.array_equal(_pillow(s), p) for s, p in zip(stored, plain)) and len(stored[0]) == K.HEADER + K.capacity(plain[0])
    paths = save_images(str(tmp_path / "out"), files[:2], index0=4)
    assert [os.path.basename(p) for p in paths] == ["pred_5.png", "pred_6.png"] and open(paths[1], "rb").read() == files[1]
    with pytest.raises(ValueError):
        render_frames(model, (torch.from_numpy(f) for f in feats), c, png=True, jpeg_quality=75, **kw)


@pytest.mark.parametrize("out_size", [None, 256])
def test_render_frames_from_landmarks_with_lossless_edge_maps(gpu_device, tmp_path, out_size):
    from livespeechportraits_amd.render_loop import render_frames_from_landmarks
    model, topo, cand = _model(tmp_path, "normal_s64_b3")
    rng = np.random.default_rng(4)
    lms = [topo.size / 2 + rng.normal(0, topo.size / 8, (73, 2)) for _ in range(5)]
    shs = [np.stack([np.linspace(0, topo.size, 18), np.full(18, topo.size - 10.0)], 1) for _ in range(5)]
    c = torch.from_numpy(cand[:1]).to(gpu_device)
    kw = dict(pad=(1, 0, 0, 2), load_size=topo.size, batch=2, save_input=True, out_size=out_size)
    plain = render_frames_from_landmarks(model, lms, shs, c, **kw)
    files = render_frames_from_landmarks(model, lms, shs, c, png=True, **kw)
    assert len(files) == 5 and all(isinstance(p, bytes) and isinstance(i, bytes) for p, i in files)
    for (p, i), (pu, iu) in zip(files, plain):
        assert iu.dtype == np.uint8 and set(np.unique(iu)) <= {0, 255} and (iu > 0).any()
        assert np.array_equal(_pillow(p), pu) and np.array_equal(_pillow(i), iu) and Image.open(io.BytesIO(i)).mode == "L"


def test_refusals_raise_before_any_launch(gpu_device):
    from livespeechportraits_amd import _native as N
    from livespeechportraits_amd.png import PngEncoder
    for size in ((0, 4), (4, 8193)):
        with pytest.raises(N.LsppngError):
            PngEncoder(size, 3, gpu_device)
    with pytest.raises(N.LsppngError):
        PngEncoder(16, 2, gpu_device)
    enc = PngEncoder((6, 5), 3, gpu_device, max_batch=2)
    enc._dst.fill_(0x5A)
    good = torch.zeros((2, 6, 5, 3), dtype=torch.uint8, device=gpu_device)
    for x in (good.float(), good.cpu(), torch.zeros((2, 5, 6, 3), dtype=torch.uint8, device=gpu_device), good.transpose(1, 2),
              torch.zeros((2, 6, 5), dtype=torch.uint8, device=gpu_device), torch.zeros((3, 6, 5, 3), dtype=torch.uint8, device=gpu_device), good[:0]):
        with pytest.raises(ValueError):
            enc.encode(x)
    torch.cuda.synchronize()
    assert (enc._dst == 0x5A).all(), "a refused call launched something"
    odd = torch.zeros((2 * 6 * 5 * 3 + 1,), dtype=torch.uint8, device=gpu_device)[1:].view(2, 6, 5, 3)      # any address: the encoder reads bytes
    assert enc.encode(odd) == enc.encode(good) and len(enc.encode(good)) == 2


# ---- live ------------------------------------------------------------------------------------------------------------------------------------
from test_gpu_landmarks import make_stage  # noqa: E402
from test_gpu_live import DEV, models, wave_of  # noqa: E402,F401  (models: the module-scoped fixture)
from test_gpu_live_pool import pool_of  # noqa: E402
from test_gpu_live_render import _avatar, generators  # noqa: E402,F401  (generators: the module-scoped fixture)


def test_live_ticks_hand_out_lossless_files(models, generators):
    """one session, the smallest pool the live-render tests use: every file of tick(png=True) decodes to the frame tick(host=True) gives for the
    same audio in a second pool"""
    from livespeechportraits_amd.live_render import LivePortraitPool
    gens, cand = generators
    meta, cfg = _avatar()
    clip = wave_of(30 * 267, seed=71)

    def run(**kw):
        pool = LivePortraitPool(pool_of(models, max_sessions=1), make_stage(cfg, meta, DEV, max_sessions=1), gens["f32"], cand, max_batch=4)
        sid = pool.open(np.zeros(12, np.float32), torch.Generator().manual_seed(72))
        got, step = [], 1500
        with pytest.raises(ValueError):
            pool.tick({sid: clip[:10]}, png=True, jpeg_quality=75)
        for at in range(0, len(clip), step):
            start, out = pool.tick({sid: clip[at:at + step]}, finish=[sid] if at + step >= len(clip) else (), **kw)[sid]
            assert start == len(got)
            got += list(out)
        return got, pool

    frames, _ = run(host=True)
    files, pool = run(png=True)
    assert len(pool._jpeg) == 1 and len(files) == len(frames) > 4
    for k, (f, want) in enumerate(zip(files, frames)):
        assert isinstance(f, bytes) and np.array_equal(_pillow(f), want), k
