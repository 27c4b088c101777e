"""The device JPEG encoder (include/lspjpeg.h, livespeechportraits_amd/jpeg.py) against Pillow's bytes: the frozen fixtures of
tests/golden/jpeg_pil.{json,npz} (tools/make_golden_jpeg.py), and the host model tests/jpeg_model.py (itself pinned to Pillow by
tests/test_jpeg_cpu.py) on what the renderer and the rasteriser really write.  Every comparison is byte for byte."""
import argparse
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import jpeg_model as M
from conftest import GOLDEN, golden_problem

pytestmark = pytest.mark.gpu


def _fixtures():
    meta = json.load(open(os.path.join(GOLDEN, "jpeg_pil.json")))
    return meta["cases"], dict(np.load(os.path.join(GOLDEN, "jpeg_pil.npz")))


def _same(data, case, arrays):
    if case["name"] in arrays:
        return data == arrays[case["name"]].tobytes()
    return len(data) == case["length"] and hashlib.sha256(data).hexdigest() == case["sha256"]


def _geometry(case):
    r = case["recipe"]
    return r["h"], r["w"], r["channels"], case["quality"]


def test_every_fixture_encodes_to_pillows_bytes(gpu_device):
    from livespeechportraits_amd.jpeg import JpegEncoder
    cases, arrays = _fixtures()
    groups = {}
    for c in cases:
        groups.setdefault(_geometry(c), []).append(c)
    bad = []
    for (h, w, ch, q), group in groups.items():
        enc = JpegEncoder((h, w), ch, q, gpu_device, max_batch=8)
        for k in range(0, len(group), 8):                                  # batches of different frames, in fixture order
            part = group[k:k + 8]
            x = torch.from_numpy(np.stack([M.make_image(c["recipe"]) for c in part])).to(gpu_device)
            got = enc.encode(x)
            bad += [c["name"] for c, g in zip(part, got) if not _same(g, c, arrays)]
    assert not bad, bad


@pytest.mark.parametrize("batch", [1, 3, 8])
@pytest.mark.parametrize("channels", [3, 1])
def test_batches_of_different_frames(gpu_device, batch, channels):
    """every slot of a batch is its own frame (its own DC predictor chain, bit offsets and byte counts)"""
    from livespeechportraits_amd.jpeg import JpegEncoder
    cases, arrays = _fixtures()
    kind = "smooth" if channels == 3 else "edges"
    slots = [c for c in cases if c["name"].startswith("%s_%s_512_s" % (kind, "c" if channels == 3 else "g"))]
    assert len(slots) == 8
    enc = JpegEncoder(512, channels, 75, gpu_device, max_batch=8)
    for rot in (0, 5):
        part = [slots[(rot + k) % 8] for k in range(batch)]
        got = enc.encode(torch.from_numpy(np.stack([M.make_image(c["recipe"]) for c in part])).to(gpu_device))
        assert len(got) == batch and all(_same(g, c, arrays) for g, c in zip(got, part)), (batch, channels, rot)


@pytest.mark.parametrize("variant,dtype", [("normal", "bf16"), ("large", "f32")])
def test_renderer_frames_encode_like_the_model(gpu_device, variant, dtype):
    """Engine.forward_image (the fused tensor2im) on the golden inputs, then the device encoder == the host model on a copy of the same
    uint8 frames, at 75 and two other qualities"""
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.engine import Engine
    from livespeechportraits_amd.jpeg import JpegEncoder
    meta, _, topo, sd, feat, cand = golden_problem("%s_512" % variant)
    e = Engine(variant, 13, 1, 3, topo.ngf, topo.num_downs, topo.size, max_batch=2, dtype=dtype)
    e.load_state_dict(sd)
    e.bind(e.pack(), gpu_device)
    f2, _ = synth.make_inputs(2, topo.size, seed=17, cand_batch=1)
    f2[0] = feat[0]
    u8 = e.forward_image(torch.from_numpy(f2).to(gpu_device), torch.from_numpy(cand).to(gpu_device))
    host = u8.cpu().numpy()
    for q in (75, 30, 95):
        got = JpegEncoder(topo.size, 3, q, gpu_device, max_batch=2).encode(u8)
        for k in range(2):
            assert got[k] == M.encode(host[k], q), (variant, dtype, q, k)
    e.close()


def test_rasteriser_edge_maps_encode_like_the_model(gpu_device):
    from livespeechportraits_amd.feature_map import FeatureMapRasteriser
    from livespeechportraits_amd.jpeg import JpegEncoder
    rng = np.random.default_rng(11)
    lm = 256 + rng.normal(0, 60, (3, 73, 2))
    sh = np.stack([np.linspace(0, 512, 18), np.full(18, 470.0)], 1)[None].repeat(3, 0) + rng.normal(0, 3, (3, 18, 2))
    r = FeatureMapRasteriser(512, 18, gpu_device)
    maps = r.rasterise(lm, sh, as_uint8=True)
    host = maps.cpu().numpy()
    assert (host > 0).any()
    for q in (75, 100):
        got = JpegEncoder(512, 1, q, gpu_device, max_batch=4).encode(maps)
        assert all(got[k] == M.encode(host[k], q) for k in range(3)), q
    # the float map and the uint8 map of ONE launch (render_frames_from_landmarks(save_input=True)) are the same picture
    f32 = torch.empty((3, 1, 512, 512), dtype=torch.float32, device=gpu_device)
    u8 = torch.empty((3, 512, 512), dtype=torch.uint8, device=gpu_device)
    r.rasterise(lm, sh, out=f32, out_u8=u8)
    assert np.array_equal(u8.cpu().numpy(), host) and np.array_equal((f32[:, 0].cpu().numpy() * 255).astype(np.uint8), host)


def _model(tmp_path, case="large_s128_b2"):
    import livespeechportraits_amd as L
    meta, _, topo, sd, _, cand = golden_problem(case)
    opt = argparse.Namespace(model="feature2face", gpu_ids=[0], isTrain=False, size=meta["variant"], ngf=meta["ngf"],
                             n_downsample_G=meta["num_downs"], fp16=0, checkpoints_dir=str(tmp_path), name="t", load_epoch="none", verbose=False)
    model = L.create_model(opt)
    model._g().load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    model.eval()
    return model, topo, cand


def test_render_frames_hands_out_pillows_files(gpu_device, tmp_path):
    """render_frames(jpeg_quality=75) over 17 maps (batches 8, 8, 1 on two lanes) == the model's encoding of the frames render_frames
    returns without the argument; on_frame sees bytes in order; save_images writes demo.py's names"""
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.jpeg import save_images
    from livespeechportraits_amd.render_loop import render_frames
    model, topo, cand = _model(tmp_path)
    feats, _ = synth.make_inputs(17, topo.size, seed=23, cand_batch=1)
    c = torch.from_numpy(cand).to(gpu_device)
    plain = render_frames(model, (torch.from_numpy(f) for f in feats), c, batch=8)
    files = render_frames(model, (torch.from_numpy(f) for f in feats), c, batch=8, jpeg_quality=75)
    assert len(files) == 17 and all(isinstance(f, bytes) for f in files)
    for k in range(17):
        assert files[k] == M.encode(plain[k], 75), k
    seen = []
    render_frames(model, (torch.from_numpy(f).to(gpu_device) for f in feats), c, batch=8, jpeg_quality=75, on_frame=lambda i, b: seen.append((i, b)))
    assert [i for i, _ in seen] == list(range(17)) and [b for _, b in seen] == files
    paths = save_images(str(tmp_path / "out"), files[:3], index0=4)
    assert [os.path.basename(p) for p in paths] == ["pred_5.jpg", "pred_6.jpg", "pred_7.jpg"] and open(paths[1], "rb").read() == files[1]


def test_render_frames_from_landmarks_with_input_maps(gpu_device, tmp_path):
    """jpeg_quality + save_input: (pred, input) pairs == the model's encodings of the uint8 frames and edge maps of the uncompressed route"""
    from livespeechportraits_amd.render_loop import render_frames_from_landmarks
    model, topo, cand = _model(tmp_path)
    rng = np.random.default_rng(4)
    lms = [topo.size / 2 + rng.normal(0, topo.size / 8, (73, 2)) for _ in range(5)]
    shs = [np.stack([np.linspace(0, topo.size, 18), np.full(18, topo.size - 10.0)], 1) for _ in range(5)]
    c = torch.from_numpy(cand).to(gpu_device)
    kw = dict(pad=(1, 0, 0, 2), load_size=topo.size, batch=2, save_input=True)
    plain = render_frames_from_landmarks(model, lms, shs, c, **kw)
    files = render_frames_from_landmarks(model, lms, shs, c, jpeg_quality=75, **kw)
    assert len(files) == 5 and all(isinstance(p, bytes) and isinstance(i, bytes) for p, i in files)
    for (p, i), (pu, iu) in zip(files, plain):
        assert iu.dtype == np.uint8 and set(np.unique(iu)) <= {0, 255}
        assert p == M.encode(pu, 75) and i == M.encode(iu, 75)
    assert [p for p, _ in files] == render_frames_from_landmarks(model, lms, shs, c, pad=(1, 0, 0, 2), load_size=topo.size, batch=2, jpeg_quality=75)


def test_poisoned_buffers_and_repeats_give_identical_bytes(gpu_device):
    """workspace and output filled with 0xFF / 0x00 / 0xA5 between calls, and repeated calls: the same bytes every time (the encoder
    must not read anything it did not write in the same call)"""
    from livespeechportraits_amd.jpeg import JpegEncoder
    cases, arrays = _fixtures()
    for kind, ch in (("smooth", 3), ("edges", 1)):
        part = [c for c in cases if c["name"].startswith("%s_%s_512_s" % (kind, "c" if ch == 3 else "g"))][:4]
        x = torch.from_numpy(np.stack([M.make_image(c["recipe"]) for c in part])).to(gpu_device)
        enc = JpegEncoder(512, ch, 75, gpu_device, max_batch=8)
        first = enc.encode(x)
        assert all(_same(g, c, arrays) for g, c in zip(first, part))
        for byte in (0xFF, 0x00, 0xA5, 0xFF):
            enc._ws.fill_(byte)
            enc._dst.fill_(byte)
            enc._sizes.fill_(-1)
            assert enc.encode(x) == first, (kind, byte)
        for _ in range(5):
            assert enc.encode(x) == first


def test_worst_case_noise_stays_inside_the_documented_bound(gpu_device):
    """q100 uniform noise (the largest files: every AC coefficient coded, dense 0xFF stuffing): within lspjpeg_capacity_bytes, equal to the
    model, and the bound is the header's formula"""
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.jpeg import JpegEncoder
    for ch in (3, 1):
        enc = JpegEncoder(512, ch, 100, gpu_device, max_batch=8)
        blocks = 512 * 512 // 64 * (3 if ch == 3 else 2) // 2
        assert enc.capacity == 2 * ((blocks * 1660 + 7) // 8) + 2
        shape = (8, 512, 512, 3) if ch == 3 else (8, 512, 512)
        x = (synth.uniform01(int(np.prod(shape)), 77 + ch) * 256).astype(np.uint8).reshape(shape)
        got = enc.encode(torch.from_numpy(x).to(gpu_device))
        assert all(len(g) - len(enc.header) <= enc.capacity for g in got)
        assert got[0] == M.encode(x[0], 100) and got[7] == M.encode(x[7], 100)


def test_refusals_raise_before_any_launch(gpu_device):
    from livespeechportraits_amd import _native as N
    from livespeechportraits_amd.jpeg import JpegEncoder
    for q in (0, 101):
        with pytest.raises(N.LspjpegError):
            JpegEncoder(512, 3, q, gpu_device)
    for size, ch in ((520, 3), (24, 3), (36, 1)):
        with pytest.raises(N.LspjpegError):
            JpegEncoder(size, ch, 75, gpu_device)
    with pytest.raises(RuntimeError):
        JpegEncoder(512, 3, 75, "cpu")
    enc = JpegEncoder(64, 3, 75, gpu_device, max_batch=2)
    enc._dst.fill_(0x5A)
    good = torch.zeros((2, 64, 64, 3), dtype=torch.uint8, device=gpu_device)
    bad = [good.float(), good.cpu(), torch.zeros((2, 64, 48, 3), dtype=torch.uint8, device=gpu_device), good.transpose(1, 2),
           torch.zeros((2, 64, 64), dtype=torch.uint8, device=gpu_device), torch.zeros((3, 64, 64, 3), dtype=torch.uint8, device=gpu_device),
           torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device=gpu_device)[:0],
           torch.zeros((3 * 64 * 64 * 3 + 1,), dtype=torch.uint8, device=gpu_device)[1:].view(3, 64, 64, 3)[:2]]
    for x in bad:
        with pytest.raises(ValueError):
            enc.encode(x)
    torch.cuda.synchronize()
    assert (enc._dst == 0x5A).all(), "a refused call launched something"
    assert len(enc.encode(good)) == 2
    # a model on the host has no encoder to feed
    from livespeechportraits_amd.render_loop import render_frames

    class Host:
        def inference_image(self, maps, cand):
            return torch.zeros((maps.shape[0], 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        render_frames(Host(), iter([torch.zeros(1, 16, 16)]), torch.zeros(1, 12, 16, 16), batch=2, jpeg_quality=75)
