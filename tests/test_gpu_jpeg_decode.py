"""The JPEG decoder on the device (include/lspjpegdec.h, jpeg.JpegDecoder, candidates.load_candidates, video.AviReader.frames): every
comparison is equality with the pixels Pillow returns, frozen under tests/golden (tools/make_golden_jpeg_decode.py), or with the numpy
restatement tests/jpeg_decode_model.py where the file is made during the test.  No tolerance anywhere.  None of this exists on the parent
commit: the whole file fails there."""
import argparse
import hashlib

import numpy as np
import pytest
import torch

import jpeg_decode_cases as K
import jpeg_decode_model as D
from conftest import golden_problem

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def decoder(gpu_device):
    from livespeechportraits_amd.jpeg import JpegDecoder
    return JpegDecoder(gpu_device, max_side=512, max_batch=256)


@pytest.fixture(scope="module")
def small_decoded(decoder):
    """all small fixtures in ONE call (every geometry, sampling, table kind and restart option side by side): name -> uint8 array"""
    _, files, _ = K.fixtures()
    names = K.small_names()
    out = decoder.decode([files[n] for n in names])
    assert decoder.last_status == [0] * len(names)
    return {n: t.cpu().numpy() for n, t in zip(names, out)}


def test_every_small_fixture_decodes_to_pillows_pixels(small_decoded):
    _, _, pixels = K.fixtures()
    assert len(small_decoded) >= 100
    for n, got in small_decoded.items():
        want = pixels[n[:-6] if n.endswith("_nodht") else n]
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), n


def test_the_512_frames_decode_to_pillows_pixels(decoder):
    """four quality-95 candidates and eight quality-75 frames (the encoder fixtures' files) in one call; the pixels are frozen as sha256"""
    meta = K.fixtures()[0]
    files = K.frames_512()
    out = decoder.decode([files[c["name"]] for c in meta["frames"]])
    for c, t in zip(meta["frames"], out):
        got = t.cpu().numpy()
        assert list(got.shape) == c["shape"] and hashlib.sha256(got.tobytes()).hexdigest() == c["pixels_sha256"], c["name"]


def test_one_call_equals_one_file_at_a_time_and_another_order(decoder, small_decoded):
    """per-file state does not leak: each file alone, and the batch reversed, give the bytes the one call gave"""
    _, files, _ = K.fixtures()
    names = K.small_names()
    for n in names:
        alone = decoder.decode([files[n]])[0].cpu().numpy()
        assert np.array_equal(alone, small_decoded[n]), n
    back = decoder.decode([files[n] for n in reversed(names)])
    for n, t in zip(reversed(names), back):
        assert np.array_equal(t.cpu().numpy(), small_decoded[n]), n
    rng = np.random.default_rng(3)
    order = [names[i] for i in rng.permutation(len(names))]
    for n, t in zip(order, decoder.decode([files[n] for n in order])):
        assert np.array_equal(t.cpu().numpy(), small_decoded[n]), n


def test_batches_larger_than_max_batch_are_split(gpu_device, small_decoded):
    from livespeechportraits_amd.jpeg import JpegDecoder
    _, files, _ = K.fixtures()
    names = K.small_names()[:23]
    out = JpegDecoder(gpu_device, max_side=128, max_batch=5).decode([files[n] for n in names])
    for n, t in zip(names, out):
        assert np.array_equal(t.cpu().numpy(), small_decoded[n]), n


@pytest.mark.parametrize("channel0", [0, 3, 6, 9])
def test_decode_into_writes_its_channels_and_nothing_else(decoder, gpu_device, channel0):
    """table[pixels] bit for bit at channels channel0 .. channel0 + 2 of a 12-channel tensor; the other channels keep the sentinel"""
    _, files, pixels = K.fixtures()
    name = K.find("_422_40x72_")
    table_np = np.random.default_rng(8).standard_normal(256).astype(np.float32)
    table = torch.from_numpy(table_np).to(gpu_device)
    out = torch.full((12, 40, 72), -7.25, dtype=torch.float32, device=gpu_device)
    decoder.decode_into([files[name]], out, channel0, table)
    got = out.cpu().numpy()
    want = np.full((12, 40, 72), -7.25, np.float32)
    want[channel0:channel0 + 3] = table_np[pixels[name]].transpose(2, 0, 1)
    assert got.tobytes() == want.tobytes()


def test_decode_into_takes_grey_and_colour_files_in_one_call(decoder, gpu_device):
    _, files, pixels = K.fixtures()
    grey, colour = K.find("_grey_40x72_"), K.find("_420_40x72_")
    table_np = np.arange(256, dtype=np.float32) * np.float32(0.5)
    out = torch.full((6, 40, 72), -1.0, dtype=torch.float32, device=gpu_device)
    decoder.decode_into([files[grey], files[colour]], out, 1, torch.from_numpy(table_np).to(gpu_device))
    got = out.cpu().numpy()
    assert np.all(got[0] == -1.0) and np.all(got[5] == -1.0)
    assert np.array_equal(got[1], table_np[pixels[grey]]) and np.array_equal(got[2:5], table_np[pixels[colour]].transpose(2, 0, 1))
    with pytest.raises(ValueError):
        decoder.decode_into([files[colour], files[colour]], out, 1, torch.from_numpy(table_np).to(gpu_device))      # channels 1..6 of 6


def test_load_candidates_is_the_formula_on_pillows_pixels(gpu_device):
    """the four 512^2 quality-95 files -> [1, 12, 512, 512]: every value is table[pixel] of the normalisation table (pinned on the formula in
    tests/test_jpeg_decode_cpu.py), and the pixels behind them are Pillow's (frozen as sha256)"""
    from livespeechportraits_amd.candidates import load_candidates, normalisation_table
    meta = K.fixtures()[0]
    cases = [c for c in meta["frames"] if c["name"].startswith("candidate_")]
    files = K.frames_512()
    out = load_candidates([files[c["name"]] for c in cases], gpu_device, size=512)
    assert out.shape == (1, 12, 512, 512) and out.dtype == torch.float32 and out.device == gpu_device
    got = out[0].cpu().numpy()
    table = normalisation_table()
    assert np.all(np.diff(table) > 0)
    idx = np.searchsorted(table, got)
    assert idx.max() <= 255 and table[idx].tobytes() == got.tobytes()       # every value is an entry of the table, bit for bit
    for j, c in enumerate(cases):
        px = np.ascontiguousarray(idx[3 * j:3 * j + 3].transpose(1, 2, 0).astype(np.uint8))
        assert hashlib.sha256(px.tobytes()).hexdigest() == c["pixels_sha256"], c["name"]


def test_load_candidates_feeds_the_engine_like_the_host_built_tensor(gpu_device, tmp_path):
    """four 64^2 files -> the `normal` fp32 engine on the weights of the golden case normal_s64_b3: the same output, bit for bit, as for the
    tensor demo.py:88-95 builds on the host from Pillow's pixels; a data root resolves candidates/normalized_full_{j}.jpg"""
    from livespeechportraits_amd.candidates import load_candidates, normalisation_table
    from livespeechportraits_amd.engine import Engine
    _, files, pixels = K.fixtures()
    names = ["candidate_%d_64x64_q95" % j for j in range(4)]
    (tmp_path / "candidates").mkdir()
    for j, n in enumerate(names):
        (tmp_path / "candidates" / ("normalized_full_%d.jpg" % j)).write_bytes(files[n])
    cand = load_candidates(str(tmp_path), gpu_device, size=64)
    table = normalisation_table()
    host = np.concatenate([table[pixels[n]].transpose(2, 0, 1) for n in names])[None]
    assert cand.cpu().numpy().tobytes() == host.tobytes()
    meta, _, topo, sd, feat, _ = golden_problem("normal_s64_b3")
    e = Engine(topo.variant, 13, 1, 3, topo.ngf, topo.num_downs, topo.size, max_batch=meta["batch"])
    e.load_state_dict(sd)
    e.bind(e.pack(), gpu_device)
    f = torch.from_numpy(feat).to(gpu_device)
    a = e.forward(f, cand).clone()
    b = e.forward(f, torch.from_numpy(host).to(gpu_device)).clone()
    torch.cuda.synchronize()
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    with pytest.raises(ValueError):
        load_candidates([files[names[0]]] * 4, gpu_device, size=512)       # 64 x 64 files where 512 x 512 are expected


def test_corrupt_files_in_a_batch_keep_their_status_and_their_sentinel(decoder, gpu_device):
    """three corrupt files (each has been through the sanitizer-built host checker: tests/test_jpeg_decode_cpu.py) among good ones: the status
    words carry the codes -- CORRUPT found by stage 1, RANGE found by stage 2, CORRUPT found by the planner --, the good files are exact, and
    the outputs of the bad ones still hold the sentinel"""
    from livespeechportraits_amd import jpeg as J
    meta, files, pixels = K.fixtures()
    good = [K.find(p) for p in ("_420_40x72_", "_rstb_47x33_", "_grey_16x16_", "_444_9x4_", "_rstr_40x72_")]
    bad = {c["name"]: c["status"] for c in meta["corrupt"]}
    assert bad == {"corrupt_scan_byte": J.CORRUPT, "corrupt_range": J.RANGE, "corrupt_cut": J.CORRUPT}
    order = [good[0], "corrupt_scan_byte", good[1], good[2], "corrupt_range", "corrupt_cut", good[3], good[4]]
    outs = []
    for n in order:
        i = J.probe(files[n])
        shape = (i.height, i.width, 3) if i.components == 3 else (i.height, i.width)
        outs.append(torch.full(shape, SENTINEL, dtype=torch.uint8, device=gpu_device) if i.status == 0 else None)
    assert [o is None for o in outs] == [n == "corrupt_cut" for n in order]          # the planner refuses that one: it has no output at all
    res = decoder.decode([files[n] for n in order], strict=False, outs=outs)
    assert decoder.last_status == [bad.get(n, 0) for n in order]
    for n, o, r in zip(order, outs, res):
        if n in bad:
            assert r is None and (o is None or bool((o == SENTINEL).all())), n
        else:
            assert r is o and np.array_equal(o.cpu().numpy(), pixels[n]), n
    with pytest.raises(J.JpegError) as e:
        decoder.decode([files[n] for n in order])
    assert (e.value.index, e.value.code, e.value.statuses) == (1, J.CORRUPT, decoder.last_status)
    # float form: the refused file's channels keep the sentinel, the good file's are written
    table = torch.arange(256, dtype=torch.float32, device=gpu_device)
    out = torch.full((6, 40, 72), -3.0, dtype=torch.float32, device=gpu_device)
    with pytest.raises(J.JpegError):
        decoder.decode_into([files["corrupt_scan_byte"], files[good[0]]], out, 0, table)
    got = out.cpu().numpy()
    assert np.all(got[:3] == -3.0) and np.array_equal(got[3:], pixels[good[0]].transpose(2, 0, 1).astype(np.float32))


def test_every_refusal_reaches_the_caller_with_its_code(decoder):
    """the refusals of tests/jpeg_decode_cases.py in one batch with a good file first: the status words are the codes"""
    _, files, pixels = K.fixtures()
    cases = K.refusals()
    good = K.find("_opt_16x16_")
    res = decoder.decode([files[good]] + [d for _, d, _ in cases], strict=False)
    assert decoder.last_status == [0] + [s for _, _, s in cases]
    assert np.array_equal(res[0].cpu().numpy(), pixels[good])
    for (what, data, status), r in zip(cases, res[1:]):
        assert (r is None) == (status != 0), what
        if status == 0:
            assert np.array_equal(r.cpu().numpy(), D.decode(data)), what


def _model(tmp_path, case="normal_s64_b3"):
    import livespeechportraits_amd as L
    meta, _, topo, sd, _, cand = golden_problem(case)
    opt = argparse.Namespace(model="feature2face", gpu_ids=[0], isTrain=False, size=meta["variant"], ngf=meta["ngf"],
                             n_downsample_G=meta["num_downs"], fp16=0, checkpoints_dir=str(tmp_path), name="t", load_epoch="none", verbose=False)
    model = L.create_model(opt)
    model._g().load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    model.eval()
    return model, topo, cand


def test_round_trip_through_the_avi(gpu_device, tmp_path, decoder):
    """16 rendered frames -> render_frames(video=AviWriter) -> AviReader.frames(): the decode of the very chunks by the numpy restatement, so
    no farther from the frames before the encode than the restatement's decode is; audio() is the written samples bit for bit"""
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.render_loop import render_frames
    from livespeechportraits_amd.video import AviReader, AviWriter
    model, topo, cand = _model(tmp_path)
    S, n = topo.size, 16
    c = torch.from_numpy(cand[:1]).to(gpu_device)
    feats, _ = synth.make_inputs(n, S, seed=31, cand_batch=1)
    maps = lambda: (torch.from_numpy(f) for f in feats)
    wave = (np.sin(np.arange(n * 16000 // 60 + 25) / 11.0) * 0.25).astype(np.float32)
    before = render_frames(model, maps(), c, batch=8)                       # the uint8 frames the encoder gets
    path = str(tmp_path / "clip.avi")
    with AviWriter(path, S, S) as w:
        assert render_frames(model, maps(), c, batch=8, video=w, audio=wave) == []
    r = AviReader(path)
    assert (r.width, r.height, r.fps, r.nframes, r.audio_rate, r.audio_format) == (S, S, 60, n, 16000, "f32")
    assert r.audio().tobytes() == wave[:n * 16000 // 60].tobytes()
    got = [t.cpu().numpy() for t in r.frames(decoder=decoder, batch=5)]     # ragged batches: 5, 5, 5, 1
    assert len(got) == n
    for i in range(n):
        want = D.decode(r.jpeg(i))
        assert got[i].shape == (S, S, 3) and np.array_equal(got[i], want), i
        pre = np.asarray(before[i]).astype(np.int64)
        assert np.abs(got[i] - pre).max() <= np.abs(want - pre).max(), i
    part = [t.cpu().numpy() for t in r.frames(3, 7, decoder=decoder)]
    assert len(part) == 4 and all(np.array_equal(a, b) for a, b in zip(part, got[3:7]))
