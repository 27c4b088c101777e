"""Progressive JPEG on the device (jpeg.JpegDecoder(progressive=True), candidates.load_candidates(progressive=True); the kernel is
jpegdec_progressive in csrc/jpegdec.hip): every comparison is equality with the pixels Pillow returns, frozen under tests/golden
(tools/make_golden_jpeg_progressive.py), or with what the baseline twins decode to.  No tolerance anywhere.  The argument does not exist on the
parent commit: every test but the last fails there."""
import hashlib

import numpy as np
import pytest
import torch

import jpeg_decode_cases as K
import jpeg_decode_model as D
import jpeg_progressive_cases as KP

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def decoder(gpu_device):
    from livespeechportraits_amd.jpeg import JpegDecoder
    return JpegDecoder(gpu_device, max_side=512, max_batch=512, progressive=True)


def _mixed():
    """[(name, file, pixels)]: every progressive fixture, a baseline fixture after every third one"""
    _, files, _, pixels = KP.fixtures()
    _, base, bpx = K.fixtures()
    bn = [n for n in K.small_names() if not n.endswith("_nodht")]
    out = []
    for k, n in enumerate(KP.small_names()):
        out.append((n, files[n], pixels[n]))
        if k % 3 == 2:
            b = bn[(k // 3) % len(bn)]
            out.append((b, base[b], bpx[b]))
    return out


@pytest.fixture(scope="module")
def mixed_decoded(decoder):
    """ONE call: every geometry, sampling, restart option and table kind, progressive and baseline side by side"""
    cases = _mixed()
    out = decoder.decode([d for _, d, _ in cases])
    assert decoder.last_status == [0] * len(cases)
    return [t.cpu().numpy() for t in out]


def test_every_progressive_fixture_decodes_to_pillows_pixels_beside_baseline_files(mixed_decoded):
    cases = _mixed()
    assert len(cases) == 152 + 50
    for (n, _, want), got in zip(cases, mixed_decoded):
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), n


def test_one_call_equals_one_file_at_a_time_and_another_order(decoder, mixed_decoded):
    cases = _mixed()
    for (n, d, _), want in zip(cases, mixed_decoded):
        assert np.array_equal(decoder.decode([d])[0].cpu().numpy(), want), n
    order = np.random.default_rng(5).permutation(len(cases))
    for i, t in zip(order, decoder.decode([cases[i][1] for i in order])):
        assert np.array_equal(t.cpu().numpy(), mixed_decoded[i]), cases[i][0]


def test_the_workspace_content_on_entry_is_irrelevant(decoder, mixed_decoded):
    """the workspace holds 0xA5 everywhere before the call: the kernel's own zeroing is what the scans add to, the blocks outside a component's
    extent (never visited by an AC scan) included"""
    cases = _mixed()
    assert decoder._ws.numel() > 0
    decoder._ws.fill_(SENTINEL)
    for (n, _, _), t, want in zip(cases, decoder.decode([d for _, d, _ in cases]), mixed_decoded):
        assert np.array_equal(t.cpu().numpy(), want), n


def test_the_512_frames_decode_to_pillows_pixels(decoder):
    """the constant frame (end-of-band runs of 4096 blocks) and the four candidates in one call; the pixels are frozen as sha256"""
    meta = KP.fixtures()[0]
    files, _ = KP.frames_512()
    out = decoder.decode([files[c["name"]] for c in meta["frames"]])
    assert len(out) == 5
    for c, t in zip(meta["frames"], out):
        got = t.cpu().numpy()
        assert list(got.shape) == c["shape"] and hashlib.sha256(got.tobytes()).hexdigest() == c["pixels_sha256"], c["name"]


def test_progressive_candidates_give_the_tensor_of_their_baseline_twins(decoder, gpu_device):
    """decode_into and load_candidates(progressive=True) on the four progressive 512^2 files: bit for bit the tensor the existing path builds
    from the baseline twins"""
    from livespeechportraits_amd.candidates import load_candidates, normalisation_table
    from livespeechportraits_amd.jpeg import JpegError
    files, twins = KP.frames_512()
    names = ["candidate_%d_512_q95_prog" % j for j in range(4)]
    want = load_candidates([twins[n] for n in names], gpu_device, size=512)
    got = load_candidates([files[n] for n in names], gpu_device, size=512, progressive=True)
    assert got.shape == (1, 12, 512, 512) and got.dtype == torch.float32 and torch.equal(got, want)
    table = torch.from_numpy(normalisation_table()).to(gpu_device)
    out = torch.full((12, 512, 512), -7.25, dtype=torch.float32, device=gpu_device)
    decoder.decode_into([files[names[0]], twins[names[1]], files[names[2]]], out, 3, table)      # progressive and baseline files in one call
    assert bool((out[:3] == -7.25).all()) and torch.equal(out[3:6], want[0, 0:3]) and torch.equal(out[6:9], want[0, 3:6]) and torch.equal(out[9:], want[0, 6:9])
    with pytest.raises(JpegError):
        load_candidates([files[n] for n in names], gpu_device, size=512)   # the default is as before


def test_refused_and_corrupt_files_in_a_batch_keep_status_and_sentinel(decoder, gpu_device):
    """the new refusals among good files of both kinds: the planner's codes and stage 1's (the scan cut short is found on the device) reach
    the caller, the outputs of the refused files keep the sentinel, the neighbours and the table-id-3 control are exact"""
    from livespeechportraits_amd import jpeg as J
    _, files, _, pixels = KP.fixtures()
    _, base, bpx = K.fixtures()
    cases = KP.refusals()
    assert J.probe(dict((w, d) for w, d, _ in cases)["a scan cut short"], progressive=True).status == 0       # the planner passes it
    good = [(files[n], pixels[n]) for n in (KP.find("_420_rstb3_31x18_"), KP.find("_grey_plain_64x64_"))] + [(base[n], bpx[n]) for n in (K.find("_rstr_40x72_"),)]
    batch, want = [], []
    for k, (what, data, status) in enumerate(cases):
        batch.append(good[k % 3][0])
        want.append((0, good[k % 3][1]))
        batch.append(data)
        want.append((status, pixels[KP.find("_420_plain_40x72_")] if status == 0 else None))
    outs = []
    for d in batch:
        i = J.probe(d, progressive=True)
        outs.append(torch.full((i.height, i.width, 3) if i.components == 3 else (i.height, i.width), SENTINEL, dtype=torch.uint8, device=gpu_device) if i.status == 0 else None)
    res = decoder.decode(batch, strict=False, outs=outs)
    assert decoder.last_status == [s for s, _ in want]
    for (status, px), o, r in zip(want, outs, res):
        if status:
            assert r is None and (o is None or bool((o == SENTINEL).all()))
        else:
            assert r is o and np.array_equal(o.cpu().numpy(), px)
    with pytest.raises(J.JpegError) as e:
        decoder.decode(batch)
    assert (e.value.index, e.value.code) == (1, cases[0][2])


def test_a_decoder_made_without_the_flag_still_refuses(gpu_device):
    from livespeechportraits_amd import jpeg as J
    _, files, _, _ = KP.fixtures()
    _, base, bpx = K.fixtures()
    b = K.find("_420_40x72_")
    dec = J.JpegDecoder(gpu_device, max_side=128)
    res = dec.decode([files[KP.find("_420_plain_40x72_")], base[b], files[KP.find("_grey_plain_1x1_")]], strict=False)
    assert dec.last_status == [J.UNSUPPORTED, 0, J.UNSUPPORTED] and res[0] is None and res[2] is None
    assert np.array_equal(res[1].cpu().numpy(), bpx[b])
