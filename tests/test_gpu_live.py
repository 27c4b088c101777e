"""GPU tests of the live audio path: the carried-state entry points of the recurrent stacks (lsprnn_forward_state), the resumable
head-pose generation (lspa2h_generate_resume), the mel window range (lspmel_compute_range) and the LiveAudioFrontEnd session on top
of them.  The acceptance test is "pushed in pieces == pushed at once, bit for bit" against the whole-clip path."""
import argparse
import os

import numpy as np
import pytest
import torch

from test_a2h_cpu import load_case

pytestmark = pytest.mark.gpu
RNN_TOL = 5e-5      # tests/test_rnn.py TOL: fp32 recurrences, 3 layers
A2H_TOL = 2e-4      # tests/test_gpu_a2h.py TOL
DEV = "cuda:0"


# ---- recurrent stacks with carried state ------------------------------------------------------------------
RNN_CASES = {"apc_gru": ("GRU", 3, 80, 512), "a2f_lstm": ("LSTM", 3, 512, 256)}


def _rnn(case, route):
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.rnn_engine import RecurrentEngine
    cell, L, I, H = RNN_CASES[case]
    sd = synth.make_rnn_state_dict(cell, L, I, H, seed=5)
    e = RecurrentEngine(cell, L, I, H, max_steps=512, per_layer=route == "layers")
    e.load_state_dict(sd)
    e.bind(torch.device(DEV))
    return e, sd


def _checked(e, fn):
    out = fn()
    assert e.status() == 0, "an inter-workgroup hand-off timed out"
    return out


@pytest.mark.parametrize("route", ["wave", "layers"])
@pytest.mark.parametrize("case", sorted(RNN_CASES))
def test_rnn_split_equals_one_call(case, route):
    e, _ = _rnn(case, route)
    T = 300
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((T, e.input_size)).astype(np.float32) * 0.5).to(DEV)
    whole = _checked(e, lambda: e.forward(x)).cpu()
    # NULL state == lsprnn_forward, bit for bit; the final state equals the last output row of the top layer
    fin = torch.empty(e.state_floats(), device=DEV)
    nul = _checked(e, lambda: e.forward_state(x, None, fin)).cpu()
    assert torch.equal(nul, whole)
    H, L = e.hidden_size, e.num_layers
    assert torch.equal(fin.cpu()[(L - 1) * H: L * H], whole[-1])
    for k in (1, T // 2, T - 1):
        s0 = torch.empty(e.state_floats(), device=DEV)
        s1 = torch.empty(e.state_floats(), device=DEV)
        a = _checked(e, lambda: e.forward_state(x[:k].contiguous(), None, s0)).cpu()
        b = _checked(e, lambda: e.forward_state(x[k:].contiguous(), s0, s1)).cpu()
        assert torch.equal(torch.cat([a, b]), whole), "split at %d" % k
        assert torch.equal(s1, fin), "final state, split at %d" % k
    with pytest.raises(Exception, match="separate"):
        e.forward_state(x, fin, fin)


@pytest.mark.parametrize("route", ["wave", "layers"])
@pytest.mark.parametrize("case", sorted(RNN_CASES))
def test_rnn_nonzero_initial_state_matches_torch(case, route):
    """Split-equality cannot see a layout that is wrong the same way on save and restore: compare with torch given (h0, c0)."""
    e, sd = _rnn(case, route)
    cell, L, I, H = RNN_CASES[case]
    T = 40
    rng = np.random.default_rng(8)
    x = rng.standard_normal((T, I)).astype(np.float32) * 0.5
    h0 = (rng.standard_normal((L, H)) * 0.5).astype(np.float32)
    c0 = (rng.standard_normal((L, H)) * 0.5).astype(np.float32)
    ref_mod = (torch.nn.GRU if cell == "GRU" else torch.nn.LSTM)(I, H, num_layers=L, batch_first=True)
    ref_mod.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    with torch.no_grad():
        xt = torch.from_numpy(x).unsqueeze(0)
        if cell == "GRU":
            ref, hn = ref_mod(xt, torch.from_numpy(h0).unsqueeze(1))
            ref_state = hn[:, 0].reshape(-1)
            st = torch.from_numpy(h0.reshape(-1))
        else:
            ref, (hn, cn) = ref_mod(xt, (torch.from_numpy(h0).unsqueeze(1), torch.from_numpy(c0).unsqueeze(1)))
            ref_state = torch.cat([hn[:, 0].reshape(-1), cn[:, 0].reshape(-1)])
            st = torch.from_numpy(np.concatenate([h0.reshape(-1), c0.reshape(-1)]))
    sin, sout = st.to(DEV), torch.empty(e.state_floats(), device=DEV)
    got = _checked(e, lambda: e.forward_state(torch.from_numpy(x).to(DEV), sin, sout)).cpu()
    err, serr = float((got - ref[0]).abs().max()), float((sout.cpu() - ref_state).abs().max())
    print("\n[rnn state %s %s] max-abs vs torch: outputs %.3e, final state %.3e" % (case, route, err, serr))
    assert err <= RNN_TOL and serr <= RNN_TOL
    # the zero-state output differs: the state is really used
    assert float((_checked(e, lambda: e.forward(torch.from_numpy(x).to(DEV))).cpu() - got).abs().max()) > 1e-3


# ---- resumable head-pose generation -----------------------------------------------------------------------
def _a2h_engine(cfg, sd, rows):
    from livespeechportraits_amd.a2h_engine import HeadposeEngine
    e = HeadposeEngine(**{k: cfg[k] for k in ("residual_layers", "residual_blocks", "residual_channels", "dilation_channels",
                                              "skip_channels", "kernel_size", "input_channels", "cond_channels", "hidden_size",
                                              "ncenter", "ndim", "loss")}, max_audio_frames=rows)
    e.load_state_dict(sd)
    e.bind(torch.device(DEV))
    return e


def _resume_chain(e, cfg, audio, pre, noise, expq, sigma, ff, cuts):
    """Frames cut into calls at `cuts`; each call passes the audio rows its frames need that earlier calls did not pass."""
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
    gmm = cfg["loss"] == "GMM"
    nframe = audio.shape[0] - ff
    bounds = [0] + list(cuts) + [nframe]
    states = [torch.empty(e.state_bytes(), dtype=torch.uint8, device=DEV) for _ in range(2)]
    outs, rows_passed, st = [], 0, None
    for i, (f0, f1) in enumerate(zip(bounds[:-1], bounds[1:])):
        r1 = f1 - 1 + ff + 1
        so = states[i & 1]
        out = e.generate_resume(d(audio[rows_passed:r1]) if r1 > rows_passed else None, rows_passed, d(pre), d(noise[f0:f1]) if gmm else None,
                                d(expq[f0:f1]) if gmm and cfg["ncenter"] > 1 else None, sigma, ff, f0, f1 - f0, st, so)
        assert e.status() == 0
        outs.append(out.cpu().numpy())
        rows_passed, st = max(rows_passed, r1), so
    return np.concatenate(outs)


@pytest.mark.parametrize("name", ["default_n300", "nc2_l4b1", "l2_l5b2"])
def test_a2h_resume_split_equals_one_call(name):
    from test_gpu_a2h import make_engine, run
    meta, cfg, sd, audio, pre, ref, noise, expq = load_case(name)
    sigma, ff = meta["sigma_scale"], meta["frame_future"]
    whole = run(make_engine(cfg, sd, torch.device(DEV)), cfg, audio, pre, noise, expq, sigma, ff, torch.device(DEV))
    n = whole.shape[0]
    e = _a2h_engine(cfg, sd, audio.shape[0])
    for k in sorted(k for k in {1, 7, 150, n - 1} if 0 < k < n):      # (a clip of 40 frames cannot be split at 150)
        got = _resume_chain(e, cfg, audio, pre, noise, expq, sigma, ff, [k])
        assert np.array_equal(got, whole), "split at %d" % k
        assert np.abs(got - ref).max() <= A2H_TOL
    # one frame per call through a projection ring of frame_future + 2 rows: rows wrap around the ring many times
    small = _a2h_engine(cfg, sd, ff + 2)
    got = _resume_chain(small, cfg, audio, pre, noise, expq, sigma, ff, list(range(1, n)))
    print("\n[a2h resume %s] one frame per call, ring %d rows: max-abs vs reference %.3e" % (name, ff + 2, np.abs(got - ref).max()))
    assert np.array_equal(got, whole)


def test_a2h_resume_refusals():
    from livespeechportraits_amd import _native as N
    meta, cfg, sd, audio, pre, ref, noise, expq = load_case("nc2_l4b1")
    ff = meta["frame_future"]
    e = _a2h_engine(cfg, sd, ff + 4)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
    s0, s1 = (torch.empty(e.state_bytes(), dtype=torch.uint8, device=DEV) for _ in range(2))
    nz, eq = d(noise[:1]), d(expq[:1])
    with pytest.raises(N.Lspa2hError, match="not passed"):        # frame 0 needs row ff
        e.generate_resume(d(audio[:ff]), 0, d(pre), nz, eq, 0.3, ff, 0, 1, None, s0)
    with pytest.raises(N.Lspa2hError, match="frame0 must be 0"):
        e.generate_resume(d(audio[:ff + 2]), 0, d(pre), nz, eq, 0.3, ff, 1, 1, None, s0)
    e.generate_resume(d(audio[:ff + 1]), 0, d(pre), nz, eq, 0.3, ff, 0, 1, None, s0)
    assert e.status() == 0
    with pytest.raises(N.Lspa2hError, match="separate"):
        e.generate_resume(d(audio[ff + 1:ff + 2]), ff + 1, None, nz, eq, 0.3, ff, 1, 1, s0, s0)
    with pytest.raises(N.Lspa2hError, match="left the projection ring"):   # frame 1 reads row ff + 1: overwritten by rows ff+5 ..
        e.generate_resume(d(audio[ff + 5:2 * ff + 9]), ff + 5, None, d(noise[1:2]), d(expq[1:2]), 0.3, ff, 1, 1, s0, s1)
    # a state that belongs to another frame is refused on the device, through the status word; the refused call writes nothing
    out = torch.full((1, cfg["ndim"]), -7777.25, device=DEV)
    s1.fill_(0xA5)
    e.generate_resume(d(audio[ff + 1:ff + 3]), ff + 1, None, d(noise[:1]), d(expq[:1]), 0.3, ff, 2, 1, s0, s1, out=out)
    assert e.status() == 0x5000000
    assert torch.equal(out.cpu(), torch.full((1, cfg["ndim"]), -7777.25)), "a refused call wrote its output"
    assert bool((s1 == 0xA5).all()), "a refused call wrote state_out"


def test_a2h_short_field_no_future_frames():
    """frame_future 0 with a receptive field of 8 and a ring of 3 rows: audio-row clamping (rows below 0 read row 0), the first frame of a
    call and the ring wrap all act within the first few steps.  One call (both kernels) == one frame per call, bit for bit."""
    from livespeechportraits_amd import synth
    from oracle import a2h_oracle
    from test_gpu_a2h import make_engine, run
    dev = torch.device(DEV)
    cfg = dict(synth.A2H_DEFAULTS, residual_layers=3, residual_blocks=1)
    sd = synth.make_a2h_state_dict(cfg, seed=11)
    n, ff, sigma = 12, 0, 0.4
    audio, pre = synth.make_a2h_inputs(n, cfg, seed=12)
    noise = torch.randn(n, cfg["ndim"], generator=torch.Generator().manual_seed(12)).numpy()
    expq = np.ones((n, 1), np.float32)
    want = a2h_oracle.stream(sd, cfg, audio, pre, noise, expq, sigma, ff)
    single = make_engine(cfg, sd, dev, max_audio_frames=n, single_workgroup=True)
    assert single.receptive_field == 8
    whole = run(single, cfg, audio, pre, noise, expq, sigma, ff, dev)
    piped = run(make_engine(cfg, sd, dev, max_audio_frames=n), cfg, audio, pre, noise, expq, sigma, ff, dev)
    chain = _resume_chain(_a2h_engine(cfg, sd, 3), cfg, audio, pre, noise, expq, sigma, ff, list(range(1, n)))
    print("\n[a2h field 8, frame_future 0] max-abs vs streaming oracle %.3e" % np.abs(whole - want).max())
    assert np.array_equal(piped, whole) and np.array_equal(chain, whole)
    assert whole.shape == want.shape and np.abs(whole - want).max() <= A2H_TOL


# ---- mel over a window range ------------------------------------------------------------------------------
@pytest.mark.parametrize("nsamples", [16000 * 3 + 77, 267, 4000])
def test_mel_range_equals_whole_clip(nsamples):
    from livespeechportraits_amd import _native as N, mel
    lib = N.load()
    wave = (0.2 * np.random.default_rng(nsamples).standard_normal(nsamples)).astype(np.float32)
    w = torch.from_numpy(wave).to(DEV)
    whole = mel.compute_mel(w).cpu()
    nwin = whole.shape[0]
    rng = np.random.default_rng(1)
    i = 0
    while i < nwin:
        k = int(rng.integers(1, 40))
        k = min(k, nwin - i)
        first = int(lib.lspmel_window_start(i)) - int(rng.integers(0, 3))     # the buffer may start a little early
        first = max(first, 0)
        last_end = int(lib.lspmel_window_start(i + k - 1)) + 266
        ended = last_end > nsamples
        stop = nsamples if ended else min(nsamples, last_end + int(rng.integers(0, 50)))
        got = mel.compute_mel_range(w[first:stop].contiguous(), first, i, k, ended).cpu()
        assert torch.equal(got, whole[i:i + k]), "windows %d..%d" % (i, i + k)
        i += k
    # the zero-padded last windows, computed alone at the end of the clip
    for j in (nwin - 1, max(nwin - 3, 0)):
        first = int(lib.lspmel_window_start(j))
        assert torch.equal(mel.compute_mel_range(w[first:].contiguous(), first, j, nwin - j, True).cpu(), whole[j:])
    # before the end, a window that reaches past the samples passed is refused
    last = nwin - 1
    first = int(lib.lspmel_window_start(last))
    if first + 266 > nsamples:
        with pytest.raises(N.LspmelError, match="not ended"):
            mel.compute_mel_range(w[first:].contiguous(), first, last, 1, False)
    with pytest.raises(N.LspmelError, match="before first_sample"):
        mel.compute_mel_range(w[first:].contiguous(), first + 1, last, 1, True)


# ---- the session ------------------------------------------------------------------------------------------
CLIP_FRAMES = 687
CLIP_SAMPLES = 183200           # int(687 / 60 * 16000)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.apc import APC_encoder
    from livespeechportraits_amd.models import create_model
    tmp = str(tmp_path_factory.mktemp("live"))
    dev = torch.device(DEV)
    apc = APC_encoder(80, 512, 3, False)
    apc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_apc_state_dict().items()})
    apc = apc.to(dev).eval()
    ck = os.path.join(tmp, "Audio2Feature.pkl")
    torch.save({"module." + k: torch.from_numpy(v) for k, v in synth.make_a2f_state_dict().items()}, ck)
    fopt = argparse.Namespace(model="audio2feature", gpu_ids=[0], isTrain=False, checkpoints_dir=tmp, name="a2f", load_epoch=ck, verbose=False,
                              feature_decoder="LSTM", loss="L2", A2L_GMM_ndim=75, A2L_GMM_ncenter=1, predict_length=1, APC_hidden_size=512,
                              frame_future=18)
    a2f = create_model(fopt)
    a2f.setup(fopt)
    a2f.eval()
    ch = os.path.join(tmp, "Audio2Headpose.pkl")
    torch.save({"module." + k: torch.from_numpy(v) for k, v in synth.make_a2h_state_dict(dict(synth.A2H_DEFAULTS)).items()}, ch)
    hopt = argparse.Namespace(
        model="audio2headpose", gpu_ids=[0], isTrain=False, checkpoints_dir=tmp, name="x", load_epoch=ch, verbose=False,
        feature_decoder="WaveNet", loss="GMM", A2H_GMM_ndim=12, A2H_GMM_ncenter=1, APC_hidden_size=512,
        A2H_wavenet_residual_layers=7, A2H_wavenet_residual_blocks=2, A2H_wavenet_residual_channels=128,
        A2H_wavenet_dilation_channels=128, A2H_wavenet_skip_channels=256, A2H_wavenet_kernel_size=2, time_frame_length=1,
        A2H_wavenet_use_bias=True, A2H_wavenet_input_channels=12, A2H_wavenet_cond_channels=512, frame_future=15)
    a2h = create_model(hopt)
    a2h.setup(hopt)
    a2h.eval()
    hopt.A2H_receptive_field = a2h.Audio2Headpose.module.WaveNet.receptive_field        # demo.py:164
    db = synth.make_feature_database(4000, 8, 512, 24)[0]
    return dict(apc=apc, a2f=a2f, a2h=a2h, fopt=fopt, hopt=hopt, db=db, tmp=tmp)


def wave_of(nsamples, seed=1):
    return (0.1 * np.random.default_rng(seed).standard_normal(nsamples)).astype(np.float32)


def session(m, **kw):
    from livespeechportraits_amd.live import LiveAudioFrontEnd
    return LiveAudioFrontEnd(m["apc"], m["a2f"], m["a2h"], m["db"], True, 10, 1.0, np.zeros(12, np.float32), 0.3, device=DEV,
                             feature_opt=m["fopt"], headpose_opt=m["hopt"], **kw)


def whole_clip(m, wave, seed):
    """The parent commit's path through the existing public functions (demo.py:183-216 with the drop-ins)."""
    from livespeechportraits_amd import manifold, mel
    dev = torch.device(DEV)
    mels = mel.compute_mel(torch.from_numpy(wave).to(dev)).unsqueeze(0)
    feats = m["apc"].forward(mels, torch.Tensor([mels.shape[1]]))[0]
    assert m["apc"]._engine.status() == 0
    feats = manifold.project(feats.contiguous(), torch.from_numpy(m["db"]).to(dev), 10, 1.0).cpu().numpy()
    mouth = m["a2f"].generate_sequences(feats, 16000, 60, fill_zero=True, opt=m["fopt"])
    torch.manual_seed(seed)
    poses = m["a2h"].generate_sequences(feats, np.zeros(12, np.float32), fill_zero=True, sigma_scale=0.3, opt=m["hopt"])
    return mouth, poses


def frame_pieces(nsamples, start=0):
    """pushes of exactly one frame of audio (266 or 267 samples)"""
    out, k, pos = [], 0, start
    while pos < nsamples:
        nxt = min(int((k + 1) * 16000 / 60), nsamples)
        if nxt > pos:
            out.append(nxt - pos)
            pos = nxt
        k += 1
    return out


def stream(m, wave, pieces, seed, counts=True, **kw):
    from livespeechportraits_amd.live import LiveScheduler
    s = session(m, **kw)
    pred = LiveScheduler(s.ff_mouth, s.ff_head, s.sched.max_chunk)
    torch.manual_seed(seed)
    mouth, poses, pos = [], [], 0
    for k in pieces:
        out = s.push(wave[pos:pos + k], host=True)
        pred.plan_push(k)
        pos += k
        assert out.mouth_start == sum(len(x) for x in mouth) and out.pose_start == sum(len(x) for x in poses)
        mouth.append(out.mouth)
        poses.append(out.poses)
        if counts:
            assert (out.mouth_start + len(out.mouth), out.pose_start + len(out.poses)) == (pred.m, pred.h)
    out = s.finish(host=True)
    mouth.append(out.mouth)
    poses.append(out.poses)
    with pytest.raises(RuntimeError, match="ended"):
        s.push(wave[:10])
    return np.concatenate(mouth), np.concatenate(poses)


def test_session_equals_whole_clip_for_every_chunking(models):
    wave = wave_of(CLIP_SAMPLES)
    ref_mouth, ref_poses = whole_clip(models, wave, seed=7)
    assert ref_mouth.shape == (CLIP_FRAMES, 75) and ref_poses.shape == (CLIP_FRAMES - 15, 12)
    rng = np.random.default_rng(5)
    rand, left = [], CLIP_SAMPLES
    while left:
        rand.append(min(left, int(rng.integers(1, 8001))))
        left -= rand[-1]
    ways = {"whole": [CLIP_SAMPLES], "per_frame": frame_pieces(CLIP_SAMPLES), "random_1_8000": rand,
            "one_sample_then_frames": [1] * 3000 + frame_pieces(CLIP_SAMPLES, 3000)}
    for name, pieces in ways.items():
        assert sum(pieces) == CLIP_SAMPLES
        mouth, poses = stream(models, wave, pieces, seed=7)
        assert np.array_equal(mouth, ref_mouth), name
        assert np.array_equal(poses.astype(np.float64), ref_poses), name
    # a caller's generator instead of the global one; rings three times shorter than the stream (max_chunk_samples 2000:
    # a sample buffer of ~3 000 samples and a projection ring of ~30 rows against 183 200 samples and 687 rows)
    g = torch.Generator().manual_seed(7)
    mouth, poses = stream(models, wave, [CLIP_SAMPLES], seed=99, max_chunk_samples=2000, generator=g)
    assert np.array_equal(mouth, ref_mouth) and np.array_equal(poses.astype(np.float64), ref_poses)


@pytest.mark.parametrize("frames", [1, 16])
def test_session_short_clips(models, frames):
    """1 frame: shorter than both lookaheads; 16 frames: between them -- one pose, and every mouth row only at finish()."""
    n = int(frames * 16000 / 60) + 1
    wave = wave_of(n, seed=frames)
    ref_mouth, ref_poses = whole_clip(models, wave, seed=3)
    s = session(models)
    torch.manual_seed(3)
    out = s.push(wave, host=True)
    assert len(out.mouth) == 0 and len(out.poses) == 0
    fin = s.finish(host=True)
    assert fin.mouth.shape == (frames, 75) and np.array_equal(fin.mouth, ref_mouth)
    assert fin.poses.shape == (max(frames - 15, 0), 12) and np.array_equal(fin.poses.astype(np.float64), ref_poses)


def test_session_memory_is_bounded(models):
    wave = wave_of(CLIP_SAMPLES, seed=4)
    s = session(models)
    pieces = frame_pieces(CLIP_SAMPLES)
    pos = 0
    for k in pieces[:40]:
        s.push(wave[pos:pos + k]); pos += k
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for rep in range(1000):
        k = pieces[40 + rep % (len(pieces) - 40)]
        if pos + k > CLIP_SAMPLES:
            pos = 0
        s.push(wave[pos:pos + k]); pos += k
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base


def test_session_refusals(models, tmp_path):
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.live import LiveAudioFrontEnd
    from livespeechportraits_amd.models import create_model
    s = session(models)
    with pytest.raises(ValueError):
        s.push(np.zeros(100, np.float64))
    with pytest.raises(ValueError):
        s.push(np.zeros((2, 100), np.float32))
    with pytest.raises(ValueError):
        s.push(torch.zeros(100, dtype=torch.float16, device=DEV))
    s.push(torch.zeros(100, device=DEV))
    s.finish()
    with pytest.raises(RuntimeError, match="ended"):
        s.push(np.zeros(1, np.float32))
    with pytest.raises(RuntimeError):
        s.finish()
    with pytest.raises(RuntimeError, match="GPU"):
        LiveAudioFrontEnd(models["apc"], models["a2f"], models["a2h"], models["db"], True, 10, 1.0,
                          np.zeros(12, np.float32), 0.3, device="cpu")
    ck = os.path.join(str(tmp_path), "Audio2Headpose.pkl")
    torch.save({"module." + k: torch.from_numpy(v) for k, v in synth.make_a2h_lstm_state_dict(512, 1, 12, "GMM").items()}, ck)
    lopt = argparse.Namespace(model="audio2headpose", gpu_ids=[0], isTrain=False, checkpoints_dir=str(tmp_path), name="x", load_epoch=ck,
                              verbose=False, feature_decoder="LSTM", loss="GMM", A2H_GMM_ndim=12, A2H_GMM_ncenter=1, APC_hidden_size=512,
                              frame_future=15)
    lstm = create_model(lopt)
    lstm.setup(lopt)
    with pytest.raises(NotImplementedError, match="LSTM"):
        LiveAudioFrontEnd(models["apc"], models["a2f"], lstm, models["db"], True, 10, 1.0, np.zeros(12, np.float32), 0.3, device=DEV,
                          feature_opt=models["fopt"], headpose_opt=lopt)


def test_session_real_time(models):
    """Per-push wall time (call -> frames on the host) for pushes of one frame of audio over the 687-frame clip, with the
    feature database of bench.py's pipeline (30 000 rows).  demo.py runs at 60 fps, so a frame of audio must be processed within
    1/60 s: that bound is derived, not tuned.  tools/live_latency.py records the same numbers in profiles/live_latency.txt."""
    import time
    from livespeechportraits_amd import synth
    m = dict(models, db=synth.make_feature_database(30000, 8, 512, 24)[0])
    wave = wave_of(CLIP_SAMPLES, seed=11)
    s = session(m)
    pos, ts = 0, []
    for k in frame_pieces(CLIP_SAMPLES):
        t0 = time.perf_counter()
        s.push(wave[pos:pos + k], host=True)
        ts.append(time.perf_counter() - t0)
        pos += k
    s.finish()
    ts = np.array(ts)
    p50, p99 = np.percentile(ts, 50), np.percentile(ts, 99)
    print("\n[live] per-frame push: p50 %.3f ms, p99 %.3f ms, max %.3f ms" % (p50 * 1e3, p99 * 1e3, ts.max() * 1e3))
    assert p99 < 1.0 / 60
