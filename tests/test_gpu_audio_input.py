"""The audio input stage on the device (include/lsprs.h, livespeechportraits_amd/audio_input.py) against the float64 restatement of its
contract (tests/resample_model.py, itself held to scipy's polyphase resampler by tests/test_audio_input_cpu.py), and against itself.

Bounds.  Against the model: the device's max-abs error may be at most 4 x the error of the model's own float32 sequential restatement on
the same input (3-5e-7 for N(0, 0.3) input); the margin covers fmaf against separate rounding of product and sum.  Stop band: a 10 kHz
tone at 48 kHz in comes out below -100 dB (the float64 model gives -154 dB, float32 rounding puts the floor near -123 dB, a wrong phase
or tap offset shows above -60 dB).  Everything else is bit for bit: pieces against the whole, a session in a crowd against the session
alone, int16 stereo against its host-converted mono, the pool's frames against a pool fed the resampled clip, the recorded audio."""
import numpy as np
import pytest
import torch

import avi_parser as P
import resample_model as RM
from test_audio_input_cpu import _wav
from test_gpu_landmarks import make_stage
from test_gpu_live import DEV, models, wave_of  # noqa: F401  (models: the module-scoped fixture)
from test_gpu_live_pool import pool_of
from test_gpu_live_render import _avatar, generators  # noqa: F401  (generators: the module-scoped fixture)

pytestmark = pytest.mark.gpu

CLIP_LENGTHS = {48000: 2000, 44100: 1500, 32000: 1300, 24000: 1000, 22050: 800, 8000: 300}      # 667, 545, 650, 667, 581, 600 outputs
STREAM_RATES = (48000, 44100, 8000)
MAX_PUSH = 3000


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture(scope="module")
def all_rates():
    from livespeechportraits_amd.audio_input import AudioInputStage
    return [AudioInputStage(RM.RATES[:3], DEV, max_sessions=1, max_push=64), AudioInputStage(RM.RATES[3:], DEV, max_sessions=1, max_push=64)]


@pytest.fixture(scope="module")
def stage():
    from livespeechportraits_amd.audio_input import AudioInputStage
    return AudioInputStage(STREAM_RATES, DEV, max_sessions=16, max_push=MAX_PUSH)


def _noise(n, seed, fmt="f32", channels=1):
    x = np.random.default_rng(seed).normal(0, 0.3, (n, channels) if channels > 1 else n)
    if fmt == "s16":
        return np.clip(np.rint(x * 32768 / 2), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


@pytest.mark.parametrize("rate", RM.RATES)
def test_whole_clip_against_the_float64_model(all_rates, rate):
    st = all_rates[0] if rate in all_rates[0].rates[:3] else all_rates[1]
    L, M, R = RM.ratio(rate)
    main = CLIP_LENGTHS[rate]
    assert RM.n_out(rate, main) > 2 * 256 and RM.n_out(rate, main) % 256
    if rate == 44100:
        phases = np.bincount((np.arange(RM.n_out(rate, main)) * M) % L, minlength=L)
        assert phases.min() >= 3
    for n in (main, 1, 5, R):
        x = _noise(n, rate + n)
        got = st.resample_clip(x, rate).cpu().numpy()
        want = RM.resample64(x.astype(np.float64), rate)
        assert got.dtype == np.float32 and got.shape == want.shape == (RM.n_out(rate, n),)
        err = np.abs(got - want).max()
        own = np.abs(RM.resample32_sequential(x, rate) - want).max()
        print("rate %d, %d samples -> %d: device vs float64 model %.3g, float32 sequential restatement vs the model %.3g" % (rate, n, len(got), err, own))
        assert err <= 4 * own


def test_a_tone_above_the_band_is_stopped(stage):
    n = 12000
    x = np.sin(2 * np.pi * 10000 * np.arange(n) / 48000).astype(np.float32)
    y = stage.resample_clip(x, 48000).cpu().numpy().astype(np.float64)
    mid = y[len(y) // 4: len(y) * 3 // 4]
    level = 20 * np.log10(np.sqrt(np.mean(mid ** 2)) / np.sqrt(np.mean(x.astype(np.float64) ** 2)))
    print("10 kHz at 48 kHz in: %.1f dB re the input" % level)
    assert level < -100


def _stream(st, raw, rate, pieces, fmt="f32", channels=1, last_push=True, device_every=3):
    """push ``raw`` in ``pieces`` through one session -> the concatenated output; every ``device_every``-th piece goes in as a device tensor"""
    sid = st.open(rate, fmt, channels)
    out, pos, nxt = [], 0, 0
    for i, k in enumerate(pieces):
        piece = raw[pos:pos + k]
        pos += k
        if i % device_every == 1:
            piece = torch.from_numpy(np.ascontiguousarray(piece)).to(DEV)
        fin = last_push and i == len(pieces) - 1
        start, y = st.tick({sid: piece}, finish=[sid] if fin else [])[sid]
        assert start == nxt and y.is_cuda and y.dtype == torch.float32
        nxt += y.shape[0]
        out.append(y)
    if not last_push:
        start, y = st.finish(sid)
        assert start == nxt
        out.append(y)
    assert pos == len(raw) and sid not in st.open_sessions
    return torch.cat(out)


def _pieces(rate, total, seed):
    M = RM.ratio(rate)[1]
    head = [1, 7, 0, 800, 799, 2, M - 1, 3000]
    rng, out = np.random.default_rng(seed), list(head)
    while sum(out) < total:
        out.append(min(int(rng.integers(0, MAX_PUSH + 1)), total - sum(out)))
    return out


@pytest.mark.parametrize("rate", STREAM_RATES)
def test_pushed_in_pieces_equals_pushed_at_once(stage, rate):
    ring = stage.history + stage.max_push
    total = 3 * ring + 517
    x = _noise(total, rate)
    whole = stage.resample_clip(x, rate)
    pieces = _pieces(rate, total, rate)
    assert sum(pieces) == total > 3 * ring and whole.shape[0] == RM.n_out(rate, total)
    before = stage.launches
    assert same_bits(_stream(stage, x, rate, pieces, last_push=True), whole)
    assert stage.launches - before == sum(1 for k in pieces if k)                  # one launch per tick that brings samples (an empty push emits nothing)
    assert same_bits(_stream(stage, x, rate, pieces, last_push=False), whole)


def test_sixteen_sessions_in_one_tick_equal_each_alone(stage):
    rng = np.random.default_rng(16)
    spec = [(STREAM_RATES[i % 3], "s16" if i % 2 else "f32", 2 if (i // 2) % 2 else 1) for i in range(16)]
    raws = [_noise(int(rng.integers(2000, 5000)), 100 + i, fmt, ch) for i, (rate, fmt, ch) in enumerate(spec)]
    cuts = []
    for raw in raws:                                                               # four ticks each; a session may bring nothing to a tick
        c = sorted(int(v) for v in rng.integers(0, len(raw) + 1, 3))
        cuts.append([c[0], c[1] - c[0], c[2] - c[1], len(raw) - c[2]])
    sids = [stage.open(*s) for s in spec]
    assert len(stage.open_sessions) == 16
    with pytest.raises(RuntimeError, match="all 16"):
        stage.open(48000)
    got, pos = [[] for _ in spec], [0] * 16
    before = stage.launches
    for t in range(4):
        push = {}
        for i, sid in enumerate(sids):
            piece = raws[i][pos[i]:pos[i] + cuts[i][t]]
            pos[i] += cuts[i][t]
            if cuts[i][t] or i % 5:
                push[sid] = torch.from_numpy(np.ascontiguousarray(piece)).to(DEV) if (i + t) % 4 == 0 else piece
        out = stage.tick(push, finish=sids if t == 3 else [])
        for i, sid in enumerate(sids):
            if sid in out:
                got[i].append(out[sid][1])
    assert stage.launches - before == 4 and not stage.open_sessions                # ONE launch per tick, whatever the sessions
    for i, (rate, fmt, ch) in enumerate(spec):
        alone = _stream(stage, raws[i], rate, cuts[i], fmt, ch)
        assert same_bits(torch.cat(got[i]), alone), spec[i]
        assert same_bits(alone, stage.resample_clip(raws[i], rate))


@pytest.mark.parametrize("rate", [48000, 44100])
def test_s16_stereo_equals_f32_mono_of_the_host_converted_samples(stage, rate):
    raw = _noise(1777, 5, "s16", 2)
    raw[:4] = [[32767, 32767], [-32768, -32768], [32767, -32768], [1, 0]]
    mono = RM.to_mono_f32(raw)
    assert same_bits(stage.resample_clip(raw, rate), stage.resample_clip(mono, rate))
    assert same_bits(stage.resample_clip(raw[:, 0].copy(), rate), stage.resample_clip(RM.to_mono_f32(raw[:, 0]), rate))
    f2 = _noise(900, 6, "f32", 2)
    assert same_bits(stage.resample_clip(f2, rate), stage.resample_clip(RM.to_mono_f32(f2), rate))


def test_sixteen_kilohertz_is_not_resampled(stage):
    x = _noise(1234, 7)
    before = stage.launches
    assert same_bits(stage.resample_clip(x, 16000), x)
    sid = stage.open(16000)
    a = stage.tick({sid: x[:700]})[sid]
    b = stage.tick({sid: torch.from_numpy(x[700:]).to(DEV)}, finish=[sid])[sid]
    assert (a[0], b[0]) == (0, 700) and same_bits(torch.cat([a[1], b[1]]), x)
    assert stage.launches == before                                                # the input bits, no launch
    raw = _noise(1000, 8, "s16", 2)                                                # int16 stereo at 16 kHz: converted and downmixed, not filtered
    assert same_bits(stage.resample_clip(raw, 16000), RM.to_mono_f32(raw))
    assert same_bits(_stream(stage, raw, 16000, [300, 0, 700], "s16", 2), RM.to_mono_f32(raw))


def test_a_poisoned_ring_changes_nothing():
    from livespeechportraits_amd.audio_input import AudioInputStage
    st = AudioInputStage([44100], DEV, max_sessions=2, max_push=500)
    x = _noise(3 * (st.history + 500) + 11, 9)
    whole = st.resample_clip(x, 44100)
    st._state.fill_(float("nan"))
    st.open(44100)                                                                 # slot 0 stays idle; the stream runs in slot 1
    pieces = [500] * (len(x) // 500) + [len(x) % 500]
    got = _stream(st, x, 44100, pieces)
    assert st._state.view(2, -1)[0].isnan().all() and same_bits(got, whole) and not got.isnan().any()


def test_refused_arguments_change_nothing(stage):
    x = _noise(4000, 10)
    sid = stage.open(48000)
    first = stage.tick({sid: x[:1000]})[sid][1]
    before = stage.launches
    with pytest.raises(ValueError, match="f32"):
        stage.tick({sid: x[1000:2000].astype(np.float64)})
    with pytest.raises(ValueError, match="f32"):
        stage.tick({sid: np.zeros((10, 2), np.float32)})
    with pytest.raises(ValueError, match="max_push"):
        stage.tick({sid: np.zeros(MAX_PUSH + 1, np.float32)})
    with pytest.raises(KeyError):
        stage.tick({sid: x[1000:2000], sid + 1000: x[:10]})
    with pytest.raises(ValueError, match="not one of"):
        stage.open(32000)
    with pytest.raises(ValueError, match="channels"):
        stage.open(48000, "s16", 3)
    assert stage.launches == before
    rest = stage.tick({sid: x[1000:]}, finish=[sid])[sid][1]
    assert same_bits(torch.cat([first, rest]), stage.resample_clip(x, 48000))
    with pytest.raises(KeyError):
        stage.tick({sid: x[:10]})


def test_load_audio_resamples_a_stereo_s16_file(stage, tmp_path):
    from livespeechportraits_amd.audio_input import load_audio
    raw = _noise(2205, 11, "s16", 2)
    path = tmp_path / "a.wav"
    path.write_bytes(_wav(raw, 44100, before=[(b"LIST", b"odd")]))
    want = stage.resample_clip(raw, 44100)
    assert want.shape[0] == 800
    assert same_bits(load_audio(str(path), device=DEV), want) and same_bits(load_audio(str(path), device=DEV, stage=stage), want)
    ref = _noise(999, 12)
    path.write_bytes(_wav(ref, 16000))                                             # shaped like the reference's clip: format 3, mono, 16 kHz
    before = stage.launches
    got = load_audio(str(path), device=DEV, stage=stage)
    assert got.is_cuda and same_bits(got, ref) and stage.launches == before


# ---- inside LivePortraitPool ---------------------------------------------------------------------------------------------------------------
FRAMES = 72


@pytest.fixture(scope="module")
def pool_runs(models, generators, tmp_path_factory):
    """A session opened at 48 kHz int16 (recorded) and a plain 16 kHz session, a frame of audio per tick, in one pool with the input stage;
    then a pool built without it, fed the resampled clip in the pieces the stage emitted, and the same plain audio."""
    from livespeechportraits_amd.audio_input import AudioInputStage
    from livespeechportraits_amd.live_render import LivePortraitPool
    from livespeechportraits_amd.video import AviWriter
    gens, cand = generators
    meta, cfg = _avatar()
    root = tmp_path_factory.mktemp("audio_input")
    raw = np.clip(np.rint(wave_of(FRAMES * 800 + 311, seed=71) * 32768), -32768, 32767).astype(np.int16)
    plain = wave_of(FRAMES * 267 + 100, seed=72)
    inp = AudioInputStage([48000], DEV, max_sessions=2, max_push=4000)
    whole = inp.resample_clip(raw, 48000)

    def make(audio_input, **kw):
        return LivePortraitPool(pool_of(models, max_sessions=2), make_stage(cfg, meta, DEV, max_sessions=2), gens["f32"], cand, max_batch=4,
                                audio_input=audio_input, **kw)

    def run(pool, a_pieces, a_clip, b_pieces, open_a):
        sa = open_a(pool)
        sb = pool.open(np.zeros(12, np.float32), torch.Generator().manual_seed(82))
        res = {sa: [], sb: []}
        heard, pa, pb = [], 0, 0
        for t, (ka, kb) in enumerate(zip(a_pieces, b_pieces)):
            last = t == len(a_pieces) - 1
            out = pool.tick({sa: a_clip[pa:pa + ka], sb: plain[pb:pb + kb]}, finish=[sa, sb] if last else [])
            pa, pb = pa + ka, pb + kb
            for sid in (sa, sb):
                res[sid].append((out[sid][0], out[sid][1].cpu().numpy()))
            if sa in pool.last_heard:
                heard.append(pool.last_heard[sa])
        assert not pool.open_sessions
        return res[sa], res[sb], heard

    a_pieces = [800] * FRAMES + [311]
    b_pieces = [267] * FRAMES + [100]
    writer = AviWriter(str(root / "a.avi"), 512, 512)
    first = make(inp, record_quality=75)
    assert first.delay == 18 + 40
    launches = inp.launches
    fa, fb, heard = run(first, a_pieces, raw, b_pieces,
                        lambda p: p.open(np.zeros(12, np.float32), torch.Generator().manual_seed(81), video=writer, input_rate=48000, input_format="s16"))
    launches = inp.launches - launches
    writer.close()
    assert not inp.open_sessions
    second = make(None)
    sa, sb, none = run(second, [h[1].shape[0] for h in heard], whole, b_pieces, lambda p: p.open(np.zeros(12, np.float32), torch.Generator().manual_seed(81)))
    return dict(first=(fa, fb), second=(sa, sb), heard=heard, whole=whole, launches=launches, ticks=len(a_pieces), avi=open(writer.path, "rb").read(), none=none)


def test_a_48_khz_session_renders_what_its_resampled_clip_renders(pool_runs):
    r = pool_runs
    assert r["launches"] == r["ticks"] and r["none"] == []
    heard = r["heard"]
    assert [h[0] for h in heard] == list(np.cumsum([0] + [h[1].shape[0] for h in heard[:-1]]))
    assert same_bits(torch.cat([h[1] for h in heard]), r["whole"])                 # the models heard the whole-clip signal, in pieces
    for got, want in zip(r["first"], r["second"]):                                 # the 48 kHz session, then the plain one beside it
        assert [g[0] for g in got] == [w[0] for w in want]
        assert sum(len(g[1]) for g in got) >= 10
        for g, w in zip(got, want):
            assert g[1].dtype == np.uint8 and g[1].shape == w[1].shape and np.array_equal(g[1], w[1])


def test_the_recorded_audio_is_what_the_models_heard(pool_runs):
    p = P.parse(pool_runs["avi"])
    n = len(p["video"])
    assert n == sum(len(g[1]) for g in pool_runs["first"][0]) >= 10
    assert [st["strf"]["nSamplesPerSec"] for st in p["streams"] if "nSamplesPerSec" in st["strf"]] == [16000]
    want = pool_runs["whole"].cpu().numpy()[:n * 16000 // 60]
    assert p["audio"].dtype == np.float32 and p["audio"].tobytes() == want.tobytes()


def test_pool_refusals_leave_the_pool_as_it_was(models, generators):
    from livespeechportraits_amd.audio_input import AudioInputStage
    from livespeechportraits_amd.live_render import LivePortraitPool
    gens, cand = generators
    meta, cfg = _avatar()
    inp = AudioInputStage([48000], DEV, max_sessions=1, max_push=20000)
    with pytest.raises(ValueError, match="input stage has 1 sessions"):
        LivePortraitPool(pool_of(models, max_sessions=2), make_stage(cfg, meta, DEV, max_sessions=2), gens["f32"], cand, audio_input=inp)
    plain = LivePortraitPool(pool_of(models, max_sessions=1), make_stage(cfg, meta, DEV, max_sessions=1), gens["f32"], cand)
    with pytest.raises(ValueError, match="without audio_input"):
        plain.open(np.zeros(12, np.float32), input_rate=48000)
    with pytest.raises(ValueError, match="go with input_rate"):
        plain.open(np.zeros(12, np.float32), input_format="s16")
    pool = LivePortraitPool(pool_of(models, max_sessions=1), make_stage(cfg, meta, DEV, max_sessions=1), gens["f32"], cand, audio_input=inp)
    with pytest.raises(ValueError, match="not one of"):
        pool.open(np.zeros(12, np.float32), input_rate=44100)
    assert not pool.open_sessions and not pool.audio.open_sessions and not inp.open_sessions
    sid = pool.open(np.zeros(12, np.float32), input_rate=48000, input_format="s16", input_channels=2)
    with pytest.raises(ValueError, match="at 16 kHz"):
        pool.tick({sid: np.zeros((3 * pool.max_tick_samples + 3, 2), np.int16)})
    with pytest.raises(ValueError, match="s16"):
        pool.tick({sid: np.zeros((800, 2), np.float32)})
    assert inp.launches == 0 and inp._sess[pool._in[sid]].sched.n == 0
    out = pool.tick({sid: np.zeros((800, 2), np.int16)})
    assert out[sid][0] == 0 and tuple(out[sid][1].shape) == (0, 512, 512, 3) and inp.launches == 1
    assert pool.last_heard[sid][1].shape[0] == (800 - 192 + 2) // 3
    pool.close(sid)
    assert not inp.open_sessions
