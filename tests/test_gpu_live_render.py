"""LivePortraitPool (livespeechportraits_amd/live_render.py): audio pushed into a pool, frames or JPEG files out of the same tick.

Nothing here has a tolerance of its own.  A session's live rows are those of a LiveSessionPool on the same audio (pinned on the whole-clip
audio path by tests/test_gpu_live_pool.py); its points must equal the landmark stage's whole-clip call on those rows (pinned on the
reference by tests/test_gpu_landmarks.py; the outer-lip points of flipped frames follow the streamed rule); its frames must equal, bit for
bit, what render_frames_from_landmarks returns for the same points in the pool's own groups; its JPEG files must equal JpegEncoder's."""
import argparse

import numpy as np
import pytest
import torch

import landmark_model as M
from test_gpu_landmarks import OUTER, make_stage
from test_gpu_live import DEV, models, wave_of  # noqa: F401  (models: the module-scoped fixture)
from test_gpu_live_pool import pool_of
from test_landmarks_cpu import load_case

pytestmark = pytest.mark.gpu

# the audio models carry synthetic weights, so their rows are not landmark-sized: the avatar's AMPs scale them down to a face that stays in view
AMPS = dict(amp=[0.004, 0.004, 0.004], rot_amp=0.5, trans_amp=0.002)


def _avatar():
    meta, a, cfg = load_case("may")
    meta = dict(meta, settings=dict(meta["settings"], **AMPS))
    cfg = dict(cfg, **AMPS)
    return meta, cfg


@pytest.fixture(scope="module")
def generators():
    import livespeechportraits_amd as L
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.topology import build_topology
    topo = build_topology("normal", ngf=64, num_downs=8, size=512)
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.make_state_dict(topo, 3).items()}
    out = {}
    for name, fp16 in (("f32", 0), ("f16", 1)):
        opt = argparse.Namespace(model="feature2face", gpu_ids=[0], isTrain=False, size="normal", ngf=64, n_downsample_G=8, fp16=fp16,
                                 checkpoints_dir=".", name="t", load_epoch="none", verbose=False)
        model = L.create_model(opt)
        model._g().load_state_dict(sd)
        model.eval()
        out[name] = model
    _, cand = synth.make_inputs(1, 512, seed=5, cand_batch=1)
    return out, torch.from_numpy(cand).to(DEV)


def _pieces(n, seed, top=4000):
    rng, out = np.random.default_rng(seed), []
    while n > 0:
        k = min(n, int(rng.integers(1, top)))
        out.append(k)
        n -= k
    return out


def _audio_rows(m, clips, seeds):
    """the live rows of every clip: a LiveSessionPool alone, one session per clip with its own generator"""
    pool = pool_of(m, max_sessions=len(clips))
    sids = {k: pool.open(np.zeros(12, np.float32), torch.Generator().manual_seed(seeds[k])) for k in clips}
    mouth, poses = {k: [] for k in clips}, {k: [] for k in clips}
    pos = {k: 0 for k in clips}
    pieces = {k: _pieces(len(w), 100 + k) for k, w in clips.items()}
    while any(pieces.values()):
        push = {}
        for k in clips:
            if pieces[k]:
                n = pieces[k].pop(0)
                push[sids[k]] = clips[k][pos[k]:pos[k] + n]
                pos[k] += n
        out = pool.tick(push, finish=[sids[k] for k in clips if sids[k] in push and not pieces[k]], host=True)
        for k in clips:
            if sids[k] in out:
                mouth[k].append(out[sids[k]].mouth)
                poses[k].append(out[sids[k]].poses)
    return {k: (np.concatenate(mouth[k]).astype(np.float32).reshape(-1, 75), np.concatenate(poses[k]).astype(np.float32).reshape(-1, 12)) for k in clips}


def _check_points(got, stage, rows, cfg, meta):
    n = min(rows[0].shape[0], rows[1].shape[0])
    assert got.shape == (n, 91, 2)
    if n == 0:
        return
    whole = stage.clip(rows[0], rows[1]).cpu().numpy()
    assert np.isfinite(whole).all() and whole.min() > -512 and whole.max() < 1024, "the synthetic rows leave the view: adjust AMPS"
    flip = M.mouth_path(rows[0], n, cfg)[2]
    differ = np.zeros((n, 91), bool)
    differ[np.ix_(flip, OUTER)] = True
    assert np.array_equal(got[~differ], whole[~differ])
    if len(flip):
        model = M.clip(rows[0], rows[1], cfg, meta["proj_f64"], outer="frame")["points"]
        assert np.abs(got[differ].astype(np.float64) - model[differ]).max() <= 2 * meta["reference_f32_error_px"]


@pytest.mark.parametrize("plan", ["f32", "f16"])
def test_pool_frames_equal_the_existing_path_on_the_pools_own_groups(models, generators, plan):
    from livespeechportraits_amd.jpeg import JpegEncoder
    from livespeechportraits_amd.live_render import LivePortraitPool
    from livespeechportraits_amd.render_loop import render_frames_from_landmarks
    gens, cand = generators
    model = gens[plan]
    meta, cfg = _avatar()
    nsamp = lambda frames: int(frames * 16000 / 60) + 1
    clips = {0: wave_of(nsamp(110), seed=21), 1: wave_of(nsamp(140), seed=22), 2: wave_of(nsamp(1), seed=23), 3: wave_of(nsamp(90), seed=24)}
    seeds = {k: 50 + k for k in clips}
    rows = _audio_rows(models, clips, seeds)
    check_stage = make_stage(cfg, meta, DEV, max_sessions=1)
    for k in clips:                                            # in view, before anything is drawn
        n = min(rows[k][0].shape[0], rows[k][1].shape[0])
        if n:
            w = check_stage.clip(*rows[k]).cpu().numpy()
            assert np.isfinite(w).all() and w.min() > -512 and w.max() < 1024, "the synthetic rows leave the view: adjust AMPS"

    pool = LivePortraitPool(pool_of(models, max_sessions=4), make_stage(cfg, meta, DEV, max_sessions=4), model, cand, max_batch=4)
    assert pool.delay == 18 + 40
    enc = JpegEncoder(512, 3, 75, DEV, max_batch=4)
    sids, pos = {}, {k: 0 for k in clips}
    pieces = {k: _pieces(len(w), 100 + k, top=1000) for k, w in clips.items()}     # about two frames of audio per tick
    start_tick = {0: 0, 1: 0, 2: 1, 3: 3}
    points = {k: [] for k in clips}
    nframes = {k: 0 for k in clips}
    tick = checked = jpegs = 0
    while any(pieces.values()) or len(sids) < len(clips):
        for k in clips:
            if k not in sids and start_tick[k] <= tick:
                sids[k] = pool.open(np.zeros(12, np.float32), torch.Generator().manual_seed(seeds[k]))
        push, fin = {}, []
        for k in clips:
            if k in sids and pieces[k]:
                n = pieces[k].pop(0)
                push[sids[k]] = clips[k][pos[k]:pos[k] + n]
                pos[k] += n
                if not pieces[k]:
                    fin.append(sids[k])
        as_jpeg = tick % 3 == 2 or bool(fin)
        out = pool.tick(push, finish=fin, host=True, jpeg_quality=75 if as_jpeg else None)
        assert set(out) == set(push)
        pts = pool.last_points.cpu().numpy()
        by = {sid: k for k, sid in sids.items()}
        at = 0
        for sid in sorted(out):
            start, frames = out[sid]
            k = by[sid]
            assert start == nframes[k]
            points[k].append(pts[at:at + len(frames)])
            at += len(frames)
            nframes[k] += len(frames)
        assert at == pts.shape[0] == sum(len(g) for g in pool.last_groups)
        assert all(1 <= len(g) <= 4 for g in pool.last_groups)
        # the same points, in the pool's own groups, through the existing path
        flat = [f for sid in sorted(out) for f in out[sid][1]]
        owner = [(sid, out[sid][0] + i) for sid in sorted(out) for i in range(len(out[sid][1]))]
        assert [o for g in pool.last_groups for o in g] == owner
        g0 = 0
        for g in pool.last_groups:
            p = pts[g0:g0 + len(g)]
            want = render_frames_from_landmarks(model, list(p[:, :73]), list(p[:, 73:]), cand, pad=None, load_size=512, batch=len(g))
            if as_jpeg:
                files = enc.encode(torch.from_numpy(np.stack(want)).to(DEV))
                assert all(isinstance(f, bytes) and f == w for f, w in zip(flat[g0:g0 + len(g)], files)), "JPEG bytes, tick %d" % tick
                jpegs += len(g)
            else:
                for f, w in zip(flat[g0:g0 + len(g)], want):
                    assert f.dtype == np.uint8 and f.shape == (512, 512, 3) and np.array_equal(f, w), "frame, tick %d" % tick
                checked += len(g)
            g0 += len(g)
        tick += 1
    assert not pool.open_sessions and not pool.audio.open_sessions and not pool.stage.sched
    assert checked >= 20 and jpegs >= 20, (checked, jpegs)
    for k in clips:
        got = np.concatenate(points[k]) if points[k] else np.zeros((0, 91, 2), np.float32)
        _check_points(got, check_stage, rows[k], cfg, meta)
    assert nframes[2] == 0 and nframes[1] == min(rows[1][0].shape[0], rows[1][1].shape[0]) >= 80


def test_a_reopened_slot_starts_clean(models, generators):
    """hazard leg: a session is closed mid-clip and its slot reopened with other audio; the new session's points and frames are those of a
    fresh pool (rings, carried states and the scheduler all start over)"""
    from livespeechportraits_amd.live_render import LivePortraitPool
    gens, cand = generators
    meta, cfg = _avatar()
    nsamp = lambda frames: int(frames * 16000 / 60) + 1
    first, second = wave_of(nsamp(150), seed=31), wave_of(nsamp(110), seed=32)

    def run(pool, sid, wave, seed, stop_after=None):
        pts, frames, pos = [], [], 0
        pieces = _pieces(len(wave), seed, top=1200)
        for i, n in enumerate(pieces):
            last = i == len(pieces) - 1
            out = pool.tick({sid: wave[pos:pos + n]}, finish=[sid] if last else [], host=True)
            pos += n
            pts.append(pool.last_points.cpu().numpy())
            frames.append(out[sid][1])
            if stop_after is not None and pos >= stop_after:
                return None
        return np.concatenate(pts), np.concatenate(frames)

    used = LivePortraitPool(pool_of(models, max_sessions=1), make_stage(cfg, meta, DEV, max_sessions=1), gens["f32"], cand, max_batch=8)
    s0 = used.open(np.zeros(12, np.float32), torch.Generator().manual_seed(1))
    run(used, s0, first, 7, stop_after=len(first) * 3 // 4)                # frames have been emitted, the rings are full
    assert used.stage.sched[used._lm[s0]].e > 0
    used.close(s0)
    s1 = used.open(np.zeros(12, np.float32), torch.Generator().manual_seed(2))
    assert used.audio.plan.slot[s1] == 0 and used.stage._slot[used._lm[s1]] == 0
    got = run(used, s1, second, 8)
    fresh = LivePortraitPool(pool_of(models, max_sessions=1), make_stage(cfg, meta, DEV, max_sessions=1), gens["f32"], cand, max_batch=8)
    want = run(fresh, fresh.open(np.zeros(12, np.float32), torch.Generator().manual_seed(2)), second, 8)
    assert got[0].shape[0] >= 60 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_pool_refusals(models, generators):
    from livespeechportraits_amd.live_render import LivePortraitPool
    gens, cand = generators
    meta, cfg = _avatar()
    with pytest.raises(ValueError, match="sessions"):
        LivePortraitPool(pool_of(models, max_sessions=4), make_stage(cfg, meta, DEV, max_sessions=2), gens["f32"], cand)
    with pytest.raises(ValueError, match="max_push"):
        LivePortraitPool(pool_of(models, max_sessions=1), make_stage(cfg, meta, DEV, max_sessions=1, max_push=20), gens["f32"], cand)
    pool = LivePortraitPool(pool_of(models, max_sessions=1), make_stage(cfg, meta, DEV, max_sessions=1), gens["f32"], cand)
    sid = pool.open(np.zeros(12, np.float32))
    with pytest.raises(ValueError, match="at most"):
        pool.tick({sid: np.zeros(pool.max_tick_samples + 1, np.float32)})
    with pytest.raises(ValueError, match="jpeg_quality"):
        pool.tick({sid: np.zeros(300, np.float32)}, jpeg_quality=0)
    with pytest.raises(KeyError):
        pool.tick({sid + 5: np.zeros(300, np.float32)})
    out = pool.tick({sid: np.zeros(300, np.float32)})                      # nothing final yet: an empty device tensor
    assert out[sid][0] == 0 and tuple(out[sid][1].shape) == (0, 512, 512, 3) and out[sid][1].is_cuda
    pool.close(sid)
    with pytest.raises(RuntimeError, match="closed"):
        pool.tick({sid: np.zeros(300, np.float32)})
