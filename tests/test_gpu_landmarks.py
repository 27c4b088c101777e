"""The landmark stage on the device (include/lsplmk.h, livespeechportraits_amd/landmarks.py) against the fixtures frozen from the
reference's own functions (tests/golden/landmarks_*, tools/make_golden_landmarks.py) and the numpy model (tests/landmark_model.py, itself
pinned to the fixtures by tests/test_landmarks_cpu.py).  Reads tests/golden/ only.

Bounds.  Float points: the device's error against the stored float64 evaluation may be at most 2 x the reference's own float32 error
against it (maxima per fixture; the device and the reference are two float32 evaluation orders of the same formulas -- the reference's
goes through BLAS).  Truncated points: int(x), what the rasteriser draws, equals the reference's for every coordinate whose reference
value is not within 1e-3 of an integer (at most 1 % of a fixture).  Streamed against whole clip: bit for bit."""
import numpy as np
import pytest
import torch

import landmark_model as M
from test_landmarks_cpu import CASES, load_case

pytestmark = pytest.mark.gpu

OUTER = M.UPPER_OUTER + M.LOWER_OUTER


def make_stage(cfg, meta, dev, **kw):
    from livespeechportraits_amd.landmarks import LandmarkStage
    st = meta["settings"]
    return LandmarkStage(cfg["mean_pts3d"], cfg["std_mean_pts3d"], cfg["candidate_eye_brow"], cfg["mean_translation"], cfg["camera_intrinsic"], cfg["scale"],
                         cfg["shoulder3D"], cfg["ref_trans"], shoulder_AMP=st["shoulder_amp"], AMP_method=st["amp_method"], Feat_AMPs=st["amp"],
                         rot_AMP=st["rot_amp"], trans_AMP=st["trans_amp"], Feat_smooth_sigma=st["mouth_sigma"], Head_smooth_sigma=st["head_sigma"],
                         relative_rotation=cfg["relative_rotation"], relative_translation=cfg["relative_translation"], image_pad=cfg["image_pad"],
                         device=dev, proj_f64=meta["proj_f64"], **kw)


@pytest.mark.parametrize("case", CASES)
def test_whole_clip_against_the_reference_fixture(gpu_device, case):
    from livespeechportraits_amd.feature_map import FeatureMapRasteriser
    meta, a, cfg = load_case(case)
    stage = make_stage(cfg, meta, gpu_device)
    mouth, poses = torch.from_numpy(a["pred_Feat"]).to(gpu_device), torch.from_numpy(a["pred_Head"]).to(gpu_device)
    pts = stage.clip(mouth, poses)
    torch.cuda.synchronize()
    assert torch.equal(mouth.cpu(), torch.from_numpy(a["pred_Feat"])) and torch.equal(poses.cpu(), torch.from_numpy(a["pred_Head"]))
    got, ref = pts.cpu().numpy(), a["points"]
    assert got.dtype == np.float32 and got.shape == ref.shape == (meta["nframe"], 91, 2)
    err = float(np.abs(got.astype(np.float64) - a["points_f64"]).max())
    print("%s: device vs float64 %.3g px, reference vs float64 %.3g px, device vs reference %.3g px"
          % (case, err, meta["reference_f32_error_px"], float(np.abs(got.astype(np.float64) - ref).max())))
    assert err <= 2 * meta["reference_f32_error_px"]
    near = np.abs(ref - np.round(ref)) < 1e-3
    assert near.mean() <= 0.01
    assert np.array_equal(got.astype(np.int32)[~near], ref.astype(np.int32)[~near])
    # what is drawn: the edge maps from the device's points and from the reference's, frame by frame
    ras = FeatureMapRasteriser(512, 18, gpu_device)
    clean = ~near.reshape(near.shape[0], -1).any(axis=1)
    assert clean.sum() >= 0.5 * len(clean)
    for k0 in range(0, len(clean), 32):
        mine = ras.rasterise_points(pts[k0:k0 + 32].contiguous(), as_uint8=True).cpu().numpy()
        theirs = ras.rasterise_points(torch.from_numpy(ref[k0:k0 + 32]).to(gpu_device), as_uint8=True).cpu().numpy()
        for i in range(mine.shape[0]):
            if clean[k0 + i]:
                assert np.array_equal(mine[i], theirs[i]), "edge map of frame %d differs" % (k0 + i)
        assert mine.any()
    # the same call from host arrays, and with the 6 pose columns alone
    again = stage.clip(a["pred_Feat"], np.ascontiguousarray(a["pred_Head"][:, :6]))
    assert torch.equal(again, pts)


def _sessions(a, n, rng):
    """n sessions on one avatar: slices of the fixture's rows of different lengths; most with fewer poses than mouth rows (as the audio
    stages make them), some the other way round, one shorter than every radius, one empty"""
    nm, nh = a["pred_Feat"].shape[0], a["pred_Head"].shape[0]
    out = {}
    for i in range(n):
        length = [0, 5, 30][i] if i < 3 else int(rng.integers(45, 110))
        off = int(rng.integers(0, min(nm, nh) - length + 1))
        lp = max(0, length - 15) if i % 4 != 3 else length
        lm = length if i % 4 != 3 else max(0, length - int(rng.integers(0, 9)))
        out[i] = (a["pred_Feat"][off:off + lm], a["pred_Head"][off:off + lp])
    return out


def run_streamed(stage, sessions, dev, seed, max_push, starts=None):
    """Drive ``sessions`` ({name: (mouth rows, poses)}) through the stage with ragged pushes; a session opens at its start tick (or when a
    slot is free), pushes 0..max_push rows of each kind per tick and finishes with or after its last rows.  -> {name: points}; the per-tick
    emission is checked against the scheduler's rule on the way."""
    rng = {k: np.random.default_rng([seed, k]) for k in sessions}
    dev_rows = {k: (torch.from_numpy(np.ascontiguousarray(m)).to(dev), torch.from_numpy(np.ascontiguousarray(p)).to(dev)) for k, (m, p) in sessions.items()}
    starts = starts or {k: 0 for k in sessions}
    waiting, live, done = sorted(sessions), {}, {}
    pos, parts = {}, {k: [] for k in sessions}
    tick = 0
    while waiting or live:
        for k in list(waiting):
            if starts[k] <= tick and len(live) < stage.max_sessions:
                live[k] = stage.open()
                pos[k] = [0, 0]
                waiting.remove(k)
        frames, finish = {}, []
        for k, sid in live.items():
            m, p = dev_rows[k]
            r = rng[k]
            nm, np_ = min(int(r.integers(0, max_push + 1)), m.shape[0] - pos[k][0]), min(int(r.integers(0, max_push + 1)), p.shape[0] - pos[k][1])
            if pos[k][0] < m.shape[0] and pos[k][1] < p.shape[0] and abs(pos[k][0] + nm - pos[k][1] - np_) > 20:
                nm, np_ = (nm, 0) if pos[k][0] < pos[k][1] else (0, np_)
            if r.integers(0, 5) == 0:
                continue                                        # this session sits the tick out
            frames[sid] = (m[pos[k][0]:pos[k][0] + nm], pos[k][0], p[pos[k][1]:pos[k][1] + np_], pos[k][1])
            pos[k][0] += nm
            pos[k][1] += np_
            if pos[k][0] == m.shape[0] and pos[k][1] == p.shape[0] and r.integers(0, 2) == 0:
                finish.append(sid)
        out = stage.tick(frames, finish=finish)
        assert set(out) == set(frames) | set(finish)
        for k, sid in list(live.items()):
            if sid in out:
                start, pts = out[sid]
                assert start == sum(t.shape[0] for t in parts[k])
                parts[k].append(pts)
            if sid in finish:
                done[k] = torch.cat(parts[k]) if parts[k] else torch.empty(0, 91, 2, device=dev)
                del live[k]
        tick += 1
        assert tick < 2000
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in done.items()}


def _check_streamed(got, stage, sessions, cfg, meta, dev, max_lookahead=None):
    """bit for bit the whole-clip call's, except the outer-lip points of flipped frames: those follow the model's streamed rule"""
    flipped = 0
    for k, (m, p) in sessions.items():
        n = min(m.shape[0], p.shape[0])
        assert got[k].shape == (n, 91, 2), (k, got[k].shape, n)
        if n == 0:
            continue
        whole = stage.clip(m, p).cpu().numpy()
        flip = M.mouth_path(m, n, cfg)[2]
        differ = np.zeros((n, 91), bool)
        differ[np.ix_(flip, OUTER)] = True
        assert np.array_equal(got[k][~differ], whole[~differ]), "session %d: a streamed point differs from the whole-clip call" % k
        if len(flip):
            model = M.clip(m, p, cfg, meta["proj_f64"], outer="frame")["points"]
            assert np.abs(got[k][differ].astype(np.float64) - model[differ]).max() <= 2 * meta["reference_f32_error_px"]
            flipped += len(flip)
    return flipped


def test_streamed_sessions_equal_the_whole_clip_call(gpu_device):
    """16 slots, 22 sessions of different lengths with ragged pushes: six join when a slot has become free.  Then session 7 alone, with
    the same pushes: its points do not depend on who shares the tick."""
    meta, a, cfg = load_case("crossed")
    rng = np.random.default_rng(11)
    sessions = _sessions(a, 22, rng)
    sessions[21] = (a["pred_Feat"][20:110], a["pred_Head"][20:95])          # one that surely contains the crossed stretch
    starts = {k: int(rng.integers(0, 6)) if k < 16 else 8 for k in sessions}
    stage = make_stage(cfg, meta, gpu_device, max_push=16)
    got = run_streamed(stage, sessions, gpu_device, seed=3, max_push=16, starts=starts)
    assert _check_streamed(got, stage, sessions, cfg, meta, gpu_device) >= 20
    assert not stage.sched and len(stage._free) == 16
    for k in (7, 21):
        alone = run_streamed(make_stage(cfg, meta, gpu_device, max_push=16, max_sessions=1), {k: sessions[k]}, gpu_device, seed=3, max_push=16)
        assert np.array_equal(alone[k], got[k])


@pytest.mark.parametrize("case", ["delta", "xy", "lowermore", "short"])
def test_streamed_amp_methods_and_short_clips(gpu_device, case):
    """the delta AMP reads the smoothed frame before; a mouth sigma of 0; clips shorter than the radii, which only finish can emit"""
    meta, a, cfg = load_case(case)
    sessions = {0: (a["pred_Feat"], a["pred_Head"]), 1: (a["pred_Feat"][3:40], a["pred_Head"][3:33]), 2: (a["pred_Feat"][:7], a["pred_Head"][:9])}
    stage = make_stage(cfg, meta, gpu_device, max_push=8, max_sessions=3)
    got = run_streamed(stage, sessions, gpu_device, seed=case.__len__(), max_push=8)
    _check_streamed(got, stage, sessions, cfg, meta, gpu_device)
    whole = stage.clip(a["pred_Feat"], a["pred_Head"]).cpu().numpy()
    assert np.abs(whole.astype(np.float64) - a["points_f64"]).max() <= 2 * meta["reference_f32_error_px"]


@pytest.mark.parametrize("lookahead", [0, 8])
def test_max_lookahead_follows_the_models_truncated_window(gpu_device, lookahead):
    """not the reference's filter: pinned on the numpy restatement only, to the float tolerance"""
    meta, a, cfg = load_case("crossed")
    stage = make_stage(cfg, meta, gpu_device, max_push=8, max_sessions=4, max_lookahead=lookahead)
    sessions = {0: (a["pred_Feat"], a["pred_Head"]), 1: (a["pred_Feat"][10:25], a["pred_Head"][10:22]), 2: (a["pred_Feat"][30:100], a["pred_Head"][30:100])}
    got = run_streamed(stage, sessions, gpu_device, seed=5, max_push=8)
    for k, (m, p) in sessions.items():
        model = M.clip(m, p, cfg, meta["proj_f64"], outer="frame", max_lookahead=lookahead)["points"]
        err = float(np.abs(got[k].astype(np.float64) - model).max())
        print("lookahead %d, session %d: device vs model %.3g px" % (lookahead, k, err))
        assert err <= 2 * meta["reference_f32_error_px"]
    exact = M.clip(*sessions[0], cfg, meta["proj_f64"], outer="frame")["points"]
    assert np.abs(got[0] - exact).max() > 0.05                 # and it IS another filter
    # the delay is the stated number of frames: one row of each kind per tick
    sid = stage.open()
    m, p = torch.from_numpy(a["pred_Feat"]).to(gpu_device), torch.from_numpy(a["pred_Head"]).to(gpu_device)
    for t in range(60):                                        # the start reflection reads rows 0..39: the first frame waits for them
        start, pts = stage.tick({sid: (m[t:t + 1], t, p[t:t + 1], t)})[sid]
        assert pts.shape[0] == (0 if t < 39 else 40 - lookahead if t == 39 else 1) and (t <= 39 or start == t - lookahead)
    stage.close(sid)


def test_refusals(gpu_device):
    meta, a, cfg = load_case("short")
    from livespeechportraits_amd.landmarks import LandmarkStage
    base = dict(shoulder_AMP=0.5, AMP_method="XYZ", Feat_AMPs=[2, 2, 2], rot_AMP=1, trans_AMP=0.5, Feat_smooth_sigma=1.5, Head_smooth_sigma=[5, 10], device=gpu_device)
    args = (cfg["mean_pts3d"], cfg["std_mean_pts3d"], cfg["candidate_eye_brow"], cfg["mean_translation"], cfg["camera_intrinsic"], cfg["scale"], cfg["shoulder3D"], cfg["ref_trans"])
    with pytest.raises(NotImplementedError, match="CloseSmall"):
        LandmarkStage(*args, **dict(base, AMP_method="CloseSmall", Feat_AMPs=[1] * 6))
    with pytest.raises(ValueError, match="sigma of 0"):
        LandmarkStage(*args, **dict(base, Head_smooth_sigma=[0, 10]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        LandmarkStage(*args, **dict(base, device="cpu"))
    stage = LandmarkStage(*args, **dict(base, max_sessions=2, max_push=4, max_skew=4))
    s0, s1 = stage.open(), stage.open()
    with pytest.raises(RuntimeError, match="sessions of the stage are open"):
        stage.open()
    m, p = torch.from_numpy(a["pred_Feat"]).to(gpu_device), torch.from_numpy(a["pred_Head"]).to(gpu_device)
    with pytest.raises(ValueError, match="expects"):
        stage.tick({s0: (m[:2], 1, p[:2], 0)})
    for t in range(0, 88, 4):
        stage.tick({s0: (m[:4], t, None, 0)})                  # mouth rows alone: nothing can be emitted, the ring fills
    with pytest.raises(RuntimeError, match="ring"):
        stage.tick({s0: (m[:4], 88, None, 0), s1: (m[:2], 0, p[:2], 0)})
    assert stage.sched[s1].m == 0 and stage.sched[s0].m == 88   # the refused tick changed nothing
    stage.close(s0)
    with pytest.raises(KeyError):
        stage.tick({s0: (m[:1], 0, p[:1], 0)})
    assert stage.finish(s1)[1].shape == (0, 91, 2)
