"""The landmark stage without a device: the numpy model (tests/landmark_model.py) against the fixtures frozen from the reference's own
functions (tools/make_golden_landmarks.py), the pure-Python LandmarkScheduler, the host half of the C ABI (include/lsplmk.h) and its
ctypes declarations."""
import ctypes
import glob
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import landmark_model as M

CASES = sorted(os.path.basename(p)[len("landmarks_"):-len(".json")] for p in glob.glob(os.path.join(GOLDEN, "landmarks_*.json")))


def load_case(name):
    with open(os.path.join(GOLDEN, "landmarks_%s.json" % name)) as f:
        meta = json.load(f)
    a = dict(np.load(os.path.join(GOLDEN, "landmarks_%s.npz" % name)))
    a.update(np.load(os.path.join(GOLDEN, "landmarks_%s_points.npz" % name)))
    cfg = dict(meta["settings"])
    for k in ("mean_pts3d", "std_mean_pts3d", "candidate_eye_brow", "mean_translation", "ref_trans", "camera_intrinsic", "relative_rotation",
              "relative_translation", "shoulder3D"):
        cfg[k] = a[k]
    cfg["scale"] = a["scale"][()]                     # numpy.float64, as sio.loadmat(...)['scale'][0, 0]
    cfg["image_pad"] = [int(v) for v in a["image_pad"]]
    return meta, a, cfg


def test_the_fixture_set_covers_what_it_must():
    assert {"may", "obama1", "short", "xy", "lowermore", "delta", "crossed"} <= set(CASES)
    metas = {c: load_case(c)[0] for c in CASES}
    assert metas["may"]["nframe"] >= 300 and metas["obama1"]["nframe"] >= 300
    assert metas["may"]["settings"] == dict(mouth_sigma=1.5, head_sigma=[5, 10], amp_method="XYZ", amp=[2, 2, 2], rot_amp=1, trans_amp=0.5, shoulder_amp=0.5)
    assert metas["obama1"]["settings"] == dict(mouth_sigma=1, head_sigma=[2, 8], amp_method="XYZ", amp=[1.5, 1.5, 1.5], rot_amp=1, trans_amp=1, shoulder_amp=0.5)
    assert metas["short"]["nframe"] < M.radius(min(metas["short"]["settings"]["head_sigma"]))
    assert {m["settings"]["amp_method"] for m in metas.values()} == {"XY", "XYZ", "LowerMore", "delta"}
    assert metas["crossed"]["flipped_frames"] >= 20
    assert any(m["settings"]["mouth_sigma"] == 0 for m in metas.values())


@pytest.mark.parametrize("case", CASES)
def test_model_reproduces_the_reference_at_every_tap(case):
    """Bit for bit where the reference's arithmetic is numpy / scipy element-wise code; the projected points go through BLAS ``dot`` in the
    reference, so they agree to 2 x the reference's own float32 error against a float64 evaluation (two float32 evaluation orders of the
    same formula), which the generator measured and stored."""
    meta, a, cfg = load_case(case)
    got = M.clip(a["pred_Feat"], a["pred_Head"], cfg, meta["proj_f64"])
    for tap in ("mouth_smooth", "mouth_final", "headpose", "final_pts3d"):
        assert got[tap].dtype == a[tap].dtype and got[tap].shape == a[tap].shape, tap
        assert np.array_equal(got[tap], a[tap]), "%s: max |diff| %.3g" % (tap, np.abs(got[tap].astype(np.float64) - a[tap]).max())
    assert got["points"].dtype == np.float32 and got["points"].shape == a["points"].shape == (meta["nframe"], 91, 2)
    err = float(np.abs(got["points"].astype(np.float64) - a["points"]).max())
    print("%s: model vs reference points %.3g px (reference vs float64 %.3g px)" % (case, err, meta["reference_f32_error_px"]))
    assert err <= 2 * meta["reference_f32_error_px"]
    # the float64 yardstick itself is the stored one
    assert np.array_equal(M.project_f64(a["headpose"], a["final_pts3d"], cfg), a["points_f64"])
    assert meta["reference_f32_error_px"] == float(np.abs(a["points"].astype(np.float64) - a["points_f64"]).max())


@pytest.mark.parametrize("case", CASES)
def test_near_integer_coordinates_are_rare_and_the_model_truncates_like_the_reference(case):
    """int(x) is what the rasteriser draws.  Coordinates whose reference value lies within 1e-3 of an integer are left out of that
    comparison; they may be at most 1 % of a fixture (0.2 % expected for spread-out coordinates)."""
    meta, a, cfg = load_case(case)
    ref = a["points"]
    near = np.abs(ref - np.round(ref)) < 1e-3
    assert near.mean() <= 0.01 and abs(near.mean() - meta["near_integer_share"]) < 1e-12
    got = M.clip(a["pred_Feat"], a["pred_Head"], cfg, meta["proj_f64"])["points"]
    assert np.array_equal(got.astype(np.int32)[~near], ref.astype(np.int32)[~near])
    assert ref.min() >= 0 and ref.max() < 512


def test_streamed_rules_of_the_model():
    """outer="frame" changes only the outer-lip y of flipped frames; max_lookahead >= the radii changes nothing; a cut window changes the
    filtered values and keeps unit gain"""
    meta, a, cfg = load_case("crossed")
    clip = M.clip(a["pred_Feat"], a["pred_Head"], cfg, meta["proj_f64"])
    frame = M.clip(a["pred_Feat"], a["pred_Head"], cfg, meta["proj_f64"], outer="frame")
    flip = clip["flip"]
    assert len(flip) == meta["flipped_frames"] and np.array_equal(flip, frame["flip"])
    diff = clip["mouth_final"] != frame["mouth_final"]
    outer = [i - 46 for i in M.UPPER_OUTER + M.LOWER_OUTER]
    allowed = np.zeros_like(diff)
    allowed[np.ix_(flip, outer, [1])] = True
    assert diff.any() and not (diff & ~allowed).any()
    for k in ("mouth_smooth", "headpose"):
        assert np.array_equal(clip[k], frame[k])
    same = M.clip(a["pred_Feat"], a["pred_Head"], cfg, meta["proj_f64"], max_lookahead=40)
    assert np.array_equal(same["points"], clip["points"])
    cut = M.clip(a["pred_Feat"], a["pred_Head"], cfg, meta["proj_f64"], max_lookahead=3)
    assert not np.array_equal(cut["headpose"], clip["headpose"])
    for sigma, f in ((1.5, 0), (5, 3), (10, 12)):
        w = M.gaussian_taps(sigma, f)
        r = M.radius(sigma)
        assert abs(w[0] + w[1:].sum() + w[1:f + 1].sum() - 1) < 1e-14 and len(w) == r + 1
    const = np.full((50, 2), 3.25, np.float32)
    assert np.array_equal(M.gaussian_filter_reflect(const, 5, 2), const)


def test_package_taps_are_the_models():
    from livespeechportraits_amd import landmarks as L
    for sigma in (0, 1, 1.5, 2, 5, 8, 10):
        assert L.radius(sigma) == M.radius(sigma) == int(4 * sigma + 0.5)
        for f in (None, 0, 3, 100):
            assert np.array_equal(L.gaussian_taps(sigma, f), M.gaussian_taps(sigma, f))


# ---- the scheduler -------------------------------------------------------------------------------------------------------------------
def _drive(rng, sched, total_m, total_p, max_push):
    """random ragged pushes until both totals are in, then finish: -> [(plan, mouth rows so far, poses so far)]"""
    m = p = 0
    log = []
    while m < total_m or p < total_p:
        nm, np_ = min(int(rng.integers(0, max_push + 1)), total_m - m), min(int(rng.integers(0, max_push + 1)), total_p - p)
        if m < total_m and p < total_p and abs((m + nm) - (p + np_)) > 12:            # the two inputs keep pace, as the audio stages' outputs do
            nm, np_ = (nm, 0) if m < p else (0, np_)
        done = m + nm == total_m and p + np_ == total_p and rng.integers(0, 2) == 0
        log.append((sched.push(nm, np_, finish=bool(done)), m + nm, p + np_))
        m, p = m + nm, p + np_
        if done:
            return log
    log.append((sched.push(0, 0, finish=True), m, p))
    return log


@pytest.mark.parametrize("lookahead", [None, 0, 4, 25])
def test_scheduler_emits_every_frame_once_in_order_and_never_early(lookahead):
    from livespeechportraits_amd.landmarks import LandmarkScheduler
    rng = np.random.default_rng(5)
    r = (6, 20, 40)
    f = r if lookahead is None else tuple(min(x, lookahead) for x in r)
    for _ in range(40):                               # "several sessions": each with its own scheduler, as the stage keeps them
        total_m = int(rng.integers(0, 260))
        total_p = max(0, total_m - int(rng.integers(0, 16)))
        sched = LandmarkScheduler(*r, ring_rows=2 * 40 + 2 + 16 + 32, max_lookahead=lookahead)
        assert sched.delay == max(f)
        nxt = 0
        for plan, m, p in _drive(rng, sched, total_m, total_p, 16):
            assert plan.emit0 == nxt and plan.n_emit >= 0
            assert plan.mouth_have + plan.mouth_fresh == m and plan.pose_have + plan.pose_fresh == p
            last = plan.emit0 + plan.n_emit - 1
            # a frame's window: its future taps, and the rows the reflection at the start of the clip mirrors into its past taps
            complete = lambda k: k + f[0] < min(m, p) and k + max(f[1], f[2]) < p and r[0] - 1 - k < min(m, p) and r[2] - 1 - k < p
            if plan.nframe < 0 and plan.n_emit:
                assert all(complete(k) for k in range(plan.emit0, last + 1))
                assert not complete(last + 1)                                          # and not later than need be
            elif plan.nframe < 0:
                assert not complete(nxt)
            else:
                assert plan.nframe == min(total_m, total_p) and last == plan.nframe - 1 or plan.n_emit == 0 and nxt == plan.nframe
            nxt += plan.n_emit
        assert nxt == min(total_m, total_p) and sched.ended
        with pytest.raises(RuntimeError):
            sched.push(1, 1)


def test_scheduler_lookahead_shortens_the_delay_to_the_stated_frames():
    from livespeechportraits_amd.landmarks import LandmarkScheduler
    for look, delay in ((None, 40), (10, 10), (0, 0)):
        s = LandmarkScheduler(6, 20, 40, ring_rows=200, max_lookahead=look)
        emitted = 0
        for t in range(100):                          # one row of each per tick
            emitted += s.push(1, 1).n_emit
            assert emitted == (0 if t + 1 < 40 else t + 1 - delay)   # the first frame waits for the 40 rows its start reflection reads
    with pytest.raises(ValueError):
        LandmarkScheduler(6, 20, 40, ring_rows=200, max_lookahead=-1)


def test_scheduler_refuses_what_the_ring_cannot_hold_and_stays_as_it_was():
    from livespeechportraits_amd.landmarks import LandmarkScheduler
    s = LandmarkScheduler(6, 20, 40, ring_rows=2 * 40 + 2 + 8)
    with pytest.raises(ValueError):
        LandmarkScheduler(6, 20, 40, ring_rows=81)
    for _ in range(20):
        s.push(4, 4)
    state = (s.m, s.p, s.e)
    with pytest.raises(RuntimeError, match="ring"):
        s.push(60, 60)                                # 80 rows + 60 > 90
    with pytest.raises(RuntimeError, match="ring"):
        s.push(50, 0)                                 # the mouth runs ahead of the poses: nothing can be emitted, the rows pile up
    assert (s.m, s.p, s.e) == state
    s.push(8, 8)


# ---- the C ABI's host half -----------------------------------------------------------------------------------------------------------
def test_native_declares_every_function_of_the_header():
    from livespeechportraits_amd import _native as N
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsplmk.h")).read(), flags=re.S)
    declared = set(re.findall(r"^[A-Za-z_][A-Za-z0-9_ \*]*?\b(lsplmk_[A-Za-z0-9_]+)\s*\(", src, flags=re.M))
    assert len(declared) >= 12 and declared == set(N.LMK_SIGNATURES), declared ^ set(N.LMK_SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "lsplmk.h")).read()
    assert int(re.search(r"#define LSPLMK_ABI_VERSION (\d+)", hdr).group(1)) == N.LMK_ABI_VERSION
    assert int(re.search(r"#define LSPLMK_MAX_SESSIONS (\d+)", hdr).group(1)) == N.LMK_MAX_SESSIONS
    for name, i in N.LMK_AMP_IDS.items():
        macro = {"XY": "XY", "XYZ": "XYZ", "LowerMore": "LOWER_MORE", "delta": "DELTA", "CloseSmall": "CLOSE_SMALL"}[name]
        assert int(re.search(r"#define LSPLMK_AMP_%s (\d+)" % macro, hdr).group(1)) == i
    # the structs have the header's layout: its field names in order
    for struct, cls in (("lsplmk_config", N.LmkConfig), ("lsplmk_session_call", N.LmkSessionCall)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        names = []
        for stmt in body.split(";"):
            stmt = stmt.strip()
            if stmt:
                names += [re.sub(r"\[.*\]", "", n).strip(" *") for n in re.sub(r"^(const\s+)?\w+\s+", "", stmt).split(",")]
        assert names == [f[0] for f in cls._fields_], struct


def _config(N, arrays, **over):
    import landmark_model as M
    sig = over.pop("sigmas", (1.5, 5.0, 10.0))
    fut = over.pop("future", None)
    r = [M.radius(s) for s in sig]
    f = r if fut is None else [min(x, fut) for x in r]
    arrays.update(taps=[np.ascontiguousarray(M.gaussian_taps(s, ff)) for s, ff in zip(sig, f)],
                  mean_mouth=np.arange(54, dtype=np.float64), base=np.zeros((73, 3), np.float32), brow=np.zeros((2, 16, 3), np.float32),
                  idx=np.asarray(M.EYE_BROW_INDICES, np.int32), v3=np.zeros(3, np.float32), m33=np.eye(3, dtype=np.float32), sh=np.zeros((18, 3), np.float64))
    cfg = N.LmkConfig(abi_version=N.LMK_ABI_VERSION, amp_method=N.LMK_AMP_IDS["XYZ"], proj_f64=1, n_candidates=2, max_sessions=4, ring_rows=2 * max(r) + 2 + 16,
                      radius_mouth=r[0], radius_rot=r[1], radius_trans=r[2], future_mouth=f[0], future_rot=f[1], future_trans=f[2],
                      sigma_mouth=sig[0], sigma_rot=sig[1], sigma_trans=sig[2], scale=1.0, rot_amp=1, trans_amp=1, shoulder_amp=0.5)
    a = arrays
    for name, arr in (("taps_mouth", a["taps"][0]), ("taps_rot", a["taps"][1]), ("taps_trans", a["taps"][2]), ("mean_mouth", a["mean_mouth"]),
                      ("base_pts", a["base"]), ("brow", a["brow"]), ("brow_indices", a["idx"]), ("mean_translation", a["v3"]), ("camera_intrinsic", a["m33"]),
                      ("view_rotation", a["m33"]), ("view_translation", a["v3"]), ("shoulder3d", a["sh"]), ("ref_trans", a["v3"])):
        setattr(cfg, name, arr.ctypes.data)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def test_create_refuses_what_the_issue_excludes_and_packs_the_hosts_taps():
    """lsplmk_create / params_bytes / pack_params / state_bytes / clip_workspace_bytes are host calls (no device)"""
    from livespeechportraits_amd import _native as N
    lib = N.load()
    keep = {}
    h = ctypes.c_void_p()
    N.check_lmk(lib.lsplmk_create(ctypes.byref(_config(N, keep)), ctypes.byref(h)))
    n = lib.lsplmk_params_bytes(h)
    blob = np.zeros(n, np.uint8)
    N.check_lmk(lib.lsplmk_pack_params(h, blob.ctypes.data, n))
    for w in keep["taps"]:                            # the host's double taps travel as they are
        assert w.tobytes() in blob.tobytes()
    assert keep["mean_mouth"].tobytes() in blob.tobytes()
    assert lib.lsplmk_state_bytes(h) == 4 * (2 * 40 + 2 + 16) * 60 * 4
    assert lib.lsplmk_clip_workspace_bytes(300) == (1 + 4 * 300) * 8
    assert lib.lsplmk_pack_params(h, blob.ctypes.data, n - 1) == -1
    # a tick before the binds is a state error, and so is a clip
    assert lib.lsplmk_tick(h, 0, None, None) == -4
    lib.lsplmk_destroy(h)
    for over, code, word in ((dict(amp_method=N.LMK_AMP_IDS["CloseSmall"]), -2, b"CloseSmall"), (dict(sigmas=(1.5, 0.0, 10.0)), -2, b"sigma of 0"),
                             (dict(sigmas=(1.5, 5.0, 0.0)), -2, b"sigma of 0"), (dict(radius_rot=19), -1, b"radius"), (dict(future_trans=41), -1, b"future"),
                             (dict(ring_rows=81), -1, b"ring_rows"), (dict(max_sessions=17), -1, b"max_sessions"), (dict(abi_version=7), -1, b"abi"),
                             (dict(sigmas=(1.5, 5.0, 40.0)), -2, b"sigma above"), (dict(shoulder3d=None), -1, b"null")):
        h = ctypes.c_void_p()
        rc = lib.lsplmk_create(ctypes.byref(_config(N, {}, **over)), ctypes.byref(h))
        assert rc == code and word in lib.lsplmk_last_error() and not h.value, (over, rc, lib.lsplmk_last_error())
    h = ctypes.c_void_p()                             # a mouth sigma of 0 is "no filter"
    N.check_lmk(lib.lsplmk_create(ctypes.byref(_config(N, {}, sigmas=(0.0, 2.0, 8.0))), ctypes.byref(h)))
    lib.lsplmk_destroy(h)


def test_tick_refuses_counts_that_break_the_rules_before_anything_is_enqueued():
    """lsplmk_tick checks every count against the finality rules and the ring before it launches.  Those checks are lsplmk_check_tick, which
    touches no device and follows no pointer: nothing here can enqueue a kernel, whatever the checks let through"""
    from livespeechportraits_amd import _native as N
    lib = N.load()
    keep = {}
    h = ctypes.c_void_p()
    N.check_lmk(lib.lsplmk_create(ctypes.byref(_config(N, keep)), ctypes.byref(h)))
    fake = np.zeros(16, np.float64).ctypes.data        # a non-null address, only compared with NULL

    def call(**kw):
        c = (N.LmkSessionCall * 2)()
        base = dict(slot=0, mouth_have=50, mouth_fresh=4, pose_have=50, pose_fresh=4, pose_stride=12, emit0=10, n_emit=4, nframe=-1,
                    mouth_dev=fake, poses_dev=fake, out_dev=fake)
        base.update(kw)
        for k, v in base.items():
            setattr(c[0], k, v)
        c[1].slot = 1
        c[1].pose_stride = 6
        return lib.lsplmk_check_tick(h, 2, c), lib.lsplmk_last_error()

    assert call()[0] == 0                                                                                   # frames 10..13 of 54 rows: complete
    assert call(n_emit=5) == (-1, b"tick: session 0: emits a frame whose window is not complete")        # frame 14 needs pose 54
    assert call(mouth_fresh=0, mouth_have=19)[1].endswith(b"window is not complete")                       # frame 13 needs mouth row 19
    assert call(nframe=54, emit0=50, n_emit=5)[1].endswith(b"past nframe")
    assert call(nframe=53)[1].endswith(b"at finish")
    assert call(nframe=54, emit0=50, n_emit=4)[0] == 0
    assert call(pose_stride=5)[0] == -1 and call(slot=4)[0] == -1 and call(slot=1)[1].endswith(b"named twice")
    assert call(out_dev=None)[1].endswith(b"null pointer")
    assert call(mouth_have=120, pose_have=120, emit0=20, n_emit=0)[0] == -4                                # rows 0.. are long gone from a 98-row ring
    assert call(mouth_fresh=99, pose_fresh=99, n_emit=0)[0] == -4
    assert lib.lsplmk_check_tick(h, 5, None) == -1
    assert lib.lsplmk_tick(h, 2, None, None) == -4                                                          # not bound: a state error before anything else
    lib.lsplmk_destroy(h)
    # with a cut window (max_lookahead 3) frame 0's future taps need 4 rows, but the reflection at the start of the clip mirrors rows
    # 0..39 into its past taps: a call that emits it with fewer rows is refused
    N.check_lmk(lib.lsplmk_create(ctypes.byref(_config(N, keep, future=3)), ctypes.byref(h)))
    for have in (0, 20, 35):
        assert call(mouth_have=have, pose_have=have, emit0=0, n_emit=1)[1].endswith(b"window is not complete"), have      # have + 4 rows < 40
    assert call(mouth_have=36, pose_have=36, emit0=0, n_emit=38)[1].endswith(b"window is not complete")                 # frame 37 needs row 40
    assert call(mouth_have=36, pose_have=36, emit0=0, n_emit=37)[0] == 0
    lib.lsplmk_destroy(h)


def test_pool_planner_preview_counts_what_rounds_hands_out_and_advances_nothing():
    """LivePortraitPool refuses a tick its landmark rings cannot take BEFORE the audio stages run: it needs the row counts of the tick from
    host arithmetic alone (PoolPlanner.preview)"""
    import copy
    from livespeechportraits_amd.live_pool import PoolPlanner
    rng = np.random.default_rng(0)
    plan = PoolPlanner(4, 18, 15, 255, 16000, 16)
    sids = [plan.open() for _ in range(3)]
    seen = 0
    for t in range(200):
        lengths = {s: int(rng.integers(0, 3000)) for s in sids if rng.integers(0, 4)}
        fin = set(sids[:1]) if t == 150 else set()
        before = copy.deepcopy((plan.sched, plan.prime))
        pv = plan.preview(lengths, fin)
        assert all(vars(plan.sched[s]) == vars(before[0][s]) and vars(plan.prime[s]) == vars(before[1][s]) for s in plan.sched)
        got = {s: [0, 0] for s in set(lengths) | fin}
        for work in plan.rounds(lengths, fin):
            for sid, p, _, _, _ in work:
                got[sid][0] += p.mouth[1] - p.mouth[0]
                got[sid][1] += p.poses[1] - p.poses[0]
        assert pv == {s: tuple(v) for s, v in got.items()}
        seen += sum(v[0] + v[1] for v in got.values())
        for s in fin:
            plan.close(s)
            sids.remove(s)
    assert seen > 1000
