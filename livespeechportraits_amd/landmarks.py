"""demo.py's "5. Post-Processing" (demo.py:215-255) on the device: mouth rows and head poses in, the ``[91, 2]`` point array of the
rasteriser out (include/lsplmk.h, csrc/landmarks.hip; DESIGN.md "Landmark stage").

``LandmarkStage.clip`` is the whole-clip form and computes what the reference's functions compute (funcs/utils.py: landmark_smooth_3d,
mouth_pts_AMP, solve_intersect_mouth, headpose_smooth, project_landmarks, plus the shoulder block and the image-pad shift).
``open`` / ``tick`` / ``finish`` / ``close`` are the streamed form for up to 16 sessions: one launch per tick whatever the number of
sessions, no device-to-host read -- every count comes from ``LandmarkScheduler``, which needs no device.

A streamed frame is bit for bit the whole-clip frame, with two stated departures:

* the outer-lip correction.  ``solve_intersect_mouth`` (utils.py:352-354) moves the outer lips of every flipped frame by the mean of the
  half-differences over ALL flipped frames of the clip, which a stream cannot know.  ``tick`` uses the mean of the frame's own three
  half-differences; ``clip`` keeps the reference's rule.  Only the y of points 47..51 and 53..57 of flipped frames differs.
* ``max_lookahead=L`` (default None: exact).  The exact filter delays a frame by the largest radius (sigma 10 -> 40 frames, 667 ms at
  60 fps).  With L set, the future side of each window is cut to L taps and the taps are renormalised; the result is then NOT the
  reference's (tests pin it on the numpy restatement of tests/landmark_model.py only).  The past side keeps scipy's reflection at the
  start of the clip, which reads rows 0 .. r - 1: the first frame still waits for r rows, the delay is L frames from then on.

There is no CPU path."""
from __future__ import annotations

import ctypes
from typing import Dict, NamedTuple, Optional, Sequence

import numpy as np

AMP_METHODS = ("XY", "XYZ", "LowerMore", "delta")
EYE_BROW_INDICES = (27, 65, 28, 68, 29, 67, 30, 66, 31, 72, 32, 69, 33, 70, 34, 71)     # demo.py:75
N_POINTS = 91
MAX_SESSIONS = 16


def radius(sigma: float) -> int:
    """scipy's gaussian_filter1d: int(truncate * sigma + 0.5) with truncate = 4"""
    return int(4.0 * float(sigma) + 0.5)


def gaussian_taps(sigma: float, future: Optional[int] = None) -> np.ndarray:
    """The taps of scipy's _gaussian_kernel1d(sigma, 0, radius) in double, centre first: w[0..r].  ``future`` < r: the window keeps only
    that many future taps and is renormalised (max_lookahead; not the reference's filter)."""
    r = radius(sigma)
    if r == 0:
        return np.ones(1, np.float64)
    sigma2 = float(sigma) * float(sigma)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / sigma2 * x ** 2)
    phi = phi / phi.sum()
    w = np.ascontiguousarray(phi[r:])
    if future is not None and future < r:
        w = w / (phi[: r + 1 + future].sum())
    return w


class LandmarkPlan(NamedTuple):
    """What one push of one session does (the fields of lsplmk_session_call)."""
    mouth_have: int
    mouth_fresh: int
    pose_have: int
    pose_fresh: int
    emit0: int
    n_emit: int
    nframe: int           # -1 while the session runs


class LandmarkScheduler:
    """When a frame becomes final, without a device.  Frame k is final when its windows are complete:

        k + f_mouth < min(mouth rows, poses)   and   k + max(f_rot, f_trans) < poses

    (f = the filter radius, or max_lookahead when that is smaller; the mouth filter reflects at nframe = min(mouth rows, poses) as
    demo.py:217 slices before it smooths, so its window has to lie below both counts), or when the session has finished: then every frame
    below nframe is final and the end reflection applies.  The reflection at the START of a clip mirrors rows 0 .. r - 1 - k into frame
    k's past taps, so those rows must be present as well: with max_lookahead the first frame waits for r rows (then r - f frames come at
    once) and the delay is f frames from there on.  ``ring_rows`` bounds what one push may bring: the rows the next frame still
    reads (radius + 1 back) plus the push must fit."""

    def __init__(self, r_mouth: int, r_rot: int, r_trans: int, ring_rows: int, max_lookahead: Optional[int] = None):
        if max_lookahead is not None and max_lookahead < 0:
            raise ValueError("max_lookahead must be >= 0 frames (or None for the exact filter)")
        cut = (lambda r: r) if max_lookahead is None else (lambda r: min(r, int(max_lookahead)))
        self.r = (int(r_mouth), int(r_rot), int(r_trans))
        self.f = tuple(cut(r) for r in self.r)
        self.ring_rows = int(ring_rows)
        if self.ring_rows < 2 * max(self.r) + 2:
            raise ValueError("ring_rows must be at least 2 * radius + 2")
        self.m = self.p = self.e = 0
        self.ended = False

    @property
    def delay(self) -> int:
        """frames between the newest row and the newest final frame while both inputs keep pace (after the first r rows)"""
        return max(self.f)

    def push(self, n_mouth: int, n_poses: int, finish: bool = False) -> LandmarkPlan:
        if self.ended:
            raise RuntimeError("the session has finished")
        if n_mouth < 0 or n_poses < 0:
            raise ValueError("negative row count")
        m, p = self.m + n_mouth, self.p + n_poses
        if finish:
            nframe = end = min(m, p)
        else:
            nframe = -1
            # the start reflection mirrors rows 0 .. r - 1 - k into frame k's past taps: they must be there too (implied by the first rule
            # for the exact filter; with max_lookahead it is what delays the first frames)
            started = self.r[0] - 1 - self.e < min(m, p) and max(self.r[1], self.r[2]) - 1 - self.e < p
            end = max(min(min(m, p) - self.f[0], p - max(self.f[1], self.f[2])), self.e) if started else self.e
        low_m, low_p = max(0, self.e - self.r[0] - 1), max(0, self.e - max(self.r[1], self.r[2]))
        if (self.m > low_m and m - low_m > self.ring_rows) or (self.p > low_p and p - low_p > self.ring_rows) or max(n_mouth, n_poses) > self.ring_rows:
            raise RuntimeError("a push of %d mouth rows / %d poses does not fit the ring of %d rows (%d mouth rows and %d poses are still "
                               "needed): raise max_push or max_skew" % (n_mouth, n_poses, self.ring_rows, self.m - low_m, self.p - low_p))
        plan = LandmarkPlan(self.m, n_mouth, self.p, n_poses, self.e, end - self.e, nframe)
        self.m, self.p, self.e, self.ended = m, p, end, bool(finish)
        return plan


class LandmarkStage:
    """One avatar's landmark stage on one device.

    Arguments are what demo.py:81-126 loads (``from_demo_assets`` takes them under demo.py's names).  ``proj_f64``: whether
    project_landmarks runs in double after ``rot.dot(pts)`` -- None follows THIS numpy's promotion of ``scale * float32 array`` (float64
    for a numpy.float64 ``scale`` under numpy >= 2, float32 under numpy 1.x or for a Python float).  The rings hold
    ``2 * radius + 2 + max_push + max_skew`` rows per session: ``max_push`` = the most rows of one kind in one tick, ``max_skew`` = how far
    one input may run ahead of the other (in the live audio path the two counts differ by the models' frame_future values: poses lead by
    3 rows while a session runs, the mouth tail of 18 rows comes at finish)."""

    def __init__(self, mean_pts3d, std_mean_pts3d, candidate_eye_brow, mean_translation, camera_intrinsic, scale, shoulder3D, ref_trans,
                 shoulder_AMP: float, AMP_method: str, Feat_AMPs: Sequence[float], rot_AMP: float, trans_AMP: float, Feat_smooth_sigma: float,
                 Head_smooth_sigma: Sequence[float], relative_rotation=None, relative_translation=None, image_pad=None,
                 eye_brow_indices=EYE_BROW_INDICES, device="cuda:0", max_sessions: int = MAX_SESSIONS, max_push: int = 64, max_skew: int = 32,
                 max_lookahead: Optional[int] = None, proj_f64: Optional[bool] = None):
        import torch
        from . import _native as N
        self.torch, self.N = torch, N
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("the landmark stage runs on the MI355X only (no CPU path); the reference's host path is demo.py:215-255")
        if AMP_method == "CloseSmall":
            raise NotImplementedError("the CloseSmall AMP method is not supported: its close branch rescales every frame of the clip once per "
                                      "closed frame (funcs/utils.py:310-323) and no shipped config uses it")
        if AMP_method not in AMP_METHODS:
            raise ValueError("AMP_method must be one of %s" % (AMP_METHODS,))
        need = {"XY": 2, "XYZ": 3, "LowerMore": 6, "delta": 2}[AMP_method]
        amps = [float(a) for a in Feat_AMPs]
        if len(amps) != need:
            raise ValueError("AMP method %s takes %d parameters" % (AMP_method, need))
        rot_sigma, trans_sigma = (float(s) for s in Head_smooth_sigma)
        if rot_sigma == 0 or trans_sigma == 0:
            raise ValueError("a head-pose sigma of 0 is refused (scipy's gaussian_filter1d divides by it; no shipped config has one)")
        self.device = dev
        self.lib = N.load()
        self.sigmas = (float(Feat_smooth_sigma), rot_sigma, trans_sigma)
        self.radii = tuple(radius(s) for s in self.sigmas)
        self.max_lookahead = None if max_lookahead is None else int(max_lookahead)
        self.future = tuple(r if self.max_lookahead is None else min(r, self.max_lookahead) for r in self.radii)
        self.taps = tuple(gaussian_taps(s, f) for s, f in zip(self.sigmas, self.future))
        self.max_sessions, self.max_push = int(max_sessions), int(max_push)
        self.ring_rows = 2 * max(self.radii) + 2 + self.max_push + int(max_skew)
        if proj_f64 is None:
            proj_f64 = (scale * np.ones(1, np.float32)).dtype == np.float64
        self.proj_f64 = bool(proj_f64)

        mean = np.asarray(mean_pts3d)
        idx = np.asarray(eye_brow_indices, np.int32).reshape(16)
        cand = np.asarray(candidate_eye_brow)
        if mean.shape != (73, 3) or cand.ndim != 3 or cand.shape[1:] != (16, 3) or cand.shape[0] < 1:
            raise ValueError("mean_pts3d must be [73, 3] and candidate_eye_brow [Nc, 16, 3] with Nc >= 1")
        f32 = lambda a, shape: np.ascontiguousarray(np.asarray(a).astype(np.float32).reshape(shape))
        arrays = dict(
            taps_mouth=self.taps[0], taps_rot=self.taps[1], taps_trans=self.taps[2],
            mean_mouth=np.ascontiguousarray(mean[46:64].astype(np.float64)),
            base_pts=f32(std_mean_pts3d, (73, 3)),
            brow=np.ascontiguousarray((cand + mean[idx]).astype(np.float32)),              # demo.py:241, cast as the assignment into final_pts3d casts
            brow_indices=np.ascontiguousarray(idx),
            mean_translation=f32(mean_translation, 3), camera_intrinsic=f32(camera_intrinsic, (3, 3)),
            view_rotation=f32(np.eye(3) if relative_rotation is None else relative_rotation, (3, 3)),
            view_translation=f32(np.zeros(3) if relative_translation is None else relative_translation, 3),
            shoulder3d=np.ascontiguousarray(np.asarray(shoulder3D).astype(np.float64).reshape(18, 3)),        # the sum with it is formed in the asset's own type
            ref_trans=f32(ref_trans, 3))
        top, bottom, left, right = image_pad if image_pad is not None else (0, 0, 0, 0)
        cfg = N.LmkConfig(abi_version=N.LMK_ABI_VERSION, amp_method=N.LMK_AMP_IDS[AMP_method], proj_f64=int(self.proj_f64), n_candidates=cand.shape[0],
                          max_sessions=self.max_sessions, ring_rows=self.ring_rows, radius_mouth=self.radii[0], radius_rot=self.radii[1],
                          radius_trans=self.radii[2], future_mouth=self.future[0], future_rot=self.future[1], future_trans=self.future[2],
                          sigma_mouth=self.sigmas[0], sigma_rot=self.sigmas[1], sigma_trans=self.sigmas[2], scale=float(scale),
                          rot_amp=float(rot_AMP), trans_amp=float(trans_AMP), shoulder_amp=float(shoulder_AMP), pad_dx=float(right - left),
                          pad_dy=float(top - bottom))
        for i, a in enumerate(amps):
            cfg.amp[i] = a
        for name, a in arrays.items():
            setattr(cfg, name, a.ctypes.data)
        self.h = ctypes.c_void_p()
        N.check_lmk(self.lib.lsplmk_create(ctypes.byref(cfg), ctypes.byref(self.h)))
        nbytes = int(self.lib.lsplmk_params_bytes(self.h))
        host = np.zeros(nbytes, np.uint8)
        N.check_lmk(self.lib.lsplmk_pack_params(self.h, host.ctypes.data, nbytes))
        with torch.cuda.device(dev):
            self._params = torch.from_numpy(host).to(dev)                                   # uploaded once
            self._state = torch.zeros(int(self.lib.lsplmk_state_bytes(self.h)) // 4, dtype=torch.float32, device=dev)
        N.check_lmk(self.lib.lsplmk_bind_params(self.h, ctypes.c_void_p(self._params.data_ptr()), nbytes))
        N.check_lmk(self.lib.lsplmk_bind_state(self.h, ctypes.c_void_p(self._state.data_ptr()), self._state.numel() * 4))
        self._free = list(range(self.max_sessions))
        self._slot: Dict[int, int] = {}
        self.sched: Dict[int, LandmarkScheduler] = {}
        self._next = 0
        self.last_points = None

    @classmethod
    def from_demo_assets(cls, config, mean_pts3d, std_mean_pts3d, candidate_eye_brow, mean_translation, camera_intrinsic, camera, scale, shoulder3D,
                         ref_trans, image_pad=None, **kw):
        """The arrays of demo.py:81-108 under their names there, ``camera`` = utils.camera() (its relative_rotation / relative_translation),
        ``config`` = the loaded yaml (demo.py:119-126 reads the AMP and smoothing entries from it)."""
        mp = config["model_params"]
        return cls(mean_pts3d, std_mean_pts3d, candidate_eye_brow, mean_translation, camera_intrinsic, scale, shoulder3D, ref_trans,
                   shoulder_AMP=mp["Headpose"]["shoulder_AMP"], AMP_method=mp["Audio2Mouth"]["AMP"][0], Feat_AMPs=mp["Audio2Mouth"]["AMP"][1:],
                   rot_AMP=mp["Headpose"]["AMP"][0], trans_AMP=mp["Headpose"]["AMP"][1], Feat_smooth_sigma=mp["Audio2Mouth"]["smooth"],
                   Head_smooth_sigma=mp["Headpose"]["smooth"], relative_rotation=camera.relative_rotation,
                   relative_translation=camera.relative_translation, image_pad=image_pad, **kw)

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            self.lib.lsplmk_destroy(h)

    # ---- whole clip --------------------------------------------------------------------------------------------------------------
    def _rows(self, t, width, what):
        torch = self.torch
        if not isinstance(t, torch.Tensor):
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(t, np.float32)))
        t = t.to(self.device)
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < width or (width == 75 and t.shape[1] != 75):
            raise ValueError("%s must be float32 [N, %s%d] (got %s %s)" % (what, "" if width == 75 else ">= ", width, t.dtype, tuple(t.shape)))
        if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) != t.shape[1]):
            t = t.contiguous()
        return t

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def clip(self, mouth, poses):
        """mouth rows [N_m, 75] (pred_Feat) and head poses [N_h, >= 6] (pred_Head) -> float32 [min(N_m, N_h), 91, 2] on the device:
        pred_landmarks then pred_shoulders (pad shift applied) of demo.py:235-255.  The inputs are not modified."""
        torch = self.torch
        m, p = self._rows(mouth, 75, "mouth"), self._rows(poses, 6, "poses")
        n = min(m.shape[0], p.shape[0])
        with torch.cuda.device(self.device):
            out = torch.empty(n, N_POINTS, 2, dtype=torch.float32, device=self.device)
            nws = int(self.lib.lsplmk_clip_workspace_bytes(n))
            ws = torch.empty(nws // 8, dtype=torch.float64, device=self.device)
            ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
            self.N.check_lmk(self.lib.lsplmk_clip(self.h, ptr(m), m.shape[0], ptr(p), p.shape[0], p.shape[1], ptr(out), ptr(ws), nws, self._stream()))
        return out

    # ---- streamed ----------------------------------------------------------------------------------------------------------------
    def open(self) -> int:
        """A new session in a free ring slot -> its id (never reused; the slot is)."""
        if not self._free:
            raise RuntimeError("all %d sessions of the stage are open: close one first" % self.max_sessions)
        sid, self._next = self._next, self._next + 1
        self._slot[sid] = self._free.pop(0)
        self.sched[sid] = LandmarkScheduler(*self.radii, ring_rows=self.ring_rows, max_lookahead=self.max_lookahead)
        return sid

    def close(self, sid: int) -> None:
        self._check(sid)
        self._free.append(self._slot.pop(sid))
        self._free.sort()
        del self.sched[sid]

    def _check(self, sid) -> None:
        if sid not in self._slot:
            raise KeyError("unknown or closed landmark session %r" % (sid,))

    def tick(self, frames, finish=()):
        """``frames``: {session id: LiveFrames} (or any (mouth, mouth_start, poses, pose_start); device tensors, taken as they are) of the rows
        that became final in this tick; ``finish``: sessions that end after them (closed afterwards).  -> {id: (frame_start, points
        [k, 91, 2])} for every session named: the frames that became final.  One launch; nothing is read back."""
        torch = self.torch
        frames = dict(frames.items() if hasattr(frames, "items") else frames or ())
        finish = list(finish)
        named = sorted(set(frames) | set(finish))
        for sid in named:
            self._check(sid)
        rows = {}
        for sid in named:
            sch = self.sched[sid]
            if sid in frames:
                mouth, m0, poses, p0 = frames[sid]
                m = self._rows(mouth, 75, "mouth") if mouth is not None and len(mouth) else None
                p = self._rows(poses, 6, "poses") if poses is not None and len(poses) else None
                if (m is not None and m0 != sch.m) or (p is not None and p0 != sch.p):
                    raise ValueError("session %d: rows start at mouth %d / pose %d, the stage expects %d / %d" % (sid, m0, p0, sch.m, sch.p))
            else:
                m = p = None
            rows[sid] = (m, p)
        # plan every session before any state changes: a refused push leaves the stage as it was
        saved = {sid: (self.sched[sid].m, self.sched[sid].p, self.sched[sid].e, self.sched[sid].ended) for sid in named}
        plans = {}

        def restore():
            for sid, (a, b, c, d) in saved.items():
                s = self.sched[sid]
                s.m, s.p, s.e, s.ended = a, b, c, d
        try:
            for sid in named:
                m, p = rows[sid]
                plans[sid] = self.sched[sid].push(0 if m is None else m.shape[0], 0 if p is None else p.shape[0], sid in finish)
        except Exception:
            restore()
            raise
        total = sum(pl.n_emit for pl in plans.values())
        calls = (self.N.LmkSessionCall * max(len(named), 1))()
        result = {}
        with torch.cuda.device(self.device):
            out = torch.empty(total, N_POINTS, 2, dtype=torch.float32, device=self.device)
            at = 0
            for i, sid in enumerate(named):
                pl, (m, p) = plans[sid], rows[sid]
                o = out[at: at + pl.n_emit]
                at += pl.n_emit
                c = calls[i]
                c.slot, c.mouth_have, c.mouth_fresh, c.pose_have, c.pose_fresh = self._slot[sid], pl.mouth_have, pl.mouth_fresh, pl.pose_have, pl.pose_fresh
                c.pose_stride = p.shape[1] if p is not None else 6
                c.emit0, c.n_emit, c.nframe = pl.emit0, pl.n_emit, pl.nframe
                c.mouth_dev = m.data_ptr() if m is not None else None
                c.poses_dev = p.data_ptr() if p is not None else None
                c.out_dev = o.data_ptr() if pl.n_emit else None
                result[sid] = (pl.emit0, o)
            if named:
                rc = self.lib.lsplmk_tick(self.h, len(named), calls, self._stream())
                if rc != 0:                                                                # refused: nothing was enqueued, the stage stays as it was
                    restore()
                    self.N.check_lmk(rc)
            self.last_points = out                                                         # all frames of the tick, in ascending session id
        for sid in finish:
            self.close(sid)
        return result

    def finish(self, sid: int):
        """End a session without new rows -> (frame_start, points) of the frames still pending."""
        return self.tick({}, finish=[sid])[sid]
