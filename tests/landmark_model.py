"""A numpy restatement of demo.py's "5. Post-Processing" (demo.py:217-255 with funcs/utils.py:182-242, :246-367 and the image-pad shift
of face_dataset.py:289-294) -- the CPU model of the landmark stage (include/lsplmk.h), as tests/jpeg_model.py is of the JPEG encoder.

It is written operation by operation in the precisions the reference's functions produce, so that it reproduces the fixtures of
tools/make_golden_landmarks.py bit for bit wherever the reference does not go through a BLAS ``dot``, and it adds what the reference has
no form of: the streamed outer-lip rule (``outer="frame"``) and the truncated window (``max_lookahead``).  Needs numpy only."""
import math

import numpy as np

UPPER_OUTER = list(range(47, 52))
UPPER_INNER = [63, 62, 61]
LOWER_INNER = [58, 59, 60]
LOWER_OUTER = list(range(57, 52, -1))
LOWER_MOUTH = [53, 54, 55, 56, 57, 58, 59, 60]
UPPER_MOUTH = [46, 47, 48, 49, 50, 51, 52, 61, 62, 63]
EYE_BROW_INDICES = np.array([27, 65, 28, 68, 29, 67, 30, 66, 31, 72, 32, 69, 33, 70, 34, 71], np.int32)


def radius(sigma):
    return int(4.0 * float(sigma) + 0.5)


def gaussian_taps(sigma, future=None):
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius), centre first; ``future`` < radius: cut and renormalised"""
    r = radius(sigma)
    if r == 0:
        return np.ones(1)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    phi = phi / phi.sum()
    w = phi[r:].copy()
    if future is not None and future < r:
        w = w / phi[: r + 1 + future].sum()
    return w


def reflect(i, n):
    """scipy's `reflect` boundary (d c b a | a b c d | d c b a), any distance"""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def gaussian_filter_reflect(x, sigma, future=None):
    """gaussian_filter1d(x, sigma, axis=0) as scipy's NI_Correlate1D computes it for a symmetric kernel: double line buffers, the centre tap
    first, then (x[k - j] + x[k + j]) * w[j] for j = r .. 1; the result is cast to x's dtype.  ``future``: taps with j > future lose their
    future half."""
    n = x.shape[0]
    r = radius(sigma)
    f = r if future is None else min(r, future)
    w = gaussian_taps(sigma, f)
    xd = x.astype(np.float64)
    k = np.arange(n)
    tmp = xd * w[0]
    for j in range(r, 0, -1):
        past = xd[reflect(k - j, n)]
        tmp = tmp + ((past + xd[reflect(k + j, n)]) * w[j] if j <= f else past * w[j])
    return tmp.astype(x.dtype)


def mouth_path(mouth_rows, nframe, cfg, outer="clip", max_lookahead=None):
    """demo.py:218-225 for points 46..63 (the only ones that reach final_pts3d): -> (smoothed, final), both double [nframe, 18, 3]"""
    m = np.asarray(mouth_rows)[:nframe, 21:75].astype(np.float64).reshape(nframe, 18, 3)
    sigma = cfg["mouth_sigma"]
    sm = m if sigma == 0 else gaussian_filter_reflect(m.reshape(nframe, 54), sigma, max_lookahead).reshape(nframe, 18, 3)
    method, paras = cfg["amp_method"], cfg["amp"]
    p = sm.copy()
    if method == "XY":
        p[:, :, 0] *= paras[0]
        p[:, :, 1] *= paras[1]
    elif method == "XYZ":
        for d in range(3):
            p[:, :, d] *= paras[d]
    elif method == "LowerMore":
        up, lo = [i - 46 for i in UPPER_MOUTH], [i - 46 for i in LOWER_MOUTH]
        for d in range(3):
            p[:, up, d] *= paras[d]
            p[:, lo, d] *= paras[3 + d]
    elif method == "delta":
        diff = paras[0] * (p[1:] - p[:-1])
        p[1:] += diff
    else:
        raise ValueError(method)
    p = p + np.asarray(cfg["mean_pts3d"])[46:64]
    ui, li = [i - 46 for i in UPPER_INNER], [i - 46 for i in LOWER_INNER]
    uo, lo_ = [i - 46 for i in UPPER_OUTER], [i - 46 for i in LOWER_OUTER]
    lower_y, upper_y = p[:, li, 1], p[:, ui, 1]
    flip = np.where((lower_y > upper_y).sum(axis=1) == 3)[0]
    half = (lower_y[flip] - upper_y[flip]) * 0.5
    p[flip[:, None], ui, 1] += half
    p[flip[:, None], li, 1] -= half
    if len(flip):
        if outer == "clip":
            mean = half.mean()
        else:                                                   # the streamed rule: the frame's own three half-differences
            mean = (((half[:, 0] + half[:, 1]) + half[:, 2]) / 3.0)[:, None]
        p[flip[:, None], uo, 1] += mean
        p[flip[:, None], lo_, 1] -= mean
    return sm, p, flip


def head_path(poses, cfg, max_lookahead=None):
    """demo.py:228-232 on the whole pose sequence: float32 [N_h, 6]"""
    h = np.array(np.asarray(poses)[:, :6], np.float32)
    h[:, 0:3] *= np.float32(cfg["rot_amp"])
    h[:, 3:6] *= np.float32(cfg["trans_amp"])
    rot = gaussian_filter_reflect(h[:, :3], cfg["head_sigma"][0], max_lookahead)
    trans = gaussian_filter_reflect(h[:, 3:], cfg["head_sigma"][1], max_lookahead)
    out = np.concatenate([rot, trans], axis=1).astype(np.float32)
    out[:, 3:] += np.asarray(cfg["mean_translation"], np.float32)
    out[:, 0] += np.float32(180)
    return out


def final_points3d(mouth_final, cfg):
    """demo.py:236-241: float32 [n, 73, 3]"""
    n = mouth_final.shape[0]
    mean, cand = np.asarray(cfg["mean_pts3d"]), np.asarray(cfg["candidate_eye_brow"])
    idx = np.asarray(cfg.get("eye_brow_indices", EYE_BROW_INDICES))
    fin = np.zeros([n, 73, 3], np.float32)
    fin[:] = np.asarray(cfg["std_mean_pts3d"])
    fin[:, 46:64] = mouth_final
    for k in range(n):
        fin[k, idx] = cand[k % cand.shape[0]] + mean[idx]
    return fin


def _dot3_f32(a, b):
    """[3, 3] float32 . [3, n] float32, the three products of a row summed left to right in float32"""
    a, b = a.astype(np.float32), b.astype(np.float32)
    return np.stack([(a[d, 0] * b[0] + a[d, 1] * b[1]) + a[d, 2] * b[2] for d in range(3)])


def _dot3_f64(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.stack([(a[d, 0] * b[0] + a[d, 1] * b[1]) + a[d, 2] * b[2] for d in range(3)])


def angle2matrix(angles):
    """utils.py:182-211: np.deg2rad of float32 angles stays float32; math.cos / sin in double; double products; float32"""
    x, y, z = (float(np.deg2rad(np.float32(a))) for a in angles[:3])
    Rx = np.array([[1, 0, 0], [0, math.cos(x), -math.sin(x)], [0, math.sin(x), math.cos(x)]])
    Ry = np.array([[math.cos(y), 0, math.sin(y)], [0, 1, 0], [-math.sin(y), 0, math.cos(y)]])
    Rz = np.array([[math.cos(z), -math.sin(z), 0], [math.sin(z), math.cos(z), 0], [0, 0, 1]])
    return _dot3_f64(Rz, _dot3_f64(Ry, Rx)).astype(np.float32)


def project(headpose, fin, cfg, proj_f64):
    """demo.py:242-255 + the pad shift: float32 [n, 91, 2].  ``proj_f64``: numpy >= 2 makes ``scale * rot.dot(pts.T)`` float64 for a
    numpy.float64 scale, and everything after it double; numpy 1.x keeps float32."""
    n = fin.shape[0]
    K = np.asarray(cfg["camera_intrinsic"], np.float32)
    vR, vT = np.asarray(cfg["relative_rotation"], np.float32), np.asarray(cfg["relative_translation"], np.float32)
    out = np.zeros([n, 91, 2], np.float32)
    wide = np.float64 if proj_f64 else np.float32
    scale = wide(cfg["scale"])
    dot = _dot3_f64 if proj_f64 else _dot3_f32
    ref_trans, sh3 = np.asarray(cfg["ref_trans"], np.float32), np.asarray(cfg["shoulder3D"])     # float32 or float64, as loaded
    top, bottom, left, right = cfg.get("image_pad") or (0, 0, 0, 0)
    for k in range(n):
        rot = angle2matrix(headpose[k])
        h = scale * _dot3_f32(rot, fin[k].T).astype(wide) + headpose[k, 3:][:, None].astype(wide)
        v = dot(vR, h) + vT[:, None].astype(wide)
        q = dot(K, v)
        out[k, :73, 0] = q[0] / q[2]
        out[k, :73, 1] = q[1] / q[2]
        s = (sh3 + (headpose[k, 3:] - ref_trans) * np.float32(cfg["shoulder_amp"])).astype(np.float32)   # a float64 asset: summed in double, rounded once
        qs = _dot3_f32(K, s.T)
        out[k, 73:, 0] = qs[0] / qs[2] + np.float32(right - left)
        out[k, 73:, 1] = qs[1] / qs[2] + np.float32(top - bottom)
    return out


def project_f64(headpose, fin, cfg):
    """The same formulas evaluated in float64 throughout from the float32 head poses and final_pts3d (no float32 rounding anywhere): the
    yardstick that the reference's own float32 error, and the device's, are measured against.  float64 [n, 91, 2]"""
    n = fin.shape[0]
    K = np.asarray(cfg["camera_intrinsic"], np.float64)
    vR, vT = np.asarray(cfg["relative_rotation"], np.float64), np.asarray(cfg["relative_translation"], np.float64)
    ref_trans, sh3 = np.asarray(cfg["ref_trans"], np.float64), np.asarray(cfg["shoulder3D"], np.float64)
    top, bottom, left, right = cfg.get("image_pad") or (0, 0, 0, 0)
    out = np.zeros([n, 91, 2])
    for k in range(n):
        x, y, z = (math.radians(float(a)) for a in headpose[k, :3])
        Rx = np.array([[1, 0, 0], [0, math.cos(x), -math.sin(x)], [0, math.sin(x), math.cos(x)]])
        Ry = np.array([[math.cos(y), 0, math.sin(y)], [0, 1, 0], [-math.sin(y), 0, math.cos(y)]])
        Rz = np.array([[math.cos(z), -math.sin(z), 0], [math.sin(z), math.cos(z), 0], [0, 0, 1]])
        t = headpose[k, 3:].astype(np.float64)
        h = float(cfg["scale"]) * (Rz @ (Ry @ Rx)) @ fin[k].T.astype(np.float64) + t[:, None]
        q = K @ (vR @ h + vT[:, None])
        out[k, :73] = (q[:2] / q[2]).T
        s = sh3 + (t - ref_trans) * float(cfg["shoulder_amp"])
        qs = K @ s.T
        out[k, 73:] = (qs[:2] / qs[2]).T + np.array([right - left, top - bottom], np.float64)
    return out


def clip(mouth_rows, poses, cfg, proj_f64, outer="clip", max_lookahead=None):
    """The whole block -> dict of every tap: mouth_smooth, mouth_final (double [n, 18, 3]), flip (indices), headpose (float32 [N_h, 6]),
    final_pts3d (float32 [n, 73, 3]), points (float32 [n, 91, 2]).  outer="frame" and max_lookahead give what the streamed stage emits
    (its frames do not depend on how the rows were pushed)."""
    nframe = min(np.asarray(mouth_rows).shape[0], np.asarray(poses).shape[0])
    sm, fin_m, flip = mouth_path(mouth_rows, nframe, cfg, outer, max_lookahead)
    hp = head_path(poses, cfg, max_lookahead)
    fin = final_points3d(fin_m, cfg)
    return dict(mouth_smooth=sm, mouth_final=fin_m, flip=flip, headpose=hp, final_pts3d=fin, points=project(hp, fin, cfg, proj_f64))
