#!/usr/bin/env python3
"""Freeze outputs of the reference's OWN post-processing functions into tests/golden/landmarks_*.npz / .json.

Executes the reference's own program text on synthetic inputs: lines 217-255 of its demo.py (which call funcs/utils.py, imported unmodified) and
the image-pad shift of datasets/face_dataset.py:289-294 are read from the checkout that --reference names, at generation time, and run in a
namespace prepared here.  None of that text is kept in this repository.  Modules that funcs/
imports and that may be absent (librosa, sklearn, tqdm) are stubbed; none of the functions used touch them.

The avatar is invented: intrinsics from the pinhole formulas (fx = fy = 1100 px, principal point at the centre of 512 x 512), a face of
about 15 cm at 60 cm, nothing copied from any asset.  Per case the fixture stores the inputs, the avatar's arrays, the taps (smoothed
mouth, final mouth, head pose, final_pts3d) and, in landmarks_<case>_points.npz, the reference's points and a float64 evaluation of the
same formulas (tests/landmark_model.project_f64).  The json records the numpy / scipy versions, the dtype of ``scale * rot.dot(pts.T)``
(float64 under numpy >= 2), the reference's own float32 error against the float64 evaluation, and the share of coordinates within 1e-3 of
an integer (int() of those is not compared; asserted <= 1 %, another seed is taken otherwise)."""
import argparse
import json
import os
import sys
import textwrap
import types
import warnings

import numpy as np
import scipy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import landmark_model as M                         # noqa: E402

EYE_BROW = np.array([27, 65, 28, 68, 29, 67, 30, 66, 31, 72, 32, 69, 33, 70, 34, 71], np.int32)     # demo.py:75
MOUTH_INDICES = np.concatenate([np.arange(4, 11), np.arange(46, 64)])                                # demo.py:74
MAY = dict(mouth_sigma=1.5, head_sigma=[5, 10], amp_method="XYZ", amp=[2, 2, 2], rot_amp=1, trans_amp=0.5, shoulder_amp=0.5)
OBAMA1 = dict(mouth_sigma=1, head_sigma=[2, 8], amp_method="XYZ", amp=[1.5, 1.5, 1.5], rot_amp=1, trans_amp=1, shoulder_amp=0.5)
# name -> (mouth rows, poses, settings, crossed-lip stretch)
CASES = {
    "may": (315, 300, MAY, None),                                                          # config/May.yaml
    "obama1": (318, 303, OBAMA1, None),                                                    # config/Obama1.yaml
    "short": (25, 10, MAY, None),                                                          # 10 frames: shorter than both head-pose radii (20, 40)
    "xy": (90, 80, dict(MAY, mouth_sigma=0, amp_method="XY", amp=[1.8, 1.3]), None),        # and a mouth sigma of 0: no filter
    "lowermore": (80, 84, dict(OBAMA1, amp_method="LowerMore", amp=[1.2, 1.5, 1.1, 1.8, 2.2, 1.4]), None),   # fewer mouth rows than poses
    "delta": (95, 80, dict(MAY, amp_method="delta", amp=[0.7, 1.0]), None),
    "crossed": (135, 120, MAY, (40, 70)),                                                  # frames 40..69: all three inner-lip pairs crossed
}


def make_avatar(rng):
    """An invented avatar with plausible magnitudes (metres): what demo.py:81-108 loads"""
    std = np.zeros([73, 3])
    ang = np.linspace(0, 2 * np.pi, 46, endpoint=False)
    std[:46] = np.stack([0.07 * np.cos(ang), 0.02 + 0.085 * np.sin(ang), 0.03 * np.cos(2 * ang)], 1) * rng.uniform(0.5, 1.0, (46, 1))
    outer = np.linspace(np.pi, -np.pi, 12, endpoint=False)                      # 46 left corner, 47..51 upper, 52 right corner, 53..57 lower
    std[46:58] = np.stack([0.028 * np.cos(outer), -0.045 + 0.011 * np.sin(outer), 0.035 + 0 * outer], 1)
    std[58:61] = [[-0.012, -0.0475, 0.034], [0.0, -0.048, 0.034], [0.012, -0.0475, 0.034]]      # lower inner
    std[61:64] = [[0.012, -0.0425, 0.034], [0.0, -0.042, 0.034], [-0.012, -0.0425, 0.034]]      # upper inner: 63 over 58, 62 over 59, 61 over 60
    std[64:] = np.stack([rng.uniform(-0.05, 0.05, 9), rng.uniform(0.02, 0.05, 9), rng.uniform(0.0, 0.03, 9)], 1)
    pts3d = std + rng.normal(0, 0.002, (60, 73, 3))                             # the "training set"
    mean_pts3d = std + rng.normal(0, 0.0005, (73, 3))
    trans = (np.array([0.0, 0.02, 0.6]) + rng.normal(0, 0.01, (60, 3))).astype(np.float32)
    ys = np.linspace(0.07, 0.12, 9)
    sh = np.concatenate([np.stack([-0.03 - np.linspace(0, 0.09, 9), ys, 0.62 + 0 * ys], 1), np.stack([0.03 + np.linspace(0, 0.09, 9), ys, 0.62 + 0 * ys], 1)])
    return dict(mean_pts3d=mean_pts3d, std_mean_pts3d=pts3d.mean(axis=0), candidate_eye_brow=(pts3d - mean_pts3d)[10:, EYE_BROW],
                mean_translation=trans.mean(axis=0), ref_trans=trans[1],
                camera_intrinsic=np.array([[1100, 0, 256], [0, 1100, 256], [0, 0, 1]], np.float32),
                relative_rotation=np.diag([1, 1, 1]).astype(np.float32), relative_translation=np.zeros(3, np.float32),
                scale=np.float64(1.04), shoulder3D=(sh + rng.normal(0, 0.002, sh.shape)).astype(np.float32), image_pad=[4, 10, 3, 8])


def smooth_noise(rng, n, c, amp, corr=6):
    x = rng.normal(0, 1, (n + 4 * corr, c))
    k = np.exp(-0.5 * (np.arange(-2 * corr, 2 * corr + 1) / corr) ** 2)
    y = np.stack([np.convolve(x[:, i], k / np.sqrt((k ** 2).sum()), "valid") for i in range(c)], 1)[:n]
    return amp * y


def make_inputs(rng, n_mouth, n_pose, crossed):
    feat = (smooth_noise(rng, n_mouth, 75, 0.0015) + rng.normal(0, 0.0004, (n_mouth, 75))).reshape(n_mouth, 25, 3)
    if crossed:
        a, b = crossed
        for pt in (58, 59, 60):                                                 # lower inner up, upper inner down: the pairs cross after the AMP
            feat[a:b, 7 + pt - 46, 1] += 0.004
        for pt in (61, 62, 63):
            feat[a:b, 7 + pt - 46, 1] -= 0.004
        feat[b + 5:b + 15, 7 + 59 - 46, 1] += 0.02                              # one pair alone crossed: not a flip
    head = np.concatenate([smooth_noise(rng, n_pose, 3, 4.0, 15) + rng.normal(0, 0.8, (n_pose, 3)),
                           smooth_noise(rng, n_pose, 3, 0.012, 20) + rng.normal(0, 0.003, (n_pose, 3)), rng.normal(0, 1, (n_pose, 6))], 1)
    return feat.reshape(n_mouth, 75).astype(np.float32), head.astype(np.float32)


def reference_lines(path, first, last, opens, closes):
    """lines first..last (1-based) of a file of the reference, dedented -- read at generation time, never stored.  ``opens`` / ``closes``
    must occur in the first / last line: a reference checkout whose lines have moved is refused."""
    with open(path) as f:
        lines = f.readlines()[first - 1:last]
    if not lines or opens not in lines[0] or closes not in lines[-1]:
        raise SystemExit("%s:%d-%d is not the block this generator runs (expected %r ... %r)" % (path, first, last, opens, closes))
    return textwrap.dedent("".join(lines))


class RecordingUtils:
    """funcs.utils with one tap: the array landmark_smooth_3d returns (points 46..63), which demo.py overwrites on its next line"""

    def __init__(self, utils):
        self._utils, self.mouth_smooth = utils, None

    def __getattr__(self, name):
        return getattr(self._utils, name)

    def landmark_smooth_3d(self, *a, **kw):
        out = self._utils.landmark_smooth_3d(*a, **kw)
        self.mouth_smooth = out[:, 46:64].copy()
        return out


def run_reference(ref_root, utils, feat, head, av, st):
    """Executes the reference's own text: demo.py:217-255 in a namespace that holds what demo.py:73-126 would have loaded, then the pad
    shift of get_feature_image (face_dataset.py:289-294) once per frame, as get_data_test_mode applies it.  Nothing of either is kept here."""
    block = compile(reference_lines(os.path.join(ref_root, "demo.py"), 217, 255, "nframe = min(", "pred_shoulders[k] ="), "demo.py:217-255", "exec")
    shift = compile(reference_lines(os.path.join(ref_root, "datasets", "face_dataset.py"), 289, 294, "image_pad is not None", "delta_y"),
                    "face_dataset.py:289-294", "exec")
    rec = RecordingUtils(utils)
    head_amp = st["rot_amp"], st["trans_amp"]
    ns = dict(np=np, utils=rec, tqdm=lambda it, **kw: it, camera=utils.camera(), pred_Feat=feat, pred_Head=head.copy(),
              mouth_indices=MOUTH_INDICES, eye_brow_indices=EYE_BROW, Feat_smooth_sigma=st["mouth_sigma"], Head_smooth_sigma=st["head_sigma"],
              AMP_method=st["amp_method"], Feat_AMPs=st["amp"], rot_AMP=head_amp[0], trans_AMP=head_amp[1], shoulder_AMP=st["shoulder_amp"],
              **{k: av[k] for k in ("mean_pts3d", "std_mean_pts3d", "candidate_eye_brow", "mean_translation", "camera_intrinsic", "scale",
                                    "shoulder3D", "ref_trans")})
    assert np.array_equal(ns["camera"].relative_rotation, av["relative_rotation"]) and np.array_equal(ns["camera"].relative_translation, av["relative_translation"])
    with warnings.catch_warnings():                                             # no flipped frame: the reference takes the mean of an empty slice (unused)
        warnings.simplefilter("ignore", RuntimeWarning)
        exec(block, ns)
    for frame in ns["pred_shoulders"]:
        exec(shift, dict(shoulders=frame, image_pad=av["image_pad"]))
    wide = (av["scale"] * utils.angle2matrix(ns["pred_headpose"][0][:3]).dot(ns["final_pts3d"][0].T)).dtype
    return dict(mouth_smooth=rec.mouth_smooth, mouth_final=ns["pred_pts3d"][:, 46:64].copy(), headpose=ns["pred_headpose"], final_pts3d=ns["final_pts3d"],
                points=np.concatenate([ns["pred_landmarks"], ns["pred_shoulders"]], 1)), str(wide)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (read only, at generation time)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    for name in ("librosa", "librosa.filters", "sklearn", "sklearn.neighbors", "tqdm"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    for mod, attr, val in (("librosa.filters", "mel", None), ("sklearn.neighbors", "KDTree", None), ("tqdm", "tqdm", lambda it, **kw: it)):
        if not hasattr(sys.modules[mod], attr):
            setattr(sys.modules[mod], attr, val)
    sys.path.insert(0, args.reference)
    from funcs import utils                                                     # the reference module
    os.makedirs(args.out, exist_ok=True)
    for ci, (name, (n_mouth, n_pose, st, crossed)) in enumerate(CASES.items()):
        for attempt in range(20):
            seed = 1000 * (ci + 1) + attempt
            rng = np.random.default_rng(seed)
            av = make_avatar(rng)
            feat, head = make_inputs(rng, n_mouth, n_pose, crossed)
            ref, wide = run_reference(args.reference, utils, feat, head, av, st)
            pts = ref["points"]
            share = float((np.abs(pts - np.round(pts)) < 1e-3).mean())
            if share <= 0.01:
                break
            print("%s: seed %d has %.2f %% of its coordinates within 1e-3 of an integer: another seed" % (name, seed, 100 * share))
        else:
            raise SystemExit("%s: no seed met the 1 %% condition" % name)
        assert pts.min() >= 0 and pts.max() < 512, (name, pts.min(), pts.max())
        cfg = dict(av, **st)
        p64 = M.project_f64(ref["headpose"], ref["final_pts3d"], cfg)
        ref_err = float(np.abs(pts.astype(np.float64) - p64).max())
        pre = M.mouth_path(feat, pts.shape[0], cfg)[2]                          # which frames flip (for the record)
        if crossed:
            assert set(range(crossed[0] + 3, crossed[1] - 3)) <= set(pre.tolist()), "the crossed stretch does not flip"
        np.savez_compressed(os.path.join(args.out, "landmarks_%s.npz" % name), pred_Feat=feat, pred_Head=head,
                            **{k: np.asarray(v) for k, v in av.items()}, mouth_smooth=ref["mouth_smooth"], mouth_final=ref["mouth_final"],
                            headpose=ref["headpose"], final_pts3d=ref["final_pts3d"])
        np.savez_compressed(os.path.join(args.out, "landmarks_%s_points.npz" % name), points=pts, points_f64=p64)
        meta = dict(settings=st, seed=seed, n_mouth=n_mouth, n_pose=n_pose, nframe=int(pts.shape[0]), numpy=np.__version__, scipy=scipy.__version__,
                    scale_times_dot_dtype=wide, proj_f64=wide == "float64", reference_f32_error_px=ref_err, near_integer_share=share,
                    flipped_frames=int(len(pre)), crossed=list(crossed) if crossed else None,
                    note="reference_f32_error_px = max |reference points - float64 evaluation of the same formulas| over the fixture")
        with open(os.path.join(args.out, "landmarks_%s.json" % name), "w") as f:
            json.dump(meta, f, indent=1, sort_keys=True)
            f.write("\n")
        print("%-10s nframe %3d  seed %d  %s  reference fp32 error %.2e px  near-integer %.2f %%  flipped %d  points %.0f..%.0f"
              % (name, pts.shape[0], seed, wide, ref_err, 100 * share, len(pre), pts.min(), pts.max()))


if __name__ == "__main__":
    main()
