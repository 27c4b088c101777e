/* lsplmk.h -- C ABI of the landmark stage: demo.py's "5. Post-Processing" between the audio models and the rasteriser, on the device.
 * Exported by livespeechportraits_amd/liblspf2f.so; gfx950 only, no CPU path.
 *
 * Replaces, per frame (reference file:line):
 *   demo.py:217-225        mouth rows -> pred_pts3d: landmark_smooth_3d, mouth_pts_AMP, + mean_pts3d, solve_intersect_mouth
 *   demo.py:228-232        head pose: * rot_AMP / trans_AMP, headpose_smooth, + mean_translation, + 180
 *   demo.py:235-244        final_pts3d (std mean, mouth 46..63, eyebrow candidate k % Nc) and project_landmarks
 *   demo.py:247-255        the shoulder points
 *   face_dataset.py:289-294 the image-pad shift of the shoulders
 *   funcs/utils.py:182-242 angle2matrix / project_landmarks,  :246-367 the smoothing, AMP and crossed-lip functions
 * Output per frame: float32 [91][2] -- 73 landmarks then 18 shoulder points, the array lspraster_edge_maps takes.
 *
 * Arithmetic (what the reference's functions compute under numpy / scipy): the mouth path is double until the cast into final_pts3d; the
 * Gaussian filter is scipy's symmetric correlate1d (centre tap first, then (x[k-j] + x[k+j]) * w[j] for j = r..1, double accumulation,
 * `reflect` boundaries); the head pose is float32 with that double accumulation; angle2matrix takes float32 radians, double cos / sin and
 * double 3x3 products, cast to float32; rot . pts is float32; the rest of project_landmarks is double when `proj_f64` (numpy >= 2: a float64
 * scalar times a float32 array is float64) and float32 otherwise; the shoulders are float32 (their 3-D sum in the type of the shoulder3D asset).  No FMA contraction anywhere.
 * Only mouth points 46..63 (columns 21..74 of a 75-wide mouth row) survive into final_pts3d, so only those are filtered.
 *
 * A frame is computed by ONE workgroup from its window of rows, wherever the rows lie: in a session's ring (rows of earlier calls) or in
 * the call's own input.  lsplmk_clip and lsplmk_tick run the same device code, so a streamed frame equals the whole-clip frame bit for bit
 * -- except the outer-lip correction of solve_intersect_mouth (utils.py:352-354), which uses a mean over every flipped frame of the clip:
 * lsplmk_clip keeps that rule, lsplmk_tick uses the mean of the frame's own three half-differences.  With a `future` radius below the
 * filter radius (max_lookahead) the future side of a window is cut and the taps are renormalised by the host: not the reference's result.
 *
 * Conventions: device pointers, nothing allocated by the library, no synchronisation, returns 0 or a negative code (lsplmk_last_error()).
 * create / params_bytes / pack_params / state_bytes / clip_workspace_bytes touch no device.
 */
#ifndef LSPLMK_H
#define LSPLMK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden: exactly the functions declared below are exported */
#pragma GCC visibility push(default)

#define LSPLMK_OK 0
#define LSPLMK_ERR_INVALID_ARGUMENT (-1)
#define LSPLMK_ERR_UNSUPPORTED (-2)
#define LSPLMK_ERR_HIP (-3)
#define LSPLMK_ERR_STATE (-4)

#define LSPLMK_ABI_VERSION 1
#define LSPLMK_MAX_SESSIONS 16
#define LSPLMK_MAX_RADIUS 128      /* sigma <= 32 */
#define LSPLMK_POINTS 91           /* 73 landmarks + 18 shoulder points */
#define LSPLMK_MOUTH_ROW 75        /* floats per mouth row (25 points: 4..10, 46..63) */

#define LSPLMK_AMP_XY 0
#define LSPLMK_AMP_XYZ 1
#define LSPLMK_AMP_LOWER_MORE 2
#define LSPLMK_AMP_DELTA 3
#define LSPLMK_AMP_CLOSE_SMALL 4   /* refused: its "close" branch rescales every frame of the clip once per closed frame */

typedef struct lsplmk_handle lsplmk_handle;

/* All pointers are HOST arrays, read by lsplmk_create only.  The taps are the host's (double, scipy's _gaussian_kernel1d), centre first:
 * taps_x[0..radius_x]; radius_x must equal int(4 sigma_x + 0.5) (0 and taps {1.0} for a mouth sigma of 0; a head-pose sigma of 0 is
 * refused).  future_x <= radius_x is the number of future taps kept (== radius_x: the exact filter). */
typedef struct lsplmk_config {
    int32_t abi_version;
    int32_t amp_method;                 /* LSPLMK_AMP_* */
    int32_t proj_f64;                   /* 1: project_landmarks in double after rot . pts (numpy >= 2), 0: float32 (numpy 1.x) */
    int32_t n_candidates;               /* Nc >= 1 rows of the eyebrow table */
    int32_t max_sessions;               /* 1..LSPLMK_MAX_SESSIONS ring slots */
    int32_t ring_rows;                  /* rows per ring */
    int32_t radius_mouth, radius_rot, radius_trans;
    int32_t future_mouth, future_rot, future_trans;
    double sigma_mouth, sigma_rot, sigma_trans;
    double amp[6];                      /* XY: x y; XYZ: x y z; LowerMore: upper x y z, lower x y z; delta: x (y unused) */
    double scale;
    float rot_amp, trans_amp, shoulder_amp;
    float pad_dx, pad_dy;               /* right - left, top - bottom of image_pad; 0 without a pad */
    const double *taps_mouth, *taps_rot, *taps_trans;
    const double *mean_mouth;           /* [18][3] mean_pts3d[46:64] */
    const float *base_pts;              /* [73][3] std_mean_pts3d as float32 */
    const float *brow;                  /* [Nc][16][3] candidate_eye_brow + mean_pts3d[eye_brow_indices], as float32 */
    const int32_t *brow_indices;        /* [16] distinct indices in 0..72 outside 46..63 */
    const float *mean_translation;      /* [3] */
    const float *camera_intrinsic;      /* [3][3] */
    const float *view_rotation;         /* [3][3] camera.relative_rotation */
    const float *view_translation;      /* [3] */
    const double *shoulder3d;           /* [18][3] in double, exact for a float32 or a float64 asset (the reference adds in the asset's type) */
    const float *ref_trans;             /* [3] */
} lsplmk_config;

/* one session of a tick.  Rows / poses [0, have) are in the slot's ring, the `fresh` ones are this call's; the call stores them.
 * Frames [emit0, emit0 + n_emit) are written to out_dev.  While the session runs (nframe < 0) a frame k may be emitted when
 *   k + future_mouth < min(mouth rows, poses)   and   k + max(future_rot, future_trans) < poses
 * (the mouth filter reflects at nframe = min(mouth rows, poses), demo.py:217, so its window must lie below both counts) and the rows that
 * the reflection at the start of the clip mirrors into its past taps are present (radius - 1 - k < the same counts; implied by the first
 * rule when future == radius); at finish
 * nframe = min(total mouth rows, total poses) and every frame below it may be emitted, with the end reflection. */
typedef struct lsplmk_session_call {
    int32_t slot;
    int32_t mouth_have, mouth_fresh;
    int32_t pose_have, pose_fresh, pose_stride;   /* floats per pose row, >= 6 */
    int32_t emit0, n_emit;
    int32_t nframe;                     /* -1 while the session runs */
    int32_t reserved;
    const float *mouth_dev;             /* [mouth_fresh][75] */
    const float *poses_dev;             /* [pose_fresh][pose_stride] */
    float *out_dev;                     /* [n_emit][91][2] */
} lsplmk_session_call;

int lsplmk_create(const lsplmk_config *cfg, lsplmk_handle **out);
int lsplmk_destroy(lsplmk_handle *h);
const char *lsplmk_last_error(void);
int lsplmk_abi_version(void);

/* the avatar's constants and taps as one blob: packed on the host, uploaded once by the caller, bound as a device pointer */
size_t lsplmk_params_bytes(const lsplmk_handle *h);
int lsplmk_pack_params(const lsplmk_handle *h, void *host_buf, size_t bytes);
int lsplmk_bind_params(lsplmk_handle *h, const void *params_dev, size_t bytes);
/* the rings of all max_sessions slots; their content on entry is irrelevant (a session starts with have == 0) */
size_t lsplmk_state_bytes(const lsplmk_handle *h);
int lsplmk_bind_state(lsplmk_handle *h, void *state_dev, size_t bytes);

/* whole clip: mouth_dev [n_mouth][75], poses_dev [n_poses][pose_stride] -> out_dev [min(n_mouth, n_poses)][91][2]; the reference's
 * outer-lip rule (clip mean).  Three launches.  workspace: lsplmk_clip_workspace_bytes(nframe) bytes. */
size_t lsplmk_clip_workspace_bytes(int nframe);
int lsplmk_clip(const lsplmk_handle *h, const float *mouth_dev, int n_mouth, const float *poses_dev, int n_poses, int pose_stride,
                float *out_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream);

/* one tick of up to max_sessions sessions (distinct slots): ONE launch -- a workgroup per (session, emitted frame), one per session that
 * stores its fresh rows.  The counts are checked against the rules above and the ring size; nothing is enqueued when one is refused. */
int lsplmk_tick(const lsplmk_handle *h, int nsessions, const lsplmk_session_call *calls, void *hip_stream);
/* those checks alone: touches no device, follows no pointer, needs no bind */
int lsplmk_check_tick(const lsplmk_handle *h, int nsessions, const lsplmk_session_call *calls);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
