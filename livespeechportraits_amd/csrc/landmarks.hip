// landmarks.hip -- the landmark stage (include/lsplmk.h): demo.py:217-255 per frame, one workgroup per (session, emitted frame).
//
// Latency-bound work: a frame is 54 + 6 filtered columns of at most 2 * 128 + 1 taps and 91 projected points, a few thousand fp64
// operations -- far below what one CU does in a microsecond.  So the geometry follows the dependencies, not the arithmetic: 128 lanes (two
// waves) per frame, wave 0 filters the mouth columns while wave 1 filters the six pose columns, two barriers, then one lane per point.
// All frames of all sessions of a tick are independent workgroups of ONE launch; the launch overhead is the cost.
// Built with -ffp-contract=off: every product and sum rounds where numpy's does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lsplmk.h"

namespace lsplmk {

constexpr int NT = 128;
constexpr int MC = 54;                 // mouth columns that survive: points 46..63
constexpr int MOUTH_OFF = 21;          // their offset in a 75-wide mouth row (7 points 4..10 come first)
constexpr int NLM = 73, NSH = 18;
constexpr int ROWF = MC + 6;           // floats per ring row: mouth columns then the pose

struct Params {
    int32_t n_cand, amp_method, proj_f64, ring_rows;
    int32_t r[3], rf[3];               // mouth, rot, trans: radius and future radius
    int32_t brow_slot[NLM];            // -1, or the eyebrow slot 0..15 of the landmark
    int32_t pad_;
    double scale, delta_amp;
    double amp[MC], mean_mouth[MC];
    double taps[3][LSPLMK_MAX_RADIUS + 1];
    double sh3[NSH * 3];               // shoulder3D as loaded (float32 or float64 asset)
    float base[NLM * 3];
    float mean_trans[3], K[9], vR[9], vT[3], ref_trans[3];
    float rot_amp, trans_amp, sh_amp, pad_dx, pad_dy;
    float pad2_;
};                                     // float brow[n_cand][16][3] follows
static_assert(sizeof(Params) % 8 == 0, "the eyebrow table follows the struct");

struct Sess {
    const float *mouth, *poses;
    float *out;
    float *ring;                       // the slot's ring_rows x ROWF floats
    int32_t m_have, m_fresh, p_have, p_fresh, p_stride, emit0, blk_end, nframe, p_total;
};

struct TickArgs {
    Sess s[LSPLMK_MAX_SESSIONS];
    int32_t n, emit_blocks, mode, pad_;       // mode 0: own-frame outer-lip mean; 1: pre-pass (flip + half-differences -> ws); 2: clip mean from ws[0]
    double *ws;
};

__device__ __forceinline__ int reflect(long long i, long long n)
{
    if (i >= 0 && i < n) return (int)i;
    const long long p = 2 * n;
    long long m = i % p;
    if (m < 0) m += p;
    return (int)(m < n ? m : p - 1 - m);
}

// row `idx` of a session's mouth (pose == 0) or pose (pose == 1) sequence, column c
__device__ __forceinline__ float row_at(const Sess &s, int cap, int idx, int c, int pose)
{
    if (pose) return idx >= s.p_have ? s.poses[(size_t)(idx - s.p_have) * s.p_stride + c] : s.ring[(size_t)(idx % cap) * ROWF + MC + c];
    return idx >= s.m_have ? s.mouth[(size_t)(idx - s.m_have) * LSPLMK_MOUTH_ROW + MOUTH_OFF + c] : s.ring[(size_t)(idx % cap) * ROWF + c];
}

// scipy's symmetric correlate1d at frame k; `a` scales the float32 input first (the head pose's AMP; 1 for the mouth)
__device__ double filt(const Sess &s, int cap, int k, int c, int pose, long long n, int r, int rf, const double *w, float a)
{
    double tmp = (double)(row_at(s, cap, k, c, pose) * a) * w[0];
    for (int j = r; j >= 1; --j) {
        const double past = (double)(row_at(s, cap, reflect((long long)k - j, n), c, pose) * a);
        if (j <= rf)
            tmp += (past + (double)(row_at(s, cap, reflect((long long)k + j, n), c, pose) * a)) * w[j];
        else
            tmp += past * w[j];
    }
    return tmp;
}

__device__ __forceinline__ double rnd(double v, int f64) { return f64 ? v : (double)(float)v; }
__device__ __forceinline__ float fdiv(float a, float b) { return (float)((double)a / (double)b); }   // correctly rounded float32 quotient

__device__ void mat3(const double *a, const double *b, double *o)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[i * 3 + j] = (a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j]) + a[i * 3 + 2] * b[6 + j];
}

__global__ __launch_bounds__(NT) void lmk_frames(const Params *__restrict__ P, const TickArgs A)
{
    __shared__ double pm[MC];
    __shared__ float hp[6];
    __shared__ float R[9];
    const int t = threadIdx.x, b = blockIdx.x, cap = P->ring_rows;
    if (b >= A.emit_blocks) {                                  // store a session's fresh rows in its ring
        const Sess &s = A.s[b - A.emit_blocks];
        for (int i = t; i < s.m_fresh * MC; i += NT) {
            const int row = i / MC, c = i - row * MC;
            s.ring[(size_t)((s.m_have + row) % cap) * ROWF + c] = s.mouth[(size_t)row * LSPLMK_MOUTH_ROW + MOUTH_OFF + c];
        }
        for (int i = t; i < s.p_fresh * 6; i += NT) {
            const int row = i / 6, c = i - row * 6;
            s.ring[(size_t)((s.p_have + row) % cap) * ROWF + MC + c] = s.poses[(size_t)row * s.p_stride + c];
        }
        return;
    }
    int si = 0;
    while (si < A.n - 1 && b >= A.s[si].blk_end) ++si;
    const Sess &s = A.s[si];
    const int f = b - (si ? A.s[si - 1].blk_end : 0);         // frame of this call
    const int k = s.emit0 + f;
    const long long big = 1LL << 40;
    const long long nm = s.nframe >= 0 ? s.nframe : big, np_ = s.p_total >= 0 ? s.p_total : big;

    if (t < MC) {                                              // demo.py:222-224
        const double sm = filt(s, cap, k, t, 0, nm, P->r[0], P->rf[0], P->taps[0], 1.0f);
        double v;
        if (P->amp_method == LSPLMK_AMP_DELTA) {
            v = sm;
            if (k >= 1) v = sm + P->delta_amp * (sm - filt(s, cap, k - 1, t, 0, nm, P->r[0], P->rf[0], P->taps[0], 1.0f));
        } else {
            v = sm * P->amp[t];
        }
        pm[t] = v + P->mean_mouth[t];
    } else if (t >= 64 && t < 70 && A.mode != 1) {             // demo.py:228-232
        const int c = t - 64, g = c < 3 ? 1 : 2;
        float v = (float)filt(s, cap, k, c, 1, np_, P->r[g], P->rf[g], P->taps[g], c < 3 ? P->rot_amp : P->trans_amp);
        if (c >= 3) v += P->mean_trans[c - 3];
        if (c == 0) v += 180.0f;
        hp[c] = v;
    }
    __syncthreads();
    if (t == 0) {                                              // solve_intersect_mouth: lower inner 58 59 60 against upper inner 63 62 61
        const int li[3] = {(58 - 46) * 3 + 1, (59 - 46) * 3 + 1, (60 - 46) * 3 + 1};
        const int ui[3] = {(63 - 46) * 3 + 1, (62 - 46) * 3 + 1, (61 - 46) * 3 + 1};
        const bool flip = pm[li[0]] > pm[ui[0]] && pm[li[1]] > pm[ui[1]] && pm[li[2]] > pm[ui[2]];
        double hd[3];
        for (int i = 0; i < 3; ++i) hd[i] = (pm[li[i]] - pm[ui[i]]) * 0.5;
        if (A.mode == 1) {
            double *w = A.ws + 1 + (size_t)k * 4;
            w[0] = flip ? 1.0 : 0.0;
            w[1] = hd[0]; w[2] = hd[1]; w[3] = hd[2];
        } else if (flip) {
            const double m = A.mode == 2 ? A.ws[0] : ((hd[0] + hd[1]) + hd[2]) / 3.0;
            for (int i = 0; i < 3; ++i) { pm[ui[i]] += hd[i]; pm[li[i]] -= hd[i]; }
            for (int p = 47; p <= 51; ++p) pm[(p - 46) * 3 + 1] += m;
            for (int p = 53; p <= 57; ++p) pm[(p - 46) * 3 + 1] -= m;
        }
    } else if (t == 64 && A.mode != 1) {                       // angle2matrix: float32 radians, double cos / sin, Rz . (Ry . Rx), float32
        const float d2r = 3.141592653589793238462643383279502884f / 180.0f;
        const double x = (double)(hp[0] * d2r), y = (double)(hp[1] * d2r), z = (double)(hp[2] * d2r);
        const double cx = cos(x), sx = sin(x), cy = cos(y), sy = sin(y), cz = cos(z), sz = sin(z);
        const double Rx[9] = {1, 0, 0, 0, cx, -sx, 0, sx, cx}, Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy}, Rz[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1};
        double T[9], Rd[9];
        mat3(Ry, Rx, T);
        mat3(Rz, T, Rd);
        for (int i = 0; i < 9; ++i) R[i] = (float)Rd[i];
    }
    __syncthreads();
    if (A.mode == 1 || t >= NLM + NSH) return;
    float *o = s.out + ((size_t)f * LSPLMK_POINTS + t) * 2;
    if (t < NLM) {                                             // demo.py:236-244, project_landmarks
        float q[3];
        const int bs = P->brow_slot[t];
        const float *brow = reinterpret_cast<const float *>(P + 1);
        for (int d = 0; d < 3; ++d)
            q[d] = t >= 46 && t < 64 ? (float)pm[(t - 46) * 3 + d] : bs >= 0 ? brow[((size_t)(k % P->n_cand) * 16 + bs) * 3 + d] : P->base[t * 3 + d];
        const int f64 = P->proj_f64;
        const double sc = f64 ? P->scale : (double)(float)P->scale;
        double H[3], V[3], Q[3];
        for (int d = 0; d < 3; ++d) {
            const float rp = (R[d * 3] * q[0] + R[d * 3 + 1] * q[1]) + R[d * 3 + 2] * q[2];
            H[d] = rnd(rnd(sc * (double)rp, f64) + (double)hp[3 + d], f64);
        }
        for (int d = 0; d < 3; ++d)
            V[d] = rnd(rnd(rnd(rnd((double)P->vR[d * 3] * H[0], f64) + rnd((double)P->vR[d * 3 + 1] * H[1], f64), f64) + rnd((double)P->vR[d * 3 + 2] * H[2], f64), f64)
                       + (double)P->vT[d], f64);
        for (int d = 0; d < 3; ++d)
            Q[d] = rnd(rnd(rnd((double)P->K[d * 3] * V[0], f64) + rnd((double)P->K[d * 3 + 1] * V[1], f64), f64) + rnd((double)P->K[d * 3 + 2] * V[2], f64), f64);
        o[0] = (float)(Q[0] / Q[2]);
        o[1] = (float)(Q[1] / Q[2]);
    } else {                                                   // demo.py:247-255 and face_dataset.py:289-294, float32
        const int i = t - NLM;
        float sh[3], q[3];
        // shoulder3D + diff_trans * shoulder_AMP: the product is float32; the sum is float32 for a float32 asset and double, rounded once on
        // assignment, for a float64 one -- one double sum rounded to float32 is both
        for (int d = 0; d < 3; ++d) sh[d] = (float)(P->sh3[i * 3 + d] + (double)((hp[3 + d] - P->ref_trans[d]) * P->sh_amp));
        for (int d = 0; d < 3; ++d) q[d] = (P->K[d * 3] * sh[0] + P->K[d * 3 + 1] * sh[1]) + P->K[d * 3 + 2] * sh[2];
        o[0] = fdiv(q[0], q[2]) + P->pad_dx;
        o[1] = fdiv(q[1], q[2]) + P->pad_dy;
    }
}

// ws[0] = mean of the half-differences of every flipped frame (half_inner_y_diff.mean(), utils.py:352), in a fixed order
__global__ __launch_bounds__(256) void lmk_clip_mean(double *ws, int n)
{
    __shared__ double sum[256];
    __shared__ double cnt[256];
    const int t = threadIdx.x;
    double a = 0.0, c = 0.0;
    for (int k = t; k < n; k += 256) {
        const double *w = ws + 1 + (size_t)k * 4;
        if (w[0] != 0.0) { a += (w[1] + w[2]) + w[3]; c += 3.0; }
    }
    sum[t] = a; cnt[t] = c;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) { sum[t] += sum[t + h]; cnt[t] += cnt[t + h]; }
        __syncthreads();
    }
    if (t == 0) ws[0] = cnt[0] > 0.0 ? sum[0] / cnt[0] : 0.0;
}

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }

}  // namespace lsplmk

using namespace lsplmk;

struct lsplmk_handle {
    std::vector<unsigned char> blob;   // Params + the eyebrow table
    int max_sessions = 0, ring_rows = 0;
    int r[3] = {0, 0, 0}, rf[3] = {0, 0, 0};
    const Params *params_dev = nullptr;
    float *state_dev = nullptr;
};

static int launch(const lsplmk_handle *h, const TickArgs &a, int blocks, void *stream, const char *what)
{
    if (blocks <= 0) return LSPLMK_OK;
    hipLaunchKernelGGL(lmk_frames, dim3(blocks), dim3(NT), 0, static_cast<hipStream_t>(stream), h->params_dev, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LSPLMK_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    return LSPLMK_OK;
}

extern "C" {

const char *lsplmk_last_error(void) { return g_err.c_str(); }
int lsplmk_abi_version(void) { return LSPLMK_ABI_VERSION; }

int lsplmk_create(const lsplmk_config *c, lsplmk_handle **out)
{
    if (!out) return fail(LSPLMK_ERR_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    if (!c || c->abi_version != LSPLMK_ABI_VERSION) return fail(LSPLMK_ERR_INVALID_ARGUMENT, "null config or abi_version mismatch");
    if (c->amp_method == LSPLMK_AMP_CLOSE_SMALL)
        return fail(LSPLMK_ERR_UNSUPPORTED, "the CloseSmall AMP method is not supported: its close branch rescales every frame of the clip once per closed frame "
                                            "(funcs/utils.py:310-323), which has no streamed form, and no shipped config uses it");
    if (c->amp_method < 0 || c->amp_method > LSPLMK_AMP_DELTA) return fail(LSPLMK_ERR_INVALID_ARGUMENT, "unknown amp_method");
    if (c->sigma_rot <= 0 || c->sigma_trans <= 0)
        return fail(LSPLMK_ERR_UNSUPPORTED, "a head-pose sigma of 0 is refused (scipy's gaussian_filter1d divides by it; no shipped config has one)");
    if (c->sigma_mouth < 0) return fail(LSPLMK_ERR_INVALID_ARGUMENT, "negative mouth sigma");
    const double sig[3] = {c->sigma_mouth, c->sigma_rot, c->sigma_trans};
    const int r[3] = {c->radius_mouth, c->radius_rot, c->radius_trans}, rf[3] = {c->future_mouth, c->future_rot, c->future_trans};
    const double *taps[3] = {c->taps_mouth, c->taps_rot, c->taps_trans};
    for (int i = 0; i < 3; ++i) {
        if (r[i] != (int)(4.0 * sig[i] + 0.5)) return fail(LSPLMK_ERR_INVALID_ARGUMENT, "a radius is not int(4 sigma + 0.5)");
        if (r[i] > LSPLMK_MAX_RADIUS) return fail(LSPLMK_ERR_UNSUPPORTED, "sigma above 32 (radius above LSPLMK_MAX_RADIUS)");
        if (rf[i] < 0 || rf[i] > r[i]) return fail(LSPLMK_ERR_INVALID_ARGUMENT, "a future radius must be in 0..radius");
        if (!taps[i]) return fail(LSPLMK_ERR_INVALID_ARGUMENT, "null taps");
    }
    if (c->n_candidates < 1) return fail(LSPLMK_ERR_INVALID_ARGUMENT, "n_candidates must be >= 1");
    if (c->max_sessions < 1 || c->max_sessions > LSPLMK_MAX_SESSIONS) return fail(LSPLMK_ERR_INVALID_ARGUMENT, "max_sessions must be in 1..16");
    const int rmax = std::max(r[0], std::max(r[1], r[2]));
    if (c->ring_rows < 2 * rmax + 2) return fail(LSPLMK_ERR_INVALID_ARGUMENT, "ring_rows must be at least 2 * radius + 2 (plus the largest push)");
    if (!c->mean_mouth || !c->base_pts || !c->brow || !c->brow_indices || !c->mean_translation || !c->camera_intrinsic || !c->view_rotation ||
        !c->view_translation || !c->shoulder3d || !c->ref_trans)
        return fail(LSPLMK_ERR_INVALID_ARGUMENT, "null array in the config");

    lsplmk_handle *h = new lsplmk_handle;
    h->blob.assign(sizeof(Params) + (size_t)c->n_candidates * 48 * sizeof(float), 0);
    Params *p = reinterpret_cast<Params *>(h->blob.data());
    p->n_cand = c->n_candidates; p->amp_method = c->amp_method; p->proj_f64 = c->proj_f64 ? 1 : 0; p->ring_rows = c->ring_rows;
    for (int i = 0; i < 3; ++i) {
        p->r[i] = h->r[i] = r[i]; p->rf[i] = h->rf[i] = rf[i];
        std::memcpy(p->taps[i], taps[i], (size_t)(r[i] + 1) * sizeof(double));
    }
    for (int i = 0; i < NLM; ++i) p->brow_slot[i] = -1;
    for (int i = 0; i < 16; ++i) {
        const int idx = c->brow_indices[i];
        if (idx < 0 || idx >= NLM || (idx >= 46 && idx < 64) || p->brow_slot[idx] >= 0) {
            delete h;
            return fail(LSPLMK_ERR_INVALID_ARGUMENT, "brow_indices must be 16 distinct landmarks outside the mouth (46..63)");
        }
        p->brow_slot[idx] = i;
    }
    p->scale = c->scale;
    p->delta_amp = c->amp[0];
    for (int pt = 46; pt < 64; ++pt) {
        const bool lower = pt >= 53 && pt <= 60;                // lower_mouth of utils.py:272; the rest of 46..63 is upper_mouth
        for (int d = 0; d < 3; ++d) {
            double a = 1.0;
            if (c->amp_method == LSPLMK_AMP_XY) a = d < 2 ? c->amp[d] : 1.0;
            else if (c->amp_method == LSPLMK_AMP_XYZ) a = c->amp[d];
            else if (c->amp_method == LSPLMK_AMP_LOWER_MORE) a = c->amp[(lower ? 3 : 0) + d];
            p->amp[(pt - 46) * 3 + d] = a;
        }
    }
    std::memcpy(p->mean_mouth, c->mean_mouth, sizeof p->mean_mouth);
    std::memcpy(p->base, c->base_pts, sizeof p->base);
    std::memcpy(p->mean_trans, c->mean_translation, sizeof p->mean_trans);
    std::memcpy(p->K, c->camera_intrinsic, sizeof p->K);
    std::memcpy(p->vR, c->view_rotation, sizeof p->vR);
    std::memcpy(p->vT, c->view_translation, sizeof p->vT);
    std::memcpy(p->sh3, c->shoulder3d, sizeof p->sh3);
    std::memcpy(p->ref_trans, c->ref_trans, sizeof p->ref_trans);
    p->rot_amp = c->rot_amp; p->trans_amp = c->trans_amp; p->sh_amp = c->shoulder_amp; p->pad_dx = c->pad_dx; p->pad_dy = c->pad_dy;
    std::memcpy(p + 1, c->brow, (size_t)c->n_candidates * 48 * sizeof(float));
    h->max_sessions = c->max_sessions;
    h->ring_rows = c->ring_rows;
    *out = h;
    return LSPLMK_OK;
}

int lsplmk_destroy(lsplmk_handle *h)
{
    delete h;
    return LSPLMK_OK;
}

size_t lsplmk_params_bytes(const lsplmk_handle *h) { return h ? h->blob.size() : 0; }

int lsplmk_pack_params(const lsplmk_handle *h, void *host_buf, size_t bytes)
{
    if (!h || !host_buf || bytes < h->blob.size()) return fail(LSPLMK_ERR_INVALID_ARGUMENT, "pack_params: null argument or buffer too small");
    std::memcpy(host_buf, h->blob.data(), h->blob.size());
    return LSPLMK_OK;
}

int lsplmk_bind_params(lsplmk_handle *h, const void *params_dev, size_t bytes)
{
    if (!h || !params_dev || bytes < h->blob.size() || (reinterpret_cast<uintptr_t>(params_dev) & 7))
        return fail(LSPLMK_ERR_INVALID_ARGUMENT, "bind_params: null or misaligned pointer, or fewer than lsplmk_params_bytes() bytes");
    h->params_dev = static_cast<const Params *>(params_dev);
    return LSPLMK_OK;
}

size_t lsplmk_state_bytes(const lsplmk_handle *h) { return h ? (size_t)h->max_sessions * h->ring_rows * ROWF * sizeof(float) : 0; }

int lsplmk_bind_state(lsplmk_handle *h, void *state_dev, size_t bytes)
{
    if (!h || !state_dev || bytes < lsplmk_state_bytes(h) || (reinterpret_cast<uintptr_t>(state_dev) & 3))
        return fail(LSPLMK_ERR_INVALID_ARGUMENT, "bind_state: null or misaligned pointer, or fewer than lsplmk_state_bytes() bytes");
    h->state_dev = static_cast<float *>(state_dev);
    return LSPLMK_OK;
}

size_t lsplmk_clip_workspace_bytes(int nframe) { return nframe < 0 ? 0 : (1 + (size_t)nframe * 4) * sizeof(double); }

int lsplmk_clip(const lsplmk_handle *h, const float *mouth_dev, int n_mouth, const float *poses_dev, int n_poses, int pose_stride,
                float *out_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream)
{
    if (!h || !h->params_dev) return fail(LSPLMK_ERR_STATE, "clip: no handle, or lsplmk_bind_params has not been called");
    if (n_mouth < 0 || n_poses < 0 || pose_stride < 6) return fail(LSPLMK_ERR_INVALID_ARGUMENT, "clip: negative count or pose_stride < 6");
    const int n = std::min(n_mouth, n_poses);
    if (n == 0) return LSPLMK_OK;
    if (!mouth_dev || !poses_dev || !out_dev || !workspace_dev) return fail(LSPLMK_ERR_INVALID_ARGUMENT, "clip: null pointer");
    if (workspace_bytes < lsplmk_clip_workspace_bytes(n) || (reinterpret_cast<uintptr_t>(workspace_dev) & 7))
        return fail(LSPLMK_ERR_INVALID_ARGUMENT, "clip: workspace smaller than lsplmk_clip_workspace_bytes(nframe), or misaligned");
    TickArgs a;
    std::memset(&a, 0, sizeof a);
    Sess &s = a.s[0];
    s.mouth = mouth_dev; s.poses = poses_dev; s.out = out_dev; s.ring = nullptr;
    s.m_have = 0; s.m_fresh = n_mouth; s.p_have = 0; s.p_fresh = n_poses; s.p_stride = pose_stride; s.emit0 = 0; s.blk_end = n;
    s.nframe = n; s.p_total = n_poses;
    a.n = 1; a.emit_blocks = n; a.ws = static_cast<double *>(workspace_dev);
    a.mode = 1;
    int rc = launch(h, a, n, hip_stream, "clip pre-pass");
    if (rc) return rc;
    hipLaunchKernelGGL(lmk_clip_mean, dim3(1), dim3(256), 0, static_cast<hipStream_t>(hip_stream), a.ws, n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LSPLMK_ERR_HIP, std::string("clip mean launch: ") + hipGetErrorString(e));
    a.mode = 2;
    return launch(h, a, n, hip_stream, "clip");
}

// every count of a tick against the finality rules and the ring: what lsplmk_tick checks before it enqueues anything.  Follows no pointer.
int lsplmk_check_tick(const lsplmk_handle *h, int nsessions, const lsplmk_session_call *calls)
{
    if (!h) return fail(LSPLMK_ERR_INVALID_ARGUMENT, "tick: null handle");
    if (nsessions < 0 || nsessions > h->max_sessions || (nsessions && !calls)) return fail(LSPLMK_ERR_INVALID_ARGUMENT, "tick: nsessions outside 0..max_sessions");
    const int cap = h->ring_rows;
    const int fpose = std::max(h->rf[1], h->rf[2]), rpose = std::max(h->r[1], h->r[2]);
    unsigned used = 0;
    for (int i = 0; i < nsessions; ++i) {
        const lsplmk_session_call &c = calls[i];
        const std::string who = "tick: session " + std::to_string(i) + ": ";
        if (c.slot < 0 || c.slot >= h->max_sessions || (used >> c.slot & 1)) return fail(LSPLMK_ERR_INVALID_ARGUMENT, who + "slot out of range or named twice");
        used |= 1u << c.slot;
        if (c.mouth_have < 0 || c.mouth_fresh < 0 || c.pose_have < 0 || c.pose_fresh < 0 || c.emit0 < 0 || c.n_emit < 0 || c.pose_stride < 6)
            return fail(LSPLMK_ERR_INVALID_ARGUMENT, who + "negative count or pose_stride < 6");
        if ((c.mouth_fresh && !c.mouth_dev) || (c.pose_fresh && !c.poses_dev) || (c.n_emit && !c.out_dev)) return fail(LSPLMK_ERR_INVALID_ARGUMENT, who + "null pointer");
        const long long m = (long long)c.mouth_have + c.mouth_fresh, p = (long long)c.pose_have + c.pose_fresh;
        if (m > (1 << 30) || p > (1 << 30)) return fail(LSPLMK_ERR_UNSUPPORTED, who + "more than 2^30 rows");
        const long long last = (long long)c.emit0 + c.n_emit - 1;
        if (c.nframe >= 0) {
            if (c.nframe != std::min(m, p)) return fail(LSPLMK_ERR_INVALID_ARGUMENT, who + "nframe must be min(mouth rows, poses) at finish");
            if (last >= c.nframe) return fail(LSPLMK_ERR_INVALID_ARGUMENT, who + "emits frames past nframe");
        } else if (c.n_emit && (last + h->rf[0] >= std::min(m, p) || last + fpose >= p ||
                                // the start reflection mirrors rows 0 .. r - 1 - k into frame k's past taps
                                (long long)h->r[0] - 1 - c.emit0 >= std::min(m, p) || (long long)rpose - 1 - c.emit0 >= p)) {
            return fail(LSPLMK_ERR_INVALID_ARGUMENT, who + "emits a frame whose window is not complete");
        }
        // the oldest row a frame of this call reads (the delta AMP reads frame k - 1 too); everything from it on must fit the ring
        const long long low_m = std::max(0LL, (long long)c.emit0 - h->r[0] - 1), low_p = std::max(0LL, (long long)c.emit0 - rpose);
        if ((c.mouth_have > low_m && m - low_m > cap) || (c.pose_have > low_p && p - low_p > cap) || c.mouth_fresh > cap || c.pose_fresh > cap)
            return fail(LSPLMK_ERR_STATE, who + "the ring (ring_rows) cannot hold the rows that the next frame still needs plus this push");
    }
    return LSPLMK_OK;
}

int lsplmk_tick(const lsplmk_handle *h, int nsessions, const lsplmk_session_call *calls, void *hip_stream)
{
    if (!h || !h->params_dev || !h->state_dev) return fail(LSPLMK_ERR_STATE, "tick: no handle, or bind_params / bind_state has not been called");
    const int rc = lsplmk_check_tick(h, nsessions, calls);
    if (rc) return rc;
    TickArgs a;
    std::memset(&a, 0, sizeof a);
    const int cap = h->ring_rows;
    int blocks = 0;
    for (int i = 0; i < nsessions; ++i) {
        const lsplmk_session_call &c = calls[i];
        Sess &s = a.s[i];
        s.mouth = c.mouth_dev; s.poses = c.poses_dev; s.out = c.out_dev; s.ring = h->state_dev + (size_t)c.slot * cap * ROWF;
        s.m_have = c.mouth_have; s.m_fresh = c.mouth_fresh; s.p_have = c.pose_have; s.p_fresh = c.pose_fresh; s.p_stride = c.pose_stride;
        s.emit0 = c.emit0; s.nframe = c.nframe; s.p_total = c.nframe >= 0 ? c.pose_have + c.pose_fresh : -1;
        blocks += c.n_emit;
        s.blk_end = blocks;
    }
    a.n = nsessions; a.emit_blocks = blocks; a.mode = 0;
    return launch(h, a, blocks + nsessions, hip_stream, "tick");
}

}  // extern "C"
