// resample.hip -- the audio input stage (include/lsprs.h): raw capture audio of any supported rate -> 16 kHz mono float32, streamed.
//
// A polyphase FIR with a table per rate: output j reads 2R + 1 input samples around c_j = (j M) div L with the taps of phase (j M) mod L.
// A frame of live audio is a few hundred outputs of a few hundred taps per session: far below a microsecond of one CU, so the launch is
// the cost and ALL sessions of ALL rates of a tick are ONE launch.  A workgroup owns 256 consecutive outputs of one session (the grid is
// the prefix sum over the sessions) and stages their input span -- ceil(256 M / L) + 2R + 1 samples -- into LDS once: each staged sample
// comes from the session's history ring when it lies before the call's first fresh sample and from the call's fresh buffer otherwise
// ("wherever the rows lie", as landmarks.hip); int16 is converted and two channels are downmixed on the way in, so a raw sample is read
// once; zeros stand below 0 and, at finish, at or above N.  Then one lane per output runs its phase's taps through one accumulator, in
// ascending tap order -- `taps()` below, the only place an output is computed, for a clip and for a tick.  One more workgroup per session
// copies the tail of the fresh input (as mono float32) into the ring.
//
// RING INVARIANT (lsprs.h): capacity = history + max_push, sample n at ring[n mod capacity]; a launch reads [have - history, have) and
// writes [have, have + fresh), fresh <= max_push: fewer than `capacity` consecutive indices, so the written slots are disjoint from the
// read ones and the copy workgroup runs unordered against the others.  lsprs_check_tick holds every call to it.
//
// Table layout [tap][phase]: the 64 lanes of a wave have consecutive outputs, their phases step by M mod L, and all gather within the
// one row of L floats of tap i (640 bytes at 44.1 kHz, 1 280 at 22.05 kHz).  With L == 1 the coefficient is wave-uniform and has a
// loop of its own: this toolchain reads it with uniform-address vector loads, eight taps in two dwordx4 (one cache line for the wave).  Lanes read LDS at stride M / L: conflict-free at 48 kHz (3), 2-way at 32 kHz.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lsprs.h"

namespace lsprs {

constexpr int NT = 256;                       // lanes = outputs per workgroup
constexpr int ZEROS = 64;
constexpr double BETA = 14.769656459379492, ROLLOFF = 0.9475937167399596;
// the widest span: Fi = 192 kHz (M / L = 12, R = 768): ceil(255 * 12) + 2 * 768 + 1 = 4 597 floats; create refuses a rate that needs more
constexpr int LDS_FLOATS = 4608;

struct Sess {
    const void *fresh;                        // raw, [total - have][channels]
    float *out;                               // output out0 at out[0]
    float *ring;                              // the slot's `cap` floats; null for a clip (have == 0)
    const float *coef;                        // [2R + 1][L]
    long long have, total, out0, n_out;       // stream samples before / after this call, first output, outputs
    int32_t blk_end;                          // prefix sum of output workgroups
    int32_t L, M, R, fmt, channels, pad_;
};

struct Args {
    Sess s[LSPRS_MAX_SESSIONS];
    int32_t n, out_blocks, cap, hist;
};

// fresh sample m of the call as mono float32
__device__ __forceinline__ float raw_at(const Sess &s, long long m)
{
    if (s.fmt == LSPRS_FMT_S16) {
        const int16_t *p = static_cast<const int16_t *>(s.fresh);
        if (s.channels == 1) return (float)p[m] / 32768.0f;
        const float a = (float)p[2 * m] / 32768.0f, b = (float)p[2 * m + 1] / 32768.0f;
        return (a + b) * 0.5f;
    }
    const float *p = static_cast<const float *>(s.fresh);
    if (s.channels == 1) return p[m];
    return (p[2 * m] + p[2 * m + 1]) * 0.5f;
}

// one output: taps in ascending order through one accumulator, one fmaf per tap.  x: the output's 2R + 1 staged samples.
__device__ __forceinline__ float taps(const float *__restrict__ coef, const float *x, int L, int p, int ntaps)
{
    float acc = 0.0f;
    if (L == 1) {
        for (int i = 0; i < ntaps; ++i) acc = fmaf(coef[i], x[i], acc);                 // wave-uniform address
    } else {
        const float *c = coef + p;
        for (int i = 0; i < ntaps; ++i) acc = fmaf(c[(size_t)i * L], x[i], acc);
    }
    return acc;
}

__global__ __launch_bounds__(NT) void rs_outputs(const Args A)
{
    __shared__ float xs[LDS_FLOATS];
    const int t = threadIdx.x, b = blockIdx.x;
    if (b >= A.out_blocks) {                                                           // the session's fresh tail -> its ring
        const Sess &s = A.s[b - A.out_blocks];
        if (!s.ring) return;
        const long long n0 = std::max(s.have, s.total - (long long)A.hist);
        for (long long n = n0 + t; n < s.total; n += NT) s.ring[(int)(n % A.cap)] = raw_at(s, n - s.have);
        return;
    }
    int si = 0;
    while (si < A.n - 1 && b >= A.s[si].blk_end) ++si;
    const Sess &s = A.s[si];
    const int blk = b - (si ? A.s[si - 1].blk_end : 0);
    const long long j0 = s.out0 + (long long)blk * NT, left = s.n_out - (long long)blk * NT;
    const int nj = (int)std::min<long long>(NT, left);
    if (nj <= 0) return;
    const int L = s.L, M = s.M, R = s.R;
    const long long c_first = j0 * M / L, c_last = (j0 + nj - 1) * M / L;
    const long long base = c_first - R;
    const int count = std::min((int)(c_last - c_first) + 2 * R + 1, LDS_FLOATS);
    const unsigned cap = (unsigned)A.cap;
    const unsigned base_mod = (unsigned)(((base % (long long)cap) + cap) % cap);
    for (int k = t; k < count; k += NT) {
        const long long n = base + k;
        float v = 0.0f;
        if (n >= 0 && n < s.total) v = n >= s.have ? raw_at(s, n - s.have) : s.ring[(base_mod + (unsigned)k) % cap];
        xs[k] = v;
    }
    __syncthreads();
    if (t < nj) {
        const long long jm = (j0 + t) * M, c = jm / L;
        const int p = (int)(jm - c * L), at = (int)(c - c_first);
        if (at + 2 * R + 1 <= count) s.out[(long long)blk * NT + t] = taps(s.coef, xs + at, L, p, 2 * R + 1);
    }
}

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }

struct Rate {
    int fi = 0, L = 0, M = 0, R = 0;
    size_t offset = 0;                        // floats into the blob
};

static double bessel_i0(double x)
{
    const double q = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

// h at u = num / L input samples
static double kernel_at(long long num, int L, int M)
{
    const long long lim = (long long)ZEROS * std::max(L, M);                           // |s u| < Z  <=>  |num| < Z max(L, M)
    if (std::llabs(num) >= lim) return 0.0;
    const double s = M > L ? (double)L / M : 1.0, u = (double)num / L;
    const double a = s * ROLLOFF * u, w = s * u / ZEROS;
    const double pi = 3.14159265358979323846;
    const double sinc = a == 0.0 ? 1.0 : std::sin(pi * a) / (pi * a);
    return s * ROLLOFF * sinc * bessel_i0(BETA * std::sqrt(std::max(0.0, 1.0 - w * w))) / bessel_i0(BETA);
}

}  // namespace lsprs

using namespace lsprs;

struct lsprs_handle {
    std::vector<float> blob;
    Rate rate[LSPRS_MAX_RATES];
    int n_rates = 0, max_sessions = 0, max_push = 0, hist = 0, cap = 0;
    const float *params_dev = nullptr;
    float *state_dev = nullptr;
    long long launches = 0;
};

static long long out_count(const Rate &r, long long n, int finished)
{
    const long long m = finished ? n : n - r.R;
    return m <= 0 ? 0 : (m * r.L + r.M - 1) / r.M;
}

static int launch(lsprs_handle *h, const Args &a, long long blocks, void *stream, const char *what)
{
    if (blocks <= 0) return LSPRS_OK;
    if (blocks > 0x7fffffffLL) return fail(LSPRS_ERR_UNSUPPORTED, std::string(what) + ": more than 2^31 workgroups");
    hipLaunchKernelGGL(rs_outputs, dim3((unsigned)blocks), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LSPRS_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    ++h->launches;
    return LSPRS_OK;
}

extern "C" {

const char *lsprs_last_error(void) { return g_err.c_str(); }
int lsprs_abi_version(void) { return LSPRS_ABI_VERSION; }

int lsprs_create(const lsprs_config *c, lsprs_handle **out)
{
    if (!out) return fail(LSPRS_ERR_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    if (!c || c->abi_version != LSPRS_ABI_VERSION) return fail(LSPRS_ERR_INVALID_ARGUMENT, "null config or abi_version mismatch");
    if (c->n_rates < 1 || c->n_rates > LSPRS_MAX_RATES) return fail(LSPRS_ERR_UNSUPPORTED, "n_rates must be in 1..LSPRS_MAX_RATES (4)");
    if (c->max_sessions < 1 || c->max_sessions > LSPRS_MAX_SESSIONS) return fail(LSPRS_ERR_INVALID_ARGUMENT, "max_sessions must be in 1..16");
    if (c->max_push < 1 || c->max_push > (1 << 24)) return fail(LSPRS_ERR_INVALID_ARGUMENT, "max_push must be in 1..2^24");
    Rate rates[LSPRS_MAX_RATES];
    size_t total = 0;
    int rmax = 0;
    for (int k = 0; k < c->n_rates; ++k) {
        const int fi = c->rates[k];
        const std::string who = "rate " + std::to_string(fi) + ": ";
        if (fi < LSPRS_MIN_RATE || fi > LSPRS_MAX_RATE) return fail(LSPRS_ERR_UNSUPPORTED, who + "outside 8000..192000");
        for (int q = 0; q < k; ++q)
            if (c->rates[q] == fi) return fail(LSPRS_ERR_INVALID_ARGUMENT, who + "named twice");
        int a = fi, b = LSPRS_OUT_RATE;
        while (b) { const int r = a % b; a = b; b = r; }
        Rate &r = rates[k];
        r.fi = fi; r.L = LSPRS_OUT_RATE / a; r.M = fi / a;
        // Fi == 16000: no resampling (what librosa.load does at the target rate); else R = ceil(Z / s)
        r.R = fi == LSPRS_OUT_RATE ? 0 : (r.M > r.L ? (int)(((long long)ZEROS * r.M + r.L - 1) / r.L) : ZEROS);
        const long long table = (long long)r.L * (2 * r.R + 1);
        if (table > LSPRS_MAX_TABLE)
            return fail(LSPRS_ERR_UNSUPPORTED, who + "its table of L * (2R + 1) = " + std::to_string(table) + " coefficients exceeds " + std::to_string(LSPRS_MAX_TABLE));
        if (((long long)(NT - 1) * r.M + r.L - 1) / r.L + 2 * r.R + 1 > LDS_FLOATS) return fail(LSPRS_ERR_UNSUPPORTED, who + "the input span of 256 outputs does not fit the LDS staging buffer");
        r.offset = total;
        total += ((size_t)table + 3) & ~(size_t)3;                                     // every table 16-byte aligned
        rmax = std::max(rmax, r.R);
    }
    lsprs_handle *h = new lsprs_handle;
    h->blob.assign(total, 0.0f);
    for (int k = 0; k < c->n_rates; ++k) {
        const Rate &r = h->rate[k] = rates[k];
        float *t = h->blob.data() + r.offset;
        for (int i = 0; i <= 2 * r.R; ++i)
            for (int p = 0; p < r.L; ++p)                                              // coef[p][i] = float32(h(p / L + R - i)), tap-major
                t[(size_t)i * r.L + p] = r.R == 0 ? 1.0f : (float)kernel_at(p + (long long)(r.R - i) * r.L, r.L, r.M);
    }
    h->n_rates = c->n_rates; h->max_sessions = c->max_sessions; h->max_push = c->max_push;
    h->hist = 2 * rmax;
    h->cap = h->hist + c->max_push;
    *out = h;
    return LSPRS_OK;
}

int lsprs_destroy(lsprs_handle *h)
{
    delete h;
    return LSPRS_OK;
}

int lsprs_rate_info(const lsprs_handle *h, int k, int32_t *L, int32_t *M, int32_t *R, size_t *table_offset_bytes)
{
    if (!h || k < 0 || k >= h->n_rates) return fail(LSPRS_ERR_INVALID_ARGUMENT, "rate_info: null handle or rate index out of range");
    if (L) *L = h->rate[k].L;
    if (M) *M = h->rate[k].M;
    if (R) *R = h->rate[k].R;
    if (table_offset_bytes) *table_offset_bytes = h->rate[k].offset * sizeof(float);
    return LSPRS_OK;
}

int lsprs_history(const lsprs_handle *h) { return h ? h->hist : 0; }

size_t lsprs_params_bytes(const lsprs_handle *h) { return h ? h->blob.size() * sizeof(float) : 0; }

int lsprs_pack_params(const lsprs_handle *h, void *host_buf, size_t bytes)
{
    if (!h || !host_buf || bytes < lsprs_params_bytes(h)) return fail(LSPRS_ERR_INVALID_ARGUMENT, "pack_params: null argument or buffer too small");
    std::memcpy(host_buf, h->blob.data(), lsprs_params_bytes(h));
    return LSPRS_OK;
}

int lsprs_bind_params(lsprs_handle *h, const void *params_dev, size_t bytes)
{
    if (!h || !params_dev || bytes < lsprs_params_bytes(h) || (reinterpret_cast<uintptr_t>(params_dev) & 15))
        return fail(LSPRS_ERR_INVALID_ARGUMENT, "bind_params: null or misaligned pointer, or fewer than lsprs_params_bytes() bytes");
    h->params_dev = static_cast<const float *>(params_dev);
    return LSPRS_OK;
}

size_t lsprs_state_bytes(const lsprs_handle *h) { return h ? (size_t)h->max_sessions * h->cap * sizeof(float) : 0; }

int lsprs_bind_state(lsprs_handle *h, void *state_dev, size_t bytes)
{
    if (!h || !state_dev || bytes < lsprs_state_bytes(h) || (reinterpret_cast<uintptr_t>(state_dev) & 3))
        return fail(LSPRS_ERR_INVALID_ARGUMENT, "bind_state: null or misaligned pointer, or fewer than lsprs_state_bytes() bytes");
    h->state_dev = static_cast<float *>(state_dev);
    return LSPRS_OK;
}

int64_t lsprs_out_count(const lsprs_handle *h, int rate_index, int64_t n_in_total, int finished)
{
    if (!h || rate_index < 0 || rate_index >= h->n_rates) return fail(LSPRS_ERR_INVALID_ARGUMENT, "out_count: null handle or rate index out of range");
    if (n_in_total < 0 || n_in_total > (1LL << 40)) return fail(LSPRS_ERR_UNSUPPORTED, "out_count: a stream has 0..2^40 samples");
    return out_count(h->rate[rate_index], n_in_total, finished);
}

static int check_format(int format, int channels, const std::string &who)
{
    if (format != LSPRS_FMT_F32 && format != LSPRS_FMT_S16) return fail(LSPRS_ERR_INVALID_ARGUMENT, who + "format must be LSPRS_FMT_F32 or LSPRS_FMT_S16");
    if (channels != 1 && channels != 2) return fail(LSPRS_ERR_UNSUPPORTED, who + std::to_string(channels) + " channels (1 or 2 are supported)");
    return LSPRS_OK;
}

static void fill(Sess &s, const lsprs_handle *h, const Rate &r, int format, int channels)
{
    s.coef = h->params_dev + r.offset;
    s.L = r.L; s.M = r.M; s.R = r.R; s.fmt = format; s.channels = channels;
}

int lsprs_clip(lsprs_handle *h, int rate_index, int format, int channels, const void *in_dev, int64_t n_in, float *out_dev, int64_t n_out,
               void *hip_stream)
{
    if (!h || !h->params_dev) return fail(LSPRS_ERR_STATE, "clip: no handle, or lsprs_bind_params has not been called");
    if (rate_index < 0 || rate_index >= h->n_rates) return fail(LSPRS_ERR_INVALID_ARGUMENT, "clip: rate index out of range");
    const int rc = check_format(format, channels, "clip: ");
    if (rc) return rc;
    if (n_in < 0 || n_in > (1LL << 40)) return fail(LSPRS_ERR_UNSUPPORTED, "clip: 0..2^40 samples");
    const Rate &r = h->rate[rate_index];
    if (n_out != out_count(r, n_in, 1)) return fail(LSPRS_ERR_INVALID_ARGUMENT, "clip: n_out must be lsprs_out_count(rate_index, n_in, 1)");
    if (n_out == 0) return LSPRS_OK;
    if (!in_dev || !out_dev) return fail(LSPRS_ERR_INVALID_ARGUMENT, "clip: null pointer");
    Args a;
    std::memset(&a, 0, sizeof a);
    Sess &s = a.s[0];
    fill(s, h, r, format, channels);
    s.fresh = in_dev; s.out = out_dev; s.ring = nullptr;
    s.have = 0; s.total = n_in; s.out0 = 0; s.n_out = n_out;
    const long long blocks = (n_out + NT - 1) / NT;
    if (blocks > 0x7fffffffLL) return fail(LSPRS_ERR_UNSUPPORTED, "clip: more than 2^31 workgroups");
    s.blk_end = (int32_t)blocks;
    a.n = 1; a.out_blocks = (int32_t)blocks; a.cap = 1; a.hist = 0;
    return launch(h, a, blocks, hip_stream, "clip");
}

// every count of a tick against the finality rule and the ring invariant: what lsprs_tick checks before it enqueues anything.  Follows no pointer.
int lsprs_check_tick(const lsprs_handle *h, int nsessions, const lsprs_session_call *calls)
{
    if (!h) return fail(LSPRS_ERR_INVALID_ARGUMENT, "tick: null handle");
    if (nsessions < 0 || nsessions > h->max_sessions || (nsessions && !calls)) return fail(LSPRS_ERR_INVALID_ARGUMENT, "tick: nsessions outside 0..max_sessions");
    unsigned used = 0;
    for (int i = 0; i < nsessions; ++i) {
        const lsprs_session_call &c = calls[i];
        const std::string who = "tick: session " + std::to_string(i) + ": ";
        if (c.slot < 0 || c.slot >= h->max_sessions || (used >> c.slot & 1)) return fail(LSPRS_ERR_INVALID_ARGUMENT, who + "slot out of range or named twice");
        used |= 1u << c.slot;
        if (c.rate_index < 0 || c.rate_index >= h->n_rates) return fail(LSPRS_ERR_INVALID_ARGUMENT, who + "rate index out of range");
        const int rc = check_format(c.format, c.channels, who);
        if (rc) return rc;
        if (c.n_have < 0 || c.n_fresh < 0 || c.out0 < 0 || c.n_out < 0) return fail(LSPRS_ERR_INVALID_ARGUMENT, who + "negative count");
        if (c.n_fresh > h->max_push)
            return fail(LSPRS_ERR_STATE, who + std::to_string(c.n_fresh) + " fresh samples; the ring (history + max_push) takes at most " + std::to_string(h->max_push) + " per tick");
        const long long total = c.n_have + c.n_fresh;
        if (total > (1LL << 40)) return fail(LSPRS_ERR_UNSUPPORTED, who + "more than 2^40 samples");
        if ((c.n_fresh && !c.fresh_dev) || (c.n_out && !c.out_dev)) return fail(LSPRS_ERR_INVALID_ARGUMENT, who + "null pointer");
        const Rate &r = h->rate[c.rate_index];
        if (c.out0 + c.n_out > out_count(r, total, c.finished)) return fail(LSPRS_ERR_INVALID_ARGUMENT, who + "emits an output whose taps are not all present");
        // the oldest sample the first output reads must still be in the ring
        if (c.n_out && std::max(0LL, (long long)c.out0 * r.M / r.L - r.R) < c.n_have - h->hist)
            return fail(LSPRS_ERR_STATE, who + "its first output reads samples the ring no longer holds");
    }
    return LSPRS_OK;
}

int lsprs_tick(lsprs_handle *h, int nsessions, const lsprs_session_call *calls, void *hip_stream)
{
    if (!h || !h->params_dev || !h->state_dev) return fail(LSPRS_ERR_STATE, "tick: no handle, or bind_params / bind_state has not been called");
    const int rc = lsprs_check_tick(h, nsessions, calls);
    if (rc) return rc;
    Args a;
    std::memset(&a, 0, sizeof a);
    long long blocks = 0, work = 0;
    for (int i = 0; i < nsessions; ++i) {
        const lsprs_session_call &c = calls[i];
        Sess &s = a.s[i];
        fill(s, h, h->rate[c.rate_index], c.format, c.channels);
        s.fresh = c.fresh_dev; s.out = c.out_dev; s.ring = h->state_dev + (size_t)c.slot * h->cap;
        s.have = c.n_have; s.total = c.n_have + c.n_fresh; s.out0 = c.out0; s.n_out = c.n_out;
        blocks += (c.n_out + NT - 1) / NT;
        s.blk_end = (int32_t)blocks;
        work += c.n_out + c.n_fresh;
    }
    if (work == 0) return LSPRS_OK;                                                    // nothing to compute and nothing to store
    a.n = nsessions; a.out_blocks = (int32_t)blocks; a.cap = h->cap; a.hist = h->hist;
    return launch(h, a, blocks + nsessions, hip_stream, "tick");
}

int64_t lsprs_launch_count(const lsprs_handle *h) { return h ? h->launches : 0; }

}  // extern "C"
