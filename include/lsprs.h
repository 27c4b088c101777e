/* lsprs.h -- C ABI of the audio input stage: demo.py:179 (`librosa.load(path, sr=16000)`) as a streaming, pooled resampler on the device.
 * Exported by livespeechportraits_amd/liblspf2f.so; gfx950 only, no CPU path.
 *
 * Raw capture audio (any supported rate, float32 or int16, one or two interleaved channels) in, 16 kHz mono float32 out.
 *
 * The contract (PARITY-UNPINNED against librosa / resampy, which evaluate the same filter through a 512-per-zero-crossing table with
 * linear interpolation: this is the ideal filter resampy's `kaiser_best` approximates, in closed form).  Fi = input rate, Fo = 16000,
 *   g = gcd(Fi, Fo), L = Fo / g, M = Fi / g, s = min(1, Fo / Fi),
 *   Z = 64 zero crossings, beta = 14.769656459379492, rho = 0.9475937167399596           (resampy's published kaiser_best parameters)
 *   h(u) = s rho sinc(s rho u) I0(beta sqrt(1 - (s u / Z)^2)) / I0(beta)   for |s u| < Z, 0 outside      (u in input samples)
 *   R = ceil(Z / s)                                                                       (half-width in input samples)
 *   output j reads at input time j M / L: c_j = (j M) div L, p_j = (j M) mod L
 *   y[j] = sum_{i = 0 .. 2R} coef[p_j][i] x[c_j - R + i],   coef[p][i] = float32(h(p / L + R - i))
 * Input samples outside [0, N) are zero: before the stream starts and, once it has finished, past its end.  A stream of N input samples
 * has ceil(N L / M) outputs (librosa's n_samples), all computed.  Arithmetic: float32, one accumulator per output, taps in ascending i,
 * each step one fmaf -- the same device function for a clip and for a tick, so the result does not depend on how a stream was cut.
 * The tables are designed in double by lsprs_create and rounded once.  int16 is converted as x / 32768.0f; two channels are averaged as
 * (a + b) * 0.5f after conversion (librosa.to_mono).  Fi == 16000 is no resampling (librosa.load does none either): R = 0 and the one tap
 * 1.0f, i.e. format conversion and downmix only; a caller holding 16 kHz mono float32 has nothing to call.
 *
 * Finality: while a stream of N samples runs, output j is final when c_j + R <= N - 1 (lookahead R input samples: 4 ms at Fi >= 16 kHz,
 * 8 ms at 8 kHz); at finish every j < ceil(N L / M) is.  lsprs_out_count states the rule.
 *
 * The ring of a slot holds history + max_push mono float32 samples, history = 2 * (largest R of the handle); stream sample n lives in
 * ring[n mod capacity].  INVARIANT: a launch reads ring samples [have - history, have) and writes [have, have + fresh) with
 * fresh <= max_push, a span of at most `capacity` consecutive indices -- so the slots a launch writes are disjoint from the slots it
 * reads, and the copy workgroup needs no ordering against the output workgroups.  The first non-final output j0 of a running stream has
 * c_j0 >= have - R, so it reads no sample below have - 2R.  lsprs_check_tick checks both halves on every call.
 *
 * Conventions: device pointers, nothing allocated by the library, no synchronisation, returns 0 or a negative code (lsprs_last_error()).
 * create / params_bytes / pack_params / state_bytes / rate_info / out_count / check_tick touch no device.
 */
#ifndef LSPRS_H
#define LSPRS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden: exactly the functions declared below are exported */
#pragma GCC visibility push(default)

#define LSPRS_OK 0
#define LSPRS_ERR_INVALID_ARGUMENT (-1)
#define LSPRS_ERR_UNSUPPORTED (-2)
#define LSPRS_ERR_HIP (-3)
#define LSPRS_ERR_STATE (-4)

#define LSPRS_ABI_VERSION 1
#define LSPRS_MAX_SESSIONS 16
#define LSPRS_MAX_RATES 4
#define LSPRS_MIN_RATE 8000
#define LSPRS_MAX_RATE 192000
#define LSPRS_MAX_TABLE 262144      /* coefficients of one rate: L * (2R + 1) */
#define LSPRS_OUT_RATE 16000

#define LSPRS_FMT_F32 0
#define LSPRS_FMT_S16 1

typedef struct lsprs_handle lsprs_handle;

typedef struct lsprs_config {
    int32_t abi_version;
    int32_t n_rates;                    /* 1..LSPRS_MAX_RATES */
    int32_t rates[LSPRS_MAX_RATES];     /* distinct integers in LSPRS_MIN_RATE..LSPRS_MAX_RATE whose table has at most LSPRS_MAX_TABLE coefficients */
    int32_t max_sessions;               /* 1..LSPRS_MAX_SESSIONS ring slots */
    int32_t max_push;                   /* most input samples (per channel) one session brings in one tick, >= 1 */
} lsprs_config;

/* one session of a tick.  Input samples [0, n_have) of the stream are behind it (their last `history` in the slot's ring), the n_fresh
 * ones at fresh_dev are this call's ([n_fresh][channels], interleaved); the call stores their tail in the ring.  Outputs
 * [out0, out0 + n_out) are written to out_dev; out0 + n_out <= lsprs_out_count(rate_index, n_have + n_fresh, finished). */
typedef struct lsprs_session_call {
    int32_t slot;
    int32_t rate_index;
    int32_t format;                     /* LSPRS_FMT_* */
    int32_t channels;                   /* 1 or 2 */
    int64_t n_have;
    int64_t out0;
    int32_t n_fresh;
    int32_t n_out;
    int32_t finished;                   /* 1: the stream ends with this call's samples */
    int32_t reserved;
    const void *fresh_dev;
    float *out_dev;
} lsprs_session_call;

int lsprs_create(const lsprs_config *cfg, lsprs_handle **out);
int lsprs_destroy(lsprs_handle *h);
const char *lsprs_last_error(void);
int lsprs_abi_version(void);

/* L, M, R of a rate and where its table lies in the params blob: float32 [2R + 1][L], tap-major (coef[p][i] at [i * L + p]) */
int lsprs_rate_info(const lsprs_handle *h, int rate_index, int32_t *L, int32_t *M, int32_t *R, size_t *table_offset_bytes);
/* samples of history a ring keeps (2 * the largest R) */
int lsprs_history(const lsprs_handle *h);

/* the coefficient tables of all rates as one blob: packed on the host, uploaded once by the caller, bound as a device pointer */
size_t lsprs_params_bytes(const lsprs_handle *h);
int lsprs_pack_params(const lsprs_handle *h, void *host_buf, size_t bytes);
int lsprs_bind_params(lsprs_handle *h, const void *params_dev, size_t bytes);
/* the rings of all max_sessions slots; their content on entry is irrelevant (a session starts with n_have == 0) */
size_t lsprs_state_bytes(const lsprs_handle *h);
int lsprs_bind_state(lsprs_handle *h, void *state_dev, size_t bytes);

/* how many outputs of a stream with n_in_total input samples are final (negative: an error code) */
int64_t lsprs_out_count(const lsprs_handle *h, int rate_index, int64_t n_in_total, int finished);

/* whole clip: in_dev [n_in][channels] -> out_dev [n_out], n_out == lsprs_out_count(rate_index, n_in, 1).  One launch, no ring. */
int lsprs_clip(lsprs_handle *h, int rate_index, int format, int channels, const void *in_dev, int64_t n_in, float *out_dev, int64_t n_out,
               void *hip_stream);

/* one tick of up to max_sessions sessions (distinct slots) of any mix of rates and formats: ONE launch -- a workgroup per 256 outputs of
 * a session, one per session that stores its fresh samples.  Nothing is enqueued when a count is refused. */
int lsprs_tick(lsprs_handle *h, int nsessions, const lsprs_session_call *calls, void *hip_stream);
/* those checks alone: touches no device, follows no pointer, needs no bind */
int lsprs_check_tick(const lsprs_handle *h, int nsessions, const lsprs_session_call *calls);
/* kernel launches this handle has enqueued so far (clip and tick) */
int64_t lsprs_launch_count(const lsprs_handle *h);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
