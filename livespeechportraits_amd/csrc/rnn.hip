// Recurrent stacks of the audio front-end (include/lsprnn.h): multi-layer GRU / LSTM over one or several sequences, gfx950 only.
//
// The recurrent step is written once, as the __device__ functions below, and runs in two kernels: rnn_wave (one sequence) and
// rnn_wave_multi (up to LSPRNN_MAX_SEQUENCES sequences per launch).  Each has two routes, chosen at compile time:
//   STACKED (default for stacks): every layer runs in the same launch as a wavefront in time; only layer 0's input projection
//     W_ih x_t + biases comes from a gemm_f32 launch (no recurrence in it).
//   one launch per layer (STACKED = false): per layer, one gemm_f32 launch computes the input projection for every step, then one launch
//     runs that layer's recurrence.
// Either way the hidden units of a layer are split over workgroups of 512 threads: P lanes share a unit and each keeps CPP columns of the
// unit's W_hh rows in registers for the whole sequence; every step the workgroups all-gather h_{t-1} from each other through 8-byte
// {value, epoch} granules (write-through stores, polls past L1, one slot per step: cdna_hip_programming.md Guideline 16 form R2 -- the same
// hand-off as csrc/a2h.hip).  The chain is latency-bound: one poll round trip + a mat-vec slice per step.
#include "../../include/lsprnn.h"

#include <hip/hip_runtime.h>

#include "gemm_f32.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

namespace lsprnn {

constexpr int NT = 512;
constexpr unsigned SPIN_LIMIT = 1u << 22;
constexpr int AUX_SC1 = 16;
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <int CTRL> __device__ __forceinline__ float dpp_add(float v)
{
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// sum over aligned groups of P lanes (8, 16 or 32), every lane gets the total
template <int P> __device__ __forceinline__ float sum_p(float v)
{
    v = dpp_add<0x4E>(dpp_add<0xB1>(v));        // quad_perm xor 1, xor 2
    v = dpp_add<0x141>(v);                      // row_half_mirror: + the other quad of the 8
    if (P >= 16) v = dpp_add<0x140>(v);         // row_mirror: + the other half of the 16
    if (P == 32) v += __shfl_xor(v, 16);        // the neighbouring DPP row
    return v;
}
__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }
__device__ __forceinline__ float dot4(float4 w, float4 v, float acc)
{
    acc = fmaf(w.x, v.x, acc); acc = fmaf(w.y, v.y, acc); acc = fmaf(w.z, v.z, acc); acc = fmaf(w.w, v.w, acc);
    return acc;
}

// ------------------------------------------------------------------------------------------------ the recurrent step, written once
// Every kernel below is made of these.  The promise of the live path -- any split of a sequence into calls, and any grouping of sequences
// into one call, gives the same bits -- rests on all of them running the same expressions in the same order.

// the register load of one packed matrix (lsprnn_pack_weights): [workgroup][N = GATES * CPP / 4][512 threads] float4
template <int N> __device__ __forceinline__ void load_packed(float4 (&W)[N], __amdgpu_buffer_rsrc_t blob, unsigned off, int wg, int tid)
{
#pragma unroll
    for (int i = 0; i < N; ++i)
        W[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
            blob, tid * 16, (int)(off + ((unsigned)wg * N + (unsigned)i) * NT * 16u), 0));
}

// the poll of one H-vector (threads tid < H): bounded, and given up early once another workgroup has set the status word
__device__ __forceinline__ bool poll_vector(__amdgpu_buffer_rsrc_t box, int slot, int tid, int H, unsigned epoch, unsigned *status, unsigned lost, float *dst)
{
    bool ok = true;
    if (tid < H) {
        for (unsigned spins = 0;;) {
            const u32x2 g = __builtin_amdgcn_raw_buffer_load_b64(box, tid * 8, slot, AUX_SC1);
            asm volatile("" ::: "memory");
            if (g.y == epoch) { dst[tid] = __uint_as_float(g.x); break; }
            if (++spins > SPIN_LIMIT || ((spins & 1023) == 0 && __hip_atomic_load(status, RLX_AGENT) != 0)) { ok = false; break; }
            __builtin_amdgcn_s_sleep(1);
        }
        if (!ok) atomicCAS(status, 0u, lost);       // the first loss names the launch's failure
    }
    return ok;
}

// the mat-vec slice of a thread: its Q float4 of every gate's row against its column part `v` of the vector, then the sum over the P parts
template <int GATES, int P, int Q> __device__ __forceinline__ void matvec(const float4 (&W)[GATES * Q], const float *vec, float (&a)[GATES])
{
    const float4 *v = reinterpret_cast<const float4 *>(vec);
#pragma unroll
    for (int g = 0; g < GATES; ++g) a[g] = 0.f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const float4 x = v[q];
#pragma unroll
        for (int g = 0; g < GATES; ++g) a[g] = dot4(W[g * Q + q], x, a[g]);
    }
#pragma unroll
    for (int g = 0; g < GATES; ++g) a[g] = sum_p<P>(a[g]);
}

// the leader's cell update: xg = the input side (W_ih x_t + biases), a = W_hh h_{t-1}; returns h_t and, for the LSTM, updates c
template <int GATES> __device__ __forceinline__ float cell_update(const float (&xg)[GATES], const float (&a)[GATES], float bhn, float hprev, float &c)
{
    if (GATES == 3) {
        const float r = sigmoidf(xg[0] + a[0]);
        const float z = sigmoidf(xg[1] + a[1]);
        const float n = tanhf(xg[2] + r * (a[2] + bhn));     // b_hn stays inside r * (...)
        return (1.f - z) * n + z * hprev;
    } else {
        const float i = sigmoidf(xg[0] + a[0]);
        const float f = sigmoidf(xg[1] + a[1]);
        const float g = tanhf(xg[2] + a[2]);
        const float o = sigmoidf(xg[GATES - 1] + a[GATES - 1]);
        c = f * c + i * g;
        return o * tanhf(c);
    }
}

// the granule of one unit: {h_t, epoch}, written through to where the other workgroups' polls read
__device__ __forceinline__ void store_granule(__amdgpu_buffer_rsrc_t box, int unit, int slot, float h, unsigned epoch)
{
    u32x2 gr; gr.x = __float_as_uint(h); gr.y = epoch;
    __builtin_amdgcn_raw_buffer_store_b64(gr, box, unit * 8, slot, AUX_SC1);
}

// a unit's final state in PyTorch's layout: h [layers][H], then (LSTM) c [layers][H]
template <int GATES> __device__ __forceinline__ void store_state(float *state, int layers, int l, int H, int unit, float h, float c)
{
    state[(size_t)l * H + unit] = h;
    if (GATES == 4) state[(size_t)(layers + l) * H + unit] = c;
}

// what a lost hand-off leaves in the status word: route, sequence (bits 26..29), layer (stacked route), step
template <bool STACKED> __device__ __forceinline__ unsigned lost_code(int s, int l, int t)
{
    return (STACKED ? 0x2000000u + ((unsigned)l << 20) : 0x1000000u) + ((unsigned)s << 26) + (unsigned)t;
}

// ------------------------------------------------------------------------------------------------ the kernels
// What only the stacked route holds: the W_ih rows of a workgroup's units (V) and their biases (bg), in registers.  The per-layer
// route's specialisation is empty, so that "no V registers" holds in the source and not by dead-code elimination.
template <int GATES, int Q, bool STACKED> struct InputSide {};
template <int GATES, int Q> struct InputSide<GATES, Q, true> {
    float4 V[GATES * Q];
    float bg[GATES];
    // layer 0 takes its input side from the gemm: zero V (never multiplied) and zero biases
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t blob, unsigned wih, const float *bias, int l, int wg, int tid, bool leader, int H, int unit)
    {
#pragma unroll
        for (int i = 0; i < GATES * Q; ++i) V[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (l > 0) load_packed(V, blob, wih, wg, tid);
#pragma unroll
        for (int g = 0; g < GATES; ++g) bg[g] = (l > 0 && leader) ? bias[g * H + unit] : 0.f;
    }
};

// What both kernels, and both routes of each, are given.  Stacked: every layer runs in this launch.  Not stacked: layer `layer` alone, with
// its input projection in xproj, its whole output in out, and mailbox plane 0 under a fresh epoch.
struct StackParams {
    const float *blob; unsigned blob_bytes;
    unsigned whh[8], wih[8];       // byte offsets per layer: packed W_hh; packed W_ih (stacked, layers >= 1, same thread map)
    const float *bias[8];          // stacked, layers >= 1: b_ih (+ b_hh except the GRU's n gate), [GATES*H]
    const float *bhn[8];           // GRU: b_hn [H] (stays inside r * (...)); LSTM: unused
    const float *xproj;            // [rows][GATES*H]: W_ih x_t + b_ih (+ b_hh for every gate except the GRU's n) of layer 0 / of `layer`
    float *out;                    // [rows][H]: the top layer's output / the output of `layer`
    unsigned long long *hbox;      // [layers][rows][H] granules (not stacked: plane 0 only)
    unsigned *status;
    unsigned epoch;
    int H, layers, layer, wgs_per_layer, stride;
};

struct WaveParams {
    StackParams k;
    const float *state_in;         // null, or h [layers][H] (then, LSTM, c [layers][H]): the initial state
    float *state_out;              // null, or the final state, same layout
    int T;
};

// GATES = 3 (GRU) or 4 (LSTM); P = H / CPP lanes share a unit, each with CPP columns; a workgroup owns U = 512 / P hidden units.
//
// STACKED: layer l works on step t while layer l-1 is already on a later step.  A workgroup of layer l >= 1 also keeps the W_ih rows of its
// units resident (its input is the layer below's h_t, known only step by step) and polls two vectors per step: its own layer's h_{t-1} and
// the layer below's h_t.  Layer 0 still takes its input projection from the gemm (x is known for all steps).  Two matrices per thread, so
// the columns are cut into parts of CPP = 16 (48 + 48 VGPRs of weights for a GRU, 64 + 64 for an LSTM); 32 parts of 32 columns spilled for
// the GRU-512.  Not STACKED: one matrix per thread (no V, no hlow, no second poll), so CPP = 32: 96 VGPRs of weights for a GRU, 128 for an
// LSTM, and no add of a zero W_ih product (x + 0.0f is not a no-op for -0.0f).
//
// rnn_wave and rnn_wave_multi stay two kernels.  The single form keeps hprev / cprev in leader registers and loads its projections itself;
// the multi form keeps h, c and the staged projections in dynamic LDS.  On a chain bound by one poll round trip per step that difference is
// not known to be free; DESIGN.md (section 10, "Against the four-kernel parent") records forward_multi with one sequence against
// forward_state: the multi form is the slower one.
template <int GATES, int P, int CPP, bool STACKED> __global__ __launch_bounds__(NT) void rnn_wave(WaveParams p)
{
    __shared__ __attribute__((aligned(16))) float hvec[STACKED ? 1024 : 512];
    float *const hown = hvec, *const hlow = hvec + 512;      // own layer's h_{t-1}; STACKED only: the layer below's h_t
    const StackParams &k = p.k;
    if (blockIdx.x % k.stride) return;
    const int b = blockIdx.x / k.stride;
    const int l = STACKED ? b / k.wgs_per_layer : k.layer, wg = STACKED ? b % k.wgs_per_layer : b;
    constexpr int U = NT / P, Q = CPP / 4;                  // units per workgroup; float4 per gate per thread
    const int tid = threadIdx.x, part = tid % P, ul = tid / P;
    const int unit = wg * U + ul;
    const int H = k.H;
    const __amdgpu_buffer_rsrc_t blob = __builtin_amdgcn_make_buffer_rsrc((void *)k.blob, 0, (int)k.blob_bytes, 0x00020000);
    const unsigned plane = (unsigned)p.T * (unsigned)H * 8u, own = STACKED ? (unsigned)l * plane : 0u;
    const __amdgpu_buffer_rsrc_t box = __builtin_amdgcn_make_buffer_rsrc((void *)k.hbox, 0, (int)(plane * (STACKED ? (unsigned)k.layers : 1u)), 0x00020000);
    float4 W[GATES * Q];
    InputSide<GATES, Q, STACKED> in;
    load_packed(W, blob, k.whh[l], wg, tid);
    if constexpr (STACKED) in.load(blob, k.wih[l], k.bias[l], l, wg, tid, part == 0, H, unit);
    const float bhn = (GATES == 3 && part == 0) ? k.bhn[l][unit] : 0.f;
    const bool top = !STACKED || l + 1 == k.layers;       // the layer whose h_t is the launch's output
    float hprev = 0.f, cprev = 0.f;                       // leader lanes: own unit's state
    const float *h0 = p.state_in ? p.state_in + (size_t)l * H : nullptr;
    if (part == 0 && p.state_in) {
        hprev = h0[unit];
        if (GATES == 4) cprev = p.state_in[(size_t)(k.layers + l) * H + unit];
    }
    for (int t = 0; t < p.T; ++t) {
        float xg[GATES];
        if constexpr (STACKED) {
#pragma unroll
            for (int g = 0; g < GATES; ++g) xg[g] = in.bg[g];
        }
        if ((!STACKED || l == 0) && part == 0) {
#pragma unroll
            for (int g = 0; g < GATES; ++g) xg[g] = k.xproj[((size_t)t * GATES + g) * H + unit];
        }
        // two polls per thread at most: own layer's h_{t-1} (slot t-1), the layer below's h_t (slot t)
        bool ok = true;
        if (t == 0) {
            if (tid < H) hown[tid] = h0 ? h0[tid] : 0.f;   // initial state (zero unless carried in)
        } else {
            ok = poll_vector(box, (int)(own + (unsigned)(t - 1) * (unsigned)H * 8u), tid, H, k.epoch, k.status, lost_code<STACKED>(0, l, t), hown);
        }
        if constexpr (STACKED)
            if (ok && l > 0) ok = poll_vector(box, (int)(own - plane + (unsigned)t * (unsigned)H * 8u), tid, H, k.epoch, k.status, lost_code<STACKED>(0, l, t), hlow);
        if (!__syncthreads_and(ok)) return;
        float a[GATES], c[GATES];
        matvec<GATES, P, Q>(W, hown + part * CPP, a);
        if constexpr (STACKED) {
#pragma unroll
            for (int g = 0; g < GATES; ++g) c[g] = 0.f;
            if (l > 0) matvec<GATES, P, Q>(in.V, hlow + part * CPP, c);
        }
        if (part == 0) {
            if constexpr (STACKED) {
#pragma unroll
                for (int g = 0; g < GATES; ++g) xg[g] += c[g];   // input side: W_ih h_below + biases (layer 0: from the gemm)
            }
            const float hn = cell_update<GATES>(xg, a, bhn, hprev, cprev);
            hprev = hn;
            if (t + 1 < p.T || !top)          // consumers: this layer's next step, and (stacked) the layer above at this step
                store_granule(box, unit, (int)(own + (unsigned)t * (unsigned)H * 8u), hn, k.epoch);
            if (top) k.out[(size_t)t * H + unit] = hn;
            if (t + 1 == p.T && p.state_out) store_state<GATES>(p.state_out, k.layers, l, H, unit, hn, cprev);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ several sequences per launch
// lsprnn_forward_multi: the kernel above for up to LSPRNN_MAX_SEQUENCES independent sequences in ONE launch.  The weights a thread
// holds in registers serve every sequence of a step; what is per sequence lives in LDS: the gathered h vectors ([S][H]), the leaders' cell
// state ([S][U]) and the step's input projections ([S][GATES][U], staged while the polls are in flight).  Per sequence the products, their
// order, the sum_p reduction and the gate arithmetic are those of the single-sequence kernel, one sequence at a time (no more accumulators
// are live than there), so each sequence gets the bits of lsprnn_forward_state alone.  Sequence s owns rows [off[s], off[s] + T[s]) of
// x / xproj / out and of every mailbox plane; a sequence shorter than the longest stops taking part once its steps are done.
struct SeqTable {
    const float *state_in[LSPRNN_MAX_SEQUENCES];   // null: zeros
    float *state_out[LSPRNN_MAX_SEQUENCES];        // null: not written
    int off[LSPRNN_MAX_SEQUENCES], T[LSPRNN_MAX_SEQUENCES];
    int S, Tmax, rows;                             // rows = sum T
};

struct WaveMultiParams {
    StackParams k;
    SeqTable q;
};

template <int GATES, int P, int CPP, bool STACKED> __global__ __launch_bounds__(NT) void rnn_wave_multi(WaveMultiParams p)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];      // multi_lds_bytes() on the host
    const StackParams &k = p.k;
    if (blockIdx.x % k.stride) return;
    const int b = blockIdx.x / k.stride;
    const int l = STACKED ? b / k.wgs_per_layer : k.layer, wg = STACKED ? b % k.wgs_per_layer : b;
    constexpr int U = NT / P, Q = CPP / 4;
    const int tid = threadIdx.x, part = tid % P, ul = tid / P;
    const int unit = wg * U + ul;
    const int H = k.H, S = p.q.S;
    float *hown = lds;                             // [S][H] own layer's h_{t-1}
    float *hlow = hown + S * H;                    // [S][H] the layer below's h_t (STACKED only: not reserved otherwise)
    float *cst = STACKED ? hlow + S * H : hlow;    // [S][U]          leaders: c of the own unit
    float *xs = cst + S * U;                       // [S][GATES][U]   this step's input projections of the own units (from the gemm)
    const __amdgpu_buffer_rsrc_t blob = __builtin_amdgcn_make_buffer_rsrc((void *)k.blob, 0, (int)k.blob_bytes, 0x00020000);
    const unsigned plane = (unsigned)p.q.rows * (unsigned)H * 8u, own = STACKED ? (unsigned)l * plane : 0u;
    const __amdgpu_buffer_rsrc_t box = __builtin_amdgcn_make_buffer_rsrc((void *)k.hbox, 0, (int)(plane * (STACKED ? (unsigned)k.layers : 1u)), 0x00020000);
    float4 W[GATES * Q];
    InputSide<GATES, Q, STACKED> in;
    load_packed(W, blob, k.whh[l], wg, tid);
    if constexpr (STACKED) in.load(blob, k.wih[l], k.bias[l], l, wg, tid, part == 0, H, unit);
    const float bhn = (GATES == 3 && part == 0) ? k.bhn[l][unit] : 0.f;
    const bool top = !STACKED || l + 1 == k.layers;
    const bool gemm_in = !STACKED || l == 0;       // this layer's input projection comes from the gemm
    if (GATES == 4 && part == 0)
        for (int s = 0; s < S; ++s) cst[s * U + ul] = p.q.state_in[s] ? p.q.state_in[s][(size_t)(k.layers + l) * H + unit] : 0.f;
    for (int t = 0; t < p.q.Tmax; ++t) {
        if (gemm_in)
            for (int i = tid; i < S * GATES * U; i += NT) {
                const int s = i / (GATES * U), r = i - s * (GATES * U), g = r / U, u = r - g * U;
                if (t < p.q.T[s]) xs[i] = k.xproj[((size_t)(p.q.off[s] + t) * GATES + g) * H + wg * U + u];
            }
        bool ok = true;
        // per sequence two polls per thread at most: own layer's h_{t-1} (row t-1), the layer below's h_t (row t)
        for (int s = 0; s < S && ok; ++s) {
            if (t >= p.q.T[s]) continue;
            const unsigned row = (unsigned)(p.q.off[s] + t);
            if (t == 0) {
                const float *h0 = p.q.state_in[s] ? p.q.state_in[s] + (size_t)l * H : nullptr;
                if (tid < H) hown[s * H + tid] = h0 ? h0[tid] : 0.f;
            } else {
                ok = poll_vector(box, (int)(own + (row - 1) * (unsigned)H * 8u), tid, H, k.epoch, k.status, lost_code<STACKED>(s, l, t), hown + s * H);
            }
            if constexpr (STACKED)
                if (ok && l > 0) ok = poll_vector(box, (int)(own - plane + row * (unsigned)H * 8u), tid, H, k.epoch, k.status, lost_code<STACKED>(s, l, t), hlow + s * H);
        }
        if (!__syncthreads_and(ok)) return;
        for (int s = 0; s < S; ++s) {
            if (t >= p.q.T[s]) continue;
            float a[GATES], c[GATES];
            matvec<GATES, P, Q>(W, hown + s * H + part * CPP, a);
            if constexpr (STACKED) {
#pragma unroll
                for (int g = 0; g < GATES; ++g) c[g] = 0.f;
                if (l > 0) matvec<GATES, P, Q>(in.V, hlow + s * H + part * CPP, c);
            }
            if (part == 0) {
                float xg[GATES];
                if constexpr (STACKED) {
#pragma unroll
                    for (int g = 0; g < GATES; ++g) xg[g] = l == 0 ? xs[(s * GATES + g) * U + ul] : in.bg[g];
#pragma unroll
                    for (int g = 0; g < GATES; ++g) xg[g] += c[g];   // input side: W_ih h_below + biases (layer 0: from the gemm)
                } else {
#pragma unroll
                    for (int g = 0; g < GATES; ++g) xg[g] = xs[(s * GATES + g) * U + ul];
                }
                const float hprev = hown[s * H + unit];          // h_{t-1} of the own unit: the value the single-sequence leader keeps in a register
                float cprev = GATES == 4 ? cst[s * U + ul] : 0.f;
                const float hn = cell_update<GATES>(xg, a, bhn, hprev, cprev);
                if (GATES == 4) cst[s * U + ul] = cprev;
                const unsigned row = (unsigned)(p.q.off[s] + t);
                if (t + 1 < p.q.T[s] || !top)     // consumers: this layer's next step, and (stacked) the layer above at this step
                    store_granule(box, unit, (int)(own + row * (unsigned)H * 8u), hn, k.epoch);
                if (top) k.out[(size_t)row * H + unit] = hn;
                if (t + 1 == p.q.T[s] && p.q.state_out[s]) store_state<GATES>(p.q.state_out[s], k.layers, l, H, unit, hn, cprev);
            }
        }
        __syncthreads();
    }
}

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
static int hipfail(hipError_t e, const char *what) { return fail(LSPRNN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
static size_t align64(size_t v) { return (v + 63) & ~(size_t)63; }

struct Slot {
    std::string key;
    size_t numel = 0;
    std::vector<float> data;
    bool set = false;
};

// how a route cuts a layer: P lanes share a unit, each with CPP columns; U units per workgroup, G workgroups per layer
struct Geometry { int CPP, P, U, G; };
static Geometry geometry(int H, int cpp) { Geometry g{cpp, H / cpp, 0, 0}; g.U = NT / g.P; g.G = H / g.U; return g; }

struct Fit { bool checked = false, fits = false; };      // a cached residency answer
enum { SINGLE = 0, MULTI = 1 };                           // the kernel families
static const char *const kernel_name[2] = {"rnn_wave", "rnn_wave_multi"};

struct Workspace {
    float *xproj, *hs[2];          // the input projection; the per-layer route's ping-pong outputs of the layers below the top
    unsigned long long *box;
    unsigned *status;
};

}  // namespace lsprnn

using namespace lsprnn;

struct lsprnn_handle {
    lsprnn_config cfg{};
    int gates = 0;
    std::vector<Slot> tensors;
    std::map<std::string, int> index;
    std::vector<size_t> o_wih, o_bias, o_bhn;            // per layer, float offsets
    std::vector<size_t> o_whh[2], o_wih_stacked;         // packed W_hh per route [stacked]; packed W_ih (stacked route, layers >= 1)
    Geometry geo[2]{};                                   // [stacked]
    size_t blob_floats = 0;
    const float *blob = nullptr;
    float *ws = nullptr;
    bool boxes_clean = false;
    Fit fit[2][2];               // [family][stacked]
    int fit_device = -1;         // the device the cached residency answers belong to
    unsigned epoch = 0;
    void add(const std::string &k, size_t n) { Slot s; s.key = k; s.numel = n; index[k] = (int)tensors.size(); tensors.push_back(std::move(s)); }
    const std::vector<float> &T(const std::string &k) const { return tensors[index.at(k)].data; }
    int in_size(int l) const { return l == 0 ? cfg.input_size : cfg.hidden_size; }
    size_t xproj_floats() const { return align64((size_t)cfg.max_steps * gates * cfg.hidden_size); }
    size_t hseq_floats() const { return align64((size_t)cfg.max_steps * cfg.hidden_size); }
    size_t box_bytes() const { return (size_t)cfg.num_layers * cfg.max_steps * cfg.hidden_size * 8; }
    int blocks(bool stacked) const { return (stacked ? cfg.num_layers : 1) * geo[stacked].G; }     // polling workgroups of one launch
};

namespace lsprnn {

static Workspace carve(const lsprnn_handle *h)
{
    Workspace w;
    w.xproj = h->ws; w.hs[0] = w.xproj + h->xproj_floats(); w.hs[1] = w.hs[0] + h->hseq_floats();
    char *tail = reinterpret_cast<char *>(w.hs[1] + h->hseq_floats());
    w.box = reinterpret_cast<unsigned long long *>(tail);
    w.status = reinterpret_cast<unsigned *>(tail + h->box_bytes());
    return w;
}

static int clear_status_and_boxes(lsprnn_handle *h, const Workspace &w, hipStream_t s)
{
    if (hipMemsetAsync(w.status, 0, 64, s) != hipSuccess) return fail(LSPRNN_ERR_HIP, "hipMemsetAsync(status)");
    if (!h->boxes_clean) {   // tags are launch counters: earlier launches never match; clear what the buffer held when bound
        const hipError_t e = hipMemsetAsync(w.box, 0, h->box_bytes(), s);
        if (e != hipSuccess) return hipfail(e, "hipMemsetAsync(mailboxes)");
        h->boxes_clean = true;
    }
    return LSPRNN_OK;
}

template <bool STACKED> static const void *single_kernel(int gates, int H)
{
    constexpr int CPP = STACKED ? 16 : 32, PW = 512 / CPP, PN = 256 / CPP;
    void (*k)(WaveParams) = gates == 3 ? (H == 512 ? rnn_wave<3, PW, CPP, STACKED> : rnn_wave<3, PN, CPP, STACKED>)
                                       : (H == 512 ? rnn_wave<4, PW, CPP, STACKED> : rnn_wave<4, PN, CPP, STACKED>);
    return reinterpret_cast<const void *>(k);
}
template <bool STACKED> static const void *multi_kernel(int gates, int H)
{
    constexpr int CPP = STACKED ? 16 : 32, PW = 512 / CPP, PN = 256 / CPP;
    void (*k)(WaveMultiParams) = gates == 3 ? (H == 512 ? rnn_wave_multi<3, PW, CPP, STACKED> : rnn_wave_multi<3, PN, CPP, STACKED>)
                                            : (H == 512 ? rnn_wave_multi<4, PW, CPP, STACKED> : rnn_wave_multi<4, PN, CPP, STACKED>);
    return reinterpret_cast<const void *>(k);
}
static const void *kernel_of(const lsprnn_handle *h, int family, bool stacked)
{
    const int GT = h->gates, H = h->cfg.hidden_size;
    if (family == SINGLE) return stacked ? single_kernel<true>(GT, H) : single_kernel<false>(GT, H);
    return stacked ? multi_kernel<true>(GT, H) : multi_kernel<false>(GT, H);
}

// dynamic LDS of rnn_wave_multi for S sequences: hown (and, stacked, hlow) [S][H], cst [S][U], xs [S][GATES][U]
static size_t multi_lds_bytes(const lsprnn_handle *h, int S, bool stacked)
{
    return (size_t)S * ((stacked ? 2 : 1) * h->cfg.hidden_size + (h->gates + 1) * h->geo[stacked].U) * sizeof(float);
}

// Do the polling workgroups of one launch of this family and route fit the device at once?  Cached per handle AND device.  The multi family
// is asked at the LDS of a full call (LSPRNN_MAX_SEQUENCES sequences), so the route does not depend on nseq.
static int resident(lsprnn_handle *h, int family, bool stacked, bool *fits)
{
    int dev = -1;
    (void)hipGetDevice(&dev);
    if (dev != h->fit_device) {
        h->fit_device = dev;
        for (auto &family_fits : h->fit)
            for (Fit &f : family_fits) f = Fit{};
    }
    Fit &f = h->fit[family][stacked];
    if (!f.checked) {
        const void *kern = kernel_of(h, family, stacked);
        const std::string name = kernel_name[family];
        const size_t lds = family == MULTI ? multi_lds_bytes(h, LSPRNN_MAX_SEQUENCES, stacked) : 0;
        if (lds) {
            const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return hipfail(e, ("hipFuncSetAttribute(" + name + ")").c_str());
        }
        const hipError_t e = lspgemm::fits_resident(kern, NT, lds, h->blocks(stacked), &f.fits);
        if (e != hipSuccess) return hipfail(e, ("occupancy query (" + name + ")").c_str());
        f.checked = true;
    }
    *fits = f.fits;
    return LSPRNN_OK;
}

// Route: stacks run stacked (all layers in one launch, L * G workgroups polling each other) unless LSPRNN_FLAG_PER_LAYER asks for one launch
// per layer (G polling workgroups) -- or the device cannot hold the stack at once (a partitioned or small device): then the per-layer
// route is taken silently.
static int choose_route(lsprnn_handle *h, int family, bool *stacked)
{
    bool fits = false;
    *stacked = (h->cfg.flags & LSPRNN_FLAG_PER_LAYER) ? false : h->cfg.num_layers > 1;
    if (*stacked) {
        if (const int rc = resident(h, family, true, &fits)) return rc;
        if (fits) return LSPRNN_OK;
        *stacked = false;
    }
    if (const int rc = resident(h, family, false, &fits)) return rc;
    if (!fits)
        return fail(LSPRNN_ERR_UNSUPPORTED, std::string(kernel_name[family]) + ", one launch per layer: the G = H / U polling workgroups of a layer (16 or 4) do not fit "
                                            "this device at once -- the recurrent kernels need at least that many free workgroup slots (include/lsprnn.h)");
    return LSPRNN_OK;
}

// the parameter block both families share, for one launch: the whole stack, or layer `layer` alone writing `out`
static StackParams stack_params(lsprnn_handle *h, const Workspace &w, bool stacked, int layer, float *out)
{
    if (++h->epoch == 0) h->epoch = 1;
    StackParams p{};
    p.blob = h->blob; p.blob_bytes = (unsigned)(h->blob_floats * sizeof(float));
    for (int l = 0; l < h->cfg.num_layers; ++l) {
        p.whh[l] = (unsigned)(h->o_whh[stacked][l] * sizeof(float)); p.wih[l] = (unsigned)(h->o_wih_stacked[l] * sizeof(float));
        p.bias[l] = h->blob + h->o_bias[l]; p.bhn[l] = h->blob + h->o_bhn[l];
    }
    p.xproj = w.xproj; p.out = out; p.hbox = w.box; p.status = w.status; p.epoch = h->epoch;
    p.H = h->cfg.hidden_size; p.layers = h->cfg.num_layers; p.layer = layer; p.wgs_per_layer = h->geo[stacked].G;
    // workgroup b runs on XCD b % 8 (observed, speed only): keep the polling workgroups on as few XCDs as their number allows -- up to 32, every
    // 8th block, so that the whole all-gather sits behind one XCD's L2 (see csrc/a2h.hip)
    const int nwg = h->blocks(stacked);
    p.stride = nwg <= 32 ? 8 : (nwg <= 64 ? 4 : (nwg <= 128 ? 2 : 1));
    return p;
}

// One forward of either family over `rows` rows of x: memsets, route, then per launch (one, or one per layer) the input-projection gemm
// and the recurrence.  `fill` completes the family's parameter struct around the shared block.
template <class Params, class Fill>
static int run_stack(lsprnn_handle *h, int family, const float *x_dev, int rows, int nseq, float *out_dev, hipStream_t s, Fill fill)
{
    const Workspace w = carve(h);
    if (const int rc = clear_status_and_boxes(h, w, s)) return rc;
    bool stacked = false;
    if (const int rc = choose_route(h, family, &stacked)) return rc;
    const void *kern = kernel_of(h, family, stacked);
    const size_t lds = family == MULTI ? multi_lds_bytes(h, nseq, stacked) : 0;
    const int H = h->cfg.hidden_size, GT = h->gates, L = h->cfg.num_layers;
    const float *in = x_dev;
    for (int l = 0; l < (stacked ? 1 : L); ++l) {
        lspgemm::GemmParams g{in, h->blob + h->o_wih[l], nullptr, h->blob + h->o_bias[l], nullptr, w.xproj, rows, GT * H, h->in_size(l), 1.0f, 0};
        hipError_t e = lspgemm::launch_gemm_f32(g, s);
        if (e != hipSuccess) return hipfail(e, "input projection gemm launch");
        float *out = stacked || l + 1 == L ? out_dev : w.hs[l & 1];
        Params p{};
        p.k = stack_params(h, w, stacked, l, out);
        fill(p);
        void *args[] = {&p};
        e = hipLaunchKernel(kern, dim3(h->blocks(stacked) * p.k.stride), dim3(NT), args, lds, s);
        if (e != hipSuccess) return hipfail(e, (std::string(kernel_name[family]) + " launch").c_str());
        in = out;
    }
    return LSPRNN_OK;
}

// one matrix [GATES*H][H] in a route's register layout: workgroup w, thread t = (unit w*U + t/P, column part t%P), gate g, float4 q of its CPP columns
static void pack_matrix(float *dst, const std::vector<float> &src, int H, int GT, const Geometry &geo)
{
    const int Q = geo.CPP / 4;
    for (int w = 0; w < geo.G; ++w)
        for (int g = 0; g < GT; ++g)
            for (int q = 0; q < Q; ++q)
                for (int t = 0; t < NT; ++t)
                    for (int e = 0; e < 4; ++e) {
                        const int row = g * H + w * geo.U + t / geo.P, col = (t % geo.P) * geo.CPP + q * 4 + e;
                        dst[((((size_t)w * GT + g) * Q + q) * NT + t) * 4 + e] = src[(size_t)row * H + col];
                    }
}

}  // namespace lsprnn

extern "C" {

const char *lsprnn_last_error(void) { return g_err.c_str(); }
int lsprnn_abi_version(void) { return LSPRNN_ABI_VERSION; }

int lsprnn_create(const lsprnn_config *cfg, lsprnn_handle **out)
{
    if (!cfg || !out) return fail(LSPRNN_ERR_INVALID_ARGUMENT, "null argument");
    if (cfg->abi_version != LSPRNN_ABI_VERSION) return fail(LSPRNN_ERR_INVALID_ARGUMENT, "abi_version mismatch");
    if (cfg->cell != LSPRNN_CELL_GRU && cfg->cell != LSPRNN_CELL_LSTM) return fail(LSPRNN_ERR_INVALID_ARGUMENT, "cell");
    if (cfg->hidden_size != 256 && cfg->hidden_size != 512)
        return fail(LSPRNN_ERR_UNSUPPORTED, "hidden_size must be 256 or 512 (the sizes the reference's GRU / LSTM stacks use)");
    if (cfg->num_layers < 1 || cfg->num_layers > 8) return fail(LSPRNN_ERR_UNSUPPORTED, "num_layers in 1..8");
    if (cfg->input_size < 4 || cfg->input_size % 4) return fail(LSPRNN_ERR_SHAPE, "input_size must be a multiple of 4");
    if (cfg->max_steps < 1 || cfg->max_steps > (1 << 20)) return fail(LSPRNN_ERR_INVALID_ARGUMENT, "max_steps");
    lsprnn_handle *h = new (std::nothrow) lsprnn_handle;
    if (!h) return fail(LSPRNN_ERR_STATE, "out of host memory");
    h->cfg = *cfg;
    h->gates = cfg->cell == LSPRNN_CELL_GRU ? 3 : 4;
    // one launch per layer: one weight matrix per thread, parts of 32 columns; stacked: two matrices per thread -> parts of 16 columns
    h->geo[0] = geometry(cfg->hidden_size, 32);
    h->geo[1] = geometry(cfg->hidden_size, 16);
    const size_t H = cfg->hidden_size, gh = (size_t)h->gates * H;
    size_t o = 0;
    auto take = [&](size_t n) { const size_t at = o; o = align64(o + n); return at; };
    for (int l = 0; l < cfg->num_layers; ++l) {
        const std::string s = "_l" + std::to_string(l);
        h->add("weight_ih" + s, gh * h->in_size(l));
        h->add("weight_hh" + s, gh * H);
        h->add("bias_ih" + s, gh);
        h->add("bias_hh" + s, gh);
        h->o_wih.push_back(take(gh * h->in_size(l)));
        h->o_bias.push_back(take(gh));
        h->o_whh[0].push_back(take(gh * H));
        h->o_bhn.push_back(take(H));
        h->o_whh[1].push_back(take(gh * H));
        h->o_wih_stacked.push_back(l ? take(gh * H) : 0);
    }
    h->blob_floats = o;
    *out = h;
    return LSPRNN_OK;
}

int lsprnn_destroy(lsprnn_handle *h) { delete h; return LSPRNN_OK; }
int lsprnn_num_tensors(const lsprnn_handle *h) { return h ? (int)h->tensors.size() : fail(LSPRNN_ERR_INVALID_ARGUMENT, "null handle"); }

int lsprnn_tensor_info(const lsprnn_handle *h, int index, const char **key, size_t *numel)
{
    if (!h || index < 0 || index >= (int)h->tensors.size()) return fail(LSPRNN_ERR_INVALID_ARGUMENT, "tensor index out of range");
    if (key) *key = h->tensors[index].key.c_str();
    if (numel) *numel = h->tensors[index].numel;
    return LSPRNN_OK;
}

int lsprnn_set_tensor(lsprnn_handle *h, const char *key, const float *host_data, size_t numel)
{
    if (!h || !key || !host_data) return fail(LSPRNN_ERR_INVALID_ARGUMENT, "null argument");
    auto it = h->index.find(key);
    if (it == h->index.end()) return fail(LSPRNN_ERR_INVALID_ARGUMENT, std::string("unknown tensor key: ") + key);
    Slot &t = h->tensors[it->second];
    if (numel != t.numel) return fail(LSPRNN_ERR_SHAPE, std::string("wrong element count for ") + key);
    t.data.assign(host_data, host_data + numel);
    t.set = true;
    return LSPRNN_OK;
}

size_t lsprnn_packed_bytes(const lsprnn_handle *h) { return h ? h->blob_floats * sizeof(float) : 0; }

int lsprnn_pack_weights(lsprnn_handle *h, void *host_dst, size_t bytes)
{
    if (!h || !host_dst) return fail(LSPRNN_ERR_INVALID_ARGUMENT, "null argument");
    if (bytes < h->blob_floats * sizeof(float)) return fail(LSPRNN_ERR_SHAPE, "destination smaller than lsprnn_packed_bytes()");
    for (const Slot &t : h->tensors)
        if (!t.set) return fail(LSPRNN_ERR_STATE, "tensor not set: " + t.key);
    float *d = static_cast<float *>(host_dst);
    std::memset(d, 0, h->blob_floats * sizeof(float));
    const int H = h->cfg.hidden_size, GT = h->gates;
    for (int l = 0; l < h->cfg.num_layers; ++l) {
        const std::string s = "_l" + std::to_string(l);
        const auto &wih = h->T("weight_ih" + s), &whh = h->T("weight_hh" + s), &bih = h->T("bias_ih" + s), &bhh = h->T("bias_hh" + s);
        std::memcpy(d + h->o_wih[l], wih.data(), wih.size() * sizeof(float));
        for (int r = 0; r < GT * H; ++r) {
            const bool gru_n = GT == 3 && r >= 2 * H;          // b_hn stays with the hidden product (inside r * (...))
            d[h->o_bias[l] + r] = gru_n ? bih[r] : bih[r] + bhh[r];
        }
        if (GT == 3) std::memcpy(d + h->o_bhn[l], bhh.data() + 2 * H, sizeof(float) * H);
        pack_matrix(d + h->o_whh[0][l], whh, H, GT, h->geo[0]);
        pack_matrix(d + h->o_whh[1][l], whh, H, GT, h->geo[1]);
        if (l) pack_matrix(d + h->o_wih_stacked[l], wih, H, GT, h->geo[1]);
    }
    return LSPRNN_OK;
}

int lsprnn_bind_weights(lsprnn_handle *h, const void *packed_dev, size_t bytes)
{
    if (!h || !packed_dev) return fail(LSPRNN_ERR_INVALID_ARGUMENT, "null argument");
    if (bytes < h->blob_floats * sizeof(float)) return fail(LSPRNN_ERR_SHAPE, "blob smaller than lsprnn_packed_bytes()");
    if ((uintptr_t)packed_dev & 15) return fail(LSPRNN_ERR_INVALID_ARGUMENT, "blob must be 16-byte aligned");
    h->blob = static_cast<const float *>(packed_dev);
    return LSPRNN_OK;
}

size_t lsprnn_workspace_bytes(const lsprnn_handle *h)
{
    if (!h) return 0;
    return (h->xproj_floats() + 2 * h->hseq_floats()) * sizeof(float) + h->box_bytes() + 256;
}

int lsprnn_bind_workspace(lsprnn_handle *h, void *workspace_dev, size_t bytes)
{
    if (!h || !workspace_dev) return fail(LSPRNN_ERR_INVALID_ARGUMENT, "null argument");
    if (bytes < lsprnn_workspace_bytes(h)) return fail(LSPRNN_ERR_SHAPE, "workspace smaller than lsprnn_workspace_bytes()");
    if ((uintptr_t)workspace_dev & 15) return fail(LSPRNN_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
    h->ws = static_cast<float *>(workspace_dev);
    h->boxes_clean = false;
    return LSPRNN_OK;
}

size_t lsprnn_state_floats(const lsprnn_handle *h)
{
    if (!h) return 0;
    return (size_t)(h->gates == 4 ? 2 : 1) * h->cfg.num_layers * h->cfg.hidden_size;
}

int lsprnn_forward(lsprnn_handle *h, const float *x_dev, int T, float *out_dev, void *stream)
{
    return lsprnn_forward_state(h, x_dev, T, out_dev, nullptr, nullptr, stream);
}

int lsprnn_forward_state(lsprnn_handle *h, const float *x_dev, int T, float *out_dev, const float *state_in_dev, float *state_out_dev,
                         void *stream)
{
    if (!h || !x_dev || !out_dev) return fail(LSPRNN_ERR_INVALID_ARGUMENT, "null argument");
    if (state_in_dev && state_in_dev == state_out_dev)
        return fail(LSPRNN_ERR_INVALID_ARGUMENT, "state_in and state_out must be separate buffers (a retried call restarts from state_in)");
    if (!h->blob) return fail(LSPRNN_ERR_STATE, "weights not bound (lsprnn_bind_weights)");
    if (!h->ws) return fail(LSPRNN_ERR_STATE, "workspace not bound (lsprnn_bind_workspace)");
    if (T < 1 || T > h->cfg.max_steps) return fail(LSPRNN_ERR_SHAPE, "T out of range (max_steps)");
    return run_stack<WaveParams>(h, SINGLE, x_dev, T, 0, out_dev, static_cast<hipStream_t>(stream),
                                 [&](WaveParams &p) { p.state_in = state_in_dev; p.state_out = state_out_dev; p.T = T; });
}

int lsprnn_forward_multi(lsprnn_handle *h, int nseq, const float *x_dev, const int *T, float *out_dev, const float *const *state_in_dev,
                         float *const *state_out_dev, void *stream)
{
    if (!h || !x_dev || !out_dev || !T) return fail(LSPRNN_ERR_INVALID_ARGUMENT, "null argument");
    if (nseq < 1 || nseq > LSPRNN_MAX_SEQUENCES) return fail(LSPRNN_ERR_SHAPE, "need 1 <= nseq <= LSPRNN_MAX_SEQUENCES");
    if (!h->blob) return fail(LSPRNN_ERR_STATE, "weights not bound (lsprnn_bind_weights)");
    if (!h->ws) return fail(LSPRNN_ERR_STATE, "workspace not bound (lsprnn_bind_workspace)");
    SeqTable q{};
    long long rows = 0;
    for (int s = 0; s < nseq; ++s) {
        if (T[s] < 0) return fail(LSPRNN_ERR_SHAPE, "sequence " + std::to_string(s) + ": T < 0");
        q.off[s] = (int)rows; q.T[s] = T[s];
        rows += T[s];
        if (rows > h->cfg.max_steps) return fail(LSPRNN_ERR_SHAPE, "the steps of all sequences together exceed max_steps (the sequences share the workspace)");
        q.state_in[s] = state_in_dev ? state_in_dev[s] : nullptr;
        q.state_out[s] = state_out_dev ? state_out_dev[s] : nullptr;
        if (T[s] > q.Tmax) q.Tmax = T[s];
    }
    // a state-out buffer is written while other sequences may still read their state-in: no buffer may be both, in any pairing
    for (int s = 0; s < nseq; ++s)
        for (int r = 0; r < nseq; ++r) {
            if (q.state_out[s] && q.state_out[s] == q.state_in[r])
                return fail(LSPRNN_ERR_INVALID_ARGUMENT, "sequence " + std::to_string(s) + ": state_out is the state_in of sequence " + std::to_string(r) +
                                                         " (state_in and state_out must be separate buffers: a retried call restarts from state_in)");
            if (r != s && q.state_out[s] && q.state_out[s] == q.state_out[r])
                return fail(LSPRNN_ERR_INVALID_ARGUMENT, "sequences " + std::to_string(s) + " and " + std::to_string(r) + " share a state_out buffer");
        }
    q.S = nseq; q.rows = (int)rows;
    if (rows == 0) return LSPRNN_OK;                          // nothing to do: no sequence is touched
    return run_stack<WaveMultiParams>(h, MULTI, x_dev, (int)rows, nseq, out_dev, static_cast<hipStream_t>(stream), [&](WaveMultiParams &p) { p.q = q; });
}

int lsprnn_status(lsprnn_handle *h, void *stream, uint32_t *code)
{
    if (!h || !code) return fail(LSPRNN_ERR_INVALID_ARGUMENT, "null argument");
    if (!h->ws) return fail(LSPRNN_ERR_STATE, "workspace not bound");
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hipfail(e, "hipStreamSynchronize");
    e = hipMemcpy(code, carve(h).status, sizeof(uint32_t), hipMemcpyDeviceToHost);
    return e == hipSuccess ? LSPRNN_OK : hipfail(e, "hipMemcpy(status)");
}

int lsprnn_linear(const float *x_dev, const float *w_dev, const float *scale_dev, const float *shift_dev, float *y_dev,
                  int M, int N, int K, int leaky, void *stream)
{
    if (!x_dev || !w_dev || !shift_dev || !y_dev) return fail(LSPRNN_ERR_INVALID_ARGUMENT, "null argument");
    if (M < 1 || N < 1 || K < 4 || K % 4) return fail(LSPRNN_ERR_SHAPE, "need M, N >= 1 and K a multiple of 4");
    lspgemm::GemmParams g{x_dev, w_dev, scale_dev, shift_dev, nullptr, y_dev, M, N, K, 1.0f, leaky};
    const hipError_t e = lspgemm::launch_gemm_f32(g, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? LSPRNN_OK : hipfail(e, "linear gemm launch");
}

}  // extern "C"
