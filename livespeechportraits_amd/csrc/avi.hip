// avi.hip -- 'movi' fragments of Motion-JPEG AVI files, assembled on the device (include/lspavi.h).
//
// A batch of encoded frames is split into runs, one fragment per run (lspavi_pack: the one run that covers the batch).  The run table travels
// as kernel arguments.  Two launches per batch, whatever the content and the number of runs:
//   avi_layout  one wavefront: lane k owns frame k and finds its run in the table.  Chunk lengths (audio span of the frame, header + the
//               encoder's byte count), their padded sizes scanned across the wavefront, segmented by run; a run's fragment starts at the sum of
//               the 16-byte-rounded lengths of the runs before it.  Then the table of chunk offsets / lengths / owners and the frames' first
//               samples (workspace), the index entries and the status block.  Offsets in the workspace table are absolute (gather), those in
//               the index relative to the fragment (the file).
//   avi_gather  gather form: one lane owns an aligned 16-byte piece of the OUTPUT.  It binary-searches the offset table (a copy in LDS) for
//               the chunk the piece starts in.  A piece that lies inside one source segment (JPEG header, entropy-coded bytes, audio) is read
//               as aligned dwords and funnel-shifted into place; a piece that touches a seam (chunk header, pad byte, header -> scan, the
//               fragment's end, the end of an audio ring) is selected byte by byte.  One 16-byte store per piece.  Fragments start on 16-byte
//               boundaries, so a piece belongs to one fragment; the partial piece at a fragment's end is stored as its dwords and an even byte
//               tail, so nothing between a fragment's end and the next fragment, or above the last one, is written.
// Every output byte has exactly one writer, so the result does not depend on what the buffer held, and there is nothing to zero and no atomic.
// The kernel moves ~150 KB per batch of 8 frames of 512 x 512: it is latency-bound, and what is being bought is the single copy to the host.
#include "../../include/lspavi.h"

#include <hip/hip_runtime.h>

#include <string>

namespace lspavi {

constexpr int TAB = 2 * LSPAVI_MAX_BATCH + 8;       // table stride: 2 * 64 chunks + the end offset, rounded up
constexpr int NT = 256;                             // lanes per workgroup of avi_gather
constexpr int MAX_BLOCKS = 256;                     // avi_gather strides over the pieces: 1 MiB per pass
constexpr uint32_t FCC_VIDEO = 0x63643030u;         // '00dc'
constexpr uint32_t FCC_AUDIO = 0x62773130u;         // '01wb'

struct Run {
    const float *ring;              // stream sample i at ring[i % ring_samples]
    long long frame0, sample0;
    unsigned long long ring_samples;
    int first, count, fmt;
};

struct Params {
    const unsigned char *hdr, *slab;    // JPEG header, hlen bytes; [batch][cap]
    const uint32_t *sizes;              // [batch]
    unsigned char *out;
    uint32_t *index;                // [nch][4]
    uint32_t *status;               // [nruns][LSPAVI_STATUS_WORDS]; compact: [4], lspavi_pack's block for its one run
    uint32_t *tab;                  // [0] chunk count; [4 + TAB * {0,1,2}]: chunk offsets (+ the end), lengths, frame | video << 8 | run << 16;
                                    // then [batch] ring position of a frame's first sample, [nruns] fragment ends
    unsigned long long cap;
    int hlen, batch, nruns, rate, fps, compact;
    Run run[LSPAVI_MAX_STREAMS];
};

constexpr size_t WORKSPACE_BYTES = (4 + 3 * TAB + LSPAVI_MAX_BATCH + LSPAVI_MAX_STREAMS) * sizeof(uint32_t);

__global__ __launch_bounds__(64) void avi_layout(Params p)
{
    const int k = threadIdx.x;
    const bool on = k < p.batch;
    int j = 0;
    for (int i = 1; i < p.nruns; ++i)
        if (k >= p.run[i].first) j = i;                         // runs are ascending and cover the batch
    const Run &r = p.run[j];
    const int first = r.first;
    const bool au = on && r.fmt != LSPAVI_AUDIO_NONE;
    const uint32_t bps = r.fmt == LSPAVI_AUDIO_F32 ? 4u : 2u;
    uint32_t pos = 0, alen = 0, vlen = 0;
    if (on) {
        if (au) {
            const unsigned long long rate = static_cast<unsigned long long>(p.rate), fps = static_cast<unsigned long long>(p.fps);
            const unsigned long long f = static_cast<unsigned long long>(r.frame0 + (k - first));
            const unsigned long long s0 = f * rate / fps, s1 = (f + 1) * rate / fps;
            alen = static_cast<uint32_t>(s1 - s0) * bps;        // 2 or 4 bytes per sample: always even
            pos = static_cast<uint32_t>((static_cast<unsigned long long>(r.sample0) + s0) % r.ring_samples);
        }
        uint32_t sz = p.sizes[k];
        if (sz > p.cap) sz = static_cast<uint32_t>(p.cap);      // never true for what lspjpeg_encode wrote: keeps every read inside the slab
        vlen = static_cast<uint32_t>(p.hlen) + sz;
    }
    const uint32_t apad = au ? 8u + alen : 0u;
    const uint32_t vpad = on ? 8u + vlen + (vlen & 1u) : 0u;
    const uint32_t mine = apad + vpad, nmine = on ? (au ? 2u : 1u) : 0u;
    uint32_t inc = mine, vmax = vlen, amax = alen, cinc = nmine, rinc = nmine;
    for (int d = 1; d < 64; d <<= 1) {                          // inclusive scans: bytes, maxima and chunks inside the run, chunks of the batch
        const uint32_t t = __shfl_up(inc, d, 64), tv = __shfl_up(vmax, d, 64), ta = __shfl_up(amax, d, 64);
        const uint32_t tc = __shfl_up(cinc, d, 64), tr = __shfl_up(rinc, d, 64);
        if (k >= d) cinc += tc;
        if (k - d >= first) {
            inc += t;
            rinc += tr;
            vmax = max(vmax, tv);
            amax = max(amax, ta);
        }
    }
    uint32_t base = 0;                                          // every lane takes part in the shuffles
    for (int i = 0; i < p.nruns; ++i) {
        const uint32_t bytes = __shfl(inc, p.run[i].first + p.run[i].count - 1, 64);
        if (i < j) base += (bytes + 15u) & ~15u;
    }
    if (!on) return;
    const uint32_t start = inc - mine;                          // relative to the fragment
    uint32_t c = cinc - nmine;
    uint32_t *off = p.tab + 4, *len = off + TAB, *info = len + TAB, *smp = info + TAB, *end = smp + LSPAVI_MAX_BATCH;
    smp[k] = pos;
    if (au) {
        off[c] = base + start;
        len[c] = alen;
        info[c] = static_cast<uint32_t>(k) | (static_cast<uint32_t>(j) << 16);
        *reinterpret_cast<uint4 *>(p.index + 4 * c) = make_uint4(FCC_AUDIO, 0x10u, start, alen);
        ++c;
    }
    off[c] = base + start + apad;
    len[c] = vlen;
    info[c] = static_cast<uint32_t>(k) | 0x100u | (static_cast<uint32_t>(j) << 16);
    *reinterpret_cast<uint4 *>(p.index + 4 * c) = make_uint4(FCC_VIDEO, 0x10u, start + apad, vlen);
    if (k == first + r.count - 1) {
        end[j] = base + inc;
        uint4 *st = reinterpret_cast<uint4 *>(p.status + LSPAVI_STATUS_WORDS * j);
        if (p.compact) {                                        // one run at offset 0, its index rows from row 0
            st[0] = make_uint4(inc, rinc, vmax, amax);
        } else {
            st[0] = make_uint4(base, inc, rinc, vmax);
            st[1] = make_uint4(amax, c + 1 - rinc, 0u, 0u);
        }
        if (k == p.batch - 1) {
            off[c + 1] = base + inc;
            p.tab[0] = c + 1;
        }
    }
}

__device__ inline uint32_t pcm16(float x)
{
    float v = rintf(x * 32767.0f);
    if (!(v == v)) return 0u;
    v = fminf(fmaxf(v, -32767.0f), 32767.0f);
    return static_cast<uint32_t>(static_cast<int>(v)) & 0xFFFFu;
}

// 16 bytes from base + off, base 4-byte aligned: aligned dwords, funnel-shifted.  Every dword read holds at least one byte of the 16.
__device__ inline uint4 load16(const unsigned char *base, size_t off)
{
    const uint32_t *a = reinterpret_cast<const uint32_t *>(base + (off & ~static_cast<size_t>(3)));
    const unsigned sh = static_cast<unsigned>(off & 3) * 8;
    const uint32_t w0 = a[0], w1 = a[1], w2 = a[2], w3 = a[3];
    if (sh == 0) return make_uint4(w0, w1, w2, w3);
    const uint32_t w4 = a[4];
    const unsigned up = 32 - sh;
    return make_uint4((w0 >> sh) | (w1 << up), (w1 >> sh) | (w2 << up), (w2 >> sh) | (w3 << up), (w3 >> sh) | (w4 << up));
}

__global__ __launch_bounds__(NT) void avi_gather(Params p)
{
    __shared__ uint32_t s_off[TAB], s_len[TAB], s_info[TAB], s_smp[LSPAVI_MAX_BATCH], s_end[LSPAVI_MAX_STREAMS];
    const int nch = static_cast<int>(p.tab[0]);
    {
        const uint32_t *off = p.tab + 4, *len = off + TAB, *info = len + TAB, *smp = info + TAB, *end = smp + LSPAVI_MAX_BATCH;
        for (int i = threadIdx.x; i <= nch; i += NT) {
            s_off[i] = off[i];
            if (i < nch) {
                s_len[i] = len[i];
                s_info[i] = info[i];
            }
            if (i < p.batch) s_smp[i] = smp[i];
            if (i < p.nruns) s_end[i] = end[i];
        }
    }
    __syncthreads();
    const uint32_t npiece = (s_off[nch] + 15u) >> 4;
    const uint32_t hlen = static_cast<uint32_t>(p.hlen);

    // one byte of chunk c at offset o of the chunk (header included)
    auto byte_at = [&](int c, uint32_t o) -> uint32_t {
        const uint32_t info = s_info[c], len = s_len[c];
        const bool video = info & 0x100u;
        const int k = info & 0xFFu;
        if (o < 4) return ((video ? FCC_VIDEO : FCC_AUDIO) >> (8 * o)) & 0xFFu;
        if (o < 8) return (len >> (8 * (o - 4))) & 0xFFu;
        const uint32_t q = o - 8;
        if (q >= len) return 0u;                                                        // the pad byte
        if (video) return q < hlen ? p.hdr[q] : p.slab[static_cast<size_t>(k) * p.cap + (q - hlen)];
        const Run &r = p.run[info >> 16];
        const bool f32 = r.fmt == LSPAVI_AUDIO_F32;
        unsigned long long s = static_cast<unsigned long long>(s_smp[k]) + (f32 ? q >> 2 : q >> 1);
        if (s >= r.ring_samples) s -= r.ring_samples;                                   // a run's span is no longer than the ring
        if (f32) return reinterpret_cast<const unsigned char *>(r.ring + s)[q & 3u];
        return (pcm16(r.ring[s]) >> (8 * (q & 1))) & 0xFFu;
    };

    for (uint32_t piece = blockIdx.x * NT + threadIdx.x; piece < npiece; piece += gridDim.x * NT) {
        const uint32_t pos = piece << 4;
        int lo = 0, hi = nch - 1;
        while (lo < hi) {                                                               // the last chunk that starts at or before pos
            const int mid = (lo + hi + 1) >> 1;
            if (s_off[mid] <= pos) lo = mid; else hi = mid - 1;
        }
        const int c = lo;
        const uint32_t info = s_info[c];
        const uint32_t total = s_end[info >> 16];                                       // the end of this piece's fragment
        if (pos >= total) continue;                                                     // never: fragments start 16-byte aligned
        const uint32_t o = pos - s_off[c], len = s_len[c];
        const bool video = info & 0x100u;
        const int k = info & 0xFFu;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        bool done = false;
        if (o >= 8 && o + 16 <= 8 + len) {                                              // all 16 bytes are payload of this chunk
            const uint32_t q = o - 8;
            if (video) {
                if (q + 16 <= hlen) {
                    v = load16(p.hdr, q);
                    done = true;
                } else if (q >= hlen) {
                    v = load16(p.slab, static_cast<size_t>(k) * p.cap + (q - hlen));
                    done = true;
                }
            } else {
                const Run &r = p.run[info >> 16];
                const unsigned long long ring_bytes = r.ring_samples * 4;
                if (r.fmt == LSPAVI_AUDIO_F32) {
                    unsigned long long b = static_cast<unsigned long long>(s_smp[k]) * 4 + q;
                    if (b >= ring_bytes) b -= ring_bytes;
                    if (b + 16 <= ring_bytes) {                                         // else the ring's end falls inside the piece: a seam
                        v = load16(reinterpret_cast<const unsigned char *>(r.ring), static_cast<size_t>(b));
                        done = true;
                    }
                } else {                                                                // chunk starts are even, so q is: 8 whole samples
                    unsigned long long s = static_cast<unsigned long long>(s_smp[k]) + (q >> 1);
                    if (s >= r.ring_samples) s -= r.ring_samples;
                    if (s + 8 <= r.ring_samples) {
                        const float *w = r.ring + s;
                        v = make_uint4(pcm16(w[0]) | (pcm16(w[1]) << 16), pcm16(w[2]) | (pcm16(w[3]) << 16),
                                       pcm16(w[4]) | (pcm16(w[5]) << 16), pcm16(w[6]) | (pcm16(w[7]) << 16));
                        done = true;
                    }
                }
            }
        }
        if (!done) {                                                                    // a seam: byte by byte, over the chunks it touches
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            int cc = c;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t b = pos + j;
                if (b < total) {
                    while (b >= s_off[cc + 1]) ++cc;
                    w[j >> 2] |= byte_at(cc, b - s_off[cc]) << (8 * (j & 3));
                }
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        if (pos + 16 <= total) {
            *reinterpret_cast<uint4 *>(p.out + pos) = v;
        } else {                                                                        // the fragment's end: total is even, so 2..14 bytes
            const uint32_t r = total - pos;
            uint32_t *o32 = reinterpret_cast<uint32_t *>(p.out + pos);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const uint32_t nd = r >> 2;
            for (uint32_t j = 0; j < nd; ++j) o32[j] = w[j];
            if (r & 2u) *reinterpret_cast<unsigned short *>(p.out + pos + 4 * nd) = static_cast<unsigned short>(w[nd] & 0xFFFFu);
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

static bool format_ok(int f) { return f == LSPAVI_AUDIO_NONE || f == LSPAVI_AUDIO_S16 || f == LSPAVI_AUDIO_F32; }

static bool misaligned(const void *ptr, unsigned n) { return reinterpret_cast<uintptr_t>(ptr) % n != 0; }

// What both entry points ask of their buffers.  `need`: the entry point's own lspavi_capacity_bytes*(...); `wave`: lspavi_pack's waveform.
static int check_buffers(bool multi, const unsigned char *hdr, const unsigned char *slab, const uint32_t *sizes, int batch, const float *wave,
                         size_t need, const unsigned char *out, size_t out_capacity, const uint32_t *index, const uint32_t *status,
                         const void *workspace, size_t workspace_bytes)
{
    if (!hdr || !slab || !sizes || !out || !index || !status || !workspace) return fail(LSPAVI_ERR_INVALID_ARGUMENT, "null argument");
    if (batch < 1 || batch > LSPAVI_MAX_BATCH) return fail(LSPAVI_ERR_INVALID_ARGUMENT, "batch must be in 1..64");
    if (need == 0) return fail(LSPAVI_ERR_INVALID_ARGUMENT, "jpeg_header_len, jpeg_capacity, rate or fps out of range");
    if (need > 0xFFFFFFF0u)
        return fail(LSPAVI_ERR_UNSUPPORTED, (multi ? "fragments of " : "a fragment of ") + std::to_string(need) + (multi ? " bytes pass" : " bytes passes") +
                                                " 32-bit offsets");
    if (out_capacity < need) return fail(LSPAVI_ERR_INVALID_ARGUMENT, "out_dev needs " + std::to_string(need) + " bytes");
    if (workspace_bytes < WORKSPACE_BYTES) return fail(LSPAVI_ERR_INVALID_ARGUMENT, "workspace needs " + std::to_string(WORKSPACE_BYTES) + " bytes");
    if (misaligned(out, 16) || misaligned(index, 16) || misaligned(status, 16) || misaligned(workspace, 16))
        return fail(LSPAVI_ERR_INVALID_ARGUMENT, "out_dev, index_dev, status_dev and workspace_dev must be 16-byte aligned");
    if (misaligned(hdr, 4) || misaligned(slab, 4) || misaligned(wave, 4))
        return fail(LSPAVI_ERR_INVALID_ARGUMENT, multi ? "jpeg_header_dev and jpeg_dev must be 4-byte aligned"
                                                       : "jpeg_header_dev, jpeg_dev and wave_dev must be 4-byte aligned");
    return LSPAVI_OK;
}

// everything of Params but the run table
static Params params(const unsigned char *hdr, int hlen, const unsigned char *slab, size_t cap, const uint32_t *sizes, int batch, int nruns, int rate,
                     int fps, unsigned char *out, uint32_t *index, uint32_t *status, bool compact, void *workspace)
{
    Params p{};
    p.hdr = hdr;
    p.slab = slab;
    p.sizes = sizes;
    p.out = out;
    p.index = index;
    p.status = status;
    p.tab = static_cast<uint32_t *>(workspace);
    p.cap = cap;
    p.hlen = hlen;
    p.batch = batch;
    p.nruns = nruns;
    p.rate = rate;
    p.fps = fps;
    p.compact = compact;
    return p;
}

static int launch(const Params &p, size_t need, void *hip_stream)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    size_t blocks = (need / 16 + NT - 1) / NT;
    if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
    hipLaunchKernelGGL(avi_layout, dim3(1), dim3(64), 0, st, p);
    hipLaunchKernelGGL(avi_gather, dim3(static_cast<unsigned>(blocks)), dim3(NT), 0, st, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LSPAVI_ERR_HIP, std::string("avi launch: ") + hipGetErrorString(e));
    return LSPAVI_OK;
}

}  // namespace lspavi

using namespace lspavi;

extern "C" {

const char *lspavi_last_error(void) { return g_err.c_str(); }

size_t lspavi_capacity_bytes(int jpeg_header_len, size_t jpeg_capacity, int batch, int audio_format, int rate, int fps)
{
    if (jpeg_header_len < 2 || jpeg_header_len > 65536 || jpeg_capacity < 2 || jpeg_capacity > (size_t)1 << 31 || batch < 1 ||
        batch > LSPAVI_MAX_BATCH || !format_ok(audio_format) || rate < 1 || fps < 1 || rate > 1 << 24 || fps > 1 << 16)
        return 0;
    size_t n = static_cast<size_t>(batch) * (8 + static_cast<size_t>(jpeg_header_len) + jpeg_capacity + 1);
    if (audio_format != LSPAVI_AUDIO_NONE)
        n += static_cast<size_t>(batch) * 8 +
             (static_cast<size_t>(batch) * rate / fps + 1) * (audio_format == LSPAVI_AUDIO_F32 ? 4 : 2);
    return (n + 15) & ~static_cast<size_t>(15);
}

size_t lspavi_workspace_bytes(int batch) { return batch >= 1 && batch <= LSPAVI_MAX_BATCH ? WORKSPACE_BYTES : 0; }

int lspavi_pack(const unsigned char *jpeg_header_dev, int jpeg_header_len, const unsigned char *jpeg_dev, size_t jpeg_capacity,
                const uint32_t *sizes_dev, int batch, const float *wave_dev, int64_t wave_samples, int64_t frame0, int rate, int fps,
                int audio_format, unsigned char *out_dev, size_t out_capacity, uint32_t *index_dev, uint32_t *status_dev,
                void *workspace_dev, size_t workspace_bytes, void *hip_stream)
{
    if (!format_ok(audio_format)) return fail(LSPAVI_ERR_INVALID_ARGUMENT, "audio_format must be 0 (none), 1 (s16) or 3 (f32)");
    if ((wave_dev != nullptr) != (audio_format != LSPAVI_AUDIO_NONE))
        return fail(LSPAVI_ERR_INVALID_ARGUMENT, "a waveform needs an audio format, and an audio format a waveform");
    const size_t need = lspavi_capacity_bytes(jpeg_header_len, jpeg_capacity, batch, audio_format, rate, fps);
    if (const int rc = check_buffers(false, jpeg_header_dev, jpeg_dev, sizes_dev, batch, wave_dev, need, out_dev, out_capacity, index_dev, status_dev,
                                     workspace_dev, workspace_bytes))
        return rc;
    if (frame0 < 0 || frame0 > ((int64_t)1 << 31)) return fail(LSPAVI_ERR_INVALID_ARGUMENT, "frame0 must be in 0..2^31");
    if (wave_dev) {
        const int64_t last = (frame0 + batch) * rate / fps;
        if (wave_samples < 0 || wave_samples > ((int64_t)1 << 31))
            return fail(LSPAVI_ERR_INVALID_ARGUMENT, "wave_samples must be in 0..2^31");
        if (last > wave_samples)
            return fail(LSPAVI_ERR_INVALID_ARGUMENT, "frames " + std::to_string(frame0) + ".." + std::to_string(frame0 + batch - 1) +
                                                         " need " + std::to_string(last) + " samples, the waveform has " +
                                                         std::to_string(wave_samples));
    }
    Params p = params(jpeg_header_dev, jpeg_header_len, jpeg_dev, jpeg_capacity, sizes_dev, batch, 1, rate, fps, out_dev, index_dev, status_dev, true,
                      workspace_dev);
    // The clip is one run over the whole batch whose ring is the waveform itself: stream sample i at wave_dev[i], available [0, wave_samples).
    // Every sample the run needs lies below wave_samples (checked above), so no position reaches ring_samples and the kernels never take
    // their wrap branches.  ring_samples is at least 1 because avi_layout takes a position modulo it, also for a chunk of no samples.
    Run &d = p.run[0];
    d.first = 0;
    d.count = batch;
    d.fmt = audio_format;
    d.frame0 = frame0;
    d.ring = wave_dev;
    d.ring_samples = wave_dev && wave_samples > 0 ? static_cast<unsigned long long>(wave_samples) : 1;
    d.sample0 = 0;
    return launch(p, need, hip_stream);
}

size_t lspavi_capacity_bytes_multi(int jpeg_header_len, size_t jpeg_capacity, int batch, int runs, int rate, int fps)
{
    const size_t one = lspavi_capacity_bytes(jpeg_header_len, jpeg_capacity, batch, LSPAVI_AUDIO_F32, rate, fps);
    if (one == 0 || runs < 1 || runs > LSPAVI_MAX_STREAMS || runs > batch) return 0;
    return one + ((static_cast<size_t>(runs) * 20 + 15) & ~static_cast<size_t>(15));
}

size_t lspavi_workspace_bytes_multi(int batch) { return lspavi_workspace_bytes(batch); }

int lspavi_pack_multi(const unsigned char *jpeg_header_dev, int jpeg_header_len, const unsigned char *jpeg_dev, size_t jpeg_capacity,
                      const uint32_t *sizes_dev, int batch, const lspavi_run *runs, int nruns, int rate, int fps, unsigned char *out_dev,
                      size_t out_capacity, uint32_t *index_dev, uint32_t *status_dev, void *workspace_dev, size_t workspace_bytes,
                      void *hip_stream)
{
    if (!runs) return fail(LSPAVI_ERR_INVALID_ARGUMENT, "null argument");
    if (nruns < 1 || nruns > LSPAVI_MAX_STREAMS) return fail(LSPAVI_ERR_INVALID_ARGUMENT, "the batch must be split into 1..16 runs");
    const size_t need = lspavi_capacity_bytes_multi(jpeg_header_len, jpeg_capacity, batch, nruns <= batch ? nruns : 1, rate, fps);
    if (const int rc = check_buffers(true, jpeg_header_dev, jpeg_dev, sizes_dev, batch, nullptr, need, out_dev, out_capacity, index_dev, status_dev,
                                     workspace_dev, workspace_bytes))
        return rc;
    Params p = params(jpeg_header_dev, jpeg_header_len, jpeg_dev, jpeg_capacity, sizes_dev, batch, nruns, rate, fps, out_dev, index_dev, status_dev, false,
                      workspace_dev);
    int next = 0;
    for (int j = 0; j < nruns; ++j) {
        const lspavi_run &r = runs[j];
        const std::string who = "run " + std::to_string(j) + ": ";
        if (r.count < 1) return fail(LSPAVI_ERR_INVALID_ARGUMENT, who + "count must be >= 1");
        if (r.first != next || r.count > batch - next)
            return fail(LSPAVI_ERR_INVALID_ARGUMENT, who + "runs must be ascending and cover the batch (frames " + std::to_string(r.first) + ".." +
                                                         std::to_string(static_cast<long long>(r.first) + r.count - 1) + ", expected to start at " +
                                                         std::to_string(next) + " of " + std::to_string(batch) + ")");
        next += r.count;
        if (!format_ok(r.audio_format)) return fail(LSPAVI_ERR_INVALID_ARGUMENT, who + "audio_format must be 0 (none), 1 (s16) or 3 (f32)");
        if (r.frame0 < 0 || r.frame0 > ((int64_t)1 << 31)) return fail(LSPAVI_ERR_INVALID_ARGUMENT, who + "frame0 must be in 0..2^31");
        Run &d = p.run[j];
        d.first = r.first;
        d.count = r.count;
        d.fmt = r.audio_format;
        d.frame0 = r.frame0;
        d.ring_samples = 1;
        if (r.audio_format == LSPAVI_AUDIO_NONE) continue;
        if (!r.ring_dev || reinterpret_cast<uintptr_t>(r.ring_dev) % 4)
            return fail(LSPAVI_ERR_INVALID_ARGUMENT, who + "an audio format needs a ring, 4-byte aligned");
        if (r.ring_samples < 1 || r.ring_samples > ((int64_t)1 << 31)) return fail(LSPAVI_ERR_INVALID_ARGUMENT, who + "ring_samples must be in 1..2^31");
        if (r.sample0 < 0 || r.sample0 > ((int64_t)1 << 48)) return fail(LSPAVI_ERR_INVALID_ARGUMENT, who + "sample0 must be in 0..2^48");
        if (r.avail_begin < 0 || r.avail_end < r.avail_begin || r.avail_end - r.avail_begin > r.ring_samples)
            return fail(LSPAVI_ERR_INVALID_ARGUMENT, who + "the ring cannot hold samples " + std::to_string(r.avail_begin) + ".." + std::to_string(r.avail_end));
        const int64_t a = r.sample0 + r.frame0 * rate / fps, b = r.sample0 + (r.frame0 + r.count) * rate / fps;
        if (a < r.avail_begin || b > r.avail_end || b - a > r.ring_samples)
            return fail(LSPAVI_ERR_INVALID_ARGUMENT, who + "frames " + std::to_string(r.frame0) + ".." + std::to_string(r.frame0 + r.count - 1) +
                                                         " need samples " + std::to_string(a) + ".." + std::to_string(b) + ", the ring holds " +
                                                         std::to_string(r.avail_begin) + ".." + std::to_string(r.avail_end));
        d.ring = r.ring_dev;
        d.ring_samples = static_cast<unsigned long long>(r.ring_samples);
        d.sample0 = r.sample0;
    }
    if (next != batch)
        return fail(LSPAVI_ERR_INVALID_ARGUMENT, "the runs cover " + std::to_string(next) + " frames of a batch of " + std::to_string(batch));
    return launch(p, need, hip_stream);
}

}  // extern "C"
