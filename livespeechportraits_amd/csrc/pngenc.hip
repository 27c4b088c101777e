// pngenc.hip -- the PNG encoder of include/lsppngenc.h: four launches on the device (filter, deflate, scan, gather).  The filters, the chunk encoder
// and the sums live in pngenc_core.h, which also builds for the host alone and runs under sanitizers (make check-pngenc).
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/lsppngenc.h"
#include "pngenc_core.h"

static_assert(LSPPNG_ENC_CHUNK == lsppngenc::kChunk && LSPPNG_ENC_HEADER_BYTES == lsppngenc::kHeaderBytes, "the constants of lsppngenc.h");
static_assert(sizeof(lsppngenc::ChunkMem) <= 144 * 1024, "one chunk's working memory fits the LDS of a CU (160 KiB) with room to spare");

namespace {

using namespace lsppngenc;

thread_local std::string g_err;
int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Params {
    const unsigned char *src;               // [batch][H][W][C]
    unsigned char *lines;                   // [batch][line_stride]: the filtered scanlines
    unsigned char *slots;                   // [batch][nchunks][kSlotBytes]: the chunks' payloads
    ChunkRec *recs;                         // [batch][nchunks]
    unsigned *offsets;                      // [batch][nchunks]: of the chunks' IDATs in the frame's bytes
    unsigned char *dst;                     // [batch][cap]
    unsigned *sizes;                        // [batch]
    unsigned long long line_stride;
    Geom g;
};

// the lanes of pngenc_core.h's chunk encoder as the kThreads threads of one workgroup.  What lanes share they share through a maximum, an integer sum
// or an OR in LDS: none of them depends on the order of arrival.
struct BlockLanes {
    template <class F> __device__ void each(F f) const { f(threadIdx.x); }
    template <class F> __device__ void one(F f) const
    {
        if (threadIdx.x == 0) f();
    }
    __device__ void sync() const { __syncthreads(); }
    __device__ void maximum(uint32_t *a, uint32_t v) const { atomicMax(a, v); }
    __device__ void add(uint32_t *a, uint32_t v) const { atomicAdd(a, v); }
    __device__ void bit_or(uint32_t *a, uint32_t v) const { atomicOr(a, v); }
};

// ---- launch 1: one wave per row, four rows per workgroup.  A row reads the raw row above, never a filtered one.
__global__ __launch_bounds__(kThreads) void pngenc_filter(Params p)
{
    const unsigned lane = threadIdx.x & 63, y = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), fi = blockIdx.y;
    if (y >= p.g.height) return;
    const unsigned rowbytes = p.g.width * p.g.comps;
    const unsigned char *px = p.src + (size_t)fi * p.g.height * rowbytes;
    unsigned type = p.g.filter;
    if (type == kFilterHeuristic) {
        unsigned sums[5];
        filter_sums(px, rowbytes, p.g.comps, y, lane, 64, sums);
        for (int f = 0; f < 5; ++f)
            for (int o = 32; o; o >>= 1) sums[f] += __shfl_xor(sums[f], o, 64);
        type = filter_choice(sums);
    }
    filter_write(px, rowbytes, p.g.comps, y, type, lane, 64, p.lines + fi * p.line_stride + (size_t)y * p.g.stride);
}

// ---- launch 2: one workgroup per chunk.  LDS: sizeof(ChunkMem), about 142 KiB (per position of the chunk the hash / match length, the two candidates
// / the match and the exit, 16384 entries each; the two hash tables, the first of which becomes the staged payload; the histograms, the codes and the
// builder's scratch): one chunk per CU.
__global__ __launch_bounds__(kThreads) void pngenc_deflate(Params p)
{
    extern __shared__ __align__(16) unsigned char lds[];
    ChunkMem &m = *reinterpret_cast<ChunkMem *>(lds);
    const unsigned c = blockIdx.x, fi = blockIdx.y;
    ChunkRec *rec = p.recs + (size_t)fi * p.g.nchunks + c;
    encode_chunk(BlockLanes{}, m, p.lines + fi * p.line_stride, p.g, c, rec, nullptr);
    // (encode_chunk ends behind a barrier: the payload is whole)
    unsigned *slot = reinterpret_cast<unsigned *>(p.slots + ((size_t)fi * p.g.nchunks + c) * kSlotBytes);
    const unsigned words = (m.payload + 3) / 4;
    for (unsigned w = threadIdx.x; w < words; w += kThreads) slot[w] = m.out[w];
}

// ---- launch 3: one workgroup per frame: thread t sums a run of chunks, one lane sums the kThreads runs, every thread places its chunks
__global__ __launch_bounds__(kThreads) void pngenc_scan(Params p)
{
    __shared__ unsigned bytes[kThreads], s1[kThreads], s2[kThreads];
    const unsigned fi = blockIdx.x, t = threadIdx.x, n = p.g.nchunks, per = (n + kThreads - 1) / kThreads;
    const ChunkRec *recs = p.recs + (size_t)fi * n;
    const unsigned from = t * per < n ? t * per : n, to = (t + 1) * per < n ? (t + 1) * per : n;
    unsigned b = 0, a1 = 0, a2 = 0;
    for (unsigned c = from; c < to; ++c) {
        b += chunk_file_bytes(recs[c], c);
        a1 = (a1 + recs[c].s1) % kAdlerMod;
        a2 = (a2 + adler_s2_share(recs[c], c, p.g)) % kAdlerMod;
    }
    bytes[t] = b;
    s1[t] = a1;
    s2[t] = a2;
    __syncthreads();
    if (t == 0) {
        unsigned at = 0;
        a1 = a2 = 0;
        for (unsigned k = 0; k < kThreads; ++k) {
            const unsigned v = bytes[k];
            bytes[k] = at;
            at += v;
            a1 = (a1 + s1[k]) % kAdlerMod;
            a2 = (a2 + s2[k]) % kAdlerMod;
        }
        write_tail(p.dst + (size_t)fi * p.g.cap + at, a1, a2, p.g);
        p.sizes[fi] = at + 28;
    }
    __syncthreads();
    unsigned at = bytes[t];
    for (unsigned c = from; c < to; ++c) {
        p.offsets[(size_t)fi * n + c] = at;
        at += chunk_file_bytes(recs[c], c);
    }
}

// ---- launch 4: one workgroup per chunk: length, "IDAT", [78 01,] the payload, the CRC
__global__ __launch_bounds__(kThreads) void pngenc_gather(Params p)
{
    const unsigned c = blockIdx.x, fi = blockIdx.y;
    const size_t ci = (size_t)fi * p.g.nchunks + c;
    const ChunkRec rec = p.recs[ci];
    const unsigned char *payload = p.slots + ci * kSlotBytes;
    unsigned char *dst = p.dst + (size_t)fi * p.g.cap + p.offsets[ci];
    const unsigned nb = chunk_file_bytes(rec, c);
    for (unsigned i = threadIdx.x; i < nb; i += kThreads) dst[i] = chunk_file_byte(rec, c, payload, i);
}

}  // namespace

struct lsppng_enc_handle {
    lsppngenc::Geom g;
    unsigned char header[lsppngenc::kHeaderBytes];
};

namespace {

size_t workspace_layout(const Geom &g, int batch, size_t off[4], size_t *line_stride)
{
    const size_t nc = (size_t)batch * g.nchunks;
    *line_stride = align256(g.raw);
    size_t o = 0;
    off[0] = o; o = align256(o + (size_t)batch * *line_stride);
    off[1] = o; o = align256(o + nc * kSlotBytes);
    off[2] = o; o = align256(o + nc * sizeof(ChunkRec));
    off[3] = o; o = align256(o + nc * sizeof(unsigned));
    return o;
}

}  // namespace

extern "C" {

const char *lsppng_enc_last_error(void) { return g_err.c_str(); }

int lsppng_enc_create(int width, int height, int components, const lsppng_enc_options *options, lsppng_enc_handle **out)
{
    if (!out) return fail(LSPPNG_ENC_ERR_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    int level = 1, filter = -1;
    if (options) {
        if (options->abi_version != LSPPNG_ENC_ABI_VERSION) return fail(LSPPNG_ENC_ERR_INVALID_ARGUMENT, "lsppng_enc_options.abi_version");
        level = options->level;
        filter = options->filter;
    }
    Geom g{};
    if (!make_geom(width, height, components, level, filter, LSPPNG_MAX_SIDE, &g))
        return fail(LSPPNG_ENC_ERR_INVALID_ARGUMENT, "width and height must be in 1.." + std::to_string(LSPPNG_MAX_SIDE) +
                                                         ", components 1 or 3, level 0 or 1, filter -1..4");
    lsppng_enc_handle *h = new lsppng_enc_handle{};
    h->g = g;
    write_header(g, h->header);
    *out = h;
    return LSPPNG_ENC_OK;
}

int lsppng_enc_destroy(lsppng_enc_handle *h)
{
    delete h;
    return LSPPNG_ENC_OK;
}

int64_t lsppng_enc_header(const lsppng_enc_handle *h, unsigned char *buf, size_t cap)
{
    if (!h) return fail(LSPPNG_ENC_ERR_INVALID_ARGUMENT, "null handle");
    if (buf) {
        if (cap < kHeaderBytes) return fail(LSPPNG_ENC_ERR_INVALID_ARGUMENT, "header needs 33 bytes");
        std::copy(h->header, h->header + kHeaderBytes, buf);
    }
    return (int64_t)kHeaderBytes;
}

size_t lsppng_enc_capacity_bytes(const lsppng_enc_handle *h) { return h ? (size_t)h->g.cap : 0; }

size_t lsppng_enc_workspace_bytes(const lsppng_enc_handle *h, int batch)
{
    if (!h || batch < 1) return 0;
    size_t off[4], ls;
    return workspace_layout(h->g, batch, off, &ls);
}

int lsppng_enc_encode(const lsppng_enc_handle *h, const unsigned char *src_dev, int batch, unsigned char *dst_dev, uint32_t *sizes_dev,
                      void *workspace_dev, size_t workspace_bytes, void *hip_stream)
{
    if (!h || !src_dev || !dst_dev || !sizes_dev || !workspace_dev) return fail(LSPPNG_ENC_ERR_INVALID_ARGUMENT, "null argument");
    if (batch < 1 || batch > 65535) return fail(LSPPNG_ENC_ERR_INVALID_ARGUMENT, "batch must be in 1..65535");
    if (reinterpret_cast<uintptr_t>(workspace_dev) % 256) return fail(LSPPNG_ENC_ERR_INVALID_ARGUMENT, "workspace_dev must be 256-byte aligned");
    size_t off[4], line_stride;
    const size_t need = workspace_layout(h->g, batch, off, &line_stride);
    if (workspace_bytes < need) return fail(LSPPNG_ENC_ERR_INVALID_ARGUMENT, "workspace needs " + std::to_string(need) + " bytes");
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&pngenc_deflate), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       (int)sizeof(ChunkMem));
    if (attr != hipSuccess) return fail(LSPPNG_ENC_ERR_HIP, std::string("pngenc_deflate LDS: ") + hipGetErrorString(attr));
    char *ws = static_cast<char *>(workspace_dev);
    Params p{};
    p.src = src_dev;
    p.lines = reinterpret_cast<unsigned char *>(ws + off[0]);
    p.slots = reinterpret_cast<unsigned char *>(ws + off[1]);
    p.recs = reinterpret_cast<ChunkRec *>(ws + off[2]);
    p.offsets = reinterpret_cast<unsigned *>(ws + off[3]);
    p.dst = dst_dev;
    p.sizes = sizes_dev;
    p.line_stride = line_stride;
    p.g = h->g;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const dim3 per_chunk(h->g.nchunks, batch);
    hipLaunchKernelGGL(pngenc_filter, dim3((h->g.height + kThreads / 64 - 1) / (kThreads / 64), batch), dim3(kThreads), 0, st, p);
    hipLaunchKernelGGL(pngenc_deflate, per_chunk, dim3(kThreads), sizeof(ChunkMem), st, p);
    hipLaunchKernelGGL(pngenc_scan, dim3(batch), dim3(kThreads), 0, st, p);
    hipLaunchKernelGGL(pngenc_gather, per_chunk, dim3(kThreads), 0, st, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LSPPNG_ENC_ERR_HIP, std::string("png encode launch: ") + hipGetErrorString(e));
    return LSPPNG_ENC_OK;
}

int64_t lsppng_enc_host_file(const lsppng_enc_handle *h, const unsigned char *pixels, unsigned char *file, size_t cap, uint32_t *forms, uint32_t *rows)
{
    if (!h || !pixels || !file) return fail(LSPPNG_ENC_ERR_INVALID_ARGUMENT, "null argument");
    const Geom &g = h->g;
    if (cap < kHeaderBytes + g.cap) return fail(LSPPNG_ENC_ERR_INVALID_ARGUMENT, "file needs " + std::to_string(kHeaderBytes + g.cap) + " bytes");
    std::unique_ptr<ChunkMem> mem(new ChunkMem());
    std::vector<unsigned char> lines(g.raw), slots((size_t)g.nchunks * kSlotBytes);
    std::vector<ChunkRec> recs(g.nchunks);
    if (forms) forms[0] = forms[1] = forms[2] = 0;
    if (rows)
        for (int f = 0; f < 5; ++f) rows[f] = 0;
    return (int64_t)encode_host(g, pixels, *mem, lines.data(), slots.data(), recs.data(), file, forms, rows);
}

int lsppng_enc_host_code_lengths(const uint32_t *freq, int n, int limit, unsigned char *lengths)
{
    if (!freq || !lengths || n < 1 || n > 288 || limit < 1 || limit > 15) return fail(LSPPNG_ENC_ERR_INVALID_ARGUMENT, "n must be in 1..288, limit in 1..15");
    uint64_t total = 0, used = 0;
    for (int s = 0; s < n; ++s) {
        total += freq[s];
        used += freq[s] != 0;
    }
    if (total >> 32 || used > (1ull << limit)) return fail(LSPPNG_ENC_ERR_INVALID_ARGUMENT, "the frequencies must sum below 2^32 and fit the limit");
    std::unique_ptr<CodeScratch> sc(new CodeScratch());
    for (int s = 0; s < n; ++s) rank_symbol(freq, (uint32_t)n, (uint32_t)s, sc->order);
    build_lengths(freq, (uint32_t)n, (uint32_t)limit, *sc, lengths);
    return LSPPNG_ENC_OK;
}

}  // extern "C"
