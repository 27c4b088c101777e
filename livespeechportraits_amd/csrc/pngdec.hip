// pngdec.hip -- the PNG decoder of include/lsppng.h: three launches on the device (inflate, unfilter, store) behind a host planner.  The inflater,
// the unfilter arithmetic and the pixel fetch live in pngdec_core.h, the chunk walker and the planner in pngdec_plan.h; both also build for the host
// alone and run under sanitizers (make check-pngdec).
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/lspjpegdec.h"
#include "../../include/lsppng.h"
#include "pngdec_plan.h"

// one ctypes structure serves both planners (_native.py JpegDecOutput), and decode_out.h's forms are both headers' words
static_assert(sizeof(lsppng_dec_output) == sizeof(lspjpeg_dec_output), "the two output descriptions are one layout");
static_assert(offsetof(lsppng_dec_output, ptr) == offsetof(lspjpeg_dec_output, ptr) && offsetof(lsppng_dec_output, table) == offsetof(lspjpeg_dec_output, table), "the two output descriptions are one layout");
static_assert(offsetof(lsppng_dec_output, plane_stride) == offsetof(lspjpeg_dec_output, plane_stride) && offsetof(lsppng_dec_output, form) == offsetof(lspjpeg_dec_output, form), "the two output descriptions are one layout");
static_assert(offsetof(lsppng_dec_output, reserved) == offsetof(lspjpeg_dec_output, reserved), "the two output descriptions are one layout");
static_assert(LSPPNG_DEC_FORM_RGB8 == lspout::kFormRgb8 && LSPPNG_DEC_FORM_GRAY8 == lspout::kFormGray8 && LSPPNG_DEC_FORM_PLANAR_F32 == lspout::kFormPlanarF32, "the forms of lsppng.h");
static_assert(LSPJPEG_DEC_FORM_RGB8 == lspout::kFormRgb8 && LSPJPEG_DEC_FORM_GRAY8 == lspout::kFormGray8 && LSPJPEG_DEC_FORM_PLANAR_F32 == lspout::kFormPlanarF32, "the forms of lspjpegdec.h");

namespace {

using namespace lsppng;

thread_local std::string g_err;
int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

struct Params {
    const unsigned char *blob;              // the descriptor block on the device
    const FileDesc *files;
    unsigned *status;                       // [nfiles]
    unsigned char *ws;
    unsigned nfiles;
    unsigned long long bytes;               // of the block: no load reaches past it
};

// the lanes of pngdec_core.h's Inflater as the 64 lanes of one wave (the workgroup is that wave: its barrier orders the LDS traffic of the lanes)
struct WaveLanes {
    template <class F> __device__ void each(F f) const { f(threadIdx.x); }
    template <class F> __device__ void one(F f) const
    {
        if (threadIdx.x == 0) f();
    }
    template <class F> __device__ uint64_t sum(F f) const
    {
        unsigned long long v = f(threadIdx.x);
        for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
    }
    __device__ void sync() const { __syncthreads(); }
};

// ---- launch 1: one wave per file.  LDS: sizeof(InflateMem) = 43460 bytes per workgroup (the 32 KiB window, the 4 KiB stream ring, two decode
// tables of 2656 bytes, the code lengths and their codes), so three files inflate side by side on one CU (160 KiB).
__global__ __launch_bounds__(kLanes) void pngdec_inflate(Params p)
{
    __shared__ InflateMem mem;
    const unsigned fi = blockIdx.x;
    if (fi >= p.nfiles) return;
    const FileDesc &f = p.files[fi];
    if (f.status != ST_OK) return;
    const unsigned long long begin = f.idat_begin + 2, end = f.idat_end, ws_off = f.ws_off;
    const unsigned raw_bytes = f.raw_bytes;
    Inflater<WaveLanes> inf(WaveLanes{}, &mem, p.blob, p.bytes, begin, end, p.ws + ws_off, raw_bytes);
    const unsigned st = inf.run();
    if (st != ST_OK && threadIdx.x == 0) atomicCAS(p.status + fi, 0u, st);
}

// ---- launch 2: one wave per file, in place.  Byte x of row y needs byte x - bpp of its own row and bytes x and x - bpp of the row above, so the
// rows of a band of 64 run as a skewed wavefront: lane l owns row band + l and works on the 4-byte unit t - l at step t, one unit behind lane l - 1,
// whose unit of the step before IS the unit above (one cross-lane move per step; the unit above-left is the one the lane received a step earlier).
// Lane 0 takes the row above from LDS, where lane 63 of the band before left it.  LDS: 32 KiB (the longest row, 8192 RGBA pixels).
// A lane never reads memory another lane wrote: its raw bytes come from stage 1, behind a kernel boundary.
constexpr unsigned kMaxUnits = LSPPNG_MAX_SIDE;                // 4 * 8192 bytes / 4

__device__ __forceinline__ unsigned load_unit(const unsigned char *row, int u, unsigned rowbytes)
{
    unsigned v = 0;
    const unsigned x = 4u * (unsigned)u;
    if (x + 4 <= rowbytes) {
        __builtin_memcpy(&v, row + x, 4);
    } else {
        for (unsigned j = 0; j < 4 && x + j < rowbytes; ++j) v |= (unsigned)row[x + j] << (8 * j);
    }
    return v;
}

__global__ __launch_bounds__(kLanes) void pngdec_unfilter(Params p)
{
    __shared__ unsigned s_last[kMaxUnits];
    const unsigned fi = blockIdx.x;
    if (fi >= p.nfiles) return;
    const FileDesc &f = p.files[fi];
    if (p.status[fi] != ST_OK) return;
    const unsigned lane = threadIdx.x;
    const unsigned rowbytes = f.rowbytes, height = f.height, bpp = f.bpp, stride = 1 + rowbytes;
    const int nunits = (int)((rowbytes + 3) / 4);                              // <= kMaxUnits: rowbytes <= 4 * max_side
    const bool check = f.color_type == 3 && f.npal < (1u << f.depth);
    unsigned char *raw = p.ws + f.ws_off;
    for (int k = lane; k < nunits; k += kLanes) s_last[k] = 0;                 // the row above the first row is zeros
    __syncthreads();
    bool bad = false;
    for (unsigned band = 0; band < height; band += kLanes) {
        const unsigned y = band + lane;
        const bool have = y < height;
        unsigned char *row = raw + (size_t)(have ? y : 0) * stride + 1;
        unsigned ft = have ? row[-1] : 0u;
        if (ft > 4) {
            bad = true;
            ft = 0;
        }
        unsigned out = 0, above_prev = 0;
        unsigned next = have && lane == 0 ? load_unit(row, 0, rowbytes) : 0u;
        for (int t = 0; t < nunits + (int)kLanes - 1; ++t) {
            const int u = t - (int)lane;
            const bool active = have && u >= 0 && u < nunits;
            const unsigned handed = __shfl_up(out, 1, kLanes);                 // lane l - 1's unit of the step before: unit u of the row above
            const unsigned rawv = next;
            next = have && u + 1 >= 0 && u + 1 < nunits ? load_unit(row, u + 1, rowbytes) : 0u;
            if (!active) continue;
            const unsigned above = lane == 0 ? s_last[u] : handed;
            unsigned long long own = out, up2 = (unsigned long long)above_prev | ((unsigned long long)above << 32);
            if (u == 0) own = 0;
            const unsigned x0 = 4u * (unsigned)u;
#pragma unroll
            for (unsigned j = 0; j < 4; ++j) {
                if (x0 + j >= rowbytes) break;
                const unsigned a = (unsigned)(own >> (8 * (4 + j - bpp))) & 255u, c = (unsigned)(up2 >> (8 * (4 + j - bpp))) & 255u;
                const unsigned b = (above >> (8 * j)) & 255u;
                const unsigned r = reconstruct(ft, (rawv >> (8 * j)) & 255u, a, b, c);
                own |= (unsigned long long)r << (8 * (4 + j));
                if (check && index_bad(f, x0 + j, r)) bad = true;
            }
            out = (unsigned)(own >> 32);
            above_prev = above;
            if (x0 + 4 <= rowbytes) {
                __builtin_memcpy(row + x0, &out, 4);
            } else {
                for (unsigned j = 0; x0 + j < rowbytes; ++j) row[x0 + j] = (unsigned char)(out >> (8 * j));
            }
            if (lane == kLanes - 1) s_last[u] = out;
        }
        __syncthreads();                                                       // lane 63's row is in LDS before lane 0 of the next band reads it
    }
    if (bad) atomicCAS(p.status + fi, 0u, (unsigned)ST_CORRUPT);               // launch 3 then leaves the file's output alone
}

// ---- launch 3: one thread per pixel
constexpr int kStoreThreads = 256;

__global__ __launch_bounds__(kStoreThreads) void pngdec_store(Params p)
{
    const unsigned fi = blockIdx.y;
    const FileDesc &f = p.files[fi];
    const unsigned g = blockIdx.x * kStoreThreads + threadIdx.x;
    if (g >= f.width * f.height || p.status[fi] != ST_OK) return;
    const unsigned x = g % f.width, y = g / f.width;
    unsigned px[3];
    pixel_of(f, p.ws + f.ws_off + (size_t)y * (1 + f.rowbytes) + 1, x, px);
    lspout::store_pixel(f.form, f.out_ptr, f.table_ptr, f.plane_stride, f.ncomp, g, px);
}

void fill_info(const Parsed &f, lsppng_dec_info *info)
{
    *info = lsppng_dec_info{};
    info->status = (int32_t)f.status;
    info->width = (int32_t)f.width;
    info->height = (int32_t)f.height;
    info->color_type = (int32_t)f.color_type;
    info->depth = (int32_t)f.depth;
    info->components = (int32_t)f.ncomp;
    if (f.status != ST_OK) return;
    info->idat_bytes = f.idat_bytes;
    info->raw_bytes = f.raw_bytes;
}

}  // namespace

extern "C" {

const char *lsppng_dec_last_error(void) { return g_err.c_str(); }

int lsppng_dec_probe(const unsigned char *bytes, size_t len, lsppng_dec_info *info)
{
    if (!bytes || !info) return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "null argument");
    Parsed f;
    examine_all(bytes, len, LSPPNG_MAX_SIDE, &f);
    fill_info(f, info);
    return LSPPNG_DEC_OK;
}

int64_t lsppng_dec_plan(const unsigned char *const *files, const size_t *lens, const lsppng_dec_output *outs, int n, int max_side, void *blob, size_t cap)
{
    if (!files || !lens || n < 1 || n > 65535) return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "files, lens and 1..65535 files are required");
    if (max_side < 1 || max_side > LSPPNG_MAX_SIDE) return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "max_side must be in 1.." + std::to_string(LSPPNG_MAX_SIDE));
    for (int i = 0; i < n; ++i)
        if (!files[i]) return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "file " + std::to_string(i) + " is null");
    const int64_t need = plan(files, lens, nullptr, n, (uint32_t)max_side, nullptr);
    if (need < 0) return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "the batch needs a descriptor block of 4 GiB or more: split it");
    if (!blob) return need;
    if (cap < (size_t)need || reinterpret_cast<uintptr_t>(blob) % 16)
        return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "blob must be 16-byte aligned and hold " + std::to_string(need) + " bytes");
    std::vector<OutputDesc> od(outs ? (size_t)n : 0);
    if (outs) lspout::describe_outputs(outs, n, od.data());
    const int64_t got = plan(files, lens, outs ? od.data() : nullptr, n, (uint32_t)max_side, blob);
    if (got == -1) return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, lspout::kOutputRefusal);
    return got;
}

int lsppng_dec_summary_of(const void *blob, lsppng_dec_summary *out)
{
    const BlobHeader *h = header_of(blob);
    if (!h || !out) return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "not a descriptor block of lsppng_dec_plan");
    out->files = h->nfiles;
    out->max_pixels = h->max_pixels;
    out->bytes = h->bytes;
    out->workspace_bytes = h->workspace_bytes;
    out->status_offset = h->status_off;
    return LSPPNG_DEC_OK;
}

int lsppng_dec_plan_file(const void *blob, int i, lsppng_dec_info *info)
{
    const BlobHeader *h = header_of(blob);
    if (!h || !info || i < 0 || (uint32_t)i >= h->nfiles) return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "no such file in the block");
    const FileDesc &d = files_of(blob)[i];
    *info = lsppng_dec_info{};
    info->status = (int32_t)d.status;
    if (d.status != ST_OK) return LSPPNG_DEC_OK;
    info->width = (int32_t)d.width;
    info->height = (int32_t)d.height;
    info->color_type = (int32_t)d.color_type;
    info->depth = (int32_t)d.depth;
    info->components = (int32_t)d.ncomp;
    info->idat_bytes = d.idat_end - d.idat_begin;
    info->raw_bytes = d.raw_bytes;
    return LSPPNG_DEC_OK;
}

int lsppng_dec_host_scanlines(const void *blob, int i, unsigned char *out, size_t cap)
{
    const BlobHeader *h = header_of(blob);
    if (!h || !out || i < 0 || (uint32_t)i >= h->nfiles) return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "no such file in the block");
    const FileDesc &d = files_of(blob)[i];
    if (d.status == ST_OK && cap < d.raw_bytes) return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "out is too small for the file's scanlines");
    if (d.status != ST_OK) return (int)d.status;
    std::unique_ptr<InflateMem> mem(new InflateMem());
    std::vector<uint8_t> lines(d.raw_bytes);                                   // 16-byte aligned, as the flush's stores expect; the caller's buffer need not be
    const uint32_t st = host_scanlines(blob, i, mem.get(), lines.data());
    if (st == ST_OK) std::memcpy(out, lines.data(), lines.size());
    return (int)st;
}

int lsppng_dec_host_pixels(const void *blob, int i, unsigned char *out, size_t cap)
{
    const BlobHeader *h = header_of(blob);
    if (!h || !out || i < 0 || (uint32_t)i >= h->nfiles) return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "no such file in the block");
    const FileDesc &d = files_of(blob)[i];
    if (d.status != ST_OK) return (int)d.status;
    if (cap < (size_t)d.width * d.height * d.ncomp) return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "out is too small for the file's pixels");
    std::unique_ptr<InflateMem> mem(new InflateMem());
    std::vector<uint8_t> lines(d.raw_bytes);
    const uint32_t st = host_scanlines(blob, i, mem.get(), lines.data());
    if (st != ST_OK) return (int)st;
    return (int)host_pixels(blob, i, lines.data(), out);
}

int lsppng_dec_decode(const void *blob_host, void *blob_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream)
{
    const BlobHeader *h = header_of(blob_host);
    if (!h || !blob_dev || !workspace_dev) return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "a planned block, its device copy and a workspace are required");
    if (!h->has_outputs) return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "the block was planned without outputs (host only)");
    if (reinterpret_cast<uintptr_t>(blob_dev) % 16 || reinterpret_cast<uintptr_t>(workspace_dev) % 256)
        return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "blob_dev must be 16-byte aligned and workspace_dev 256-byte aligned");
    if (workspace_bytes < h->workspace_bytes) return fail(LSPPNG_DEC_ERR_INVALID_ARGUMENT, "workspace needs " + std::to_string(h->workspace_bytes) + " bytes");
    unsigned char *b = static_cast<unsigned char *>(blob_dev);
    Params p{};
    p.blob = b;
    p.files = reinterpret_cast<const FileDesc *>(b + h->files_off);
    p.status = reinterpret_cast<unsigned *>(b + h->status_off);
    p.ws = static_cast<unsigned char *>(workspace_dev);
    p.nfiles = h->nfiles;
    p.bytes = h->bytes;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const unsigned pixel_groups = h->max_pixels ? (h->max_pixels + kStoreThreads - 1) / kStoreThreads : 1u;     // a batch of refused files still launches
    hipLaunchKernelGGL(pngdec_inflate, dim3(h->nfiles), dim3(kLanes), 0, st, p);
    hipLaunchKernelGGL(pngdec_unfilter, dim3(h->nfiles), dim3(kLanes), 0, st, p);
    hipLaunchKernelGGL(pngdec_store, dim3(pixel_groups, h->nfiles), dim3(kStoreThreads), 0, st, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LSPPNG_DEC_ERR_HIP, std::string("png decode launch: ") + hipGetErrorString(e));
    return LSPPNG_DEC_OK;
}

}  // extern "C"
