// resize.hip -- include/lspresize.h: PIL.Image.resize for 8-bit grey and RGB images on gfx950, bit for bit.
// The coefficients come from the host (resize_core.h, Pillow's precompute_coeffs in double); the kernels run Resample.c's integer part:
//   out = clamp((2^21 + sum pixel * k) >> 22, 0, 255), horizontal pass first (rounded to uint8, into the workspace), then vertical.
// Two kernels, each in a TILE form (bounds and coefficients of the workgroup in LDS; the horizontal one also stages its input window there in
// 4-byte loads) and a GENERAL form (everything from memory: any tap count).  Every thread forms 4 consecutive BYTES of an output row, so a row of
// 3-byte pixels is stored in whole words; a word that straddles the tile's ends or an unaligned row goes byte by byte.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/lspresize.h"
#include "resize_core.h"

namespace {

using namespace rszcore;

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

constexpr int kThreads = 256;

struct Out {                       // where a pass stores: the workspace or the caller's uint8 images (U8), or float planes through the table
    unsigned char *u8;
    int64_t image_stride;          // bytes (U8), elements (PLANAR_F32)
    int64_t pitch;                 // bytes between rows (U8)
    float *f32;
    const float *table;
    int64_t plane_stride;
    int form, width, channels;
};

struct HArgs {
    const unsigned char *src;      // uint8 [n][in_h][in_w][C]
    int64_t src_stride;
    const int32_t *bounds, *coef;  // [out_w][2], [out_w][ksize]
    int ksize, in_w, out_w;
    int row0, rows;                // the pass reads input rows row0 .. row0 + rows - 1 and writes them as rows 0 .. rows - 1
    int span, lds_pitch;           // TILE: the plan's widest window (pixels) and the bytes between staged rows
    Out out;
};

struct VArgs {
    const unsigned char *src;      // uint8 rows of row_bytes bytes: the workspace (its row 0 is input row `row0`) or the caller's images
    int64_t src_stride, src_pitch;
    const int32_t *bounds, *coef;  // [out_h][2], [out_h][ksize]
    int ksize, out_h, row_bytes, row0;
    Out out;
};

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> kPrecisionBits;           // arithmetic shift, as Resample.c's clip8
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// bytes j0 .. j0 + 3 of row y of image img, those inside [lo, hi): one word where all four are and the address allows it
__device__ __forceinline__ void store4(const Out &o, int img, int y, int j0, int lo, int hi, const int v[4]) {
    if (o.form == LSPRSZ_FORM_U8) {
        unsigned char *p = o.u8 + (int64_t)img * o.image_stride + (int64_t)y * o.pitch;
        if (j0 >= lo && j0 + 4 <= hi && ((uintptr_t)(p + j0) & 3) == 0) {
            *reinterpret_cast<uint32_t *>(p + j0) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (j0 + b >= lo && j0 + b < hi) p[j0 + b] = (unsigned char)v[b];
        }
    } else {
        float *p = o.f32 + (int64_t)img * o.image_stride + (int64_t)y * o.width;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + b;
            if (j >= lo && j < hi) {
                const int x = j / o.channels, c = j - x * o.channels;
                p[(int64_t)c * o.plane_stride + x] = o.table[v[b]];
            }
        }
    }
}

// ---- horizontal pass: grid (ceil(out_w / 64), ceil(rows / 8), n) --------------------------------------------------------------------
template <int C, bool TILE>
__global__ __launch_bounds__(kThreads) void resize_horizontal(HArgs a) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int tid = threadIdx.x, img = blockIdx.z;
    const int px0 = blockIdx.x * kTilePixelsH, px1 = min(px0 + kTilePixelsH, a.out_w), npx = px1 - px0;
    const int r0 = blockIdx.y * kTileRowsH, nr = min(kTileRowsH, a.rows - r0);
    const unsigned char *src = a.src + (int64_t)img * a.src_stride + (int64_t)(a.row0 + r0) * a.in_w * C;
    const int64_t in_pitch = (int64_t)a.in_w * C;
    int32_t *s_b = reinterpret_cast<int32_t *>(lds);                       // [64][2]
    int32_t *s_k = s_b + 2 * kTilePixelsH;                                 // [64][ksize]
    unsigned char *s_pix = reinterpret_cast<unsigned char *>(s_k + (size_t)kTilePixelsH * a.ksize);   // [8][lds_pitch]
    int win_lo = 0;
    if (TILE) {
        for (int i = tid; i < 2 * npx; i += kThreads) s_b[i] = a.bounds[2 * px0 + i];
        for (int i = tid; i < npx * a.ksize; i += kThreads) s_k[i] = a.coef[(size_t)px0 * a.ksize + i];
        __syncthreads();
        // both ends of a window grow with the output index (resize_check holds every plan to it): the tile's window is first begin .. last end
        const int lo = s_b[0], hi = min(s_b[2 * (npx - 1)] + s_b[2 * (npx - 1) + 1], lo + a.span);
        win_lo = lo;
        // the window [lo, hi) of the tile's rows, in whole aligned words where the word lies inside the window
        const int nbytes = (hi - lo) * C, wpr = a.lds_pitch / 4;
        for (int it = tid; it < nr * wpr; it += kThreads) {
            const int r = it / wpr, w = it - r * wpr;
            const unsigned char *first = src + r * in_pitch + (int64_t)lo * C, *last = first + nbytes;
            const unsigned char *word = first - ((uintptr_t)first & 3) + 4 * (int64_t)w;
            if (word >= last) continue;
            unsigned char *dst = s_pix + r * a.lds_pitch + 4 * w;
            if (word >= first && word + 4 <= last) {
                *reinterpret_cast<uint32_t *>(dst) = *reinterpret_cast<const uint32_t *>(word);
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (word + b >= first && word + b < last) dst[b] = word[b];
            }
        }
        __syncthreads();
    }
    const int lo_j = px0 * C, hi_j = px1 * C;
    for (int it = tid; it < nr * 64; it += kThreads) {
        const int r = it >> 6, k = it & 63;
        int s = 0;
        if (a.out.form == LSPRSZ_FORM_U8)
            s = (int)((uintptr_t)(a.out.u8 + (int64_t)img * a.out.image_stride + (int64_t)(r0 + r) * a.out.pitch + lo_j) & 3);
        const int j0 = lo_j - s + 4 * k;
        if (j0 >= hi_j) continue;
        const unsigned char *row;
        if (TILE) {
            const unsigned char *first = src + r * in_pitch + (int64_t)win_lo * C;
            row = s_pix + r * a.lds_pitch + ((uintptr_t)first & 3) - (int64_t)win_lo * C;      // row[x * C + c] is input pixel x
        } else {
            row = src + r * in_pitch;
        }
        int v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + b;
            if (j < lo_j || j >= hi_j) continue;
            const int px = j / C, c = j - px * C;
            int xmin, cnt;
            const int32_t *kp;
            if (TILE) {
                xmin = s_b[2 * (px - px0)], cnt = s_b[2 * (px - px0) + 1], kp = s_k + (size_t)(px - px0) * a.ksize;
            } else {
                xmin = a.bounds[2 * px], cnt = a.bounds[2 * px + 1], kp = a.coef + (size_t)px * a.ksize;
            }
            const unsigned char *pp = row + (int64_t)xmin * C + c;
            int acc = 1 << (kPrecisionBits - 1);
            for (int t = 0; t < cnt; ++t) acc += (int)pp[t * C] * kp[t];
            v[b] = clip8(acc);
        }
        store4(a.out, img, r0 + r, j0, lo_j, hi_j, v);
    }
}

// ---- vertical pass: grid (ceil(row_bytes / 1024), ceil(out_h / 8), n) -----------------------------------------------------------------
template <bool TILE>
__global__ __launch_bounds__(kThreads) void resize_vertical(VArgs a) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int tid = threadIdx.x, img = blockIdx.z;
    const int bx0 = blockIdx.x * kTileBytesV, bx1 = min(bx0 + kTileBytesV, a.row_bytes);
    const int y0 = blockIdx.y * kTileRowsV, nr = min(kTileRowsV, a.out_h - y0);
    const unsigned char *src = a.src + (int64_t)img * a.src_stride;
    int32_t *s_b = reinterpret_cast<int32_t *>(lds);                       // [8][2]
    int32_t *s_k = s_b + 2 * kTileRowsV;                                   // [8][ksize]
    if (TILE) {
        for (int i = tid; i < 2 * nr; i += kThreads) s_b[i] = a.bounds[2 * y0 + i];
        for (int i = tid; i < nr * a.ksize; i += kThreads) s_k[i] = a.coef[(size_t)y0 * a.ksize + i];
        __syncthreads();
    }
    // the words follow the INPUT's alignment: a tap is one 4-byte load wherever the row allows it (every row of the workspace does)
    const int s = (int)((uintptr_t)(src + bx0) & 3);
    const int nq = (s + (bx1 - bx0) + 3) / 4;
    for (int r = 0; r < nr; ++r) {
        int ymin, cnt;
        const int32_t *kp;
        if (TILE) {
            ymin = s_b[2 * r], cnt = s_b[2 * r + 1], kp = s_k + (size_t)r * a.ksize;
        } else {
            ymin = a.bounds[2 * (y0 + r)], cnt = a.bounds[2 * (y0 + r) + 1], kp = a.coef + (size_t)(y0 + r) * a.ksize;
        }
        for (int k = tid; k < nq; k += kThreads) {
            const int j0 = bx0 - s + 4 * k;
            const bool whole = j0 >= bx0 && j0 + 4 <= bx1;
            int acc[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[b] = 1 << (kPrecisionBits - 1);
            const unsigned char *p = src + (int64_t)(ymin - a.row0) * a.src_pitch + j0;
            for (int t = 0; t < cnt; ++t, p += a.src_pitch) {
                const int kt = kp[t];
                if (whole && ((uintptr_t)p & 3) == 0) {
                    const uint32_t w = *reinterpret_cast<const uint32_t *>(p);
                    acc[0] += (int)(w & 255) * kt, acc[1] += (int)((w >> 8) & 255) * kt, acc[2] += (int)((w >> 16) & 255) * kt, acc[3] += (int)(w >> 24) * kt;
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (j0 + b >= bx0 && j0 + b < bx1) acc[b] += (int)p[b] * kt;
                }
            }
            int v[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) v[b] = clip8(acc[b]);
            store4(a.out, img, y0 + r, j0, bx0, bx1, v);
        }
    }
}

int64_t workspace_bytes_of(const PlanHeader &h, int n, int channels) {
    if (!(h.need_h && h.need_v)) return 0;
    return (int64_t)n * h.rows * (int64_t)align16((uint64_t)h.out_w * channels);
}

bool header_of(const void *blob, PlanHeader *h) {
    if (!valid_plan(blob)) return false;
    std::memcpy(h, blob, sizeof(*h));
    return true;
}

}  // namespace

extern "C" {

const char *lsprsz_last_error(void) { return g_err.c_str(); }

int64_t lsprsz_plan(int in_w, int in_h, int out_w, int out_h, int filter, void *blob, size_t cap) {
    if (const char *why = check_geometry(in_w, in_h, out_w, out_h, filter)) return fail(LSPRSZ_ERR_INVALID_ARGUMENT, std::string("lsprsz_plan: ") + why);
    const uint64_t need = plan_bytes(in_w, in_h, out_w, out_h, filter);
    if (need > kMaxPlanBytes)
        return fail(LSPRSZ_ERR_TOO_LARGE, "lsprsz_plan: the block of this geometry needs " + std::to_string(need) + " bytes, above LSPRSZ_MAX_PLAN_BYTES");
    if (!blob) return (int64_t)need;
    if (cap < need) return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_plan: the block needs " + std::to_string(need) + " bytes, cap is " + std::to_string(cap));
    if ((uintptr_t)blob & 15) return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_plan: blob must be 16-byte aligned");
    return (int64_t)build_plan(in_w, in_h, out_w, out_h, filter, (unsigned char *)blob);
}

int lsprsz_plan_info(const void *blob, lsprsz_info *info) {
    PlanHeader h;
    if (!info || !header_of(blob, &h)) return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_plan_info: not a plan block");
    info->in_w = h.in_w, info->in_h = h.in_h, info->out_w = h.out_w, info->out_h = h.out_h, info->filter = h.filter;
    info->need_h = h.need_h, info->need_v = h.need_v;
    info->ksize_h = h.need_h ? h.ksize_h : 0, info->ksize_v = h.need_v ? h.ksize_v : 0;
    info->row0 = h.row0, info->rows = h.rows;
    info->path_h = h.path_h, info->path_v = (h.need_v || !h.need_h) ? h.path_v : LSPRSZ_PATH_NONE;
    info->launches = (h.need_h && h.need_v) ? 2 : 1;
    info->lds_h = h.lds_h, info->lds_v = info->path_v == LSPRSZ_PATH_NONE ? 0 : h.lds_v;
    info->bytes = h.bytes;
    return LSPRSZ_OK;
}

int lsprsz_plan_axis(const void *blob, int axis, int32_t *bounds, size_t cap_bounds, int32_t *coefficients, size_t cap_coefficients) {
    PlanHeader h;
    if (!header_of(blob, &h) || (axis != 0 && axis != 1)) return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_plan_axis: not a plan block, or axis not 0 / 1");
    if (!(axis == 0 ? h.need_h : h.need_v)) return 0;
    const int n = axis == 0 ? h.out_w : h.out_h, ksize = axis == 0 ? h.ksize_h : h.ksize_v;
    const unsigned char *b = (const unsigned char *)blob;
    if (bounds) {
        if (cap_bounds < (size_t)n * 2) return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_plan_axis: bounds needs 2 * outputs values");
        std::memcpy(bounds, b + (axis == 0 ? h.bounds_h : h.bounds_v), (size_t)n * 8);
    }
    if (coefficients) {
        if (cap_coefficients < (size_t)n * ksize) return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_plan_axis: coefficients needs outputs * ksize values");
        std::memcpy(coefficients, b + (axis == 0 ? h.coef_h : h.coef_v), (size_t)n * ksize * 4);
    }
    return n;
}

int64_t lsprsz_workspace_bytes(const void *blob, int n, int channels) {
    PlanHeader h;
    if (!header_of(blob, &h) || n < 1 || (channels != 1 && channels != 3))
        return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_workspace_bytes: not a plan block, n < 1, or channels not 1 / 3");
    return workspace_bytes_of(h, n, channels);
}

int lsprsz_resize(const void *blob_host, const void *blob_dev, const void *src, int64_t src_stride, int n, int channels, const lsprsz_output *out,
                  void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    PlanHeader h;
    if (!header_of(blob_host, &h)) return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_resize: blob_host is not a plan block");
    if (!blob_dev || ((uintptr_t)blob_dev & 15) || !src || !out || !out->ptr) return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_resize: null or unaligned pointer");
    if (channels != 1 && channels != 3) return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_resize: channels must be 1 (grey) or 3 (RGB)");
    if (n < 1 || n > 65535) return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_resize: n must be in 1..65535");
    const int64_t in_bytes = (int64_t)h.in_h * h.in_w * channels, out_row = (int64_t)h.out_w * channels;
    if (n > 1 && src_stride < in_bytes) return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_resize: src_stride is below the bytes of an image");
    Out o{};
    o.form = out->form, o.width = h.out_w, o.channels = channels;
    if (out->form == LSPRSZ_FORM_U8) {
        if (n > 1 && out->image_stride < out_row * h.out_h) return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_resize: image_stride is below the bytes of an image");
        o.u8 = (unsigned char *)out->ptr, o.image_stride = out->image_stride, o.pitch = out_row;
    } else if (out->form == LSPRSZ_FORM_PLANAR_F32) {
        if (!out->table || ((uintptr_t)out->ptr & 3)) return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_resize: PLANAR_F32 needs a table and a float-aligned ptr");
        if (out->plane_stride < (int64_t)h.out_w * h.out_h || (n > 1 && out->image_stride < channels * out->plane_stride))
            return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_resize: plane_stride / image_stride are below a plane / an image");
        o.f32 = (float *)out->ptr, o.table = out->table, o.image_stride = out->image_stride, o.plane_stride = out->plane_stride;
    } else {
        return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_resize: unknown output form");
    }
    const int64_t ws_need = workspace_bytes_of(h, n, channels);
    if (ws_need && (!workspace_dev || ((uintptr_t)workspace_dev & 255) || (int64_t)workspace_bytes < ws_need))
        return fail(LSPRSZ_ERR_INVALID_ARGUMENT, "lsprsz_resize: the workspace needs " + std::to_string(ws_need) + " bytes, 256-byte aligned");
    hipStream_t st = (hipStream_t)hip_stream;
    const unsigned char *bd = (const unsigned char *)blob_dev;
    const int64_t ws_pitch = (int64_t)align16((uint64_t)out_row);

    const unsigned char *vsrc = (const unsigned char *)src;
    int64_t vstride = src_stride, vpitch = (int64_t)h.in_w * channels;
    int vrow0 = 0;
    if (h.need_h) {
        HArgs a{};
        a.src = (const unsigned char *)src, a.src_stride = src_stride;
        a.bounds = (const int32_t *)(bd + h.bounds_h), a.coef = (const int32_t *)(bd + h.coef_h);
        a.ksize = h.ksize_h, a.in_w = h.in_w, a.out_w = h.out_w, a.row0 = h.row0, a.rows = h.rows;
        a.span = h.span_h, a.lds_pitch = (int)lds_row_pitch(h.span_h);
        if (h.need_v) {
            Out w{};
            w.form = LSPRSZ_FORM_U8, w.width = h.out_w, w.channels = channels;
            w.u8 = (unsigned char *)workspace_dev, w.pitch = ws_pitch, w.image_stride = ws_pitch * h.rows;
            a.out = w;
            vsrc = (const unsigned char *)workspace_dev, vstride = w.image_stride, vpitch = ws_pitch, vrow0 = h.row0;
        } else {
            a.out = o;
        }
        const dim3 grid((h.out_w + kTilePixelsH - 1) / kTilePixelsH, (h.rows + kTileRowsH - 1) / kTileRowsH, n);
        const bool tile = h.path_h == kPathTile;
        const size_t lds = tile ? (size_t)kTilePixelsH * (h.ksize_h + 2) * 4 + (size_t)kTileRowsH * a.lds_pitch : 0;
        if (channels == 3) {
            if (tile) hipLaunchKernelGGL((resize_horizontal<3, true>), grid, dim3(kThreads), lds, st, a);
            else hipLaunchKernelGGL((resize_horizontal<3, false>), grid, dim3(kThreads), 0, st, a);
        } else {
            if (tile) hipLaunchKernelGGL((resize_horizontal<1, true>), grid, dim3(kThreads), lds, st, a);
            else hipLaunchKernelGGL((resize_horizontal<1, false>), grid, dim3(kThreads), 0, st, a);
        }
    }
    if (h.need_v || !h.need_h) {
        VArgs a{};
        a.src = vsrc, a.src_stride = vstride, a.src_pitch = vpitch;
        a.bounds = (const int32_t *)(bd + h.bounds_v), a.coef = (const int32_t *)(bd + h.coef_v);
        a.ksize = h.ksize_v, a.out_h = h.out_h, a.row_bytes = (int)out_row, a.row0 = vrow0;
        a.out = o;
        const dim3 grid(((int)out_row + kTileBytesV - 1) / kTileBytesV, (h.out_h + kTileRowsV - 1) / kTileRowsV, n);
        if (h.path_v == kPathTile)
            hipLaunchKernelGGL((resize_vertical<true>), grid, dim3(kThreads), (size_t)kTileRowsV * (h.ksize_v + 2) * 4, st, a);
        else
            hipLaunchKernelGGL((resize_vertical<false>), grid, dim3(kThreads), 0, st, a);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LSPRSZ_ERR_HIP, std::string("lsprsz_resize: ") + hipGetErrorString(e));
    return LSPRSZ_OK;
}

}  // extern "C"
