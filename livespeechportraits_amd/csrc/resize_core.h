// resize_core.h -- the host half of lspresize.h as plain C++: Pillow's Resample.c coefficient builder (precompute_coeffs + normalize_coeffs_8bpc)
// and the layout of the plan block.  No device code and no HIP header: resize.hip includes it for the library, resize_check.cpp builds it alone
// under AddressSanitizer and UBSan.  The translation unit that includes it is compiled with -ffp-contract=off: every product and sum below is
// rounded to double on its own, as the C of Pillow's build is.
#ifndef LSPF2F_RESIZE_CORE_H
#define LSPF2F_RESIZE_CORE_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace rszcore {

constexpr int kMaxSide = 8192;                    // LSPJPEG_MAX_SIDE
constexpr int kPrecisionBits = 32 - 8 - 2;        // Resample.c PRECISION_BITS
constexpr uint32_t kMagic = 0x5a53524cu;          // "LRSZ"
constexpr uint64_t kMaxPlanBytes = 4u << 20;      // LSPRSZ_MAX_PLAN_BYTES
constexpr int kFilters = 5;                       // box, bilinear, hamming, bicubic, lanczos

// the tile forms' shapes and LDS budget (resize.hip; include/lspresize.h states the switch-over rule)
constexpr int kTilePixelsH = 64;                  // output pixels of a horizontal tile
constexpr int kTileRowsH = 8;                     // rows of a horizontal tile
constexpr int kTileRowsV = 8;                     // output rows of a vertical tile
constexpr int kTileBytesV = 1024;                 // output bytes along x of a vertical tile
constexpr uint32_t kLdsBudget = 48 * 1024;        // bytes of LDS a tile-form workgroup may ask for

constexpr double kPi = 3.14159265358979323846;    // M_PI

inline double f_box(double x) { return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0; }
inline double f_bilinear(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}
inline double f_hamming(double x) {
    if (x < 0.0) x = -x;
    if (x == 0.0) return 1.0;
    if (x >= 1.0) return 0.0;
    x = x * kPi;
    return std::sin(x) / x * (0.54f + 0.46f * std::cos(x));     // float literals widened to double, as Resample.c writes them
}
inline double f_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
inline double f_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * kPi;
    return std::sin(x) / x;
}
inline double f_lanczos(double x) { return (-3.0 <= x && x < 3.0) ? f_sinc(x) * f_sinc(x / 3) : 0.0; }

inline double filter_value(int filter, double x) {
    switch (filter) {
    case 0: return f_box(x);
    case 1: return f_bilinear(x);
    case 2: return f_hamming(x);
    case 3: return f_bicubic(x);
    default: return f_lanczos(x);
    }
}
inline double filter_support(int filter) {
    static const double s[kFilters] = {0.5, 1.0, 1.0, 2.0, 3.0};
    return s[filter];
}

inline int axis_ksize(int in, int out, int filter) {
    double fs = (double)in / out;
    if (fs < 1.0) fs = 1.0;
    return (int)std::ceil(filter_support(filter) * fs) * 2 + 1;
}

// One axis: bounds [out][2] = (xmin, count), coefficients [out][ksize] int32 (zero past count).
inline void axis_coefficients(int in, int out, int filter, int ksize, int32_t *bounds, int32_t *kk) {
    const double scale = (double)in / out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = filter_support(filter) * fs;
    const double ss = 1.0 / fs;
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        if (xmax > ksize) xmax = ksize;           // (never: ksize covers the widest window; a guard for the arrays)
        if (xmax < 0) xmax = 0;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[(size_t)x] = filter_value(filter, (x + xmin - center + 0.5) * ss);
            ww += w[(size_t)x];
        }
        int32_t *k = kk + (size_t)xx * ksize;
        for (int x = 0; x < xmax; ++x) {
            double v = w[(size_t)x];
            if (ww != 0.0) v /= ww;
            const double scaled = v * (double)(1 << kPrecisionBits);
            k[x] = v < 0 ? (int32_t)(-0.5 + scaled) : (int32_t)(0.5 + scaled);
        }
        for (int x = xmax; x < ksize; ++x) k[x] = 0;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

// the identity axis of a plan whose sides do not change: one tap of 2^22 per output, so that the vertical kernel copies
inline void axis_identity(int n, int32_t *bounds, int32_t *kk) {
    for (int i = 0; i < n; ++i) {
        bounds[2 * i] = i;
        bounds[2 * i + 1] = 1;
        kk[i] = 1 << kPrecisionBits;
    }
}

enum { kPathNone = 0, kPathTile = 1, kPathGeneral = 2 };

struct PlanHeader {                               // the first bytes of the block; offsets are from the block's start, 16-byte aligned
    uint32_t magic, bytes;
    int32_t in_w, in_h, out_w, out_h, filter;
    int32_t need_h, need_v;                       // the passes Pillow runs; neither: the block holds an identity vertical axis (a copy)
    int32_t ksize_h, ksize_v;
    int32_t row0, rows;                           // the input rows the horizontal pass produces: [row0, row0 + rows)
    int32_t path_h, path_v;                       // kPath*
    int32_t span_h;                               // the widest input window, in pixels, of a horizontal tile of kTilePixelsH outputs
    uint32_t bounds_h, coef_h, bounds_v, coef_v;
    uint32_t lds_h, lds_v;                        // bytes of LDS of the tile forms (3 channels)
    uint32_t reserved[2];
};
static_assert(sizeof(PlanHeader) % 16 == 0, "the arrays behind the header are 16-byte aligned");

inline uint64_t align16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }

// bytes between the rows a horizontal tile stages in LDS: the window at 3 channels, up to 3 bytes of alignment slack in front, whole words
inline uint32_t lds_row_pitch(int span) { return (uint32_t)((span * 3 + 3 + 3) / 4 * 4 + 4); }

inline const char *check_geometry(int in_w, int in_h, int out_w, int out_h, int filter) {
    if (filter < 0 || filter >= kFilters) return "filter must be 0 (box), 1 (bilinear), 2 (hamming), 3 (bicubic) or 4 (lanczos); NEAREST is not offered";
    if (in_w < 1 || in_h < 1 || out_w < 1 || out_h < 1) return "every side must be at least 1";
    if (in_w > kMaxSide || in_h > kMaxSide || out_w > kMaxSide || out_h > kMaxSide) return "a side above 8192 (LSPJPEG_MAX_SIDE)";
    return nullptr;
}

// bytes the block of that geometry needs (a 64-bit count: the caller compares it with the cap)
inline uint64_t plan_bytes(int in_w, int in_h, int out_w, int out_h, int filter) {
    const bool nh = in_w != out_w, nv = in_h != out_h;
    uint64_t n = sizeof(PlanHeader);
    if (nh) n += align16((uint64_t)out_w * 8) + align16((uint64_t)out_w * axis_ksize(in_w, out_w, filter) * 4);
    const uint64_t kv = nv ? (uint64_t)axis_ksize(in_h, out_h, filter) : 1;       // identity axis when nothing changes along y
    n += align16((uint64_t)out_h * 8) + align16((uint64_t)out_h * kv * 4);
    return n;
}

// Writes the block; blob has plan_bytes() bytes and is 4-byte aligned at least.  Returns the bytes written.
inline uint64_t build_plan(int in_w, int in_h, int out_w, int out_h, int filter, unsigned char *blob) {
    const uint64_t total = plan_bytes(in_w, in_h, out_w, out_h, filter);
    std::memset(blob, 0, (size_t)total);
    PlanHeader h;
    std::memset(&h, 0, sizeof(h));
    h.magic = kMagic;
    h.bytes = (uint32_t)total;
    h.in_w = in_w, h.in_h = in_h, h.out_w = out_w, h.out_h = out_h, h.filter = filter;
    h.need_h = in_w != out_w, h.need_v = in_h != out_h;
    uint64_t at = sizeof(PlanHeader);
    if (h.need_h) {
        h.ksize_h = axis_ksize(in_w, out_w, filter);
        h.bounds_h = (uint32_t)at, at += align16((uint64_t)out_w * 8);
        h.coef_h = (uint32_t)at, at += align16((uint64_t)out_w * h.ksize_h * 4);
        axis_coefficients(in_w, out_w, filter, h.ksize_h, (int32_t *)(blob + h.bounds_h), (int32_t *)(blob + h.coef_h));
    }
    h.ksize_v = h.need_v ? axis_ksize(in_h, out_h, filter) : 1;
    h.bounds_v = (uint32_t)at, at += align16((uint64_t)out_h * 8);
    h.coef_v = (uint32_t)at, at += align16((uint64_t)out_h * h.ksize_v * 4);
    int32_t *bv = (int32_t *)(blob + h.bounds_v);
    if (h.need_v)
        axis_coefficients(in_h, out_h, filter, h.ksize_v, bv, (int32_t *)(blob + h.coef_v));
    else
        axis_identity(out_h, bv, (int32_t *)(blob + h.coef_v));
    // the row window of the horizontal pass: Resample.c ybox_first / ybox_last
    h.row0 = h.need_v ? bv[0] : 0;
    h.rows = h.need_v ? bv[2 * (out_h - 1)] + bv[2 * (out_h - 1) + 1] - h.row0 : in_h;
    if (h.need_h) {
        const int32_t *bh = (const int32_t *)(blob + h.bounds_h);
        int span = 0;
        for (int x0 = 0; x0 < out_w; x0 += kTilePixelsH) {
            const int x1 = x0 + kTilePixelsH < out_w ? x0 + kTilePixelsH : out_w;
            int lo = bh[2 * x0], hi = lo;
            for (int x = x0; x < x1; ++x) {        // (both ends grow with x, which the kernel leans on; this loop does not)
                if (bh[2 * x] < lo) lo = bh[2 * x];
                if (bh[2 * x] + bh[2 * x + 1] > hi) hi = bh[2 * x] + bh[2 * x + 1];
            }
            if (hi - lo > span) span = hi - lo;
        }
        h.span_h = span;
        const uint64_t lds = (uint64_t)kTilePixelsH * (h.ksize_h + 2) * 4 + (uint64_t)kTileRowsH * lds_row_pitch(span);
        h.lds_h = lds <= kLdsBudget ? (uint32_t)lds : 0;
        h.path_h = lds <= kLdsBudget ? kPathTile : kPathGeneral;
    }
    {
        const uint64_t lds = (uint64_t)kTileRowsV * (h.ksize_v + 2) * 4;
        h.lds_v = lds <= kLdsBudget ? (uint32_t)lds : 0;
        h.path_v = lds <= kLdsBudget ? kPathTile : kPathGeneral;
    }
    std::memcpy(blob, &h, sizeof(h));
    return total;
}

inline bool valid_plan(const void *blob) {
    if (!blob) return false;
    PlanHeader h;
    std::memcpy(&h, blob, sizeof(h));
    return h.magic == kMagic && h.bytes >= sizeof(PlanHeader) && h.bytes <= kMaxPlanBytes;
}

inline uint64_t fnv1a(const void *p, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

// FNV-1a over (ksize, bounds, coefficients) of the horizontal axis, then of the vertical one: what resize_check prints and the tests recompute
inline uint64_t plan_digest(const unsigned char *blob) {
    PlanHeader h;
    std::memcpy(&h, blob, sizeof(h));
    uint64_t d = 1469598103934665603ull;
    if (h.need_h) {
        d = fnv1a(&h.ksize_h, 4, d);
        d = fnv1a(blob + h.bounds_h, (size_t)h.out_w * 8, d);
        d = fnv1a(blob + h.coef_h, (size_t)h.out_w * h.ksize_h * 4, d);
    }
    if (h.need_v) {
        d = fnv1a(&h.ksize_v, 4, d);
        d = fnv1a(blob + h.bounds_v, (size_t)h.out_h * 8, d);
        d = fnv1a(blob + h.coef_v, (size_t)h.out_h * h.ksize_v * 4, d);
    }
    return d;
}

}  // namespace rszcore
#endif
