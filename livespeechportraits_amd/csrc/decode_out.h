// decode_out.h -- what the image decoders (jpegdec.hip, pngdec.hip) share about their outputs: the planner's view of one output, the check that an
// output's form fits its file, and the store of one pixel in that form.  The three forms are the words of include/lspjpegdec.h and include/lsppng.h
// (LSP*_DEC_FORM_*).  Plain C++ with no allocation and no library calls: the planners (jpegdec_plan.h, pngdec_plan.h) build from it for the host
// alone and run under sanitizers; the store kernels and the host twins call store_pixel.
#ifndef LSP_DECODE_OUT_H
#define LSP_DECODE_OUT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define LSPOUT_HD __host__ __device__
#else
#define LSPOUT_HD
#endif

namespace lspout {

enum : uint32_t { kFormRgb8 = 0, kFormGray8 = 1, kFormPlanarF32 = 2 };

// the planner's own view of lspjpeg_dec_output / lsppng_dec_output
struct OutputDesc {
    uint64_t ptr, table;
    int64_t plane_stride;
    uint32_t form;
};

inline uint64_t up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// od[0..n) from the public array of either header
template <class Output> inline void describe_outputs(const Output *outs, int n, OutputDesc *od)
{
    for (int i = 0; i < n; ++i) {
        od[i].ptr = reinterpret_cast<uint64_t>(outs[i].ptr);
        od[i].table = reinterpret_cast<uint64_t>(outs[i].table);
        od[i].plane_stride = outs[i].plane_stride;
        od[i].form = (uint32_t)outs[i].form;
    }
}

// RGB8 takes a file of 3 components, GRAY8 one of 1, PLANAR_F32 either, with a table and planes that hold the file's pixels
inline bool output_fits(const OutputDesc &o, uint32_t ncomp, int64_t pixels)
{
    return !(o.form > 2 || (o.form == 0 && ncomp != 3) || (o.form == 1 && ncomp != 1) || (o.form == 2 && (!o.table || o.plane_stride < pixels)));
}

constexpr const char *kOutputRefusal =
    "an output's form does not fit its file (RGB8: 3 components, GRAY8: 1, PLANAR_F32: a table and plane_stride >= H * W)";

// pixel g (row-major) of a file of ncomp components, px[0..ncomp) in 0..255, in the form the planner accepted
template <class T> LSPOUT_HD inline void store_pixel(uint32_t form, uint64_t out_ptr, uint64_t table_ptr, int64_t plane_stride, uint32_t ncomp, size_t g, const T *px)
{
    if (form == kFormPlanarF32) {
        float *out = reinterpret_cast<float *>(out_ptr);
        const float *table = reinterpret_cast<const float *>(table_ptr);
        for (uint32_t c = 0; c < ncomp; ++c) out[(size_t)c * plane_stride + g] = table[px[c]];
    } else {
        unsigned char *out = reinterpret_cast<unsigned char *>(out_ptr);
        if (ncomp == 3) {
            out[g * 3 + 0] = (unsigned char)px[0];
            out[g * 3 + 1] = (unsigned char)px[1];
            out[g * 3 + 2] = (unsigned char)px[2];
        } else {
            out[g] = (unsigned char)px[0];
        }
    }
}

}  // namespace lspout
#endif
