// gfx950: baseline JPEG encoding of uint8 frames on the device (include/lspjpeg.h), byte-identical to Pillow / libjpeg-turbo's defaults.
//
// Four launches per batch, whatever the content, all on the caller's stream:
//   1. jpeg_transform  thread per 8x8 block: colour conversion (+ 4:2:0 box for chroma), islow DCT, quantisation, the block's coefficients
//                      in zigzag order to the workspace, and the bits of its AC symbols (they depend on nothing outside the block);
//   2. jpeg_offsets    workgroup per frame: adds each block's DC bits (the difference to the previous block of its component is known once
//                      every block is quantised), exclusive scan -> the bit offset of every block, the frame's total, and zeroes the words
//                      the frame's bits will occupy;
//   3. jpeg_emit       thread per block: the block's symbols written at its offset into a big-endian bit stream of 32-bit words
//                      (a 64-bit accumulator, one atomicOr per finished word: the first and last word are shared with the neighbours);
//   4. jpeg_stuff      workgroup per frame: bytes of the stream, the last one padded with 1-bits, 0x00 after every 0xFF (count per
//                      16-byte chunk, scan, scatter), EOI, and the byte count.
// No host round trip: the variable sizes travel between the launches in the workspace.
//
// A handle with options (lspjpeg_create_opts: optimised Huffman tables, restart intervals) runs instances of its own, four launches as well:
// jpeg_transform<true> (no AC bit counts: the tables are not known yet), jpeg_tables in place of jpeg_offsets (histograms, the tables of
// jpegenc_core.h, the frame's DHT .. SOS, bit offsets per block and byte offsets per interval), jpeg_emit<true> (codes from the workspace, every
// interval padded on its own), jpeg_stuff<true> (RSTn behind every interval but the last).  The options are template parameters: the
// instances of a plain handle hold none of that code.
//
// A format handle (lspjpeg_create_format: frames of any size in 4:4:4, 4:2:2, 4:2:0 or grey) whose geometry is not the one above runs four launches
// as well: jpeg_transform_geom (thread per coded block of the grid of jpegenc_geom.h, dummy blocks included; pixels read byte by byte at clamped
// coordinates), jpeg_tables_geom and jpeg_emit_geom (the bodies of jpeg_tables and jpeg_emit<true> with the block's table and its DC difference
// taken from that grid: a dummy block's DC is read at its DC source), and jpeg_stuff<true> itself.  With the geometry above it gets the handle and
// the instances above.
#include "../../include/lspjpeg.h"

#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <vector>

#include "jpegenc_core.h"
#include "jpegenc_geom.h"

namespace lspjpeg {

constexpr int NT = 256;                     // threads per workgroup of the per-block kernels
constexpr int NS = 1024;                    // threads of the per-frame workgroups (scan, stuffing)

// ---- Annex K tables ----------------------------------------------------------------------------------------------------------
constexpr unsigned char kLumaQ[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr unsigned char kChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                        47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// natural (row-major) index of zigzag position k
constexpr int kNatural[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                              35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Huffman tables in the order DC0, AC0, DC1, AC1: code counts per length 1..16, then the symbols
constexpr unsigned char kBits[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                        {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                        {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                        {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr unsigned char kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr unsigned char kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr unsigned char kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// canonical codes (Annex C): per symbol (length << 16) | code, 0 for a symbol the table lacks
struct Codes {
    unsigned v[256];
};

constexpr Codes make_codes(const unsigned char *bits, const unsigned char *vals)
{
    Codes c{};
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i)
            c.v[vals[k++]] = ((unsigned)len << 16) | code++;
        code <<= 1;
    }
    return c;
}

__constant__ Codes kCodes[4] = {make_codes(kBits[0], kDcVals), make_codes(kBits[1], kAcLumaVals), make_codes(kBits[2], kDcVals),
                                make_codes(kBits[3], kAcChromaVals)};

struct Params {
    const unsigned char *src;
    short *coef;                            // [batch][blocks][64] zigzag
    unsigned *acbits;                       // [batch][blocks]
    unsigned *offsets;                      // [batch][blocks] bit offset of the block in its frame's stream
    unsigned *totals;                       // [batch] bits of the frame
    unsigned *words;                        // [batch][wcap] the stream, MSB first
    unsigned char *dst;
    unsigned *sizes;
    int w, h, comps, mcux, nmcu, nblk, wcap;
    unsigned long long cap;
    unsigned short div[2][64];              // qtable << 3, natural order: luma, chroma
};

// a handle with options (optimised tables, restart intervals) runs instances of its own: the instances of a plain handle see none of this
struct OptParams : Params {
    unsigned *codes;                        // [batch][4][256] (length << 16) | code per symbol: DC0 AC0 DC1 AC1 of the frame
    unsigned *istart;                       // [batch][nint + 1] first byte of every interval in the unstuffed stream; [nint] = all bytes
    unsigned *prelen;                       // [batch] bytes of the frame's DHT .. SOS in dst (0 without optimize: they are in the header)
    int restart, nint, ibl, bpm, optimize;  // MCUs per interval (0: none), intervals per frame, blocks per interval and per MCU
};
template <bool kOpts>
using ParamsOf = std::conditional_t<kOpts, OptParams, Params>;

// a format handle of another geometry than the two above (lspjpeg_create_format: any size, 4:4:4 / 4:2:2 / 4:2:0 / grey) runs the *_geom instances:
// the MCU layout comes from jpegenc_geom.h, the rest is the code of a handle with options
struct GeomParams : OptParams {
    lspgeom::Geom geo;
};

// ---- device helpers ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int nbits(int v)
{
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __clz(a) : 0;
}

__device__ __forceinline__ unsigned byte_of(const unsigned *w, int i) { return (w[i >> 2] >> ((i & 3) * 8)) & 0xffu; }   // little-endian memory

constexpr int CB = 13, P1 = 2;

// jfdctint.c jpeg_fdct_islow, one pass over the 8 elements d[0], d[S], ..., d[7S]
template <bool kRows, int S>
__device__ __forceinline__ void fdct_pass(int *d)
{
    const int sh = kRows ? CB - P1 : CB + P1;
    const int rnd = 1 << (sh - 1);
    const int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S];
    const int t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
    const int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S];
    const int t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (kRows) {
        d[0] = (t10 + t11) << P1;
        d[4 * S] = (t10 - t11) << P1;
    } else {
        d[0] = (t10 + t11 + (1 << (P1 - 1))) >> P1;
        d[4 * S] = (t10 - t11 + (1 << (P1 - 1))) >> P1;
    }
    int z1 = (t12 + t13) * 4433;
    d[2 * S] = (z1 + t13 * 6270 + rnd) >> sh;
    d[6 * S] = (z1 - t12 * 15137 + rnd) >> sh;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7 * S] = (a4 + z1 + z3 + rnd) >> sh;
    d[5 * S] = (a5 + z2 + z4 + rnd) >> sh;
    d[3 * S] = (a6 + z2 + z3 + rnd) >> sh;
    d[S] = (a7 + z1 + z4 + rnd) >> sh;
}

// index (within its frame) of the previous block of the same component, -1 for the first
__device__ __forceinline__ int prev_block(int g, int comps)
{
    if (comps == 1) return g - 1;
    const int j = g % 6;
    if (j >= 1 && j <= 3) return g - 1;
    if (g < 6) return -1;
    return j == 0 ? g - 3 : g - 6;          // Y0 follows the previous MCU's Y3; Cb / Cr follow the previous MCU's
}

__device__ __forceinline__ int table_of(int g, int comps) { return comps == 3 && g % 6 >= 4 ? 1 : 0; }
__device__ __forceinline__ int table_of(const Params &p, int g) { return table_of(g, p.comps); }
__device__ __forceinline__ int table_of(const GeomParams &p, int g) { return lspgeom::table_of(p.geo, g); }

// exclusive prefix sum over the NS threads of the workgroup; *total = the sum.  `lds` holds NS / 64 + 1 words.
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned *lds, unsigned *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned s = 0;
        for (int k = 0; k < NS / 64; ++k) {
            const unsigned t = lds[k];
            lds[k] = s;
            s += t;
        }
        lds[NS / 64] = s;
    }
    __syncthreads();
    const unsigned r = lds[wave] + x - v;
    *total = lds[NS / 64];
    __syncthreads();                        // lds is reused by the next call
    return r;
}

// islow DCT of the level-shifted samples s, quantisation (round half away from zero) with the divisors div (natural order), and the block's
// coefficients in zigzag order: in z, and as 64 shorts at dst.  The tail of jpeg_transform below, for jpeg_transform_geom (jpeg_transform keeps its
// own text: its instances are the code objects a handle of lspjpeg_create has always launched)
__device__ __forceinline__ void dct_quantise_store(int (&s)[64], const unsigned short (&div)[64], int (&z)[64], short *dst)
{
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct_pass<true, 1>(s + r * 8);
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct_pass<false, 8>(s + c);
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int v = s[kNatural[k]];
        const unsigned d = div[kNatural[k]];
        const unsigned a = ((unsigned)(v < 0 ? -v : v) + (d >> 1)) / d;
        z[k] = v < 0 ? -(int)a : (int)a;
    }
    uint4 *out = reinterpret_cast<uint4 *>(dst);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int *zz = z + k * 8;
        out[k] = make_uint4((zz[0] & 0xffff) | ((unsigned)zz[1] << 16), (zz[2] & 0xffff) | ((unsigned)zz[3] << 16),
                            (zz[4] & 0xffff) | ((unsigned)zz[5] << 16), (zz[6] & 0xffff) | ((unsigned)zz[7] << 16));
    }
}

// ---- 1. transform + quantise + AC bits ----------------------------------------------------------------------------------------
template <bool kOpts>
__global__ __launch_bounds__(NT) void jpeg_transform(ParamsOf<kOpts> p)
{
    const int f = blockIdx.y;
    const int t = blockIdx.x * NT + threadIdx.x;
    if (t >= p.nblk) return;
    int s[64];
    int g, tab;
    if (p.comps == 1) {
        g = t;
        tab = 0;
        const int bx = t % p.mcux, by = t / p.mcux;
        const unsigned char *src = p.src + ((size_t)f * p.h + (size_t)by * 8) * p.w + bx * 8;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const uint2 v = *reinterpret_cast<const uint2 *>(src + (size_t)r * p.w);
            const unsigned wv[2] = {v.x, v.y};
#pragma unroll
            for (int c = 0; c < 8; ++c) s[r * 8 + c] = (int)byte_of(wv, c) - 128;
        }
    } else {
        const int ny = 4 * p.nmcu;          // threads [0, ny): luma blocks; [ny, 6 nmcu): chroma blocks (waves stay on one path)
        const size_t row = (size_t)p.w * 3;
        if (t < ny) {
            const int m = t >> 2, j = t & 3;
            g = m * 6 + j;
            tab = 0;
            const int x0 = (m % p.mcux) * 16 + (j & 1) * 8, y0 = (m / p.mcux) * 16 + (j >> 1) * 8;
            const unsigned char *src = p.src + ((size_t)f * p.h + y0) * row + x0 * 3;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const uint2 *q = reinterpret_cast<const uint2 *>(src + r * row);
                const uint2 a = q[0], b = q[1], c = q[2];
                const unsigned wv[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
#pragma unroll
                for (int x = 0; x < 8; ++x) {
                    const int R = byte_of(wv, 3 * x), G = byte_of(wv, 3 * x + 1), B = byte_of(wv, 3 * x + 2);
                    s[r * 8 + x] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
                }
            }
        } else {
            const int u = t - ny, m = u >> 1, cr = u & 1;
            g = m * 6 + 4 + cr;
            tab = 1;
            // jccolor.c: Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16, Cr = (32768 R - 27439 G - 5329 B + ...) >> 16
            const int kr = cr ? 32768 : -11059, kg = cr ? -27439 : -21709, kb = cr ? -5329 : 32768;
            const int x0 = (m % p.mcux) * 16, y0 = (m / p.mcux) * 16;
            const unsigned char *src = p.src + ((size_t)f * p.h + y0) * row + x0 * 3;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                int sum[8];
#pragma unroll
                for (int x = 0; x < 8; ++x) sum[x] = 0;
#pragma unroll
                for (int rr = 0; rr < 2; ++rr) {
                    const uint4 *q = reinterpret_cast<const uint4 *>(src + (2 * r + rr) * row);
                    const uint4 a = q[0], b = q[1], c = q[2];
                    const unsigned wv[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
                    for (int x = 0; x < 16; ++x) {
                        const int R = byte_of(wv, 3 * x), G = byte_of(wv, 3 * x + 1), B = byte_of(wv, 3 * x + 2);
                        sum[x >> 1] += (kr * R + kg * G + kb * B + (128 << 16) + 32767) >> 16;
                    }
                }
                // jcsample.c h2v2_downsample: bias 1, 2, 1, 2 ... from the start of every output row (block columns start even)
#pragma unroll
                for (int x = 0; x < 8; ++x) s[r * 8 + x] = ((sum[x] + 1 + (x & 1)) >> 2) - 128;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct_pass<true, 1>(s + r * 8);
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct_pass<false, 8>(s + c);
    // quantise (round half away from zero), zigzag order
    int z[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int v = s[kNatural[k]];
        const unsigned d = p.div[tab][kNatural[k]];
        const unsigned a = ((unsigned)(v < 0 ? -v : v) + (d >> 1)) / d;
        z[k] = v < 0 ? -(int)a : (int)a;
    }
    uint4 *out = reinterpret_cast<uint4 *>(p.coef + ((size_t)f * p.nblk + g) * 64);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int *zz = z + k * 8;
        out[k] = make_uint4((zz[0] & 0xffff) | ((unsigned)zz[1] << 16), (zz[2] & 0xffff) | ((unsigned)zz[3] << 16),
                            (zz[4] & 0xffff) | ((unsigned)zz[5] << 16), (zz[6] & 0xffff) | ((unsigned)zz[7] << 16));
    }
    if constexpr (!kOpts) {                 // (with options the tables, or the interval the block is in, are not known yet: jpeg_tables)
        const Codes &ac = kCodes[2 * tab + 1];
        const unsigned zrl = ac.v[0xf0] >> 16, eob = ac.v[0x00] >> 16;
        unsigned bits = 0;
        int run = 0;
#pragma unroll
        for (int k = 1; k < 64; ++k) {
            if (z[k] == 0) {
                ++run;
            } else {
                while (run > 15) {
                    bits += zrl;
                    run -= 16;
                }
                const int nb = nbits(z[k]);
                bits += (ac.v[(run << 4) | nb] >> 16) + nb;
                run = 0;
            }
        }
        if (run) bits += eob;
        p.acbits[(size_t)f * p.nblk + g] = bits;
    }
}

// ---- 1'. the same for a format handle of any geometry ----------------------------------------------------------------------------------
// jccolor.c: one converted sample of component `comp` (0 Y, 1 Cb, 2 Cr) from the three bytes at px
__device__ __forceinline__ int ycc_sample(const unsigned char *px, int comp)
{
    const int R = px[0], G = px[1], B = px[2];
    if (comp == 0) return (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    const int kr = comp == 2 ? 32768 : -11059, kg = comp == 2 ? -27439 : -21709, kb = comp == 2 ? -5329 : 32768;
    return (kr * R + kg * G + kb * B + (128 << 16) + 32767) >> 16;
}

// The 64 level-shifted samples of a chroma block under luma factors (HS, VS).  jcsample.c / jcprepct.c at the edges: pixel columns repeat the
// last one BEFORE the box (the bias pattern runs on from column 0 of the plane: block columns start even), pixel rows repeat the last one up to a
// multiple of VS only, and below that the last row of the COMPONENT plane repeats: the row index is clamped in the plane, then in the picture.
template <int HS, int VS>
__device__ __forceinline__ void chroma_samples(const lspgeom::Geom &G, const lspgeom::Block &b, const unsigned char *src, int (&s)[64])
{
    const int crows = lspgeom::ceil_div(G.h, VS);
    const size_t row = (size_t)G.w * 3;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int cy = min(b.by * 8 + r, crows - 1);
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int cx = b.bx * 8 + x;
            int sum = 0;
#pragma unroll
            for (int rr = 0; rr < VS; ++rr) {
                const unsigned char *line = src + (size_t)min(cy * VS + rr, G.h - 1) * row;
#pragma unroll
                for (int cc = 0; cc < HS; ++cc) sum += ycc_sample(line + (size_t)min(cx * HS + cc, G.w - 1) * 3, b.comp);
            }
            if (HS == 2 && VS == 2)
                sum = (sum + 1 + (x & 1)) >> 2;                 // h2v2_downsample: bias 1, 2, 1, 2 ...
            else if (HS == 2)
                sum = (sum + (x & 1)) >> 1;                     // h2v1_downsample: bias 0, 1, 0, 1 ...
            s[r * 8 + x] = sum - 128;
        }
    }
}

// Thread per coded block in coding order, dummy blocks included (zero coefficients: their DC is resolved where the differences are formed).  Pixels
// are read byte by byte at clamped coordinates: with an odd width neither a row nor a frame of the batch starts on an aligned address.
__global__ __launch_bounds__(NT) void jpeg_transform_geom(GeomParams p)
{
    const int f = blockIdx.y;
    const int g = blockIdx.x * NT + threadIdx.x;
    if (g >= p.nblk) return;
    const lspgeom::Geom &G = p.geo;
    const lspgeom::Block b = lspgeom::block_of(G, g);
    short *dst = p.coef + ((size_t)f * p.nblk + g) * 64;
    if (b.dummy) {
        uint4 *out = reinterpret_cast<uint4 *>(dst);
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const unsigned char *src = p.src + (size_t)f * G.h * G.w * G.comps;
    int s[64];
    if (b.comp == 0) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const unsigned char *line = src + (size_t)min(b.by * 8 + r, G.h - 1) * G.w * G.comps;
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const int px = min(b.bx * 8 + x, G.w - 1);
                s[r * 8 + x] = (G.comps == 1 ? (int)line[px] : ycc_sample(line + (size_t)px * 3, 0)) - 128;
            }
        }
    } else if (G.vs == 2) {
        chroma_samples<2, 2>(G, b, src, s);
    } else if (G.hs == 2) {
        chroma_samples<2, 1>(G, b, src, s);
    } else {
        chroma_samples<1, 1>(G, b, src, s);
    }
    int z[64];
    dct_quantise_store(s, p.div[b.comp ? 1 : 0], z, dst);
}

__device__ __forceinline__ int dc_diff(const Params &p, int f, int g)
{
    const short *c = p.coef + (size_t)f * p.nblk * 64;
    const int pg = prev_block(g, p.comps);
    return (int)c[(size_t)g * 64] - (pg >= 0 ? (int)c[(size_t)pg * 64] : 0);
}

// ---- 2. bit offsets per block, frame totals, zeroed stream words ---------------------------------------------------------------
__global__ __launch_bounds__(NS) void jpeg_offsets(Params p)
{
    __shared__ unsigned lds[NS / 64 + 1];
    const int f = blockIdx.x;
    unsigned carry = 0;
    for (int base = 0; base < p.nblk; base += NS) {
        const int g = base + threadIdx.x;
        unsigned b = 0;
        if (g < p.nblk) {
            const int nb = nbits(dc_diff(p, f, g));
            b = p.acbits[(size_t)f * p.nblk + g] + (kCodes[2 * table_of(g, p.comps)].v[nb] >> 16) + nb;
        }
        unsigned tot;
        const unsigned ex = block_scan(b, lds, &tot);
        if (g < p.nblk) p.offsets[(size_t)f * p.nblk + g] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) p.totals[f] = carry;
    unsigned *w = p.words + (size_t)f * p.wcap;
    const unsigned nw = (carry + 31) / 32;
    for (unsigned i = threadIdx.x; i < nw; i += NS) w[i] = 0u;
}

// ---- 2'. with options: histograms, tables, DHT .. SOS, bit offsets per block, byte offsets per interval ------------------------------
__device__ __forceinline__ int dc_diff_opts(const OptParams &p, int f, int g)              // the prediction starts again in every interval
{
    const short *c = p.coef + (size_t)f * p.nblk * 64;
    const int pg = lspenc::pred_block(g, p.ibl, p.bpm);
    return (int)c[(size_t)g * 64] - (pg >= 0 ? (int)c[(size_t)pg * 64] : 0);
}

// the same on the grid of jpegenc_geom.h; a dummy block's DC is read where its chain of copies starts (dc_src), on both sides of the difference
__device__ __forceinline__ int dc_diff_opts(const GeomParams &p, int f, int g)
{
    const short *c = p.coef + (size_t)f * p.nblk * 64;
    const lspgeom::Block b = lspgeom::block_of(p.geo, g);
    const int pg = lspgeom::pred_block(b, g, p.ibl);
    return (int)c[(size_t)b.dc_src * 64] - (pg >= 0 ? (int)c[(size_t)lspgeom::block_of(p.geo, pg).dc_src * 64] : 0);
}

// fn(symbol) for every AC symbol of a block, in scan order: (run << 4) | size, 0xF0 (ZRL), 0x00 (EOB); jchuff.c encode_one_block / htest_one_block
template <class F>
__device__ __forceinline__ void for_ac_symbols(const uint4 *in, F &&fn)
{
    int run = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint4 v4 = in[q];
        const unsigned wv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (q == 0 && e == 0) continue;                     // DC
            const int v = (int)(short)(wv[e >> 1] >> ((e & 1) * 16));
            if (v == 0) {
                ++run;
                continue;
            }
            while (run > 15) {
                fn(0xf0);
                run -= 16;
            }
            fn((run << 4) | nbits(v));
            run = 0;
        }
    }
    if (run) fn(0);
}

// the minimum of a 64-bit key over the wave, in every lane
struct WaveMin {
    __device__ __forceinline__ uint64_t operator()(uint64_t k) const
    {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t y = (uint64_t)__shfl_xor((unsigned long long)k, o, 64);
            k = y < k ? y : k;
        }
        return k;
    }
};

// Workgroup per frame.  With optimize: (a) the symbol counts of the scan per table in LDS (a thread keeps its EOB count to itself until the end:
// nearly every block has one); (b) one wave per table merges (jpegenc_core.h huff_merge), one lane per table lists the symbols and assigns
// the codes; (c) all threads write DHT per table, DRI, SOS at the start of the frame's bytes.  Without: the Annex K codes.  Then, as jpeg_offsets,
// (d) the bits of every block and their exclusive scan S, (e) per interval ceil((S[end] - S[begin]) / 8) bytes and their scan, and the zeroed
// stream words.  jpeg_emit puts block g of interval i at bit 8 * istart[i] + S[g] - S[begin of i].
template <class P>                                              // OptParams, or GeomParams for the grid of jpegenc_geom.h
__device__ __forceinline__ void tables_body(const P p)
{
    __shared__ unsigned lds[NS / 64 + 1];
    __shared__ unsigned codes[4][256];
    __shared__ unsigned hist[4][256];
    __shared__ uint16_t csize[4][lspenc::kSymbols + 3];
    __shared__ unsigned char tbits[4][20], tvals[4][256];
    __shared__ int tn[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int ntab = p.comps == 3 ? 4 : 2;
    const short *coef = p.coef + (size_t)f * p.nblk * 64;
    unsigned char *dst = p.dst + (size_t)f * p.cap;
    if (p.optimize) {
        for (int i = tid; i < 4 * 256; i += NS) hist[i >> 8][i & 255] = 0u;
        __syncthreads();
        unsigned eob[2] = {0u, 0u};
        for (int g = tid; g < p.nblk; g += NS) {
            const int tab = table_of(p, g);
            atomicAdd(&hist[2 * tab][nbits(dc_diff_opts(p, f, g))], 1u);
            unsigned *h = hist[2 * tab + 1];
            unsigned e = 0;
            for_ac_symbols(reinterpret_cast<const uint4 *>(coef + (size_t)g * 64), [&](int s) {
                if (s)
                    atomicAdd(h + s, 1u);
                else
                    ++e;
            });
            eob[tab] += e;
        }
        if (eob[0]) atomicAdd(&hist[1][0], eob[0]);
        if (eob[1]) atomicAdd(&hist[3][0], eob[1]);
        __syncthreads();
        if ((tid >> 6) < ntab) lspenc::huff_merge<64>(hist[tid >> 6], tid & 63, csize[tid >> 6], WaveMin());
        __syncthreads();
        if (tid < ntab) {
            tn[tid] = lspenc::huff_finish(csize[tid], tbits[tid], tvals[tid]);
            lspenc::huff_codes(tbits[tid], tvals[tid], codes[tid]);
        }
        __syncthreads();
        int at = 0;
        for (int t = 0; t < ntab; ++t) {                        // jcmarker.c emit_dht: DC0, AC0, DC1, AC1, a segment each
            const int n = tn[t];
            for (int i = tid; i < 21 + n; i += NS) {
                const int len = 19 + n;
                dst[at + i] = i == 0 ? 0xff : i == 1 ? 0xc4 : i == 2 ? (unsigned char)(len >> 8) : i == 3 ? (unsigned char)len
                            : i == 4 ? (unsigned char)(((t & 1) << 4) | (t >> 1)) : i < 21 ? tbits[t][i - 4] : tvals[t][i - 21];
            }
            at += 21 + n;
        }
        if (tid == 0) {
            unsigned char *o = dst + at;
            if (p.restart > 0) {
                const unsigned char dri[6] = {0xff, 0xdd, 0, 4, (unsigned char)(p.restart >> 8), (unsigned char)p.restart};
                for (int i = 0; i < 6; ++i) *o++ = dri[i];
            }
            *o++ = 0xff;
            *o++ = 0xda;
            *o++ = 0;
            *o++ = (unsigned char)(6 + 2 * p.comps);
            *o++ = (unsigned char)p.comps;
            for (int c = 0; c < p.comps; ++c) {
                *o++ = (unsigned char)(c + 1);
                *o++ = c == 0 ? 0x00 : 0x11;
            }
            *o++ = 0;
            *o++ = 63;
            *o++ = 0;
            p.prelen[f] = (unsigned)(o - dst);
        }
    } else {
        for (int i = tid; i < ntab * 256; i += NS) codes[i >> 8][i & 255] = kCodes[i >> 8].v[i & 255];
        if (tid == 0) p.prelen[f] = 0u;
        __syncthreads();
    }
    for (int i = tid; i < ntab * 256; i += NS) p.codes[(size_t)f * 1024 + i] = codes[i >> 8][i & 255];
    // (d)
    unsigned *S = p.offsets + (size_t)f * p.nblk;
    unsigned carry = 0;
    for (int base = 0; base < p.nblk; base += NS) {
        const int g = base + tid;
        unsigned b = 0;
        if (g < p.nblk) {
            const int tab = table_of(p, g);
            const int nb = nbits(dc_diff_opts(p, f, g));
            b = (codes[2 * tab][nb] >> 16) + nb;
            const unsigned *ac = codes[2 * tab + 1];
            for_ac_symbols(reinterpret_cast<const uint4 *>(coef + (size_t)g * 64), [&](int s) { b += (ac[s] >> 16) + (s & 15); });
        }
        unsigned tot;
        const unsigned ex = block_scan(b, lds, &tot);
        if (g < p.nblk) S[g] = carry + ex;
        carry += tot;
    }
    __syncthreads();                                            // S is read across the workgroup below
    // (e)
    unsigned *ist = p.istart + (size_t)f * (p.nint + 1);
    unsigned bytes = 0;
    for (int base = 0; base < p.nint; base += NS) {
        const int i = base + tid;
        unsigned b = 0;
        if (i < p.nint) {
            const int e = lspenc::interval_end(i, p.ibl, p.nblk);
            b = lspenc::padded_bytes((e == p.nblk ? carry : S[e]) - S[(size_t)i * p.ibl]);
        }
        unsigned tot;
        const unsigned ex = block_scan(b, lds, &tot);
        if (i < p.nint) ist[i] = bytes + ex;
        bytes += tot;
    }
    if (tid == 0) ist[p.nint] = bytes;
    unsigned *w = p.words + (size_t)f * p.wcap;
    const unsigned nw = (bytes + 3) / 4;
    for (unsigned i = tid; i < nw; i += NS) w[i] = 0u;
}

__global__ __launch_bounds__(NS) void jpeg_tables(OptParams p) { tables_body(p); }
__global__ __launch_bounds__(NS) void jpeg_tables_geom(GeomParams p) { tables_body(p); }

// ---- 3. the symbols of every block at its offset ---------------------------------------------------------------------------------
struct BitWriter {
    unsigned *w;
    unsigned idx;
    int n;                                  // pending bits in the low end of acc
    unsigned long long acc;
    __device__ __forceinline__ void put(unsigned v, int len)    // len <= 27
    {
        acc = (acc << len) | v;
        n += len;
        if (n >= 32) {
            n -= 32;
            atomicOr(w + idx, (unsigned)(acc >> n));
            ++idx;
        }
    }
    __device__ __forceinline__ void flush()
    {
        if (n > 0) atomicOr(w + idx, (unsigned)(acc << (32 - n)));
    }
};

__device__ __forceinline__ unsigned value_bits(int v, int nb) { return (unsigned)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u); }

template <bool kOpts, class P>
__device__ __forceinline__ void emit_body(const P p)
{
    const int f = blockIdx.y;
    const int g = blockIdx.x * NT + threadIdx.x;
    if (g >= p.nblk) return;
    const int tab = table_of(p, g);
    unsigned off;
    int diff;
    const unsigned *dc, *acv;
    if constexpr (kOpts) {
        const unsigned *S = p.offsets + (size_t)f * p.nblk;
        const int i = lspenc::interval_of(g, p.ibl);
        off = 8u * p.istart[(size_t)f * (p.nint + 1) + i] + S[g] - S[(size_t)i * p.ibl];
        diff = dc_diff_opts(p, f, g);
        dc = p.codes + (size_t)f * 1024 + 2 * tab * 256;
        acv = dc + 256;
    } else {
        off = p.offsets[(size_t)f * p.nblk + g];
        diff = dc_diff(p, f, g);
        dc = kCodes[2 * tab].v;
        acv = kCodes[2 * tab + 1].v;
    }
    BitWriter bw{p.words + (size_t)f * p.wcap, off >> 5, (int)(off & 31), 0ull};
    int nb = nbits(diff);
    unsigned c = dc[nb];
    bw.put(((c & 0xffffu) << nb) | value_bits(diff, nb), (int)(c >> 16) + nb);
    const uint4 *in = reinterpret_cast<const uint4 *>(p.coef + ((size_t)f * p.nblk + g) * 64);
    int run = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint4 v4 = in[q];
        const unsigned wv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (q == 0 && e == 0) continue;                     // DC
            const int v = (int)(short)(wv[e >> 1] >> ((e & 1) * 16));
            if (v == 0) {
                ++run;
                continue;
            }
            while (run > 15) {
                const unsigned z = acv[0xf0];
                bw.put(z & 0xffffu, (int)(z >> 16));
                run -= 16;
            }
            nb = nbits(v);
            c = acv[(run << 4) | nb];
            bw.put(((c & 0xffffu) << nb) | value_bits(v, nb), (int)(c >> 16) + nb);
            run = 0;
        }
    }
    if (run) {
        c = acv[0x00];
        bw.put(c & 0xffffu, (int)(c >> 16));
    }
    if constexpr (kOpts) {                                      // jchuff.c flush_bits: the interval's last byte is filled with 1-bits here
        if (g + 1 == lspenc::interval_end(lspenc::interval_of(g, p.ibl), p.ibl, p.nblk)) {
            const unsigned pad = lspenc::pad_bits((unsigned)bw.n);
            if (pad) bw.put((1u << pad) - 1u, (int)pad);
        }
    }
    bw.flush();
}

template <bool kOpts>
__global__ __launch_bounds__(NT) void jpeg_emit(ParamsOf<kOpts> p) { emit_body<kOpts>(p); }
__global__ __launch_bounds__(NT) void jpeg_emit_geom(GeomParams p) { emit_body<true>(p); }

// ---- 4. bytes, padding, stuffing, EOI ---------------------------------------------------------------------------------------------
// With options the stream arrives padded per interval (jpeg_emit), starts behind the frame's DHT .. SOS, and RSTn follows the last byte of every
// interval but the last, behind that byte's own stuffing (jchuff.c emit_restart).
template <bool kOpts>
__global__ __launch_bounds__(NS) void jpeg_stuff(ParamsOf<kOpts> p)
{
    __shared__ unsigned lds[NS / 64 + 1];
    const int f = blockIdx.x;
    int nbytes;
    unsigned pad = 0, carry = 0;                                // pad: 1-bits that fill the last byte
    const unsigned *ist = nullptr;
    if constexpr (kOpts) {
        ist = p.istart + (size_t)f * (p.nint + 1);
        nbytes = (int)ist[p.nint];
        carry = p.prelen[f];
    } else {
        const unsigned total = p.totals[f];
        nbytes = (int)((total + 7) / 8);
        pad = (8u - (total & 7u)) & 7u;
    }
    const unsigned *w = p.words + (size_t)f * p.wcap;
    unsigned char *dst = p.dst + (size_t)f * p.cap;
    for (int base = 0; base < nbytes; base += NS * 16) {
        const int i0 = base + threadIdx.x * 16;
        const int valid = min(max(nbytes - i0, 0), 16);
        unsigned wv[4] = {0u, 0u, 0u, 0u};
        if (valid > 0) {
            const uint4 v = *reinterpret_cast<const uint4 *>(w + i0 / 4);
            wv[0] = v.x;
            wv[1] = v.y;
            wv[2] = v.z;
            wv[3] = v.w;
        }
        unsigned char b[16];
        unsigned cnt = 0;
        unsigned ends = 0;                                      // bit k: byte k of the chunk is the last of an interval that a marker follows
        int iv = 0;                                             // the interval of the chunk's first byte
        if constexpr (kOpts) {
            if (valid > 0 && p.nint > 1) {
                int lo = 0, hi = p.nint - 1;                    // the first interval that ends behind byte i0 (no interval is empty)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (ist[mid + 1] > (unsigned)i0)
                        hi = mid;
                    else
                        lo = mid + 1;
                }
                iv = lo;
                int kk = iv;
                for (int k = 0; k < valid && kk < p.nint - 1; ++k) {
                    if (ist[kk + 1] == (unsigned)(i0 + k + 1)) {
                        ends |= 1u << k;
                        ++kk;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            unsigned x = (wv[k >> 2] >> (24 - 8 * (k & 3))) & 0xffu;             // the stream is MSB first within each word
            if constexpr (!kOpts)
                if (i0 + k == nbytes - 1) x |= (1u << pad) - 1u;
            b[k] = (unsigned char)x;
            cnt += k < valid ? 1u + (x == 0xffu) : 0u;
        }
        if constexpr (kOpts) cnt += 2u * (unsigned)__popc(ends);
        unsigned tot;
        const unsigned ex = block_scan(cnt, lds, &tot);
        unsigned char *o = dst + carry + ex;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k < valid) {
                *o++ = b[k];
                if (b[k] == 0xffu) *o++ = 0;
                if constexpr (kOpts) {
                    if ((ends >> k) & 1u) {
                        *o++ = 0xff;
                        *o++ = lspenc::rst_marker((unsigned)iv++);
                    }
                }
            }
        }
        carry += tot;
    }
    if (threadIdx.x == 0) {
        dst[carry] = 0xff;
        dst[carry + 1] = 0xd9;
        p.sizes[f] = carry + 2;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace lspjpeg

using namespace lspjpeg;

struct lspjpeg_handle {
    int w, h, comps, quality;
    int mcux, nmcu, nblk, wcap;             // MCUs per row, MCUs and blocks per frame, stream words per frame
    size_t cap;
    unsigned short div[2][64];
    std::vector<unsigned char> header;
    bool opts;                              // made with optimize or a restart interval: the *<true> instances and jpeg_tables
    int optimize, restart, nint, ibl, bpm;
    int hs, vs;                             // luma sampling factors
    bool general;                           // a format handle of another geometry than lspjpeg_create's: the *_geom instances
    lspgeom::Geom geo;
};

namespace {

void put16(std::vector<unsigned char> &v, int x)
{
    v.push_back((unsigned char)(x >> 8));
    v.push_back((unsigned char)x);
}

// SOI .. SOS as libjpeg writes them (jcmarker.c): APP0 JFIF 1.01 (units 0, density 1x1), one DQT per table, SOF0, DHT DC0 AC0 [DC1 AC1], [DRI], SOS;
// SOI .. SOF0 for a handle with optimize
void build_header(lspjpeg_handle *h, const unsigned char (&q)[2][64])
{
    std::vector<unsigned char> &v = h->header;
    const int ntab = h->comps == 3 ? 2 : 1;
    const unsigned char app0[] = {0xff, 0xd8, 0xff, 0xe0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00};
    v.assign(app0, app0 + sizeof(app0));
    for (int t = 0; t < ntab; ++t) {
        v.push_back(0xff);
        v.push_back(0xdb);
        put16(v, 67);
        v.push_back((unsigned char)t);
        for (int k = 0; k < 64; ++k) v.push_back(q[t][kNatural[k]]);
    }
    v.push_back(0xff);
    v.push_back(0xc0);
    put16(v, 8 + 3 * h->comps);
    v.push_back(8);
    put16(v, h->h);
    put16(v, h->w);
    v.push_back((unsigned char)h->comps);
    for (int c = 0; c < h->comps; ++c) {
        v.push_back((unsigned char)(c + 1));
        v.push_back(c == 0 ? (unsigned char)(h->hs << 4 | h->vs) : 0x11);
        v.push_back(c == 0 ? 0 : 1);
    }
    if (h->optimize) return;                // DHT, DRI and SOS are the frame's own
    const unsigned char *vals[4] = {kDcVals, kAcLumaVals, kDcVals, kAcChromaVals};
    for (int t = 0; t < 2 * ntab; ++t) {
        int n = 0;
        for (int l = 0; l < 16; ++l) n += kBits[t][l];
        v.push_back(0xff);
        v.push_back(0xc4);
        put16(v, 3 + 16 + n);
        v.push_back((unsigned char)(((t & 1) << 4) | (t >> 1)));
        v.insert(v.end(), kBits[t], kBits[t] + 16);
        v.insert(v.end(), vals[t], vals[t] + n);
    }
    if (h->restart > 0) {                   // jcmarker.c write_scan_header: DRI between the tables and SOS
        v.push_back(0xff);
        v.push_back(0xdd);
        put16(v, 4);
        put16(v, h->restart);
    }
    v.push_back(0xff);
    v.push_back(0xda);
    put16(v, 6 + 2 * h->comps);
    v.push_back((unsigned char)h->comps);
    for (int c = 0; c < h->comps; ++c) {
        v.push_back((unsigned char)(c + 1));
        v.push_back(c == 0 ? 0x00 : 0x11);
    }
    v.push_back(0);
    v.push_back(63);
    v.push_back(0);
}

}  // namespace

extern "C" {

const char *lspjpeg_last_error(void) { return g_err.c_str(); }

// everything of a handle that does not depend on how its MCU grid is laid out: intervals, buffer sizes, tables, header
static void finish(lspjpeg_handle *h, int quality, int optimize, int restart)
{
    h->quality = quality;
    h->optimize = optimize;
    h->restart = restart;
    h->opts = optimize || restart > 0;
    h->nint = lspenc::interval_count(h->nmcu, restart);
    h->ibl = lspenc::interval_blocks(h->nmcu, restart, h->bpm);
    if (h->opts || h->general) {            // (the *_geom instances lay the stream out as a handle with options does)
        const size_t bytes = (size_t)lspenc::stream_bytes_bound((uint64_t)h->nblk, (uint64_t)h->nint, optimize ? lspenc::kBlockBitsOpt : lspenc::kBlockBitsStd);
        h->wcap = (int)(((bytes + 3) / 4 + 1 + 3) & ~(size_t)3);
        h->cap = (size_t)lspenc::capacity_bound((uint64_t)h->nblk, (uint64_t)h->nint, optimize);
    }
    if (!h->opts) {                         // no options: the bound of lspjpeg_create, whatever the geometry
        const size_t bits = (size_t)h->nblk * LSPJPEG_BLOCK_BITS;
        if (!h->general) h->wcap = (int)(((bits + 31) / 32 + 1 + 3) & ~(size_t)3);
        h->cap = 2 * ((bits + 7) / 8) + 2;
    }
    // jcparam.c jpeg_quality_scaling + jpeg_add_quant_table(force_baseline = TRUE)
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    unsigned char q[2][64];
    for (int k = 0; k < 64; ++k) {
        const int base[2] = {kLumaQ[k], kChromaQ[k]};
        for (int t = 0; t < 2; ++t) {
            int v = (base[t] * scale + 50) / 100;
            v = v < 1 ? 1 : v > 255 ? 255 : v;
            q[t][k] = (unsigned char)v;
            h->div[t][k] = (unsigned short)(v << 3);
        }
    }
    build_header(h, q);
}

static int create(int width, int height, int components, int quality, int optimize, int restart, lspjpeg_handle **out)
{
    if (components != 1 && components != 3) return fail(LSPJPEG_ERR_UNSUPPORTED, "components must be 3 (RGB, 4:2:0) or 1 (grayscale)");
    if (quality < 1 || quality > 100) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "quality must be in 1..100");
    const int m = components == 3 ? 16 : 8;
    if (width < m || height < m || width % m || height % m || width > LSPJPEG_MAX_SIDE || height > LSPJPEG_MAX_SIDE)
        return fail(LSPJPEG_ERR_UNSUPPORTED, "width and height must be multiples of " + std::to_string(m) + " in " + std::to_string(m) + ".." +
                                                 std::to_string(LSPJPEG_MAX_SIDE) + " (got " + std::to_string(width) + "x" + std::to_string(height) + ")");
    lspjpeg_handle *h = new lspjpeg_handle();
    h->w = width;
    h->h = height;
    h->comps = components;
    h->mcux = width / m;
    h->nmcu = h->mcux * (height / m);
    h->nblk = h->nmcu * (components == 3 ? 6 : 1);
    h->bpm = components == 3 ? 6 : 1;
    h->hs = h->vs = components == 3 ? 2 : 1;
    h->general = false;
    finish(h, quality, optimize, restart);
    *out = h;
    return LSPJPEG_OK;
}
int lspjpeg_create(int width, int height, int components, int quality, lspjpeg_handle **out)
{
    if (!out) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    return create(width, height, components, quality, 0, 0, out);
}

int lspjpeg_create_opts(const lspjpeg_options *o, lspjpeg_handle **out)
{
    if (!out) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    if (!o) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "null options");
    if (o->abi_version != LSPJPEG_ABI_VERSION)
        return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "lspjpeg_options.abi_version is " + std::to_string(o->abi_version) + ", this library speaks " + std::to_string(LSPJPEG_ABI_VERSION));
    if (o->optimize != 0 && o->optimize != 1) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "optimize must be 0 or 1");
    if (o->restart_interval < 0 || o->restart_interval > 65535) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "restart_interval must be in 0..65535 MCUs");
    return create(o->width, o->height, o->components, o->quality, o->optimize, o->restart_interval, out);
}

// the refusals of lspjpeg_create_format, in the order include/lspjpeg.h states them; *g receives the grid
static int check_format(const lspjpeg_format *f, lspgeom::Geom *g)
{
    if (!f) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "null format");
    if (f->abi_version != LSPJPEG_FORMAT_ABI_VERSION)
        return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "lspjpeg_format.abi_version is " + std::to_string(f->abi_version) + ", this library speaks " + std::to_string(LSPJPEG_FORMAT_ABI_VERSION));
    if (f->components != 1 && f->components != 3) return fail(LSPJPEG_ERR_UNSUPPORTED, "components must be 3 (RGB) or 1 (grayscale)");
    if (f->quality < 1 || f->quality > 100) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "quality must be in 1..100");
    if (f->width < 1 || f->height < 1 || f->width > LSPJPEG_MAX_SIDE || f->height > LSPJPEG_MAX_SIDE)
        return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "width and height must be in 1.." + std::to_string(LSPJPEG_MAX_SIDE) + " (got " + std::to_string(f->width) + "x" + std::to_string(f->height) + ")");
    if (f->optimize != 0 && f->optimize != 1) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "optimize must be 0 or 1");
    if (f->restart_interval < 0 || f->restart_interval > 65535) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "restart_interval must be in 0..65535 MCUs");
    if (f->h_samp < 1 || f->h_samp > 4 || f->v_samp < 1 || f->v_samp > 4) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "h_samp and v_samp must be in 1..4");
    const bool one = f->h_samp == 1 && f->v_samp == 1;
    if (f->components == 1 && !one) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "a grayscale frame has sampling factors (1, 1)");
    if (!one && !(f->h_samp == 2 && f->v_samp <= 2))
        return fail(LSPJPEG_ERR_UNSUPPORTED, "luma sampling factors must be (2, 2) 4:2:0, (2, 1) 4:2:2 or (1, 1) 4:4:4 (got (" + std::to_string(f->h_samp) + ", " + std::to_string(f->v_samp) + "))");
    *g = lspgeom::make_geom(f->width, f->height, f->components, f->h_samp, f->v_samp);
    if ((uint64_t)g->nblk * lspenc::kBlockBitsOpt > 0xffffffffull)
        return fail(LSPJPEG_ERR_UNSUPPORTED, std::to_string(g->nblk) + " blocks per frame: their worst-case bits do not fit the 32-bit offsets of a frame");
    return LSPJPEG_OK;
}

int lspjpeg_create_format(const lspjpeg_format *f, lspjpeg_handle **out)
{
    if (!out) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    lspgeom::Geom g;
    const int rc = check_format(f, &g);
    if (rc) return rc;
    // the geometry of lspjpeg_create: that handle, with the kernels it has always run
    const int m = g.comps == 3 ? 16 : 8;
    if ((g.comps == 1 || (g.hs == 2 && g.vs == 2)) && g.w % m == 0 && g.h % m == 0) return create(g.w, g.h, g.comps, f->quality, f->optimize, f->restart_interval, out);
    lspjpeg_handle *h = new lspjpeg_handle();
    h->w = g.w;
    h->h = g.h;
    h->comps = g.comps;
    h->mcux = g.mcux;
    h->nmcu = g.nmcu;
    h->nblk = g.nblk;
    h->bpm = g.bpm;
    h->hs = g.hs;
    h->vs = g.vs;
    h->general = true;
    h->geo = g;
    finish(h, f->quality, f->optimize, f->restart_interval);
    *out = h;
    return LSPJPEG_OK;
}

int64_t lspjpeg_host_block_map(const lspjpeg_format *f, int32_t *map, size_t cap_blocks)
{
    lspgeom::Geom g;
    const int rc = check_format(f, &g);
    if (rc) return rc;
    if (map) {
        if (cap_blocks < (size_t)g.nblk) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "the map needs room for " + std::to_string(g.nblk) + " blocks");
        for (int i = 0; i < g.nblk; ++i) {
            const lspgeom::Block b = lspgeom::block_of(g, i);
            const int32_t row[6] = {b.comp, b.bx, b.by, b.dummy, b.prev, b.dc_src};
            std::copy(row, row + 6, map + (size_t)i * 6);
        }
    }
    return g.nblk;
}

int lspjpeg_host_optimal_table(const uint32_t freq[256], unsigned char bits[17], unsigned char huffval[256], int *nsymbols)
{
    if (!freq || !bits || !huffval || !nsymbols) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "null argument");
    uint16_t codesize[lspenc::kSymbols];
    lspenc::huff_merge<1>(freq, 0, codesize, lspenc::OneLane());
    *nsymbols = lspenc::huff_finish(codesize, bits, huffval);
    return LSPJPEG_OK;
}

int lspjpeg_destroy(lspjpeg_handle *h)
{
    delete h;
    return LSPJPEG_OK;
}

int64_t lspjpeg_header(const lspjpeg_handle *h, unsigned char *buf, size_t cap)
{
    if (!h) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "null handle");
    if (buf) {
        if (cap < h->header.size()) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "header needs " + std::to_string(h->header.size()) + " bytes");
        std::copy(h->header.begin(), h->header.end(), buf);
    }
    return (int64_t)h->header.size();
}

size_t lspjpeg_capacity_bytes(const lspjpeg_handle *h) { return h ? h->cap : 0; }

static size_t workspace_layout(const lspjpeg_handle *h, int batch, size_t off[8])
{
    const size_t nb = (size_t)batch * h->nblk;
    size_t o = 0;
    off[0] = o; o = align256(o + nb * 64 * sizeof(short));
    off[1] = o; o = align256(o + nb * sizeof(unsigned));
    off[2] = o; o = align256(o + nb * sizeof(unsigned));
    off[3] = o; o = align256(o + (size_t)batch * sizeof(unsigned));
    off[4] = o; o = align256(o + (size_t)batch * h->wcap * sizeof(unsigned));
    if (h->opts || h->general) {
        off[5] = o; o = align256(o + (size_t)batch * 1024 * sizeof(unsigned));
        off[6] = o; o = align256(o + (size_t)batch * (h->nint + 1) * sizeof(unsigned));
        off[7] = o; o = align256(o + (size_t)batch * sizeof(unsigned));
    }
    return o;
}

size_t lspjpeg_workspace_bytes(const lspjpeg_handle *h, int batch)
{
    if (!h || batch < 1) return 0;
    size_t off[8];
    return workspace_layout(h, batch, off);
}

int lspjpeg_encode(const lspjpeg_handle *h, const unsigned char *src_dev, int batch, unsigned char *dst_dev, uint32_t *sizes_dev,
                   void *workspace_dev, size_t workspace_bytes, void *hip_stream)
{
    if (!h || !src_dev || !dst_dev || !sizes_dev || !workspace_dev) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "null argument");
    if (batch < 1 || batch > 65535) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "batch must be in 1..65535");
    // (the *_geom instances read bytes: a format handle of another geometry than lspjpeg_create's takes frames at any address)
    if ((!h->general && reinterpret_cast<uintptr_t>(src_dev) % 16) || reinterpret_cast<uintptr_t>(workspace_dev) % 256)
        return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "src_dev must be 16-byte aligned and workspace_dev 256-byte aligned");
    size_t off[8];
    const size_t need = workspace_layout(h, batch, off);
    if (workspace_bytes < need) return fail(LSPJPEG_ERR_INVALID_ARGUMENT, "workspace needs " + std::to_string(need) + " bytes");
    char *ws = static_cast<char *>(workspace_dev);
    GeomParams p{};
    p.src = src_dev;
    p.coef = reinterpret_cast<short *>(ws + off[0]);
    p.acbits = reinterpret_cast<unsigned *>(ws + off[1]);
    p.offsets = reinterpret_cast<unsigned *>(ws + off[2]);
    p.totals = reinterpret_cast<unsigned *>(ws + off[3]);
    p.words = reinterpret_cast<unsigned *>(ws + off[4]);
    p.dst = dst_dev;
    p.sizes = sizes_dev;
    p.w = h->w;
    p.h = h->h;
    p.comps = h->comps;
    p.mcux = h->mcux;
    p.nmcu = h->nmcu;
    p.nblk = h->nblk;
    p.wcap = h->wcap;
    p.cap = h->cap;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) p.div[t][k] = h->div[t][k];
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const dim3 per_block((h->nblk + NT - 1) / NT, batch);
    if (h->opts || h->general) {
        p.codes = reinterpret_cast<unsigned *>(ws + off[5]);
        p.istart = reinterpret_cast<unsigned *>(ws + off[6]);
        p.prelen = reinterpret_cast<unsigned *>(ws + off[7]);
        p.restart = h->restart;
        p.nint = h->nint;
        p.ibl = h->ibl;
        p.bpm = h->bpm;
        p.optimize = h->optimize;
        const OptParams &o = p;
        if (h->general) {                                       // (stuffing knows no geometry: the instance of a handle with options)
            p.geo = h->geo;
            hipLaunchKernelGGL(jpeg_transform_geom, per_block, dim3(NT), 0, st, p);
            hipLaunchKernelGGL(jpeg_tables_geom, dim3(batch), dim3(NS), 0, st, p);
            hipLaunchKernelGGL(jpeg_emit_geom, per_block, dim3(NT), 0, st, p);
            hipLaunchKernelGGL(jpeg_stuff<true>, dim3(batch), dim3(NS), 0, st, o);
        } else {
            hipLaunchKernelGGL(jpeg_transform<true>, per_block, dim3(NT), 0, st, o);
            hipLaunchKernelGGL(jpeg_tables, dim3(batch), dim3(NS), 0, st, o);
            hipLaunchKernelGGL(jpeg_emit<true>, per_block, dim3(NT), 0, st, o);
            hipLaunchKernelGGL(jpeg_stuff<true>, dim3(batch), dim3(NS), 0, st, o);
        }
    } else {
        const Params &q = p;
        hipLaunchKernelGGL(jpeg_transform<false>, per_block, dim3(NT), 0, st, q);
        hipLaunchKernelGGL(jpeg_offsets, dim3(batch), dim3(NS), 0, st, q);
        hipLaunchKernelGGL(jpeg_emit<false>, per_block, dim3(NT), 0, st, q);
        hipLaunchKernelGGL(jpeg_stuff<false>, dim3(batch), dim3(NS), 0, st, q);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LSPJPEG_ERR_HIP, std::string("jpeg launch: ") + hipGetErrorString(e));
    return LSPJPEG_OK;
}

}  // extern "C"
