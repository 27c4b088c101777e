// jpegenc_core.h -- the host/device half of the JPEG encoder's options (include/lspjpeg.h): the optimal Huffman table of a symbol histogram
// (libjpeg's jpeg_gen_optimal_table, restated from jchuff.c) and the bookkeeping of restart intervals.  Plain C++ with no allocation and no
// library calls: the kernels of jpeg.hip, lspjpeg_host_optimal_table and the stand-alone checker (jpegenc_check.cpp, built with sanitizers)
// run the SAME text.
//
// The table builder, as jchuff.c states it:
//   * a pseudo-symbol 256 of frequency 1 joins the histogram, so that no real symbol gets the all-ones code;
//   * the two least frequent live trees are merged until one is left; of equal frequencies the LARGER symbol number is taken (first for
//     c1, then for c2 among the rest); c1 keeps the sum, c2 leaves; every symbol of both trees gets one bit longer.  jchuff.c walks its
//     others[] chains to reach "every symbol of both trees"; here every symbol carries the number of its tree's root instead, which names
//     the same set;
//   * lengths above 16 are cut by the Annex K.2 adjustment on the counts per length; the pseudo-symbol's count leaves the longest length;
//   * the symbols are listed by their length BEFORE the adjustment and then by value, and the adjusted counts hand out the final lengths in
//     that order.
// Frequencies are added in 64 bits (jchuff.c uses long and treats 10^9 as infinity: no frame of at most 8192 x 8192 has that many blocks), and
// lengths above 32, where jchuff.c gives up (JERR_HUFF_CLEN_OVERFLOW), go through the same adjustment.
#ifndef LSPJPEGENC_CORE_H
#define LSPJPEGENC_CORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define LSPENC_HD __host__ __device__ __attribute__((always_inline))    // (two kernels call each function: inlined into both, as into the one before)
#define LSPENC_UNROLL _Pragma("unroll")
#else
#define LSPENC_HD
#define LSPENC_UNROLL
#endif

namespace lspenc {

constexpr int kSymbols = 257;                        // 256 real symbols and the pseudo-symbol
constexpr int kMaxLen = 256;                         // no tree over 257 leaves is deeper
constexpr uint64_t kDead = ~(uint64_t)0;

// ---- bit costs and byte bounds (the capacity argument of include/lspjpeg.h) -----------------------------------------------------------
constexpr int kBlockBitsStd = 1660;                  // Annex K tables: 11 + 11 bits of DC, 63 AC symbols of <= 16 + 10 bits
constexpr int kBlockBitsOpt = 1665;                  // optimised tables: a DC code can be 16 bits long
constexpr int kDcSymbols = 12, kAcSymbols = 162;     // categories 0..11; run 0..15 x size 1..10, EOB, ZRL: all a baseline scan can code
// DHT DC0 AC0 DC1 AC1 (marker, length, class / id, 16 counts, symbols), DRI, SOS of three components
constexpr int kPrefixBound = 2 * ((5 + 16 + kDcSymbols) + (5 + 16 + kAcSymbols)) + 6 + 14;

// MCUs per restart interval -> intervals per frame (interval 0 = none: the frame is one interval)
LSPENC_HD inline int interval_count(int nmcu, int restart) { return restart > 0 ? (nmcu + restart - 1) / restart : 1; }
// blocks per interval (the last one may be shorter)
LSPENC_HD inline int interval_blocks(int nmcu, int restart, int bpm) { return (restart > 0 && restart < nmcu ? restart : nmcu) * bpm; }
LSPENC_HD inline int interval_of(int g, int ibl) { return g / ibl; }
LSPENC_HD inline int interval_end(int i, int ibl, int nblk) { return (i + 1) * ibl < nblk ? (i + 1) * ibl : nblk; }   // first block past interval i
// the block whose DC value predicts block g's: the previous block of the same component INSIDE g's interval, -1 at its start
// (MCU = Y0 Y1 Y2 Y3 Cb Cr for bpm 6, one block for bpm 1)
LSPENC_HD inline int pred_block(int g, int ibl, int bpm)
{
    const int gi = g % ibl;
    if (bpm == 1) return gi ? g - 1 : -1;
    const int j = gi % 6;
    if (j >= 1 && j <= 3) return g - 1;
    if (gi < 6) return -1;
    return j == 0 ? g - 3 : g - 6;
}
LSPENC_HD inline uint32_t padded_bytes(uint32_t bits) { return (bits + 7u) >> 3; }
LSPENC_HD inline uint32_t pad_bits(uint32_t bits) { return (8u - (bits & 7u)) & 7u; }
LSPENC_HD inline unsigned char rst_marker(uint32_t i) { return (unsigned char)(0xd0u + (i & 7u)); }      // after interval i
// bytes of all intervals before stuffing: every interval is padded to a byte on its own
LSPENC_HD inline uint64_t stream_bytes_bound(uint64_t nblk, uint64_t nint, int block_bits) { return (nblk * (uint64_t)block_bits + 7) / 8 + nint; }
// what one frame can occupy in dst: stuffing at most doubles the padded bytes, 2 bytes of RSTn between intervals, EOI, and the tables
LSPENC_HD inline uint64_t capacity_bound(uint64_t nblk, uint64_t nint, int optimize)
{
    return (optimize ? (uint64_t)kPrefixBound : 0) + 2 * stream_bytes_bound(nblk, nint, optimize ? kBlockBitsOpt : kBlockBitsStd) + 2 * (nint - 1) + 2;
}

// ---- the merges ---------------------------------------------------------------------------------------------------------------------
// NL lanes share the 257 symbols: lane l owns symbols l, l + NL, ...  NL = 64 is one wave of the device, NL = 1 the host.  All that crosses
// lanes is the minimum of a key, which the caller supplies (`lanes_min(key)`: a wave-wide minimum in jpeg.hip, OneLane here); every lane then
// knows both trees and their frequencies and updates what it owns.
struct OneLane {
    LSPENC_HD uint64_t operator()(uint64_t k) const { return k; }
};

// key of a live tree: smaller frequency first, of equal ones the larger symbol
LSPENC_HD inline uint64_t merge_key(uint64_t freq, int sym) { return (freq << 9) | (uint64_t)(511 - sym); }

// freq[256] (the pseudo-symbol is added here); codesize[257] receives the length of every symbol before the 16-bit adjustment (0: unused).
// On the device all NL lanes of the wave call it with their lane; each writes the entries it owns.
template <int NL, class LanesMin>
LSPENC_HD inline void huff_merge(const uint32_t *freq, int lane, uint16_t *codesize, LanesMin lanes_min)
{
    constexpr int EPL = (kSymbols + NL - 1) / NL;
    uint64_t f[EPL];
    uint16_t root[EPL], len[EPL];
LSPENC_UNROLL
    for (int j = 0; j < EPL; ++j) {
        const int s = lane + j * NL;
        const uint64_t v = s < 256 ? freq[s] : s == 256 ? 1u : 0u;
        f[j] = v ? v : kDead;
        root[j] = (uint16_t)s;
        len[j] = 0;
    }
    for (;;) {
        uint64_t k1 = kDead;
LSPENC_UNROLL
        for (int j = 0; j < EPL; ++j) {
            const uint64_t k = f[j] == kDead ? kDead : merge_key(f[j], lane + j * NL);
            k1 = k < k1 ? k : k1;
        }
        k1 = lanes_min(k1);
        const int c1 = 511 - (int)(k1 & 511u);
        uint64_t k2 = kDead;
LSPENC_UNROLL
        for (int j = 0; j < EPL; ++j) {
            const uint64_t k = (f[j] == kDead || lane + j * NL == c1) ? kDead : merge_key(f[j], lane + j * NL);
            k2 = k < k2 ? k : k2;
        }
        k2 = lanes_min(k2);
        if (k2 == kDead) break;
        const int c2 = 511 - (int)(k2 & 511u);
LSPENC_UNROLL
        for (int j = 0; j < EPL; ++j) {
            const int s = lane + j * NL;
            if (s == c1) f[j] = (k1 >> 9) + (k2 >> 9);
            if (s == c2) f[j] = kDead;
            if (s < kSymbols && (root[j] == c1 || root[j] == c2)) {
                root[j] = (uint16_t)c1;
                ++len[j];
            }
        }
    }
LSPENC_UNROLL
    for (int j = 0; j < EPL; ++j) {
        const int s = lane + j * NL;
        if (s < kSymbols) codesize[s] = len[j];
    }
}

// codesize[257] of huff_merge -> bits[17] (bits[l] symbols of length l, bits[0] = 0) and huffval (the symbols in code order); returns their
// number.  One lane per table calls it.
LSPENC_HD inline int huff_finish(const uint16_t *codesize, unsigned char *bits, unsigned char *huffval)
{
    uint16_t cnt[kMaxLen + 2];
    uint16_t pos[kMaxLen + 2];
    for (int l = 0; l <= kMaxLen + 1; ++l) cnt[l] = 0;
    for (int s = 0; s < kSymbols; ++s) ++cnt[codesize[s]];
    cnt[0] = 0;                                      // unused symbols
    int p = 0;
    for (int l = 1; l <= kMaxLen; ++l) {
        pos[l] = (uint16_t)p;
        p += cnt[l];
    }
    // a lone pseudo-symbol (an empty histogram) has length 0: nothing to list
    int i = kMaxLen;
    for (; i > 16; --i) {
        while (cnt[i] > 0) {
            int j = i - 2;
            while (cnt[j] == 0) --j;
            cnt[i] -= 2;
            ++cnt[i - 1];
            cnt[j + 1] += 2;
            --cnt[j];
        }
    }
    while (i > 0 && cnt[i] == 0) --i;
    if (i > 0) --cnt[i];
    bits[0] = 0;
    for (int l = 1; l <= 16; ++l) bits[l] = (unsigned char)cnt[l];
    int n = 0;
    for (int s = 0; s < 256; ++s) {
        if (codesize[s]) {
            huffval[pos[codesize[s]]++] = (unsigned char)s;
            ++n;
        }
    }
    return n;
}

// canonical codes of (bits, huffval) (Annex C): codes[symbol] = (length << 16) | code, 0 for a symbol the table lacks
LSPENC_HD inline void huff_codes(const unsigned char *bits, const unsigned char *huffval, uint32_t *codes)
{
    for (int s = 0; s < 256; ++s) codes[s] = 0;
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int n = 0; n < bits[l]; ++n) codes[huffval[k++]] = ((uint32_t)l << 16) | code++;
        code <<= 1;
    }
}

}  // namespace lspenc
#endif
