// jpegdec_core.h -- the host/device half of the baseline JPEG decoder (include/lspjpegdec.h): the marker parser, the scan walker that finds the
// restart intervals, the decode tables, and the entropy decode of one restart interval.  Plain C++ with no allocation and no library calls: the
// planner (jpegdec.hip, host) runs the parser, the device kernel and the stand-alone host checker (jpegdec_check.cpp, built with sanitizers) run
// the SAME segment decoder, so a stream the checker has walked is a stream the kernel reads within the same bounds.
//
// What is decoded (jdhuff.c decode_mcu, jdmarker.c): SOF0, 8 bit, one interleaved scan, 1 component or YCbCr with luma 1x1 / 2x1 / 2x2, DRI,
// the file's DHT tables or Annex K's where a table is absent.  Everything else is refused with a status, never decoded differently.
//
// Under kFlagProgressive also SOF2 (jdphuff.c): walk_progressive() is the parser and scan walker of such a file (every scan, the tables and the
// restart interval in force at each, libjpeg's coef_bits bookkeeping), prog_units() the four procedures of ITU T.81 Annex G.  A progressive file
// is decoded only when it is complete (every coefficient of every component refined down to bit 0): its coefficients are then a baseline file's.
//
// Under kFlagParallel a restart interval of a baseline file is decoded by many lanes: decode_subsequence() is the decoder of one lane, shared by the
// kernel and its host twin (jpegdec_plan.h host_parallel_segment; jpegdec_par_check.cpp runs it against the serial decoder under sanitizers).
#ifndef LSPJPEGDEC_CORE_H
#define LSPJPEGDEC_CORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define LSPDEC_HD __host__ __device__
#else
#define LSPDEC_HD
#endif

namespace lspdec {

// status words (include/lspjpegdec.h LSPJPEG_DEC_STATUS_*)
enum : uint32_t { ST_OK = 0, ST_UNSUPPORTED = 1, ST_CORRUPT = 2, ST_RANGE = 3 };

constexpr int kMaxBlocksPerMcu = 6;                  // 4:2:0: Y0 Y1 Y2 Y3 Cb Cr
constexpr uint32_t kMcuBytesBound = 2560;            // >= 2 * ceil(6 * 1660 / 8) + 8: no MCU codes more bytes than this (the encoder's bound, stuffed)

// ---- a canonical Huffman table in decode form (Annex C; the layout of jdhuff.c's d_derived_tbl without its pointers)
struct HuffTable {
    uint16_t look[256];        // indexed by the next 8 bits: (length << 8) | symbol of the code of <= 8 bits that starts there, 0 when it is longer
    int32_t maxcode[17];       // [l] the largest code of length l, -1 when the table has none of that length
    int32_t valoff[17];        // [l] index into vals of the first code of length l, minus that code
    uint8_t vals[256];
    uint8_t pad[8];
};
static_assert(sizeof(HuffTable) == 912 && sizeof(HuffTable) % 16 == 0, "HuffTable is part of the descriptor block's layout");

// ---- one file of a batch, as the kernels see it
struct FileDesc {
    uint32_t status;           // what the parser found (ST_*): a file that is not ST_OK has no segments and is skipped by every stage
    uint32_t width, height, ncomp;
    uint32_t hs, vs;           // luma sampling factors (chroma is 1x1)
    uint32_t mcux, mcuy, bpm;  // MCUs per row and column, blocks per MCU
    uint32_t nblk;             // mcux * mcuy * bpm
    uint32_t restart;          // MCUs per restart interval, 0 = none
    uint32_t table0;           // index of this file's four HuffTables (DC0 AC0 DC1 AC1) in the table area
    uint32_t seg0, nseg;       // its entries of the segment list
    uint8_t dc_sel[4], ac_sel[4];   // per component: which DC / AC table
    uint64_t coef_off;         // first block of the file in the coefficient workspace
    uint64_t plane_off[3];     // byte offset of each component's block-padded plane in the plane workspace
    uint32_t plane_w[3], plane_h[3];
    uint16_t q[3][64];         // per component, natural order
    uint64_t out_ptr;          // device pointer of the output
    uint64_t table_ptr;        // device pointer of 256 floats (form 2)
    int64_t plane_stride;      // elements between the channels of a planar output (form 2)
    uint32_t form;             // 0: uint8 [H][W][3], 1: uint8 [H][W], 2: float32 planar through the table
    uint32_t progressive;      // 1: no segments of its own (nseg 0); stage 1 walks its scans instead
    uint32_t scan0, nscan;     // its entries of the scan list
};
static_assert(sizeof(FileDesc) % 8 == 0, "FileDesc is part of the descriptor block's layout");

// ---- one restart interval (a file without DRI is one segment): [begin, end) are offsets into the descriptor block, free of markers
struct SegDesc {
    uint32_t file;
    uint32_t mcu0, nmcu;
    uint32_t pad;
    uint64_t begin, end;
};

// ---- progressive files (kFlagProgressive)
constexpr uint32_t kFlagProgressive = 1u;           // include/lspjpegdec.h LSPJPEG_DEC_FLAG_PROGRESSIVE
constexpr uint32_t kMaxScans = 64;                   // include/lspjpegdec.h LSPJPEG_DEC_MAX_SCANS: a file with more is ST_UNSUPPORTED
constexpr uint32_t kBlockBytesBound = 448;           // >= 2 * ceil((64 * 26 + 30) / 8) + 8: no block of any scan codes more bytes than this (stuffed, reader's look-ahead included)

// one scan of a progressive file.  Its restart intervals are entries seg0 .. seg0 + nseg - 1 of the progressive segment list (SegDesc with mcu0 / nmcu
// counting the scan's own units: interleaved MCUs when the scan holds every component, blocks of the component's own extent when it holds one)
struct ScanDesc {
    uint32_t file;
    uint32_t units;            // MCUs, or bw * bh blocks
    uint32_t restart;          // the interval in force (DRI may change between scans), in units; 0 = none
    uint32_t bw, bh;           // one component: blocks per row and rows of ITS extent, ceil(Wc / 8) x ceil(Hc / 8); all components: mcux, mcuy
    uint32_t table0, ntab;     // its decode tables in the progressive table area: one per component of a first DC scan, one of an AC scan, none of a DC refinement
    uint32_t seg0, nseg;
    uint8_t ncomp, ss, se, ah, al, pad[3];
    uint8_t comp[4], td[4], ta[4];   // component indices (frame order) and the table ids the SOS names
    uint64_t begin, end;       // offsets into the descriptor block: the first entropy-coded byte, the marker that ends the scan
};
static_assert(sizeof(ScanDesc) == 72, "ScanDesc is part of the descriptor block's layout");

// ---- what the marker parser extracts, fixed size (no allocation)
struct Parsed {
    uint32_t status;
    uint32_t width, height, ncomp, hs, vs, restart;
    uint8_t comp_id[4], comp_q[4], dc_sel[4], ac_sel[4];
    uint8_t q_seen[4];
    uint16_t q[4][64];                  // natural order
    uint8_t huff_seen[2][2];            // [class][id]
    uint8_t huff_bits[2][2][17];        // [class][id][length 1..16]
    uint8_t huff_vals[2][2][256];
    uint64_t scan_begin;                // offset of the first entropy-coded byte
};

LSPDEC_HD inline int zigzag_to_natural(int k)
{
    // jpeg_natural_order; function-local so that host and device code index the same constant
    constexpr uint8_t t[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k];
}

// the inverse: where natural index n stands in the zigzag sequence
LSPDEC_HD inline int natural_to_zigzag(int n)
{
    constexpr uint8_t t[64] = {0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
                               10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    return t[n];
}

LSPDEC_HD inline uint32_t be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The marker parser (jdmarker.c read_markers up to the first SOS).  Every read is checked against n first.
// ---------------------------------------------------------------------------------------------------------------------------------------------
LSPDEC_HD inline uint32_t parse_markers(const uint8_t *p, size_t n, uint32_t max_side, Parsed *o)
{
    *o = Parsed{};
    bool sof = false, adobe = false;
    uint32_t adobe_transform = 0;
    if (n < 4 || p[0] != 0xff || p[1] != 0xd8) return o->status = ST_CORRUPT;
    size_t i = 2;
    for (;;) {
        if (i + 2 > n) return o->status = ST_CORRUPT;                          // data that ends early
        if (p[i] != 0xff) return o->status = ST_CORRUPT;
        while (i + 1 < n && p[i + 1] == 0xff) ++i;                             // fill bytes between segments are legal (B.1.1.2)
        if (i + 2 > n) return o->status = ST_CORRUPT;
        const uint32_t m = p[i + 1];
        i += 2;
        if (m == 0xd8 || m == 0xd9 || (m >= 0xd0 && m <= 0xd7) || m == 0x01 || m == 0x00) return o->status = ST_CORRUPT;
        if (i + 2 > n) return o->status = ST_CORRUPT;
        const size_t len = be16(p + i);
        if (len < 2 || i + len > n) return o->status = ST_CORRUPT;
        const uint8_t *s = p + i + 2;
        const size_t sl = len - 2;
        if (m == 0xc0) {                                                       // SOF0
            if (sof) return o->status = ST_CORRUPT;
            if (sl < 6) return o->status = ST_CORRUPT;
            const uint32_t nc = s[5];
            if (sl != 6 + 3 * (size_t)nc) return o->status = ST_CORRUPT;
            if (s[0] != 8) return o->status = ST_UNSUPPORTED;
            o->height = be16(s + 1);
            o->width = be16(s + 3);
            if (o->width == 0) return o->status = ST_CORRUPT;
            if (o->height == 0) return o->status = ST_UNSUPPORTED;             // the height comes in a DNL marker
            if (o->width > max_side || o->height > max_side) return o->status = ST_UNSUPPORTED;
            if (nc != 1 && nc != 3) return o->status = ST_UNSUPPORTED;
            o->ncomp = nc;
            for (uint32_t c = 0; c < nc; ++c) {
                o->comp_id[c] = s[6 + 3 * c];
                const uint32_t hv = s[7 + 3 * c], tq = s[8 + 3 * c];
                if (tq > 3 || (hv >> 4) == 0 || (hv >> 4) > 4 || (hv & 15) == 0 || (hv & 15) > 4) return o->status = ST_CORRUPT;
                o->comp_q[c] = (uint8_t)tq;
                if (c == 0) {
                    o->hs = hv >> 4;
                    o->vs = hv & 15;
                } else if (hv != 0x11) {
                    return o->status = ST_UNSUPPORTED;
                }
            }
            if (nc == 1 ? (o->hs != 1 || o->vs != 1) : !((o->hs == 1 || o->hs == 2) && (o->vs == 1 || (o->vs == 2 && o->hs == 2))))
                return o->status = ST_UNSUPPORTED;
            if (nc == 3 && o->comp_id[0] == 'R' && o->comp_id[1] == 'G' && o->comp_id[2] == 'B') return o->status = ST_UNSUPPORTED;
            sof = true;
        } else if (m >= 0xc1 && m <= 0xcf && m != 0xc4 && m != 0xc8) {         // extended, progressive, lossless, arithmetic (SOFn, DAC)
            return o->status = ST_UNSUPPORTED;
        } else if (m == 0xc4) {                                                // DHT: any number of tables
            size_t at = 0;
            while (at < sl) {
                if (at + 17 > sl) return o->status = ST_CORRUPT;
                const uint32_t tc = s[at] >> 4, th = s[at] & 15;
                if (tc > 1 || th > 3) return o->status = ST_CORRUPT;
                uint32_t count = 0;
                for (int l = 1; l <= 16; ++l) count += s[at + l];
                if (count > 256 || at + 17 + count > sl) return o->status = ST_CORRUPT;
                if (th > 1) return o->status = ST_UNSUPPORTED;                 // baseline has two tables per class
                o->huff_bits[tc][th][0] = 0;
                for (int l = 1; l <= 16; ++l) o->huff_bits[tc][th][l] = s[at + l];
                for (uint32_t k = 0; k < 256; ++k) o->huff_vals[tc][th][k] = k < count ? s[at + 17 + k] : 0;
                o->huff_seen[tc][th] = 1;
                at += 17 + count;
            }
        } else if (m == 0xdb) {                                                // DQT: any number of tables
            size_t at = 0;
            while (at < sl) {
                const uint32_t pq = s[at] >> 4, tq = s[at] & 15;
                if (tq > 3) return o->status = ST_CORRUPT;
                if (pq != 0) return o->status = pq == 1 ? ST_UNSUPPORTED : ST_CORRUPT;     // 16-bit tables
                if (at + 65 > sl) return o->status = ST_CORRUPT;
                for (int k = 0; k < 64; ++k) o->q[tq][zigzag_to_natural(k)] = s[at + 1 + k];
                o->q_seen[tq] = 1;
                at += 65;
            }
        } else if (m == 0xdd) {                                                // DRI
            if (sl != 2) return o->status = ST_CORRUPT;
            o->restart = be16(s);
        } else if (m == 0xee) {                                                // APP14: Adobe's colour transform flag
            if (sl >= 12 && s[0] == 'A' && s[1] == 'd' && s[2] == 'o' && s[3] == 'b' && s[4] == 'e') {
                adobe = true;
                adobe_transform = s[11];
            }
        } else if (m == 0xda) {                                                // SOS
            if (!sof) return o->status = ST_CORRUPT;
            if (sl < 1) return o->status = ST_CORRUPT;
            const uint32_t ns = s[0];
            if (ns < 1 || ns > 4 || sl != 4 + 2 * (size_t)ns) return o->status = ST_CORRUPT;
            if (ns != o->ncomp) return o->status = ST_UNSUPPORTED;             // several scans
            for (uint32_t c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != o->comp_id[c]) return o->status = ST_UNSUPPORTED;
                const uint32_t td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (td > 3 || ta > 3) return o->status = ST_CORRUPT;
                if (td > 1 || ta > 1) return o->status = ST_UNSUPPORTED;
                o->dc_sel[c] = (uint8_t)td;
                o->ac_sel[c] = (uint8_t)ta;
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return o->status = ST_UNSUPPORTED;
            if (adobe && adobe_transform == 0 && o->ncomp == 3) return o->status = ST_UNSUPPORTED;    // RGB, not YCbCr
            for (uint32_t c = 0; c < o->ncomp; ++c)
                if (!o->q_seen[o->comp_q[c]]) return o->status = ST_CORRUPT;
            o->scan_begin = i + len;
            return o->status = ST_OK;
        }
        // APPn, COM and the rest carry a length and are skipped
        i += len;
    }
}

LSPDEC_HD inline uint32_t mcu_count(const Parsed &f) { return ((f.width + 8 * f.hs - 1) / (8 * f.hs)) * ((f.height + 8 * f.vs - 1) / (8 * f.vs)); }

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The scan walker: finds the restart intervals of the entropy-coded data that starts at f.scan_begin.  segs may be null (count only).  A
// segment holds data bytes and 0xFF 0x00 pairs only; anything else between them is the expected RSTn, the EOI, or a refusal.
// ---------------------------------------------------------------------------------------------------------------------------------------------
LSPDEC_HD inline uint32_t walk_scan(const uint8_t *p, size_t n, const Parsed &f, uint64_t base, uint32_t file, SegDesc *segs, uint32_t cap, uint32_t *nseg,
                                  uint64_t *scan_end)
{
    const uint32_t total = mcu_count(f), ri = f.restart;
    const uint32_t want = ri ? (total + ri - 1) / ri : 1;
    size_t pos = f.scan_begin, seg_begin = f.scan_begin;
    uint32_t k = 0;
    *nseg = 0;
    *scan_end = 0;
    for (;;) {
        while (pos < n && p[pos] != 0xff) ++pos;
        if (pos + 1 >= n) return ST_CORRUPT;                                   // no EOI: data that ends early
        const uint32_t m = p[pos + 1];
        if (m == 0x00) {
            pos += 2;
            continue;
        }
        if (m == 0xff) return ST_UNSUPPORTED;                                  // fill bytes inside the scan
        const bool rst = m >= 0xd0 && m <= 0xd7;
        if (!rst && m != 0xd9) return ST_UNSUPPORTED;                          // another scan, a table, DNL ...
        if (rst && ri == 0) return ST_UNSUPPORTED;
        if (rst && m != 0xd0 + (k & 7)) return ST_CORRUPT;                     // a wrong RSTn
        if (rst ? k + 1 >= want : k + 1 != want) return ST_CORRUPT;            // one too many, or one missing
        if (segs) {
            if (k >= cap) return ST_CORRUPT;
            SegDesc &s = segs[k];
            s.file = file;
            s.mcu0 = ri ? k * ri : 0;
            s.nmcu = ri ? (total - s.mcu0 < ri ? total - s.mcu0 : ri) : total;
            s.pad = 0;
            s.begin = base + seg_begin;
            s.end = base + pos;
        }
        ++k;
        if (!rst) {
            *nseg = k;
            *scan_end = pos;                                                   // the EOI marker
            return ST_OK;
        }
        pos += 2;
        seg_begin = pos;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Decode tables.  Annex K's are the default where a file defines none (jdhuff.c std_huff_tables).  Host only: the planner builds them.
// ---------------------------------------------------------------------------------------------------------------------------------------------
inline void default_huffman(int cls, int id, uint8_t bits[17], uint8_t vals[256])
{
    static const uint8_t kBits[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                         {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                         {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                         {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
    static const uint8_t kAcLuma[162] = {
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
        0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
        0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
        0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
        0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
        0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
        0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
    static const uint8_t kAcChroma[162] = {
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
        0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
        0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
        0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
        0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
        0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
        0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
    const int t = 2 * id + cls;                                                // DC0 AC0 DC1 AC1
    bits[0] = 0;
    for (int l = 0; l < 16; ++l) bits[l + 1] = kBits[t][l];
    for (int k = 0; k < 256; ++k) vals[k] = 0;
    if (cls == 0) {
        for (int k = 0; k < 12; ++k) vals[k] = (uint8_t)k;
    } else {
        const uint8_t *v = id == 0 ? kAcLuma : kAcChroma;
        for (int k = 0; k < 162; ++k) vals[k] = v[k];
    }
}

// Annex C codes -> the decode form.  false when the counts describe no prefix code (a length with more codes than it has room for).
inline bool build_table(const uint8_t bits[17], const uint8_t vals[256], HuffTable *t)
{
    for (int k = 0; k < 256; ++k) t->look[k] = 0;
    for (int k = 0; k < 8; ++k) t->pad[k] = 0;
    uint32_t code = 0, at = 0;
    t->maxcode[0] = -1;
    t->valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const uint32_t nl = bits[l];
        if (code + nl > (1u << l)) return false;
        t->valoff[l] = (int32_t)at - (int32_t)code;
        t->maxcode[l] = nl ? (int32_t)(code + nl - 1) : -1;
        if (at + nl > 256) return false;
        for (uint32_t k = 0; k < nl; ++k, ++code, ++at) {
            if (l <= 8) {
                const uint32_t first = code << (8 - l);
                for (uint32_t j = 0; j < (1u << (8 - l)); ++j) t->look[first + j] = (uint16_t)((l << 8) | vals[at]);
            }
        }
        code <<= 1;
    }
    for (int k = 0; k < 256; ++k) t->vals[k] = vals[k];
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The entropy decode of one restart interval.  Src is the byte source: `uint8_t at(uint64_t pos) const` for pos in [begin, end) -- plain memory on
// the host, a window in LDS on the device.  The reader never asks for a byte outside [begin, end).
// ---------------------------------------------------------------------------------------------------------------------------------------------
// Track (the parallel route, kFlagParallel): the reader also remembers which of the bytes it holds were followed by a stuffed 0x00, so that
// at_bit() can say where in the STUFFED stream the next unread bit stands, and start() can take up a stream at such a place.
template <class Src, bool Track = false>
struct BitReader {
    const Src &src;
    uint64_t pos, end;
    uint64_t buf;              // the low `left` bits are the unread ones, MSB first
    int left;
    uint32_t status;
    uint32_t stuffed;          // Track: bit j set = the (j + 1)-th last byte fetched was 0xFF 0x00

    LSPDEC_HD BitReader(const Src &s, uint64_t begin, uint64_t end_) : src(s), pos(begin), end(end_), buf(0), left(0), status(ST_OK), stuffed(0) {}

    LSPDEC_HD void fill()
    {
        while (left <= 48 && pos < end) {
            const uint32_t b = src.at(pos++);
            if (b == 0xff) {                                                   // the walker left only 0xFF 0x00 in here; checked all the same
                if (pos >= end || src.at(pos) != 0) {
                    status = ST_CORRUPT;
                    end = pos;
                    return;
                }
                ++pos;
            }
            buf = (buf << 8) | b;
            left += 8;
            if (Track) stuffed = (stuffed << 1) | (b == 0xff ? 1u : 0u);
        }
    }
    // Track: the byte of the stuffed stream that holds the next unread bit (pos when nothing is buffered), and that bit's position.  Never a
    // stuffed 0x00: fill() steps over it with its 0xFF.
    LSPDEC_HD uint64_t at_byte() const
    {
        const uint32_t nb = (uint32_t)(left + 7) >> 3;
        return pos - nb - (uint32_t)__builtin_popcount(stuffed & ((1u << nb) - 1u));
    }
    LSPDEC_HD uint64_t at_bit() const { return at_byte() * 8 + (uint32_t)((8 - (left & 7)) & 7); }
    // Track: take the stream up at bit position `bit` (as at_bit() gives it, or a byte boundary: a boundary that falls on the 0x00 of a
    // 0xFF 0x00 pair moves to the byte behind it -- the walker leaves 0xFF in a segment only in such pairs, so the pair is recognised by its
    // two bytes).  `begin` is the segment's first byte: nothing in front of it is read.
    LSPDEC_HD void start(uint64_t begin, uint64_t bit)
    {
        pos = bit >> 3;
        const int off = (int)(bit & 7);
        if (off == 0 && pos > begin && pos < end && src.at(pos) == 0 && src.at(pos - 1) == 0xff) ++pos;
        buf = 0;
        left = 0;
        stuffed = 0;
        fill();
        if (off > left)
            status = ST_CORRUPT;                                               // no true state stands behind the data's end
        else
            left -= off;
    }
    // the next 16 bits, zero-padded past the end of the data
    LSPDEC_HD uint32_t peek16() const { return left >= 16 ? (uint32_t)(buf >> (left - 16)) & 0xffffu : (uint32_t)(buf << (16 - left)) & 0xffffu; }
    LSPDEC_HD bool skip(int nbits)
    {
        if (nbits > left) {
            status = ST_CORRUPT;                                               // data that ends early
            return false;
        }
        left -= nbits;
        return true;
    }
    LSPDEC_HD int symbol(const HuffTable &t)
    {
        if (left < 16) fill();
        const uint32_t w = peek16();
        const uint32_t e = t.look[w >> 8];
        if (e) return skip((int)(e >> 8)) ? (int)(e & 255u) : -1;
        for (int l = 9; l <= 16; ++l) {
            const int32_t code = (int32_t)(w >> (16 - l));
            if (code <= t.maxcode[l]) {
                const int32_t at = t.valoff[l] + code;
                if (at < 0 || at > 255) break;
                return skip(l) ? (int)t.vals[at] : -1;
            }
        }
        status = ST_CORRUPT;                                                   // a code that is in no table
        return -1;
    }
    // s bits, EXTENDed (F.2.2.1); s in 1..16
    LSPDEC_HD int receive_extend(int s)
    {
        if (left < s) fill();
        if (left < s) {
            status = ST_CORRUPT;
            return 0;
        }
        left -= s;
        const int v = (int)((buf >> left) & ((1u << s) - 1u));
        return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    }
    // s plain bits (an EOBn run's appended bits, a correction bit); s in 1..16
    LSPDEC_HD uint32_t bits(int s)
    {
        if (left < s) fill();
        if (left < s) {
            status = ST_CORRUPT;
            return 0;
        }
        left -= s;
        return (uint32_t)((buf >> left) & ((1u << s) - 1u));
    }
    // after the last MCU: what is left is the padding of the last byte, nothing more
    LSPDEC_HD bool drained() const { return pos >= end && left < 8; }
};

// One MCU: `bpm` blocks of 64 int16 in natural order into `out`, which the caller has zeroed.  comp_of[b] is the block's component.
template <class Src>
LSPDEC_HD inline uint32_t decode_mcu(BitReader<Src> &br, const HuffTable *tables, const uint8_t *dc_sel, const uint8_t *ac_sel, const uint8_t *comp_of, int bpm,
                                     int *pred, int16_t *out)
{
    for (int b = 0; b < bpm; ++b) {
        const int c = comp_of[b];
        const HuffTable &dc = tables[2 * dc_sel[c]], &ac = tables[2 * ac_sel[c] + 1];
        int16_t *blk = out + 64 * b;
        int s = br.symbol(dc);
        if (s < 0) return br.status;
        if (s > 11) return ST_CORRUPT;
        const int diff = s ? br.receive_extend(s) : 0;
        if (br.status) return br.status;
        pred[c] += diff;
        if (pred[c] < -32768 || pred[c] > 32767) return ST_RANGE;
        blk[0] = (int16_t)pred[c];
        for (int k = 1; k < 64; ++k) {
            const int rs = br.symbol(ac);
            if (rs < 0) return br.status;
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
                if (r != 15) break;                                            // EOB
                k += 15;                                                       // ZRL: sixteen zeros with the loop's own step
                if (k > 63) return ST_CORRUPT;
                continue;
            }
            if (s > 10) return ST_CORRUPT;
            k += r;
            if (k > 63) return ST_CORRUPT;                                     // a coefficient index past 63
            const int v = br.receive_extend(s);
            if (br.status) return br.status;
            blk[zigzag_to_natural(k)] = (int16_t)v;
        }
    }
    return ST_OK;
}

LSPDEC_HD inline void block_components(uint32_t ncomp, uint32_t hs, uint32_t vs, uint8_t comp_of[kMaxBlocksPerMcu], int *bpm)
{
    int n = 0;
    if (ncomp == 1) {
        comp_of[n++] = 0;
    } else {
        for (uint32_t k = 0; k < hs * vs; ++k) comp_of[n++] = 0;
        comp_of[n++] = 1;
        comp_of[n++] = 2;
    }
    for (int k = n; k < kMaxBlocksPerMcu; ++k) comp_of[k] = 0;
    *bpm = n;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Parallel decode inside a restart interval (kFlagParallel): self-synchronising Huffman decoding (Weissenberger and Schmidt 2018, 2021).
// The interval's stuffed bytes are cut into subsequences of kSubseqBytes; lane i decodes the codes that START in subsequence i (the last one may
// run past its end).  Where a lane has to start is not known in advance, so every lane but the first guesses "a DC code of block 0 starts at my
// boundary", and the guesses are repaired by a fixed point: each lane hands its exit state to the next, which decodes again if that is not the
// entry it used.  Lane 0's entry is true, so by induction every entry is true once nothing changes -- after one round per lane at the worst,
// which is the serial decode.  A decode that meets an error ends in a DEAD state: an error met from a guess is no error of the file.  A dead
// entry gives a dead exit; a lane BEHIND a dead exit does not take it over but falls back on its own guess, so that the parse takes up again behind
// the place where a wrong guess died (handing the dead state on instead lets it run ahead of the true state at the same one lane per round and
// wipe out every guess that had already met the true parse: the 512^2 q95 files then take as many rounds as they have subsequences).  The
// induction holds for the lanes with no dead exit in front of them, and only those take part in the write pass; the first dead exit of a TRUE
// entry is the file's own failure or lies behind its last block, and either ends the interval's walk.
// A JPEG stream resynchronises in bits and zigzag position after a few codes, in the block index inside the MCU after a few MCUs: 1 to 1.5 KB on
// the 512^2 test files.  The depth of a chunk is about (resynchronisation distance + one subsequence) whatever the subsequence size, so the gain
// is the chunk's bytes over that distance, and a chunk is as many lanes as a workgroup has.  The size is small so that files of a few dozen
// bytes (most test fixtures) take the many-lane path too.  A code (<= 27 bits) may be longer than a subsequence: a lane whose entry lies behind
// its own end decodes nothing and hands the state on.
// ---------------------------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kFlagParallel = 2u;              // include/lspjpegdec.h LSPJPEG_DEC_FLAG_PARALLEL
constexpr uint32_t kSubseqBytes = 8;                // of the stuffed stream, per lane
constexpr uint32_t kParLanes = 1024;                // lanes of one workgroup: an interval is walked in chunks of kParLanes subsequences

// the parser's state between two codes
struct ParState {
    uint64_t bit;              // position of the next code in the stuffed stream: 8 * (offset inside the block) + bit; never inside a stuffed 0x00
    uint16_t b, k;             // block index inside the MCU, zigzag position: k = 0 means "a DC code is next"
    uint32_t dead;             // a decode up to here met an error; a dead entry gives a dead exit
};
static_assert(sizeof(ParState) == 16, "ParState is moved as two 64-bit words");

LSPDEC_HD inline bool same_state(const ParState &a, const ParState &b) { return a.bit == b.bit && a.b == b.b && a.k == b.k && a.dead == b.dead; }

// the guess of a lane whose subsequence starts at byte `at`
template <class Src>
LSPDEC_HD inline ParState guess_state(const Src &src, uint64_t begin, uint64_t end, uint64_t at)
{
    if (at > begin && at < end && src.at(at) == 0 && src.at(at - 1) == 0xff) ++at;     // the 0x00 of a stuffed pair holds no bit
    return ParState{at * 8, 0, 0, 0};
}

// how an interval is cut
LSPDEC_HD inline uint32_t subsequences_of(uint64_t begin, uint64_t end) { return end > begin ? (uint32_t)((end - begin + kSubseqBytes - 1) / kSubseqBytes) : 1u; }

// what the file's geometry gives the subsequence decoder, in registers (no arrays indexed by the state)
struct ParGeom {
    uint32_t bpm, nluma;       // blocks per MCU; luma blocks among them (1 for a grey file)
    uint32_t dc_sel, ac_sel;   // FileDesc's selectors, one byte per component
};
LSPDEC_HD inline ParGeom par_geom(const FileDesc &f)
{
    ParGeom g;
    g.bpm = f.ncomp == 1 ? 1 : f.hs * f.vs + 2;
    g.nluma = f.ncomp == 1 ? 1 : f.hs * f.vs;
    g.dc_sel = f.dc_sel[0] | ((uint32_t)f.dc_sel[1] << 8) | ((uint32_t)f.dc_sel[2] << 16);
    g.ac_sel = f.ac_sel[0] | ((uint32_t)f.ac_sel[1] << 8) | ((uint32_t)f.ac_sel[2] << 16);
    return g;
}

struct ParResult {
    ParState exit;             // where the next lane starts (sync mode)
    uint32_t blocks;           // DC codes decoded: blocks started
    int dc[3];                 // sum of the DC differences per component
    uint32_t status;           // write mode: the first failure from this (true) entry, in stream order
    uint32_t done;             // write mode: this lane finished the interval's last block
};

// One subsequence from entry state `in`: codes are decoded while the next one starts in front of byte `limit`; reads stay inside [begin, end).
// Sync mode (Write false) decodes without writing; an error there belongs to the guess, not to the file: the exit state is dead.
// Write mode starts from a true entry: `block` is the absolute index (inside the interval) of the block `in` stands in -- the one started last
// when in.k != 0 -- and pred the DC predictions there.  Coefficients go to coef[block][64] in natural order, the running prediction into
// slot 0 under decode_mcu's int16 check, up to `total` blocks; the lane that finishes block total - 1 applies the drained() rule, and the
// interval's last lane (`last`) reports data that ends early.  The order of the checks is decode_mcu's.
template <bool Write, class Src>
LSPDEC_HD inline void decode_subsequence(const Src &src, uint64_t begin, uint64_t end, uint64_t limit, const ParState &in, const HuffTable *tables, const ParGeom &g,
                                         uint32_t block, uint32_t total, const int *pred_in, int16_t *coef, bool last, ParResult *o)
{
    o->exit = in;
    o->blocks = 0;
    o->dc[0] = o->dc[1] = o->dc[2] = 0;
    o->status = ST_OK;
    o->done = 0;
    if (in.dead) return;
    if (Write && block >= total) return;                                       // behind the interval's last block: nothing of it is decoded
    BitReader<Src, true> br(src, begin, end);
    br.start(begin, in.bit);
    uint32_t b = in.b, k = in.k, st = br.status;
    int p0 = 0, p1 = 0, p2 = 0;
    if (Write) {
        p0 = pred_in[0];
        p1 = pred_in[1];
        p2 = pred_in[2];
    }
    int16_t *blk = Write ? coef + (size_t)block * 64 : nullptr;
    while (st == ST_OK && br.at_byte() < limit) {
        const uint32_t c = b < g.nluma ? 0u : b - g.nluma + 1u;
        if (k == 0) {
            const int s = br.symbol(tables[2 * ((g.dc_sel >> (8 * c)) & 1u)]);
            if (s < 0) {
                st = br.status;
                break;
            }
            if (s > 11) {
                st = ST_CORRUPT;
                break;
            }
            const int diff = s ? br.receive_extend(s) : 0;
            if (br.status) {
                st = br.status;
                break;
            }
            ++o->blocks;
            o->dc[0] += c == 0 ? diff : 0;
            o->dc[1] += c == 1 ? diff : 0;
            o->dc[2] += c == 2 ? diff : 0;
            if (Write) {
                p0 += c == 0 ? diff : 0;
                p1 += c == 1 ? diff : 0;
                p2 += c == 2 ? diff : 0;
                const int pred = c == 0 ? p0 : c == 1 ? p1 : p2;
                if (pred < -32768 || pred > 32767) {
                    st = ST_RANGE;
                    break;
                }
                blk[0] = (int16_t)pred;
            }
            k = 1;
        } else {
            const int rs = br.symbol(tables[2 * ((g.ac_sel >> (8 * c)) & 1u) + 1]);
            if (rs < 0) {
                st = br.status;
                break;
            }
            const uint32_t r = (uint32_t)rs >> 4, s = (uint32_t)rs & 15u;
            if (s == 0) {
                if (r != 15) {
                    k = 64;                                                    // EOB
                } else {
                    if (k + 15 > 63) {                                         // ZRL: sixteen zeros
                        st = ST_CORRUPT;
                        break;
                    }
                    k += 16;
                }
            } else {
                if (s > 10) {
                    st = ST_CORRUPT;
                    break;
                }
                k += r;
                if (k > 63) {                                                  // a coefficient index past 63
                    st = ST_CORRUPT;
                    break;
                }
                const int v = br.receive_extend((int)s);
                if (br.status) {
                    st = br.status;
                    break;
                }
                if (Write) blk[zigzag_to_natural((int)k)] = (int16_t)v;
                ++k;
            }
        }
        if (k == 64) {                                                         // the block is complete
            k = 0;
            b = b + 1 == g.bpm ? 0 : b + 1;
            if (Write) {
                ++block;
                blk += 64;
                if (block == total) {
                    o->done = 1;
                    if (!br.drained()) st = ST_CORRUPT;                        // whole bytes left over
                    break;
                }
            }
        }
    }
    if (Write) {
        if (st == ST_OK && last && !o->done) st = ST_CORRUPT;                  // the data ends before the interval's last block does
        o->status = st;
        return;
    }
    o->exit.bit = br.at_bit();
    o->exit.b = (uint16_t)b;
    o->exit.k = (uint16_t)k;
    o->exit.dead = st != ST_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Progressive files (SOF2), jdphuff.c.  The four procedures of Annex G work on one block that already holds what the earlier scans left
// (natural order), so the caller moves blocks in and out; prog_units() runs `n` units of one restart interval over contiguous blocks.
// ---------------------------------------------------------------------------------------------------------------------------------------------
struct ScanState {
    int pred[4];               // DC prediction per component, unshifted (jdphuff.c last_dc_val)
    uint32_t eobrun;           // blocks still covered by the end-of-band run in force
};

LSPDEC_HD inline bool fits_int16(int v) { return v >= -32768 && v <= 32767; }

// where coefficient k (zigzag index) of a block lives: natural order in memory; the kernel stages its blocks in zigzag order, so that the one lane
// that walks the codes indexes LDS by k and looks nothing up
struct NaturalOrder {
    LSPDEC_HD static int at(int k) { return zigzag_to_natural(k); }
};
struct ZigzagOrder {
    LSPDEC_HD static int at(int k) { return k; }
};

// G.1.2.1 first DC scan: the difference is coded as in a sequential file, the value is stored shifted by Al
template <class Src>
LSPDEC_HD inline uint32_t dc_first(BitReader<Src> &br, const HuffTable &dc, int al, int *pred, int16_t *blk)
{
    const int s = br.symbol(dc);
    if (s < 0) return br.status;
    if (s > 11) return ST_CORRUPT;
    const int diff = s ? br.receive_extend(s) : 0;
    if (br.status) return br.status;
    *pred += diff;
    if (!fits_int16(*pred)) return ST_RANGE;
    const int v = *pred * (1 << al);
    if (!fits_int16(v)) return ST_RANGE;
    blk[0] = (int16_t)v;
    return ST_OK;
}

// G.1.2.1 DC refinement: one bit per block
template <class Src>
LSPDEC_HD inline uint32_t dc_refine(BitReader<Src> &br, int al, int16_t *blk)
{
    const uint32_t b = br.bits(1);
    if (br.status) return br.status;
    if (b) blk[0] = (int16_t)(blk[0] | (1 << al));
    return ST_OK;
}

// an EOBn symbol (run r < 15, size 0): 2^r blocks plus r appended bits, this block included
template <class Src>
LSPDEC_HD inline uint32_t eob_run(BitReader<Src> &br, int r, uint32_t *eobrun)
{
    *eobrun = 1u << r;
    if (r) {
        *eobrun += br.bits(r);
        if (br.status) return br.status;
    }
    return ST_OK;
}

// G.1.2.2 first AC scan of the band ss..se
template <class Order, class Src>
LSPDEC_HD inline uint32_t ac_first(BitReader<Src> &br, const HuffTable &ac, int ss, int se, int al, uint32_t *eobrun, int16_t *blk)
{
    if (*eobrun) {
        --*eobrun;
        return ST_OK;
    }
    for (int k = ss; k <= se; ++k) {
        const int rs = br.symbol(ac);
        if (rs < 0) return br.status;
        const int r = rs >> 4, s = rs & 15;
        if (s == 0) {
            if (r != 15) {
                const uint32_t st = eob_run(br, r, eobrun);
                if (st) return st;
                --*eobrun;
                return ST_OK;
            }
            k += 15;                                                       // ZRL: sixteen zeros with the loop's own step
            if (k > se) return ST_CORRUPT;
            continue;
        }
        if (s > 10) return ST_CORRUPT;
        k += r;
        if (k > se) return ST_CORRUPT;                                     // a coefficient index past Se
        const int v = br.receive_extend(s) * (1 << al);
        if (br.status) return br.status;
        if (!fits_int16(v)) return ST_RANGE;
        blk[Order::at(k)] = (int16_t)v;
    }
    return ST_OK;
}

// one correction bit for a coefficient with history (jdphuff.c decode_mcu_AC_refine): the magnitude grows by 1 << al when that bit is not set yet
template <class Src>
LSPDEC_HD inline uint32_t ac_correct(BitReader<Src> &br, int al, int16_t *c)
{
    const uint32_t b = br.bits(1);
    if (br.status) return br.status;
    if (b && ((int)*c & (1 << al)) == 0) {
        const int v = *c >= 0 ? *c + (1 << al) : *c - (1 << al);
        if (!fits_int16(v)) return ST_RANGE;
        *c = (int16_t)v;
    }
    return ST_OK;
}

// G.1.2.3 AC refinement of the band ss..se
template <class Order, class Src>
LSPDEC_HD inline uint32_t ac_refine(BitReader<Src> &br, const HuffTable &ac, int ss, int se, int al, uint32_t *eobrun, int16_t *blk)
{
    int k = ss;
    if (*eobrun == 0) {
        for (; k <= se; ++k) {
            const int rs = br.symbol(ac);
            if (rs < 0) return br.status;
            int r = rs >> 4, s = rs & 15;
            if (s) {
                if (s != 1) return ST_CORRUPT;
                s = br.bits(1) ? (1 << al) : -(1 << al);                   // the new coefficient's value; its place comes after r zeros
                if (br.status) return br.status;
            } else if (r != 15) {
                const uint32_t st = eob_run(br, r, eobrun);
                if (st) return st;
                break;                                                     // the rest of the band is handled below, as part of the run
            }
            // pass r coefficients without history (ZRL: r = 15 and the one the loop steps over), correcting the ones with history on the way
            for (; k <= se; ++k) {
                int16_t *c = blk + Order::at(k);
                if (*c) {
                    const uint32_t st = ac_correct(br, al, c);
                    if (st) return st;
                } else if (--r < 0) {
                    break;
                }
            }
            if (k > se) return ST_CORRUPT;                                 // the band ends before the coefficient's (or the sixteenth zero's) place
            if (s) blk[Order::at(k)] = (int16_t)s;
        }
    }
    if (*eobrun) {
        for (; k <= se; ++k) {
            int16_t *c = blk + Order::at(k);
            if (*c) {
                const uint32_t st = ac_correct(br, al, c);
                if (st) return st;
            }
        }
        --*eobrun;
    }
    return ST_OK;
}

// n units of a restart interval of scan sc: `blocks` holds n * bpu blocks in the scan's own order (bpu = the MCU's blocks, or 1), comp_of as for
// decode_mcu, tabs the scan's tables, Order how a block is laid out.  The caller checks br.drained() after an interval's last unit and
// st.eobrun == 0 after the scan's.
template <class Order, class Src>
LSPDEC_HD inline uint32_t prog_units(BitReader<Src> &br, const ScanDesc &sc, const HuffTable *tabs, const uint8_t *comp_of, int bpu, ScanState &st, int16_t *blocks,
                                     uint32_t n)
{
    for (uint32_t u = 0; u < n; ++u)
        for (int b = 0; b < bpu; ++b) {
            int16_t *blk = blocks + ((size_t)u * bpu + b) * 64;
            const int c = sc.ncomp == 1 ? 0 : comp_of[b];                  // a scan of all components names them in frame order (walk_progressive)
            uint32_t r;
            if (sc.ss == 0)
                r = sc.ah == 0 ? dc_first(br, tabs[c], sc.al, &st.pred[c], blk) : dc_refine(br, sc.al, blk);
            else
                r = sc.ah == 0 ? ac_first<Order>(br, tabs[0], sc.ss, sc.se, sc.al, &st.eobrun, blk) : ac_refine<Order>(br, tabs[0], sc.ss, sc.se, sc.al, &st.eobrun, blk);
            if (r != ST_OK) return r;
        }
    return ST_OK;
}

// where block `at` (unit * bpu + b in the scan's own order) lives in the file's MCU-ordered coefficients.  A scan of one component walks the
// blocks of that component's own extent in raster order, which is narrower than the MCU grid when the image ends inside an MCU.
LSPDEC_HD inline uint32_t prog_block_index(const FileDesc &f, const ScanDesc &sc, uint32_t at)
{
    if (sc.ncomp != 1 || f.ncomp == 1) return at;                          // interleaved, or one component: the raster is the MCU order
    const uint32_t by = at / sc.bw, bx = at - by * sc.bw, c = sc.comp[0];
    if (c) return (by * f.mcux + bx) * f.bpm + f.hs * f.vs + c - 1;
    return ((by / f.vs) * f.mcux + bx / f.hs) * f.bpm + (by % f.vs) * f.hs + bx % f.hs;
}

// ---- the parser and scan walker of a progressive file: the whole file, marker by marker
struct ProgFile {
    uint32_t status;
    uint32_t width, height, ncomp, hs, vs;
    uint32_t restart0;                  // the interval in force at the first scan
    uint32_t nscan, nseg, ntab;         // scans, restart intervals of all scans, table snapshots
    uint8_t comp_id[4], comp_q[4], q_seen[4];
    uint16_t q[4][64];                  // natural order
    uint8_t huff_seen[2][4];
    uint8_t huff_bits[2][4][17];
    uint8_t huff_vals[2][4][256];
    int8_t coef_al[3][64];              // jdphuff.c coef_bits: the Al each coefficient has reached, -1 before its first scan
    uint64_t data_begin, data_end;      // the first entropy-coded byte of the first scan, the EOI marker
};

// Walks p[0, n).  scans / segs / tabs may be null (count only); otherwise they take at most the given counts and offsets are file offsets + base.
// Host only (build_table).
inline uint32_t walk_progressive(const uint8_t *p, size_t n, uint32_t max_side, ProgFile *o, uint64_t base, uint32_t file, ScanDesc *scans, uint32_t scan_cap,
                                 SegDesc *segs, uint32_t seg_cap, HuffTable *tabs, uint32_t tab_cap)
{
    *o = ProgFile{};
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 64; ++k) o->coef_al[c][k] = -1;
    bool sof = false, adobe = false;
    uint32_t adobe_transform = 0, restart = 0;
    if (n < 4 || p[0] != 0xff || p[1] != 0xd8) return o->status = ST_CORRUPT;
    size_t i = 2;
    for (;;) {
        if (i + 2 > n) return o->status = ST_CORRUPT;                          // data that ends early
        if (p[i] != 0xff) return o->status = ST_CORRUPT;
        while (i + 1 < n && p[i + 1] == 0xff) ++i;                             // fill bytes between segments
        if (i + 2 > n) return o->status = ST_CORRUPT;
        const uint32_t m = p[i + 1];
        i += 2;
        if (m == 0xd9) {                                                       // EOI
            if (o->nscan == 0) return o->status = ST_CORRUPT;
            for (uint32_t c = 0; c < o->ncomp; ++c)
                for (int k = 0; k < 64; ++k)
                    if (o->coef_al[c][k] != 0) return o->status = ST_UNSUPPORTED;     // incomplete: libjpeg would smooth, or show a coarser image
            o->data_end = i - 2;
            return o->status = ST_OK;
        }
        if (m == 0xd8 || (m >= 0xd0 && m <= 0xd7) || m == 0x01 || m == 0x00) return o->status = ST_CORRUPT;
        if (i + 2 > n) return o->status = ST_CORRUPT;
        const size_t len = be16(p + i);
        if (len < 2 || i + len > n) return o->status = ST_CORRUPT;
        const uint8_t *s = p + i + 2;
        const size_t sl = len - 2;
        if (m == 0xc2) {                                                       // SOF2
            if (sof) return o->status = ST_CORRUPT;
            if (sl < 6) return o->status = ST_CORRUPT;
            const uint32_t nc = s[5];
            if (sl != 6 + 3 * (size_t)nc) return o->status = ST_CORRUPT;
            if (s[0] != 8) return o->status = ST_UNSUPPORTED;
            o->height = be16(s + 1);
            o->width = be16(s + 3);
            if (o->width == 0) return o->status = ST_CORRUPT;
            if (o->height == 0) return o->status = ST_UNSUPPORTED;             // the height comes in a DNL marker
            if (o->width > max_side || o->height > max_side) return o->status = ST_UNSUPPORTED;
            if (nc != 1 && nc != 3) return o->status = ST_UNSUPPORTED;
            o->ncomp = nc;
            for (uint32_t c = 0; c < nc; ++c) {
                o->comp_id[c] = s[6 + 3 * c];
                const uint32_t hv = s[7 + 3 * c], tq = s[8 + 3 * c];
                if (tq > 3 || (hv >> 4) == 0 || (hv >> 4) > 4 || (hv & 15) == 0 || (hv & 15) > 4) return o->status = ST_CORRUPT;
                o->comp_q[c] = (uint8_t)tq;
                if (c == 0) {
                    o->hs = hv >> 4;
                    o->vs = hv & 15;
                } else if (hv != 0x11) {
                    return o->status = ST_UNSUPPORTED;
                }
            }
            if (nc == 1 ? (o->hs != 1 || o->vs != 1) : !((o->hs == 1 || o->hs == 2) && (o->vs == 1 || (o->vs == 2 && o->hs == 2))))
                return o->status = ST_UNSUPPORTED;
            if (nc == 3 && o->comp_id[0] == 'R' && o->comp_id[1] == 'G' && o->comp_id[2] == 'B') return o->status = ST_UNSUPPORTED;
            if (nc == 3 && (o->comp_id[0] == o->comp_id[1] || o->comp_id[0] == o->comp_id[2] || o->comp_id[1] == o->comp_id[2])) return o->status = ST_CORRUPT;
            sof = true;
        } else if (m >= 0xc0 && m <= 0xcf && m != 0xc4 && m != 0xc8) {         // SOF0 with several scans, extended, lossless, arithmetic (SOFn, DAC)
            return o->status = ST_UNSUPPORTED;
        } else if (m == 0xc4) {                                                // DHT: any number of tables, ids 0..3; a later one replaces an earlier one
            size_t at = 0;
            while (at < sl) {
                if (at + 17 > sl) return o->status = ST_CORRUPT;
                const uint32_t tc = s[at] >> 4, th = s[at] & 15;
                if (tc > 1 || th > 3) return o->status = ST_CORRUPT;
                uint32_t count = 0;
                for (int l = 1; l <= 16; ++l) count += s[at + l];
                if (count > 256 || at + 17 + count > sl) return o->status = ST_CORRUPT;
                o->huff_bits[tc][th][0] = 0;
                for (int l = 1; l <= 16; ++l) o->huff_bits[tc][th][l] = s[at + l];
                for (uint32_t k = 0; k < 256; ++k) o->huff_vals[tc][th][k] = k < count ? s[at + 17 + k] : 0;
                o->huff_seen[tc][th] = 1;
                at += 17 + count;
            }
        } else if (m == 0xdb) {                                                // DQT
            if (o->nscan) return o->status = ST_UNSUPPORTED;                   // libjpeg latches a component's table at its first scan
            size_t at = 0;
            while (at < sl) {
                const uint32_t pq = s[at] >> 4, tq = s[at] & 15;
                if (tq > 3) return o->status = ST_CORRUPT;
                if (pq != 0) return o->status = pq == 1 ? ST_UNSUPPORTED : ST_CORRUPT;
                if (at + 65 > sl) return o->status = ST_CORRUPT;
                for (int k = 0; k < 64; ++k) o->q[tq][zigzag_to_natural(k)] = s[at + 1 + k];
                o->q_seen[tq] = 1;
                at += 65;
            }
        } else if (m == 0xdc) {                                                // DNL
            return o->status = ST_UNSUPPORTED;
        } else if (m == 0xdd) {                                                // DRI: holds for the scans that follow
            if (sl != 2) return o->status = ST_CORRUPT;
            restart = be16(s);
        } else if (m == 0xee && o->nscan == 0) {                               // APP14: Adobe's colour transform flag
            if (sl >= 12 && s[0] == 'A' && s[1] == 'd' && s[2] == 'o' && s[3] == 'b' && s[4] == 'e') {
                adobe = true;
                adobe_transform = s[11];
            }
        } else if (m == 0xda) {                                                // SOS
            if (!sof) return o->status = ST_CORRUPT;
            if (sl < 1) return o->status = ST_CORRUPT;
            const uint32_t ns = s[0];
            if (ns < 1 || ns > 4 || sl != 4 + 2 * (size_t)ns) return o->status = ST_CORRUPT;
            if (o->nscan == kMaxScans) return o->status = ST_UNSUPPORTED;
            ScanDesc sc{};
            sc.file = file;
            sc.ncomp = (uint8_t)ns;
            for (uint32_t j = 0; j < ns; ++j) {
                uint32_t c = 0;
                while (c < o->ncomp && o->comp_id[c] != s[1 + 2 * j]) ++c;
                if (c == o->ncomp) return o->status = ST_CORRUPT;              // an unknown component
                for (uint32_t e = 0; e < j; ++e)
                    if (sc.comp[e] == c) return o->status = ST_CORRUPT;        // a repeated one
                sc.comp[j] = (uint8_t)c;
                sc.td[j] = s[2 + 2 * j] >> 4;
                sc.ta[j] = s[2 + 2 * j] & 15;
                if (sc.td[j] > 3 || sc.ta[j] > 3) return o->status = ST_CORRUPT;
            }
            sc.ss = s[1 + 2 * ns];
            sc.se = s[2 + 2 * ns];
            sc.ah = s[3 + 2 * ns] >> 4;
            sc.al = s[3 + 2 * ns] & 15;
            // libjpeg's rules for a scan of a progressive file (jdphuff.c start_pass_phuff_decoder: "bad progression parameters")
            if (sc.ss > sc.se || sc.se > 63 || (sc.ss == 0 && sc.se != 0) || (sc.ss != 0 && ns != 1) || (sc.ah != 0 && sc.al != sc.ah - 1) || sc.al > 13)
                return o->status = ST_CORRUPT;
            if (ns != 1 && ns != o->ncomp) return o->status = ST_UNSUPPORTED;  // an MCU of two components out of three
            for (uint32_t j = 0; ns > 1 && j < ns; ++j)
                if (sc.comp[j] != j) return o->status = ST_UNSUPPORTED;        // components out of frame order
            if (o->nscan == 0) {
                if (adobe && adobe_transform == 0 && o->ncomp == 3) return o->status = ST_UNSUPPORTED;    // RGB, not YCbCr
                for (uint32_t c = 0; c < o->ncomp; ++c)
                    if (!o->q_seen[o->comp_q[c]]) return o->status = ST_CORRUPT;
            }
            // the progression (coef_bits): libjpeg warns and decodes on, this decoder refuses
            for (uint32_t j = 0; j < ns; ++j) {
                int8_t *al = o->coef_al[sc.comp[j]];
                if (sc.ss != 0 && al[0] < 0) return o->status = ST_UNSUPPORTED;             // AC before the component's DC
                for (int k = sc.ss; k <= sc.se; ++k) {
                    if (sc.ah == 0 ? al[k] != -1 : al[k] != (int8_t)sc.ah) return o->status = ST_UNSUPPORTED;
                    al[k] = (int8_t)sc.al;
                }
            }
            // the tables the scan decodes with, as they stand now
            sc.table0 = o->ntab;
            sc.ntab = sc.ss ? 1 : sc.ah ? 0 : ns;
            for (uint32_t j = 0; j < sc.ntab; ++j) {
                const int cls = sc.ss ? 1 : 0, id = sc.ss ? sc.ta[0] : sc.td[j];
                if (!o->huff_seen[cls][id]) return o->status = ST_UNSUPPORTED;              // a table the file has not defined
                HuffTable t;
                if (!build_table(o->huff_bits[cls][id], o->huff_vals[cls][id], &t)) return o->status = ST_CORRUPT;
                if (tabs) {
                    if (o->ntab + j >= tab_cap) return o->status = ST_CORRUPT;
                    tabs[o->ntab + j] = t;
                }
            }
            o->ntab += sc.ntab;
            // geometry of the scan
            const uint32_t mcux = (o->width + 8 * o->hs - 1) / (8 * o->hs), mcuy = (o->height + 8 * o->vs - 1) / (8 * o->vs);
            if (ns > 1 || o->ncomp == 1) {
                sc.bw = mcux;
                sc.bh = mcuy;
            } else {
                const uint32_t wc = sc.comp[0] ? (o->width + o->hs - 1) / o->hs : o->width, hc = sc.comp[0] ? (o->height + o->vs - 1) / o->vs : o->height;
                sc.bw = (wc + 7) / 8;
                sc.bh = (hc + 7) / 8;
            }
            sc.units = sc.bw * sc.bh;
            sc.restart = restart;
            if (o->nscan == 0) {
                o->restart0 = restart;
                o->data_begin = i + len;
            }
            // the entropy-coded data: restart intervals up to the next marker that is no RSTn
            const uint32_t ri = restart, want = ri ? (sc.units + ri - 1) / ri : 1;
            size_t pos = i + len, seg_begin = pos;
            uint32_t k = 0;
            sc.begin = base + pos;
            sc.seg0 = o->nseg;
            for (;;) {
                while (pos < n && p[pos] != 0xff) ++pos;
                if (pos + 1 >= n) return o->status = ST_CORRUPT;               // data that ends early
                const uint32_t mm = p[pos + 1];
                if (mm == 0x00) {
                    pos += 2;
                    continue;
                }
                if (mm == 0xff) return o->status = ST_UNSUPPORTED;             // fill bytes inside the scan
                const bool rst = mm >= 0xd0 && mm <= 0xd7;
                if (rst && ri == 0) return o->status = ST_UNSUPPORTED;
                if (rst && mm != 0xd0 + (k & 7)) return o->status = ST_CORRUPT;            // a wrong RSTn: the numbering starts again at every scan
                if (rst ? k + 1 >= want : k + 1 != want) return o->status = ST_CORRUPT;    // one too many, or one missing
                if (segs) {
                    if (o->nseg + k >= seg_cap) return o->status = ST_CORRUPT;
                    SegDesc &g = segs[o->nseg + k];
                    g.file = file;
                    g.mcu0 = ri ? k * ri : 0;
                    g.nmcu = ri ? (sc.units - g.mcu0 < ri ? sc.units - g.mcu0 : ri) : sc.units;
                    g.pad = 0;
                    g.begin = base + seg_begin;
                    g.end = base + pos;
                }
                ++k;
                if (!rst) break;
                pos += 2;
                seg_begin = pos;
            }
            sc.nseg = k;
            sc.end = base + pos;
            o->nseg += k;
            if (scans) {
                if (o->nscan >= scan_cap) return o->status = ST_CORRUPT;
                scans[o->nscan] = sc;
            }
            ++o->nscan;
            i = pos;                                                           // the marker that ended the scan is read next
            continue;
        }
        // APPn, COM and the rest carry a length and are skipped
        i += len;
    }
}

}  // namespace lspdec
#endif
