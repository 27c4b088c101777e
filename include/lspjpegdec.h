/* lspjpegdec.h -- C ABI of the baseline JPEG decoder: the inverse of lspjpeg.h, and the way image files reach the renderer.
 * Exported by livespeechportraits_amd/liblspf2f.so; the decode is gfx950 only, the probe and the planner are host code and touch no device.
 *
 * Replaces (reference file:line):
 *   demo.py:88-95   imread(normalized_full_{j}.jpg) -> ToTensor(normalize 0.5 / 0.5) -> cat: the four candidate images, [1, 12, 512, 512]
 *   demo.py:39-41   cv2.imread of the JPEG frames a run wrote
 * For the same file the pixels are the ones Pillow (libjpeg-turbo, default settings) returns, bit for bit.  The arithmetic is libjpeg's:
 *   entropy    jdhuff.c decode_mcu: the file's DHT tables, Annex K's where one is absent; DC predicted per component, reset at every RSTn;
 *   dequantise coef * qtable[natural]; a product outside int16 gives the file the RANGE status (the library's SIMD path multiplies in 16 bits);
 *   IDCT       jidctint.c jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2): columns descaled by 11, rows by 18, then the range table on x & 1023
 *              (< 128: x + 128, < 512: 255, < 896: 0, else x - 896).  The library's SIMD transform (jidctint-sse2 / -avx2) adds in0 +- in4,
 *              in7 + in3 and in5 + in1 in 16 bits, packs each pass to int16 and saturates where the table wraps; a block that leaves those
 *              lanes (no encoder writes one) is RANGE as well, so that a decoded file always has Pillow's pixels;
 *   upsampling jdsample.c h2v2_fancy_upsample / h2v1_fancy_upsample on the component's true size dw = ceil(W / 2) [dh = ceil(H / 2)]; when
 *              dw <= 2 the library replicates instead (h2v2_upsample / h2v1_upsample): the narrow-image rule;
 *   colour     jdcolor.c ycc_rgb_convert, FIX(x) = int(x * 65536 + 0.5), clamped to 0..255.
 * Decoded: SOF0, 8 bit; 1 component, or YCbCr with luma 1x1, 2x1 or 2x2 and chroma 1x1; one interleaved scan (Ss 0, Se 63, Ah / Al 0); any
 * width and height up to max_side (partial MCUs included); DRI; optimised tables; APPn / COM skipped.
 * UNSUPPORTED (never decoded differently): progressive / extended / lossless / arithmetic files, 16-bit DQT, other sampling factors, several
 * scans, 2 or 4 components, RGB files (Adobe APP14 transform 0, or component ids R G B), Huffman table ids above 1, a height of 0 (DNL), fill
 * bytes or markers inside the scan other than the expected RSTn and EOI.
 * CORRUPT: a code that is in no table, a coefficient index past 63, a DC size above 11 or an AC size above 10, a wrong, missing or extra RSTn,
 * data that ends early (a segment, a scan without EOI), whole bytes left over in a restart interval, a malformed marker segment.
 * RANGE: a DC value or a dequantised coefficient outside int16, or a block outside the 16-bit lanes of the transform (see IDCT above).
 *
 * A batch holds files of different geometries.  lspjpeg_dec_plan() lays it out in ONE descriptor block on the host: per-file quantisation
 * tables, decode tables, output description, the entropy-coded bytes, and one entry per restart interval (found by scanning for RSTn).  The
 * caller copies the block to the device and calls lspjpeg_dec_decode(): 3 launches whatever the content --
 *   1. entropy decode: one wave per restart interval, the stream staged through LDS in 16-byte loads, int16 coefficients in natural order;
 *   2. dequantise + IDCT: one thread per block, uint8 component planes, block-padded;
 *   3. upsample + colour + store: one thread per pixel, into the output form of the file.
 * A file without restart markers (Pillow's default, and lspjpeg.h's own output) is one interval: such files are decoded in parallel with each
 * other only.  A file that fails keeps its status word (uint32 per file inside the device copy of the block, at status_offset) and its output
 * is left untouched.
 *
 * Conventions as in lspjpeg.h: device pointers, nothing allocated on the device by the library, no synchronisation, everything enqueued on the
 * given hipStream_t, no environment reads; returns 0 or a negative code (lspjpeg_dec_last_error()).
 */
#ifndef LSPJPEGDEC_H
#define LSPJPEGDEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#pragma GCC visibility push(default)

#define LSPJPEG_DEC_OK 0
#define LSPJPEG_DEC_ERR_INVALID_ARGUMENT (-1)
#define LSPJPEG_DEC_ERR_HIP (-3)

/* per-file status words */
#define LSPJPEG_DEC_STATUS_OK 0
#define LSPJPEG_DEC_STATUS_UNSUPPORTED 1
#define LSPJPEG_DEC_STATUS_CORRUPT 2
#define LSPJPEG_DEC_STATUS_RANGE 3

/* output forms */
#define LSPJPEG_DEC_FORM_RGB8 0     /* uint8 [H][W][3]: 3-component files */
#define LSPJPEG_DEC_FORM_GRAY8 1    /* uint8 [H][W]: 1-component files */
#define LSPJPEG_DEC_FORM_PLANAR_F32 2 /* float32 table[value] at ptr + c * plane_stride + y * W + x, c < components */

typedef struct lspjpeg_dec_info {
    int32_t status;                 /* LSPJPEG_DEC_STATUS_*: the header AND the marker structure of the scan */
    int32_t width, height, components;
    int32_t hsamp, vsamp;           /* luma sampling factors */
    int32_t restart_interval;       /* MCUs, 0 = none */
    int32_t mcus, segments;         /* MCUs of the scan; restart intervals found */
    int32_t default_tables;         /* bit (2 * id + class) set: that Huffman table is Annex K's because the file has none */
    uint64_t scan_offset, scan_bytes; /* the entropy-coded data: from the byte after SOS up to the EOI marker */
} lspjpeg_dec_info;

typedef struct lspjpeg_dec_output {
    void *ptr;                      /* device pointer; NULL in every entry plans for the host only (lspjpeg_dec_host_coefficients) */
    const float *table;             /* device pointer of 256 floats (PLANAR_F32) */
    int64_t plane_stride;           /* elements between channels (PLANAR_F32) */
    int32_t form;
    int32_t reserved;
} lspjpeg_dec_output;

typedef struct lspjpeg_dec_summary {
    uint32_t files, segments;
    uint32_t max_blocks, max_pixels; /* of one file: the grid of stages 2 and 3 */
    uint64_t total_blocks;
    uint64_t bytes;                 /* of the descriptor block */
    uint64_t workspace_bytes;
    uint64_t status_offset;         /* of the uint32 [files] status words inside the block */
} lspjpeg_dec_summary;

const char *lspjpeg_dec_last_error(void);

/* geometry, sampling, restart interval and whether the file can be decoded; max side LSPJPEG_MAX_SIDE of lspjpeg.h (8192) */
int lspjpeg_dec_probe(const unsigned char *bytes, size_t len, lspjpeg_dec_info *info);

/* Lays n files out in one descriptor block.  blob == NULL: returns the bytes needed.  Otherwise writes the block (cap >= that many bytes;
 * blob 16-byte aligned) and returns its size.  A file the parser refuses gets its status in the block and costs nothing else; outs[i] of such a
 * file is ignored.  outs[i].form must fit the file's components.  Negative on an invalid argument. */
int64_t lspjpeg_dec_plan(const unsigned char *const *files, const size_t *lens, const lspjpeg_dec_output *outs, int n, int max_side, void *blob,
                         size_t cap);
int lspjpeg_dec_summary_of(const void *blob, lspjpeg_dec_summary *out);
/* what the planner recorded, for checks: file i's info (scan_offset is then the offset of its data inside the block), its quantisation table of
 * component c in natural order, and segment k as (file, first MCU, MCUs, begin, end) with begin / end offsets inside the block */
int lspjpeg_dec_plan_file(const void *blob, int i, lspjpeg_dec_info *info);
int lspjpeg_dec_plan_qtable(const void *blob, int i, int c, uint16_t out[64]);
int lspjpeg_dec_plan_segment(const void *blob, int k, uint32_t *file, uint32_t *mcu0, uint32_t *nmcu, uint64_t *begin, uint64_t *end);
/* stage 1 on the host, with the code the kernel runs: file i's int16 coefficients, [blocks][64] in MCU order, natural order inside a block.
 * Returns the file's status word after stage 1 (>= 0) or a negative code; out must hold mcus * blocks-per-MCU * 64 values, and its content
 * means something only on status 0. */
int lspjpeg_dec_host_coefficients(const void *blob, int i, int16_t *out, size_t cap_values);

/* Enqueues the three stages.  blob_host is the planner's block, blob_dev its copy on the device (16-byte aligned; the kernels write only its
 * status words), workspace_dev 256-byte aligned with summary.workspace_bytes bytes; its content on entry is irrelevant. */
int lspjpeg_dec_decode(const void *blob_host, void *blob_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
