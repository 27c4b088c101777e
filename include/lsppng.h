/* lsppng.h -- C ABI of the PNG decoder: the lossless way image files reach the renderer, beside lspjpegdec.h.
 * Exported by livespeechportraits_amd/liblspf2f.so; the decode is gfx950 only, the probe, the planner and the host twins are host code and touch no
 * device.
 *
 * Replaces (reference file:line):
 *   demo.py:88-95   imread(normalized_full_{j}) -> ToTensor(normalize 0.5 / 0.5) -> cat, for candidate crops kept as PNG
 * For the same file the pixels are the ones Pillow returns, bit for bit: np.asarray(Image.open(f).convert("RGB")) for colour types 2, 3 and 6 (the
 * palette lookup for type 3; the alpha channel of type 6 dropped, not composited), Image.open(f).convert("L") for types 0 and 4 (alpha dropped).
 *
 * Decoded (status 0): non-interlaced files of colour type 2 (RGB), 6 (RGBA), 0 (grey) and 4 (grey + alpha) at bit depth 8, and of colour type 3
 * (palette) at bit depth 1, 2, 4 and 8; any width and height from 1 up to max_side (at most LSPPNG_MAX_SIDE); all five filter types, mixed freely
 * between rows; any number of IDAT chunks, empty ones included, cut anywhere in the stream; stored, fixed-Huffman and dynamic-Huffman deflate blocks
 * in any order.  Ancillary chunks are skipped, tRNS among them: alpha is no output.
 *
 * The arithmetic is the PNG specification's (section 9, Filtering):
 *   bpp = max(1, channels * depth / 8); a = the reconstructed byte bpp to the left (0 before the row's start), b = the reconstructed byte above,
 *   c = the one above a; the row above the first row is zeros;
 *   None: x; Sub: x + a; Up: x + b; Average: x + floor((a + b) / 2) on the 9-bit sum; Paeth: x + the one of a, b, c nearest to a + b - c, ties in
 *   the order a, b, c; all modulo 256.
 *   Palette files: pixel x of a row is the depth-bit field x of it, most significant bits first; its PLTE entry is the pixel.
 *
 * UNSUPPORTED (never decoded differently): Adam7 interlace; bit depth 16; grey at depth 1, 2 or 4; a side above max_side; APNG (acTL / fcTL / fdAT
 * present); an unknown critical chunk.
 * CORRUPT, found by the host planner in the container: a wrong signature; a chunk that runs past the file; a wrong CRC on any chunk, ancillary ones
 * included; a chunk type with a non-letter byte; IHDR not first, not 13 bytes, or repeated; zero width or height (or one of 2^31 and above);
 * compression or filter method not 0, an interlace method above 1; an illegal colour type / bit depth pair; for type 3: PLTE missing, after IDAT,
 * repeated, of a length not divisible by 3, empty, or with more than 2^depth entries; IDAT chunks not consecutive, or no IDAT; IEND missing or not
 * empty; bytes after IEND; a zlib header that is not CM 8, CINFO at most 7, check bits divisible by 31, FDICT 0.  A CORRUPT container is CORRUPT
 * whatever else it holds; an UNSUPPORTED file's zlib header is not looked at.
 * CORRUPT, found on the device by the code the host twin runs, in the stream: block type 3; a stored block whose LEN is not the complement of NLEN;
 * HLIT above 286 or HDIST above 30; a repeat code 16 with nothing before it; a repeat that runs past HLIT + HDIST; no code for symbol 256; an
 * over-subscribed code-length set; an incomplete one, except a literal/length or distance code that is a single code of one bit (zlib's inftrees.c
 * admits it) and a distance code with no code at all (RFC 1951 3.2.7: a block of literals only); the code-length code itself may be neither; a bit
 * pattern that is in no code; length symbol 286 or 287, distance symbol 30 or 31; a distance that reaches before the first output byte; output that
 * would pass H * (1 + rowbytes) bytes, or a final block that ends short of it; input that ends inside the stream; an Adler-32 that does not match;
 * bytes left in the IDAT data after the Adler-32; a filter byte above 4; a palette index at or past the PLTE entry count.
 * Several of these are stricter than Pillow (which stops reading once the last row is out, takes a missing IEND and does not check IDAT's CRC).  The
 * contract has one direction: a file with status 0 has Pillow's pixels, and a refused file leaves its output untouched.
 *
 * A batch holds files of different geometries.  lsppng_dec_plan() lays it out in ONE descriptor block on the host: per file the geometry, the output
 * description, the palette and the concatenated IDAT payload; a refused file costs its status word only.  The caller copies the block to the device
 * and calls lsppng_dec_decode(): 3 launches whatever the content --
 *   1. pngdec_inflate: one wave per file.  The symbol walk is wave-uniform; the lanes stage the stream through LDS in 16-byte loads, fill the decode
 *      tables, copy matches 64 bytes per step inside a 32 KiB window kept in LDS, flush the window in 16-byte stores and sum the Adler-32;
 *   2. pngdec_unfilter: one wave per file, in place: lane l owns row 64 * band + l and runs l steps (of 4 bytes) behind lane l - 1, taking the row
 *      above from that lane by a cross-lane move; the last row of a band waits in LDS for the next band.  The palette indices are checked here, so
 *      that a refused file is refused before its first pixel is stored;
 *   3. pngdec_store: one thread per pixel: palette lookup, alpha drop, the table of PLANAR_F32, into the file's output form.
 * A file that fails keeps its status word (uint32 per file inside the device copy of the block, at status_offset) and its output is left untouched.
 *
 * Conventions as in lspjpegdec.h: device pointers, nothing allocated on the device by the library, no synchronisation, everything enqueued on the
 * given hipStream_t, no environment reads; returns 0 or a negative code (lsppng_dec_last_error()).
 */
#ifndef LSPPNG_H
#define LSPPNG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#pragma GCC visibility push(default)

#define LSPPNG_DEC_OK 0
#define LSPPNG_DEC_ERR_INVALID_ARGUMENT (-1)
#define LSPPNG_DEC_ERR_HIP (-3)

#define LSPPNG_MAX_SIDE 8192

/* per-file status words */
#define LSPPNG_DEC_STATUS_OK 0
#define LSPPNG_DEC_STATUS_UNSUPPORTED 1
#define LSPPNG_DEC_STATUS_CORRUPT 2

/* output forms: those of lspjpegdec.h */
#define LSPPNG_DEC_FORM_RGB8 0       /* uint8 [H][W][3]: colour types 2, 3, 6 */
#define LSPPNG_DEC_FORM_GRAY8 1      /* uint8 [H][W]: colour types 0, 4 */
#define LSPPNG_DEC_FORM_PLANAR_F32 2 /* float32 table[value] at ptr + c * plane_stride + y * W + x, c < components */

typedef struct lsppng_dec_info {
    int32_t status;                 /* LSPPNG_DEC_STATUS_*: the container and the zlib header */
    int32_t width, height;
    int32_t color_type, depth;
    int32_t components;             /* of the output: 3 or 1 */
    uint64_t idat_bytes;            /* the concatenated IDAT payload */
    uint64_t raw_bytes;             /* height * (1 + rowbytes): the filtered scanlines */
} lsppng_dec_info;

typedef struct lsppng_dec_output {
    void *ptr;                      /* device pointer; NULL in every entry plans for the host only */
    const float *table;             /* device pointer of 256 floats (PLANAR_F32) */
    int64_t plane_stride;           /* elements between channels (PLANAR_F32) */
    int32_t form;
    int32_t reserved;
} lsppng_dec_output;

typedef struct lsppng_dec_summary {
    uint32_t files, max_pixels;     /* max_pixels of one file: the grid of launch 3 */
    uint64_t bytes;                 /* of the descriptor block */
    uint64_t workspace_bytes;
    uint64_t status_offset;         /* of the uint32 [files] status words inside the block */
} lsppng_dec_summary;

const char *lsppng_dec_last_error(void);

/* geometry, colour type, depth and whether the file can be decoded (max side LSPPNG_MAX_SIDE); host only */
int lsppng_dec_probe(const unsigned char *bytes, size_t len, lsppng_dec_info *info);

/* Lays n files out in one descriptor block.  blob == NULL: returns the bytes needed.  Otherwise writes the block (cap >= that many bytes; blob
 * 16-byte aligned) and returns its size.  A file the planner refuses gets its status in the block and costs nothing else; outs[i] of such a file is
 * ignored.  outs[i].form must fit the file's components.  Negative on an invalid argument. */
int64_t lsppng_dec_plan(const unsigned char *const *files, const size_t *lens, const lsppng_dec_output *outs, int n, int max_side, void *blob, size_t cap);
int lsppng_dec_summary_of(const void *blob, lsppng_dec_summary *out);
/* what the planner recorded for file i, for checks */
int lsppng_dec_plan_file(const void *blob, int i, lsppng_dec_info *info);
/* launch 1 and the Adler-32 check on the host, with the code the kernel runs (the lanes as loops): returns the file's status word (>= 0) or a
 * negative code; out holds raw_bytes filtered scanlines on status 0 and means nothing otherwise */
int lsppng_dec_host_scanlines(const void *blob, int i, unsigned char *out, size_t cap);
/* launches 2 and 3 likewise, behind launch 1: the status word, and on status 0 the pixels [H][W][components] */
int lsppng_dec_host_pixels(const void *blob, int i, unsigned char *out, size_t cap);

/* Enqueues the three launches.  blob_host is the planner's block, blob_dev its copy on the device (16-byte aligned; the kernels write only its status
 * words), workspace_dev 256-byte aligned with summary.workspace_bytes bytes; its content on entry is irrelevant. */
int lsppng_dec_decode(const void *blob_host, void *blob_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
