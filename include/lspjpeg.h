/* lspjpeg.h -- C ABI of the baseline JPEG encoder of the render loop: the frames demo.py writes, encoded on the device.
 * Exported by livespeechportraits_amd/liblspf2f.so; gfx950 only, no CPU path for the encode (the header is built on the host).
 *
 * Replaces, per frame (reference file:line):
 *   demo.py:268-272            visualizer.save_images(save_root, visuals, str(ind + 1)): pred_<n>.jpg, and input_<n>.jpg with save_input
 *   util/visualizer.py:120-136 save_images -> util/util.py:70-72 save_image: Image.fromarray(img).save(path), a `.jpg` name
 * i.e. Pillow's defaults: quality 75 (any 1..100 here), baseline, 4:2:0 for colour, the standard Huffman tables, a JFIF 1.01 header.  For the
 * same uint8 pixels the file (lspjpeg_header() bytes + one frame's encoded bytes) is byte-identical to what Pillow (libjpeg-turbo) writes:
 *   colour     jccolor.c rgb_ycc_convert (16 fractional bits), jcsample.c h2v2_downsample (2x2 box, bias 1, 2, 1, 2 ... per output row);
 *   transform  jfdctint.c jpeg_fdct_islow on samples - 128, output scaled by 8;
 *   quantise   divisor qtable[k] << 3, rounded half away from zero (what jcdctmgr.c's reciprocal multiply computes);
 *   tables     Annex K scaled by jpeg_quality_scaling (q < 50 ? 5000 / q : 200 - 2q; (t * s + 50) / 100 clamped to 1..255);
 *   entropy    zigzag order, DC predicted per component over the whole frame (no restart markers), MCU = Y0 Y1 Y2 Y3 Cb Cr (grayscale: one
 *              block), ZRL / EOB with the four standard tables, 0xFF followed by 0x00, the final byte padded with 1-bits, then EOI.
 * With options (lspjpeg_create_opts; Pillow's optimize=True, restart_marker_rows / restart_marker_blocks), still byte for byte Pillow's file:
 *   restart    jchuff.c emit_restart: after every restart_interval MCUs but the last group the bits are padded to a byte with 1-bits (stuffed
 *              with 0x00 if that makes 0xFF), FF D0+n follows unstuffed (n = 0..7, wrapping), and every component's DC prediction starts
 *              again at 0; no marker behind the last interval.  jcmarker.c: DRI (FF DD 00 04 hi lo) between the last DHT and SOS.
 *   optimize   jchuff.c's two passes per frame: the scan's symbols are counted per table id (12 DC categories, 256 AC run / size symbols
 *              with ZRL and EOB; id 0 for Y, 1 for Cb and Cr; DC differences under the restart rule), and jpeg_gen_optimal_table builds each
 *              table (csrc/jpegenc_core.h states it).  The frame's bytes are then DHT DC0, AC0 [, DC1, AC1] (a segment each), [DRI,] SOS, the
 *              scan, EOI, and lspjpeg_header() ends behind SOF0.  A file is header + frame bytes either way.
 * A format handle (lspjpeg_create_format; Pillow's subsampling=0 / 1 / 2 and pictures of any size), still byte for byte Pillow's file.  With
 * luma factors (hs, vs) = (2, 2) for 4:2:0, (2, 1) for 4:2:2, (1, 1) for 4:4:4 (csrc/jpegenc_geom.h states the grid):
 *   MCU grid   colour: ceil(W / 8hs) x ceil(H / 8vs) MCUs, each its hs * vs luma blocks (row-major), Cb, Cr.  Grey: a non-interleaved scan, one
 *              block per MCU, ceil(W / 8) x ceil(H / 8) blocks.  SOF0 carries the true W and H, hs << 4 | vs for luma and 0x11 for chroma.
 *   columns    jcsample.c expand_right_edge: the last pixel of a row is repeated BEFORE downsampling, and the bias patterns run on from column 0
 *              into the padding: h2v2 (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2 ...; h2v1 (a + b + bias) >> 1 with bias 0, 1, 0, 1 ...;
 *              4:4:4 chroma is the converted sample itself.
 *   rows       jcprepct.c: the last pixel row is repeated up to a multiple of vs only; the plane is downsampled; then the last row of each
 *              COMPONENT plane is repeated down to the block grid (for even H under 4:2:0 the padded chroma rows repeat box(H - 2, H - 1)).
 *   dummy      jccoefct.c: a luma block of an edge MCU whose column >= ceil(W / 8) or row >= ceil(H / 8) is not transformed: its AC coefficients
 *              are 0 and its quantised DC is that of the block before it in the MCU's coding order (a chain: Y3 = Y2 = Y1 = Y0 in the bottom-right
 *              MCU).  It codes as DC category 0 + EOB, and counts in optimize's histograms and in the DC prediction.  The first luma block of an
 *              MCU and the chroma blocks are never dummy.
 *   restart    the interval counts MCUs of that grid (Pillow's restart_marker_rows: rows * MCUs per row, capped at 65535).
 *   the rest   tables, DCT, quantiser, entropy coding, stuffing, optimize, DRI / RSTn: as above.
 * Not supported: other sampling factors, progressive, EXIF / ICC.
 *
 * Output bound (per frame, what lspjpeg_capacity_bytes() returns): a block codes at most 11 + 11 bits of DC (longest DC code, 11-bit
 * difference) and at most 63 AC symbols of <= 16 + 10 bits (a nonzero coefficient, a ZRL for 16 zeros or one EOB per block: never more
 * symbols than AC positions), so T <= 1660 bits per block; stuffing at most doubles the ceil(T / 8) bytes; + 2 bytes of EOI:
 *     capacity = 2 * ceil(blocks * 1660 / 8) + 2,   blocks = H * W / 64 * (components == 3 ? 1.5 : 1)
 * (a format handle: blocks = MCUs * blocks per MCU of its grid, dummy blocks included: a dummy block codes 6 bits without optimize: category 0 and EOB)
 * Nothing the encoder writes can pass it, so there is no overflow path.
 * A handle made with options restates the bound from its parts (a handle without keeps the value above exactly):
 *   bits per block  B = 1660 with the Annex K tables; 1665 with optimize, where a DC code can be 16 bits long: 16 + 11 + 63 * (16 + 10);
 *   stream bytes    every interval is padded to a byte on its own, at most 7 bits each: P <= ceil(blocks * B / 8) + intervals;
 *   stuffing        at most doubles them (the padded byte of an interval included): 2 * P;
 *   markers         2 bytes of RSTn behind every interval but the last, 2 bytes of EOI;
 *   tables          with optimize the frame's own DHT x 4, DRI, SOS: at most 2 * (21 + 12) + 2 * (21 + 162) + 6 + 14 = 452 bytes (a baseline scan
 *                   has 12 DC categories and 162 AC symbols: run 0..15 x size 1..10, EOB, ZRL);
 *     capacity = [452 +] 2 * (ceil(blocks * B / 8) + intervals) + 2 * (intervals - 1) + 2,   intervals = ceil(MCUs / restart_interval) or 1
 * and again nothing the encoder writes can pass it: every term bounds what one owner writes.
 *
 * Conventions: device pointers, nothing allocated by the library, no synchronisation, enqueued on the given hipStream_t in a fixed number of
 * launches (4) whatever the content; returns 0 or a negative code (lspjpeg_last_error()).  create / header / capacity_bytes / workspace_bytes
 * touch no device.
 */
#ifndef LSPJPEG_H
#define LSPJPEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden: exactly the functions declared below are exported */
#pragma GCC visibility push(default)

#define LSPJPEG_OK 0
#define LSPJPEG_ERR_INVALID_ARGUMENT (-1)
#define LSPJPEG_ERR_UNSUPPORTED (-2)
#define LSPJPEG_ERR_HIP (-3)

#define LSPJPEG_MAX_SIDE 8192       /* keeps a frame's bit offsets below 2^32 (4:2:0 and grey; lspjpeg_create_format checks its own grid) */
#define LSPJPEG_BLOCK_BITS 1660     /* worst-case coded bits of one 8x8 block (see the bound above) */

typedef struct lspjpeg_handle lspjpeg_handle;

/* components 3: frames uint8 [H][W][3] RGB (Engine.forward_image), H and W multiples of 16; components 1: uint8 [H][W] (the edge maps of
 * FeatureMapRasteriser.rasterise(as_uint8=True)), multiples of 8.  quality 1..100.  Builds the quantisation tables and the file header. */
int lspjpeg_create(int width, int height, int components, int quality, lspjpeg_handle **out);

/* The same with options; abi_version = LSPJPEG_ABI_VERSION.  optimize 0 and restart_interval 0 give what lspjpeg_create gives. */
#define LSPJPEG_ABI_VERSION 1
typedef struct lspjpeg_options {
    int32_t abi_version;
    int32_t width, height, components, quality;
    int32_t optimize;           /* 0 / 1: per-frame optimal Huffman tables (libjpeg's optimize_coding) */
    int32_t restart_interval;   /* MCUs per restart interval, 0 = none, at most 65535 */
} lspjpeg_options;
int lspjpeg_create_opts(const lspjpeg_options *o, lspjpeg_handle **out);

/* Frames of any size in 4:4:4, 4:2:2 or 4:2:0, or grey frames of any size; abi_version = LSPJPEG_FORMAT_ABI_VERSION.  The same kind of handle:
 * header, capacity_bytes, workspace_bytes, encode and destroy work on it unchanged, in four launches.  A format whose geometry lspjpeg_create
 * takes (4:2:0 with both sides multiples of 16, grey with multiples of 8) gives that handle and its kernels (src_dev 16-byte aligned); any
 * other runs kernels of its own, which read src_dev byte by byte: no alignment is asked of it.
 * Refused before any device work: INVALID_ARGUMENT for values out of range (abi_version, quality, sides outside 1..LSPJPEG_MAX_SIDE, optimize,
 * restart_interval, factors outside 1..4, a grey frame with factors other than (1, 1)); UNSUPPORTED for components other than 1 or 3, for a
 * factor pair other than the three above, e.g. (1, 2), and for a grid whose worst-case bit count blocks * 1665 does not fit 32 bits (4:4:4 at
 * 8192 x 8192). */
#define LSPJPEG_FORMAT_ABI_VERSION 1
typedef struct lspjpeg_format {
    int32_t abi_version;
    int32_t width, height, components, quality;   /* any 1..LSPJPEG_MAX_SIDE */
    int32_t optimize, restart_interval;            /* as lspjpeg_options */
    int32_t h_samp, v_samp;                        /* luma: (2,2) (2,1) (1,1); components 1: (1,1) */
} lspjpeg_format;
int lspjpeg_create_format(const lspjpeg_format *f, lspjpeg_handle **out);
int lspjpeg_destroy(lspjpeg_handle *h);
const char *lspjpeg_last_error(void);

/* the file's bytes from SOI through SOS (APP0 JFIF 1.01, DQT per table, SOF0, DHT per table, [DRI,] SOS; through SOF0 for a handle with
 * optimize): copied to buf when cap is large enough (buf may be NULL to query); returns the length, or a negative code */
int64_t lspjpeg_header(const lspjpeg_handle *h, unsigned char *buf, size_t cap);
/* bytes reserved per frame in dst (the bound above, for the handle's options) */
size_t lspjpeg_capacity_bytes(const lspjpeg_handle *h);
size_t lspjpeg_workspace_bytes(const lspjpeg_handle *h, int batch);

/* batch frames:  src_dev    uint8 frames, contiguous, [batch][H][W][components]
 *                dst_dev    uint8 [batch][capacity]: frame i's [DHT .. SOS with optimize,] entropy-coded segment + EOI at dst_dev + i * capacity
 *                sizes_dev  uint32 [batch]: its byte count (the file is header + those bytes)
 *                workspace  lspjpeg_workspace_bytes(h, batch) bytes; its content on entry is irrelevant */
int lspjpeg_encode(const lspjpeg_handle *h, const unsigned char *src_dev, int batch, unsigned char *dst_dev, uint32_t *sizes_dev,
                   void *workspace_dev, size_t workspace_bytes, void *hip_stream);

/* jpeg_gen_optimal_table on the host, with the code the kernel runs (csrc/jpegenc_core.h): freq[s] occurrences of symbol s -> bits[1..16]
 * codes per length (bits[0] = 0), the symbols in code order, and their number.  For the tests. */
int lspjpeg_host_optimal_table(const uint32_t freq[256], unsigned char bits[17], unsigned char huffval[256], int *nsymbols);

/* The block grid of a format on the host, with the code the kernels run (csrc/jpegenc_geom.h): per coded block, in coding order, six int32:
 * component (0 Y, 1 Cb, 2 Cr), block column and row in the component's plane, dummy (0 / 1), the index of the previous block of the component
 * in the frame (-1 for the first), and the index of the block whose quantised DC this one codes (itself unless dummy).  map may be NULL to
 * query; returns the number of blocks, or a negative code (the refusals of lspjpeg_create_format).  For the tests. */
int64_t lspjpeg_host_block_map(const lspjpeg_format *f, int32_t *map, size_t cap_blocks);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
