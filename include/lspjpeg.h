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
 * Not supported: 4:4:4, progressive, optimised Huffman tables, restart markers, EXIF / ICC.
 *
 * Output bound (per frame, what lspjpeg_capacity_bytes() returns): a block codes at most 11 + 11 bits of DC (longest DC code, 11-bit
 * difference) and at most 63 AC symbols of <= 16 + 10 bits (a nonzero coefficient, a ZRL for 16 zeros or one EOB per block: never more
 * symbols than AC positions), so T <= 1660 bits per block; stuffing at most doubles the ceil(T / 8) bytes; + 2 bytes of EOI:
 *     capacity = 2 * ceil(blocks * 1660 / 8) + 2,   blocks = H * W / 64 * (components == 3 ? 1.5 : 1)
 * Nothing the encoder writes can pass it, so there is no overflow path.
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

#define LSPJPEG_MAX_SIDE 8192       /* keeps a frame's bit offsets below 2^32 */
#define LSPJPEG_BLOCK_BITS 1660     /* worst-case coded bits of one 8x8 block (see the bound above) */

typedef struct lspjpeg_handle lspjpeg_handle;

/* components 3: frames uint8 [H][W][3] RGB (Engine.forward_image), H and W multiples of 16; components 1: uint8 [H][W] (the edge maps of
 * FeatureMapRasteriser.rasterise(as_uint8=True)), multiples of 8.  quality 1..100.  Builds the quantisation tables and the file header. */
int lspjpeg_create(int width, int height, int components, int quality, lspjpeg_handle **out);
int lspjpeg_destroy(lspjpeg_handle *h);
const char *lspjpeg_last_error(void);

/* the file's bytes from SOI through SOS (APP0 JFIF 1.01, DQT per table, SOF0, DHT per table, SOS): copied to buf when cap is large
 * enough (buf may be NULL to query); returns the length, or a negative code */
int64_t lspjpeg_header(const lspjpeg_handle *h, unsigned char *buf, size_t cap);
/* bytes reserved per frame in dst (the bound above) */
size_t lspjpeg_capacity_bytes(const lspjpeg_handle *h);
size_t lspjpeg_workspace_bytes(const lspjpeg_handle *h, int batch);

/* batch frames:  src_dev    uint8 frames, contiguous, [batch][H][W][components]
 *                dst_dev    uint8 [batch][capacity]: frame i's entropy-coded segment + EOI at dst_dev + i * capacity
 *                sizes_dev  uint32 [batch]: its byte count (the file is header + those bytes)
 *                workspace  lspjpeg_workspace_bytes(h, batch) bytes; its content on entry is irrelevant */
int lspjpeg_encode(const lspjpeg_handle *h, const unsigned char *src_dev, int batch, unsigned char *dst_dev, uint32_t *sizes_dev,
                   void *workspace_dev, size_t workspace_bytes, void *hip_stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
