/* lspjpegdec.h -- C ABI of the JPEG decoder (baseline files; complete progressive files as an option): the inverse of lspjpeg.h, and the way image files reach the renderer.
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
 * Progressive files (SOF2) are an option: LSPJPEG_DEC_FLAG_PROGRESSIVE in lspjpeg_dec_probe_flags() / lspjpeg_dec_plan_flags().  Without the flag
 * nothing above changes: a progressive file is UNSUPPORTED, and a batch of baseline files runs the three launches it always ran.  Under the flag
 * (jdphuff.c, ITU T.81 Annex G):
 *   decoded      SOF2, 8 bit; 1 component, or YCbCr with the sampling factors above; Huffman table ids 0..3, redefined between scans at will (the
 *                planner keeps, per scan, the tables as they stand at its SOS); up to LSPJPEG_DEC_MAX_SCANS scans; DRI between scans (an interval
 *                counts interleaved MCUs in a scan of all components, and the component's own blocks in a scan of one: such a scan covers
 *                ceil(Wc / 8) x ceil(Hc / 8) blocks of the component's own extent in raster order, not the MCU-padded grid); RSTn numbered from 0 in
 *                every scan; APPn / COM between scans.  The four procedures: first DC scan (difference shifted by Al, prediction per component,
 *                reset at RSTn), DC refinement (one bit per block), first AC scan (run / size symbols, EOBn runs, band Ss..Se), AC refinement
 *                (correction bits, new +-(1 << Al) coefficients, ZRL counting coefficients without history only).  The file must be COMPLETE: at
 *                EOI every coefficient 0..63 of every component has been refined down to Al = 0.  libjpeg then applies no block smoothing and the
 *                coefficients are those of the baseline file of the same image, so stages 2 and 3 are the ones above;
 *   UNSUPPORTED  an incomplete file; a progression libjpeg warns about and decodes on (a coefficient whose first scan has Ah != 0, whose later
 *                scan has Ah != the Al reached, or that is coded again after reaching Al = 0; AC before the component's DC); a DQT after the first
 *                SOS (libjpeg latches tables per component); DNL; a scan of two components out of three, or of all components in another order than
 *                the frame's; a scan that uses a Huffman table the file has not defined by then; more than LSPJPEG_DEC_MAX_SCANS scans; SOF0 files
 *                with several scans, with or without the flag; and 16-bit DQT, RGB / Adobe transform 0, other sampling factors, fill bytes inside
 *                a scan, as above;
 *   CORRUPT      a scan libjpeg refuses: Ss > Se, Se > 63, Ss = 0 with Se != 0, an AC scan with more than one component, Ah != 0 with
 *                Al != Ah - 1, Al > 13, an unknown or repeated component; in the data: a code in no table, a coefficient (or a ZRL) past Se, a DC
 *                size above 11, an AC size above 10 in a first scan or other than 0 / 1 in a refinement, an end-of-band run that reaches past the
 *                scan's last block (a run still open at an RSTn is dropped there, as libjpeg does), a wrong, missing or extra RSTn, data that ends
 *                early, whole bytes left over in a restart interval;
 *   RANGE        a DC prediction, a shifted value or a corrected coefficient outside int16.
 * A block with progressive files costs ONE more launch, whatever their number: jpegdec_progressive, one wave per progressive file, which zeroes
 * the file's coefficients and walks its scans in file order over them (a refinement needs what the earlier scans left).  Stages 2 and 3 then run
 * once for all files; baseline and progressive files mix freely.  Not done: parallelism inside a progressive file (the restart intervals of one
 * scan, or independent scans, on several waves): two waves writing different coefficients of one block would break the 16-byte block moves, and a
 * refinement scan reads what the earlier scans left.  That stays out of scope under LSPJPEG_DEC_FLAG_PARALLEL too: progressive files are decoded
 * in parallel with each other only.
 * For a progressive file lspjpeg_dec_info.restart_interval is the interval in force at the first scan, mcus the interleaved MCUs of the frame,
 * segments the restart intervals of ALL scans, scan_offset / scan_bytes the bytes from the first scan's data up to the EOI marker (the markers
 * between the scans included); default_tables is 0.
 *
 * Parallel decode INSIDE a restart interval of a baseline file is an option: LSPJPEG_DEC_FLAG_PARALLEL in lspjpeg_dec_plan_flags()
 * (lspjpeg_dec_probe_flags() accepts the flag and ignores it).  Without the flag nothing above changes: the block is byte for byte the same and
 * the same kernels run.  Under the flag every restart interval of every baseline file is cut into subsequences of a fixed number of bytes of the
 * stuffed stream (lspjpeg_dec_plan_parallel() reports it), and stage 1 of those files is ONE launch of another kernel, jpegdec_entropy_parallel:
 * one workgroup per restart interval whose lanes each decode one subsequence from a guessed parser state, repair the guesses by handing exit
 * states on until nothing changes (self-synchronising Huffman decoding, Weissenberger and Schmidt 2018 / 2021: exact, because the first lane's
 * state is true; uncapped, so at the worst as slow as the serial walk), and then write the coefficients in today's layout.  Status words are the
 * serial decoder's for every file, the earliest failure in stream order inside an interval included; stages 2 and 3 are untouched.
 * lspjpeg_dec_decode() under the flag still enqueues 3 launches whatever the content (4 when the block holds progressive files, which go through
 * jpegdec_progressive exactly as without the flag), synchronises nothing and allocates nothing; the route keeps its state in LDS, so
 * summary.workspace_bytes does not grow.  The flag combines freely with LSPJPEG_DEC_FLAG_PROGRESSIVE.
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

/* flags of lspjpeg_dec_probe_flags / lspjpeg_dec_plan_flags */
#define LSPJPEG_DEC_FLAG_PROGRESSIVE 1u
#define LSPJPEG_DEC_FLAG_PARALLEL 2u    /* baseline files: stage 1 decodes inside a restart interval in parallel (plan only; the probe ignores it) */
#define LSPJPEG_DEC_MAX_SCANS 64    /* of one progressive file; more is UNSUPPORTED */

/* one scan of a progressive file, as the planner recorded it */
typedef struct lspjpeg_dec_scan {
    int32_t components;             /* 1, or all of the frame's (interleaved) */
    uint8_t component[4];           /* indices in frame order */
    uint8_t dc_table[4], ac_table[4]; /* the table ids its SOS names, per scan component */
    int32_t ss, se, ah, al;
    int32_t restart_interval;       /* the DRI in force, in units; 0 = none */
    int32_t units;                  /* interleaved MCUs, or the one component's own blocks: ceil(Wc / 8) * ceil(Hc / 8) */
    int32_t segments;               /* restart intervals found */
    int32_t reserved;
    uint64_t begin, end;            /* inside the block: the first entropy-coded byte, the marker that ends the scan */
} lspjpeg_dec_scan;

const char *lspjpeg_dec_last_error(void);

/* geometry, sampling, restart interval and whether the file can be decoded; max side LSPJPEG_MAX_SIDE of lspjpeg.h (8192) */
int lspjpeg_dec_probe(const unsigned char *bytes, size_t len, lspjpeg_dec_info *info);

/* Lays n files out in one descriptor block.  blob == NULL: returns the bytes needed.  Otherwise writes the block (cap >= that many bytes;
 * blob 16-byte aligned) and returns its size.  A file the parser refuses gets its status in the block and costs nothing else; outs[i] of such a
 * file is ignored.  outs[i].form must fit the file's components.  Negative on an invalid argument. */
int64_t lspjpeg_dec_plan(const unsigned char *const *files, const size_t *lens, const lspjpeg_dec_output *outs, int n, int max_side, void *blob,
                         size_t cap);
/* The two above with flags (LSPJPEG_DEC_FLAG_*); flags = 0 is exactly lspjpeg_dec_probe / lspjpeg_dec_plan. */
int lspjpeg_dec_probe_flags(const unsigned char *bytes, size_t len, unsigned flags, lspjpeg_dec_info *info);
int64_t lspjpeg_dec_plan_flags(const unsigned char *const *files, const size_t *lens, const lspjpeg_dec_output *outs, int n, int max_side, unsigned flags,
                               void *blob, size_t cap);
/* for checks: the number of scans of file i (0 for a file that was not planned as a progressive one), and scan s of it */
int lspjpeg_dec_plan_scans(const void *blob, int i);
int lspjpeg_dec_plan_scan(const void *blob, int i, int s, lspjpeg_dec_scan *out);
/* for checks: how restart interval k (as lspjpeg_dec_plan_segment counts them) is cut under LSPJPEG_DEC_FLAG_PARALLEL: the bytes of one
 * subsequence and their number.  Negative on a block planned without the flag. */
int lspjpeg_dec_plan_parallel(const void *blob, int k, uint32_t *subseq_bytes, uint32_t *subsequences);
int lspjpeg_dec_summary_of(const void *blob, lspjpeg_dec_summary *out);
/* what the planner recorded, for checks: file i's info (scan_offset is then the offset of its data inside the block), its quantisation table of
 * component c in natural order, and segment k as (file, first MCU, MCUs, begin, end) with begin / end offsets inside the block */
int lspjpeg_dec_plan_file(const void *blob, int i, lspjpeg_dec_info *info);
int lspjpeg_dec_plan_qtable(const void *blob, int i, int c, uint16_t out[64]);
int lspjpeg_dec_plan_segment(const void *blob, int k, uint32_t *file, uint32_t *mcu0, uint32_t *nmcu, uint64_t *begin, uint64_t *end);
/* stage 1 on the host, with the code the kernel runs: file i's int16 coefficients, [blocks][64] in MCU order, natural order inside a block.
 * Returns the file's status word after stage 1 (>= 0) or a negative code; out must hold mcus * blocks-per-MCU * 64 values, and its content
 * means something only on status 0.  A progressive file's scans are run in file order with the procedures the kernel runs. */
int lspjpeg_dec_host_coefficients(const void *blob, int i, int16_t *out, size_t cap_values);
/* for checks: what this thread's last lspjpeg_dec_host_coefficients did on a block planned with LSPJPEG_DEC_FLAG_PARALLEL (it then runs the kernel's
 * subsequence decoder, fixed point and write pass with the lanes as loops): the most rounds the fixed point took in any chunk, and the number of
 * true entry states that stood inside a block.  Both 0 for any other block. */
int lspjpeg_dec_host_parallel_stats(uint32_t *rounds, uint32_t *midblock_entries);

/* Enqueues the three stages (and, between stages 1 and 2, the progressive files' launch when the block holds any).  blob_host is the planner's block, blob_dev its copy on the device (16-byte aligned; the kernels write only its
 * status words), workspace_dev 256-byte aligned with summary.workspace_bytes bytes; its content on entry is irrelevant. */
int lspjpeg_dec_decode(const void *blob_host, void *blob_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
