/* lspavi.h -- C ABI of the Motion-JPEG AVI muxer of the render loop: a batch of encoded frames and its audio become finished file bytes on
 * the device.  Exported by livespeechportraits_amd/liblspf2f.so; gfx950 only (the container's headers and index are host code, video.py).
 *
 * Replaces, per clip (reference file:line):
 *   demo.py:275-285  write_video_with_audio: every pred_<n>.jpg read back, re-encoded (DIVX) and muxed with the clip's WAV by an external program
 * with an AVI 1.0 file whose video chunks ARE the JPEG files of include/lspjpeg.h ('MJPG') and whose audio stream is the 16 kHz waveform
 * (float PCM as the reference's `-codec copy` of a float WAV, or 16-bit PCM).  DIVX, OpenDML and files >= 2 GiB are not supported.
 *
 * lspavi_pack() writes one fragment of the file's 'movi' list, for frames frame0 .. frame0 + batch - 1:
 *     per frame k:  ['01wb' <4 bytes length> samples [s(frame0 + k), s(frame0 + k + 1)),  s(f) = f * rate / fps (integer division)]   with audio
 *                    '00dc' <4 bytes length> <jpeg header bytes> <frame k's entropy-coded bytes + EOI>  [0x00 when the length is odd]
 * Audio formats: LSPAVI_AUDIO_F32 copies the samples bit for bit; LSPAVI_AUDIO_S16 writes rintf(x * 32767.0f) clamped to +-32767, NaN as 0.
 * Chunk starts are even; lengths are the unpadded ones.  Every byte of the fragment is written exactly once, by one lane, whatever the
 * buffer held before; bytes at or above the fragment's length are never touched.
 *
 * Output bound (what lspavi_capacity_bytes() returns), rounded up to a multiple of 16:
 *     batch * (8 + jpeg_header_len + jpeg_capacity + 1)  +  with audio: batch * 8 + (batch * rate / fps + 1) * bytes per sample
 * Nothing lspavi_pack writes can pass it (sizes above jpeg_capacity are clamped to it), so there is no overflow path.
 *
 * Conventions: device pointers, nothing allocated by the library, no synchronisation, enqueued on the given hipStream_t in a fixed number of
 * launches (2) whatever the content; returns 0 or a negative code (lspavi_last_error()).  capacity_bytes / workspace_bytes touch no device.
 */
#ifndef LSPAVI_H
#define LSPAVI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden: exactly the functions declared below are exported */
#pragma GCC visibility push(default)

#define LSPAVI_OK 0
#define LSPAVI_ERR_INVALID_ARGUMENT (-1)
#define LSPAVI_ERR_UNSUPPORTED (-2)
#define LSPAVI_ERR_HIP (-3)

#define LSPAVI_MAX_BATCH 64
/* audio_format: the WAVEFORMATEX wFormatTag the stream is declared with */
#define LSPAVI_AUDIO_NONE 0
#define LSPAVI_AUDIO_S16 1
#define LSPAVI_AUDIO_F32 3

const char *lspavi_last_error(void);

/* bytes a fragment of `batch` frames can take (the bound above); 0 for arguments lspavi_pack would refuse */
size_t lspavi_capacity_bytes(int jpeg_header_len, size_t jpeg_capacity, int batch, int audio_format, int rate, int fps);
size_t lspavi_workspace_bytes(int batch);

/* batch frames:  jpeg_header_dev  the lspjpeg_header() bytes, uploaded once by the caller; 4-byte aligned
 *                jpeg_dev         uint8 [batch][jpeg_capacity] and
 *                sizes_dev        uint32 [batch], exactly what lspjpeg_encode left; jpeg_dev 4-byte aligned
 *                wave_dev         float32 [wave_samples], the clip's waveform (NULL: no audio chunks, audio_format LSPAVI_AUDIO_NONE);
 *                                 s(frame0 + batch) <= wave_samples is checked here, on the host
 *                out_dev          uint8 [out_capacity], 16-byte aligned, out_capacity >= lspavi_capacity_bytes(...)
 *                index_dev        uint32 [2 * batch][4]: per chunk, in file order: ckid, flags (0x10), offset of the chunk header relative to
 *                                 the fragment's start, unpadded length -- `chunk count` rows are written (batch, with audio 2 * batch)
 *                status_dev       uint32 [4]: fragment bytes, chunk count, largest video chunk, largest audio chunk (unpadded lengths)
 *                workspace        lspavi_workspace_bytes(batch) bytes, 16-byte aligned; its content on entry is irrelevant
 * Sources are read as aligned dwords: the buffers must be readable up to the next multiple of 4 of their lengths. */
int lspavi_pack(const unsigned char *jpeg_header_dev, int jpeg_header_len, const unsigned char *jpeg_dev, size_t jpeg_capacity,
                const uint32_t *sizes_dev, int batch, const float *wave_dev, int64_t wave_samples, int64_t frame0, int rate, int fps,
                int audio_format, unsigned char *out_dev, size_t out_capacity, uint32_t *index_dev, uint32_t *status_dev,
                void *workspace_dev, size_t workspace_bytes, void *hip_stream);

/* ---- many files from one batch: live sessions (livespeechportraits_amd/live_render.py) ------------------------------------------------
 * lspavi_pack_multi() splits one encoded batch into at most LSPAVI_MAX_STREAMS runs.  A run is the consecutive frames
 * [first, first + count) of the batch, count >= 1; runs are ascending and cover the batch.  Every run is a fragment of a file of its own:
 * its bytes and its index entries (offsets relative to its own start) are exactly what lspavi_pack() writes for those frames alone from a
 * linear waveform.  The audio of a run comes from a ring: stream sample i lives at ring_dev[i % ring_samples], and the file's frame k carries
 * stream samples sample0 + [s(k), s(k + 1)), s as above on the FILE's frame numbers -- so a file may begin at any stream frame.
 * The host side of the call refuses a run whose span sample0 + [s(frame0), s(frame0 + count)) leaves [avail_begin, avail_end) or is longer
 * than the ring, and launches nothing then: the device never reads a sample the caller did not vouch for.
 *
 * Output: run j's fragment starts at a 16-byte-aligned offset of out_dev (status row j).  Every byte below a fragment's length is written
 * exactly once, by one lane; the up to 14 bytes between a fragment's end and the next fragment's start and everything above the last
 * fragment are never touched.  Still two launches per call, whatever the number of runs.
 *
 * Output bound (lspavi_capacity_bytes_multi), a multiple of 16: lspavi_pack's bound with the audio term at 4 bytes per sample, plus per run
 * 16 bytes (alignment) and 4 bytes (each run may round one sample up):
 *     batch * (8 + jpeg_header_len + jpeg_capacity + 1)  +  batch * 8 + (batch * rate / fps + 1) * 4  +  runs * 20 */
#define LSPAVI_MAX_STREAMS 16

typedef struct lspavi_run {
    int32_t first, count;        /* frames [first, first + count) of the batch */
    int32_t audio_format;        /* LSPAVI_AUDIO_*, per run: the files belong to the caller */
    int32_t reserved;            /* 0 */
    int64_t frame0;              /* the FILE's number of the run's first frame, 0..2^31 */
    const float *ring_dev;       /* float32 [ring_samples], 4-byte aligned; NULL with LSPAVI_AUDIO_NONE (the fields below are then ignored) */
    int64_t ring_samples;        /* 1..2^31 */
    int64_t sample0;             /* the stream sample of the first sample of the file's frame 0, >= 0 */
    int64_t avail_begin, avail_end; /* the ring holds stream samples [avail_begin, avail_end), at most ring_samples of them */
} lspavi_run;

/* uint32 per status row: offset of the fragment in out_dev, fragment bytes, chunk count, largest video chunk, largest audio chunk
 * (unpadded lengths), the fragment's first row in index_dev, 0, 0 */
#define LSPAVI_STATUS_WORDS 8

/* 0 for arguments lspavi_pack_multi would refuse; no device is touched */
size_t lspavi_capacity_bytes_multi(int jpeg_header_len, size_t jpeg_capacity, int batch, int runs, int rate, int fps);
size_t lspavi_workspace_bytes_multi(int batch);

/* As lspavi_pack, with:  runs        nruns entries, read during the call (they travel to the device as kernel arguments: nothing is uploaded)
 *                        index_dev   uint32 [2 * batch][4]: the chunks of all runs in batch order; run j's rows start at its status row's
 *                                    word 5, offsets relative to the run's own fragment
 *                        status_dev  uint32 [nruns][LSPAVI_STATUS_WORDS]
 *                        workspace   lspavi_workspace_bytes_multi(batch) bytes */
int lspavi_pack_multi(const unsigned char *jpeg_header_dev, int jpeg_header_len, const unsigned char *jpeg_dev, size_t jpeg_capacity,
                      const uint32_t *sizes_dev, int batch, const lspavi_run *runs, int nruns, int rate, int fps, unsigned char *out_dev,
                      size_t out_capacity, uint32_t *index_dev, uint32_t *status_dev, void *workspace_dev, size_t workspace_bytes,
                      void *hip_stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
