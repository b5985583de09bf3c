/*
 * swc_flac.h — FLAC on the device path: a batch of FLAC files, one frame per work item.  A header of its own beside swc.h,
 * swc_audio.h, swc_codes.h and the metrics headers.  Two halves, two libraries:
 *
 *   swc_flac_index (libswc_io.so, host C, csrc/swc_flac.c): walks a stream WITHOUT entropy decoding and returns one
 *       record per frame.  Both CRCs of every frame are checked here, and the sample total.
 *   swc_flac_decode_batch (libswc_hip.so, csrc/swc_flac_gpu.hip): the compressed bytes of B files -> interleaved int16
 *       samples, all frames of all files in parallel.  The frame decoder itself is csrc/swc_flac_frame.h, one text for host
 *       and device.  The MD5 signature of STREAMINFO is NOT checked on this path (it needs the decoded samples on the host).
 *
 * Conventions of the device half are those of swc_codes.h: device pointers, `stream` a hipStream_t passed as void*, every
 * call only enqueues, 0 on success or a negative SWC_E_* code with swc_last_error() giving the text; nothing allocates or
 * synchronises; arguments are checked before any launch.  Format source: RFC 9639.
 */
#ifndef SWC_FLAC_H_
#define SWC_FLAC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* return codes of swc_flac_index: the FLAC_E_* of csrc/swc_flac.c, and one more */
#define SWC_FLAC_E_FORMAT (-1)   /* not a FLAC stream / malformed */
#define SWC_FLAC_E_CRC (-2)      /* a frame failed its CRC-8 or CRC-16 */
#define SWC_FLAC_E_UNSUP (-3)    /* reserved codes, frame parameters that contradict STREAMINFO */
#define SWC_FLAC_E_SPACE (-4)    /* more samples than the caller's ceiling */
#define SWC_FLAC_E_HOSTONLY (-6) /* a valid stream that is not for the device path: more than 16 bits per sample, more than
                                    8 channels, variable block size, frame numbers that do not count from 0 (a stream cut out
                                    of another), a frame above SWC_FLAC_MAX_FRAME_BYTES; swc_flac_decode (the host decoder)
                                    takes it */

/* per-frame status words of swc_flac_decode_batch (and of swc_flac_decode_frame, csrc/swc_flac_frame.h) */
#define SWC_FLAC_ST_OK 0
#define SWC_FLAC_ST_ENTRY 1      /* the table entry (frame or its file) points outside a buffer or contradicts itself: dropped, never read */
#define SWC_FLAC_ST_RESERVED 2   /* a reserved code: subframe type, padding bit, residual method, precision 1111, negative shift */
#define SWC_FLAC_ST_ORDER 3      /* partition or predictor order inconsistent with the block size, wasted bits >= sample width */
#define SWC_FLAC_ST_LENGTH 4     /* the last subframe, byte aligned, does not end exactly at n_bytes - 2 */
#define SWC_FLAC_ST_TRUNCATED 5  /* the subframes need more bits than the frame holds */
#define SWC_FLAC_ST_RANGE 6      /* a decoded sample does not fit the subframe's sample width (RFC 9639 forbids it) */

#define SWC_FLAC_MAX_BLOCKSIZE 65536
#define SWC_FLAC_MAX_BPS 16
#define SWC_FLAC_MAX_CHANNELS 8
#define SWC_FLAC_MAX_FRAME_BYTES (1 << 24) /* 16 MiB: eight verbatim 17-bit channels of 65 536 samples take 1.1 MiB; bit counts inside a
                                              frame (unary runs included) then fit 32 bits */
#define SWC_FLAC_MAX_FRAMES (1 << 24)   /* frames per swc_flac_decode_batch call */
#define SWC_FLAC_PLANE_ALIGN 64         /* int32 elements: every file's planes start on a 256-byte boundary of the workspace */

/* One frame.  Complete: the device re-parses nothing of the frame header. */
typedef struct swc_flac_frame {
    int64_t byte_off;      /* of the frame's sync code: in the stream (swc_flac_index), in `bytes` (swc_flac_decode_batch) */
    int64_t first_sample;  /* per channel, within its file */
    int32_t n_bytes;       /* whole frame: header, subframes, padding, CRC-16 */
    int32_t blocksize;     /* samples per channel, 1 .. SWC_FLAC_MAX_BLOCKSIZE */
    int32_t file;          /* index into files[] (0 from swc_flac_index) */
    int32_t hdr_bytes;     /* header length including its CRC-8: the first subframe starts here */
    int32_t chan_assign;   /* the header's channel assignment: 0 .. 7 independent (channels - 1), 8 left/side, 9 side/right, 10 mid/side */
    int32_t reserved;      /* 0 */
} swc_flac_frame;

/* One file of a batch. */
typedef struct swc_flac_file {
    int64_t out_off;       /* ELEMENT offset in out_i16 of sample 0, channel 0; the file owns [out_off, out_off + n_samples channels) */
    int64_t n_samples;     /* per channel */
    int64_t plane_off;     /* int32 ELEMENT offset in the workspace of this file's planes [channels][n_samples] */
    int32_t first_frame;   /* the file's frames are frames[first_frame, first_frame + n_frames), in stream order */
    int32_t n_frames;
    int32_t channels;      /* 1 .. 8 */
    int32_t bps;           /* 4 .. 16 */
    int32_t blocksize;     /* the stream's fixed block size: every frame but the last holds this many samples */
    int32_t reserved;      /* 0 */
} swc_flac_file;

/* What swc_flac_index says of the stream as a whole. */
typedef struct swc_flac_stream {
    int64_t total;         /* samples per channel = the sum of the frames' block sizes (= STREAMINFO's total when that is non-zero) */
    int64_t first_frame;   /* byte offset of the first frame */
    int32_t rate, channels, bps, blocksize;
} swc_flac_stream;

/*
 * Host index of one stream (libswc_io.so).  Skips an ID3v2 tag, parses the metadata blocks, then walks the frames: at a frame
 * start the header is parsed and its CRC-8 checked; the frame ends at the next position where a header parses with a valid
 * CRC-8, carries the following frame number, and the running CRC-16 from the frame's start equals the two bytes in front of
 * it (a false sync inside a frame fails that and is skipped); the last frame ends at the end of the data.  Frame k of the
 * stream must carry the number k (numbering is absolute, from 0): first_sample = k blocksize is what the device relies on.
 * Writes at most `cap` records to `frames` (may be NULL when cap == 0) and returns the NUMBER OF FRAMES of the stream — call
 * again with more room if it exceeds cap — or a negative SWC_FLAC_E_* code.  max_samples (> 0) is the caller's ceiling of
 * samples per channel: a stream whose STREAMINFO or whose frames claim more is SWC_FLAC_E_SPACE; nothing is sized by the
 * stream's own claims.
 */
int64_t swc_flac_index(const uint8_t* data, size_t n, int64_t max_samples, swc_flac_stream* info, swc_flac_frame* frames,
                       int64_t cap);

/*
 * The workspace of one swc_flac_decode_batch call, plain host arithmetic over HOST arrays of B entries: file b's planes are
 * channels[b] * n_samples[b] int32 at element offset plane_off[b] (written when plane_off is not NULL), each on a
 * SWC_FLAC_PLANE_ALIGN boundary.  Returns the size in bytes (a multiple of 256, 0 for an empty batch), -1 for a bad argument.
 */
int64_t swc_flac_decode_workspace_bytes(const int64_t* n_samples, const int32_t* channels, int32_t B, int64_t* plane_off);

/*
 * B files -> their samples, in two launches.
 *
 * Input   `bytes` [n_bytes] holds the files' frames, anywhere, at any alignment; `frames` [n_frames] and `files` [B] are
 *         DEVICE tables (swc_flac_index's records with byte_off rebased and `file` set).  An entry that does not lie inside
 *         its buffer — a frame outside bytes, a span outside out_i16 or the workspace, a block outside its file, a file index
 *         outside [0, B) — or that contradicts itself is dropped with SWC_FLAC_ST_ENTRY and never read through.
 * Frame   kernel: one work item per frame runs swc_flac_decode_frame into int32 planes of the workspace and stores
 *         status[f], one int32 per frame, EVERY frame's word is written.  Whatever the bytes say, only bytes of the frame are
 *         read and only the frame's own block of its planes is written.
 * Output  kernel: undoes the stereo decorrelation, shifts bps < 16 up by 16 - bps, narrows to int16 and writes sample i,
 *         channel c of file b at out_i16[out_off[b] + i channels + c].  Every sample of every file whose frames all have
 *         status 0 is written; NOTHING else of out_i16 is: not a file with a failed frame, not the gaps between files.
 *         The spans of the files (out_i16 and planes) must not overlap — the tables live on the device, so that is the
 *         CALLER's check.  A file's samples depend on that file's bytes alone: not on B, its place in the batch, the
 *         alignment of its bytes or the launch geometry.  No atomics.
 * Checks  pointers (all may be NULL when n_frames == 0), n_bytes >= 0, 0 <= n_frames <= SWC_FLAC_MAX_FRAMES,
 *         0 <= B <= 65535, out_elems >= 0, workspace 16-byte aligned, workspace_bytes >= 0.  n_frames == 0 launches nothing.
 */
int swc_flac_decode_batch(const void* bytes, int64_t n_bytes, const swc_flac_frame* frames, int32_t n_frames,
                          const swc_flac_file* files, int32_t B, int16_t* out_i16, int64_t out_elems, int32_t* status,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* The same with the frame kernel's mapping given: frames_per_wave active lanes of every 64-lane wave (1, 2, 4 ... 64), 0 = the
 * library's choice.  Results do not depend on it; tools/bench_flac.py measures it. */
int swc_flac_decode_batch_ex(const void* bytes, int64_t n_bytes, const swc_flac_frame* frames, int32_t n_frames,
                             const swc_flac_file* files, int32_t B, int16_t* out_i16, int64_t out_elems, int32_t* status,
                             void* workspace, int64_t workspace_bytes, int32_t frames_per_wave, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_FLAC_H_ */
