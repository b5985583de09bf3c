/*
 * swc_flac_enc.h — FLAC written on the device: a batch of mono int16 waveforms -> their complete .flac file images, one
 * frame per workgroup.  A header of its own beside swc_flac.h (the decode direction), csrc/swc_flac_enc.hip behind it.
 * Conventions are those of swc_codes.h: device pointers, `stream` a hipStream_t passed as void*, every call only enqueues, 0
 * on success or a negative SWC_E_* code with swc_last_error() giving the text; nothing allocates or synchronises; every
 * argument is checked before any launch.  Format source: RFC 9639.
 *
 * ------------------------------------------------------------------------------------------------------------------------
 * THE FORMAT CONTRACT (normative: tests/flac_fixed_ref.py restates it in numpy from this text alone)
 *
 * The encoder is deterministic: a file's bytes are a function of its samples, the rate, the block size and the MD5 switch.
 *
 * Input    One row of n >= 1 mono int16 samples.  Block size BS in {256, 512, 1024, 2048, 4096}.  Rate: one of RFC 9639's
 *          frame-header table (88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000: codes 1 .. 11),
 *          or any other rate 1 .. 65535 (code 0b1101 = 13, the rate in Hz in 16 bits behind the block-size bytes).  Nothing
 *          else: no second channel, other widths, LPC subframes, wasted bits or Rice escape codes.
 *
 * Frames   Frame k holds the samples [k BS, min(n, (k + 1) BS)); bs is their count.  In order:
 *            bytes 0-1  0xFF 0xF8 (sync, fixed block size)
 *            byte 2     block-size code << 4 | rate code.  Block-size code: 8 + log2(BS / 256) when bs == BS.  A shorter
 *                       (last) frame uses 6 when bs <= 256 (bs - 1 follows in 8 bits) and 7 otherwise (bs - 1 in 16 bits):
 *                       a short frame never uses a table code, also not when bs is 256, 512 ...
 *            byte 3     0x08: channel assignment 0, sample-size code 4 (16 bits), reserved bit 0
 *            then       the frame number k in the UTF-8-like coding (1 byte below 2^7, 2 below 2^11, 3 below 2^16, 4 below
 *                       2^21, 5 below 2^26), the block-size bytes (code 6 / 7), the rate bytes (code 13), big endian
 *            then       CRC-8 (polynomial 0x07, initial value 0) over all header bytes before it.
 *          The longest header is 4 + 5 + 2 + 2 + 1 = SWC_FLAC_ENC_MAX_HEADER = 14 bytes.  One subframe follows, zero bits up
 *          to the next byte boundary, then CRC-16 (polynomial 0x8005, initial value 0, big endian) over the whole frame
 *          before it.
 *
 * Subframe For the block s[0 .. bs), all arithmetic in exact integers.  Candidates and their sizes in bits:
 *            CONSTANT  only when all samples are equal: 8 + 16.  Header byte 0x00, then s[0] in 16 bits.
 *            VERBATIM  8 + 16 bs.  Header byte 0x02, then every sample in 16 bits (two's complement, big endian).
 *            FIXED (o, p)  for every predictor order o in 0 .. min(4, bs - 1) and partition order p in 0 .. 6 with
 *                      bs mod 2^p == 0 and (bs >> p) > o:
 *                        e[i], i in [o, bs), is the o-th finite difference (o = 0: s[i]; 1: s[i] - s[i-1];
 *                          2: s[i] - 2 s[i-1] + s[i-2]; 3: s[i] - 3 s[i-1] + 3 s[i-2] - s[i-3];
 *                          4: s[i] - 4 s[i-1] + 6 s[i-2] - 4 s[i-3] + s[i-4]); |e| <= 2^19.
 *                        zz[i] = 2 e when e >= 0, else -2 e - 1.
 *                        Partition j in 0 .. 2^p - 1 of length L = bs >> p covers i in [max(j L, o), (j + 1) L).
 *                        cost(j, k) = sum over the partition of (zz >> k), plus (k + 1) times its sample count.
 *                        k_j = the SMALLEST k in 0 .. 14 that minimises cost(j, k).
 *                        bits(o, p) = 8 + 16 o + 6 + sum over j of (4 + cost(j, k_j)).
 *                      Written as: header byte (8 + o) << 1, the o warm-up samples s[0 .. o) in 16 bits each, 2 bits 00 (Rice
 *                      method 0), p in 4 bits, then per partition k_j in 4 bits (never the escape code 15) and per sample
 *                      zz >> k_j zero bits, a one bit, and the low k_j bits of zz.
 *          Choice: the fewest bits.  Among candidates of equal size CONSTANT comes first, then the FIXED candidates by
 *          smaller o, then smaller p; VERBATIM is taken only when nothing else is strictly smaller.
 *
 * Stream   "fLaC", then one STREAMINFO block flagged last (0x80 0x00 0x00 0x22 and 34 bytes; 42 bytes with the marker):
 *          minimum and maximum block size, both BS (16 bits each); minimum and maximum frame size in bytes as found over
 *          the file's frames (24 bits each); rate (20 bits), channels - 1 = 0 (3 bits), bits per sample - 1 = 15 (5 bits),
 *          n (36 bits); the MD5 (RFC 1321) of the row's 2 n bytes as they lie in memory (little endian), or 16 zero bytes
 *          when MD5 is switched off.  Then the frames, back to back.
 * ------------------------------------------------------------------------------------------------------------------------
 */
#ifndef SWC_FLAC_ENC_H_
#define SWC_FLAC_ENC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_FLAC_ENC_STREAM_HEADER 42 /* "fLaC" + the STREAMINFO block */
#define SWC_FLAC_ENC_MAX_HEADER 14    /* the longest frame header, CRC-8 included */
#define SWC_FLAC_ENC_MAX_FRAMES (1 << 24) /* frames per swc_flac_encode_batch call: B * ceil(max_n / blocksize) */
#define SWC_FLAC_ENC_MAX_RATE_BITS 65535  /* the largest rate outside RFC 9639's table */

/*
 * Sizes of one swc_flac_encode_batch call, plain host arithmetic over a HOST array of B lengths.
 *   *out_cap (written when out_cap is not NULL): the worst-case total output in bytes, the sum over the files with
 *       n_samples[b] > 0 of 42 + ceil(n / blocksize) * (SWC_FLAC_ENC_MAX_HEADER + 1 + 2) + 2 n (every frame VERBATIM).
 *   returns the workspace size in bytes for B files of up to max(n_samples) samples each (a multiple of 256, 0 for B == 0),
 *       or -1 for a bad argument: B outside 0 .. 65535, a NULL array with B > 0, a block size outside the five, a length
 *       outside 0 .. 2^31 - 1, more than SWC_FLAC_ENC_MAX_FRAMES frames.
 * With F = ceil(max_n / blocksize) frames per file at most and SLOT = (SWC_FLAC_ENC_MAX_HEADER + 1 + 2 blocksize + 2) rounded
 * up to 16, the workspace holds, each part on a 256-byte boundary: int64 frame offsets [B][F], int32 frame sizes [B][F], 16
 * MD5 bytes [B], int32 {min, max} frame size [B][2], and the frame slots [B][F][SLOT].
 */
int64_t swc_flac_encode_workspace_bytes(const int64_t* n_samples, int32_t B, int32_t blocksize, int64_t* out_cap);

/*
 * B waveforms -> B file images, back to back.
 *
 * Input   `rows` [B] DEVICE array of the rows' addresses (int16, 2-byte alignment is all a row needs), `n_samples` [B] DEVICE
 *         int64 lengths; max_n is the host's bound on them.  A row with n <= 0 — or, against the caller's word, n > max_n —
 *         has size 0 and writes nothing.  rate and blocksize as in the contract above; md5 != 0 computes the signature.
 * Output  Image b is the contract's stream for row b and lies at out[byte_off[b] .. byte_off[b] + sizes[b]); byte_off[0] = 0
 *         and byte_off[b + 1] = byte_off[b] + sizes[b]: row order, no gaps.  byte_off and sizes are DEVICE int64 [B].
 *         Nothing of `out` behind the last image is written and nothing outside the workspace.  An image depends on its row's
 *         samples alone: not on B, its place in the batch, max_n, the row's alignment or what the buffers held before.
 * Kernels frame (one workgroup per frame: the exhaustive search, the bits, both CRCs, into a fixed-stride slot of the
 *         workspace), MD5 (one lane per file; only when md5 != 0), layout per file (exclusive scan of its frame sizes, their
 *         minimum and maximum), layout across files (exclusive scan of the file sizes), gather (slots and the 42 header bytes
 *         into the images).  Phases are ordered by being separate launches; no workgroup waits for another; no float
 *         arithmetic, no global atomics.
 * Checks  rows, n_samples, out, byte_off, sizes, workspace not NULL; byte_off / sizes / n_samples / rows 8-byte aligned, the
 *         workspace 16-byte; 0 <= B <= 65535; 0 <= max_n < 2^31; B * ceil(max_n / blocksize) <= SWC_FLAC_ENC_MAX_FRAMES;
 *         out_bytes >= the worst case of B files of max_n samples (swc_flac_encode_workspace_bytes's *out_cap for B lengths
 *         max_n), so no image can leave the buffer; workspace_bytes >= that function's result for those lengths.
 *         B == 0 launches nothing (and then every pointer may be NULL).
 */
int swc_flac_encode_batch(const void* rows, const int64_t* n_samples, int32_t rate, int32_t blocksize, int32_t md5, void* out,
                          int64_t out_bytes, int64_t* byte_off, int64_t* sizes, void* workspace, int64_t workspace_bytes,
                          int64_t max_n, int32_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_FLAC_ENC_H_ */
