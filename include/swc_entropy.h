/*
 * swc_entropy.h — C-ABI of the SWC2 code container of libswc_hip.so: a ragged batch of utterances <-> their SWC2 file images,
 * every (utterance, group) stream entropy-coded on the device by an adaptive range coder over the FSQ levels, every image under a
 * CRC-32.  A header of its own beside swc_codes.h (the SWC1 container, which stays what it is), csrc/swc_entropy.hip behind it,
 * csrc/swc_entropy_model.h the arithmetic that host and device share.  Conventions are those of swc_flac_enc.h: device pointers,
 * `stream` a hipStream_t passed as void*, every call only enqueues, 0 on success or a negative SWC_E_* code with the library's
 * last-error text saying why; nothing allocates or synchronises; every argument is checked before any launch.
 *
 * No trained checkpoint exists for this codec: every size quoted for this container was measured on codes of synthetic weights or
 * on generated streams.  Nobody has measured the gain on real speech codes.
 *
 * ------------------------------------------------------------------------------------------------------------------------
 * THE FORMAT CONTRACT (normative: tests/entropy_ref.py restates it in plain Python from this text alone).  All fields are little
 * endian; everything is exact integer arithmetic: an image is a function of its codes and levels alone.
 *
 * Limits   1 <= G <= 8 groups.  Four levels L0 .. L3, each in 2 .. 16; n_codes = L0 L1 L2 L3 <= 16384.  T <= SWC_ENTROPY_MAX_FRAMES
 *          = 65536 frames.  w = the bit length of n_codes - 1 (11 for the shipped [8, 7, 6, 6]; at least 4).  Level d of code c
 *          is (c / base_d) % L_d with base = 1, L0, L0 L1, L0 L1 L2.
 *
 * Image     0  "SWC2"        4  u32 T          8  u8 G        9  u8 0 (version)
 *          10  u8 L0 L1 L2 L3                 14  u16 0
 *          16  u32 body_bytes = 4 G + the sum of len_g
 *          20  u32 crc = zlib's CRC-32 over the bytes [0, 20) followed by the bytes [24, 24 + body_bytes)
 *          24  G x u32: (mode_g << 24) | len_g       then the G streams back to back, in group order
 *
 * Modes    0  raw: code t at bits [w t, w t + w) of the stream, least-significant bit first; (T w + 7) / 8 bytes, pad bits zero.
 *          1  adaptive, order 0.        2  adaptive, order 1.
 *          The encoder produces all three and keeps the shortest; a tie goes to the lowest mode number, so a chosen adaptive
 *          stream is strictly shorter than raw (and, ending in the coder's four bytes, at least 4 bytes long).  An empty
 *          utterance has G streams of mode 0 and length 0: 24 + 4 G bytes.  A stream that holds an invalid value (outside
 *          [0, n_codes), compared at the element's full width) is written raw with the low w bits of every value, and each
 *          invalid value adds one to the `bad` counter: what the SWC1 pack does.
 *
 * Model    Each dimension d has rows of L_d counts, all starting at 1.  Order 0: one row per dimension.  Order 1: L_d rows per
 *          dimension; the row used is the level of dimension d in the previous frame, row 0 for frame 0.  The symbols of a frame
 *          are coded in the order d = 0, 1, 2, 3.  After symbol s is coded: row[s] += 24; if sum(row) > 8192 then every entry
 *          becomes (x + 1) >> 1.  (A dimension's rows depend on that dimension's history alone.)
 *
 * Coder    32-bit state, no carries, TOP = 1 << 24, BOT = 1 << 16, all arithmetic mod 2^32:
 *            encode(cum, f, tot):  range /= tot;  low += cum * range;  range *= f;
 *                while ((low ^ (low + range)) < TOP  ||  (range < BOT && ((range = (0 - low) & (BOT - 1)), true))):
 *                    emit low >> 24;  low <<= 8;  range <<= 8
 *            start: low = 0, range = 0xffffffff;  finish: emit the four bytes of low, high byte first.
 *            decode: code = the first four bytes, high byte first (missing bytes read as 0);  range /= tot;
 *                v = min((code - low) / range, tot - 1);  s = the symbol with cum(s) <= v < cum(s) + f(s);  then the same update,
 *                shifting a byte into code (code = code << 8 | byte; bytes behind the stream read as 0) where the encoder emits one.
 *
 * Three properties, each with its argument:
 *  1. range >= BOT holds between symbols.  The loop ends only when its second clause is false with the first, that is with
 *     range >= BOT.  A row's sum is at most 8192 (it is halved as soon as it exceeds that), so range / tot >= 2^16 / 2^13 = 8: no
 *     division is by zero; f >= 1 keeps range >= 8 after the narrowing; cum + f <= tot gives (cum + f) (range / tot) <= range, so
 *     no product wraps.
 *  2. Renormalisation emits at most SWC_ENTROPY_MAX_RENORM = 3 bytes per symbol.  The second clause replaces range by
 *     x = (0 - low) & 0xffff only when low and low + range differ in their top byte with range < 2^16, so low lies x <= range
 *     below a multiple of 2^24 and x >= 1.  After k turns the low 8 k bits of low are zero, so x is then a multiple of 2^(8 k).
 *     Turn 1 leaves range >= 2^8 (from range >= 8 or x >= 1, times 2^8); turn 2 leaves range >= 2^16 (both range and x are
 *     >= 2^8); a turn 3 can then only come from the first clause and leaves range >= 2^24, with which the first clause is false.
 *  3. The decoder's low and range follow the encoder's recurrence over the symbols it decodes, and every decoded symbol is a
 *     valid one (v is clamped below tot, every count of a valid symbol is >= 1): they never depend on a stream byte except
 *     through a valid symbol, so properties 1 and 2 hold for any bytes.  Any bytes therefore decode to T valid codes in exactly
 *     4 T symbol steps of at most 3 byte reads each.
 *  Every device loop has a trip count that is a function of T, G and the levels: corrupt input costs a wrong answer, never a
 *  long-running kernel.
 * ------------------------------------------------------------------------------------------------------------------------
 */
#ifndef SWC_ENTROPY_H_
#define SWC_ENTROPY_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_ENTROPY_HEADER_BYTES 24
#define SWC_ENTROPY_MAX_FRAMES 65536
#define SWC_ENTROPY_MAX_GROUPS 8
#define SWC_ENTROPY_MIN_LEVEL 2
#define SWC_ENTROPY_MAX_LEVEL 16
#define SWC_ENTROPY_MAX_CODES 16384
#define SWC_ENTROPY_INC 24        /* added to the coded symbol's count */
#define SWC_ENTROPY_LIMIT 8192    /* a row whose sum exceeds this is halved */
#define SWC_ENTROPY_MAX_RENORM 3  /* bytes per symbol at most (property 2) */

/* swc_entropy_parse's refusals */
#define SWC_ENTROPY_E_MAGIC (-1)     /* not "SWC2" */
#define SWC_ENTROPY_E_VERSION (-2)   /* version or reserved bytes not 0 */
#define SWC_ENTROPY_E_LIMITS (-3)    /* G, T or a level outside the limits */
#define SWC_ENTROPY_E_TRUNCATED (-4) /* fewer bytes than the header and body_bytes announce */
#define SWC_ENTROPY_E_TABLE (-5)     /* a mode above 2, a raw length that is not (T w + 7) / 8, an adaptive length outside
                                        [4, raw), or lengths that do not sum to body_bytes */
#define SWC_ENTROPY_E_CRC (-6)

/* 24 + 4 G + G ((T w + 7) / 8): the largest image of T frames (every stream raw), or -1 for an argument outside the limits.
 * Plain host arithmetic. */
int64_t swc_entropy_worst_bytes(int64_t T, int32_t G, const int32_t* levels4);

/*
 * Sizes of one swc_entropy_encode_batch call, plain host arithmetic over a HOST array of B lengths.
 *   *out_cap (written when out_cap is not NULL): the worst-case total output, the sum of swc_entropy_worst_bytes over the rows.
 *   returns the workspace size in bytes for B rows of up to max(n_frames) frames (a multiple of 256, 0 for B == 0), or -1 for a
 *       bad argument: B outside 0 .. 65535, a NULL array with B > 0, G or levels outside the limits, a length outside
 *       0 .. SWC_ENTROPY_MAX_FRAMES.
 * With SLOT = (max_T w + 7) / 8 rounded up to 4, the workspace holds, each part on a 256-byte boundary: int32 adaptive stream
 * lengths [B][G][2], uint32 table entries [B][G], and the adaptive streams' slots [B][G][2][SLOT].
 */
int64_t swc_entropy_workspace_bytes(const int64_t* n_frames, int32_t B, int32_t G, const int32_t* levels4, int64_t* out_cap);

/*
 * B utterances -> their B SWC2 images, back to back.
 *
 * Rows    `rows`, `ldg` and `n_frames` are DEVICE arrays of B int64 each, the address-list convention of the batched pack call of
 *         swc_codes.h: rows[b] is the address of utterance b's group-0 row, ldg[b] its group stride in ELEMENTS, code (g, t) is
 *         the element rows[b][g ldg[b] + t]; elements are `elem_size` = 4 (int32) or 8 (int64) bytes, one size per call.
 *         n_frames[b] <= 0 is an empty utterance and rows[b] is not read; max_frames is the host's upper bound of n_frames[]: a
 *         row that claims more is coded as max_frames frames.  `levels_host4`: the four levels, a HOST array.
 * Output  image b lies at out[byte_off[b] .. byte_off[b] + sizes[b]); byte_off[0] = 0, byte_off[b + 1] = byte_off[b] + sizes[b]:
 *         row order, no gaps.  byte_off and sizes are DEVICE int64 [B].  Nothing of `out` behind the last image is written and
 *         nothing outside the workspace.  An image depends on its own row's codes alone: not on B, its place in the batch,
 *         max_frames, the row's alignment or what the buffers held before.
 * Count   `bad` (may be NULL) is a DEVICE int32 counter, incremented by one for every invalid value.  The caller zeroes it.
 * Kernels code (one wave per (utterance, group, order): the adaptive streams into slots of the workspace; a write past the slot
 *         is dropped while the length goes on counting, and such a stream cannot win), layout (the modes, the table entries, the
 *         exclusive scan of the image sizes over B), gather (header, table and the chosen streams into the images, raw streams
 *         packed from the codes; aligned dword stores inside an image, single bytes at its ragged ends), crc (one workgroup per
 *         image: a CRC per lane over its share, combined by x^(8 n) mod P; the four bytes at 20).  Phases are ordered by being
 *         separate launches; no workgroup waits for another; no float arithmetic.
 * Checks  rows, ldg, n_frames, levels_host4, out, byte_off, sizes, workspace not NULL; the device arrays 8-byte aligned, the
 *         workspace 16-byte; 0 <= B <= 65535; elem_size 4 or 8; 1 <= G <= 8 and the levels inside the limits;
 *         0 <= max_frames <= SWC_ENTROPY_MAX_FRAMES; out_bytes >= B swc_entropy_worst_bytes(max_frames), so no image can leave
 *         the buffer; workspace_bytes >= swc_entropy_workspace_bytes for B lengths max_frames.  B == 0 launches nothing.
 */
int swc_entropy_encode_batch(const void* const* rows, const int64_t* ldg, const int64_t* n_frames, int32_t elem_size,
                             const int32_t* levels_host4, int32_t G, int32_t max_frames, void* out, int64_t out_bytes,
                             int64_t* byte_off, int64_t* sizes, int32_t* bad, void* workspace, int64_t workspace_bytes, int32_t B,
                             void* stream);

/*
 * The inverse, in ONE launch: B G streams inside one device byte buffer -> the zero-padded int32 batch codes[g ldg + b ldb + t],
 * g < G, b < B, t < L.  (The host has parsed the images with swc_entropy_parse: it needs them to size anything.)
 *
 * Input   stream (b, g) = the stream_len[b G + g] bytes at bytes + stream_off[b G + g], of mode stream_mode[b G + g]; utterance b
 *         has n_frames[b] frames.  All four are DEVICE arrays (int64, int64, int32, int64).  No alignment is needed and only
 *         bytes of the streams are read; bytes a stream should have but has not read as 0.  A stream that does not lie inside
 *         [0, in_bytes), a mode outside 0 .. 2 or a negative n_frames[b] counts as ONE bad value and gives an empty row;
 *         n_frames[b] > L is cut at L.
 * Output  every t in [0, L) of every (g, b) row is written: the code for t < n_frames[b], 0 from there to L, exactly as the
 *         batched unpack of swc_codes.h does.  Nothing else is written.
 * Count   `bad` (may be NULL) is incremented by one for every raw value >= n_codes (the codebook size of the model the codes are
 *         for); values pass through unchanged.  An adaptive stream yields values below L0 L1 L2 L3 only, whatever its bytes.
 * Checks  pointers, 0 <= B <= 65535, 1 <= G <= 8, the levels, 0 <= L <= SWC_ENTROPY_MAX_FRAMES, ldb >= L, ldg >= B ldb,
 *         in_bytes >= 0, n_codes >= 1.
 */
int swc_entropy_decode_batch(const void* bytes, int64_t in_bytes, const int64_t* stream_off, const int64_t* stream_len,
                             const int32_t* stream_mode, const int64_t* n_frames, const int32_t* levels_host4, int32_t G,
                             int32_t* codes, int64_t ldg, int64_t ldb, int64_t L, int32_t B, int32_t n_codes, int32_t* bad,
                             void* stream);

/*
 * One image on the HOST (plain host code, no device): validates the magic, the version, the limits, the stream table (every
 * entry and its sum against body_bytes) and, when check_crc != 0, the CRC.  Reads image[0, bytes) only and nothing behind the
 * image, so a concatenation of images is walked by moving on by 24 + body_bytes = stream_off[G - 1] + stream_len[G - 1].
 * Writes *T, *G, levels4[4], and stream_off / stream_len / stream_mode [8] (offsets from the image's first byte); any of them may
 * be NULL.  Returns 0 or one of SWC_ENTROPY_E_*; nothing is written on a refusal past the entries already walked.
 */
int swc_entropy_parse(const void* image, int64_t bytes, int32_t check_crc, int32_t* T, int32_t* G, int32_t* levels4,
                      int64_t* stream_off, int64_t* stream_len, int32_t* stream_mode);

#ifdef __cplusplus
}
#endif
#endif /* SWC_ENTROPY_H_ */
