/*
 * swc_units.h — C-ABI of the token-level measures of libswc_hip.so: what a ragged batch of code streams uses of its
 * codebooks (swc_code_usage), and how far apart two batches of code streams are, position by position and as an edit
 * distance (swc_code_compare).  A header of its own beside swc_codes.h (same library, same conventions: device pointers,
 * `stream` a hipStream_t passed as void*, every call only enqueues, 0 on success or a negative SWC_E_* code with
 * swc_last_error() giving the text; nothing allocates or synchronises; every argument is checked before any launch; B == 0
 * launches nothing).  Everything here is exact integer arithmetic: there is no float operation on the device, and the
 * results do not depend on B, the order of the rows, their strides, max_frames or the launch geometry.  The text below is
 * normative: tests/units_ref.py restates it in plain Python and the kernels are compared with that bit for bit.
 *
 * Common definitions
 *
 *   Utterance  given as in swc_codes_pack_batch: `rows`, `ldg`, `n_frames` are DEVICE arrays of B int64 each.  rows[b] is the
 *              address of utterance b's group-0 row, ldg[b] its group stride in ELEMENTS: code (g, t) is the element
 *              rows[b][g ldg[b] + t], g < G.  Elements are `elem_size` = 4 (int32) or 8 (int64) bytes, one size per call; a
 *              row needs the alignment of its element only (encode()'s strided int32 views are taken as they are).
 *   Length     T_b = n_frames[b] clamped into [0, max_frames] on the device.  rows[b] of an utterance with T_b == 0 is not
 *              read.
 *   Groups     1 <= G <= SWC_UNITS_MAX_GROUPS.
 *   Levels     `levels_host4` is a HOST pointer to four values L0 .. L3 that swc_fsq_encode_levels would accept (each in
 *              2 .. 1024); n_codes = L0 L1 L2 L3 must not exceed SWC_UNITS_MAX_CODES (one group's int32 histogram is then at
 *              most 64 KB of LDS, and a symbol fits 16 bits).  Level d of a code c is (c / base_d) % L_d with
 *              base = 1, L0, L0 L1, L0 L1 L2 (the packing of swc_fsq_encode_levels).
 *   Invalid    a value outside [0, n_codes) (compared at the element's full width) is INVALID: it is counted as bad, it is
 *              never binned, it has no levels, and it EQUALS NOTHING, ITSELF INCLUDED.  Two values are "equal" when both are
 *              valid and the same number; "both valid" positions are those where neither value is invalid.
 */
#ifndef SWC_UNITS_H_
#define SWC_UNITS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_UNITS_MAX_GROUPS 8
#define SWC_UNITS_MAX_CODES 16384
/* the longest stream swc_code_compare looks at (655 s at 12.5 Hz): both symbol rows and the edit distance's boundary row
 * then fit the LDS of one compute unit */
#define SWC_UNITS_MAX_FRAMES 8192
/* frames of one (utterance, group) that one workgroup of swc_code_usage counts */
#define SWC_UNITS_CHUNK 1024
/* the longest utterance swc_code_usage takes (as SWC_CODEFILE_MAX_FRAMES) */
#define SWC_UNITS_USAGE_MAX_FRAMES (1 << 24)
/* rows of the edit distance's matrix that one strip holds (one per thread) */
#define SWC_UNITS_STRIP 256

/*
 * Codebook usage of B utterances, ACCUMULATED into three device arrays the caller zeroes once: calls over the batches of a
 * corpus add up and nothing needs to be read back in between.
 *
 *   hist     int64 [G][n_codes]   hist[g][c] += the number of (b, t), t < T_b, with code (g, t) of utterance b valid and == c
 *   repeats  int64 [G]            repeats[g] += the number of (b, t), 1 <= t < T_b, where code (g, t) equals code (g, t - 1)
 *                                 (both valid and the same number)
 *   totals   int64 [2]            totals[0] += the sum of T_b (frames seen); totals[1] += the number of invalid values among
 *                                 the G T_b values of every utterance
 *
 * Nothing else is written.  The additions are 64-bit integer atomics, so the arrays are bit-identical whatever B, the order
 * of the rows, the strides, max_frames (where it cuts nothing) or the geometry.
 * Checks  pointers, 0 <= B <= 65535, elem_size, 1 <= G <= SWC_UNITS_MAX_GROUPS, the levels,
 *         0 <= max_frames <= SWC_UNITS_USAGE_MAX_FRAMES.
 */
int swc_code_usage(const void* const* rows, const int64_t* ldg, const int64_t* n_frames, int32_t elem_size,
                   const int32_t* levels_host4, int32_t G, int32_t max_frames, int64_t* hist, int64_t* repeats,
                   int64_t* totals, int32_t B, void* stream);

/*
 * B pairs of code streams: side a (the reference) and side b, each its own address list and its own lengths
 * Ta = n_a[b], Tb = n_b[b], both clamped into [0, max_frames], max_frames <= SWC_UNITS_MAX_FRAMES.  n = min(Ta, Tb).
 * Every element of every output below is written (plain stores), and nothing else is.  All outputs are int32.
 *
 *   match        [B][G]     the number of t < n where code_a(g, t) equals code_b(g, t)
 *   both_valid   [B][G]     the number of t < n where both values are valid (the denominator of the next two)
 *   level_match  [B][G][4]  over the t < n where both values are valid: those where level d of both is the same
 *   level_l1     [B][G][4]  over the same t: the sum of |level_d(a) - level_d(b)|
 *   frame_match  [B]        the number of t < n where the codes of ALL G groups are equal
 *   bad          [B][2]     the invalid values of side a among its G Ta values, and of side b among its G Tb values
 *   edit         [B][G]     the Levenshtein distance (insertion, deletion and substitution cost 1 each; two symbols match
 *                           when they are equal in the sense above, so an invalid value matches nothing) between the two
 *                           streams of group g.  With dedup == 0 the streams are the Ta and Tb values as they are.  With
 *                           dedup != 0 every run of equal consecutive values is first collapsed to one: value t is kept when
 *                           t == 0 or it does not equal value t - 1 (so every invalid value is kept, and so is the value
 *                           behind one)
 *   len_a, len_b [B][G]     the lengths the edit distance ran on (Ta and Tb without dedup)
 *
 * edit is len_b when len_a == 0 and len_a when len_b == 0.
 * Checks  pointers, 0 <= B <= 65535, elem_size, 1 <= G <= SWC_UNITS_MAX_GROUPS, the levels,
 *         0 <= max_frames <= SWC_UNITS_MAX_FRAMES.
 */
int swc_code_compare(const void* const* rows_a, const int64_t* ldg_a, const int64_t* n_a, const void* const* rows_b,
                     const int64_t* ldg_b, const int64_t* n_b, int32_t elem_size, const int32_t* levels_host4, int32_t G,
                     int32_t max_frames, int32_t dedup, int32_t* match, int32_t* both_valid, int32_t* level_match,
                     int32_t* level_l1, int32_t* frame_match, int32_t* bad, int32_t* edit, int32_t* len_a, int32_t* len_b,
                     int32_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_UNITS_H_ */
