/*
 * swc_activity.h — C-ABI of the batched speech activity measures of libswc_hip.so: the ITU-T P.56 active speech level, the
 * long-term level, the activity factor and the sample peak of every row of a ragged batch in one call, the runs of active
 * samples the P.56 criterion defines (a deterministic activity detector), and the gain that brings a row to a target active
 * level, computed and applied on the device.  A header of its own beside swc_loudness.h (same library, same conventions:
 * device pointers, `stream` a hipStream_t passed as void*, every call only enqueues, 0 on success or a negative SWC_E_* code
 * with swc_last_error() giving the text; nothing allocates or synchronises).
 *
 * The definition (normative; tests/activity_ref.py restates it in numpy from this text alone).  It is ITU-T P.56 method B as
 * restated here.  Where the ITU's own program reaches the level by bisection to a tolerance, this text uses the closed form of
 * the same linear interpolation between two thresholds.
 *
 *   input        rows are mono f32, full scale 1.0.  A row has n = min(max(n_in[b], 0), max_n_in) >= 0 samples x[0 .. n).  One
 *                integer rate fs applies to a call, 8000 <= fs <= 48000 (any integer: no multiple-of-10 rule).
 *   constants    T = 0.03 s, g = exp(-1 / (fs T)); the hangover I = floor(hangover_s fs + 0.5) samples (hangover_s = 0.2 in
 *                P.56; 0 <= I <= 24000 here); the margin M = margin_db (15.9 dB in P.56; 0 < M <= 100 here).
 *   envelope     p_i = g p_{i-1} + (1 - g) |x_i|,  q_i = g q_{i-1} + (1 - g) p_i,  p_{-1} = q_{-1} = 0: the state is zero before
 *                sample 0, and the recursion runs in float64 over the whole row.  (The pole is 0.9979 at 16 kHz: thousands of
 *                samples of memory; nothing is started "a little earlier from zero" anywhere; see Bits below.)
 *   activity     at a threshold c: last(i) = the largest i' <= i with q_{i'} >= c (minus infinity when there is none); sample i
 *                is active iff i - last(i) <= I; a(c) = the count of active samples.
 *   levels       sq = the sum of x_i^2 in float64; the long-term level L = 10 log10(sq / n).  The thresholds are
 *                c_j = 2^(j - 15), j = 0 .. 14, with a_j = a(c_j), A_j = 10 log10(sq / a_j), C_j = 20 log10(c_j) and
 *                D_j = A_j - C_j.  Walk j upward.  At the first j with a_j = 0 the active level is undefined.  At the first j
 *                with D_j <= M the active level is A = A_j when j = 0 or D_j = M, and otherwise
 *                A = A_{j-1} + t (A_j - A_{j-1}) with t = (D_{j-1} - M) / (D_{j-1} - D_j).  When no j of 0 .. 14 has D_j <= M
 *                the active level is undefined as well.
 *                The activity factor is 10^((L - A) / 10); the working threshold is c* = 10^((A - M) / 20).
 *   runs         the maximal intervals [s, e) of samples active at c*, in ascending order.  A run and the gap behind it span at
 *                least I + 2 samples, so a row has at most n / (I + 2) + 1 runs: the capacity of the run list is derived from
 *                that bound (ld_runs below) and cannot overflow.
 *   values       per row, float64: the active level A (dB relative to full scale), the long-term level L (dB), the activity
 *                factor, c* (linear), the sample peak max |x_i| (linear; an unsigned maximum over the bit patterns: a NaN
 *                wins), the count of samples active at c*, the count of runs, and the index j of the crossing (for tests).
 *                A, L, the factor, c* and j are NaN where undefined: n = 0, sq = 0, or no crossing.  Such a row has no run
 *                and no active sample.  The fifteen counts a_j come back as int64 as well.
 *
 * Arithmetic: float64.  The row is cut into sub-blocks of SWC_ACTIVITY_SUBBLOCK samples and tiles of SWC_ACTIVITY_TILE
 * samples, both constants; a sub-block's squares are added in ascending i, the sub-blocks' sums by SWC_ACTIVITY_THREADS lanes
 * (lane t adds sub-blocks t, t + 256, ... in ascending order, the lanes' sums are added in ascending lane order).  Counts are
 * integers.  There is no atomic anywhere.
 *
 * swc_activity_normalise: from a row's values as swc_activity wrote them (device memory; nothing is read back),
 *   gain = min(10^((target_db - A) / 20), 1 / peak) in float64, rounded to f32 once; gain = 1 where A is NaN or the peak is 0
 *   or not finite;  out[b][i] = x_b[i] * gain, one f32 multiply.
 */
#ifndef SWC_ACTIVITY_H_
#define SWC_ACTIVITY_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_ACTIVITY_MIN_FS 8000
#define SWC_ACTIVITY_MAX_FS 48000
#define SWC_ACTIVITY_MAX_N 1073741824   /* max_n_in <= 2^30 samples */
#define SWC_ACTIVITY_MAX_HANGOVER 24000 /* I <= 24000 samples (0.5 s at 48 kHz) */
#define SWC_ACTIVITY_SUBBLOCK 256       /* samples per sub-block (one lane each) of the filter passes */
#define SWC_ACTIVITY_GROUP 64           /* sub-blocks per workgroup of the filter passes and per step of the carry */
#define SWC_ACTIVITY_TILE 4096          /* samples per workgroup of the sliding-window passes */
#define SWC_ACTIVITY_THREADS 256        /* lanes of the sliding-window and level kernels */
#define SWC_ACTIVITY_THRESHOLDS 15      /* c_j = 2^(j - 15), j = 0 .. 14: int64 per row of `counts` */
#define SWC_ACTIVITY_VALUES 8           /* doubles per row of `values` */
#define SWC_ACTIVITY_UNMEASURED 1       /* flags bit 0: A is NaN or the peak is 0 or not finite: the gain is 1 */
#define SWC_ACTIVITY_PEAK_LIMITED 2     /* flags bit 1: 1 / peak, not the target, set the gain */
/* values[b] = active level (dB), long-term level (dB), activity factor, c* (linear), sample peak (linear), samples active at
 * c*, runs (whole numbers, as doubles), the crossing's j (a whole number, or NaN) */
#define SWC_ACTIVITY_ACTIVE_LEVEL 0
#define SWC_ACTIVITY_LONG_TERM 1
#define SWC_ACTIVITY_FACTOR 2
#define SWC_ACTIVITY_THRESHOLD 3
#define SWC_ACTIVITY_SAMPLE_PEAK 4
#define SWC_ACTIVITY_ACTIVE_SAMPLES 5
#define SWC_ACTIVITY_RUNS 6
#define SWC_ACTIVITY_CROSSING 7

/* The constants of a rate, plain host arithmetic in float64: *g = exp(-1 / (0.03 fs)), *hangover = I, *subblock = the
 * sub-block length (SWC_ACTIVITY_SUBBLOCK), m4 = the 2 x 2 transition of the state (p, q) over one sub-block of silence,
 * row-major, built by running the recursion on the two unit states.  0, or -1 for an fs or a hangover_s the header refuses or a
 * null pointer (nothing is written then). */
int swc_activity_coefficients(int32_t fs, double hangover_s, double* g, int32_t* hangover, int32_t* subblock, double* m4);

/* Bytes of workspace swc_activity needs for B rows of at most max_n_in samples:
 *   up256(B S 2 8) + up256(B S 8) + up256(B S 4) + up256(B up256(max_n_in)) + up256(B NT 16 4) + up256(B NT 4 4)
 * with S = ceil(max_n_in / 256), NT = ceil(max_n_in / 4096) and up256(v) = v rounded up to a multiple of 256 (the state at the
 * start of every sub-block, its sum of squares, its peak, one byte per sample, the fifteen counts and the run counts of every
 * tile).  Plain host arithmetic; -1 for B outside 0..65535, max_n_in outside 0..2^30 or an fs the header refuses. */
int64_t swc_activity_workspace_bytes(int32_t B, int64_t max_n_in, int32_t fs);

/*
 * The values, the fifteen counts and the runs of every row of a ragged batch.
 *
 * Rows    `x_rows` and `n_in` are DEVICE arrays of B addresses and B lengths.  A row needs 4-byte alignment only.  A row with
 *         n_in[b] <= 0 is empty and its address is not read.  max_n_in is the HOST's bound on the lengths (it sizes the
 *         launches and the workspace); a longer row is cut at max_n_in.
 * Output  `values`: float64 [B][8] as listed above; `counts`: int64 [B][15], the a_j; every entry of every row is written.
 *         `runs`: int64 [B][ld_runs][2], run r of row b as (s, e); the first values[b][6] entries of a row are written and
 *         nothing else.  ld_runs >= max_n_in / (I + 2) + 1.
 * Work    `workspace`: workspace_bytes >= swc_activity_workspace_bytes(B, max_n_in, fs) bytes of device memory, 256-byte
 *         aligned.  What it held before does not matter; what it holds afterwards is unspecified.
 * Bits    the segmentation is fixed by the constants above, not by the launch: a row's values, counts and runs depend on its
 *         samples, fs, margin_db and hangover_s only, not on B, the row's index, the alignment of its address, max_n_in or the
 *         launch geometry.
 * Checks  every argument is checked before anything is launched.
 * Limits  0 <= B <= 65535 (B == 0: nothing is launched); 0 <= max_n_in <= 2^30.
 */
int swc_activity(const void* const* x_rows, const int64_t* n_in, int64_t max_n_in, int32_t fs, double margin_db, double hangover_s,
                 double* values, int64_t* counts, int64_t* runs, int64_t ld_runs, void* workspace, int64_t workspace_bytes,
                 int32_t B, void* stream);

/*
 * Rows scaled to a target active level without clipping, from the values of swc_activity, without a read-back.
 *
 * Rows    as above, a row's length being max(n_in[b], 0) (the output's cols is the bound); `values` float64 [B][8] (device)
 *         as swc_activity wrote them for the same rows.
 * Level   `target_db` in dB relative to full scale (dBov; -26 before P.862 / P.863 / P.808 tests): a finite number.
 * Output  `out`: f32 [B][ld_out], the zero-padded batch contract of swc_resample: columns [0, cols) of every row are written
 *         (the row's min(n, cols) scaled samples, zeros behind them) and nothing else; cols <= ld_out.
 *         `gains`: f32 [B], `flags`: int32 [B] (SWC_ACTIVITY_UNMEASURED, SWC_ACTIVITY_PEAK_LIMITED).  Each of the three may be
 *         null, not all: the conventions of swc_loudness_normalise.
 * Checks  every argument is checked before anything is launched.  0 <= B <= 65535.
 */
int swc_activity_normalise(const void* const* x_rows, const int64_t* n_in, const double* values, double target_db, float* out,
                           int64_t ld_out, int64_t cols, float* gains, int32_t* flags, int32_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_ACTIVITY_H_ */
