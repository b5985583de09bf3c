/*
 * swc_pitch.h — C-ABI of the batched pitch measures of libswc_hip.so: the F0 track of every row of a ragged batch and, for
 * pairs, F0 RMSE in cents, gross pitch error, voicing decision error, V/UV F1 and F0 correlation in one call.  A header of
 * its own beside swc_spectral.h (same library, same conventions: device pointers, `stream` a hipStream_t passed as void*,
 * every call only enqueues, 0 on success or a negative SWC_E_* code with swc_last_error() giving the text; nothing
 * allocates or synchronises).
 *
 * The definition (normative; tests/pitch_ref.py restates it in numpy).  It is YIN (de Cheveigne and Kawahara 2002, steps
 * 1 - 5) restated so that every decision is exact integer arithmetic: the result does not depend on summation order, launch
 * geometry or signal level.
 *
 * Parameters of a call: the rate sr (Hz, an integer >= 1), the window W, the lags tau_min .. tau_max, the hop H, with
 *   2 <= tau_min < tau_max <= 1024,  16 <= W <= 2048,  W * tau_max <= 2^21,  H >= 1.
 *
 * For a row of n = min(max(n_in[b], 0), max_n_in) f32 samples x[0 .. n):
 *
 *   level    peak = max |x[i]|.
 *            peak == 0 (or n == 0): T as below, every frame is unvoiced.
 *            peak NaN or Inf: the row is "not defined": every f0 of its T frames is NaN, every tau is -1, and every pair
 *            value it enters is NaN (counts = T, 0, 0, 0).  No other row is touched.
 *            otherwise peak = m 2^e with m in [0.5, 1) (frexp) and
 *              q[i] = clamp(rint(x[i] 2^(15 - e)), -32767, 32767)        rint = round half to even
 *            The product is exact (a power of two).  The clamp is symmetric on purpose: |q| <= 32767 means a pair of
 *            products fits a signed 32-bit accumulator and (a - b)^2 < 2^32.
 *   frames   span = W + tau_max; T = 0 when n < span, else 1 + floor((n - span) / H).  Frame t reads q[t H .. t H + span).
 *            There is no padding.
 *   d        d(tau) = sum_{j < W} (q[t H + j] - q[t H + j + tau])^2, tau = 0 .. tau_max, in int64
 *            S(tau) = sum_{k = 1 .. tau} d(k)
 *            By the limits d tau < 2^53 and S < 2^53: both convert to double exactly.
 *   d'       d'(0) = 1; d'(tau) = 1 where S(tau) == 0; otherwise d'(tau) = double(d(tau) tau) / double(S(tau)): one IEEE
 *            division of two exactly converted integers.
 *   choice   c = the smallest tau in [tau_min, tau_max] with S(tau) > 0 and 20 d(tau) tau < 3 S(tau) (threshold 0.15,
 *            compared in int64).  None: the frame is unvoiced, tau = 0 and f0 = 0.  Otherwise, while c + 1 <= tau_max and
 *            d'(c + 1) < d'(c): c <- c + 1.
 *   refine   when c + 1 <= tau_max: a, b, g = d'(c - 1), d'(c), d'(c + 1) and den = (a - 2 b) + g; when den > 0:
 *            off = clamp((0.5 (a - g)) / den, -1, 1).  Otherwise (c == tau_max, or den <= 0) off = 0.
 *            f0 = sr / (c + off) in double, rounded to f32 once, at the store.  Every double operation is rounded on its
 *            own, in the order written (no contraction).  A voiced frame has tau = c >= tau_min and f0 > 0.
 *
 * For a pair (x clean, y degraded) of n samples each, from the STORED tracks (the f32 f0 widened to double; a frame is
 * voiced when its f0 > 0), so that the values are a pure function of what the call returns; T is common to both:
 *
 *   n_vx, n_vy, n_vv  frames voiced in x, in y, in both
 *   f0_rmse_cents     sqrt((1 / n_vv) sum (1200 log2(fy / fx))^2)              over the both-voiced frames
 *   gpe               the share of the both-voiced frames with |fy / fx - 1| > 0.2
 *   vde               the share of the T frames whose voiced flags differ
 *   vuv_f1            2 n_vv / (n_vx + n_vy)
 *   f0_corr           Pearson's r of (fx, fy) over the both-voiced frames, two-pass: the means first, then
 *                     sum (fx - mx)(fy - my) / sqrt(sum (fx - mx)^2 sum (fy - my)^2)
 *
 *   A value is NaN where its denominator is zero: T == 0 (vde and the two voiced shares), n_vv == 0 (rmse, gpe),
 *   n_vx + n_vy == 0 (vuv_f1), n_vv < 2 or a zero variance (f0_corr); n <= 0 gives T == 0.  Identical rows give exactly
 *   f0_rmse_cents = 0, gpe = 0, vde = 0 and (with a voiced frame) vuv_f1 = 1.
 *
 * Arithmetic of the pair values: double; lane l of 64 adds the frames t = l, l + 64, ... in ascending order, the 64 partial
 * sums are added in ascending lane order: one fixed order that depends on T alone.  No float atomics.  A value is rounded to
 * f32 once, at the store.  (The only atomic of the call is an unsigned integer maximum over |x|'s bit patterns: exact.)
 */
#ifndef SWC_PITCH_H_
#define SWC_PITCH_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_PITCH_MIN_TAU 2
#define SWC_PITCH_MAX_TAU 1024
#define SWC_PITCH_MIN_WIN 16
#define SWC_PITCH_MAX_WIN 2048
#define SWC_PITCH_MAX_WORK 2097152   /* W * tau_max <= 2^21 */
#define SWC_PITCH_THRESHOLD_NUM 3    /* 20 d tau < 3 S: threshold 0.15 */
#define SWC_PITCH_THRESHOLD_DEN 20
#define SWC_PITCH_FRAMES_PER_GROUP 4 /* frames (one wave each) per workgroup of the frame kernel */
#define SWC_PITCH_VALUES 8           /* floats per row of `values` */
#define SWC_PITCH_COUNTS 4           /* ints per row of `counts` */

/* Bytes of workspace swc_pitch needs for B rows of at most max_n_in samples, whatever outputs are asked for and with or
 * without y_rows:  up256(2 B 4) + up256(2 B T 4)  with  T = max_n_in < W + tau_max ? 0 : 1 + (max_n_in - W - tau_max) / H
 * and up256(v) = v rounded up to a multiple of 256 (the two rows' peaks as uint32, then their f32 f0 tracks).  Plain host
 * arithmetic; -1 for B outside 0..65535, max_n_in < 0, W, tau_max or H outside the limits above, or T >= 2^31. */
int64_t swc_pitch_workspace_bytes(int32_t B, int64_t max_n_in, int32_t W, int32_t tau_max, int32_t H);

/*
 * The F0 tracks of a ragged batch and, for pairs, the pitch measures.
 *
 * Rows    `x_rows`, `y_rows` and `n_in` are DEVICE arrays of B addresses, B addresses and B lengths.  A row needs 4-byte
 *         alignment only.  A row with n_in[b] <= 0 is empty and its addresses are not read.  max_n_in is the HOST's bound on
 *         the lengths (it sizes the launches and the workspace); a longer row is cut at max_n_in.  `y_rows` may be null:
 *         the call then tracks x only, and `values`, `tau_y` and `f0_y` must be null too.
 * Tracks  `tau_x`, `tau_y`: int32 [B][ldt]; `f0_x`, `f0_y`: f32 [B][ldt].  Each may be null.  ldt >= T(max_n_in) when one of
 *         them is not.  Entries t >= T of a row are NOT written.
 * Pairs   `values`: f32 [B][8] = f0_rmse_cents, f0_corr, gpe, vde, vuv_f1, n_vx / T, n_vy / T, 0.
 *         `counts`: int32 [B][4] = T, n_vx, n_vy, n_vv (without y_rows: T, n_vx, 0, 0).  Each may be null.
 * Work    `workspace`: workspace_bytes >= swc_pitch_workspace_bytes(B, max_n_in, W, tau_max, H) bytes of device memory,
 *         256-byte aligned.  What it held before does not matter; what it holds afterwards is unspecified.
 * Bits    a row's results depend on its samples and the parameters only: not on B, the row's index, the alignment of its
 *         address, max_n_in, ldt, the launch geometry or which outputs are asked for.
 * Checks  every argument is checked before anything is launched.
 * Limits  0 <= B <= 65535 (B == 0: nothing is launched); frame counts below 2^31; the parameter limits above.
 */
int swc_pitch(const void* const* x_rows, const void* const* y_rows, const int64_t* n_in, int64_t max_n_in, int32_t sr,
              int32_t W, int32_t tau_min, int32_t tau_max, int32_t H, int32_t* tau_x, float* f0_x, int32_t* tau_y, float* f0_y,
              int64_t ldt, float* values, int32_t* counts, void* workspace, int64_t workspace_bytes, int32_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_PITCH_H_ */
