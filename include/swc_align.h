/*
 * swc_align.h — C-ABI of the batched time alignment of libswc_hip.so: the constant delay (an integer lag), the correlation at
 * that lag and the level ratio of every (clean, degraded) pair of a ragged batch in one call, so that the pair can be handed to
 * swc_stoi / swc_quality / swc_spectral / swc_pitch as two offset views of the same memory.  A header of its own beside
 * swc_pitch.h (same library, same conventions: device pointers, `stream` a hipStream_t passed as void*, every call only
 * enqueues, 0 on success or a negative SWC_E_* code with swc_last_error() giving the text; nothing allocates or synchronises).
 *
 * The definition (normative; tests/align_ref.py restates it in numpy).  Every decision is exact integer arithmetic: the result
 * does not depend on summation order, launch geometry or signal level.
 *
 * Parameters of a call: the search range L (lags -L .. L, 0 <= L <= 32768) and the mode (SWC_ALIGN_WAVEFORM or _ENVELOPE).
 *
 * For pair b, x = x_rows[b] (clean) has nx = min(max(n_x[b], 0), max_nx) f32 samples and y = y_rows[b] (degraded) has
 * ny = min(max(n_y[b], 0), max_ny); the two lengths are separate and the rows are NOT cut to the shorter one.
 *
 *   level     per row v of n samples, on its own (the words of swc_pitch.h): peak = max |v[i]|; peak = m 2^e with m in [0.5, 1)
 *             (frexp; e = 0 for peak == 0) and
 *               q[i] = clamp(rint(v[i] 2^(15 - e)), -32767, 32767)        rint = round half to even
 *             The product is exact (a power of two).  The clamp is symmetric on purpose: |q| <= 32767 means a pair of
 *             products fits a signed 32-bit accumulator.  A NaN or Inf peak on either side makes the PAIR "not defined".
 *   sequence  SWC_ALIGN_WAVEFORM: s[i] = q[i].
 *             SWC_ALIGN_ENVELOPE: s[i] = |q[i]| - mu with mu = floor(sum_i |q[i]| / n) in int64: the rectified signal at full
 *             rate with its integer mean removed (|s| <= 32767 still).
 *             Outside [0, n) a sequence is 0 in both modes (not -mu).
 *   corr.     c[d] = sum_i sx[i] sy[i + d] over the i with 0 <= i < nx and 0 <= i + d < ny, for d = -L .. L, in int64.
 *             d > 0 means y is delayed by d samples.  With n <= 2^22 every sum is below 2^22 2^30 = 2^52 < 2^53.
 *   choice    d* = the d with the largest c[d] among those with c[d] > 0; ties go to the smaller |d|, then to d >= 0; all
 *             comparisons in int64.  If no c[d] > 0 then d* = 0.
 *   overlap   x0 = max(0, -d*), y0 = max(0, d*), m = max(0, min(nx - x0, ny - y0)): x[x0 .. x0 + m) faces y[y0 .. y0 + m).
 *   values    over the overlap (i = 0 .. m - 1 of x0 + i, y0 + i), in int64 and then double, each operation rounded once in
 *             the order written (no contraction):
 *               Sxx = sum sx^2, Syy = sum sy^2, Exx = sum qx^2, Eyy = sum qy^2
 *               corr = double(c[d*]) / sqrt(double(Sxx) double(Syy))                 NaN when the product is 0
 *               gain = ldexp(sqrt(double(Exx) / double(Eyy)), ex - ey)               NaN when Eyy == 0
 *             gain is the factor that brings y to x's level.  Each value is rounded to f32 once, at the store.
 *   empty     an empty pair (nx <= 0 or ny <= 0) or a not-defined pair gives info = 0, 0, 0, 0, values = NaN, NaN, 0, 0 and
 *             c[d] = 0 for every d.  The addresses of an empty pair are not read.  No other row is touched.
 *
 * The only atomics of the call are an unsigned integer maximum over |v|'s bit patterns and int64 integer additions: exact in
 * any order.  No float atomics.
 */
#ifndef SWC_ALIGN_H_
#define SWC_ALIGN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_ALIGN_WAVEFORM 0
#define SWC_ALIGN_ENVELOPE 1
#define SWC_ALIGN_MAX_LAG 32768     /* L */
#define SWC_ALIGN_MAX_N 4194304     /* max_nx, max_ny <= 2^22 */
#define SWC_ALIGN_CHUNK 4096        /* samples of x a workgroup of the correlation kernel takes */
#define SWC_ALIGN_LAG_BLOCK 256     /* lags a workgroup of the correlation kernel takes */
#define SWC_ALIGN_SPILL 256         /* samples of x (128 pairs) an int32 accumulator takes between two spills into int64 */
#define SWC_ALIGN_INFO 4            /* ints per row of `info` */
#define SWC_ALIGN_VALUES 4          /* floats per row of `values` */

/* Bytes of workspace swc_align needs, whatever outputs are asked for and in either mode:
 *   up256(2 B 4) + up256(2 B 8) + up256(8 B 8) + up256(B (2 L + 1) 8)
 * with up256(v) = v rounded up to a multiple of 256 (the rows' peaks as uint32, their sum |q| as int64, eight int64 words per
 * pair for the energies and d*, every c[d] as int64).
 * Plain host arithmetic; -1 for B outside 0..65535, max_nx or max_ny outside 0..2^22, L outside 0..32768. */
int64_t swc_align_workspace_bytes(int32_t B, int64_t max_nx, int64_t max_ny, int32_t L);

/*
 * The lag, the overlap, the correlation and the level ratio of every pair of a ragged batch.
 *
 * Rows    `x_rows`, `y_rows`, `n_x` and `n_y` are DEVICE arrays of B addresses, B addresses, B lengths and B lengths.  A row
 *         needs 4-byte alignment only.  max_nx and max_ny are the HOST's bounds on the lengths (they size the launches); a
 *         longer row is cut there.
 * Outputs `info`: int32 [B][4] = d*, x0, y0, m.  `values`: f32 [B][4] = corr, gain, 0, 0.  `xc`: int64 [B][ldc], the whole
 *         c[-L .. L] of every row (c[d] at column d + L), ldc >= 2 L + 1; entries at and beyond 2 L + 1 are NOT written.
 *         Each may be null.
 * Work    `workspace`: workspace_bytes >= swc_align_workspace_bytes(B, max_nx, max_ny, L) bytes of device memory, 256-byte
 *         aligned.  What it held before does not matter (the call initialises whatever it accumulates into); what it holds
 *         afterwards is unspecified.
 * Bits    a pair's results depend on its samples, L and the mode only: not on B, the pair's index, the alignment of its
 *         addresses, max_nx, max_ny, ldc, the launch geometry or which outputs are asked for.
 * Checks  every argument is checked before anything is launched.
 * Limits  0 <= B <= 65535 (B == 0: nothing is launched); 0 <= max_nx, max_ny <= 2^22; 0 <= L <= 32768.
 */
int swc_align(const void* const* x_rows, const void* const* y_rows, const int64_t* n_x, const int64_t* n_y, int64_t max_nx,
              int64_t max_ny, int32_t L, int32_t mode, int32_t* info, float* values, int64_t* xc, int64_t ldc, void* workspace,
              int64_t workspace_bytes, int32_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_ALIGN_H_ */
