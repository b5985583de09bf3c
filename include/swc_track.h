/*
 * swc_track.h — C-ABI of the sub-sample lag track of libswc_hip.so: the lag of every segment of every (clean, degraded) pair of
 * a ragged batch to a fraction of a sample (swc_lag_track), one line lag(t) = a + b t per pair fitted to that track
 * (swc_lag_fit), and the degraded row resampled onto the clean row's clock along that line (swc_warp).  swc_align
 * (swc_align.h) finds a constant integer delay; this header starts from it (its `info` column 0 is the centre lag d0) and
 * covers what swc_align leaves out: a lag that is not an integer and, with two clocks, not constant.  A header of its own
 * beside swc_align.h (same library, same conventions: device pointers, `stream` a hipStream_t passed as void*, every call only
 * enqueues, 0 on success or a negative SWC_E_* code with swc_last_error() giving the text; nothing allocates or synchronises).
 *
 * The definition (normative; tests/track_ref.py restates it in numpy).
 *
 * 1. swc_lag_track.  Parameters: the segment length S and hop H in samples of x (S == 0: one segment, the whole row), the
 *    search half-range Rs (0 <= Rs <= 1024), the mode, and per pair the centre lag d0 (any int32).  W = 16, P = 32,
 *    R = Rs + W + 1.
 *
 *   rows      as in swc_align.h: x = x_rows[b] has nx = min(max(n_x[b], 0), max_nx) f32 samples, y has ny likewise; the
 *             two lengths are separate.
 *   level     exactly the level of swc_align.h, restated: per row v of n samples, peak = max |v[i]| = m 2^e with m in
 *             [0.5, 1) (frexp; e = 0 for peak == 0), q[i] = clamp(rint(v[i] 2^(15 - e)), -32767, 32767), rint = round half to
 *             even.  A NaN or Inf peak on either side makes the PAIR "not defined".
 *   sequence  exactly the sequence of swc_align.h, restated: SWC_ALIGN_WAVEFORM (0): s[i] = q[i].  SWC_ALIGN_ENVELOPE (1):
 *             s[i] = |q[i]| - mu, mu = floor(sum_i |q[i]| / n) in int64 over the WHOLE row.  Outside [0, n) s is 0.
 *   segments  a defined pair with nx > 0 and ny > 0 has K segments: K = 1 when S == 0 or nx <= S, else
 *             K = ceil((nx - S) / H) + 1.  Segment k covers the x indices [k H, min(k H + S, nx)) (S == 0: [0, nx)); the last
 *             one may be shorter than S.  An empty or not-defined pair has K = 0.
 *   corr.     c_k[d] = sum_i sx[i] sy[i + d0 + d] over the i of segment k with 0 <= i + d0 + d < ny, for d = -R .. R, in
 *             int64.  With n <= 2^22 every sum is below 2^52.
 *   peak      d* = the d with |d| <= Rs and the largest c_k[d] among those with c_k[d] > 0; ties go to the smaller |d|, then
 *             to d >= 0 (the rule of swc_align.h), all in int64.  No such d: the segment is "not defined".
 *   sub-      ct(j) = sum_{t = -W .. W} double(c_k[d* + t]) T[j][t] for j = -P/2 - 1 .. P/2 + 1, where T is the table passed in
 *   sample    (row j + P/2 + 1, column t + W; [P + 3][2 W + 1] doubles):
 *               T[j][t] = sinc(t - j / P) (0.5 + 0.5 cos(pi (t - j / P) / (W + 1))),   sinc(u) = sin(pi u) / (pi u), sinc(0) = 1
 *             built on the host in float64 (a device sin would not reproduce it).  Each ct(j) is ONE chain in ascending t from
 *             +0.0: acc = acc + double(c) T, the product rounded, then the sum rounded (no contraction).  j* = the interior
 *             j (|j| <= P/2) with the largest ct(j); ties go to the smaller |j|, then to j >= 0.  With ym = ct(j* - 1),
 *             y0 = ct(j*), yp = ct(j* + 1), each operation rounded once in the order written:
 *               num = ym - yp;  den = (ym - y0) + (yp - y0);  delta = den < 0 ? 0.5 * (num / den) : 0
 *               delta = min(max(delta, -0.5), 0.5)
 *               lag_k = double(d0 + d*) + (double(j*) + delta) / P
 *   values    lo = max(k H, -(d0 + d*)), hi = min(segment end, ny - (d0 + d*)): the i of the segment that face a y sample at
 *             the lag d0 + d*.  Sxx_k = sum sx[i]^2, Syy_k = sum sy[i + d0 + d*]^2 over lo <= i < hi in int64, and
 *               rho_k = double(c_k[d*]) / sqrt(double(Sxx_k) double(Syy_k))      (the product is > 0 when c_k[d*] > 0)
 *               weight_k = double(Sxx_k)
 *               t_k = double(lo + hi - 1) * 0.5       the mean index of the segment's valid x samples
 *   status    bit 0 (SWC_TRACK_DEFINED): the segment is defined.  Bit 1 (SWC_TRACK_EDGE): |d*| == Rs, the peak lies on the
 *             edge of the search range (with Rs == 0 every defined segment carries it).
 *   outputs   per pair and segment slot k < ldk: vals[4] = lag_k, rho_k, weight_k, t_k; status; and the whole c_k.  A slot
 *             that is not defined, or at or beyond the pair's K, gets NaN, NaN, 0, NaN, status 0 (its c_k is what the sums
 *             give: 0 at and beyond K).  nseg[b] = K.
 *
 *   The only atomics of the call: none.  A workgroup owns its (pair, segment, block of lags) and every intermediate word
 *   has one writer.  Everything up to rho and the interpolation is integer arithmetic.
 *
 * 2. swc_lag_fit.  Per pair, over its segments k = 0 .. K - 1 in ascending k, all in float64, each operation rounded once in
 *    the order written.  With l = lag, w = weight, t = centre:
 *      usable   U1 = { k : status_k has SWC_TRACK_DEFINED and rho_k >= rho_min }
 *      line(U)  sw = sum w;  tm = (sum w t) / sw;  lm = (sum w l) / sw;
 *               stt = sum w ((t - tm) (t - tm));  stl = sum w ((t - tm) (l - lm));
 *               drift: b = stl / stt, a = lm - b tm.   no drift: b = 0, a = lm.
 *               (every sum one chain in ascending k from +0.0; a term is (w * x) or w * (y), rounded, then added)
 *      passes   (a1, b1) = line(U1);  U2 = { k in U1 : |l_k - (a1 + b1 t_k)| <= 1 };  (a, b) = line(U2)
 *      residual rms = sqrt((sum_{U2} w (r r)) / sw) with r = l_k - (a + b t_k)
 *      counts   used = |U2| (|U1| when the first pass already raises flag 1 or 2: there is no second), offered = K
 *      flags    SWC_FIT_NO_DRIFT (1): a drift fit with fewer than 2 segments in U1 or U2, or stt == 0;  SWC_FIT_NO_LAG (2):
 *               no segment in U1 or U2;  SWC_FIT_EDGE (4): a segment of U2 carries SWC_TRACK_EDGE.
 *               A pair with flag 1 or 2 gets a = double(d0), b = 0, rms = NaN.
 *    Stated limit: the track follows a lag that stays within Rs samples of d0 over the row.  Beyond that the segments lose
 *    their peak (or find it on the edge); this is reported through the flags, not guessed.
 *
 * 3. swc_warp.  Per pair, from a, b (doubles at fit[b ld_fit + 0], [.. + 1]):
 *      A = rint(a 2^32), Q = rint((1 + b) 2^32) as int64 (rint of the rounded product; round half to even)
 *      the pair is "not warped" (x0 = m = 0, flag 1, the row all zeros) unless |a| <= 2^23 and |b| <= 0.01 (NaN fails both)
 *      pos(i) = A + i Q,  ip(i) = pos >> 32 (floor),  frac = pos & (2^32 - 1),  phase = frac >> 24,
 *      wt = float(frac & (2^24 - 1)) 2^-24   (exact)
 *      x0 = max(0, ceil(-A / Q)): the first i >= 0 with ip(i) >= 0;  last = floor((ny 2^32 - 1 - A) / Q): the last i with
 *      ip(i) <= ny - 1;  m = max(0, min(min(last + 1, nx) - x0, cols)).  All in int64; an empty row gives m = 0, and m == 0
 *      gives x0 = 0.
 *      h(t) = fmaf(wt, H[phase + 1][t] - H[phase][t], H[phase][t]) for t = -15 .. 16, H the f32 table passed in
 *      ([257][32], column t + 15): H[p][t] = float(sinc(t - p / 256) (0.5 + 0.5 cos(pi (t - p / 256) / 16))), from float64
 *      out[c] = sum_t h(t) y[ip(x0 + c) + t] for c < m: ONE f32 fmaf chain in ascending t from +0.0, y = 0 outside the row;
 *      out[c] = 0 for m <= c < cols.  The bits depend on the row, a, b and the table only (the contract of swc_resample).
 *      x[x0 .. x0 + m) faces out[0 .. m).
 */
#ifndef SWC_TRACK_H_
#define SWC_TRACK_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_TRACK_W 16                /* W: correlation values on either side of the integer peak that the interpolation reads */
#define SWC_TRACK_P 32                /* P: sub-sample positions per sample */
#define SWC_TRACK_TABLE_ROWS 35       /* P + 3 */
#define SWC_TRACK_TABLE_COLS 33       /* 2 W + 1 */
#define SWC_TRACK_MAX_RANGE 1024      /* Rs */
#define SWC_TRACK_MAX_N 4194304       /* max_nx, max_ny, cols <= 2^22 */
#define SWC_TRACK_MAX_SEGMENTS 4096   /* segments of the longest row: swc_track_segments(max_nx, S, H) */
#define SWC_TRACK_CHUNK 4096          /* samples of x a workgroup of the correlation kernel stages at a time */
#define SWC_TRACK_LAG_BLOCK 256       /* lags a workgroup of the correlation kernel takes */
#define SWC_TRACK_SPILL 256           /* samples of x an int32 accumulator takes between two spills into int64 */
#define SWC_TRACK_VALUES 4            /* doubles per segment slot of `vals` */
#define SWC_TRACK_DEFINED 1
#define SWC_TRACK_EDGE 2
#define SWC_FIT_VALUES 4              /* doubles per row of `fit`: a, b, rms, 0 */
#define SWC_FIT_COUNTS 4              /* ints per row of `counts`: used, offered, flags, 0 */
#define SWC_FIT_NO_DRIFT 1
#define SWC_FIT_NO_LAG 2
#define SWC_FIT_EDGE 4
#define SWC_WARP_TAPS 32              /* t = -15 .. 16 */
#define SWC_WARP_PHASES 256           /* the table has SWC_WARP_PHASES + 1 rows */
#define SWC_WARP_BLOCK 256            /* outputs per workgroup */
#define SWC_WARP_INFO 4               /* ints per row of `info`: x0, m, flag (1: not warped), 0 */
#define SWC_WARP_MAX_DRIFT 0.01       /* |b| */
#define SWC_WARP_MAX_LAG 8388608      /* |a| <= 2^23 */

/* K of the header for a row of n samples: 0 for n <= 0, 1 when S == 0 or n <= S, else ceil((n - S) / H) + 1.
 * Plain host arithmetic; -1 for n > 2^22, S < 0, or S > 0 with H < 1. */
int64_t swc_track_segments(int64_t n, int32_t S, int32_t H);

/* Bytes of workspace swc_lag_track needs, whatever outputs are asked for and in either mode:
 *   up256(2 B 4) + up256(2 B 8) + up256(B K (2 R + 1) 8),   K = swc_track_segments(max_nx, S, H), R = Rs + 17
 * with up256(v) = v rounded up to a multiple of 256 (the rows' peaks as uint32, their sums of |q| as int64, every c_k[d] as
 * int64).  Plain host arithmetic; -1 for B outside 0..65535, max_nx or max_ny outside 0..2^22, Rs outside 0..1024, S or H out
 * of range, or K > SWC_TRACK_MAX_SEGMENTS. */
int64_t swc_lag_track_workspace_bytes(int32_t B, int64_t max_nx, int64_t max_ny, int32_t S, int32_t H, int32_t Rs);

/*
 * The lag of every segment of every pair of a ragged batch.
 *
 * Rows    `x_rows`, `y_rows`, `n_x`, `n_y`, max_nx, max_ny: as in swc_align.  `d0`: DEVICE int32, pair b's centre lag at
 *         d0[b ld_d0] (ld_d0 >= 1; column 0 of swc_align's `info` with ld_d0 = 4).
 * Table   `table`: DEVICE f64 [35][33], the T of the definition.
 * Outputs `vals`: f64 [B][ldk][4]; `status`: int32 [B][ldk]; `nseg`: int32 [B]; `xc`: int64 [B][ldk][ldc], c_k[d] at column
 *         d + R, ldc >= 2 R + 1.  Each may be null.  ldk >= K = swc_track_segments(max_nx, S, H); slots at and beyond K and
 *         columns at and beyond 2 R + 1 are NOT written.
 * Work    `workspace`: workspace_bytes >= swc_lag_track_workspace_bytes(...) bytes of device memory, 256-byte aligned.  What
 *         it held before does not matter; what it holds afterwards is unspecified.
 * Bits    a pair's results depend on its samples, d0, S, H, Rs, the mode and the table only: not on B, the pair's index, the
 *         alignment of its addresses, max_nx, max_ny, ld_d0, ldk, ldc, the launch geometry or which outputs are asked for.
 * Checks  every argument is checked before anything is launched.
 * Limits  0 <= B <= 65535 (B == 0: nothing is launched); 0 <= max_nx, max_ny <= 2^22; 0 <= Rs <= 1024; S >= 0, H >= 1 when
 *         S > 0; K <= SWC_TRACK_MAX_SEGMENTS.
 */
int swc_lag_track(const void* const* x_rows, const void* const* y_rows, const int64_t* n_x, const int64_t* n_y, int64_t max_nx,
                  int64_t max_ny, const int32_t* d0, int64_t ld_d0, int32_t S, int32_t H, int32_t Rs, int32_t mode,
                  const double* table, double* vals, int32_t* status, int64_t ldk, int32_t* nseg, int64_t* xc, int64_t ldc,
                  void* workspace, int64_t workspace_bytes, int32_t B, void* stream);

/*
 * One line per pair through its track (definition 2).  `vals`, `status`, `nseg`, ldk: what swc_lag_track wrote; pair b reads
 * min(max(nseg[b], 0), kmax) segments, 0 <= kmax <= ldk, kmax <= SWC_TRACK_MAX_SEGMENTS.  `d0`, ld_d0 as above.  rho_min in
 * [-1, 1]; drift 0 or 1.  `fit`: f64 [B][4] = a, b, rms, 0.  `counts`: int32 [B][4] = used, offered, flags, 0; may be null.
 * One thread per pair, fixed order: the bits depend on the pair's track and the parameters only.  0 <= B <= 65535.
 */
int swc_lag_fit(const double* vals, const int32_t* status, int64_t ldk, const int32_t* nseg, int32_t kmax, const int32_t* d0,
                int64_t ld_d0, double rho_min, int32_t drift, double* fit, int32_t* counts, int32_t B, void* stream);

/*
 * The degraded rows on the clean rows' clock (definition 3).  `fit`: DEVICE f64, pair b's a and b at fit[b ld_fit] and
 * fit[b ld_fit + 1] (ld_fit >= 2; swc_lag_fit's output with ld_fit = 4).  `table`: DEVICE f32 [257][32].  `out`: f32
 * [B][ld_out], ld_out >= cols; columns [0, cols) of every row are written, nothing beyond.  `info`: int32 [B][4] = x0, m, flag,
 * 0; may be null.  0 <= B <= 65535, 0 <= max_nx, max_ny, cols <= 2^22.  No workspace.
 */
int swc_warp(const void* const* y_rows, const int64_t* n_x, const int64_t* n_y, int64_t max_nx, int64_t max_ny, const double* fit,
             int64_t ld_fit, const float* table, float* out, int64_t ld_out, int64_t cols, int32_t* info, int32_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_TRACK_H_ */
