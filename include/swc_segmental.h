/*
 * swc_segmental.h — C-ABI of the batched LPC-domain and segmental measures of libswc_hip.so: the log-likelihood ratio (LLR),
 * the Itakura-Saito distance (IS), the LPC cepstral distance (CD), the segmental SNR (SegSNR) and the frequency-weighted
 * segmental SNR (fwSegSNR) of a ragged batch of pairs in one call (Quackenbush, Barnwell and Clements 1988; Hu and Loizou
 * 2008).  A header of its own beside swc_spectral.h (same library, same conventions: device pointers, `stream` a hipStream_t
 * passed as void*, every call only enqueues, 0 on success or a negative SWC_E_* code with swc_last_error() giving the text;
 * nothing allocates or synchronises).
 *
 * The definition (normative; tests/segmental_ref.py restates it in float64 numpy from this text alone).  A pair is x (clean)
 * and y (degraded), each n = min(max(n_in[b], 0), max_n_in) f32 samples.  Parameters: the window W (a power of two, 64 ..
 * 2048), the LPC order P (1 .. 32), the number of bands K (0 .. 64).  "fl32" rounds to f32; everything else is float64, every
 * operation rounded on its own (no fused multiply-add whose result could differ: see Arithmetic).
 *
 *   frames       H = W / 4; T = 1 + floor((n - W) / H) for n >= W, else 0.  Frame t covers samples t H .. t H + W - 1: only
 *                whole frames are used, nothing outside [0, n) is read.  w[i] = 0.5 - 0.5 cos(2 pi i / W), evaluated in float64
 *                and rounded to f32 once.  v_x[i] = fl32(w[i] x[t H + i]), v_y likewise (the product frame_magnitudes forms).
 *   sums         every sum over the samples of a frame, sum_{i=0}^{L-1} term(i), is formed in four parts: with Q = W / 4, part c
 *                adds the terms i = c Q .. min((c + 1) Q, L) - 1 in ascending i from 0.0 (an empty part is 0.0), and the sum
 *                is ((part 0 + part 1) + part 2) + part 3.
 *   autocorr.    R_s[k] = sum_{i=0}^{W-1-k} v_s[i] v_s[i + k], k = 0 .. P, s in {x, y} (each product of two f32 is exact in
 *                float64).  S = R_x[0], D = sum_{i=0}^{W-1} (v_x[i] - v_y[i])^2 (the difference is exact in float64).  Then
 *                R_s[0] is multiplied by (1 + 2^-20): the white-noise correction that keeps Levinson conditioned on tonal frames.
 *   LPC frame    iff R_x[0] > 0 and R_y[0] > 0: a test on exact zero (a NaN fails it): digital silence on either side leaves
 *                the frame out of the three LPC measures.  It is counted, not guessed.  T_lpc = the number of LPC frames.
 *   Levinson     a = (1, a_1 .. a_P) from R:  E = R[0]; for m = 1 .. P:
 *                  acc = R[m]; for i = 1 .. m - 1 ascending: acc = acc + a_i R[m - i]
 *                  k_m = -acc / E
 *                  for i = 1 .. m - 1: a'_i = a_i + k_m a_{m-i}; then a_i = a'_i for those i, and a_m = k_m
 *                  E = E (1 - k_m k_m)
 *   forms        q(a, R): s_i = sum_{j=0}^{P} R[|i - j|] a_j (j ascending from 0.0), q = sum_{i=0}^{P} a_i s_i (i ascending
 *                from 0.0).  num = q(a_y, R_x), den = q(a_x, R_x), g_y = q(a_y, R_y).  den is a quadratic form, NOT Levinson's
 *                E (the two differ in the last digits): identical rows give num == den bit for bit.
 *   clamps       lo(v, c) = (v < c) ? c : v and hi(v, c) = (v > c) ? c : v: a NaN stays a NaN.
 *   llr_t        hi(lo(ln(num / den), 0), 2)
 *   is_t         hi((den / g_y) (num / den) + ln(g_y / den) - 1, 100)
 *   cd_t         cepstrum of the predictor p_k = -a_k: c[m] = p_m + sum_{k=1}^{m-1} ((k / m) c[k]) p_{m-k}, m = 1 .. P (k
 *                ascending, the sum started at p_m);  cd_t = hi(4.342944819032518 sqrt(2 sum_{m=1}^{P} (c_x[m] - c_y[m])^2), 10)
 *                (the constant is 10 / ln 10; m ascending from 0.0).
 *   seg_t        -10 if S == 0; else 35 if D == 0; else hi(lo(10 log10(S / D), -10), 35).  Every frame counts.
 *   fw_t         (K > 0 and a band table)  X[f], Y[f] = the f32 magnitudes frame_magnitudes<W, 2> gives for the frame
 *                (csrc/swc_frame_fft.h: an f32 FFT of v_x and v_y).  Ex[j], Ey[j] = the mel_band sums (f32, one fmaf per bin,
 *                ascending f) of band j over the packed table, in the format of swc_spectral.h: fb_first, fb_count, fb_off,
 *                fb_w, fb_w_len, with the same cuts into [0, F) and into the weight array.  Then in float64:
 *                  Emax = the largest Ex[j] (from 0.0: m = (Ex[j] > m or Ex[j] is NaN) ? Ex[j] : m, j ascending: a NaN stays)
 *                  u_j = (Ex[j] / Emax)^0.2;  d_j = Ex[j] - Ey[j]
 *                  s_j = -10 if Ex[j] == 0; else 35 if d_j == 0; else hi(lo(10 log10((Ex[j] Ex[j]) / (d_j d_j)), -10), 35)
 *                  fw_t = 35 - (sum_j u_j (35 - s_j)) / (sum_j u_j), both sums with j ascending from 0.0.
 *                A frame with Emax == 0 (every weight zero) is left out; T_fw counts the frames that remain.  The weights are
 *                Loizou's Ex^0.2 up to the common factor Emax^-0.2, which leaves fw_t unchanged as a real number and makes it
 *                invariant, bit for bit, under a scaling of both rows by a power of two; written from 35 down so that
 *                identical rows give exactly 35.
 *   row values   float64 vals[b][0 .. 7] = llr, is, cd, segsnr, fwsegsnr, T, T_lpc, T_fw.
 *                llr and cd: the mean of the K95 = (19 T_lpc + 10) / 20 (integer division) smallest values of the LPC frames,
 *                defined without a sort: v* = the K95-th smallest value; value = (the sum of the frame values < v*, added in
 *                frame order, + (K95 - their count) v*) / K95.  (Order and "<" are those of the float64 bit patterns, which for
 *                values >= 0 are those of the values.)  A NaN among the LPC frames' values makes the row's value NaN.
 *                is: the mean over the LPC frames, in frame order.  segsnr: the mean over the T frames, in frame order.
 *                fwsegsnr: the mean over the T_fw frames, in frame order.  A value whose frame count is 0 is NaN.
 *                NaN or Inf in a row reaches that row's values and no other row's.
 *                Identical rows give exactly llr 0, is 0, cd 0, segsnr 35 and fwsegsnr 35.
 *   track        optional, float64 [B][ld_t][5]: llr_t, is_t, cd_t, seg_t, fw_t of the first min(T, ld_t) frames, NaN where a
 *                frame was left out of a measure: where a reconstruction fails, and every stage per frame for the tests.
 *
 * Deviations from Loizou's scripts, on purpose: the window is a power of two (30 ms rounded up), not 30 ms; R[0] carries the
 * 2^-20 correction; and the spectra of fwSegSNR are NOT normalised to unit sum: a level error is an error for a codec
 * (metrics.level_matched removes it for callers who want that).
 *
 * Arithmetic: the translation unit is compiled without floating-point contraction, so every operation above rounds on its own,
 * as in numpy.  No float atomics; every sum has one fixed order that depends on the row alone.
 */
#ifndef SWC_SEGMENTAL_H_
#define SWC_SEGMENTAL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_SEGMENTAL_MIN_WIN 64
#define SWC_SEGMENTAL_MAX_WIN 2048
#define SWC_SEGMENTAL_MAX_ORDER 32   /* P */
#define SWC_SEGMENTAL_MAX_BANDS 64   /* K */
#define SWC_SEGMENTAL_VALUES 8       /* doubles per row of `vals` */
#define SWC_SEGMENTAL_MEASURES 5     /* doubles per frame of `track` */
/* vals[b] = */
#define SWC_SEGMENTAL_LLR 0
#define SWC_SEGMENTAL_IS 1
#define SWC_SEGMENTAL_CD 2
#define SWC_SEGMENTAL_SEGSNR 3
#define SWC_SEGMENTAL_FWSEGSNR 4
#define SWC_SEGMENTAL_FRAMES 5       /* T, T_lpc and T_fw: whole numbers, as doubles */
#define SWC_SEGMENTAL_FRAMES_LPC 6
#define SWC_SEGMENTAL_FRAMES_FW 7

/* Bytes of workspace swc_segmental needs for B rows of at most max_n_in samples:
 *   up256(B Tm (2 (P + 1) + 2) 8) + up256(B Tm 5 8)
 * with Tm = the frame count T of a row of max_n_in samples and up256(v) = v rounded up to a multiple of 256 (per frame the two
 * autocorrelations, D and fw_t; then the five frame values).  Plain host arithmetic; -1 for B outside 0..65535, max_n_in < 0, a
 * W, P or K the header refuses, or a frame count of 2^31 or more. */
int64_t swc_segmental_workspace_bytes(int32_t B, int64_t max_n_in, int32_t W, int32_t P, int32_t K);

/*
 * The five measures of a ragged batch of pairs (x_b clean, y_b degraded), each n_in[b] f32 samples.
 *
 * Rows    `x_rows`, `y_rows` and `n_in` are DEVICE arrays of B addresses, B addresses and B lengths.  A row needs 4-byte
 *         alignment only.  A row with n_in[b] <= 0 is empty and its addresses are not read.  max_n_in is the HOST's bound on
 *         the lengths (it sizes the launches and the workspace); a longer row is cut at max_n_in.
 * Bands   the K filters as a packed DEVICE table in the format of swc_spectral.h (fb_first[j] the first bin of filter j,
 *         fb_count[j] its number of bins, 0 for an empty filter, fb_off[j] where its weights start in fb_w, fb_w_len the
 *         length of fb_w).  The kernel cuts every filter's range into [0, W / 2 + 1) and into [0, fb_w_len): a bad table gives
 *         wrong numbers, never an access outside the spectrum or the weights.  With K == 0, or any of the four pointers null,
 *         no fwSegSNR work is done at all: fwsegsnr is NaN and T_fw is 0.
 * Outputs `vals`: float64 [B][8], every entry written.  `track`: float64 [B][ld_t][5] or null; the first min(T, ld_t) frames
 *         of a row are written and nothing else.  Nothing else is written outside the workspace.
 * Work    `workspace`: workspace_bytes >= swc_segmental_workspace_bytes(B, max_n_in, W, P, K) bytes of device memory, 256-byte
 *         aligned.  What it held before does not matter; what it holds afterwards is unspecified.
 * Bits    a row's values and track depend on its samples, W, P, K and the band table only: not on B, the row's index, the
 *         alignment of its addresses, max_n_in, the launch geometry or which outputs are asked for (with K == 0 the other
 *         four values are unchanged).
 * Checks  every argument is checked before anything is launched.
 * Limits  0 <= B <= 65535 (B == 0: nothing is launched); frame counts below 2^31.
 */
int swc_segmental(const void* const* x_rows, const void* const* y_rows, const int64_t* n_in, int64_t max_n_in, int32_t W, int32_t P,
                  int32_t K, const int32_t* fb_first, const int32_t* fb_count, const int32_t* fb_off, const float* fb_w,
                  int64_t fb_w_len, double* vals, double* track, int64_t ld_t, void* workspace, int64_t workspace_bytes, int32_t B,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_SEGMENTAL_H_ */
