/*
 * swc_loudness.h — C-ABI of the batched loudness measures of libswc_hip.so: integrated loudness, loudness range, the largest
 * momentary and short-term loudness, sample peak and true peak of every row of a ragged batch in one call (ITU-R BS.1770-4
 * gating, EBU Tech 3342 range), and the gain that brings a row to a target loudness under a true-peak ceiling, computed and
 * applied on the device.  A header of its own beside swc_align.h and swc_mcd.h (same library, same conventions: device
 * pointers, `stream` a hipStream_t passed as void*, every call only enqueues, 0 on success or a negative SWC_E_* code with
 * swc_last_error() giving the text; nothing allocates or synchronises).
 *
 * The definition (normative; tests/loudness_ref.py restates it in numpy).  Rows are mono f32.  One rate fs applies to a call,
 * 8000 <= fs <= 48000 and fs a multiple of 10 (so that a tenth of a second is a whole number of samples); any other fs is
 * refused.  A row has n = min(max(n_in[b], 0), max_n_in) samples x[0 .. n).
 *
 *   K-weighting  two biquads in cascade, y[i] = b0 x[i] + b1 x[i-1] + b2 x[i-2] - a1 y[i-1] - a2 y[i-2], derived from fs on the
 *                host in float64 (swc_loudness_coefficients returns them) and handed to the kernels as five numbers each:
 *                shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196
 *                           K = tan(pi f0 / fs), Vh = 10^(G / 20), Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2
 *                           b = [(Vh + Vb K / Q + K^2), 2 (K^2 - Vh), (Vh - Vb K / Q + K^2)] / a0
 *                           a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 *                high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773, the same K and a0 form
 *                           b = [1, -2, 1]
 *                           a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 *                At fs = 48000 these are the table of BS.1770 to 9e-16.  The filters run from sample 0 with zero initial
 *                state over the whole row, in float64.  (The high-pass pole radius is 0.9950 at 48 kHz: nothing is started
 *                "a little earlier from zero" anywhere; see Bits below.)
 *   energies     a sub-block is L = fs / 10 samples; S = floor(n / L); z_k = (sum of y[i]^2 over i in [k L, (k + 1) L)) / L for
 *                k < S, the squares added in ascending i, in float64.  A trailing partial sub-block is not used for loudness.
 *   momentary    N = max(S - 3, 0) blocks of 400 ms, one per sub-block hop: e_j = (((z_j + z_j+1) + z_j+2) + z_j+3) / 4,
 *                l_j = -0.691 + 10 log10(e_j).
 *   short-term   N3 = max(S - 29, 0) blocks of 3 s at the same hop: the 30 z added in ascending order, divided by 30,
 *                s_j = -0.691 + 10 log10(.).
 *   integrated   BS.1770-4 over the momentary blocks: A = {j : l_j > -70}; Gamma = -0.691 + 10 log10(mean of e_j over A) - 10;
 *                K = {j in A : l_j > Gamma}; I = -0.691 + 10 log10(mean of e_j over K).  NaN when K is empty.
 *   range        EBU Tech 3342 over the short-term values: A3 = {j : s_j > -70}; G3 = -0.691 + 10 log10(mean of the
 *                short-term energies over A3) - 20; K3 = {j in A3 : s_j > G3}; with the n3 values of K3 in ascending order v,
 *                LRA = v[floor(0.95 (n3 - 1) + 0.5)] - v[floor(0.10 (n3 - 1) + 0.5)].  NaN when K3 is empty.
 *   maxima       the largest l_j and the largest s_j (of all blocks, gated or not); NaN when there is no block (-inf for
 *                blocks of digital silence).
 *   sample peak  max |x[i]| over the whole row (linear; 0 for an empty row).
 *   true peak    the largest magnitude of what swc_resample (swc_audio.h) returns for the row from fs to 4 fs with the table
 *                the caller passes (the project's 4 x interpolator: 4 phases of `run` taps, wavio.resample_taps(1, 4) gives 15):
 *                output 4 f + p is ONE ascending fmaf chain over the run taps of phase p on x[f - width + tap_start[p] + k],
 *                zeros outside [0, n), in f32: the bits of swc_resample's output.  No 4 x copy of the row is written.  (This is
 *                not the FIR table of BS.1770 Annex 2.)  Both peaks are unsigned maxima over the bit patterns of |v|: a NaN
 *                wins.  A row with a NaN or Inf sample shows it there; its loudness values are then unspecified.
 *
 * Arithmetic: float64, every sum in one fixed order that depends on n and fs alone (a lane adds its blocks in ascending order,
 * the lanes' partial sums are added in ascending lane order).  The percentiles are chosen by exact radix selection on the bit
 * patterns of the short-term energies (64 counting passes), not by a sort: a row's length is not capped by on-chip memory.  The
 * only atomics are unsigned integer maxima and integer counts: exact in any order.
 *
 * swc_loudness_normalise: from a row's values as swc_loudness wrote them (device memory; nothing is read back),
 *   g = min(10^((target - I) / 20), 10^(ceiling / 20) / truepeak) in float64, rounded to f32 once; g = 1 where I is NaN or
 *   the true peak is 0 or not finite;  out[b][i] = x_b[i] * g, one f32 multiply.
 */
#ifndef SWC_LOUDNESS_H_
#define SWC_LOUDNESS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_LOUDNESS_MIN_FS 8000
#define SWC_LOUDNESS_MAX_FS 48000
#define SWC_LOUDNESS_MAX_N 1073741824 /* max_n_in <= 2^30 samples */
#define SWC_LOUDNESS_VALUES 8         /* doubles per row of `values` */
#define SWC_LOUDNESS_MAX_WIDTH 64     /* one-sided width of the true-peak interpolator, in input samples */
#define SWC_LOUDNESS_GROUP 64         /* sub-blocks (one lane each) per workgroup of the two filter passes */
#define SWC_LOUDNESS_UNMEASURED 1     /* flags bit 0: I is NaN or the true peak is 0 or not finite: the gain is 1 */
#define SWC_LOUDNESS_PEAK_LIMITED 2   /* flags bit 1: the true-peak ceiling, not the target, set the gain */
/* values[b] = integrated (LUFS), range (LU), largest momentary, largest short-term (LUFS), sample peak, true peak (linear),
 * momentary blocks N, blocks kept by both gates |K| (whole numbers, as doubles) */
#define SWC_LOUDNESS_I 0
#define SWC_LOUDNESS_LRA 1
#define SWC_LOUDNESS_MOMENTARY_MAX 2
#define SWC_LOUDNESS_SHORT_TERM_MAX 3
#define SWC_LOUDNESS_SAMPLE_PEAK 4
#define SWC_LOUDNESS_TRUE_PEAK 5
#define SWC_LOUDNESS_BLOCKS 6
#define SWC_LOUDNESS_BLOCKS_KEPT 7

/* The K-weighting of rate fs, plain host arithmetic in float64: k10 = shelf b0, b1, b2, a1, a2, high-pass b0, b1, b2, a1, a2.
 * 0, or -1 for an fs the header refuses (k10 is then not written). */
int swc_loudness_coefficients(int32_t fs, double* k10);

/* Bytes of workspace swc_loudness needs for B rows of at most max_n_in samples at rate fs:
 *   up256(2 B 4) + up256(B S 4 8) + up256(B S 8) + up256(B S 8)    with S = max_n_in / (fs / 10)
 * and up256(v) = v rounded up to a multiple of 256 (the two peaks of a row as uint32, the four-element filter state at the
 * start of every sub-block, the z_k, the short-term energies).  Plain host arithmetic; -1 for B outside 0..65535, max_n_in
 * outside 0..2^30 or an fs the header refuses. */
int64_t swc_loudness_workspace_bytes(int32_t B, int64_t max_n_in, int32_t fs);

/*
 * The eight loudness values of every row of a ragged batch.
 *
 * Rows    `x_rows` and `n_in` are DEVICE arrays of B addresses and B lengths.  A row needs 4-byte alignment only.  A row with
 *         n_in[b] <= 0 is empty and its address is not read.  max_n_in is the HOST's bound on the lengths (it sizes the
 *         launches and the workspace); a longer row is cut at max_n_in.
 * Table   `taps_packed` f32 [4][run] and `tap_start` int32 [4] (device), `width`, `run`: the packed 1 : 4 table of swc_resample
 *         (swc_audio.h), 1 <= run <= 2 width + 1, 0 <= width <= 64.  A tap_start outside 0 .. 2 width + 1 - run is clamped.
 * Output  `values`: float64 [B][8] as listed above; every entry of every row is written.
 * Work    `workspace`: workspace_bytes >= swc_loudness_workspace_bytes(B, max_n_in, fs) bytes of device memory, 256-byte
 *         aligned.  What it held before does not matter; what it holds afterwards is unspecified.
 * Bits    the segmentation is fixed by fs, not by the launch: a row's values depend on its samples, fs and the table only, not
 *         on B, the row's index, the alignment of its address, max_n_in or the launch geometry.
 * Checks  every argument is checked before anything is launched.
 * Limits  0 <= B <= 65535 (B == 0: nothing is launched); 0 <= max_n_in <= 2^30.
 */
int swc_loudness(const void* const* x_rows, const int64_t* n_in, int64_t max_n_in, int32_t fs, int32_t width,
                 const float* taps_packed, const int32_t* tap_start, int32_t run, double* values, void* workspace,
                 int64_t workspace_bytes, int32_t B, void* stream);

/*
 * Rows scaled to a target loudness under a true-peak ceiling, from the values of swc_loudness, without a read-back.
 *
 * Rows    as above, a row's length being max(n_in[b], 0) (the output's cols is the bound); `values` float64 [B][8] (device)
 *         as swc_loudness wrote them for the same rows.
 * Level   `target` in LUFS and `ceiling` in dB (true peak, relative to full scale): finite numbers.
 * Output  `out`: f32 [B][ld_out], the zero-padded batch contract of swc_resample: columns [0, cols) of every row are written
 *         (the row's min(n, cols) scaled samples, zeros behind them) and nothing else; cols <= ld_out.
 *         `gains`: f32 [B], `flags`: int32 [B] (SWC_LOUDNESS_UNMEASURED, SWC_LOUDNESS_PEAK_LIMITED).  Each of the three may be
 *         null, not all.
 * Checks  every argument is checked before anything is launched.  0 <= B <= 65535.
 */
int swc_loudness_normalise(const void* const* x_rows, const int64_t* n_in, const double* values, double target, double ceiling,
                           float* out, int64_t ld_out, int64_t cols, float* gains, int32_t* flags, int32_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_LOUDNESS_H_ */
