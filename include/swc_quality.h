/*
 * swc_quality.h — C-ABI of the batched quality call of libswc_hip.so: STOI, ESTOI and SI-SDR of a ragged batch of pairs in
 * one call.  A header of its own beside swc_metrics.h (same library, same conventions: device pointers, `stream` a
 * hipStream_t passed as void*, every call only enqueues, 0 on success or a negative SWC_E_* code with swc_last_error()
 * giving the text; nothing allocates or synchronises).  swc_metrics.h keeps declaring swc_stoi alone.
 *
 * STOI   exactly the algorithm of swc_metrics.h (its steps 1 - 5), from the same kernels: stoi[b] and segs[b] equal
 *        swc_stoi's bit for bit.
 *
 * ESTOI  extended STOI (Jensen, Taal 2016; `pystoi` with extended=True).  The constants and the steps 1, 2, 3 and 5 are those of
 *        swc_metrics.h: the same 10 kHz signals, the same kept frames src[0..K), the same band spectra Xt, Yt [15][M],
 *        M = K - 1, S = M - 29, and estoi = 1e-5 with segs = 0 when M < 30 (also n_in <= 0, K <= 1).  Step 4 becomes, for
 *        each segment m = 30..M with A = Xt[:, m-30:m] and Bm = Yt[:, m-30:m] (15 bands x 30 frames each):
 *          4a. from every band row (30 values) subtract its mean over the 30 frames, then divide it by (its norm + EPS)
 *          4b. from every frame column (15 values) of the result subtract its mean over the 15 bands, then divide it by
 *              (its norm + EPS)
 *          4c. e_m = (1 / 30) sum over all 450 elements of A * Bm
 *          4d. estoi = sum over m of e_m / S
 *        No clipping and no rescaling of Bm.  EPS = 2^-52.  pystoi adds EPS * randn to the matrices before each of 4a and
 *        4b and divides by the plain norm; the deterministic `norm + EPS` form above is the contract here (the two differ
 *        by ~1e-15 on anything but an all-constant row or column).
 *
 * SI-SDR scale-invariant signal-to-distortion ratio (Le Roux, Wisdom, Erdogan, Hershey 2019), in dB, of the rows AS GIVEN: at
 *        the input rate, all n = min(max(n_in[b], 0), max_n_in) samples, no resampling, no frame removal.
 *          1. mx, my the means of x and y; x' = x - mx, y' = y - my
 *          2. alpha = sum x' y' / (sum x' x' + EPS)
 *          3. Et = sum (alpha x')^2, En = sum (y' - alpha x')^2
 *          4. si_sdr = 10 log10((Et + EPS) / (En + EPS))           (so never above 10 log10(Et / EPS + 1))
 *          5. n <= 0: si_sdr = NaN.  "Not defined" — unlike STOI's 1e-5 for a short row, which is a value pystoi reports.
 *        Two passes in float64: pass 1 sums x, y, x x, x y (mx, my and alpha follow from them), pass 2 sums (alpha x')^2 and
 *        (y' - alpha x')^2 sample by sample, so that a 100 dB result is not the difference of two large sums.  The value
 *        is rounded to f32 once, at the store.
 */
#ifndef SWC_QUALITY_H_
#define SWC_QUALITY_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_ESTOI_GROUP 4      /* segments (one wave each) per workgroup of the ESTOI segment kernel */
#define SWC_SISDR_CHUNK 8192   /* samples per workgroup of the SI-SDR sum kernel: one partial record per (row, chunk) */

/* Bytes of workspace swc_quality needs for B rows of at most max_n_in samples at rates orig : new_ (reduced by their gcd,
 * new_ the 10 kHz side), whatever outputs are asked for: swc_stoi's layout, then the ESTOI and SI-SDR intermediates.  The
 * function cannot see which outputs a call will ask for, so a call for si_sdr alone still reserves the STOI part it never
 * touches (about 130 bytes per 128 samples of max_n_in and row at 1 : 1, the resampled copies on top at another ratio); a
 * host that wants SI-SDR only keeps that small by sizing and calling with orig == new_ == 1, as the Python front end does.
 * Plain host arithmetic; -1 for B outside 0..65535, max_n_in < 0 or a rate < 1. */
int64_t swc_quality_workspace_bytes(int32_t B, int64_t max_n_in, int32_t orig, int32_t new_);

/*
 * STOI, ESTOI and SI-SDR of a ragged batch of pairs (x_b clean, y_b degraded), each n_in[b] f32 samples at one rate.
 *
 * Rows    `x_rows`, `y_rows` and `n_in` are DEVICE arrays of B addresses, B addresses and B lengths.  A row needs 4-byte
 *         alignment only.  A row with n_in[b] <= 0 is empty and its addresses are not read.  max_n_in is the HOST's bound on
 *         the lengths (it sizes the launches and the workspace); a longer row is cut at max_n_in.
 * Filter  orig, new_, width, taps_packed, tap_start, run: the packed 10 kHz table of swc_stoi
 *         (simwhisper_codec_amd.metrics.stoi_table).  With orig == new_ == 1 the table is not read (the pointers must still be
 *         non-null when stoi or estoi is asked for).  orig and new_ are >= 1 in every call.
 * Outputs `stoi`, `estoi`, `si_sdr`: f32 [B] each; any of them may be null, at least one is not.  A null output skips the
 *         kernels only it needs.  `segs` (int32 [B], may be null): the number S of segments STOI and ESTOI average (0 for a
 *         row that is too short, whose stoi and estoi are 1e-5); written when stoi or estoi is asked for, untouched otherwise.
 *         With stoi == estoi == NULL the table pointers may be null as well, the resampler's limits do not apply and neither
 *         swc_resample nor any of the energy / selection / spectrum kernels is launched: SI-SDR of 44.1 kHz rows works.
 *         Nothing else is written outside the workspace.
 * Work    `workspace`: workspace_bytes >= swc_quality_workspace_bytes(B, max_n_in, orig, new_) bytes of device memory,
 *         256-byte aligned.  Every intermediate lives there; what it held before does not matter, and what it holds
 *         afterwards is unspecified.
 * Bits    no float atomics; every sum has one fixed order that depends on the row alone.  A row's three values depend on
 *         its samples and the table only: not on B, the row's index, the alignment of its addresses, max_n_in, the launch
 *         geometry or which other outputs are asked for.  STOI / ESTOI are f32 throughout (the DFT on the f32 MFMA), SI-SDR
 *         accumulates in float64.  NaN or Inf in a row propagates into that row's values and into no other row.
 * Checks  every argument is checked before anything is launched.
 * Limits  0 <= B <= 65535 (B == 0: nothing is launched); when stoi or estoi is asked for, the resampler's LDS limit of
 *         swc_audio.h (441 : 100 does not fit and is refused) and the 10 kHz length of max_n_in below 2^31.
 */
int swc_quality(const void* const* x_rows, const void* const* y_rows, const int64_t* n_in, int64_t max_n_in, int32_t orig,
                int32_t new_, int32_t width, const float* taps_packed, const int32_t* tap_start, int32_t run, float* stoi,
                float* estoi, int32_t* segs, float* si_sdr, void* workspace, int64_t workspace_bytes, int32_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_QUALITY_H_ */
