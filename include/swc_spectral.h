/*
 * swc_spectral.h — C-ABI of the batched spectral distances of libswc_hip.so: the multi-scale mel distance, the
 * multi-resolution STFT distance and the log-spectral distance (LSD) of a ragged batch of pairs in one call.  A header of
 * its own beside swc_quality.h (same library, same conventions: device pointers, `stream` a hipStream_t passed as void*,
 * every call only enqueues, 0 on success or a negative SWC_E_* code with swc_last_error() giving the text; nothing
 * allocates or synchronises).
 *
 * The definition (normative; tests/spectral_ref.py restates it in float64).  For a pair (x clean, y degraded) of
 * n = min(max(n_in[b], 0), max_n_in) f32 samples and a scale with window W (a power of two, 32 .. 2048):
 *
 *   hop H = W / 4, bins F = W / 2 + 1, frames T = 1 + floor(n / H)
 *   window   w[i] = 0.5 - 0.5 cos(2 pi i / W), i = 0 .. W - 1                     (periodic Hann)
 *   frame t  v[i] = w[i] * x[t H - W / 2 + i], ZERO wherever that index leaves [0, n)
 *            (torch.stft(center=True, pad_mode="constant"))
 *   X[t, f]  = | sum_i v[i] exp(-2 pi i f i / W) |, f = 0 .. W / 2; Y[t, f] the same from y
 *   clamp    c(v) = (v < 1e-5) ? 1e-5 : v                                         (a NaN stays a NaN: this is not fmaxf)
 *   mel      Mx[t, m] = sum_f fb[m][f] X[t, f], m = 0 .. M - 1, My from Y
 *            mel_s    = (1 / (T M)) sum_{t, m} | log10 c(Mx) - log10 c(My) |
 *   STFT     logmag_s = (1 / (T F)) sum_{t, f} | 2 log10 c(X) - 2 log10 c(Y) |
 *            mag_s    = (1 / (T F)) sum_{t, f} | X - Y |
 *   LSD      lsd_s    = (1 / T) sum_t sqrt( (1 / F) sum_f (2 log10 c(X) - 2 log10 c(Y))^2 )
 *
 *   mel[b]   = sum of mel_s over the scales flagged SWC_SPECTRAL_MEL
 *   stft[b]  = sum of (logmag_s + mag_s) over the scales flagged SWC_SPECTRAL_STFT
 *   lsd[b]   = lsd_s of the one scale flagged SWC_SPECTRAL_LSD (0 when no scale carries the flag; two are refused)
 *   parts[b][s][0 .. 3] = mel_s, logmag_s, mag_s, lsd_s of scale s; an entry the scale's flags do not cover is 0
 *
 *   n <= 0: every value asked for is NaN ("not defined", as SI-SDR of an empty pair; in `parts` the entries the flags
 *   cover).  NaN or Inf in a row reaches that row's values and no other row's.  Identical rows give exactly 0.0 in every
 *   value: X and Y come from the same device code, one real transform each.
 *
 * Arithmetic: f32 throughout a frame (an FFT in LDS: even / odd packing into W / 2 complex points, radix 2, twiddles and the
 * window evaluated in float64 and rounded once), every sum of a frame in one fixed order; the frames of a run are added in
 * frame order in float64, the runs of a row in ascending order in float64, and a value is rounded to f32 once, at the store.
 */
#ifndef SWC_SPECTRAL_H_
#define SWC_SPECTRAL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_SPECTRAL_MAX_SCALES 8
#define SWC_SPECTRAL_MEL 1    /* flag bits of a scale */
#define SWC_SPECTRAL_STFT 2
#define SWC_SPECTRAL_LSD 4
#define SWC_SPECTRAL_MIN_WIN 32
#define SWC_SPECTRAL_MAX_WIN 2048

/* Frames per workgroup of the frame kernel ("run"), per window length: one partial record per (row, scale, run).  Chosen so
 * that every workgroup has the same amount of window work, W * run = 32768 samples (a run advances 8192 samples of the row). */
#define SWC_SPECTRAL_RUN_32 1024
#define SWC_SPECTRAL_RUN_64 512
#define SWC_SPECTRAL_RUN_128 256
#define SWC_SPECTRAL_RUN_256 128
#define SWC_SPECTRAL_RUN_512 64
#define SWC_SPECTRAL_RUN_1024 32
#define SWC_SPECTRAL_RUN_2048 16

/* Bytes of workspace swc_spectral needs for B rows of at most max_n_in samples and the scale list win[0 .. n_scales) (a
 * HOST array), whatever outputs are asked for: per scale B * ceil((1 + max_n_in / H) / run) records of four float64, each
 * scale's block rounded up to 256 bytes.  Plain host arithmetic; -1 for B outside 0..65535, max_n_in < 0, n_scales outside
 * 0..SWC_SPECTRAL_MAX_SCALES, a null win with n_scales > 0, a window that is not one of the seven powers of two, or a frame
 * count of 2^31 or more. */
int64_t swc_spectral_workspace_bytes(int32_t B, int64_t max_n_in, const int32_t* win, int32_t n_scales);

/*
 * The three distances of a ragged batch of pairs (x_b clean, y_b degraded), each n_in[b] f32 samples.
 *
 * Rows    `x_rows`, `y_rows` and `n_in` are DEVICE arrays of B addresses, B addresses and B lengths.  A row needs 4-byte
 *         alignment only.  A row with n_in[b] <= 0 is empty and its addresses are not read.  max_n_in is the HOST's bound on
 *         the lengths (it sizes the launches and the workspace); a longer row is cut at max_n_in.
 * Scales  `win`, `n_mels`, `flags`: HOST arrays of n_scales <= SWC_SPECTRAL_MAX_SCALES entries: the window W, the number
 *         M of mel filters (>= 0; 1 .. F when the scale is flagged MEL) and the flag bits.  A scale without flags costs nothing.
 * Mel     the banks of ALL scales as one packed DEVICE table, in scale order (scale s owns the n_mels[s] filters after those
 *         of the scales before it, flagged or not): fb_first[k] the first bin of filter k, fb_count[k] its number of bins
 *         (0: an empty filter, Mx = 0), fb_off[k] where its weights start in fb_w, fb_w_len the length of fb_w (f32).  The
 *         kernel cuts every filter's range into [0, F) and into [0, fb_w_len): a bad table gives wrong numbers, never an
 *         access outside the spectrum or the weights.  The four pointers may be null when no MEL work is asked for.
 * Outputs `mel`, `stft`, `lsd`: f32 [B] each; `parts`: f32 [B][n_scales][4].  Any of the four may be null, at least one is
 *         not.  A null output skips the work only it needs: without `parts`, a scale's MEL / STFT / LSD work is done only
 *         when `mel` / `stft` / `lsd` is asked for.  Nothing else is written outside the workspace.
 * Work    `workspace`: workspace_bytes >= swc_spectral_workspace_bytes(B, max_n_in, win, n_scales) bytes of device memory,
 *         256-byte aligned.  Every intermediate lives there; what it held before does not matter, and what it holds
 *         afterwards is unspecified.
 * Bits    no float atomics; every sum has one fixed order that depends on the row alone.  A row's values depend on its
 *         samples, the scale list and the mel table only: not on B, the row's index, the alignment of its addresses,
 *         max_n_in, the launch geometry or which other outputs are asked for.
 * Checks  every argument is checked before anything is launched.
 * Limits  0 <= B <= 65535 (B == 0: nothing is launched); each W one of 32, 64, 128, 256, 512, 1024, 2048; at most one scale
 *         flagged LSD; frame counts below 2^31.
 */
int swc_spectral(const void* const* x_rows, const void* const* y_rows, const int64_t* n_in, int64_t max_n_in,
                 const int32_t* win, const int32_t* n_mels, const int32_t* flags, int32_t n_scales, const int32_t* fb_first,
                 const int32_t* fb_count, const int32_t* fb_off, const float* fb_w, int64_t fb_w_len, float* mel, float* stft,
                 float* lsd, float* parts, void* workspace, int64_t workspace_bytes, int32_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_SPECTRAL_H_ */
