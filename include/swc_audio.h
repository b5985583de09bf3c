/*
 * swc_audio.h — C-ABI of the audio front end of libswc_hip.so: what happens to a waveform before the codec's
 * first kernel.  A header of its own beside swc.h (same library, same conventions: device pointers, `stream` a
 * hipStream_t passed as void*, every call only enqueues, 0 on success or a negative SWC_E_* code with
 * swc_last_error() giving the text; nothing allocates or synchronises).
 *
 * The reference leaves sample-rate conversion to torchaudio on the host (utils/helpers.py:86-87:
 * `torchaudio.transforms.Resample(sr, target)(wav)` after the channel mean of helpers.py:82-83), one file at a time.
 */
#ifndef SWC_AUDIO_H_
#define SWC_AUDIO_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_PCM_F32 0 /* rows are mono float samples */
#define SWC_PCM_I16 1 /* rows are 16-bit integers, `ch` channels interleaved (the data chunk of a PCM16 WAV) */

/* f32 words of LDS one workgroup of swc_resample may use (64 KiB; see "Limits" below) */
#define SWC_RESAMPLE_MAX_LDS_FLOATS 16384

/* ceil(new_rate * n_in / orig_rate): the output length of swc_resample for a row of n_in samples (0 for n_in <= 0;
 * -1 for a rate < 1).  Plain host arithmetic. */
int64_t swc_resample_out_len(int64_t n_in, int32_t orig_rate, int32_t new_rate);

/*
 * Sample-rate conversion of a ragged batch in ONE launch: band-limited sinc interpolation as a polyphase FIR
 * (torchaudio's documented `sinc_interp_hann`; replaces utils/helpers.py:82-87 of the reference, the channel mean
 * included).  `orig` and `new_` are the two rates REDUCED by their gcd, `width` the one-sided filter width in input
 * samples, taps = 2 width + orig.  With K[new_][taps] the f32 filter table of simwhisper_codec_amd.wavio.resample_taps,
 *
 *   out[b][f * new_ + p] = sum_t K[p][t] * xpad_b[f * orig + t],   xpad_b[i] = x_b[i - width] inside [0, n_in[b]), else 0
 *   for f * new_ + p < n_out[b] = swc_resample_out_len(n_in[b], orig, new_)
 *
 * Rows    `rows` and `n_in` are DEVICE arrays of B row addresses and B lengths in samples per channel (the convention
 *         of swc_gather_rows: views into one staging buffer cost nothing).  A row needs the alignment of its element
 *         only (4 bytes for f32, 2 for int16); 16-byte aligned spans are read with 16-byte loads.  n_in[b] <= 0 gives
 *         an all-zero row and its address is not read.
 * Input   in_format SWC_PCM_F32: x_b[i] = row[i], `ch` must be 1.
 *         in_format SWC_PCM_I16: x_b[i] = (float)(row[i ch] + ... + row[i ch + ch - 1], summed in int32) * (float)(2^-15 / ch),
 *         ch in 1..8.  The integer sum is exact and exactly representable, so this is ONE rounding.  For ch = 1 and 2 it
 *         is bit for bit what wavio.load_audio computes on the host (sample / 32768, then numpy's f32 mean); for ch > 2
 *         numpy's mean rounds after every addition and after the division, several roundings instead of this one.
 *         Down-mix, scaling and filtering happen in the one kernel: no f32 copy at the input rate is written.
 * Table   the filter is mostly zeros where the reduced ratio is large (44.1 -> 16 kHz: 475 taps per phase, 33 - 34 of
 *         them non-zero).  It is passed packed: `tap_start[new_]` (int32, 0 <= tap_start[p] <= taps - run) and
 *         `taps_packed[new_][run]` = K[p][tap_start[p] .. tap_start[p] + run), `run` >= the longest non-zero run of
 *         any phase, every non-zero tap of phase p inside its window.  Built on the host from the table's own f32
 *         values (a device sinf would not reproduce the float64-built table); both are DEVICE arrays.
 * Sum     every output sample is ONE chain acc = fmaf(taps_packed[p][k], xpad[...], acc), k = 0 .. run - 1 ascending,
 *         acc starting at +0: its bits depend on the row's samples and the table only, not on B, the row's index,
 *         the alignment of its address, cols, ld_out or the launch geometry.  (Taps outside the window are exact
 *         zeros: skipping them changes no bit for finite input.)
 * Output  out is [B][ld_out] f32.  Columns [0, cols) of every row are written: samples in [0, n_out[b]), zeros in
 *         [n_out[b], cols) (a row longer than cols is cut at cols).  Nothing is written in [cols, ld_out), before
 *         row 0 or behind row B - 1.  This is the zero-padded batch encode() needs.
 * Limits  B <= 65535; the input span of 256 outputs and the phases they use must fit the LDS tile:
 *         (255 / new_ + 1) * orig + taps + min(new_, 256) * ((run | 1) + 1) <= SWC_RESAMPLE_MAX_LDS_FLOATS
 *         (every pair of the usual audio rates 8 ... 192 kHz does).
 */
int swc_resample(const void* const* rows, const int64_t* n_in, int32_t in_format, int32_t ch, int32_t orig, int32_t new_,
                 int32_t width, const float* taps_packed, const int32_t* tap_start, int32_t run, float* out,
                 int64_t ld_out, int64_t cols, int32_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_AUDIO_H_ */
