/*
 * swc_metrics.h — C-ABI of the quality metrics of libswc_hip.so: what says how good a reconstruction is.  A header of
 * its own beside swc.h, swc_audio.h and swc_codes.h (same library, same conventions: device pointers, `stream` a
 * hipStream_t passed as void*, every call only enqueues, 0 on success or a negative SWC_E_* code with
 * swc_last_error() giving the text; nothing allocates or synchronises).
 *
 * The reference computes STOI per file pair on one host core (tools/base_eval/evaluate_model.py, `pystoi` with
 * extended=False).  STOI (Taal, Hendriks, Heusdens, Jensen 2011) is a closed algorithm with fixed constants:
 *
 *   FS 10000, frame 256, hop 128, NFFT 512, 15 one-third octave bands from 150 Hz, 30 frames per segment, BETA -15 dB,
 *   dynamic range 40 dB, EPS 2^-52, window w[i] = hanning(258)[1 + i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257), i = 0..255.
 *
 *   1. x10, y10 = the pair resampled to 10 kHz by swc_resample with the caller's table (skipped for orig == new_ == 1)
 *   2. frames of x10 at 0, 128, ... <= len - 256; e_f = 20 log10(|w x10[f]|_2 + EPS); frame f is kept iff
 *      max_f e - 40 - e_f < 0; src[0..K) the kept frames, ascending; xs, ys = overlap-add at hop 128 of the kept windowed
 *      frames of x10, y10 (the same src for both), length (K - 1) 128 + 256
 *   3. M = K - 1 STFT frames of xs, ys at 0, 128, ... < len - 256, windowed by w again, zero-padded to 512;
 *      Xt[j][m] = sqrt(sum of |X[k]|^2 over the bins [edge_j, edge_j+1)), edges 7 9 11 14 17 22 27 34 43 55 69 87 109 138
 *      174 219; Yt likewise
 *   4. for m = 30..M (S = M - 29 segments) and every band j, a = Xt[j][m-30:m], b = Yt[j][m-30:m]:
 *      b *= |a| / (|b| + EPS); b = min(b, a (1 + 10^(15/20))); both minus their mean, both over their norm + EPS;
 *      rho = sum a b;  d = sum rho / (15 S)
 *   5. M < 30 (also n_in <= 0, K <= 1): segs = 0 and d = 1e-5 (pystoi's convention, kept so that numbers compare)
 */
#ifndef SWC_METRICS_H_
#define SWC_METRICS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_STOI_FS 10000
#define SWC_STOI_SHORT 1e-5f /* d of a row with fewer than 30 STFT frames */
#define SWC_STOI_TILE 16     /* STFT frames one workgroup of the spectrum kernel transforms */

/* Bytes of workspace swc_stoi needs for B rows of at most max_n_in samples at rates orig : new_ (reduced by their gcd,
 * new_ the 10 kHz side).  Plain host arithmetic; -1 for B outside 0..65535, max_n_in < 0 or a rate < 1. */
int64_t swc_stoi_workspace_bytes(int32_t B, int64_t max_n_in, int32_t orig, int32_t new_);

/*
 * STOI of a ragged batch of pairs (x_b clean, y_b degraded), each n_in[b] f32 samples at one rate.
 *
 * Rows    `x_rows`, `y_rows` and `n_in` are DEVICE arrays of B addresses, B addresses and B lengths (the convention of
 *         swc_resample and swc_gather_rows).  A row needs 4-byte alignment only.  A row with n_in[b] <= 0 is "too short"
 *         and its addresses are not read.  max_n_in is the HOST's bound on the lengths (it sizes the launches and the
 *         workspace); a longer row is cut at max_n_in.
 * Filter  orig, new_, width, taps_packed, tap_start, run: the packed table of swc_resample (swc_audio.h) for the rate
 *         conversion to 10 kHz, orig : new_ = fs : 10000 reduced.  For STOI it holds the Kaiser-windowed sinc of the
 *         published algorithm, K[ph][t] = new_ h[ph orig - (t - width) new_ + L], width = ceil(L / new_), built by the
 *         host in float64 (simwhisper_codec_amd.metrics.stoi_table).  With orig == new_ == 1 the table is not read
 *         (the pointers must still be non-null) and the rows are used as they are.
 * Output  d[b] (f32) and segs[b] (int32) for b in [0, B): the score and the number S of segments it averages
 *         (0 and 1e-5 for a row that is too short).  Nothing else is written outside the workspace.
 * Work    `workspace`: workspace_bytes >= swc_stoi_workspace_bytes(B, max_n_in, orig, new_) bytes of device memory,
 *         256-byte aligned.  Every intermediate lives there; what it held before does not matter, and what it holds
 *         afterwards is unspecified.
 * Bits    no float atomics; every sum has one fixed order that depends on the row alone.  d[b] and segs[b] depend on
 *         the row's samples and the table only: not on B, the row's index, the alignment of its addresses, max_n_in or
 *         the launch geometry.  The DFT runs on the f32 MFMA (f32 operands, f32 accumulation).
 *         NaN or Inf in a row propagates into that row's d (no particular value is promised) and into no other row.
 * Limits  0 <= B <= 65535 (B == 0: nothing is launched); the resampler's LDS limit of swc_audio.h (44.1 kHz -> 10 kHz,
 *         441 : 100 with 320 taps per phase, does not fit and is refused); the 10 kHz length of max_n_in below 2^31.
 */
int swc_stoi(const void* const* x_rows, const void* const* y_rows, const int64_t* n_in, int64_t max_n_in, int32_t orig,
             int32_t new_, int32_t width, const float* taps_packed, const int32_t* tap_start, int32_t run, float* d,
             int32_t* segs, void* workspace, int64_t workspace_bytes, int32_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_METRICS_H_ */
