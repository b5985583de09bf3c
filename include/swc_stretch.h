/*
 * swc_stretch.h — C-ABI of the time stretch of libswc_hip.so: every row of a ragged batch played at another speed without a
 * change of pitch, by waveform-similarity overlap-add (WSOLA, Verhelst and Roelands 1993) with a least-squares search in exact
 * integer arithmetic (swc_stretch).  Together with a resampler it is a pitch shift.  A header of its own
 * (csrc/swc_stretch.hip behind it; same library, same conventions as the other headers: device pointers, `stream` a hipStream_t
 * passed as void*, every call only enqueues, 0 on success or a negative SWC_E_* code with the library's last-error text saying
 * why; nothing allocates or synchronises; every argument is checked before any launch; 0 <= B <= 65535 and B == 0 launches
 * nothing).  The text below is normative: tests/stretch_ref.py restates it in numpy from this text alone.
 *
 * Common definitions
 *
 *   Rows     `x_rows` and `n` are DEVICE arrays of B row addresses and B int64 lengths in samples.  A row is f32 and needs
 *            4-byte alignment only.  n_b = n[b] clamped into [0, max_n]; max_n is the HOST's bound on the lengths (it sizes the
 *            launches), 0 <= max_n <= SWC_STRETCH_MAX_N.  The address of an empty row is not read.
 *   Output   `out` is [B][ld] f32.  Columns [0, cols) of every row are written: samples in [0, len_b), zeros in [len_b, cols),
 *            where len_b is the call's output length of row b (a longer row is cut at cols).  Nothing is written in
 *            [cols, ld), before row 0 or behind row B - 1: the zero-padded batch the encoder takes.  0 <= cols <= ld.
 *   Stores   every store to device memory is an ordinary vector store or a vector atomic from plain C++.
 *
 * Parameters of a call
 *
 *   W        the window in samples: a multiple of 8, SWC_STRETCH_MIN_W <= W <= SWC_STRETCH_MAX_W.  Hs = W / 2 is the hop of
 *            the output.
 *   D        the search half-range in samples, 0 <= D <= SWC_STRETCH_MAX_D.
 *   num/den  the speed as a fraction: 1 <= num, den <= SWC_STRETCH_MAX_TERM and 1/4 <= num / den <= 4.  A speed above 1 gives
 *            a shorter row.
 *
 * The definition, per row x of n = n_b samples
 *
 *   level      peak = max |x[i]|; peak = m 2^e with m in [0.5, 1) (frexp; e = 0 for peak == 0) and
 *                q[i] = clamp(rint(x[i] 2^(15 - e)), -32767, 32767)        rint = round half to even
 *              The product is exact (a power of two).  The clamp is symmetric: |q| <= 32767.  Q(i) = q[i] for 0 <= i < n and
 *              0 outside; X(i) = x[i] for 0 <= i < n and 0 outside.  A row whose peak is NaN or Inf is "not defined": its
 *              output is zeros over [0, cols), its positions and distances are 0 and its flag is SWC_STRETCH_UNDEFINED.
 *   lengths    n_out = ceil(n den / num) samples of output (swc_stretch_out_len) in J = ceil(n_out / Hs) frames m = 0 .. J - 1.
 *   positions  a_m = floor(m Hs num / den) in int64: where frame m would be read at a constant speed.  s_{-1} = -Hs, s_0 = 0,
 *              and for m >= 1, with p = s_{m-1} + Hs (the natural continuation of frame m - 1):
 *                Dm(d) = sum_{t < W} (Q(p + t) - Q(a_m + d + t))^2         for every d in [-D, D], in exact int64
 *                d_m   = the d with the smallest Dm(d); ties go to the smaller |d|, then to d >= 0
 *                s_m   = a_m + d_m
 *              Least squares and not the raw correlation: the exact continuation has Dm = 0 and wins, so num == den is the
 *              identity (every d_m = 0) and a periodic row stays the same periodic row.
 *   output     len_b = min(n_out, cols).  For 0 <= t < len_b with j = floor(t / Hs) and u = t - j Hs:
 *                y[t] = fmaf(w[u], X(s_j + u), w[u + Hs] * X(s_{j-1} + Hs + u))
 *              The product is rounded to f32 once, then comes one f32 fused multiply-add.
 *                w[k] = (float)(0.5 - 0.5 cos(2 pi k / W)), k < W, evaluated in float64: the periodic Hann window, whose two
 *              halves add up to 1.
 *
 * Every decision is integer arithmetic: a row's positions and samples depend on the row, W, D, num and den only, not on B, the
 * row's index, the alignment of its address, max_n, cols, ld, ldm, the launch geometry or which outputs are asked for.
 */
#ifndef SWC_STRETCH_H_
#define SWC_STRETCH_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_STRETCH_MIN_W 16
#define SWC_STRETCH_MAX_W 2048
#define SWC_STRETCH_MAX_D 1024
/* the largest numerator and denominator of a speed */
#define SWC_STRETCH_MAX_TERM 65535
/* the largest num / den and den / num */
#define SWC_STRETCH_MAX_RATIO 4
/* the longest input row */
#define SWC_STRETCH_MAX_N (1 << 22)
/* samples of one row's output that one workgroup of the synthesis writes */
#define SWC_STRETCH_CHUNK 4096
/* the flag of a row that is not defined */
#define SWC_STRETCH_UNDEFINED 1

/* ceil(n den / num): the samples a row of n gives; plain host arithmetic.  -1 for n outside 0 .. SWC_STRETCH_MAX_N or a speed
 * outside its limits. */
int64_t swc_stretch_out_len(int64_t n, int32_t num, int32_t den);

/* Bytes of workspace swc_stretch needs, whatever outputs are asked for:
 *   up256(4 B) + up256(4 W) + up256(4 B Jmax)        Jmax = ceil(ceil(max_n den / num) / (W / 2))
 * with up256(v) = v rounded up to a multiple of 256: the rows' peaks as uint32, the window, every s_m as int32.  Plain host
 * arithmetic; -1 where an argument is outside its limits. */
int64_t swc_stretch_workspace_bytes(int32_t B, int64_t max_n, int32_t W, int32_t num, int32_t den);

/*
 * The stretch of every row of a ragged batch.
 *
 *   out    under the output contract above with len_b = min(n_out, cols)                                  (may be null)
 *   pos    int32 [B][ldm]: s_m in column m for m < J_b and 0 in [J_b, Jmax); nothing in [Jmax, ldm)      (may be null)
 *   dist   int64 [B][ldm]: the minimal Dm in column m (0 for m = 0), laid out like pos                   (may be null)
 *   flags  int32 [B]: SWC_STRETCH_UNDEFINED or 0                                                         (may be null)
 * At least one of the four is given; ldm >= Jmax where pos or dist is.  cols and ld are looked at only where out is given.
 *
 * Work    `workspace`: workspace_bytes >= swc_stretch_workspace_bytes(B, max_n, W, num, den) bytes of device memory, 256-byte
 *         aligned.  What it held before changes nothing; what it holds afterwards is unspecified.
 * Checks  B, W, D, num, den, max_n, 0 <= cols <= ld, ldm, the pointers and their alignment (8 bytes for x_rows, n and dist,
 *         4 for out, pos and flags), the workspace's size and alignment: all before anything is launched.
 */
int swc_stretch(const void* const* x_rows, const int64_t* n, int64_t max_n, int32_t W, int32_t D, int32_t num, int32_t den, float* out,
                int64_t ld, int64_t cols, int32_t* pos, int64_t* dist, int64_t ldm, int32_t* flags, void* workspace,
                int64_t workspace_bytes, int32_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_STRETCH_H_ */
