/*
 * swc_degrade.h — C-ABI of the degradations of libswc_hip.so: reproducible noise (swc_noise), mixing a noise row into a speech
 * row at a signal-to-noise ratio whose gain is computed on the device (swc_mix), and the convolution of a ragged batch with
 * impulse responses of up to 131072 taps (swc_convolve).  A header of its own (csrc/swc_degrade.hip behind it; same library, same
 * conventions as the metric headers: device pointers, `stream` a hipStream_t passed as void*, every call only enqueues, 0 on
 * success or a negative SWC_E_* code with the library's last-error text saying why; nothing allocates or synchronises; every
 * argument is checked before any launch; 0 <= B <= 65535 and B == 0 launches nothing).  The text below is normative:
 * tests/degrade_ref.py restates it in numpy from this text alone.
 *
 * Common definitions
 *
 *   Rows     `rows` and `n` are DEVICE arrays of B row addresses and B int64 lengths in samples.  A row is f32 and needs 4-byte
 *            alignment only.  A length below 0 counts as 0; the address of an empty row is not read.
 *   Output   `out` is [B][ld] f32.  Columns [0, cols) of every row are written: samples in [0, len_b), zeros in [len_b, cols),
 *            where len_b is the call's output length of row b (a longer row is cut at cols).  Nothing is written in
 *            [cols, ld), before row 0 or behind row B - 1: the zero-padded batch the encoder takes.  0 <= cols <= ld.
 *   Stores   every store to device memory is an ordinary vector store or a vector atomic from plain C++.
 */
#ifndef SWC_DEGRADE_H_
#define SWC_DEGRADE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the longest impulse response of swc_convolve (8.2 s at 16 kHz) */
#define SWC_CONV_MAX_TAPS 131072
/* samples of one partition of an impulse response and of one block of output; the transforms have twice as many points */
#define SWC_CONV_BLOCK 1024
/* the longest row swc_convolve takes */
#define SWC_CONV_MAX_N (1 << 30)
/* the most impulse responses of one swc_convolve call */
#define SWC_CONV_MAX_IRS 65535
/* samples of one row that one workgroup of swc_noise and swc_mix writes */
#define SWC_DEGRADE_CHUNK 4096
/* flag bits of swc_mix */
#define SWC_MIX_UNMIXED 1
#define SWC_MIX_OVER 2

/*
 * Noise.  Sample i (0 <= i < n[b]) of row b is a function of (seed, s = stream_ids[b], j = first + i) alone, in exact integer
 * arithmetic:
 *
 *   (w0, w1, w2, w3) = Philox4x32-10 (Salmon et al. 2011, as Random123 has it) of the counter (j lo32, j hi32, s lo32, s hi32)
 *   under the key (seed lo32, seed hi32).  One round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to
 *       (hi(0xCD9E8D57 c2) ^ c1 ^ k0,  lo(0xCD9E8D57 c2),  hi(0xD2511F53 c0) ^ c3 ^ k1,  lo(0xD2511F53 c0))
 *   with hi / lo the halves of the 64-bit product; after every round but the tenth the key becomes
 *   (k0 + 0x9E3779B9, k1 + 0xBB67AE85) mod 2^32.
 *   h = the sum of the eight 16-bit halves of w0 .. w3;  V = 2 h - 8 * 65535;  sample = V * 2^-19 (exact in f32).
 *
 * This is an Irwin-Hall sum of eight uniform variables: zero mean, variance (8/3)(2^32 - 1) / 2^38 (about 1/24, -13.8 dB
 * relative to full scale), |sample| < 1, and an excess kurtosis of -0.15.  It is close to Gaussian in the middle and has no
 * tails: it is NOT Gaussian noise, and nothing here calls it that.  It is white: samples are independent.
 *
 *   stream_ids  DEVICE int64 [B], taken as 64 unsigned bits: the batches of a corpus give every row its own id and do not
 *               repeat one another
 *   first       >= 0: the index of column 0 in the stream (a row can be produced in pieces)
 *   out         under the output contract above with len_b = n[b]
 * Bits depend on (seed, stream id, first + i) only: not on B, the row's index, ld, cols or the geometry.
 * Checks  pointers, 0 <= B <= 65535, first >= 0, 0 <= cols <= ld.
 */
int swc_noise(uint64_t seed, const int64_t* stream_ids, const int64_t* n, int64_t first, float* out, int64_t ld, int64_t cols,
              int32_t B, void* stream);

/*
 * Mixing at a signal-to-noise ratio.  With x_b the speech row (n_b = n_x[b] samples) and v_b the noise row (m_b = n_noise[b]):
 *
 *   out_b[i] = fmaf(v_b[i mod m_b], g_b, x_b[i])            one f32 fused multiply-add, 0 <= i < n_b
 *   g_b      = (float) 10^((Lx_b - Ln_b - snr_b) / 20)      evaluated in float64, rounded to f32 once
 *
 * Lx_b = lx[b lx_stride], Ln_b = ln[b ln_stride], snr_b = snr[b snr_stride]: three DEVICE float64 arrays, each with a stride in
 * ELEMENTS (>= 0; 0 gives every row the same value): a level in dB per row of the speech and of the noise, as a measuring call
 * left them on the device, and the target in dB.  They can be column views of one matrix of values, and which level they are
 * (active, long-term, a loudness) is the caller's choice.  A noise row shorter than the speech row wraps around; of a longer one
 * the first n_b samples are used.
 *
 * A row whose Lx, Ln or snr is not finite, or whose m_b is 0, is copied unmixed (out_b = x_b), gets the gain 0 and the flag
 * SWC_MIX_UNMIXED.  (A finite exponent beyond f32's range gives g_b = inf or 0 like any other f32 rounding.)
 *
 *   out    under the output contract above with len_b = n_b                                    (may be null)
 *   gains  f32 [B]: g_b                                                                         (may be null)
 *   flags  int32 [B]: SWC_MIX_UNMIXED | SWC_MIX_OVER, the second where some |out_b[i]| > 1, i < min(n_b, cols): the mixture
 *          leaves full scale and a 16-bit file of it would clip                                 (may be null)
 * At least one of the three is given.  `cols` bounds the samples looked at also where out is null.
 * Checks  pointers, 0 <= B <= 65535, strides >= 0, 0 <= cols <= ld.
 */
int swc_mix(const void* const* x_rows, const int64_t* n_x, const void* const* noise_rows, const int64_t* n_noise, const double* lx,
            int64_t lx_stride, const double* ln, int64_t ln_stride, const double* snr, int64_t snr_stride, float* out, int64_t ld,
            int64_t cols, float* gains, int32_t* flags, int32_t B, void* stream);

/*
 * Convolution with impulse responses.  With h_r the R responses (`h_rows`, `h_len`: DEVICE arrays of R addresses and R int64
 * lengths L_r, clamped into [0, max_L] on the device; 1 <= L_r is expected, L_r = 0 gives a zero row), r = h_index[b] (DEVICE
 * int64 [B], clamped into [0, R); may be null when R == 1) and x_b zero outside [0, n_b), n_b = n[b] clamped into [0, max_n]:
 *
 *   y_b[i] = sum_{k < L_r} h_r[k] x_b[i + d - k]        0 <= i < len_b = min(n_b + extra, cols)
 *
 * d is the index of the direct path in the responses: the output stays sample-aligned with the input, and code streams of
 * the two compare frame for frame.  extra = 0 keeps every row's length; extra = max_L - 1 - d keeps the whole tail.
 * 1 <= max_L <= SWC_CONV_MAX_TAPS, 0 <= d < max_L, 0 <= extra <= max_L - 1, 0 <= max_n <= SWC_CONV_MAX_N, 1 <= R <=
 * SWC_CONV_MAX_IRS.
 *
 * The method is normative, because it fixes the bits: uniformly partitioned overlap-save with blocks of N = SWC_CONV_BLOCK
 * samples and real transforms of 2 N points done as N packed complex points.
 *
 *   Twiddles   t[q] = exp(-2 pi i q / (2 N)), q < N, evaluated in float64 and rounded to f32.
 *   Forward    of 2 N real samples v: z[k] = v[2 k] + i v[2 k + 1]; Z = the N-point DFT of z by radix-2 decimation in time
 *              (bit-reversed input, stages of half-size 1, 2, .. N / 2, a butterfly (u, v) -> (u + w v, u - w v) with
 *              w = t[k N / h] for the k-th butterfly of a group of half-size h); then for f < N, with A = Z[f] and
 *              Bc = conj Z[(N - f) mod N]:  E = (A + Bc) / 2,  O = -i (A - Bc) / 2,  S[f] = E + t[f] O.  S[0] is real and its
 *              imaginary part holds the Nyquist bin Re Z[0] - Im Z[0] instead (packed beside DC).  All in f32.
 *   Windows    window w of row b is the 2 N samples x_b[N (w - 1) + d + t], t < 2 N; X_b,w its forward transform.
 *   Partitions partition p of response r is h_r[N p + t] for t < N and zero for N <= t < 2 N; H_r,p its forward transform;
 *              P_r = ceil(L_r / N).
 *   Sum        for output block j (samples N j .. N j + N - 1): Y[f] = sum over p = 0 .. P_r - 1 ascending, skipping every p
 *              whose window j - p holds no sample of the row (n_b = 0, N (j - p + 1) + d <= 0 or N (j - p - 1) + d >= n_b), of
 *              X_b,j-p[f] H_r,p[f]: for f >= 1 the complex product accumulated as
 *                  re = fmaf(Xr, Hr, fmaf(-Xi, Hi, re)),  im = fmaf(Xr, Hi, fmaf(Xi, Hr, im)),
 *              for f = 0 the two real products re = fmaf(Xr, Hr, re), im = fmaf(Xi, Hi, im); all from +0.
 *   Inverse    Z'[0] = (Y[0].re + Y[0].im, Y[0].re - Y[0].im); for 1 <= f < N, with A = Y[f] and Bc = conj Y[N - f]:
 *              E = A + Bc,  P = A - Bc,  O = conj(t[f]) P,  Z'[f] = E + i O.  z' = the same radix-2 network over Z' with
 *              conj(w) in place of w; the 2 N real samples are v'[2 k] = Re z'[k] / (2 N), v'[2 k + 1] = Im z'[k] / (2 N)
 *              (an exact scaling), and y_b[N j + t] = v'[N + t], t < N.
 *
 * A row's output depends on its samples, its response, d and extra only: not on B, the row's index, the other rows' responses,
 * max_n, cols or the geometry.
 *
 * Workspace  swc_convolve_workspace_bytes(B, max_n, R, max_L) = 8 N (B W + R Pmax) bytes with W = ceil(max_n / N) + 2 windows
 *            a row and Pmax = ceil(max_L / N); -1 where an argument is outside its limits.  256-byte aligned.  It holds the
 *            spectra; what it held before changes nothing.
 * Checks  pointers, 0 <= B <= 65535, R, max_L, d, extra, max_n, 0 <= cols <= ld, the workspace's size and alignment.
 */
int64_t swc_convolve_workspace_bytes(int32_t B, int64_t max_n, int32_t R, int32_t max_L);
int swc_convolve(const void* const* x_rows, const int64_t* n, int64_t max_n, const void* const* h_rows, const int64_t* h_len,
                 int32_t R, int32_t max_L, const int64_t* h_index, int32_t d, int32_t extra, float* out, int64_t ld, int64_t cols,
                 void* workspace, int64_t workspace_bytes, int32_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_DEGRADE_H_ */
