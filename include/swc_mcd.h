/*
 * swc_mcd.h — C-ABI of the mel-cepstral distortion of libswc_hip.so, in two calls: swc_cepstra turns a ragged batch of
 * waveforms into mel cepstra, swc_dtw finds the exact dynamic-time-warping path of a batch of feature pairs (or walks the
 * diagonal: plain MCD).  A header of its own beside swc_align.h (same library, same conventions: device pointers, `stream` a
 * hipStream_t passed as void*, every call only enqueues, 0 on success or a negative SWC_E_* code with swc_last_error() giving
 * the text; nothing allocates or synchronises).
 *
 * ---- swc_cepstra (normative; tests/mcd_ref.py restates it in float64) ----
 *
 * Parameters of a call: the window W (a power of two, 32 .. 2048), the hop H (1 <= H <= W), one packed mel bank of M filters
 * (the fb_first / fb_count / fb_off / fb_w / fb_w_len format of swc_spectral.h, 1 <= M <= W / 2 + 1) and a linear map
 * dct[K][M] (f32, 1 <= K <= 32).  For row r of n = min(max(n_in[r], 0), max_n_in) f32 samples:
 *
 *   frames   T = 1 + floor(n / H); bins F = W / 2 + 1
 *   window   w[i] = 0.5 - 0.5 cos(2 pi i / W), i = 0 .. W - 1                       (periodic Hann, as swc_spectral.h)
 *   frame t  v[i] = w[i] * x[t H - W / 2 + i], ZERO wherever that index leaves [0, n)
 *   X[t, f]  = | sum_i v[i] exp(-2 pi i f i / W) |, f = 0 .. W / 2
 *   mel      A[t, m] = sum_f fb[m][f] X[t, f], every filter's range cut into [0, F) and into [0, fb_w_len)
 *   clamp    c(v) = (v < 1e-5) ? 1e-5 : v                                           (a NaN stays a NaN: this is not fmaxf)
 *   log      L[t, m] = ln c(A[t, m])
 *   cepstra  cep[t, k] = sum_m dct[k][m] L[t, m], k = 0 .. K - 1
 *
 * Arithmetic: f32 throughout a frame (the FFT in LDS of swc_spectral: even / odd packing into W / 2 complex points, radix 2,
 * twiddles and the window evaluated in float64 and rounded once); every sum of a frame in one fixed order (ascending f,
 * ascending m, one fused multiply-add per term).  What a frame computes depends on its samples and the tables only: identical
 * rows give bit-identical cepstra, wherever they stand in the batch.
 * An empty row (n <= 0) has 0 frames and its address is not read.  NaN or Inf in a row reaches the frames that cover it.
 *
 * ---- swc_dtw (normative; tests/dtw_ref.py restates it in numpy int64) ----
 *
 * Pair b is x = xf[b] with Tx = min(max(tx[b], 0), Tmax_x) frames and y = yf[b] with Ty = min(max(ty[b], 0), Tmax_y) frames of
 * D features each (1 <= D <= 32, D <= ldf; columns k >= D and frames t >= T are never read).  Parameters of a call: the band
 * r >= 0 and the mode (SWC_DTW_WARP or SWC_DTW_DIAGONAL).  Every decision is exact integer arithmetic.
 *
 *   scale     pk = max |v| over the Tx D entries of x AND the Ty D entries of y (the unsigned maximum over the bit patterns
 *             of |v|: any NaN or Inf wins and makes the pair "not defined").  pk = m 2^e with m in [0.5, 1) (frexp; e = 0 for
 *             pk == 0) and, on BOTH sides with this one e,
 *               q = clamp(rint(v 2^(13 - e)), -8191, 8191)                 rint = round half to even; the product is exact
 *             so that every difference qx - qy fits int16.
 *   cost      s[i][j] = sum_k (qx[i][k] - qy[j][k])^2 <= 32 16382^2 < 2^33 (int64; eight terms fit an int32)
 *             d[i][j] = floor(sqrt(256 s[i][j])) as an exact integer square root, d < 2^21
 *   band      r == 0: every cell is allowed.  r >= 1: cell (i, j) is allowed iff |i Ty - j Tx| <= r max(Tx, Ty) in int64.
 *             Both corners are always allowed; consecutive rows (columns) of the band overlap, so the end is reachable.
 *   DTW       C[0][0] = d[0][0], N[0][0] = 1.  An allowed cell takes the best predecessor among (i-1, j-1), (i-1, j),
 *             (i, j-1) that exists, is allowed and is reachable: the smallest C, then the smallest N, then in that order
 *             (diagonal, then (i-1, j), then (i, j-1)); C = d + C_pred, N = 1 + N_pred.  A cell without such a predecessor is
 *             not reachable.  With C < 2^35 and N <= 16383 the pair (C, N) is one 64-bit key C 2^14 + N, and "best" is the
 *             smallest key.  total = C[Tx-1][Ty-1], N = N[Tx-1][Ty-1], and the path is the N cells from (0, 0) to
 *             (Tx-1, Ty-1) that the choices name.
 *   diagonal  SWC_DTW_DIAGONAL: the path is (t, t), t < min(Tx, Ty); N = min(Tx, Ty), total = sum_t d[t][t]; r is ignored.
 *   mean      total / (16 N) 2^(e - 13): the mean distance per path step in the features' own unit, each operation rounded
 *             once in float64 (the division, then the exact scaling), rounded to f32 once at the store.
 *   empty     an empty pair (Tx == 0 or Ty == 0) or a not-defined pair gives info = 0, 0, 0, 0, total = 0, mean = NaN and no
 *             path entry; no other pair is touched.  All-zero features give total = 0 and mean = 0.0.
 *
 * The only atomic of the call is an unsigned integer maximum over |v|'s bit patterns.  No float atomics.
 */
#ifndef SWC_MCD_H_
#define SWC_MCD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_CEPSTRA_MAX_K 32        /* rows of dct */
#define SWC_CEPSTRA_CLAMP 1e-5f     /* floor of the mel energies before the logarithm */
#define SWC_DTW_WARP 0
#define SWC_DTW_DIAGONAL 1
#define SWC_DTW_MAX_FRAMES 8192     /* Tmax_x, Tmax_y */
#define SWC_DTW_MAX_D 32            /* features per frame */
#define SWC_DTW_QBITS 13            /* |q| <= 2^13 - 1 */
#define SWC_DTW_STRIP 256           /* rows of the cost matrix a workgroup walks at a time (one per thread) */
#define SWC_DTW_INFO 4              /* ints per row of `info` */

/* Bytes of workspace swc_cepstra needs: 0 (every intermediate lives in LDS).  -1 for B outside 0..65535, max_n_in < 0, a W
 * that is not one of the seven powers of two, H outside 1..W or 2^31 frames or more. */
int64_t swc_cepstra_workspace_bytes(int32_t R, int64_t max_n_in, int32_t W, int32_t H);

/*
 * The mel cepstra of R rows (either side of a pair: one call serves both sides).
 *
 * Rows    `rows` and `n_in` are DEVICE arrays of R addresses and R lengths.  A row needs 4-byte alignment only.  A row with
 *         n_in[r] <= 0 is empty and its address is not read.  max_n_in is the HOST's bound on the lengths; a longer row is cut.
 * Tables  the mel bank as in swc_spectral.h (DEVICE arrays of M entries, fb_w of fb_w_len f32); `dct` a DEVICE f32 [K][M].
 * Outputs `cep`: f32 [R][T_max][ldf], T_max = 1 + floor(max_n_in / H), ldf >= K; entries with t >= T_r or k >= K are NOT
 *         written.  `frames`: int32 [R] = T_r, or 0 for an empty row.  Both are required.
 * Work    `workspace` may be null when workspace_bytes is 0; otherwise 256-byte aligned.
 * Checks  every argument is checked before anything is launched.
 * Limits  0 <= R <= 65535 (R == 0: nothing is launched); W one of 32 .. 2048; 1 <= H <= W; 1 <= M <= W / 2 + 1; 1 <= K <= 32.
 */
int swc_cepstra(const void* const* rows, const int64_t* n_in, int64_t max_n_in, int32_t W, int32_t H, int32_t M,
                const int32_t* fb_first, const int32_t* fb_count, const int32_t* fb_off, const float* fb_w, int64_t fb_w_len,
                const float* dct, int32_t K, float* cep, int64_t ldf, int32_t* frames, void* workspace, int64_t workspace_bytes,
                int32_t R, void* stream);

/* Bytes of workspace swc_dtw needs, with up256(v) = v rounded up to a multiple of 256:
 *   up256(4 B) + up256(8 B) + up256(64 B Tmax_x) + up256(64 B Tmax_y) + up256(2 8 B Tmax_y)
 *   + (with_path ? up256(4 B Tmax_x ceil(Tmax_y / 16)) : 0)
 * (the pairs' peaks as uint32, their final keys as uint64, the two quantised sides with 32 int16 per frame whatever D is, two
 * rows of keys per pair for the strip boundary, the 2-bit directions with sixteen cells per word).  Plain host arithmetic;
 * -1 for B outside 0..65535 or a Tmax outside 0..8192. */
int64_t swc_dtw_workspace_bytes(int32_t B, int32_t Tmax_x, int32_t Tmax_y, int32_t with_path);

/*
 * The exact DTW (or the diagonal) of every feature pair of a batch.
 *
 * Inputs  `xf`: f32 [B][Tmax_x][ldf], `yf`: f32 [B][Tmax_y][ldf]; `tx`, `ty`: DEVICE int32 [B] frame counts, clamped into
 *         [0, Tmax] on the device.
 * Outputs `total`: int64 [B].  `info`: int32 [B][4] = N, Tx, Ty, e.  `mean`: f32 [B].  `path`: int32 [B][ldp][2], the N
 *         cells (i, j) from (0, 0) to the end, ldp >= Tmax_x + Tmax_y - 1 (ldp >= 0 when either Tmax is 0); entries at and
 *         beyond N are NOT written.  Each may be null, at least one is not.
 * Work    `workspace`: workspace_bytes >= swc_dtw_workspace_bytes(B, Tmax_x, Tmax_y, path != null) bytes of device memory,
 *         256-byte aligned.  What it held before does not matter; what it holds afterwards is unspecified.
 * Bits    a pair's results depend on its Tx D and Ty D features, r and the mode only: not on B, the pair's index, ldf, Tmax_x,
 *         Tmax_y, ldp, padding columns or frames, the launch geometry or which outputs are asked for.
 * Checks  every argument is checked before anything is launched.
 * Limits  0 <= B <= 65535 (B == 0: nothing is launched); 1 <= D <= 32, D <= ldf; 0 <= Tmax_x, Tmax_y <= 8192; r >= 0.
 */
int swc_dtw(const float* xf, const float* yf, const int32_t* tx, const int32_t* ty, int32_t Tmax_x, int32_t Tmax_y, int32_t D,
            int64_t ldf, int32_t band, int32_t mode, int64_t* total, int32_t* info, float* mean, int32_t* path, int64_t ldp,
            void* workspace, int64_t workspace_bytes, int32_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_MCD_H_ */
