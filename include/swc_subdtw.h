/*
 * swc_subdtw.h — C-ABI of the subsequence DTW of libswc_hip.so, in two calls: swc_cmvn normalises the cepstra of a ragged
 * batch of rows per coefficient, swc_subdtw cuts one side of every feature pair into short overlapping patches and finds, for
 * every patch on its own, the best-matching stretch anywhere in the other side (free start and end on the reference axis, a
 * small step set given by the caller), then the median of the patch costs: a score after WARP-Q (Jassim, Skoglund, Chinen,
 * Hines, ICASSP 2021); the raw alignment cost, not that paper's mapped MOS.  A header of its own beside swc_mcd.h (same
 * library, same conventions: device pointers, `stream` a hipStream_t passed as void*, every call only enqueues, 0 on success or
 * a negative SWC_E_* code with swc_last_error() giving the text; nothing allocates or synchronises).
 *
 * ---- swc_cmvn (normative; tests/subdtw_ref.py restates it in float64) ----
 *
 * Row r has T = min(max(frames[r], 0), Tmax) frames of K coefficients c[t][k] (the cep / frames layout swc_cepstra writes).
 * For every coefficient k < K, in float64 (an f32 input converts exactly):
 *
 *   sum    S(v) = the sum of v[t] over t < T in ONE order: blocks of 256 consecutive frames (the last one shorter), inside a
 *          block serially in ascending t starting from 0.0, then the blocks' sums serially in ascending block order starting
 *          from 0.0.  One rounding per addition.
 *   mean   m = S(c) / T
 *   var    v = S((c - m) (c - m)) / T: the population variance; the difference, the product and every addition rounded once
 *          each (nothing is contracted into a fused multiply-add)
 *   out    out[t][k] = (float)((c - m) / sqrt(v)), sqrt and the division correctly rounded, ONE rounding to f32 at the store;
 *          0.0f when v == 0 (a constant column, and every column of a row of one frame)
 *
 * Entries with t >= T or k >= K are NOT written; a row of 0 frames writes nothing.  A NaN (or Inf) in a column makes that
 * column NaN, and no other column.  out == cep with ldo == ldf is allowed (in place); any other overlap is not.
 *
 * ---- swc_subdtw (normative; tests/subdtw_ref.py restates it in numpy int64) ----
 *
 * Pair b is q = qf[b] (the degraded side: the one that is cut into patches) with Tq = min(max(tq[b], 0), Tmax_q) frames and
 * y = yf[b] (the reference side: the one that is searched) with Ty = min(max(ty[b], 0), Tmax_y) frames of D features each
 * (1 <= D <= 32, D <= ldf; columns k >= D and frames t >= T are never read).  Parameters of a call: the patch length Lp
 * (0 .. 256), the patch step Sp >= 1 and a step set of 1 .. 4 distinct steps (di, dj) with 0 <= di, dj <= 3, di + dj >= 1 and
 * at least one step with di >= 1 (di rows of the patch, dj columns of the reference).  Every decision is exact integer
 * arithmetic.
 *
 *   patches   Lp >= 1: P = 0 when Tq < Lp, else 1 + floor((Tq - Lp) / Sp); patch p is the L = Lp frames [p Sp, p Sp + Lp) of q.
 *             Lp == 0: the pair's whole query is its one patch (L = Tq, P = 1) when 1 <= Tq <= 256.  Otherwise P = 0 and, as
 *             the one entry such a pair writes, entry 0 of `cost` / `info` is 0 / 0, 0, 0, SWC_SUBDTW_ST_QUERY.
 *             P_max of a call is P at Tq = Tmax_q (Lp >= 1), or 1 (Lp == 0).
 *   scale     exactly swc_dtw's (swc_mcd.h): pk = max |v| over the Tq D entries of q AND the Ty D entries of y as the unsigned
 *             maximum over bit patterns (NaN or Inf wins: the pair is "not defined"), pk = m 2^e, and on both sides
 *             q = clamp(rint(v 2^(13 - e)), -8191, 8191).  A pair with Tq == 0 or Ty == 0 is empty: its features are not read.
 *   cost      exactly swc_dtw's: d[i][j] = floor(sqrt(256 sum_k (qq[i][k] - qy[j][k])^2)), d <= 91 * 16382 < 2^21
 *   DP        for a patch with rows i = 0 .. L-1 and columns j = 0 .. Ty-1:
 *             row 0: C[0][j] = d[0][j], N[0][j] = 1, origin[0][j] = j for every j (the free start); row 0 takes no predecessor.
 *             i >= 1: among the steps (di, dj) whose predecessor (i - di, j - dj) exists (i - di >= 0, j - dj >= 0) and is
 *             reachable, the one with the smallest key C 2^14 + N, ties going to the step given first.  Then C = d + C_pred,
 *             N = 1 + N_pred, origin = origin_pred; cells that a step skips are not charged.  Without such a predecessor the
 *             cell is not reachable.
 *   bound     a path has at most L + Ty - 1 <= 256 + 8192 - 1 cells, so N < 2^14, and C <= 91 * 16382 * 8447 < 2^35: the key
 *             of swc_dtw (C 2^14 + N < 2^49) is kept.
 *   end       b* = the reachable cell (L-1, j) with the smallest key, ties going to the smallest j.  Per patch:
 *             cost = C(b*) (int64), info = N(b*), start = origin(b*), end = j(b*), status.  Status: SWC_SUBDTW_ST_OK;
 *             SWC_SUBDTW_ST_UNREACHABLE when row L-1 has no reachable cell (Ty too short for the steps, Ty == 0);
 *             SWC_SUBDTW_ST_UNDEFINED when the pair is not defined.  A patch that is not ok has cost 0 and info 0, 0, 0, status.
 *   score     per pair, the median of the costs of its ok patches as exact integers: the middle one of an odd count n, and
 *             (double)(lo + hi) / 2 (exact) for an even count, with lo and hi the costs of ranks n / 2 - 1 and n / 2.  Then ONE
 *             exact scaling by 2^(e - 13) / 16 in float64 brings it into the features' own unit (the cost summed along the
 *             path, not divided by N).  NaN when no patch is ok.  patches[b] = (ok patches, P); exps[b] = e (0 for an empty or
 *             not-defined pair).
 *
 * The only atomic of the call is an unsigned integer maximum over |v|'s bit patterns.  No float atomics.
 */
#ifndef SWC_SUBDTW_H_
#define SWC_SUBDTW_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWC_SUBDTW_MAX_PATCH 256        /* rows of a patch: one per thread, one strip */
#define SWC_SUBDTW_MAX_STEPS 4          /* steps of a step set */
#define SWC_SUBDTW_MAX_STRIDE 3         /* di, dj of a step */
#define SWC_SUBDTW_MAX_FRAMES 8192      /* Tmax_q, Tmax_y (SWC_DTW_MAX_FRAMES) */
#define SWC_SUBDTW_MAX_D 32             /* features per frame (SWC_DTW_MAX_D) */
#define SWC_SUBDTW_INFO 4               /* ints per patch of `info`: N, start, end, status */
#define SWC_SUBDTW_ST_OK 0
#define SWC_SUBDTW_ST_UNREACHABLE 1
#define SWC_SUBDTW_ST_UNDEFINED 2
#define SWC_SUBDTW_ST_QUERY 3           /* Lp == 0 and the query has 0 or more than 256 frames */
#define SWC_CMVN_BLOCK 256              /* frames of a partial sum */

/*
 * Every row's cepstra normalised to zero mean and unit variance per coefficient.
 *
 * Inputs  `cep`: f32 [R][Tmax][ldf]; `frames`: DEVICE int32 [R], clamped into [0, Tmax] on the device.
 * Output  `out`: f32 [R][Tmax][ldo]; entries with t >= T_r or k >= K are NOT written.  out == cep with ldo == ldf is allowed.
 * Checks  every argument is checked before anything is launched.
 * Limits  0 <= R <= 65535 (R == 0: nothing is launched); 0 <= Tmax < 2^31 - 1; 1 <= K <= 32; ldf, ldo >= K.
 */
int swc_cmvn(const float* cep, const int32_t* frames, int32_t Tmax, int32_t K, int64_t ldf, float* out, int64_t ldo, int32_t R,
             void* stream);

/* Bytes of workspace swc_subdtw needs, with up256(v) = v rounded up to a multiple of 256 and P_max as above:
 *   up256(4 B) + up256(64 B Tmax_q) + up256(64 B Tmax_y) + up256(8 B max(P_max, 1))
 * (the pairs' peaks as uint32, the two quantised sides with 32 int16 per frame whatever D is, one int64 per patch).  Plain host
 * arithmetic; -1 for B outside 0..65535, a Tmax outside 0..8192, Lp outside 0..256 or Sp < 1. */
int64_t swc_subdtw_workspace_bytes(int32_t B, int32_t Tmax_q, int32_t Tmax_y, int32_t Lp, int32_t Sp);

/*
 * The subsequence DTW of every patch of every feature pair of a batch, and every pair's median.
 *
 * Inputs  `qf`: f32 [B][Tmax_q][ldf], `yf`: f32 [B][Tmax_y][ldf]; `tq`, `ty`: DEVICE int32 [B] frame counts, clamped into
 *         [0, Tmax] on the device.  `steps`: a HOST array of 2 n_steps int32, di then dj of every step, in the order that
 *         resolves ties; it is read before the call returns.
 * Outputs `cost`: int64 [B][ldp]; `info`: int32 [B][ldp][4] = N, start, end, status; ldp >= P_max.  Entries with p >= P of the
 *         pair are NOT written (but see SWC_SUBDTW_ST_QUERY).  `score`: float64 [B].  `patches`: int32 [B][2] = ok, P.
 *         `exps`: int32 [B] = e.  Each may be null, at least one is not.
 * Work    `workspace`: workspace_bytes >= swc_subdtw_workspace_bytes(B, Tmax_q, Tmax_y, Lp, Sp) bytes of device memory, 256-byte
 *         aligned.  What it held before does not matter; what it holds afterwards is unspecified.
 * Bits    a pair's results depend on its Tq D and Ty D features, Lp, Sp and the step set only: not on B, the pair's index, ldf,
 *         ldp, Tmax_q, Tmax_y, padding columns or frames, the launch geometry or which outputs are asked for.
 * Checks  every argument is checked before anything is launched.
 * Limits  0 <= B <= 65535 (B == 0: nothing is launched); 1 <= D <= 32, D <= ldf; 0 <= Tmax_q, Tmax_y <= 8192; 0 <= Lp <= 256;
 *         Sp >= 1; 1 <= n_steps <= 4.
 */
int swc_subdtw(const float* qf, const float* yf, const int32_t* tq, const int32_t* ty, int32_t Tmax_q, int32_t Tmax_y, int32_t D,
               int64_t ldf, int32_t Lp, int32_t Sp, const int32_t* steps, int32_t n_steps, int64_t* cost, int32_t* info,
               int64_t ldp, double* score, int32_t* patches, int32_t* exps, void* workspace, int64_t workspace_bytes, int32_t B,
               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SWC_SUBDTW_H_ */
