// swc_cmvn and swc_subdtw (include/swc_subdtw.h): per-row cepstral mean / variance normalisation, and the subsequence DTW of
// every patch of every feature pair with the pair's median.  No workgroup waits for another.  Built with -ffp-contract=off: the
// header fixes the rounding of every float64 operation of swc_cmvn.
//   cmvn_kernel               one workgroup of 256 threads per row: thread (k = tid & 31, lane = tid >> 5) sums coefficient k over
//                             block `lane` of eight blocks of 256 frames at a time, serially in t; thread (k, 0) adds the eight
//                             partial sums in block order to its running total.  Twice (mean, then variance), then every thread
//                             normalises the frames t = lane, lane + 8, ... of its coefficient.
//   dtw_peak_kernel, dtw_quant_kernel   swc_dtw's own (swc_dtw_dev.h): the pair's peak, both sides as int16 in the workspace.
//   subdtw_dp_kernel<G>       grid (patch, pair), ceil(L / 64) waves: thread r owns row r of the patch (L <= 256: exactly one strip,
//                             so nothing crosses a strip boundary through the workspace) with its G = ceil(D / 8) groups of
//                             eight int16 in registers.  At step s it is at column j = s - r (an anti-diagonal per step).  The y
//                             frames stream through swc_dtw's LDS ring of two blocks of 256 frames, refilled every 256 steps.
//                             The keys (C 2^14 + N) and origins of the last 8 steps live in an LDS ring indexed by step & 7: the
//                             predecessor (i - di, j - dj) is what thread r - di wrote di + dj <= 6 steps earlier, so a step
//                             writes slot s & 7 and reads slots (s - 1 .. s - 6) & 7: one barrier per step, and no slot is
//                             written while it is read.  The step set is a kernel argument (four bits per step), not a
//                             template parameter: up to four 8-byte LDS reads per cell, and the origin of the chosen one.
//                             The thread of the last row keeps the running (key, j, origin) minimum and stores the patch.
//   subdtw_median_kernel      one workgroup per pair: the rank of every ok patch's cost among the ok costs, by counting over the
//                             order (cost, patch index); the patches of ranks (n - 1) / 2 and n / 2 are the median's two ends.
// Every loop is bounded by Ty + L, P or B.  Every store to global memory is an ordinary vector store from plain C++; the only
// atomic is the unsigned maximum of the peak.
#include "swc_dtw_dev.h"
#include "swc_subdtw.h"

namespace {

// ---------------------------------------------------------------- swc_cmvn ----

constexpr int CM_THREADS = 256;
constexpr int CM_BLOCK = SWC_CMVN_BLOCK;   // frames of a partial sum
constexpr int CM_K = 32;                   // coefficients: tid & 31
constexpr int CM_LANES = CM_THREADS / CM_K;  // blocks summed at a time
static_assert(CM_K == SWC_CEPSTRA_MAX_K, "a thread per coefficient");

// S(v) of the header for coefficient k, v = c (PASS 0) or (c - m)^2 (PASS 1); the result is valid in the threads of lane 0
template <int PASS>
__device__ __forceinline__ double cmvn_sum(const float* c, long ldf, int T, int K, int k, int lane, double m,
                                           double (&part)[CM_LANES][CM_K]) {
    const int nblk = (T + CM_BLOCK - 1) / CM_BLOCK;
    double total = 0.0;
    for (int b0 = 0; b0 < nblk; b0 += CM_LANES) {  // (uniform: every thread takes part in every barrier)
        const int blk = b0 + lane;
        double a = 0.0;
        if (k < K && blk < nblk) {
            const int t0 = blk * CM_BLOCK, t1 = T - t0 < CM_BLOCK ? T : t0 + CM_BLOCK;
            for (int t = t0; t < t1; ++t) {
                const double v = (double)c[(long)t * ldf + k];
                if (PASS == 0) {
                    a += v;
                } else {
                    const double d = v - m;
                    a += d * d;
                }
            }
        }
        part[lane][k] = a;
        __syncthreads();
        if (lane == 0) {
            for (int l = 0; l < CM_LANES && b0 + l < nblk; ++l) total += part[l][k];
        }
        __syncthreads();
    }
    return total;
}

// grid (R).  cep and out may be the same array: no __restrict__
__global__ __launch_bounds__(CM_THREADS) void cmvn_kernel(const float* cep, const int32_t* __restrict__ frames, int tmax, int K,
                                                          long ldf, float* out, long ldo) {
    __shared__ double s_part[CM_LANES][CM_K];
    __shared__ double s_mean[CM_K];
    __shared__ double s_var[CM_K];
    const int r = blockIdx.x, tid = threadIdx.x, k = tid & (CM_K - 1), lane = tid / CM_K;
    const int T = clamp_frames(frames, r, tmax);
    if (T <= 0) return;  // uniform over the workgroup
    const float* c = cep + (long)r * tmax * ldf;
    float* o = out + (long)r * tmax * ldo;
    const double s1 = cmvn_sum<0>(c, ldf, T, K, k, lane, 0.0, s_part);
    if (lane == 0) s_mean[k] = s1 / (double)T;
    __syncthreads();
    const double m = s_mean[k];
    const double s2 = cmvn_sum<1>(c, ldf, T, K, k, lane, m, s_part);
    if (lane == 0) s_var[k] = s2 / (double)T;
    __syncthreads();
    if (k >= K) return;
    const double v = s_var[k], sd = __dsqrt_rn(v);
    for (int t = lane; t < T; t += CM_LANES) {
        const double d = (double)c[(long)t * ldf + k] - m;
        o[(long)t * ldo + k] = v == 0.0 ? 0.0f : (float)__ddiv_rn(d, sd);
    }
}

// ---------------------------------------------------------------- swc_subdtw ----

constexpr int SD_MAXL = SWC_SUBDTW_MAX_PATCH;
constexpr int SD_RING = 8;                          // steps of keys and origins kept in LDS
constexpr int SD_YB = DT_S;                         // frames of a block of the y ring
static_assert(SD_MAXL == DT_THREADS, "a thread owns one row of a patch");
static_assert(2 * SWC_SUBDTW_MAX_STRIDE < SD_RING, "a predecessor is at most 6 steps old, and slot s & 7 is not one a step reads");
static_assert(SWC_SUBDTW_MAX_FRAMES == SWC_DTW_MAX_FRAMES && SWC_SUBDTW_MAX_D == SWC_DTW_MAX_D, "swc_dtw's limits");
static_assert(SD_MAXL + SWC_SUBDTW_MAX_FRAMES - 1 < (1 << DT_NBITS), "N <= L + Ty - 1 fits the key's low bits");
static_assert(DT_DMAX * (SD_MAXL + SWC_SUBDTW_MAX_FRAMES - 1LL) < (1LL << 35), "C < 2^35, so a key is below 2^49");
static_assert(SWC_SUBDTW_MAX_FRAMES <= 65536, "an origin fits 16 bits");

// L, P and the first frame's stride of a pair (include/swc_subdtw.h "patches")
__device__ __forceinline__ void patch_geometry(int Tq, int Lp, int Sp, int& L, int& P) {
    if (Lp > 0) {
        L = Lp;
        P = Tq < Lp ? 0 : 1 + (Tq - Lp) / Sp;
    } else {
        L = Tq;
        P = (Tq >= 1 && Tq <= SD_MAXL) ? 1 : 0;
    }
}

__device__ __forceinline__ void store_patch(int64_t* cost, int32_t* info, long at, long long c, int n, int start, int end, int status) {
    if (cost != nullptr) cost[at] = c;
    if (info != nullptr) *reinterpret_cast<int4*>(info + at * SWC_SUBDTW_INFO) = make_int4(n, start, end, status);
}

// grid (P_max, B), ceil(L / 64) * 64 threads: patch p of pair b
template <int G>
__global__ __launch_bounds__(DT_THREADS) void subdtw_dp_kernel(const int32_t* __restrict__ tq, const int32_t* __restrict__ ty,
                                                               int tmax_q, int tmax_y, int Lp, int Sp, int nst, unsigned steps,
                                                               const unsigned* __restrict__ peaks, const uint4* __restrict__ qq,
                                                               const uint4* __restrict__ yq, long long* __restrict__ wcost,
                                                               long ldw, int64_t* __restrict__ cost, int32_t* __restrict__ info,
                                                               long ldp) {
    constexpr int YS = G + 1;                         // uint4 per frame of the ring: one of padding against bank conflicts
    __shared__ uint4 s_y[2 * SD_YB * YS];             // frame j at block (j >> 8) & 1, slot j & 255
    __shared__ u64 s_key[SD_RING][SD_MAXL];           // [step & 7][thread that wrote it]
    __shared__ unsigned short s_org[SD_RING][SD_MAXL];
    const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
    const int Tq = clamp_frames(tq, b, tmax_q), Ty = clamp_frames(ty, b, tmax_y);
    int L, P;
    patch_geometry(Tq, Lp, Sp, L, P);
    const long at = (long)b * ldp + p;
    if (p >= P) {  // (everything up to the loop is uniform over the workgroup)
        if (Lp == 0 && p == 0 && tid == 0) store_patch(cost, info, at, 0, 0, 0, 0, SWC_SUBDTW_ST_QUERY);
        return;
    }
    int status = SWC_SUBDTW_ST_OK;
    if (Ty <= 0) status = SWC_SUBDTW_ST_UNREACHABLE;  // an empty pair: its peak was not taken
    else if (!peak_defined(peaks[b])) status = SWC_SUBDTW_ST_UNDEFINED;
    if (status != SWC_SUBDTW_ST_OK) {
        if (tid == 0) {
            wcost[(long)b * ldw + p] = -1;
            store_patch(cost, info, at, 0, 0, 0, 0, status);
        }
        return;
    }
    const int i0 = Lp > 0 ? p * Sp : 0;               // i0 + L <= Tq
    const bool mine = tid < L;
    uint4 x[G];
#pragma unroll
    for (int g = 0; g < G; ++g) x[g] = mine ? qq[((long)b * tmax_q + i0 + tid) * (DT_QW / 4) + g] : make_uint4(0u, 0u, 0u, 0u);
    const uint4* yrow = yq + (long)b * tmax_y * (DT_QW / 4);
    u64 end_key = DT_INF;
    int end_j = 0, end_org = 0;
    const int nsteps = Ty + L - 1;
    for (int s = 0; s < nsteps; ++s) {
        if ((s & (SD_YB - 1)) == 0) {  // the next 256 frames of y
            const int blk = (s >> 8) & 1;
            for (int f = tid; f < SD_YB; f += nthr) {
                if (s + f < Ty) {
#pragma unroll
                    for (int g = 0; g < G; ++g) s_y[(blk * SD_YB + f) * YS + g] = yrow[(long)(s + f) * (DT_QW / 4) + g];
                }
            }
        }
        __syncthreads();
        const int j = s - tid;
        u64 key = DT_INF;
        unsigned org = 0;
        if (mine && j >= 0 && j < Ty) {
            u64 best = DT_INF;
            if (tid == 0) {  // the free start
                best = 0;
                org = (unsigned)j;
            } else {
                int slot = 0, thr = 0;
                for (int k = 0; k < nst; ++k) {
                    const int di = (int)(steps >> (4 * k)) & 3, dj = (int)(steps >> (4 * k + 2)) & 3;
                    if (tid >= di && j >= dj) {
                        const int sl = (s - di - dj) & (SD_RING - 1);
                        const u64 v = s_key[sl][tid - di];
                        if (v < best) {  // a tie stays with the step given first
                            best = v;
                            slot = sl;
                            thr = tid - di;
                        }
                    }
                }
                if (best != DT_INF) org = s_org[slot][thr];
            }
            if (best != DT_INF) {
                uint4 y[G];
#pragma unroll
                for (int g = 0; g < G; ++g) y[g] = s_y[(((j >> 8) & 1) * SD_YB + (j & (SD_YB - 1))) * YS + g];
                key = best + ((u64)local_cost<G>(x, y) << DT_NBITS) + 1u;
                if (tid == L - 1 && key < end_key) {  // a tie stays with the smallest j
                    end_key = key;
                    end_j = j;
                    end_org = (int)org;
                }
            }
        }
        s_key[s & (SD_RING - 1)][tid] = key;
        s_org[s & (SD_RING - 1)][tid] = (unsigned short)org;
    }
    if (tid != L - 1) return;
    if (end_key == DT_INF) {
        wcost[(long)b * ldw + p] = -1;
        store_patch(cost, info, at, 0, 0, 0, 0, SWC_SUBDTW_ST_UNREACHABLE);
    } else {
        const long long c = (long long)(end_key >> DT_NBITS);
        wcost[(long)b * ldw + p] = c;
        store_patch(cost, info, at, c, (int)(end_key & ((1u << DT_NBITS) - 1u)), end_org, end_j, SWC_SUBDTW_ST_OK);
    }
}

// grid (B): the median of pair b's ok patches
__global__ __launch_bounds__(DT_THREADS) void subdtw_median_kernel(const int32_t* __restrict__ tq, const int32_t* __restrict__ ty,
                                                                   int tmax_q, int tmax_y, int Lp, int Sp,
                                                                   const unsigned* __restrict__ peaks,
                                                                   const long long* __restrict__ wcost, long ldw,
                                                                   double* __restrict__ score, int32_t* __restrict__ patches,
                                                                   int32_t* __restrict__ exps) {
    __shared__ int s_cnt[DT_THREADS / 64];
    __shared__ long long s_end[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tq = clamp_frames(tq, b, tmax_q), Ty = clamp_frames(ty, b, tmax_y);
    int L, P;
    patch_geometry(Tq, Lp, Sp, L, P);
    const long long* c = wcost + (long)b * ldw;
    int mine = 0;
    for (int p = tid; p < P; p += DT_THREADS) mine += c[p] >= 0 ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = mine;
    __syncthreads();
    int n = 0;
#pragma unroll
    for (int w = 0; w < DT_THREADS / 64; ++w) n += s_cnt[w];
    const int r_lo = (n - 1) / 2, r_hi = n / 2;
    for (int p = tid; p < P; p += DT_THREADS) {
        const long long v = c[p];
        if (v < 0) continue;
        int rank = 0;
        for (int q = 0; q < P; ++q) {
            const long long w = c[q];
            rank += (w >= 0 && (w < v || (w == v && q < p))) ? 1 : 0;
        }
        if (rank == r_lo) s_end[0] = v;   // ranks are distinct: one writer each
        if (rank == r_hi) s_end[1] = v;
    }
    __syncthreads();
    if (tid != 0) return;
    const unsigned pk = peaks[b];
    const int e = (Tq > 0 && Ty > 0 && peak_defined(pk)) ? peak_exp(pk) : 0;
    if (score != nullptr) {
        double m = __builtin_nan("");
        if (n > 0) m = ldexp((double)(s_end[0] + s_end[1]) * 0.5, e - SWC_DTW_QBITS - 4);  // both products are exact
        score[b] = m;
    }
    if (patches != nullptr) {
        patches[2 * b] = n;
        patches[2 * b + 1] = P;
    }
    if (exps != nullptr) exps[b] = e;
}

int patches_max(int tmax_q, int Lp, int Sp) {
    if (Lp == 0) return 1;
    return tmax_q < Lp ? 0 : 1 + (tmax_q - Lp) / Sp;
}

bool subdtw_limits_ok(int B, int tmax_q, int tmax_y, int Lp, int Sp) {
    return B >= 0 && B <= 65535 && tmax_q >= 0 && tmax_q <= SWC_SUBDTW_MAX_FRAMES && tmax_y >= 0 && tmax_y <= SWC_SUBDTW_MAX_FRAMES &&
           Lp >= 0 && Lp <= SWC_SUBDTW_MAX_PATCH && Sp >= 1;
}

// where swc_subdtw keeps what inside its workspace (byte offsets): the peaks [B] u32 (what the one memset clears), the quantised
// sides [B][Tmax][32] i16 and the patch costs [B][ldw] i64 (-1: not ok)
struct SubLayout {
    size_t peaks, qq, yq, wcost, total;
    long ldw;
};

SubLayout sub_layout(int B, int tmax_q, int tmax_y, int Lp, int Sp) {
    SubLayout P;
    size_t o = 0;
    const int pm = patches_max(tmax_q, Lp, Sp);
    P.ldw = pm > 1 ? pm : 1;
    P.peaks = o; o += up256((size_t)B * sizeof(unsigned));
    P.qq = o; o += up256((size_t)B * tmax_q * DT_QW * sizeof(unsigned));
    P.yq = o; o += up256((size_t)B * tmax_y * DT_QW * sizeof(unsigned));
    P.wcost = o; o += up256((size_t)B * (size_t)P.ldw * sizeof(long long));
    P.total = o;
    return P;
}

}  // namespace

extern "C" int swc_cmvn(const float* cep, const int32_t* frames, int32_t Tmax, int32_t K, int64_t ldf, float* out, int64_t ldo,
                        int32_t R, void* stream) {
    SWC_CHECK_ARG(cep && frames && out, "swc_cmvn: null pointer");
    SWC_CHECK_ARG(R >= 0 && R <= 65535, "swc_cmvn: R=%d (0..65535)", R);
    SWC_CHECK_ARG(Tmax >= 0 && Tmax < 0x7fffffff, "swc_cmvn: Tmax=%d frames out of range", Tmax);
    SWC_CHECK_ARG(K >= 1 && K <= SWC_CEPSTRA_MAX_K, "swc_cmvn: K=%d coefficients (1..%d)", K, SWC_CEPSTRA_MAX_K);
    SWC_CHECK_ARG(ldf >= K && ldo >= K, "swc_cmvn: ldf=%ld, ldo=%ld, K=%d coefficients", (long)ldf, (long)ldo, K);
    SWC_CHECK_ARG(out != cep || ldo == ldf, "swc_cmvn: in place (out == cep) needs ldo == ldf, got ldf=%ld, ldo=%ld", (long)ldf, (long)ldo);
    if (R == 0 || Tmax == 0) return SWC_OK;
    hipLaunchKernelGGL(cmvn_kernel, dim3((unsigned)R), dim3(CM_THREADS), 0, (hipStream_t)stream, cep, frames, Tmax, K, (long)ldf, out,
                       (long)ldo);
    SWC_CHECK_LAUNCH("swc_cmvn");
    return SWC_OK;
}

extern "C" int64_t swc_subdtw_workspace_bytes(int32_t B, int32_t Tmax_q, int32_t Tmax_y, int32_t Lp, int32_t Sp) {
    if (!subdtw_limits_ok(B, Tmax_q, Tmax_y, Lp, Sp)) return -1;
    return (int64_t)sub_layout(B, Tmax_q, Tmax_y, Lp, Sp).total;
}

extern "C" int swc_subdtw(const float* qf, const float* yf, const int32_t* tq, const int32_t* ty, int32_t Tmax_q, int32_t Tmax_y,
                          int32_t D, int64_t ldf, int32_t Lp, int32_t Sp, const int32_t* steps, int32_t n_steps, int64_t* cost,
                          int32_t* info, int64_t ldp, double* score, int32_t* patches, int32_t* exps, void* workspace,
                          int64_t workspace_bytes, int32_t B, void* stream) {
    SWC_CHECK_ARG(qf && yf && tq && ty && steps && workspace, "swc_subdtw: null pointer");
    SWC_CHECK_ARG(cost || info || score || patches || exps, "swc_subdtw: no output (cost, info, score, patches and exps are all null)");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_subdtw: B=%d (0..65535)", B);
    SWC_CHECK_ARG(Tmax_q >= 0 && Tmax_q <= SWC_SUBDTW_MAX_FRAMES && Tmax_y >= 0 && Tmax_y <= SWC_SUBDTW_MAX_FRAMES,
                  "swc_subdtw: Tmax_q=%d, Tmax_y=%d frames out of range (0..%d)", Tmax_q, Tmax_y, SWC_SUBDTW_MAX_FRAMES);
    SWC_CHECK_ARG(D >= 1 && D <= SWC_SUBDTW_MAX_D, "swc_subdtw: D=%d features (1..%d)", D, SWC_SUBDTW_MAX_D);
    SWC_CHECK_ARG(ldf >= D, "swc_subdtw: ldf=%ld, D=%d features", (long)ldf, D);
    SWC_CHECK_ARG(Lp >= 0 && Lp <= SWC_SUBDTW_MAX_PATCH, "swc_subdtw: patch length Lp=%d (0..%d)", Lp, SWC_SUBDTW_MAX_PATCH);
    SWC_CHECK_ARG(Sp >= 1, "swc_subdtw: patch step Sp=%d (>= 1)", Sp);
    SWC_CHECK_ARG(n_steps >= 1 && n_steps <= SWC_SUBDTW_MAX_STEPS, "swc_subdtw: n_steps=%d steps (1..%d)", n_steps, SWC_SUBDTW_MAX_STEPS);
    unsigned packed = 0;
    bool advances = false;
    for (int k = 0; k < n_steps; ++k) {
        const int di = steps[2 * k], dj = steps[2 * k + 1];
        SWC_CHECK_ARG(di >= 0 && di <= SWC_SUBDTW_MAX_STRIDE && dj >= 0 && dj <= SWC_SUBDTW_MAX_STRIDE && di + dj >= 1,
                      "swc_subdtw: step %d is (%d, %d): 0 <= di, dj <= %d and di + dj >= 1", k, di, dj, SWC_SUBDTW_MAX_STRIDE);
        for (int l = 0; l < k; ++l)
            SWC_CHECK_ARG(steps[2 * l] != di || steps[2 * l + 1] != dj, "swc_subdtw: step (%d, %d) is given twice (steps %d and %d)", di,
                          dj, l, k);
        advances = advances || di >= 1;
        packed |= ((unsigned)di | ((unsigned)dj << 2)) << (4 * k);
    }
    SWC_CHECK_ARG(advances, "swc_subdtw: no step with di >= 1: the last row of a patch is never reached");
    const int pm = patches_max(Tmax_q, Lp, Sp);
    SWC_CHECK_ARG((cost == nullptr && info == nullptr) || ldp >= pm, "swc_subdtw: ldp=%ld, a pair has up to %d patches", (long)ldp, pm);
    const SubLayout P = sub_layout(B, Tmax_q, Tmax_y, Lp, Sp);
    SWC_CHECK_ARG(workspace_bytes >= (int64_t)P.total, "swc_subdtw: workspace of %ld bytes, %ld needed (swc_subdtw_workspace_bytes)",
                  (long)workspace_bytes, (long)P.total);
    SWC_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "swc_subdtw: workspace must be 256-byte aligned");
    if (B == 0) return SWC_OK;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* base = reinterpret_cast<unsigned char*>(workspace);
    unsigned* peaks = reinterpret_cast<unsigned*>(base + P.peaks);
    unsigned* qq = reinterpret_cast<unsigned*>(base + P.qq);
    unsigned* yq = reinterpret_cast<unsigned*>(base + P.yq);
    long long* wcost = reinterpret_cast<long long*>(base + P.wcost);
    if (hipMemsetAsync(workspace, 0, P.qq, st) != hipSuccess) {  // the peaks
        (void)hipGetLastError();
        swc_set_error("swc_subdtw: clearing the peaks failed");
        return SWC_E_LAUNCH;
    }
    if (Tmax_q > 0 && Tmax_y > 0) {
        const int t_big = Tmax_q > Tmax_y ? Tmax_q : Tmax_y;
        const dim3 grid((unsigned)((t_big + DT_PK_FRAMES - 1) / DT_PK_FRAMES), (unsigned)B, 2u);
        hipLaunchKernelGGL(dtw_peak_kernel, grid, dim3(DT_THREADS), 0, st, qf, yf, tq, ty, Tmax_q, Tmax_y, D, (long)ldf, peaks);
        SWC_CHECK_LAUNCH("swc_subdtw (peak)");
        hipLaunchKernelGGL(dtw_quant_kernel, grid, dim3(DT_THREADS), 0, st, qf, yf, tq, ty, Tmax_q, Tmax_y, D, (long)ldf,
                           (const unsigned*)peaks, qq, yq);
        SWC_CHECK_LAUNCH("swc_subdtw (quantise)");
    }
    if (pm > 0) {
        const int l_max = Lp > 0 ? Lp : (Tmax_q < SD_MAXL ? Tmax_q : SD_MAXL);
        const int threads = l_max <= 64 ? 64 : (l_max + 63) / 64 * 64;
        const dim3 grid((unsigned)pm, (unsigned)B);
        const uint4* qq4 = reinterpret_cast<const uint4*>(qq);
        const uint4* yq4 = reinterpret_cast<const uint4*>(yq);
#define SWC_SUBDTW_CASE(GR)                                                                                                  \
    case GR:                                                                                                                 \
        hipLaunchKernelGGL(subdtw_dp_kernel<GR>, grid, dim3((unsigned)threads), 0, st, tq, ty, Tmax_q, Tmax_y, Lp, Sp, n_steps, \
                           packed, (const unsigned*)peaks, qq4, yq4, wcost, P.ldw, cost, info, (long)ldp);                   \
        break
        switch ((D + 7) / 8) {
            SWC_SUBDTW_CASE(1);
            SWC_SUBDTW_CASE(2);
            SWC_SUBDTW_CASE(3);
            SWC_SUBDTW_CASE(4);
        }
#undef SWC_SUBDTW_CASE
        SWC_CHECK_LAUNCH("swc_subdtw (recurrence)");
    }
    if (score != nullptr || patches != nullptr || exps != nullptr) {
        hipLaunchKernelGGL(subdtw_median_kernel, dim3((unsigned)B), dim3(DT_THREADS), 0, st, tq, ty, Tmax_q, Tmax_y, Lp, Sp,
                           (const unsigned*)peaks, (const long long*)wcost, P.ldw, score, patches, exps);
        SWC_CHECK_LAUNCH("swc_subdtw (median)");
    }
    return SWC_OK;
}
