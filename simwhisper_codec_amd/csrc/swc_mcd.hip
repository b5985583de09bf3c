// swc_cepstra and swc_dtw (include/swc_mcd.h): mel cepstra of a ragged batch of rows, and the exact DTW of a batch of feature
// pairs.  No workgroup waits for another.
//   cepstra_frames_kernel<W>  the frame kernel of swc_spectral.hip for ONE signal and any hop (geometry, tables, FFT in LDS and
//                             mel band are swc_frame_fft.h, which both include): a workgroup of 256 threads takes a run of
//                             32768 / W consecutive frames of one row, a team of min(W / 2, 256) threads owns a frame.  Per
//                             frame: its W / 2 + 1 magnitudes, then thread m the m-th mel sum and its logarithm into LDS, then
//                             thread k the k-th cepstral coefficient: every sum sequential in one thread, one fmaf per term.
//   dtw_peak_kernel           max |v| over both sides of a pair as an unsigned maximum over bit patterns, one atomic per workgroup.
//   dtw_quant_kernel          both sides as int16 against the pair's one scale, 32 per frame (zero from column D on), in the workspace.
//   dtw_dp_kernel<G>          one workgroup of 256 threads per pair walks the cost matrix in strips of SWC_DTW_STRIP = 256 rows,
//                             thread r owning row i0 + r with its G = ceil(D / 8) groups of eight int16 in registers.  At step s
//                             it is at column j = s - r (an anti-diagonal per step).  The y frames stream through an LDS ring of
//                             two blocks of 256 frames, refilled every 256 steps.  The key (C 2^14 + N) of (i-1, j) is what
//                             thread r - 1 wrote to LDS one step earlier (two buffers, one barrier per step), (i-1, j-1) is
//                             what this thread read one step earlier, (i, j-1) its own last key.  Thread 0's neighbour is the last
//                             row of the strip before, which went to the workspace (two rows per pair, used in turn) and comes
//                             back through LDS 256 columns at a time.  Registers and LDS do not depend on T.  With `path` every
//                             thread collects the 2-bit choices of sixteen cells of its row in a register and stores the word.
//   dtw_diag_kernel<G>        SWC_DTW_DIAGONAL: one workgroup per pair, int64 sum of d[t][t], the path written as it goes.
//   dtw_finish_kernel         one thread per pair: total, info, mean.   dtw_backtrack_kernel: one thread per pair walks the
//                             direction bits from the end and writes the N cells.
// Everything up to the one division of `mean` is integer arithmetic.  Every store to global memory is an ordinary vector store
// from plain C++; the only atomic is the unsigned maximum of the peak.
#include "swc_frame_fft.h"
#include "swc_mcd.h"
#include "swc_dtw_dev.h"

namespace {

// ---------------------------------------------------------------- swc_cepstra ----

constexpr int CP_THREADS = FR_THREADS;
constexpr int CP_RUN_SAMPLES = FR_RUN_SAMPLES;  // W * frames of a run
constexpr float CP_CLAMP = SWC_CEPSTRA_CLAMP;

__device__ __forceinline__ float clamp_floor(float v) { return v < CP_CLAMP ? CP_CLAMP : v; }  // NaN stays NaN

// grid (runs, R rows)
template <int W>
__global__ __launch_bounds__(CP_THREADS) void cepstra_frames_kernel(
    const void* const* __restrict__ rows, const int64_t* __restrict__ n_in, long max_n, int H, int M,
    const int32_t* __restrict__ fb_first, const int32_t* __restrict__ fb_count, const int32_t* __restrict__ fb_off,
    const float* __restrict__ fb_w, long fb_w_len, const float* __restrict__ dct, int K, float* __restrict__ cep, long ldf,
    long t_max, int32_t* __restrict__ frames) {
    using G = FrameGeo<W>;
    constexpr int N = G::N, F = G::F, TS = G::TS, TEAMS = G::TEAMS, R = G::R;
    __shared__ float2 s_tw[N];  // exp(-2 pi i q / W)
    __shared__ float s_win[W];
    __shared__ float2 s_z[TEAMS][N];
    __shared__ float s_mag[TEAMS][F + 1];
    __shared__ float s_log[TEAMS][F + 1];  // M <= F
    const int b = blockIdx.y, tid = threadIdx.x, team = tid / TS, lt = tid % TS;
    const long n = clamp_len(n_in, b, max_n);
    const long T = n > 0 ? 1 + n / H : 0;
    if (blockIdx.x == 0 && tid == 0) frames[b] = (int32_t)T;
    if (n <= 0) return;  // an empty row: its address is not read (uniform over the workgroup)
    const long t0 = (long)blockIdx.x * R;
    if (t0 >= T) return;
    const int nfr = (int)(T - t0 < R ? T - t0 : R);
    const float* row[1] = {reinterpret_cast<const float*>(rows[b])};
    frame_tables<W>(s_tw, s_win, tid);

    for (int pass = 0; pass * TEAMS < nfr; ++pass) {  // (uniform: every team takes part in every barrier)
        const int r = pass * TEAMS + team;
        const bool active = r < nfr;                  // a team past the row's last frame works on zeros and stores nothing
        const long start = (t0 + r) * (long)H - N;    // the frame's first sample
        frame_magnitudes<W, 1>(row, n, start, active, lt, s_tw, s_win, &s_z[team], &s_mag[team]);
        for (int m = lt; m < M; m += TS) {
            float a[1];
            mel_band<F, 1>(fb_first[m], fb_count[m], fb_off[m], fb_w, fb_w_len, &s_mag[team], a);
            s_log[team][m] = logf(clamp_floor(a[0]));
        }
        __syncthreads();
        for (int k = lt; k < K; k += TS) {
            const float* c = dct + (long)k * M;
            float a = 0.0f;
            for (int m = 0; m < M; ++m) a = fmaf(c[m], s_log[team][m], a);
            if (active) cep[((long)b * t_max + (t0 + r)) * ldf + k] = a;
        }
        __syncthreads();  // s_z, s_mag and s_log are free again
    }
}

template <int W>
void launch_cepstra(dim3 grid, hipStream_t st, const void* const* rows, const int64_t* n_in, long max_n, int H, int M,
                    const int32_t* fb_first, const int32_t* fb_count, const int32_t* fb_off, const float* fb_w, long fb_w_len,
                    const float* dct, int K, float* cep, long ldf, long t_max, int32_t* frames) {
    hipLaunchKernelGGL(cepstra_frames_kernel<W>, grid, dim3(CP_THREADS), 0, st, rows, n_in, max_n, H, M, fb_first, fb_count, fb_off,
                       fb_w, fb_w_len, dct, K, cep, ldf, t_max, frames);
}

// T_max of a call, or -1 when the arguments have none
long cepstra_frames(int R, long max_n, int W, int H) {
    if (R < 0 || R > 65535 || max_n < 0 || !valid_window(W) || H < 1 || H > W) return -1;
    const long T = 1 + max_n / H;
    return T >= 0x7fffffffL ? -1 : T;
}

// ---------------------------------------------------------------- swc_dtw ----

// (the limits, quantise13, local_cost, dtw_peak_kernel and dtw_quant_kernel are swc_dtw_dev.h, which swc_subdtw.hip includes too)

// grid (B): the recurrence of pair b, strip by strip
template <int G>
__global__ __launch_bounds__(DT_THREADS) void dtw_dp_kernel(const int32_t* __restrict__ tx, const int32_t* __restrict__ ty,
                                                            int tmax_x, int tmax_y, int band, const unsigned* __restrict__ peaks,
                                                            const uint4* __restrict__ xq, const uint4* __restrict__ yq,
                                                            u64* __restrict__ bound, unsigned* __restrict__ dirs, long dir_ld,
                                                            u64* __restrict__ res) {
    constexpr int YS = G + 1;                         // uint4 per frame of the ring: one of padding against bank conflicts
    __shared__ uint4 s_y[2 * DT_S * YS];              // frame j at block (j >> 8) & 1, slot j & 255
    __shared__ u64 s_key[2][DT_S + 1];                // [step parity][1 + thread that wrote it]
    __shared__ u64 s_up[2][DT_S];                     // the row above the strip, 256 columns at a time
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tx = clamp_frames(tx, b, tmax_x), Ty = clamp_frames(ty, b, tmax_y);
    if (Tx <= 0 || Ty <= 0 || !peak_defined(peaks[b])) return;  // uniform over the workgroup
    const long long width = (long long)band * (Tx > Ty ? Tx : Ty);
    const uint4* yrow = yq + (long)b * tmax_y * (DT_QW / 4);
    for (int i0 = 0, strip = 0; i0 < Tx; i0 += DT_S, ++strip) {
        const int nrows = Tx - i0 < DT_S ? Tx - i0 : DT_S, i = i0 + tid;
        const bool mine = tid < nrows;
        uint4 x[G];
#pragma unroll
        for (int g = 0; g < G; ++g) x[g] = mine ? xq[((long)b * tmax_x + i) * (DT_QW / 4) + g] : make_uint4(0u, 0u, 0u, 0u);
        const u64* b_in = bound + ((long)b * 2 + ((strip + 1) & 1)) * tmax_y;   // written by the strip before
        u64* b_out = bound + ((long)b * 2 + (strip & 1)) * tmax_y;
        const bool writes_bound = tid == nrows - 1 && i0 + DT_S < Tx;           // the last row, when another strip follows
        s_key[0][tid + 1] = DT_INF;
        s_key[1][tid + 1] = DT_INF;
        if (tid == 0) s_key[0][0] = s_key[1][0] = DT_INF;
        u64 left = DT_INF, diag = DT_INF;
        unsigned word = 0;
        long long off = (long long)i * Ty + (long long)tid * Tx;  // i Ty - j Tx at j = s - tid: Tx less with every step
        const int steps = Ty + nrows - 1;
        for (int s = 0; s < steps; ++s) {
            if ((s & (DT_S - 1)) == 0) {  // the next 256 frames of y and keys of the row above
                const int jj = s + tid, blk = (s >> 8) & 1;
                if (jj < Ty) {
#pragma unroll
                    for (int g = 0; g < G; ++g) s_y[(blk * DT_S + tid) * YS + g] = yrow[(long)jj * (DT_QW / 4) + g];
                }
                s_up[blk][tid] = (strip > 0 && jj < Ty) ? b_in[jj] : DT_INF;
            }
            __syncthreads();
            const int j = s - tid;
            const u64 up = tid == 0 ? s_up[(s >> 8) & 1][s & (DT_S - 1)] : s_key[(s + 1) & 1][tid];
            u64 key = DT_INF;
            if (mine && j >= 0 && j < Ty) {
                unsigned dir = 3u;
                if (band == 0 || (off < 0 ? -off : off) <= width) {
                    u64 best = diag;
                    dir = 0u;
                    if (up < best) { best = up; dir = 1u; }
                    if (left < best) { best = left; dir = 2u; }
                    if (i == 0 && j == 0) best = 0;
                    if (best != DT_INF) {
                        uint4 y[G];
#pragma unroll
                        for (int g = 0; g < G; ++g) y[g] = s_y[(((j >> 8) & 1) * DT_S + (j & (DT_S - 1))) * YS + g];
                        key = best + ((u64)local_cost<G>(x, y) << DT_NBITS) + 1u;
                    }
                }
                left = key;
                if (dirs != nullptr) {
                    word |= dir << (2 * (j & 15));
                    if ((j & 15) == 15 || j == Ty - 1) {
                        dirs[((long)b * tmax_x + i) * dir_ld + (j >> 4)] = word;
                        word = 0;
                    }
                }
                if (writes_bound) b_out[j] = key;
                if (i == Tx - 1 && j == Ty - 1) res[b] = key;
            }
            diag = up;
            off -= Tx;
            s_key[s & 1][tid + 1] = key;
        }
        __syncthreads();  // the strip's last row is in the workspace, and LDS is free again
    }
}

// grid (B): the diagonal of pair b
template <int G>
__global__ __launch_bounds__(DT_THREADS) void dtw_diag_kernel(const int32_t* __restrict__ tx, const int32_t* __restrict__ ty,
                                                              int tmax_x, int tmax_y, const unsigned* __restrict__ peaks,
                                                              const uint4* __restrict__ xq, const uint4* __restrict__ yq,
                                                              int32_t* __restrict__ path, long ldp, u64* __restrict__ res) {
    __shared__ long long wsum[DT_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tx = clamp_frames(tx, b, tmax_x), Ty = clamp_frames(ty, b, tmax_y);
    if (Tx <= 0 || Ty <= 0 || !peak_defined(peaks[b])) return;
    const int n = Tx < Ty ? Tx : Ty;
    long long sum = 0;
    for (int t = tid; t < n; t += DT_THREADS) {
        uint4 x[G], y[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            x[g] = xq[((long)b * tmax_x + t) * (DT_QW / 4) + g];
            y[g] = yq[((long)b * tmax_y + t) * (DT_QW / 4) + g];
        }
        sum += local_cost<G>(x, y);
        if (path != nullptr) {
            path[((long)b * ldp + t) * 2] = t;
            path[((long)b * ldp + t) * 2 + 1] = t;
        }
    }
    sum = wave_sum_i64(sum);
    if ((tid & 63) == 0) wsum[tid >> 6] = sum;
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < DT_THREADS / 64; ++w) sum += wsum[w];
    res[b] = ((u64)sum << DT_NBITS) + (u64)n;
}

// one thread per pair: total, info, mean
__global__ __launch_bounds__(64) void dtw_finish_kernel(const int32_t* __restrict__ tx, const int32_t* __restrict__ ty, int tmax_x,
                                                        int tmax_y, const unsigned* __restrict__ peaks, const u64* __restrict__ res,
                                                        int64_t* __restrict__ total, int32_t* __restrict__ info,
                                                        float* __restrict__ mean, int B) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int Tx = clamp_frames(tx, b, tmax_x), Ty = clamp_frames(ty, b, tmax_y);
    const unsigned pk = peaks[b];
    u64 key = DT_INF;
    if (Tx > 0 && Ty > 0 && peak_defined(pk)) key = res[b];
    const bool ok = key != DT_INF;
    const long long c = ok ? (long long)(key >> DT_NBITS) : 0;
    const int n = ok ? (int)(key & ((1u << DT_NBITS) - 1u)) : 0, e = peak_exp(pk);
    if (total != nullptr) total[b] = c;
    if (info != nullptr) {
        int32_t* o = info + (long)b * SWC_DTW_INFO;
        o[0] = n;
        o[1] = ok ? Tx : 0;
        o[2] = ok ? Ty : 0;
        o[3] = ok ? e : 0;
    }
    if (mean != nullptr) {
        double m = __builtin_nan("");
        if (ok && n > 0) m = ldexp(__ddiv_rn((double)c, (double)(16 * n)), e - SWC_DTW_QBITS);
        mean[b] = (float)m;
    }
}

// one thread per pair: from the end along the direction bits, cell k of the path at entry k
__global__ __launch_bounds__(64) void dtw_backtrack_kernel(const int32_t* __restrict__ tx, const int32_t* __restrict__ ty, int tmax_x,
                                                           int tmax_y, const unsigned* __restrict__ peaks, const u64* __restrict__ res,
                                                           const unsigned* __restrict__ dirs, long dir_ld, int32_t* __restrict__ path,
                                                           long ldp, int B) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int Tx = clamp_frames(tx, b, tmax_x), Ty = clamp_frames(ty, b, tmax_y);
    if (Tx <= 0 || Ty <= 0 || !peak_defined(peaks[b])) return;
    const u64 key = res[b];
    if (key == DT_INF) return;
    const int n = (int)(key & ((1u << DT_NBITS) - 1u));  // <= Tx + Ty - 1 <= ldp
    int i = Tx - 1, j = Ty - 1;
    int32_t* o = path + (long)b * ldp * 2;
    for (int k = n - 1; k >= 0 && k < Tx + Ty - 1 && i >= 0 && j >= 0; --k) {
        o[2 * k] = i;
        o[2 * k + 1] = j;
        const unsigned dir = (dirs[((long)b * tmax_x + i) * dir_ld + (j >> 4)] >> (2 * (j & 15))) & 3u;
        if (dir != 2u) --i;
        if (dir != 1u) --j;
    }
}

bool dtw_limits_ok(int B, int tmax_x, int tmax_y) {
    return B >= 0 && B <= 65535 && tmax_x >= 0 && tmax_x <= SWC_DTW_MAX_FRAMES && tmax_y >= 0 && tmax_y <= SWC_DTW_MAX_FRAMES;
}

// where swc_dtw keeps what inside its workspace (byte offsets): the peaks [B] u32 and the final keys [B] u64 (what the one
// memset clears), the quantised sides [B][Tmax][32] i16, the boundary keys [B][2][Tmax_y] u64 and, with a path, the
// directions [B][Tmax_x][dir_ld] u32
struct WsLayout {
    size_t peaks, res, xq, yq, bound, dirs, total;
    long dir_ld;
};

WsLayout ws_layout(int B, int tmax_x, int tmax_y, bool with_path) {
    WsLayout P;
    size_t o = 0;
    P.dir_ld = (tmax_y + 15) / 16;
    P.peaks = o; o += up256((size_t)B * sizeof(unsigned));
    P.res = o; o += up256((size_t)B * sizeof(u64));
    P.xq = o; o += up256((size_t)B * tmax_x * DT_QW * sizeof(unsigned));
    P.yq = o; o += up256((size_t)B * tmax_y * DT_QW * sizeof(unsigned));
    P.bound = o; o += up256((size_t)B * 2 * tmax_y * sizeof(u64));
    P.dirs = o; o += with_path ? up256((size_t)B * tmax_x * (size_t)P.dir_ld * sizeof(unsigned)) : 0;
    P.total = o;
    return P;
}

}  // namespace

extern "C" int64_t swc_cepstra_workspace_bytes(int32_t R, int64_t max_n_in, int32_t W, int32_t H) {
    return cepstra_frames(R, max_n_in, W, H) < 0 ? -1 : 0;
}

extern "C" int swc_cepstra(const void* const* rows, const int64_t* n_in, int64_t max_n_in, int32_t W, int32_t H, int32_t M,
                           const int32_t* fb_first, const int32_t* fb_count, const int32_t* fb_off, const float* fb_w,
                           int64_t fb_w_len, const float* dct, int32_t K, float* cep, int64_t ldf, int32_t* frames, void* workspace,
                           int64_t workspace_bytes, int32_t R, void* stream) {
    SWC_CHECK_ARG(rows && n_in && fb_first && fb_count && fb_off && fb_w && dct && cep && frames, "swc_cepstra: null pointer");
    SWC_CHECK_ARG(R >= 0 && R <= 65535, "swc_cepstra: R=%d (0..65535)", R);
    SWC_CHECK_ARG(max_n_in >= 0, "swc_cepstra: max_n_in=%ld out of range", (long)max_n_in);
    SWC_CHECK_ARG(valid_window(W), "swc_cepstra: window W=%d (a power of two, 32..2048)", W);
    SWC_CHECK_ARG(H >= 1 && H <= W, "swc_cepstra: hop H=%d (1..W=%d)", H, W);
    SWC_CHECK_ARG(M >= 1 && M <= W / 2 + 1, "swc_cepstra: n_mels M=%d (1..%d with W=%d)", M, W / 2 + 1, W);
    SWC_CHECK_ARG(fb_w_len >= 0 && fb_w_len < 0x7fffffffL, "swc_cepstra: fb_w_len=%ld out of range", (long)fb_w_len);
    SWC_CHECK_ARG(K >= 1 && K <= SWC_CEPSTRA_MAX_K, "swc_cepstra: K=%d coefficients (1..%d)", K, SWC_CEPSTRA_MAX_K);
    SWC_CHECK_ARG(ldf >= K, "swc_cepstra: ldf=%ld, K=%d coefficients", (long)ldf, K);
    const long t_max = cepstra_frames(R, max_n_in, W, H);
    SWC_CHECK_ARG(t_max >= 0, "swc_cepstra: max_n_in=%ld gives 2^31 frames or more at H=%d", (long)max_n_in, H);
    SWC_CHECK_ARG(workspace_bytes >= 0, "swc_cepstra: workspace of %ld bytes, 0 needed (swc_cepstra_workspace_bytes)",
                  (long)workspace_bytes);
    SWC_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "swc_cepstra: workspace must be 256-byte aligned");
    if (R == 0) return SWC_OK;
    hipStream_t st = (hipStream_t)stream;
    const long run = CP_RUN_SAMPLES / W;
    const dim3 grid((unsigned)((t_max + run - 1) / run), (unsigned)R);
#define SWC_CEPSTRA_CASE(WIN)                                                                                                     \
    case WIN:                                                                                                                     \
        launch_cepstra<WIN>(grid, st, rows, n_in, (long)max_n_in, H, M, fb_first, fb_count, fb_off, fb_w, (long)fb_w_len, dct, K, \
                            cep, (long)ldf, t_max, frames);                                                                       \
        break
    switch (W) {
        SWC_CEPSTRA_CASE(32);
        SWC_CEPSTRA_CASE(64);
        SWC_CEPSTRA_CASE(128);
        SWC_CEPSTRA_CASE(256);
        SWC_CEPSTRA_CASE(512);
        SWC_CEPSTRA_CASE(1024);
        SWC_CEPSTRA_CASE(2048);
    }
#undef SWC_CEPSTRA_CASE
    SWC_CHECK_LAUNCH("swc_cepstra (frames)");
    return SWC_OK;
}

extern "C" int64_t swc_dtw_workspace_bytes(int32_t B, int32_t Tmax_x, int32_t Tmax_y, int32_t with_path) {
    if (!dtw_limits_ok(B, Tmax_x, Tmax_y)) return -1;
    return (int64_t)ws_layout(B, Tmax_x, Tmax_y, with_path != 0).total;
}

extern "C" int swc_dtw(const float* xf, const float* yf, const int32_t* tx, const int32_t* ty, int32_t Tmax_x, int32_t Tmax_y,
                       int32_t D, int64_t ldf, int32_t band, int32_t mode, int64_t* total, int32_t* info, float* mean,
                       int32_t* path, int64_t ldp, void* workspace, int64_t workspace_bytes, int32_t B, void* stream) {
    SWC_CHECK_ARG(xf && yf && tx && ty && workspace, "swc_dtw: null pointer");
    SWC_CHECK_ARG(total || info || mean || path, "swc_dtw: no output (total, info, mean and path are all null)");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_dtw: B=%d (0..65535)", B);
    SWC_CHECK_ARG(Tmax_x >= 0 && Tmax_x <= SWC_DTW_MAX_FRAMES && Tmax_y >= 0 && Tmax_y <= SWC_DTW_MAX_FRAMES,
                  "swc_dtw: Tmax_x=%d, Tmax_y=%d frames out of range (0..%d)", Tmax_x, Tmax_y, SWC_DTW_MAX_FRAMES);
    SWC_CHECK_ARG(D >= 1 && D <= SWC_DTW_MAX_D, "swc_dtw: D=%d features (1..%d)", D, SWC_DTW_MAX_D);
    SWC_CHECK_ARG(ldf >= D, "swc_dtw: ldf=%ld, D=%d features", (long)ldf, D);
    SWC_CHECK_ARG(band >= 0, "swc_dtw: band r=%d (>= 0)", band);
    SWC_CHECK_ARG(mode == SWC_DTW_WARP || mode == SWC_DTW_DIAGONAL, "swc_dtw: mode=%d (0 warp, 1 diagonal)", mode);
    const bool work = Tmax_x > 0 && Tmax_y > 0;
    const long steps = work ? (long)Tmax_x + Tmax_y - 1 : 0;
    SWC_CHECK_ARG(path == nullptr || ldp >= steps, "swc_dtw: ldp=%ld, a path has up to %ld cells", (long)ldp, steps);
    const WsLayout P = ws_layout(B, Tmax_x, Tmax_y, path != nullptr);
    SWC_CHECK_ARG(workspace_bytes >= (int64_t)P.total, "swc_dtw: workspace of %ld bytes, %ld needed (swc_dtw_workspace_bytes)",
                  (long)workspace_bytes, (long)P.total);
    SWC_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "swc_dtw: workspace must be 256-byte aligned");
    if (B == 0) return SWC_OK;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* base = reinterpret_cast<unsigned char*>(workspace);
    unsigned* peaks = reinterpret_cast<unsigned*>(base + P.peaks);
    u64* res = reinterpret_cast<u64*>(base + P.res);
    unsigned* xq = reinterpret_cast<unsigned*>(base + P.xq);
    unsigned* yq = reinterpret_cast<unsigned*>(base + P.yq);
    u64* bound = reinterpret_cast<u64*>(base + P.bound);
    unsigned* dirs = path != nullptr ? reinterpret_cast<unsigned*>(base + P.dirs) : nullptr;
    if (hipMemsetAsync(workspace, 0, P.xq, st) != hipSuccess) {  // the peaks and the final keys
        (void)hipGetLastError();
        swc_set_error("swc_dtw: clearing the peaks failed");
        return SWC_E_LAUNCH;
    }
    if (work) {
        const int t_big = Tmax_x > Tmax_y ? Tmax_x : Tmax_y;
        const dim3 grid((unsigned)((t_big + DT_PK_FRAMES - 1) / DT_PK_FRAMES), (unsigned)B, 2u);
        hipLaunchKernelGGL(dtw_peak_kernel, grid, dim3(DT_THREADS), 0, st, xf, yf, tx, ty, Tmax_x, Tmax_y, D, (long)ldf, peaks);
        SWC_CHECK_LAUNCH("swc_dtw (peak)");
        hipLaunchKernelGGL(dtw_quant_kernel, grid, dim3(DT_THREADS), 0, st, xf, yf, tx, ty, Tmax_x, Tmax_y, D, (long)ldf,
                           (const unsigned*)peaks, xq, yq);
        SWC_CHECK_LAUNCH("swc_dtw (quantise)");
        const uint4* xq4 = reinterpret_cast<const uint4*>(xq);
        const uint4* yq4 = reinterpret_cast<const uint4*>(yq);
        const int groups = (D + 7) / 8;
#define SWC_DTW_CASE(GR)                                                                                                         \
    case GR:                                                                                                                     \
        if (mode == SWC_DTW_WARP)                                                                                                \
            hipLaunchKernelGGL(dtw_dp_kernel<GR>, dim3((unsigned)B), dim3(DT_THREADS), 0, st, tx, ty, Tmax_x, Tmax_y, band,      \
                               (const unsigned*)peaks, xq4, yq4, bound, dirs, P.dir_ld, res);                                    \
        else                                                                                                                     \
            hipLaunchKernelGGL(dtw_diag_kernel<GR>, dim3((unsigned)B), dim3(DT_THREADS), 0, st, tx, ty, Tmax_x, Tmax_y,          \
                               (const unsigned*)peaks, xq4, yq4, path, (long)ldp, res);                                          \
        break
        switch (groups) {
            SWC_DTW_CASE(1);
            SWC_DTW_CASE(2);
            SWC_DTW_CASE(3);
            SWC_DTW_CASE(4);
        }
#undef SWC_DTW_CASE
        SWC_CHECK_LAUNCH(mode == SWC_DTW_WARP ? "swc_dtw (recurrence)" : "swc_dtw (diagonal)");
        if (path != nullptr && mode == SWC_DTW_WARP) {
            hipLaunchKernelGGL(dtw_backtrack_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, tx, ty, Tmax_x, Tmax_y,
                               (const unsigned*)peaks, (const u64*)res, (const unsigned*)dirs, P.dir_ld, path, (long)ldp, B);
            SWC_CHECK_LAUNCH("swc_dtw (backtrack)");
        }
    }
    if (total != nullptr || info != nullptr || mean != nullptr) {
        hipLaunchKernelGGL(dtw_finish_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, tx, ty, Tmax_x, Tmax_y,
                           (const unsigned*)peaks, (const u64*)res, total, info, mean, B);
        SWC_CHECK_LAUNCH("swc_dtw (finish)");
    }
    return SWC_OK;
}
