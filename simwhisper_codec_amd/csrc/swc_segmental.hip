// swc_segmental (include/swc_segmental.h): LLR, Itakura-Saito, LPC cepstral distance, segmental SNR and frequency-weighted
// segmental SNR of a ragged batch of pairs.  Three kinds of launch, no workgroup waits for another:
//   segmental_frames_kernel<W>  a workgroup of 256 threads takes one run of 32768 / W consecutive frames of one pair, a team of
//                               min(W / 2, 256) threads owns a frame (the geometry of swc_frame_fft.h).  The team forms v_x
//                               and v_y in LDS, then the 2 (P + 1) + 1 sums of the frame, each in the header's four parts: one
//                               thread per (sum, part), sequential in i, the parts added in order by one thread per sum.  With a
//                               band table the two magnitudes come from frame_magnitudes<W, 2> and the bands from mel_band,
//                               unchanged; a thread per band forms u_j and u_j (35 - s_j), one thread adds them in band order.
//                               The frame's record (R_x, R_y, D, fw_t) goes to the workspace.  What a frame computes does not
//                               depend on its place in the run or on the run's place in the row.
//   segmental_lpc_kernel        the serial part, one lane per frame, all frames of the batch in parallel: two Levinson
//                               recursions, three quadratic forms, two cepstra, SegSNR.  Five float64 per frame to the workspace.
//   segmental_finish_kernel     one workgroup per row: the counts, the exact radix selection of v* for llr and cd (one bit per
//                               pass on the float64 bit patterns, as loud_gate_kernel), the fixed-order means (tiles of 256
//                               frames loaded in parallel, added in frame order by one thread per measure), `vals`, `track`.
// The file is compiled with -ffp-contract=off (build.py): the header fixes the rounding of every float64 operation.
#include "swc_frame_fft.h"
#include "swc_segmental.h"

namespace {

constexpr int SG_THREADS = FR_THREADS;
constexpr int SG_MAXP = SWC_SEGMENTAL_MAX_ORDER, SG_MAXK = SWC_SEGMENTAL_MAX_BANDS;
constexpr int SG_MAXSUMS = 2 * (SG_MAXP + 1) + 1;               // R_x[0 .. P], R_y[0 .. P], D
constexpr unsigned long long SG_OUT = ~0ull;                     // a frame left out of a measure: no computed NaN has this pattern
constexpr int SG_LPC_THREADS = 64, SG_FIN_THREADS = 256;

__device__ __forceinline__ double lo_clamp(double v, double c) { return v < c ? c : v; }  // NaN stays NaN
__device__ __forceinline__ double hi_clamp(double v, double c) { return v > c ? c : v; }
__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double out64() { return __longlong_as_double((long long)SG_OUT); }
__device__ __forceinline__ unsigned long long key_of(double v) { return (unsigned long long)__double_as_longlong(v); }

__device__ __forceinline__ long frames_of(long n, int W) { return n >= W ? 1 + (n - W) / (W / 4) : 0; }

// record of a frame: R_x[0 .. P], R_y[0 .. P] (uncorrected), D, fw_t
__host__ __device__ __forceinline__ int rec_len(int P) { return 2 * (P + 1) + 2; }

template <int W>
__global__ __launch_bounds__(SG_THREADS) void segmental_frames_kernel(
    const void* const* __restrict__ x_rows, const void* const* __restrict__ y_rows, const int64_t* __restrict__ n_in, long max_n,
    int P, int K, const int32_t* __restrict__ fb_first, const int32_t* __restrict__ fb_count, const int32_t* __restrict__ fb_off,
    const float* __restrict__ fb_w, long fb_w_len, double* __restrict__ rec, long ld_frames) {
    using G = FrameGeo<W>;
    constexpr int N = G::N, F = G::F, H = W / 4, Q = W / 4, TS = G::TS, TEAMS = G::TEAMS, R = G::R;
    __shared__ float2 s_tw[N];
    __shared__ float s_win[W];
    __shared__ float2 s_z[TEAMS][2][N];
    __shared__ float s_mag[TEAMS][2][F + 1];
    __shared__ float s_v[TEAMS][2][W];                 // v_x, v_y of the team's frame
    __shared__ double s_part[TEAMS][SG_MAXSUMS][4];    // the four parts of every sum
    __shared__ float s_band[TEAMS][2][SG_MAXK];        // Ex, Ey
    __shared__ double s_u[TEAMS][SG_MAXK], s_us[TEAMS][SG_MAXK];
    const int b = blockIdx.y, tid = threadIdx.x, team = tid / TS, lt = tid % TS;
    const long n = clamp_len(n_in, b, max_n);
    const long T = frames_of(n, W), t0 = (long)blockIdx.x * R;
    if (t0 >= T) return;  // (uniform over the workgroup; an empty row's addresses are not read)
    const int nfr = (int)(T - t0 < R ? T - t0 : R);
    const float* rows[2] = {reinterpret_cast<const float*>(x_rows[b]), reinterpret_cast<const float*>(y_rows[b])};
    if (K > 0) {
        frame_tables<W>(s_tw, s_win, tid);
    } else {
        for (int i = tid; i < W; i += SG_THREADS) s_win[i] = (float)(0.5 - 0.5 * cospi(2.0 * (double)i / (double)W));
        __syncthreads();
    }
    const int nsums = 2 * (P + 1) + 1, RL = rec_len(P);

    for (int pass = 0; pass * TEAMS < nfr; ++pass) {  // (uniform: every team takes part in every barrier)
        const int r = pass * TEAMS + team;
        const bool active = r < nfr;                   // a team past the row's last frame stores nothing
        const long start = (t0 + r) * H;               // the frame's first sample; start + W <= n for an active team
        double* out = rec + ((long)b * ld_frames + (t0 + r)) * RL;
        if (active) {
            for (int i = lt; i < 2 * W; i += TS) {
                const int sig = i / W, k = i % W;
                s_v[team][sig][k] = rows[sig][start + k] * s_win[k];
            }
        }
        __syncthreads();
        if (active) {
            const float* vx = s_v[team][0];
            const float* vy = s_v[team][1];
            for (int j = lt; j < 4 * nsums; j += TS) {
                const int q = j >> 2, c = j & 3;
                double acc = 0.0;
                if (q < 2 * (P + 1)) {
                    const int sig = q / (P + 1), k = q % (P + 1);
                    const float* v = sig == 0 ? vx : vy;
                    const int L = W - k, i0 = c * Q, i1 = (c + 1) * Q < L ? (c + 1) * Q : L;
                    for (int i = i0; i < i1; ++i) acc = acc + (double)v[i] * (double)v[i + k];
                } else {
                    for (int i = c * Q; i < (c + 1) * Q; ++i) {
                        const double d = (double)vx[i] - (double)vy[i];
                        acc = acc + d * d;
                    }
                }
                s_part[team][q][c] = acc;
            }
        }
        __syncthreads();
        if (active) {
            for (int q = lt; q < nsums; q += TS) {
                const double* p = s_part[team][q];
                out[q] = ((p[0] + p[1]) + p[2]) + p[3];
            }
        }
        if (K > 0) {  // (uniform)
            frame_magnitudes<W, 2>(rows, n, start, active, lt, s_tw, s_win, s_z[team], s_mag[team]);
            for (int m = lt; m < K; m += TS) {
                float a[2];
                mel_band<F, 2>(fb_first[m], fb_count[m], fb_off[m], fb_w, fb_w_len, s_mag[team], a);
                s_band[team][0][m] = a[0];
                s_band[team][1][m] = a[1];
            }
            __syncthreads();
            double emax = 0.0;
            for (int j = 0; j < K; ++j) {
                const double e = (double)s_band[team][0][j];
                emax = (e > emax || e != e) ? e : emax;  // a NaN band wins and stays
            }
            for (int m = lt; m < K; m += TS) {
                const double ex = (double)s_band[team][0][m], ey = (double)s_band[team][1][m];
                const double u = pow(ex / emax, 0.2), d = ex - ey;
                double s;
                if (ex == 0.0) s = -10.0;
                else if (d == 0.0) s = 35.0;
                else s = hi_clamp(lo_clamp(10.0 * log10((ex * ex) / (d * d)), -10.0), 35.0);
                s_u[team][m] = u;
                s_us[team][m] = u * (35.0 - s);
            }
            __syncthreads();
            if (active && lt == 0) {
                double fw = out64();
                if (emax != 0.0) {
                    double su = 0.0, sus = 0.0;
                    for (int j = 0; j < K; ++j) {
                        su = su + s_u[team][j];
                        sus = sus + s_us[team][j];
                    }
                    fw = 35.0 - sus / su;
                }
                out[nsums] = fw;
            }
        } else if (active && lt == 0) {
            out[nsums] = out64();
        }
        __syncthreads();  // s_v, s_part, s_band, s_u are free again
    }
}

// a = (1, a_1 .. a_P) from R (corrected R[0]): the recursion of the header, the update of a done in place from both ends
__device__ __forceinline__ void levinson(const double* R, double* a, int P) {
    double E = R[0];
    a[0] = 1.0;
    for (int m = 1; m <= P; ++m) {
        double acc = R[m];
        for (int i = 1; i < m; ++i) acc = acc + a[i] * R[m - i];
        const double k = -acc / E;
        for (int i = 1; i <= m - i; ++i) {  // the pairs (i, m - i), the middle one once
            const double u = a[i], v = a[m - i];
            a[i] = u + k * v;
            if (i != m - i) a[m - i] = v + k * u;
        }
        a[m] = k;
        E = E * (1.0 - k * k);
    }
}

__device__ __forceinline__ double quad_form(const double* a, const double* R, int P) {
    double q = 0.0;
    for (int i = 0; i <= P; ++i) {
        double s = 0.0;
        for (int j = 0; j <= P; ++j) s = s + R[i > j ? i - j : j - i] * a[j];
        q = q + a[i] * s;
    }
    return q;
}

__device__ __forceinline__ void lpc_cepstrum(const double* a, double* c, int P) {
    for (int m = 1; m <= P; ++m) {
        double acc = -a[m];
        for (int k = 1; k < m; ++k) acc = acc + (((double)k / (double)m) * c[k]) * (-a[m - k]);
        c[m] = acc;
    }
}

__global__ __launch_bounds__(SG_LPC_THREADS) void segmental_lpc_kernel(const int64_t* __restrict__ n_in, long max_n, int W, int P,
                                                                      const double* __restrict__ rec, double* __restrict__ fv,
                                                                      long ld_frames) {
    const int b = blockIdx.y;
    const long t = (long)blockIdx.x * SG_LPC_THREADS + threadIdx.x;
    const long T = frames_of(clamp_len(n_in, b, max_n), W);
    if (t >= T) return;
    const double* r = rec + ((long)b * ld_frames + t) * rec_len(P);
    double Rx[SG_MAXP + 1], Ry[SG_MAXP + 1], ax[SG_MAXP + 1], ay[SG_MAXP + 1], cx[SG_MAXP + 1], cy[SG_MAXP + 1];
    for (int k = 0; k <= P; ++k) {
        Rx[k] = r[k];
        Ry[k] = r[P + 1 + k];
    }
    const double S = Rx[0], D = r[2 * (P + 1)], fw = r[2 * (P + 1) + 1];
    double seg;
    if (S == 0.0) seg = -10.0;
    else if (D == 0.0) seg = 35.0;
    else seg = hi_clamp(lo_clamp(10.0 * log10(S / D), -10.0), 35.0);
    double llr = out64(), is = out64(), cd = out64();
    if (Rx[0] > 0.0 && Ry[0] > 0.0) {
        const double corr = 1.0 + 1.0 / 1048576.0;
        Rx[0] = Rx[0] * corr;
        Ry[0] = Ry[0] * corr;
        levinson(Rx, ax, P);
        levinson(Ry, ay, P);
        const double num = quad_form(ay, Rx, P), den = quad_form(ax, Rx, P), gy = quad_form(ay, Ry, P);
        llr = hi_clamp(lo_clamp(log(num / den), 0.0), 2.0);
        is = hi_clamp(((den / gy) * (num / den) + log(gy / den)) - 1.0, 100.0);
        lpc_cepstrum(ax, cx, P);
        lpc_cepstrum(ay, cy, P);
        double acc = 0.0;
        for (int m = 1; m <= P; ++m) {
            const double d = cx[m] - cy[m];
            acc = acc + d * d;
        }
        cd = hi_clamp(4.342944819032518 * sqrt(2.0 * acc), 10.0);
    }
    double* o = fv + ((long)b * ld_frames + t) * SWC_SEGMENTAL_MEASURES;
    o[0] = llr;
    o[1] = is;
    o[2] = cd;
    o[3] = seg;
    o[4] = fw;
}

// the key of rank `rank` (0 = smallest) among measure `col` of the T frames of this row that are not left out: exact radix
// selection, one bit per pass from the top (select_rank of swc_loudness.hip on strided keys)
__device__ unsigned long long select_key(const double* __restrict__ fv, long T, int col, long rank, unsigned* cnt_sh, int tid) {
    unsigned long long prefix = 0ull;
    for (int bit = 63; bit >= 0; --bit) {
        __syncthreads();
        if (tid == 0) *cnt_sh = 0u;
        __syncthreads();
        unsigned c = 0u;
        for (long t = tid; t < T; t += SG_FIN_THREADS) {
            const unsigned long long k = key_of(fv[t * SWC_SEGMENTAL_MEASURES + col]);
            c += (k != SG_OUT && ((k ^ prefix) >> bit) == 0ull) ? 1u : 0u;  // high bits match, this bit 0
        }
        if (c) atomicAdd(cnt_sh, c);
        __syncthreads();
        const long zeros = (long)*cnt_sh;
        if (rank >= zeros) {
            rank -= zeros;
            prefix |= 1ull << bit;
        }
    }
    return prefix;
}

__global__ __launch_bounds__(SG_FIN_THREADS) void segmental_finish_kernel(const int64_t* __restrict__ n_in, long max_n, int W,
                                                                         const double* __restrict__ fv_all, long ld_frames,
                                                                         double* __restrict__ vals, double* __restrict__ track,
                                                                         long ld_t) {
    __shared__ double tile[SG_FIN_THREADS][SWC_SEGMENTAL_MEASURES];
    __shared__ unsigned cnt_sh, cnt_lpc, cnt_fw;
    const int b = blockIdx.x, tid = threadIdx.x;
    const long T = frames_of(clamp_len(n_in, b, max_n), W);
    const double* fv = fv_all + (long)b * ld_frames * SWC_SEGMENTAL_MEASURES;
    if (tid == 0) {
        cnt_lpc = 0u;
        cnt_fw = 0u;
    }
    __syncthreads();
    unsigned c_lpc = 0u, c_fw = 0u;
    for (long t = tid; t < T; t += SG_FIN_THREADS) {
        c_lpc += key_of(fv[t * SWC_SEGMENTAL_MEASURES + 0]) != SG_OUT ? 1u : 0u;
        c_fw += key_of(fv[t * SWC_SEGMENTAL_MEASURES + 4]) != SG_OUT ? 1u : 0u;
    }
    if (c_lpc) atomicAdd(&cnt_lpc, c_lpc);
    if (c_fw) atomicAdd(&cnt_fw, c_fw);
    __syncthreads();
    const long T_lpc = (long)cnt_lpc, T_fw = (long)cnt_fw;
    const long K95 = (19 * T_lpc + 10) / 20;
    unsigned long long star[2] = {0ull, 0ull};  // v* of llr and of cd
    if (T_lpc > 0) {  // (uniform over the workgroup)
        star[0] = select_key(fv, T, 0, K95 - 1, &cnt_sh, tid);
        star[1] = select_key(fv, T, 2, K95 - 1, &cnt_sh, tid);
    }
    // the means: tiles of 256 frames loaded in parallel, added in frame order by thread k for measure k
    double sum = 0.0;
    long below = 0;
    bool bad = false;
    double* tr = track != nullptr ? track + (long)b * ld_t * SWC_SEGMENTAL_MEASURES : nullptr;
    for (long t0 = 0; t0 < T; t0 += SG_FIN_THREADS) {
        const long t = t0 + tid;
        __syncthreads();
        if (t < T) {
#pragma unroll
            for (int k = 0; k < SWC_SEGMENTAL_MEASURES; ++k) {
                const double v = fv[t * SWC_SEGMENTAL_MEASURES + k];
                tile[tid][k] = v;
                if (tr != nullptr && t < ld_t) tr[t * SWC_SEGMENTAL_MEASURES + k] = key_of(v) == SG_OUT ? nan64() : v;
            }
        }
        __syncthreads();
        if (tid < SWC_SEGMENTAL_MEASURES) {
            const int m = (int)(T - t0 < SG_FIN_THREADS ? T - t0 : SG_FIN_THREADS);
            for (int i = 0; i < m; ++i) {
                const double v = tile[i][tid];
                const unsigned long long k = key_of(v);
                if (k == SG_OUT) continue;
                if (tid == 0 || tid == 2) {
                    if (v != v) bad = true;
                    else if (k < star[tid >> 1]) {
                        sum = sum + v;
                        below += 1;
                    }
                } else {
                    sum = sum + v;
                }
            }
        }
    }
    double* o = vals + (long)b * SWC_SEGMENTAL_VALUES;
    if (tid == 0 || tid == 2) {
        const double vs = __longlong_as_double((long long)star[tid >> 1]);
        o[tid] = (T_lpc == 0 || bad) ? nan64() : (sum + (double)(K95 - below) * vs) / (double)K95;
    } else if (tid == 1) {
        o[1] = T_lpc > 0 ? sum / (double)T_lpc : nan64();
    } else if (tid == 3) {
        o[3] = T > 0 ? sum / (double)T : nan64();
    } else if (tid == 4) {
        o[4] = T_fw > 0 ? sum / (double)T_fw : nan64();
    } else if (tid == 5) {
        o[5] = (double)T;
    } else if (tid == 6) {
        o[6] = (double)T_lpc;
    } else if (tid == 7) {
        o[7] = (double)T_fw;
    }
}

bool valid_segmental_window(int w) { return w >= SWC_SEGMENTAL_MIN_WIN && w <= SWC_SEGMENTAL_MAX_WIN && (w & (w - 1)) == 0; }

// frames of a row of max_n samples, or -1 when the parameters are refused or the count does not fit 31 bits
long max_frames(long max_n, int W, int P, int K) {
    if (max_n < 0 || !valid_segmental_window(W) || P < 1 || P > SG_MAXP || K < 0 || K > SG_MAXK) return -1;
    const long T = max_n >= W ? 1 + (max_n - W) / (W / 4) : 0;
    return T >= 0x7fffffffL ? -1 : T;
}

struct SgLayout {
    size_t rec, fv, total;
};

SgLayout sg_layout(int B, long Tm, int P) {
    SgLayout L;
    L.rec = 0;
    L.fv = up256((size_t)B * (size_t)Tm * (size_t)rec_len(P) * sizeof(double));
    L.total = L.fv + up256((size_t)B * (size_t)Tm * SWC_SEGMENTAL_MEASURES * sizeof(double));
    return L;
}

template <int W>
void launch_segmental_frames(dim3 grid, hipStream_t st, const void* const* x_rows, const void* const* y_rows, const int64_t* n_in,
                             long max_n, int P, int K, const int32_t* fb_first, const int32_t* fb_count, const int32_t* fb_off,
                             const float* fb_w, long fb_w_len, double* rec, long ld_frames) {
    hipLaunchKernelGGL(segmental_frames_kernel<W>, grid, dim3(SG_THREADS), 0, st, x_rows, y_rows, n_in, max_n, P, K, fb_first,
                       fb_count, fb_off, fb_w, fb_w_len, rec, ld_frames);
}

}  // namespace

extern "C" int64_t swc_segmental_workspace_bytes(int32_t B, int64_t max_n_in, int32_t W, int32_t P, int32_t K) {
    if (B < 0 || B > 65535) return -1;
    const long Tm = max_frames(max_n_in, W, P, K);
    if (Tm < 0) return -1;
    return (int64_t)sg_layout(B, Tm, P).total;
}

extern "C" int swc_segmental(const void* const* x_rows, const void* const* y_rows, const int64_t* n_in, int64_t max_n_in, int32_t W,
                             int32_t P, int32_t K, const int32_t* fb_first, const int32_t* fb_count, const int32_t* fb_off,
                             const float* fb_w, int64_t fb_w_len, double* vals, double* track, int64_t ld_t, void* workspace,
                             int64_t workspace_bytes, int32_t B, void* stream) {
    SWC_CHECK_ARG(x_rows && y_rows && n_in && vals && workspace, "swc_segmental: null pointer");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_segmental: B=%d (0..65535)", B);
    SWC_CHECK_ARG(max_n_in >= 0, "swc_segmental: max_n_in=%ld out of range", (long)max_n_in);
    SWC_CHECK_ARG(valid_segmental_window(W), "swc_segmental: window W=%d (a power of two, %d..%d)", W, SWC_SEGMENTAL_MIN_WIN,
                  SWC_SEGMENTAL_MAX_WIN);
    SWC_CHECK_ARG(P >= 1 && P <= SG_MAXP, "swc_segmental: order P=%d (1..%d)", P, SG_MAXP);
    SWC_CHECK_ARG(K >= 0 && K <= SG_MAXK, "swc_segmental: bands K=%d (0..%d)", K, SG_MAXK);
    SWC_CHECK_ARG(fb_w_len >= 0 && fb_w_len < 0x7fffffffL, "swc_segmental: fb_w_len=%ld out of range", (long)fb_w_len);
    SWC_CHECK_ARG(track == nullptr || ld_t >= 0, "swc_segmental: ld_t=%ld out of range", (long)ld_t);
    const long Tm = max_frames(max_n_in, W, P, K);
    SWC_CHECK_ARG(Tm >= 0, "swc_segmental: max_n_in=%ld gives 2^31 frames or more at W=%d", (long)max_n_in, W);
    const SgLayout L = sg_layout(B, Tm, P);
    SWC_CHECK_ARG(workspace_bytes >= (int64_t)L.total, "swc_segmental: workspace of %ld bytes, %ld needed (swc_segmental_workspace_bytes)",
                  (long)workspace_bytes, (long)L.total);
    SWC_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "swc_segmental: workspace must be 256-byte aligned");
    if (B == 0) return SWC_OK;
    hipStream_t st = (hipStream_t)stream;
    const int Keff = (fb_first && fb_count && fb_off && fb_w) ? K : 0;
    double* rec = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + L.rec);
    double* fv = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + L.fv);
    const long max_n = max_n_in;
    if (Tm > 0) {
        const long R = FR_RUN_SAMPLES / W;
        const dim3 grid((unsigned)((Tm + R - 1) / R), (unsigned)B);
#define SWC_SEGMENTAL_CASE(WIN)                                                                                                \
    case WIN:                                                                                                                  \
        launch_segmental_frames<WIN>(grid, st, x_rows, y_rows, n_in, max_n, P, Keff, fb_first, fb_count, fb_off, fb_w,         \
                                     (long)fb_w_len, rec, Tm);                                                                 \
        break
        switch (W) {
            SWC_SEGMENTAL_CASE(64);
            SWC_SEGMENTAL_CASE(128);
            SWC_SEGMENTAL_CASE(256);
            SWC_SEGMENTAL_CASE(512);
            SWC_SEGMENTAL_CASE(1024);
            SWC_SEGMENTAL_CASE(2048);
        }
#undef SWC_SEGMENTAL_CASE
        SWC_CHECK_LAUNCH("swc_segmental (frames)");
        const dim3 lgrid((unsigned)((Tm + SG_LPC_THREADS - 1) / SG_LPC_THREADS), (unsigned)B);
        hipLaunchKernelGGL(segmental_lpc_kernel, lgrid, dim3(SG_LPC_THREADS), 0, st, n_in, max_n, (int)W, (int)P, (const double*)rec, fv, Tm);
        SWC_CHECK_LAUNCH("swc_segmental (lpc)");
    }
    hipLaunchKernelGGL(segmental_finish_kernel, dim3((unsigned)B), dim3(SG_FIN_THREADS), 0, st, n_in, max_n, (int)W, (const double*)fv, Tm,
                       vals, track, (long)ld_t);
    SWC_CHECK_LAUNCH("swc_segmental (finish)");
    return SWC_OK;
}
