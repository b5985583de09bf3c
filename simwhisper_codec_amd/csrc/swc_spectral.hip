// swc_spectral (include/swc_spectral.h): multi-scale mel, multi-resolution STFT and log-spectral distance of a ragged batch
// of pairs.  Two kinds of launch, no workgroup waits for another:
//   spectral_frames_kernel<W>  one per scale with work.  A workgroup of 256 threads takes one run of SWC_SPECTRAL_RUN_<W>
//                              consecutive frames of one row, a team of min(W / 2, 256) threads owns a frame; the magnitudes
//                              of the frame's two signals come from swc_frame_fft.h (geometry, tables, FFT in LDS, mel band:
//                              shared with swc_mcd.hip).  At W = 256 alone the load, FFT and unpack stay written out here:
//                              through the header the same instructions are scheduled differently there and that scale takes
//                              0.023 ms (4.9 %) longer; the other six windows do not change (profiles/frame_fft_ab.txt).  A
//                              change to frame_magnitudes is made in that copy too; tests/test_frame_bits_gpu.py holds both to
//                              their bits.  The magnitudes are reduced to four f32 sums in a fixed order.  What a frame
//                              computes does not depend on its place in the run: its four sums go to an LDS slot of their
//                              own, and four threads add the slots in frame order in float64 into the record of the run.
//   spectral_finish_kernel     one workgroup per row adds the run records of every scale in ascending order in float64 (loads
//                              in parallel, adds in order, as sisdr_finish_kernel), divides, sums the scales and rounds once.
#include "swc_frame_fft.h"

namespace {

constexpr int SP_THREADS = FR_THREADS;
constexpr int SP_RUN_SAMPLES = FR_RUN_SAMPLES;  // W * SWC_SPECTRAL_RUN_<W>
constexpr float SP_CLAMP = 1e-5f;
static_assert(SWC_SPECTRAL_RUN_32 * 32 == SP_RUN_SAMPLES && SWC_SPECTRAL_RUN_64 * 64 == SP_RUN_SAMPLES &&
                  SWC_SPECTRAL_RUN_128 * 128 == SP_RUN_SAMPLES && SWC_SPECTRAL_RUN_256 * 256 == SP_RUN_SAMPLES &&
                  SWC_SPECTRAL_RUN_512 * 512 == SP_RUN_SAMPLES && SWC_SPECTRAL_RUN_1024 * 1024 == SP_RUN_SAMPLES &&
                  SWC_SPECTRAL_RUN_2048 * 2048 == SP_RUN_SAMPLES,
              "every run length is 32768 / W");

// what the finish kernel needs to know about the scales (passed by value)
struct Scales {
    int n;
    int W[SWC_SPECTRAL_MAX_SCALES], M[SWC_SPECTRAL_MAX_SCALES], flags[SWC_SPECTRAL_MAX_SCALES], eff[SWC_SPECTRAL_MAX_SCALES];
    long runs[SWC_SPECTRAL_MAX_SCALES];     // records per row
    long rec_off[SWC_SPECTRAL_MAX_SCALES];  // in float64 elements from the workspace's start
};

__device__ __forceinline__ float clamp_floor(float v) { return v < SP_CLAMP ? SP_CLAMP : v; }  // NaN stays NaN

// the sum of v over the TS threads of a team, the same value in each of them, in one fixed order: an xor butterfly inside the
// wave, then the team's waves in ascending order through LDS.  Every thread of the workgroup calls it
template <int TS, int TW>
__device__ __forceinline__ void team_sum4(float (&v)[4], float (*red)[4], int lt) {
    constexpr int inwave = TS < 64 ? TS : 64;
#pragma unroll
    for (int o = inwave / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += __shfl_xor(v[k], o);
    }
    if (TW > 1) {
        if ((lt & 63) == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) red[lt >> 6][k] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float s = red[0][k];
#pragma unroll
            for (int w = 1; w < TW; ++w) s += red[w][k];
            v[k] = s;
        }
    }
}

template <int W>
__global__ __launch_bounds__(SP_THREADS) void spectral_frames_kernel(
    const void* const* __restrict__ x_rows, const void* const* __restrict__ y_rows, const int64_t* __restrict__ n_in, long max_n,
    int eff, int M, int fb_base, const int32_t* __restrict__ fb_first, const int32_t* __restrict__ fb_count,
    const int32_t* __restrict__ fb_off, const float* __restrict__ fb_w, long fb_w_len, double* __restrict__ rec, long runs) {
    using G = FrameGeo<W>;
    constexpr int N = G::N, F = G::F, H = W / 4, TS = G::TS, TEAMS = G::TEAMS, TW = G::TW, R = G::R, LOGN = G::LOGN;
    __shared__ float2 s_tw[N];              // exp(-2 pi i q / W)
    __shared__ float s_win[W];
    __shared__ float2 s_z[TEAMS][2][N];     // [team][x, y]
    __shared__ float s_mag[TEAMS][2][F + 1];
    __shared__ float s_red[TEAMS][TW][4];
    __shared__ float s_frame[R][4];         // the four sums of every frame of the run
    const int b = blockIdx.y, tid = threadIdx.x, team = tid / TS, lt = tid % TS;
    const long n = clamp_len(n_in, b, max_n);
    if (n <= 0) return;  // an empty row: its addresses are not read (uniform over the workgroup)
    const long T = 1 + n / H, t0 = (long)blockIdx.x * R;
    if (t0 >= T) return;
    const int nfr = (int)(T - t0 < R ? T - t0 : R);
    const float* rows[2] = {reinterpret_cast<const float*>(x_rows[b]), reinterpret_cast<const float*>(y_rows[b])};
    frame_tables<W>(s_tw, s_win, tid);

    for (int pass = 0; pass * TEAMS < nfr; ++pass) {  // (uniform: every team takes part in every barrier)
        const int r = pass * TEAMS + team;
        const bool active = r < nfr;                  // a team past the row's last frame works on zeros and stores nothing
        const long start = (t0 + r) * H - N;          // the frame's first sample
        if constexpr (W != 256) {
            frame_magnitudes<W, 2>(rows, n, start, active, lt, s_tw, s_win, s_z[team], s_mag[team]);
        } else {  // frame_magnitudes<256, 2> written out: inlined from the header this one window is 4.9 % slower
            // the two windowed frames, packed z[k] = v[2 k] + i v[2 k + 1], stored where the in-place transform wants them
            for (int i = lt; i < 2 * N; i += TS) {
                const int sig = i / N, k = i % N;
                const long i0 = start + 2 * k;
                const float* p = rows[sig];
                const float v0 = (active && i0 >= 0 && i0 < n) ? p[i0] * s_win[2 * k] : 0.0f;
                const float v1 = (active && i0 + 1 >= 0 && i0 + 1 < n) ? p[i0 + 1] * s_win[2 * k + 1] : 0.0f;
                s_z[team][sig][__brev((unsigned)k) >> (32 - LOGN)] = make_float2(v0, v1);
            }
            __syncthreads();
#pragma unroll 1
            for (int lh = 0; lh < LOGN; ++lh) {
                const int h = 1 << lh;
                for (int i = lt; i < N; i += TS) {  // N / 2 butterflies of x, then N / 2 of y
                    const int sig = i / (N / 2), j = i % (N / 2);
                    const int k = j & (h - 1), a = ((j >> lh) << (lh + 1)) + k;
                    const float2 w = s_tw[k << (LOGN - lh)];  // exp(-2 pi i k / (2 h))
                    float2* z = s_z[team][sig];
                    const float2 u = z[a], v = z[a + h];
                    const float tr = w.x * v.x - w.y * v.y, ti = w.x * v.y + w.y * v.x;
                    z[a] = make_float2(u.x + tr, u.y + ti);
                    z[a + h] = make_float2(u.x - tr, u.y - ti);
                }
                __syncthreads();
            }
            // unpack: with A = Z[f], Bc = conj Z[N - f]: E = (A + Bc) / 2, O = -i (A - Bc) / 2, P = tw[f] O;
            // |X[f]| = |E + P|, |X[N - f]| = |E - P|, f = 0 .. N / 2
            for (int i = lt; i < 2 * (N / 2 + 1); i += TS) {
                const int sig = i / (N / 2 + 1), f = i % (N / 2 + 1);
                const float2* z = s_z[team][sig];
                const float2 A = z[f], B = z[(N - f) & (N - 1)], w = s_tw[f];
                const float er = 0.5f * (A.x + B.x), ei = 0.5f * (A.y - B.y);
                const float orr = 0.5f * (A.y + B.y), oi = -0.5f * (A.x - B.x);
                const float pr = w.x * orr - w.y * oi, pi = w.x * oi + w.y * orr;
                const float ar = er + pr, ai = ei + pi, br = er - pr, bi = ei - pi;
                s_mag[team][sig][f] = sqrtf(ar * ar + ai * ai);
                s_mag[team][sig][N - f] = sqrtf(br * br + bi * bi);
            }
            __syncthreads();
        }
        const float* mx = s_mag[team][0];
        const float* my = s_mag[team][1];
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // mel, log-magnitude L1, magnitude L1, squared log difference
        if (eff & (SWC_SPECTRAL_STFT | SWC_SPECTRAL_LSD)) {
            for (int f = lt; f < F; f += TS) {
                const float X = mx[f], Y = my[f];
                const float d = 2.0f * log10f(clamp_floor(X)) - 2.0f * log10f(clamp_floor(Y));
                v[1] += fabsf(d);
                v[2] += fabsf(X - Y);
                v[3] = fmaf(d, d, v[3]);
            }
        }
        if (eff & SWC_SPECTRAL_MEL) {
            for (int m = lt; m < M; m += TS) {
                float a[2];
                mel_band<F, 2>(fb_first[fb_base + m], fb_count[fb_base + m], fb_off[fb_base + m], fb_w, fb_w_len, s_mag[team], a);
                v[0] += fabsf(log10f(clamp_floor(a[0])) - log10f(clamp_floor(a[1])));
            }
        }
        team_sum4<TS, TW>(v, s_red[team], lt);
        if (active && lt == 0) {
            s_frame[r][0] = v[0];
            s_frame[r][1] = v[1];
            s_frame[r][2] = v[2];
            s_frame[r][3] = sqrtf(v[3] / (float)F);
        }
        __syncthreads();  // s_red and s_mag are free again
    }
    if (tid < 4) {
        double acc = 0.0;
        for (int r = 0; r < nfr; ++r) acc += (double)s_frame[r][tid];
        rec[((long)b * runs + blockIdx.x) * 4 + tid] = acc;
    }
}

// the records of row b, scale by scale, in ascending run order (64 at a time through LDS: the loads in parallel, the adds in
// order); then the means, the sums over the scales and one rounding per value
__global__ __launch_bounds__(64) void spectral_finish_kernel(const int64_t* __restrict__ n_in, long max_n,
                                                             const double* __restrict__ ws, Scales S, float* __restrict__ mel,
                                                             float* __restrict__ stft, float* __restrict__ lsd,
                                                             float* __restrict__ parts) {
    __shared__ double tile[64][4];
    __shared__ double tot[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long n = clamp_len(n_in, b, max_n);
    const float nan = __builtin_nanf("");
    double mel_sum = 0.0, stft_sum = 0.0, lsd_val = 0.0;
    for (int s = 0; s < S.n; ++s) {
        const int W = S.W[s], H = W / 4, F = W / 2 + 1, R = SP_RUN_SAMPLES / W;
        const long T = 1 + n / H;
        const long C = (n > 0 && S.eff[s] != 0) ? (T + R - 1) / R : 0;  // <= S.runs[s]: the records of this row that were written
        const double* r = ws + S.rec_off[s] + (long)b * S.runs[s] * 4;
        double acc = 0.0;
        for (long c0 = 0; c0 < C; c0 += 64) {
            const long c = c0 + tid;
            if (c < C) {
#pragma unroll
                for (int k = 0; k < 4; ++k) tile[tid][k] = r[c * 4 + k];
            }
            __syncthreads();
            if (tid < 4) {
                const int m = (int)(C - c0 < 64 ? C - c0 : 64);
                for (int i = 0; i < m; ++i) acc += tile[i][tid];
            }
            __syncthreads();
        }
        if (tid < 4) tot[tid] = acc;
        __syncthreads();
        if (tid == 0) {
            const int fl = S.flags[s], eff = S.eff[s];
            const double tf = (double)T * (double)F;
            const double mel_s = tot[0] / ((double)T * (double)S.M[s]), logmag_s = tot[1] / tf, mag_s = tot[2] / tf,
                         lsd_s = tot[3] / (double)T;
            if (eff & SWC_SPECTRAL_MEL) mel_sum += mel_s;
            if (eff & SWC_SPECTRAL_STFT) stft_sum += logmag_s + mag_s;
            if (eff & SWC_SPECTRAL_LSD) lsd_val = lsd_s;
            if (parts != nullptr) {  // (then eff == flags)
                float* p = parts + ((long)b * S.n + s) * 4;
                p[0] = (fl & SWC_SPECTRAL_MEL) ? (n > 0 ? (float)mel_s : nan) : 0.0f;
                p[1] = (fl & SWC_SPECTRAL_STFT) ? (n > 0 ? (float)logmag_s : nan) : 0.0f;
                p[2] = (fl & SWC_SPECTRAL_STFT) ? (n > 0 ? (float)mag_s : nan) : 0.0f;
                p[3] = (fl & SWC_SPECTRAL_LSD) ? (n > 0 ? (float)lsd_s : nan) : 0.0f;
            }
        }
        __syncthreads();  // tot is free again
    }
    if (tid != 0) return;
    if (mel != nullptr) mel[b] = n > 0 ? (float)mel_sum : nan;
    if (stft != nullptr) stft[b] = n > 0 ? (float)stft_sum : nan;
    if (lsd != nullptr) lsd[b] = n > 0 ? (float)lsd_val : nan;
}

// records per row of one scale, or -1 when its frame count does not fit 31 bits
long runs_of(long max_n, int W) {
    const long T = 1 + max_n / (W / 4);
    if (T >= 0x7fffffffL) return -1;
    const long R = SP_RUN_SAMPLES / W;
    return (T + R - 1) / R;
}

template <int W>
void launch_frames(dim3 grid, hipStream_t st, const void* const* x_rows, const void* const* y_rows, const int64_t* n_in, long max_n,
                   int eff, int M, int fb_base, const int32_t* fb_first, const int32_t* fb_count, const int32_t* fb_off,
                   const float* fb_w, long fb_w_len, double* rec, long runs) {
    hipLaunchKernelGGL(spectral_frames_kernel<W>, grid, dim3(SP_THREADS), 0, st, x_rows, y_rows, n_in, max_n, eff, M, fb_base,
                       fb_first, fb_count, fb_off, fb_w, fb_w_len, rec, runs);
}

// where swc_spectral keeps what inside its workspace: per scale the records per row and the byte offset of its
// [B][runs][4] f64 records.  A scale with a window that is not valid, or with too many frames, has runs -1 and takes no room.
struct WsLayout {
    long runs[SWC_SPECTRAL_MAX_SCALES];
    size_t rec[SWC_SPECTRAL_MAX_SCALES];
    size_t total;
    bool ok;  // every scale has a place
};

WsLayout ws_layout(int B, long max_n, const int32_t* win, int n_scales) {
    WsLayout P;
    P.total = 0;
    P.ok = true;
    for (int s = 0; s < n_scales; ++s) {
        P.runs[s] = valid_window(win[s]) ? runs_of(max_n, win[s]) : -1;
        P.rec[s] = P.total;
        if (P.runs[s] < 0) P.ok = false;
        else P.total += up256((size_t)B * (size_t)P.runs[s] * 4 * sizeof(double));
    }
    return P;
}

}  // namespace

extern "C" int64_t swc_spectral_workspace_bytes(int32_t B, int64_t max_n_in, const int32_t* win, int32_t n_scales) {
    if (B < 0 || B > 65535 || max_n_in < 0 || n_scales < 0 || n_scales > SWC_SPECTRAL_MAX_SCALES) return -1;
    if (n_scales > 0 && win == nullptr) return -1;
    const WsLayout P = ws_layout(B, max_n_in, win, n_scales);
    return P.ok ? (int64_t)P.total : -1;
}

extern "C" int swc_spectral(const void* const* x_rows, const void* const* y_rows, const int64_t* n_in, int64_t max_n_in,
                            const int32_t* win, const int32_t* n_mels, const int32_t* flags, int32_t n_scales,
                            const int32_t* fb_first, const int32_t* fb_count, const int32_t* fb_off, const float* fb_w,
                            int64_t fb_w_len, float* mel, float* stft, float* lsd, float* parts, void* workspace,
                            int64_t workspace_bytes, int32_t B, void* stream) {
    SWC_CHECK_ARG(x_rows && y_rows && n_in && workspace && win && n_mels && flags, "swc_spectral: null pointer");
    SWC_CHECK_ARG(mel || stft || lsd || parts, "swc_spectral: no output (mel, stft, lsd and parts are all null)");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_spectral: B=%d (0..65535)", B);
    SWC_CHECK_ARG(max_n_in >= 0, "swc_spectral: max_n_in=%ld out of range", (long)max_n_in);
    SWC_CHECK_ARG(n_scales >= 1 && n_scales <= SWC_SPECTRAL_MAX_SCALES, "swc_spectral: n_scales=%d (1..%d)", n_scales,
                  SWC_SPECTRAL_MAX_SCALES);
    Scales S;
    S.n = n_scales;
    int fb_base[SWC_SPECTRAL_MAX_SCALES];
    int n_lsd = 0, filters = 0;
    bool mel_work = false;
    const WsLayout P = ws_layout(B, max_n_in, win, n_scales);
    const int want = (mel ? SWC_SPECTRAL_MEL : 0) | (stft ? SWC_SPECTRAL_STFT : 0) | (lsd ? SWC_SPECTRAL_LSD : 0);
    for (int s = 0; s < n_scales; ++s) {
        const int W = win[s], F = W / 2 + 1;
        SWC_CHECK_ARG(valid_window(W), "swc_spectral: scale %d: window W=%d (a power of two, %d..%d)", s, W, SWC_SPECTRAL_MIN_WIN,
                      SWC_SPECTRAL_MAX_WIN);
        SWC_CHECK_ARG((flags[s] & ~(SWC_SPECTRAL_MEL | SWC_SPECTRAL_STFT | SWC_SPECTRAL_LSD)) == 0, "swc_spectral: scale %d: flags=%d",
                      s, flags[s]);
        SWC_CHECK_ARG(n_mels[s] >= 0 && n_mels[s] <= F && (!(flags[s] & SWC_SPECTRAL_MEL) || n_mels[s] >= 1),
                      "swc_spectral: scale %d: n_mels=%d (1..%d with W=%d when MEL is flagged)", s, n_mels[s], F, W);
        n_lsd += (flags[s] & SWC_SPECTRAL_LSD) ? 1 : 0;
        SWC_CHECK_ARG(P.runs[s] >= 0, "swc_spectral: max_n_in=%ld gives 2^31 frames or more at W=%d", (long)max_n_in, W);
        S.W[s] = W;
        S.M[s] = n_mels[s];
        S.flags[s] = flags[s];
        S.eff[s] = parts != nullptr ? flags[s] : (flags[s] & want);
        S.runs[s] = P.runs[s];
        S.rec_off[s] = (long)(P.rec[s] / sizeof(double));
        fb_base[s] = filters;
        filters += n_mels[s];
        mel_work = mel_work || (S.eff[s] & SWC_SPECTRAL_MEL);
    }
    SWC_CHECK_ARG(n_lsd <= 1, "swc_spectral: %d scales are flagged LSD (at most one)", n_lsd);
    SWC_CHECK_ARG(!mel_work || (fb_first && fb_count && fb_off && fb_w), "swc_spectral: null pointer (MEL work needs the mel table)");
    SWC_CHECK_ARG(fb_w_len >= 0 && fb_w_len < 0x7fffffffL, "swc_spectral: fb_w_len=%ld out of range", (long)fb_w_len);
    SWC_CHECK_ARG(workspace_bytes >= (int64_t)P.total, "swc_spectral: workspace of %ld bytes, %ld needed (swc_spectral_workspace_bytes)",
                  (long)workspace_bytes, (long)P.total);
    SWC_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "swc_spectral: workspace must be 256-byte aligned");
    if (B == 0) return SWC_OK;
    hipStream_t st = (hipStream_t)stream;
    double* ws = reinterpret_cast<double*>(workspace);
    const long max_n = max_n_in;
    for (int s = 0; s < n_scales; ++s) {
        if (S.eff[s] == 0) continue;
        const dim3 grid((unsigned)S.runs[s], (unsigned)B);
        double* rec = ws + S.rec_off[s];
#define SWC_SPECTRAL_CASE(WIN)                                                                                                    \
    case WIN:                                                                                                                     \
        launch_frames<WIN>(grid, st, x_rows, y_rows, n_in, max_n, S.eff[s], S.M[s], fb_base[s], fb_first, fb_count, fb_off, fb_w, \
                           (long)fb_w_len, rec, S.runs[s]);                                                                       \
        break
        switch (S.W[s]) {
            SWC_SPECTRAL_CASE(32);
            SWC_SPECTRAL_CASE(64);
            SWC_SPECTRAL_CASE(128);
            SWC_SPECTRAL_CASE(256);
            SWC_SPECTRAL_CASE(512);
            SWC_SPECTRAL_CASE(1024);
            SWC_SPECTRAL_CASE(2048);
        }
#undef SWC_SPECTRAL_CASE
        SWC_CHECK_LAUNCH("swc_spectral (frames)");
    }
    hipLaunchKernelGGL(spectral_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, n_in, max_n, (const double*)ws, S, mel, stft, lsd,
                       parts);
    SWC_CHECK_LAUNCH("swc_spectral (finish)");
    return SWC_OK;
}
