// What the two framed-FFT kernels share (spectral_frames_kernel<W> of swc_spectral.hip, cepstra_frames_kernel<W> of
// swc_mcd.hip): the run and team geometry, the twiddle and window tables, the windowed frames of S signals transformed in LDS
// into W / 2 + 1 magnitudes each, and the mel band over them.  Helpers only, as swc_metric_common.h: no kernel lives here.
// swc_stoi.hip's DFT is an MFMA product against a table, not this FFT, and stays where it is.
// cepstra_frames_kernel uses all of it (S = 1), spectral_frames_kernel too (S = 2) but for frame_magnitudes at W = 256: there
// it keeps the same three loops written out, because inlined from here they are scheduled differently and that one window
// measured 4.9 % slower (profiles/frame_fft_ab.txt).  A change to frame_magnitudes is made there too.
//
// A workgroup of 256 threads takes one run of 32768 / W consecutive frames of one row.  A TEAM of TS = min(W / 2, 256) threads
// owns a frame (a quarter of a wave at W = 32, a wave at W = 128, the workgroup from W = 512 on), so 256 / TS frames are in
// flight per pass.  Per frame the S windowed frames are loaded (zero outside [0, n), nothing outside the row is read), each
// packed into W / 2 complex points in bit-reversed order, transformed in place by the same radix-2 butterflies (the work index
// carries the signal, so all S go through the same instructions) and unpacked into W / 2 + 1 magnitudes.
// Twiddles exp(-2 pi i q / W), q < W / 2, and the window are evaluated in float64 (sincospi / cospi) once per workgroup and
// kept in LDS as f32; the FFT stages and the unpacking both read that one table.
// LDS banking: a butterfly reads two float2 (ds_read_b64, 64 banks); from half-size 32 on a team's lanes read consecutive
// float2 (conflict-free), the first five stages read with a stride of 2 .. 32 float2 between pairs of lanes (2-way).
// The LDS arrays belong to the kernels: float2 s_tw[N], float s_win[W], float2 s_z[TEAMS][S][N], float s_mag[TEAMS][S][F + 1].
#pragma once
#include "swc_metric_common.h"
#include "swc_spectral.h"

constexpr int FR_THREADS = 256;
constexpr int FR_RUN_SAMPLES = 32768;  // W * frames of a run
static_assert(SWC_SPECTRAL_MIN_WIN == 32 && SWC_SPECTRAL_MAX_WIN == 2048, "swc_mcd.h states swc_spectral.h's window limits as 32 .. 2048");

static inline bool valid_window(int w) { return w >= SWC_SPECTRAL_MIN_WIN && w <= SWC_SPECTRAL_MAX_WIN && (w & (w - 1)) == 0; }

template <int W>
struct FrameGeo {
    static constexpr int N = W / 2, F = W / 2 + 1;
    static constexpr int TS = N < FR_THREADS ? N : FR_THREADS;  // threads that own a frame
    static constexpr int TEAMS = FR_THREADS / TS;               // frames in flight
    static constexpr int TW = TS < 64 ? 1 : TS / 64;            // waves of a team
    static constexpr int R = FR_RUN_SAMPLES / W;                // frames of a run
    static constexpr int LOGN = __builtin_ctz(N);
    static_assert(R % TEAMS == 0 && TS * TEAMS == FR_THREADS, "a run is a whole number of passes");
};

// the two tables of a workgroup.  Every thread of the workgroup calls it; it ends with a barrier
template <int W>
__device__ __forceinline__ void frame_tables(float2* s_tw, float* s_win, int tid) {
    for (int q = tid; q < FrameGeo<W>::N; q += FR_THREADS) {
        double sn, cs;
        sincospi(-2.0 * (double)q / (double)W, &sn, &cs);
        s_tw[q] = make_float2((float)cs, (float)sn);
    }
    for (int i = tid; i < W; i += FR_THREADS) s_win[i] = (float)(0.5 - 0.5 * cospi(2.0 * (double)i / (double)W));
    __syncthreads();
}

// mag[sig][0 .. W / 2] = |FFT of the windowed frame that starts at sample `start` of rows[sig]|, sig < S, by the team whose
// thread this is (lt = its index in the team; z, mag = the team's slices).  A team that is not `active` works on zeros.
// Every thread of the workgroup calls it: 2 + log2(W / 2) barriers, the last one after the magnitudes are written
template <int W, int S>
__device__ __forceinline__ void frame_magnitudes(const float* const (&rows)[S], long n, long start, bool active, int lt,
                                                 const float2* s_tw, const float* s_win, float2 (*z)[W / 2],
                                                 float (*mag)[W / 2 + 2]) {
    using G = FrameGeo<W>;
    constexpr int N = G::N, TS = G::TS, LOGN = G::LOGN;
    // the windowed frames, packed z[k] = v[2 k] + i v[2 k + 1], stored where the in-place transform wants them
    for (int i = lt; i < S * N; i += TS) {
        const int sig = S == 1 ? 0 : i / N, k = S == 1 ? i : i % N;
        const long i0 = start + 2 * k;
        const float* p = rows[sig];
        const float v0 = (active && i0 >= 0 && i0 < n) ? p[i0] * s_win[2 * k] : 0.0f;
        const float v1 = (active && i0 + 1 >= 0 && i0 + 1 < n) ? p[i0 + 1] * s_win[2 * k + 1] : 0.0f;
        z[sig][__brev((unsigned)k) >> (32 - LOGN)] = make_float2(v0, v1);
    }
    __syncthreads();
#pragma unroll 1
    for (int lh = 0; lh < LOGN; ++lh) {
        const int h = 1 << lh;
        for (int i = lt; i < S * (N / 2); i += TS) {  // N / 2 butterflies of one signal, then of the next
            const int sig = S == 1 ? 0 : i / (N / 2), j = S == 1 ? i : i % (N / 2);
            const int k = j & (h - 1), a = ((j >> lh) << (lh + 1)) + k;
            const float2 w = s_tw[k << (LOGN - lh)];  // exp(-2 pi i k / (2 h))
            float2* zs = z[sig];
            const float2 u = zs[a], v = zs[a + h];
            const float tr = w.x * v.x - w.y * v.y, ti = w.x * v.y + w.y * v.x;
            zs[a] = make_float2(u.x + tr, u.y + ti);
            zs[a + h] = make_float2(u.x - tr, u.y - ti);
        }
        __syncthreads();
    }
    // unpack: with A = Z[f], Bc = conj Z[N - f]: E = (A + Bc) / 2, O = -i (A - Bc) / 2, P = tw[f] O;
    // |X[f]| = |E + P|, |X[N - f]| = |E - P|, f = 0 .. N / 2
    for (int i = lt; i < S * (N / 2 + 1); i += TS) {
        const int sig = S == 1 ? 0 : i / (N / 2 + 1), f = S == 1 ? i : i % (N / 2 + 1);
        const float2* zs = z[sig];
        const float2 A = zs[f], B = zs[(N - f) & (N - 1)], w = s_tw[f];
        const float er = 0.5f * (A.x + B.x), ei = 0.5f * (A.y - B.y);
        const float orr = 0.5f * (A.y + B.y), oi = -0.5f * (A.x - B.x);
        const float pr = w.x * orr - w.y * oi, pi = w.x * oi + w.y * orr;
        const float ar = er + pr, ai = ei + pi, br = er - pr, bi = ei - pi;
        mag[sig][f] = sqrtf(ar * ar + ai * ai);
        mag[sig][N - f] = sqrtf(br * br + bi * bi);
    }
    __syncthreads();
}

// acc[sig] = sum_f w[f] mag[sig][f] over the bins of one mel filter (first bin, count, offset of its weights in fb_w), cut
// into [0, F) and into [0, fb_w_len): sequential in f, one fmaf per term and signal, each weight read once.  (The sums are
// locals copied out at the end: accumulating through the reference costs spectral_frames_kernel 2 - 4 VGPRs.)
template <int F, int S>
__device__ __forceinline__ void mel_band(long first, long cnt, long off, const float* fb_w, long fb_w_len,
                                         const float (*mag)[F + 1], float (&acc)[S]) {
    const long lo = first < 0 ? 0 : first, hi = first + cnt < F ? first + cnt : F;  // cut into [0, F)
    float a[S] = {};
    for (long f = lo; f < hi; ++f) {
        const long wi = off + (f - first);
        if (wi < 0 || wi >= fb_w_len) continue;  // cut into the weight array
        const float w = fb_w[wi];
#pragma unroll
        for (int sig = 0; sig < S; ++sig) a[sig] = fmaf(w, mag[sig][f], a[sig]);
    }
#pragma unroll
    for (int sig = 0; sig < S; ++sig) acc[sig] = a[sig];
}
