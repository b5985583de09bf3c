// swc_noise, swc_mix and swc_convolve (include/swc_degrade.h): reproducible noise, mixing at a signal-to-noise ratio whose gain
// is computed on the device, and partitioned FFT convolution of a ragged batch with long impulse responses.
//   noise_kernel        grid (chunks, B): a workgroup of 256 threads writes SWC_DEGRADE_CHUNK columns of one row, one Philox4x32-10
//                       block per sample (integer arithmetic; the one float operation is the exact scaling of V).
//   mix_head_kernel     grid (B / 256): one thread per row: the gain (float64 pow, rounded once) and flag bit 0.
//   mix_kernel          grid (chunks, B): thread 0 evaluates the row's gain again (the same device function: the same bits), the
//                       workgroup mixes SWC_DEGRADE_CHUNK columns; the index into the noise row is reduced modulo m once per
//                       thread and then stepped.  One atomicOr per wave that saw a sample beyond full scale.
//   conv_spectra_kernel grid (runs, rows): CV_RUN consecutive windows of one input row, or partitions of one impulse response,
//                       each transformed in LDS (1024 packed complex points, radix-2, the network of swc_frame_fft.h's
//                       frame_magnitudes) and unpacked into 1024 float2 of spectrum, the Nyquist bin beside DC.  A window that
//                       holds no sample of its row, and a partition behind the response's end, is not written and never read.
//   conv_sum_kernel     grid (output blocks, B): sums X[j - p] H[p] over the partitions of the row's own response (4 bins per
//                       thread in registers), re-packs the sum through LDS, runs the inverse network and stores the second
//                       half of the 2048 samples.  A block behind the row's output length stores zeros and returns.
// The transforms and the unpacking live here, not in swc_frame_fft.h: that header's W = 256 path is sensitive to rescheduling.
// LDS of the two convolution kernels: 8 KB of twiddles + 8 KB (spectra) or 16 KB (sum) of points.  The twiddles are evaluated
// in float64 once per workgroup.  Every store to global memory is an ordinary vector store or a vector atomic from plain C++.
#include "swc_common.h"
#include "swc_degrade.h"

namespace {

constexpr int DG_THREADS = 256;
constexpr int DG_CHUNK = SWC_DEGRADE_CHUNK;
constexpr int DG_PER = DG_CHUNK / DG_THREADS;
constexpr int CV_N = SWC_CONV_BLOCK;
constexpr int CV_LOGN = 10;
constexpr int CV_RUN = 8;  // windows (partitions) one workgroup of conv_spectra_kernel transforms: the twiddle table is built once
static_assert(CV_N == 1 << CV_LOGN && CV_N % DG_THREADS == 0, "1024 packed points, 4 per thread");

__device__ __forceinline__ long clamp_len(long v, long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---------------------------------------------------------------- swc_noise ----

__device__ __forceinline__ int philox_v(unsigned k0, unsigned k1, unsigned long long j, unsigned long long s) {
    unsigned c0 = (unsigned)j, c1 = (unsigned)(j >> 32), c2 = (unsigned)s, c3 = (unsigned)(s >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const unsigned h = (c0 & 0xffffu) + (c0 >> 16) + (c1 & 0xffffu) + (c1 >> 16) + (c2 & 0xffffu) + (c2 >> 16) + (c3 & 0xffffu) + (c3 >> 16);
    return 2 * (int)h - 8 * 65535;
}

__global__ __launch_bounds__(DG_THREADS) void noise_kernel(unsigned long long seed, const int64_t* __restrict__ ids,
                                                           const int64_t* __restrict__ lens, long first, float* __restrict__ out,
                                                           long ld, long cols) {
    const int b = blockIdx.y;
    const long n = lens[b] < 0 ? 0 : lens[b];
    const unsigned long long s = (unsigned long long)ids[b];
    float* o = out + (long)b * ld;
    long i = (long)blockIdx.x * DG_CHUNK + threadIdx.x;
#pragma unroll 1
    for (int k = 0; k < DG_PER; ++k, i += DG_THREADS) {
        if (i >= cols) break;
        o[i] = i < n ? (float)philox_v((unsigned)seed, (unsigned)(seed >> 32), (unsigned long long)(first + i), s) * 0x1p-19f : 0.0f;
    }
}

// ---------------------------------------------------------------- swc_mix ----

__device__ __forceinline__ float mix_gain(const double* lx, long slx, const double* ln, long sln, const double* snr, long ssnr, int b,
                                          long m, bool* mixed) {
    const double a = lx[b * slx], c = ln[b * sln], t = snr[b * ssnr];
    const bool ok = isfinite(a) && isfinite(c) && isfinite(t) && m > 0;
    *mixed = ok;
    return ok ? (float)pow(10.0, (a - c - t) / 20.0) : 0.0f;
}

__global__ __launch_bounds__(DG_THREADS) void mix_head_kernel(const int64_t* __restrict__ n_noise, const double* lx, long slx,
                                                              const double* ln, long sln, const double* snr, long ssnr,
                                                              float* __restrict__ gains, int* __restrict__ flags, int B) {
    const int b = blockIdx.x * DG_THREADS + threadIdx.x;
    if (b >= B) return;
    bool mixed;
    const float g = mix_gain(lx, slx, ln, sln, snr, ssnr, b, n_noise[b], &mixed);
    if (gains) gains[b] = g;
    if (flags) flags[b] = mixed ? 0 : SWC_MIX_UNMIXED;
}

__global__ __launch_bounds__(DG_THREADS) void mix_kernel(const void* const* __restrict__ x_rows, const int64_t* __restrict__ n_x,
                                                         const void* const* __restrict__ v_rows, const int64_t* __restrict__ n_noise,
                                                         const double* lx, long slx, const double* ln, long sln, const double* snr,
                                                         long ssnr, float* __restrict__ out, long ld, long cols,
                                                         int* __restrict__ flags) {
    __shared__ float s_g;
    __shared__ int s_mixed;
    const int tid = threadIdx.x, b = blockIdx.y;
    const long n = n_x[b] < 0 ? 0 : n_x[b];
    const long m = n_noise[b] < 0 ? 0 : n_noise[b];
    if (tid == 0) {
        bool mixed;
        s_g = mix_gain(lx, slx, ln, sln, snr, ssnr, b, m, &mixed);
        s_mixed = mixed;
    }
    __syncthreads();
    const float g = s_g;
    const bool mixed = s_mixed != 0;
    const float* x = n > 0 ? reinterpret_cast<const float*>(x_rows[b]) : nullptr;
    const float* v = mixed ? reinterpret_cast<const float*>(v_rows[b]) : nullptr;
    float* o = out ? out + (long)b * ld : nullptr;
    long i = (long)blockIdx.x * DG_CHUNK + tid;
    long r = mixed ? i % m : 0;
    const long step = mixed ? DG_THREADS % m : 0;
    bool over = false;
#pragma unroll 1
    for (int k = 0; k < DG_PER; ++k, i += DG_THREADS) {
        if (i < cols) {
            float y = 0.0f;
            if (i < n) {
                const float xv = x[i];
                y = mixed ? fmaf(v[r], g, xv) : xv;
                over = over || fabsf(y) > 1.0f;
            }
            if (o) o[i] = y;
        }
        r += step;
        if (r >= m) r -= m;
    }
    if (flags != nullptr) {
        const bool any = __ballot(over) != 0;
        if (any && (tid & 63) == 0) atomicOr(flags + b, SWC_MIX_OVER);
    }
}

// ---------------------------------------------------------------- swc_convolve ----

// t[q] = exp(-2 pi i q / (2 N)), q < N.  Every thread of the workgroup calls it; it ends with a barrier
__device__ __forceinline__ void conv_tables(float2* s_tw, int tid) {
    for (int q = tid; q < CV_N; q += DG_THREADS) {
        double sn, cs;
        sincospi(-(double)q / (double)CV_N, &sn, &cs);
        s_tw[q] = make_float2((float)cs, (float)sn);
    }
    __syncthreads();
}

__device__ __forceinline__ int brev10(int k) { return (int)(__brev((unsigned)k) >> (32 - CV_LOGN)); }

// the radix-2 network over z[0 .. N) (bit-reversed input, natural output), with conj(w) where INV.  Ends with a barrier
template <bool INV>
__device__ __forceinline__ void conv_fft(float2* z, const float2* s_tw, int tid) {
#pragma unroll 1
    for (int lh = 0; lh < CV_LOGN; ++lh) {
        const int h = 1 << lh;
        for (int j = tid; j < CV_N / 2; j += DG_THREADS) {
            const int k = j & (h - 1), a = ((j >> lh) << (lh + 1)) + k;
            float2 w = s_tw[k << (CV_LOGN - lh)];
            if (INV) w.y = -w.y;
            const float2 u = z[a], v = z[a + h];
            const float tr = fmaf(w.x, v.x, -(w.y * v.y)), ti = fmaf(w.x, v.y, w.y * v.x);
            z[a] = make_float2(u.x + tr, u.y + ti);
            z[a + h] = make_float2(u.x - tr, u.y - ti);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int conv_first_window(int d) { return -((d + CV_N - 1) >> CV_LOGN); }
// window w (samples N (w - 1) + d .. N (w + 1) + d - 1) holds a sample of a row of n
__device__ __forceinline__ bool conv_window_live(long w, int d, long n) {
    return n > 0 && (w + 1) * CV_N + d > 0 && (w - 1) * CV_N + d < n;
}

// kind 0: `rows` are the input rows, `per` = W windows each; kind 1: the impulse responses, `per` = Pmax partitions each
__global__ __launch_bounds__(DG_THREADS) void conv_spectra_kernel(const void* const* __restrict__ rows, const int64_t* __restrict__ lens,
                                                                  long max_len, int kind, int d, int per, float2* __restrict__ spec) {
    __shared__ float2 s_tw[CV_N];
    __shared__ float2 s_z[CV_N];
    const int tid = threadIdx.x, row = blockIdx.y;
    const long n = clamp_len(lens[row], max_len);
    const int i_lo = blockIdx.x * CV_RUN, i_hi = i_lo + CV_RUN < per ? i_lo + CV_RUN : per;
    const int w_lo = conv_first_window(d);
    // (uniform) whether this run has anything to transform at all
    bool any = false;
    for (int idx = i_lo; idx < i_hi; ++idx) any = any || (kind == 0 ? conv_window_live((long)idx + w_lo, d, n) : (long)idx * CV_N < n);
    if (!any) return;
    conv_tables(s_tw, tid);
    const float* p = reinterpret_cast<const float*>(rows[row]);  // n > 0 here
    for (int idx = i_lo; idx < i_hi; ++idx) {
        const bool live = kind == 0 ? conv_window_live((long)idx + w_lo, d, n) : (long)idx * CV_N < n;
        if (!live) continue;  // (uniform)
        const long s0 = kind == 0 ? ((long)idx + w_lo - 1) * CV_N + d : (long)idx * CV_N;
        const int span = kind == 0 ? 2 * CV_N : CV_N;  // a partition's second half is zero
        for (int k = tid; k < CV_N; k += DG_THREADS) {
            const long i0 = s0 + 2 * k;
            const float v0 = (2 * k < span && i0 >= 0 && i0 < n) ? p[i0] : 0.0f;
            const float v1 = (2 * k + 1 < span && i0 + 1 >= 0 && i0 + 1 < n) ? p[i0 + 1] : 0.0f;
            s_z[brev10(k)] = make_float2(v0, v1);
        }
        __syncthreads();
        conv_fft<false>(s_z, s_tw, tid);
        float2* o = spec + ((long)row * per + idx) * CV_N;
        for (int f = tid; f < CV_N; f += DG_THREADS) {
            const float2 A = s_z[f], B = s_z[(CV_N - f) & (CV_N - 1)], w = s_tw[f];
            const float er = 0.5f * (A.x + B.x), ei = 0.5f * (A.y - B.y);
            const float orr = 0.5f * (A.y + B.y), oi = -0.5f * (A.x - B.x);
            const float pr = fmaf(w.x, orr, -(w.y * oi)), pi = fmaf(w.x, oi, w.y * orr);
            o[f] = f == 0 ? make_float2(A.x + A.y, A.x - A.y) : make_float2(er + pr, ei + pi);
        }
        __syncthreads();  // s_z is free again
    }
}

__global__ __launch_bounds__(DG_THREADS) void conv_sum_kernel(const int64_t* __restrict__ lens, long max_n, const int64_t* __restrict__ h_len,
                                                              int R, int max_L, const int64_t* __restrict__ h_index, int d, int extra,
                                                              int W, int Pmax, const float2* __restrict__ spec_x,
                                                              const float2* __restrict__ spec_h, float* __restrict__ out, long ld, long cols) {
    __shared__ float2 s_tw[CV_N];
    __shared__ float2 s_y[CV_N];
    __shared__ float2 s_z[CV_N];
    constexpr int PER = CV_N / DG_THREADS;
    const int tid = threadIdx.x, b = blockIdx.y;
    const long j = blockIdx.x, t0 = j * CV_N;
    const long n = clamp_len(lens[b], max_n);
    const long len = n + extra < cols ? n + extra : cols;
    float* o = out + (long)b * ld + t0;
    if (t0 >= len) {  // (uniform) behind the row's output: zeros
        for (int t = tid; t < CV_N; t += DG_THREADS)
            if (t0 + t < cols) o[t] = 0.0f;
        return;
    }
    const long r = h_index ? clamp_len(h_index[b], R - 1) : 0;
    const long L = clamp_len(h_len[r], max_L);
    const int P = (int)((L + CV_N - 1) >> CV_LOGN);
    const int w_lo = conv_first_window(d);
    conv_tables(s_tw, tid);
    float2 acc[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) acc[q] = make_float2(0.0f, 0.0f);
#pragma unroll 1
    for (int p = 0; p < P; ++p) {
        const long w = j - p;
        if (!conv_window_live(w, d, n)) continue;  // (uniform) never written by the spectra kernel either
        const long wi = w - w_lo;
        if (wi < 0 || wi >= W) continue;            // (cannot happen for n <= max_n; keeps every read inside the workspace)
        const float2* X = spec_x + ((long)b * W + wi) * CV_N;
        const float2* H = spec_h + (r * Pmax + p) * CV_N;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int f = tid + q * DG_THREADS;
            const float2 x = X[f], h = H[f];
            if (f == 0) {
                acc[q].x = fmaf(x.x, h.x, acc[q].x);
                acc[q].y = fmaf(x.y, h.y, acc[q].y);
            } else {
                acc[q].x = fmaf(x.x, h.x, fmaf(-x.y, h.y, acc[q].x));
                acc[q].y = fmaf(x.x, h.y, fmaf(x.y, h.x, acc[q].y));
            }
        }
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) s_y[tid + q * DG_THREADS] = acc[q];
    __syncthreads();
    // re-pack: Z'[f] = E + i O with E = A + conj B, O = conj(t[f]) (A - conj B), A = Y[f], B = Y[N - f]
    for (int f = tid; f < CV_N; f += DG_THREADS) {
        const float2 A = s_y[f], B = s_y[(CV_N - f) & (CV_N - 1)], w = s_tw[f];
        const float er = A.x + B.x, ei = A.y - B.y, pr = A.x - B.x, pi = A.y + B.y;
        const float orr = fmaf(w.x, pr, w.y * pi), oi = fmaf(w.x, pi, -(w.y * pr));
        s_z[brev10(f)] = f == 0 ? make_float2(A.x + A.y, A.x - A.y) : make_float2(er - oi, ei + orr);
    }
    __syncthreads();
    conv_fft<true>(s_z, s_tw, tid);
    const float* v = reinterpret_cast<const float*>(s_z) + CV_N;  // samples N .. 2 N - 1 of the 2 N
    for (int t = tid; t < CV_N; t += DG_THREADS) {
        if (t0 + t < len) o[t] = v[t] * (1.0f / (2 * CV_N));
        else if (t0 + t < cols) o[t] = 0.0f;
    }
}

bool conv_geometry_ok(int32_t B, int64_t max_n, int32_t R, int32_t max_L) {
    return B >= 0 && B <= 65535 && max_n >= 0 && max_n <= SWC_CONV_MAX_N && R >= 1 && R <= SWC_CONV_MAX_IRS && max_L >= 1 &&
           max_L <= SWC_CONV_MAX_TAPS;
}
inline long conv_windows(int64_t max_n) { return (long)((max_n + CV_N - 1) / CV_N) + 2; }
inline long conv_partitions(int32_t max_L) { return (max_L + CV_N - 1) / CV_N; }

}  // namespace

extern "C" int swc_noise(uint64_t seed, const int64_t* stream_ids, const int64_t* n, int64_t first, float* out, int64_t ld, int64_t cols,
                         int32_t B, void* stream) {
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_noise: B=%d (0..65535)", B);
    SWC_CHECK_ARG(first >= 0, "swc_noise: first=%lld (>= 0)", (long long)first);
    SWC_CHECK_ARG(cols >= 0 && cols <= ld, "swc_noise: cols=%lld, ld=%lld (0 <= cols <= ld)", (long long)cols, (long long)ld);
    if (B == 0 || cols == 0) return SWC_OK;
    SWC_CHECK_ARG(stream_ids && n && out, "swc_noise: null pointer");
    SWC_CHECK_ARG(((uintptr_t)stream_ids & 7u) == 0 && ((uintptr_t)n & 7u) == 0 && ((uintptr_t)out & 3u) == 0, "swc_noise: misaligned pointer");
    SWC_CHECK_ARG((cols + DG_CHUNK - 1) / DG_CHUNK <= 0x7fffffffLL, "swc_noise: cols=%lld", (long long)cols);
    const dim3 grid((unsigned)((cols + DG_CHUNK - 1) / DG_CHUNK), (unsigned)B), block(DG_THREADS);
    hipLaunchKernelGGL(noise_kernel, grid, block, 0, (hipStream_t)stream, (unsigned long long)seed, stream_ids, n, (long)first, out, (long)ld,
                       (long)cols);
    SWC_CHECK_LAUNCH("swc_noise");
    return SWC_OK;
}

extern "C" int swc_mix(const void* const* x_rows, const int64_t* n_x, const void* const* noise_rows, const int64_t* n_noise, const double* lx,
                       int64_t lx_stride, const double* ln, int64_t ln_stride, const double* snr, int64_t snr_stride, float* out,
                       int64_t ld, int64_t cols, float* gains, int32_t* flags, int32_t B, void* stream) {
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_mix: B=%d (0..65535)", B);
    SWC_CHECK_ARG(lx_stride >= 0 && ln_stride >= 0 && snr_stride >= 0, "swc_mix: a negative stride");
    SWC_CHECK_ARG(cols >= 0 && cols <= ld, "swc_mix: cols=%lld, ld=%lld (0 <= cols <= ld)", (long long)cols, (long long)ld);
    SWC_CHECK_ARG(out || gains || flags, "swc_mix: no output (out, gains and flags are all null)");
    if (B == 0) return SWC_OK;
    SWC_CHECK_ARG(x_rows && n_x && noise_rows && n_noise && lx && ln && snr, "swc_mix: null pointer");
    SWC_CHECK_ARG((((uintptr_t)x_rows | (uintptr_t)n_x | (uintptr_t)noise_rows | (uintptr_t)n_noise | (uintptr_t)lx | (uintptr_t)ln |
                    (uintptr_t)snr) & 7u) == 0 && (((uintptr_t)out | (uintptr_t)gains | (uintptr_t)flags) & 3u) == 0,
                  "swc_mix: misaligned pointer");
    SWC_CHECK_ARG((cols + DG_CHUNK - 1) / DG_CHUNK <= 0x7fffffffLL, "swc_mix: cols=%lld", (long long)cols);
    const dim3 block(DG_THREADS);
    if (gains || flags) {
        hipLaunchKernelGGL(mix_head_kernel, dim3((unsigned)((B + DG_THREADS - 1) / DG_THREADS)), block, 0, (hipStream_t)stream, n_noise, lx,
                           (long)lx_stride, ln, (long)ln_stride, snr, (long)snr_stride, gains, flags, (int)B);
    }
    if (cols > 0 && (out || flags)) {
        const dim3 grid((unsigned)((cols + DG_CHUNK - 1) / DG_CHUNK), (unsigned)B);
        hipLaunchKernelGGL(mix_kernel, grid, block, 0, (hipStream_t)stream, x_rows, n_x, noise_rows, n_noise, lx, (long)lx_stride, ln,
                           (long)ln_stride, snr, (long)snr_stride, out, (long)ld, (long)cols, flags);
    }
    SWC_CHECK_LAUNCH("swc_mix");
    return SWC_OK;
}

extern "C" int64_t swc_convolve_workspace_bytes(int32_t B, int64_t max_n, int32_t R, int32_t max_L) {
    if (!conv_geometry_ok(B, max_n, R, max_L)) return -1;
    return (int64_t)sizeof(float2) * CV_N * ((int64_t)B * conv_windows(max_n) + (int64_t)R * conv_partitions(max_L));
}

extern "C" int swc_convolve(const void* const* x_rows, const int64_t* n, int64_t max_n, const void* const* h_rows, const int64_t* h_len,
                            int32_t R, int32_t max_L, const int64_t* h_index, int32_t d, int32_t extra, float* out, int64_t ld,
                            int64_t cols, void* workspace, int64_t workspace_bytes, int32_t B, void* stream) {
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_convolve: B=%d (0..65535)", B);
    SWC_CHECK_ARG(R >= 1 && R <= SWC_CONV_MAX_IRS, "swc_convolve: R=%d (1..%d)", R, SWC_CONV_MAX_IRS);
    SWC_CHECK_ARG(max_L >= 1 && max_L <= SWC_CONV_MAX_TAPS, "swc_convolve: max_L=%d (1..%d)", max_L, SWC_CONV_MAX_TAPS);
    SWC_CHECK_ARG(d >= 0 && d < max_L, "swc_convolve: d=%d (0 <= d < max_L = %d)", d, max_L);
    SWC_CHECK_ARG(extra >= 0 && extra <= max_L - 1, "swc_convolve: extra=%d (0 <= extra <= max_L - 1 = %d)", extra, max_L - 1);
    SWC_CHECK_ARG(max_n >= 0 && max_n <= SWC_CONV_MAX_N, "swc_convolve: max_n=%lld (0..%d)", (long long)max_n, SWC_CONV_MAX_N);
    SWC_CHECK_ARG(cols >= 0 && cols <= ld, "swc_convolve: cols=%lld, ld=%lld (0 <= cols <= ld)", (long long)cols, (long long)ld);
    SWC_CHECK_ARG(R == 1 || h_index != nullptr, "swc_convolve: h_index may be null only when R == 1 (R=%d)", R);
    if (B == 0 || cols == 0) return SWC_OK;
    SWC_CHECK_ARG(x_rows && n && h_rows && h_len && out && workspace, "swc_convolve: null pointer");
    SWC_CHECK_ARG((((uintptr_t)x_rows | (uintptr_t)n | (uintptr_t)h_rows | (uintptr_t)h_len | (uintptr_t)h_index) & 7u) == 0 &&
                      ((uintptr_t)out & 3u) == 0 && ((uintptr_t)workspace & 255u) == 0,
                  "swc_convolve: misaligned pointer (the workspace is 256-byte aligned)");
    const int64_t need = swc_convolve_workspace_bytes(B, max_n, R, max_L);
    SWC_CHECK_ARG(workspace_bytes >= need, "swc_convolve: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    SWC_CHECK_ARG((cols + CV_N - 1) / CV_N <= 0x7fffffffLL, "swc_convolve: cols=%lld", (long long)cols);
    const int W = (int)conv_windows(max_n), Pmax = (int)conv_partitions(max_L);
    float2* spec_x = reinterpret_cast<float2*>(workspace);
    float2* spec_h = spec_x + (int64_t)B * W * CV_N;
    const dim3 block(DG_THREADS);
    hipLaunchKernelGGL(conv_spectra_kernel, dim3((unsigned)((W + CV_RUN - 1) / CV_RUN), (unsigned)B), block, 0, (hipStream_t)stream, x_rows, n,
                       (long)max_n, 0, (int)d, W, spec_x);
    hipLaunchKernelGGL(conv_spectra_kernel, dim3((unsigned)((Pmax + CV_RUN - 1) / CV_RUN), (unsigned)R), block, 0, (hipStream_t)stream, h_rows,
                       h_len, (long)max_L, 1, 0, Pmax, spec_h);
    hipLaunchKernelGGL(conv_sum_kernel, dim3((unsigned)((cols + CV_N - 1) / CV_N), (unsigned)B), block, 0, (hipStream_t)stream, n, (long)max_n,
                       h_len, (int)R, (int)max_L, h_index, (int)d, (int)extra, W, Pmax, spec_x, spec_h, out, (long)ld, (long)cols);
    SWC_CHECK_LAUNCH("swc_convolve");
    return SWC_OK;
}
