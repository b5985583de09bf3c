// Loudness on the device (include/swc_loudness.h): BS.1770-4 integrated loudness, EBU Tech 3342 range, the largest momentary and
// short-term loudness, sample peak and true peak of every row of a ragged batch, and the normalising gain computed and applied
// without a read-back.
//
// The K-weighting is a recursion (pole radius 0.995 at 48 kHz), so a row cannot simply be cut into independent pieces.  It is
// linear, though: the state at the end of a sub-block of L = fs / 10 samples is M s + (the state the sub-block leaves when it
// starts from zero), M the 4 x 4 transition over L samples.  Five launches:
//   peaks    (tiles x rows)  max |x| and the 4 x interpolated max (swc_resample's own fmaf chain) of a tile, one integer
//                            atomic maximum per workgroup
//   filter 1 (S/64 x rows)   one lane per sub-block filters its samples from zero state and leaves the final state
//   carry    (rows)          s_{k+1} = M s_k + zs_k along the row: the true state at the start of every sub-block
//   filter 2 (S/64 x rows)   one lane per sub-block filters again from its true state and leaves z_k = mean y^2
//   gate     (rows)          one workgroup per row: block energies, the two gates of I, the two gates and the radix selection of
//                            LRA, the eight values
// The two filter passes stage tiles of 64 sub-blocks x 64 samples through LDS: the global reads are rows of 64 consecutive
// floats, the lanes then walk their own sub-block out of LDS (stride 65 words: no bank conflict); the next tile's loads are in
// flight in registers while the current one is filtered.  The segmentation is fixed by fs: nothing depends on the grid.
#include "swc_metric_common.h"
#include "swc_loudness.h"
#include <math.h>

namespace {

constexpr int LG = SWC_LOUDNESS_GROUP;  // sub-blocks per workgroup of a filter pass = lanes of its one wave
constexpr int LT = 64;                  // samples of every sub-block per LDS tile
constexpr int LS = LT + 1;              // LDS row stride in words
constexpr int PK_THREADS = 256;
constexpr int PK_TILE = 2048;           // input samples per workgroup of the peak kernel
constexpr int GT_THREADS = 256;
constexpr int NM_THREADS = 256;
constexpr int NM_TILE = 4096;           // output columns per workgroup of the normalise kernel

struct KWeights {
    double k[10];  // shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
    double M[16];  // the state transition over L samples, row-major
};

// one sample through the cascade (both biquads transposed direct form II); s = z1, z2 of the shelf, z1, z2 of the high-pass
__host__ __device__ __forceinline__ double kw_step(const double* k, double* s, double x) {
    const double y1 = k[0] * x + s[0];
    s[0] = (k[1] * x + s[1]) - k[3] * y1;
    s[1] = k[2] * x - k[4] * y1;
    const double y2 = k[5] * y1 + s[2];
    s[2] = (k[6] * y1 + s[3]) - k[8] * y2;
    s[3] = k[7] * y1 - k[9] * y2;
    return y2;
}

bool fs_ok(int fs) { return fs >= SWC_LOUDNESS_MIN_FS && fs <= SWC_LOUDNESS_MAX_FS && fs % 10 == 0; }

void coefficients(int fs, double* k) {
    const double pi = 3.14159265358979323846;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(pi * f0 / fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        k[0] = (Vh + Vb * K / Q + K * K) / a0;
        k[1] = 2.0 * (K * K - Vh) / a0;
        k[2] = (Vh - Vb * K / Q + K * K) / a0;
        k[3] = 2.0 * (K * K - 1.0) / a0;
        k[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(pi * f0 / fs);
        const double a0 = 1.0 + K / Q + K * K;
        k[5] = 1.0;
        k[6] = -2.0;
        k[7] = 1.0;
        k[8] = 2.0 * (K * K - 1.0) / a0;
        k[9] = (1.0 - K / Q + K * K) / a0;
    }
}

// M: column c is what L silent samples leave of the unit state e_c
void transition(const double* k, int L, double* M) {
    for (int c = 0; c < 4; ++c) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        s[c] = 1.0;
        for (int i = 0; i < L; ++i) (void)kw_step(k, s, 0.0);
        for (int r = 0; r < 4; ++r) M[r * 4 + c] = s[r];
    }
}

__device__ __forceinline__ double loud(double e) { return -0.691 + 10.0 * log10(e); }

// ---- peaks ----

__global__ __launch_bounds__(PK_THREADS) void loud_peak_kernel(const void* const* __restrict__ rows, const int64_t* __restrict__ n_in,
                                                              long max_n, int width, const float* __restrict__ taps_packed,
                                                              const int* __restrict__ tap_start, int run, unsigned* __restrict__ peaks) {
    extern __shared__ __attribute__((aligned(16))) float pk_smem[];
    __shared__ unsigned red[2][PK_THREADS / 64];
    const int tid = threadIdx.x, b = blockIdx.y;
    const long n = clamp_len(n_in, b, max_n);
    const long i0 = (long)blockIdx.x * PK_TILE;
    if (i0 >= n) return;  // (uniform over the workgroup)
    const int cnt = (int)(n - i0 < PK_TILE ? n - i0 : PK_TILE);
    const int taps = 2 * width + 1;
    float* xs = pk_smem;                 // xs[s] = x[i0 - width + s], s in [0, cnt + 2 width), zeros outside the row
    float* tab = pk_smem + PK_TILE + taps;  // [4][run]
    __shared__ int st[4];
    const float* x = reinterpret_cast<const float*>(rows[b]);
    const int span = cnt + 2 * width;
    for (int s = tid; s < span; s += PK_THREADS) {
        const long i = i0 - width + s;
        xs[s] = (i >= 0 && i < n) ? x[i] : 0.0f;
    }
    for (int idx = tid; idx < 4 * run; idx += PK_THREADS) tab[idx] = taps_packed[idx];
    if (tid < 4) {
        const int v = tap_start[tid];
        st[tid] = v < 0 ? 0 : (v > taps - run ? taps - run : v);
    }
    __syncthreads();
    unsigned sp = 0u, tp = 0u;
    for (int f = tid; f < cnt; f += PK_THREADS) {
        sp = max(sp, __float_as_uint(fabsf(xs[f + width])));
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float* t = tab + p * run;
            const float* v = xs + f + st[p];  // f + st + k <= cnt - 1 + 2 width
            float acc = 0.0f;
            for (int k = 0; k < run; ++k) acc = fmaf(t[k], v[k], acc);
            tp = max(tp, __float_as_uint(fabsf(acc)));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sp = max(sp, (unsigned)__shfl_xor((int)sp, o));
        tp = max(tp, (unsigned)__shfl_xor((int)tp, o));
    }
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = sp;
        red[1][tid >> 6] = tp;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PK_THREADS / 64; ++w) {
            sp = max(sp, red[0][w]);
            tp = max(tp, red[1][w]);
        }
        atomicMax(peaks + 2 * b, sp);
        atomicMax(peaks + 2 * b + 1, tp);
    }
}

// ---- the two filter passes ----

template <bool SECOND>
__global__ __launch_bounds__(LG) void loud_filter_kernel(const void* const* __restrict__ rows, const int64_t* __restrict__ n_in,
                                                        long max_n, int L, KWeights kw, double* __restrict__ states,
                                                        double* __restrict__ z, long ld) {
    __shared__ float tile[LG * LS];
    const int lane = threadIdx.x, b = blockIdx.y;
    const long n = clamp_len(n_in, b, max_n);
    const long S = n / L;
    const long k0 = (long)blockIdx.x * LG;
    if (k0 >= S) return;  // (uniform over the workgroup)
    const int nsb = (int)(S - k0 < LG ? S - k0 : LG);
    const bool live = lane < nsb;
    const float* x = reinterpret_cast<const float*>(rows[b]) + k0 * L;  // sub-block k0 + r, sample j: x[r L + j] (below S L <= n)
    double* srow = states + ((long)b * ld + k0 + lane) * 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (SECOND && live) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = srow[i];
    }
    double acc = 0.0;
    float pre[LG];
#pragma unroll
    for (int r = 0; r < LG; ++r) pre[r] = (r < nsb && lane < L) ? x[(long)r * L + lane] : 0.0f;
    for (int j0 = 0; j0 < L; j0 += LT) {
        __syncthreads();  // the tile before this one has been walked
#pragma unroll
        for (int r = 0; r < LG; ++r) tile[r * LS + lane] = pre[r];
        __syncthreads();
        const int j1 = j0 + LT;
        if (j1 < L) {
#pragma unroll
            for (int r = 0; r < LG; ++r) pre[r] = (r < nsb && j1 + lane < L) ? x[(long)r * L + j1 + lane] : 0.0f;
        }
        if (live) {
            const int cnt = L - j0 < LT ? L - j0 : LT;
            const float* mine = tile + lane * LS;
            for (int j = 0; j < cnt; ++j) {
                const double y = kw_step(kw.k, s, (double)mine[j]);
                if (SECOND) acc += y * y;
            }
        }
    }
    if (!live) return;
    if (SECOND) {
        z[(long)b * ld + k0 + lane] = acc / (double)L;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) srow[i] = s[i];
    }
}

// states[b][k] holds the zero-state final state of sub-block k on entry, the true state at its start on exit.  One wave per row:
// 64 sub-blocks at a time through LDS, lane 0 walks them
__global__ __launch_bounds__(64) void loud_carry_kernel(const int64_t* __restrict__ n_in, long max_n, int L, KWeights kw,
                                                       double* __restrict__ states, long ld) {
    __shared__ double buf[64 * 4];
    const int lane = threadIdx.x, b = blockIdx.x;
    const long S = clamp_len(n_in, b, max_n) / L;
    double* row = states + (long)b * ld * 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};  // (lane 0's)
    for (long k0 = 0; k0 < S; k0 += 64) {
        const int cnt = (int)(S - k0 < 64 ? S - k0 : 64);
        if (lane < cnt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) buf[lane * 4 + i] = row[(k0 + lane) * 4 + i];
        }
        __syncthreads();
        if (lane == 0) {
            for (int k = 0; k < cnt; ++k) {
                double t[4], nx[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    t[i] = buf[k * 4 + i];
                    buf[k * 4 + i] = s[i];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    nx[r] = (((kw.M[r * 4] * s[0] + kw.M[r * 4 + 1] * s[1]) + kw.M[r * 4 + 2] * s[2]) + kw.M[r * 4 + 3] * s[3]) + t[r];
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i] = nx[i];
            }
        }
        __syncthreads();
        if (lane < cnt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) row[(k0 + lane) * 4 + i] = buf[lane * 4 + i];
        }
        __syncthreads();
    }
}

// ---- gating ----

// the sum of the workgroup's values in ascending thread order: every thread returns the same bits
__device__ __forceinline__ double block_sum(double v, double* sh, int tid) {
    __syncthreads();  // sh is free again
    sh[tid] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < GT_THREADS; ++i) t += sh[i];
    return t;
}

__device__ __forceinline__ double block_max(double v, double* sh, int tid) {
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    double t = sh[0];
    for (int i = 1; i < GT_THREADS; ++i) t = fmax(t, sh[i]);
    return t;
}

// the value of rank `rank` (0 = smallest) among the keys of this row that are not the all-ones mark: exact radix selection, one
// bit per pass from the top.  Keys are bit patterns of positive doubles: their order is the order of the values.
__device__ double select_rank(const unsigned long long* __restrict__ keys, long N3, long rank, unsigned* cnt_sh, int tid) {
    unsigned long long prefix = 0ull;
    for (int bit = 63; bit >= 0; --bit) {
        __syncthreads();
        if (tid == 0) *cnt_sh = 0u;
        __syncthreads();
        unsigned c = 0u;
        for (long j = tid; j < N3; j += GT_THREADS) c += ((keys[j] ^ prefix) >> bit) == 0ull ? 1u : 0u;  // high bits match, this bit 0
        if (c) atomicAdd(cnt_sh, c);
        __syncthreads();
        const long zeros = (long)*cnt_sh;
        if (rank >= zeros) {
            rank -= zeros;
            prefix |= 1ull << bit;
        }
    }
    return __longlong_as_double((long long)prefix);
}

__global__ __launch_bounds__(GT_THREADS) void loud_gate_kernel(const int64_t* __restrict__ n_in, long max_n, int L,
                                                              const double* __restrict__ z, double* __restrict__ ste, long ld,
                                                              const unsigned* __restrict__ peaks, double* __restrict__ values) {
    __shared__ double sh[GT_THREADS];
    __shared__ unsigned cnt_sh;
    const int tid = threadIdx.x, b = blockIdx.x;
    const long S = clamp_len(n_in, b, max_n) / L;
    const long N = S >= 4 ? S - 3 : 0, N3 = S >= 30 ? S - 29 : 0;
    const double* zr = z + (long)b * ld;
    double* st = ste + (long)b * ld;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double ninf = -HUGE_VAL;

    // integrated loudness: the absolute gate, the relative gate
    double sumA = 0.0, cntA = 0.0, mx = ninf;
    for (long j = tid; j < N; j += GT_THREADS) {
        const double e = (((zr[j] + zr[j + 1]) + zr[j + 2]) + zr[j + 3]) * 0.25;
        mx = fmax(mx, e);
        if (loud(e) > -70.0) {
            sumA += e;
            cntA += 1.0;
        }
    }
    sumA = block_sum(sumA, sh, tid);
    cntA = block_sum(cntA, sh, tid);
    mx = block_max(mx, sh, tid);
    const double gamma = loud(sumA / cntA) - 10.0;  // (not used when cntA == 0: nothing passes the absolute gate then)
    double sumK = 0.0, cntK = 0.0;
    for (long j = tid; j < N; j += GT_THREADS) {
        const double e = (((zr[j] + zr[j + 1]) + zr[j + 2]) + zr[j + 3]) * 0.25;
        const double l = loud(e);
        if (l > -70.0 && l > gamma) {
            sumK += e;
            cntK += 1.0;
        }
    }
    sumK = block_sum(sumK, sh, tid);
    cntK = block_sum(cntK, sh, tid);

    // loudness range: the short-term energies, their two gates, the kept ones as keys
    double sum3 = 0.0, cnt3 = 0.0, mx3 = ninf;
    for (long j = tid; j < N3; j += GT_THREADS) {
        double e = 0.0;
        for (int i = 0; i < 30; ++i) e += zr[j + i];
        e = e / 30.0;
        st[j] = e;
        mx3 = fmax(mx3, e);
        if (loud(e) > -70.0) {
            sum3 += e;
            cnt3 += 1.0;
        }
    }
    sum3 = block_sum(sum3, sh, tid);
    cnt3 = block_sum(cnt3, sh, tid);
    mx3 = block_max(mx3, sh, tid);
    const double g3 = loud(sum3 / cnt3) - 20.0;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(st);
    double kept3 = 0.0;
    for (long j = tid; j < N3; j += GT_THREADS) {  // (a thread reads back what it wrote itself)
        const double l = loud(st[j]);
        if (l > -70.0 && l > g3) kept3 += 1.0;
        else keys[j] = ~0ull;
    }
    kept3 = block_sum(kept3, sh, tid);
    double lra = nan;
    if (kept3 > 0.0) {  // (uniform over the workgroup)
        const long hi = (long)floor(__dadd_rn(__dmul_rn(0.95, kept3 - 1.0), 0.5));
        const long lo = (long)floor(__dadd_rn(__dmul_rn(0.10, kept3 - 1.0), 0.5));
        const double vhi = select_rank(keys, N3, hi, &cnt_sh, tid);
        const double vlo = select_rank(keys, N3, lo, &cnt_sh, tid);
        lra = loud(vhi) - loud(vlo);
    }
    if (tid == 0) {
        double* v = values + (long)b * SWC_LOUDNESS_VALUES;
        v[SWC_LOUDNESS_I] = cntK > 0.0 ? loud(sumK / cntK) : nan;
        v[SWC_LOUDNESS_LRA] = lra;
        v[SWC_LOUDNESS_MOMENTARY_MAX] = N > 0 ? loud(mx) : nan;
        v[SWC_LOUDNESS_SHORT_TERM_MAX] = N3 > 0 ? loud(mx3) : nan;
        v[SWC_LOUDNESS_SAMPLE_PEAK] = (double)__uint_as_float(peaks[2 * b]);
        v[SWC_LOUDNESS_TRUE_PEAK] = (double)__uint_as_float(peaks[2 * b + 1]);
        v[SWC_LOUDNESS_BLOCKS] = (double)N;
        v[SWC_LOUDNESS_BLOCKS_KEPT] = cntK;
    }
}

// ---- normalise ----

__global__ __launch_bounds__(NM_THREADS) void loud_normalise_kernel(const void* const* __restrict__ rows, const int64_t* __restrict__ n_in,
                                                                   const double* __restrict__ values, double target, double ceiling,
                                                                   float* __restrict__ out, long ld_out, long cols,
                                                                   float* __restrict__ gains, int* __restrict__ flags) {
    __shared__ float g_sh;
    const int tid = threadIdx.x, b = blockIdx.y;
    if (tid == 0) {
        const double I = values[(long)b * SWC_LOUDNESS_VALUES + SWC_LOUDNESS_I];
        const double tp = values[(long)b * SWC_LOUDNESS_VALUES + SWC_LOUDNESS_TRUE_PEAK];
        double g = 1.0;
        int fl = 0;
        if (I != I || !(tp > 0.0) || tp > 1.7976931348623157e308) {
            fl = SWC_LOUDNESS_UNMEASURED;
        } else {
            const double gt = pow(10.0, (target - I) / 20.0), gc = pow(10.0, ceiling / 20.0) / tp;
            g = gt;
            if (gc < gt) {
                g = gc;
                fl = SWC_LOUDNESS_PEAK_LIMITED;
            }
        }
        g_sh = (float)g;
        if (blockIdx.x == 0) {
            if (gains != nullptr) gains[b] = (float)g;
            if (flags != nullptr) flags[b] = fl;
        }
    }
    __syncthreads();
    if (out == nullptr) return;
    const float g = g_sh;
    long n = n_in[b];
    n = n < 0 ? 0 : (n > cols ? cols : n);
    const long j0 = (long)blockIdx.x * NM_TILE;
    const long jend = j0 + NM_TILE < cols ? j0 + NM_TILE : cols;
    float* orow = out + (long)b * ld_out;
    const float* x = reinterpret_cast<const float*>(rows[b]);  // (not read when n == 0)
    const bool vec = n > 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(orow)) & 15u) == 0;
    for (long j = j0 + tid * 4; j < jend; j += NM_THREADS * 4) {
        if (vec && j + 4 <= n) {  // (j is a multiple of 4: both addresses stay 16-byte aligned)
            const float4 q = *reinterpret_cast<const float4*>(x + j);
            *reinterpret_cast<float4*>(orow + j) = make_float4(__fmul_rn(q.x, g), __fmul_rn(q.y, g), __fmul_rn(q.z, g), __fmul_rn(q.w, g));
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (j + i < jend) orow[j + i] = j + i < n ? __fmul_rn(x[j + i], g) : 0.0f;
        }
    }
}

struct WsLayout {
    size_t peaks, states, z, ste, total;
};

// the workspace of B rows of at most S sub-blocks: one place for swc_loudness_workspace_bytes and swc_loudness
WsLayout ws_layout(int B, long S) {
    WsLayout P;
    size_t o = 0;
    P.peaks = o;  o += up256((size_t)2 * B * sizeof(unsigned));
    P.states = o; o += up256((size_t)B * S * 4 * sizeof(double));
    P.z = o;      o += up256((size_t)B * S * sizeof(double));
    P.ste = o;    o += up256((size_t)B * S * sizeof(double));
    P.total = o;
    return P;
}

}  // namespace

extern "C" int swc_loudness_coefficients(int32_t fs, double* k10) {
    if (!fs_ok(fs) || k10 == nullptr) return -1;
    coefficients(fs, k10);
    return 0;
}

extern "C" int64_t swc_loudness_workspace_bytes(int32_t B, int64_t max_n_in, int32_t fs) {
    if (B < 0 || B > 65535 || max_n_in < 0 || max_n_in > SWC_LOUDNESS_MAX_N || !fs_ok(fs)) return -1;
    return (int64_t)ws_layout(B, (long)(max_n_in / (fs / 10))).total;
}

extern "C" int swc_loudness(const void* const* x_rows, const int64_t* n_in, int64_t max_n_in, int32_t fs, int32_t width,
                            const float* taps_packed, const int32_t* tap_start, int32_t run, double* values, void* workspace,
                            int64_t workspace_bytes, int32_t B, void* stream) {
    SWC_CHECK_ARG(x_rows && n_in && taps_packed && tap_start && values && workspace, "swc_loudness: null pointer");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_loudness: B=%d (0..65535)", B);
    SWC_CHECK_ARG(max_n_in >= 0 && max_n_in <= SWC_LOUDNESS_MAX_N, "swc_loudness: max_n_in=%ld (0..2^30)", (long)max_n_in);
    SWC_CHECK_ARG(fs_ok(fs), "swc_loudness: fs=%d: a multiple of 10 in %d..%d", fs, SWC_LOUDNESS_MIN_FS, SWC_LOUDNESS_MAX_FS);
    SWC_CHECK_ARG(width >= 0 && width <= SWC_LOUDNESS_MAX_WIDTH, "swc_loudness: width=%d (0..%d)", width, SWC_LOUDNESS_MAX_WIDTH);
    SWC_CHECK_ARG(run >= 1 && run <= 2 * width + 1, "swc_loudness: table size: run=%d must be in 1..%d (2 width + 1)", run, 2 * width + 1);
    const int L = fs / 10;
    const long S = (long)(max_n_in / L);
    const WsLayout P = ws_layout(B, S);
    SWC_CHECK_ARG(workspace_bytes >= (int64_t)P.total, "swc_loudness: workspace of %ld bytes, %ld needed (swc_loudness_workspace_bytes)",
                  (long)workspace_bytes, (long)P.total);
    SWC_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "swc_loudness: workspace must be 256-byte aligned");
    if (B == 0) return SWC_OK;
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace);
    unsigned* peaks = reinterpret_cast<unsigned*>(ws + P.peaks);
    double* states = reinterpret_cast<double*>(ws + P.states);
    double* z = reinterpret_cast<double*>(ws + P.z);
    double* ste = reinterpret_cast<double*>(ws + P.ste);
    const long max_n = (long)max_n_in;
    KWeights kw;
    coefficients(fs, kw.k);
    transition(kw.k, L, kw.M);
    if (hipMemsetAsync(peaks, 0, (size_t)2 * B * sizeof(unsigned), st) != hipSuccess) {
        (void)hipGetLastError();
        swc_set_error("swc_loudness: clearing the peaks failed");
        return SWC_E_LAUNCH;
    }
    if (max_n > 0) {
        const long tiles = (max_n + PK_TILE - 1) / PK_TILE;
        const size_t lds = (size_t)(PK_TILE + 2 * width + 1 + 4 * run) * sizeof(float);
        hipLaunchKernelGGL(loud_peak_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(PK_THREADS), lds, st, x_rows, n_in, max_n,
                           (int)width, taps_packed, (const int*)tap_start, (int)run, peaks);
        SWC_CHECK_LAUNCH("swc_loudness (peaks)");
    }
    if (S > 0) {
        const dim3 grid((unsigned)((S + LG - 1) / LG), (unsigned)B);
        hipLaunchKernelGGL(loud_filter_kernel<false>, grid, dim3(LG), 0, st, x_rows, n_in, max_n, L, kw, states, z, S);
        SWC_CHECK_LAUNCH("swc_loudness (filter 1)");
        hipLaunchKernelGGL(loud_carry_kernel, dim3((unsigned)B), dim3(64), 0, st, n_in, max_n, L, kw, states, S);
        SWC_CHECK_LAUNCH("swc_loudness (carry)");
        hipLaunchKernelGGL(loud_filter_kernel<true>, grid, dim3(LG), 0, st, x_rows, n_in, max_n, L, kw, states, z, S);
        SWC_CHECK_LAUNCH("swc_loudness (filter 2)");
    }
    hipLaunchKernelGGL(loud_gate_kernel, dim3((unsigned)B), dim3(GT_THREADS), 0, st, n_in, max_n, L, (const double*)z, ste, S,
                       (const unsigned*)peaks, values);
    SWC_CHECK_LAUNCH("swc_loudness (gate)");
    return SWC_OK;
}

extern "C" int swc_loudness_normalise(const void* const* x_rows, const int64_t* n_in, const double* values, double target,
                                      double ceiling, float* out, int64_t ld_out, int64_t cols, float* gains, int32_t* flags,
                                      int32_t B, void* stream) {
    SWC_CHECK_ARG(x_rows && n_in && values, "swc_loudness_normalise: null pointer");
    SWC_CHECK_ARG(out || gains || flags, "swc_loudness_normalise: no output (out, gains and flags are null)");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_loudness_normalise: B=%d (0..65535)", B);
    SWC_CHECK_ARG(target == target && ceiling == ceiling && fabs(target) <= 1e3 && fabs(ceiling) <= 1e3,
                  "swc_loudness_normalise: target=%g LUFS, ceiling=%g dB: finite numbers expected", target, ceiling);
    SWC_CHECK_ARG(!out || (cols >= 0 && cols <= ld_out), "swc_loudness_normalise: cols=%ld must be in 0..ld_out=%ld", (long)cols,
                  (long)ld_out);
    if (B == 0) return SWC_OK;
    const long c = out ? (long)cols : 0;
    const long tiles = c > 0 ? (c + NM_TILE - 1) / NM_TILE : 1;
    SWC_CHECK_ARG(tiles <= 0x7fffffffL, "swc_loudness_normalise: cols too large");
    hipLaunchKernelGGL(loud_normalise_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(NM_THREADS), 0, (hipStream_t)stream, x_rows,
                       n_in, values, target, ceiling, c > 0 ? out : (float*)nullptr, (long)ld_out, c, gains, (int*)flags);
    SWC_CHECK_LAUNCH("swc_loudness_normalise");
    return SWC_OK;
}
