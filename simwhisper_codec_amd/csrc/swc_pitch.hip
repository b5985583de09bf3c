// swc_pitch (include/swc_pitch.h): the YIN F0 track of every row of a ragged batch and the pair measures built on it.  Three
// kinds of launch after one memset of the peaks, no workgroup waits for another:
//   pitch_peak_kernel    max |x| of every row as an unsigned maximum over the bit patterns of |x| (any NaN or Inf wins, the
//                        result is exact and does not depend on the order): one workgroup per 4096 samples.
//   pitch_frames_kernel  a workgroup of 256 threads takes SWC_PITCH_FRAMES_PER_GROUP consecutive frames of one row, one WAVE
//                        per frame; a wave works in an LDS region of its own.  It quantises the frame's span samples to int16
//                        (raw), and writes three packed views of them: the window as pairs (q[2k], q[2k+1]) split into a high
//                        and a low digit (q = 256 h + l, |h|, |l| <= 128), and the lagged side at both pair alignments,
//                        P1[k] = (q[2k+1], q[2k+2]) and Q[k] = (q[2k+2], q[2k+3]), interleaved in blocks of four dwords.
//                        Lane (m = lane / 2, p = lane % 2) owns the four lags tau = 1 + 256 pass + 8 m + p + 2 i: for all of
//                        them the lagged pairs of window pair j are X_p[j + 128 pass + 4 m + i], so per four window pairs it
//                        reads one 16-byte block of the window's two digits (the same address in every lane: a broadcast)
//                        and one new 16-byte block of X_p (consecutive lanes, consecutive blocks: conflict-free), and issues
//                        32 packed 16-bit dot products.  A digit's products stay below 2^23, so 128 window pairs fit an int32
//                        accumulator; then it is spilled into an int64 sum.  r(tau) = 256 sum_h + sum_l, and
//                        d(tau) = E(0) + E(tau) - 2 r(tau) with E(tau) = E(0) + sum_{k < tau} (q[W + k]^2 - q[k]^2).
//                        The second phase gives lane l the lags 1 + l K .. (l + 1) K, K = ceil(tau_max / 64): E and S are wave
//                        prefix sums of per-lane block sums (int64), the first lag below the threshold and the end of the
//                        descent are wave minima, d' is one float64 division per lag.
//                        Everything up to d' is integer arithmetic: any order gives the same bits.
//   pitch_pairs_kernel   one wave per row: counts and float64 sums over the stored f32 tracks in one fixed order.
// Every store to global memory is an ordinary vector store from plain C++.
#include "swc_metric_common.h"
#include "swc_pitch.h"

namespace {

constexpr int PT_WAVES = SWC_PITCH_FRAMES_PER_GROUP;
constexpr int PT_THREADS = 64 * PT_WAVES;
constexpr int PK_THREADS = 256;
constexpr int PK_CHUNK = 4096;     // samples per workgroup of the peak kernel
constexpr int PT_SPILL = 32;       // blocks of four window pairs between two spills: 128 pairs * 2 * 128 * 32767 < 2^31
static_assert(PT_SPILL * 4 * 2 * 128 * 32767LL < (1LL << 31), "a digit's dot products fit int32 between two spills");
static_assert((long long)SWC_PITCH_MAX_WORK * 65534LL * 65534LL < (1LL << 53), "d tau and S convert to double exactly");

__host__ __device__ __forceinline__ long frames_of(long n, int span, int H) { return n < span ? 0 : 1 + (n - span) / H; }

// where a wave keeps what inside its LDS region (bytes, every offset a multiple of 16); the host computes the same
struct Layout {
    int njb;      // blocks of four window pairs: ceil(W / 8)
    int passes;   // passes over 256 lags: ceil(tau_max / 256)
    int nbb;      // 16-byte blocks of ONE alignment of the lagged side: njb + 32 passes + 1
    int raw, ah, al, bb, r, total;
};

__host__ __device__ __forceinline__ Layout layout_of(int W, int tau_max) {
    Layout L;
    L.njb = (W + 7) / 8;
    L.passes = (tau_max + 255) / 256;
    L.nbb = L.njb + 32 * L.passes + 1;
    const int span = W + tau_max;
    L.raw = 0;
    L.ah = L.raw + ((span * 2 + 15) & ~15);
    L.al = L.ah + L.njb * 16;
    L.bb = L.al + L.njb * 16;
    L.r = L.bb + 2 * L.nbb * 16;
    L.total = L.r + (((tau_max + 2) * 8 + 15) & ~15);
    return L;
}

__global__ __launch_bounds__(PK_THREADS) void pitch_peak_kernel(const void* const* __restrict__ x_rows,
                                                                const void* const* __restrict__ y_rows,
                                                                const int64_t* __restrict__ n_in, long max_n,
                                                                unsigned* __restrict__ peaks, int B) {
    const int b = blockIdx.y, side = blockIdx.z, tid = threadIdx.x;
    const long n = clamp_len(n_in, b, max_n);
    const long i0 = (long)blockIdx.x * PK_CHUNK;
    if (i0 >= n) return;  // (an empty row: its address is not read)
    const unsigned* p = reinterpret_cast<const unsigned*>(side == 0 ? x_rows[b] : y_rows[b]);
    const long i1 = i0 + PK_CHUNK < n ? i0 + PK_CHUNK : n;
    unsigned m = 0;
    for (long i = i0 + tid; i < i1; i += PK_THREADS) {
        const unsigned v = p[i] & 0x7fffffffu;
        m = v > m ? v : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned v = (unsigned)__shfl_xor((int)m, o);
        m = v > m ? v : m;
    }
    if ((tid & 63) == 0 && m != 0) atomicMax(peaks + (long)side * B + b, m);
}

// exclusive prefix sum over the 64 lanes
__device__ __forceinline__ long long wave_scan_excl_i64(long long v, int lane) {
    long long s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_up(s, o);
        if (lane >= o) s += u;
    }
    return s - v;
}

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(v, o);
        v = u < v ? u : v;
    }
    return v;
}

__global__ __launch_bounds__(PT_THREADS) void pitch_frames_kernel(
    const void* const* __restrict__ x_rows, const void* const* __restrict__ y_rows, const int64_t* __restrict__ n_in, long max_n,
    int sr, int W, int tau_min, int tau_max, int H, const unsigned* __restrict__ peaks, int32_t* __restrict__ tau_x,
    float* __restrict__ f0_x, int32_t* __restrict__ tau_y, float* __restrict__ f0_y, long ldt, float* __restrict__ ws_f0, long ws_T,
    int B) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int b = blockIdx.y, side = blockIdx.z, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int span = W + tau_max;
    const long n = clamp_len(n_in, b, max_n);
    const long T = frames_of(n, span, H);
    const long t0 = (long)blockIdx.x * PT_WAVES;
    if (t0 >= T) return;  // uniform over the workgroup (an empty or short row: its address is not read)
    const bool active = t0 + wave < T;
    const long t = active ? t0 + wave : T - 1;  // a wave past the row's last frame repeats it and stores nothing
    int32_t* tau_out = side == 0 ? tau_x : tau_y;
    float* f0_out = side == 0 ? f0_x : f0_y;
    float* f0_ws = ws_f0 + ((long)side * B + b) * ws_T + t;
    if (tau_out != nullptr) tau_out += (long)b * ldt + t;
    if (f0_out != nullptr) f0_out += (long)b * ldt + t;
    const unsigned pk = peaks[(long)side * B + b];
    // a silent row, or one that is not defined (uniform over the workgroup).  !peak_defined(pk) spelled out: see swc_metric_common.h
    if (pk == 0u || pk >= 0x7f800000u) {
        if (active && lane == 0) {
            const float f = pk == 0u ? 0.0f : __builtin_nanf("");
            *f0_ws = f;
            if (f0_out != nullptr) *f0_out = f;
            if (tau_out != nullptr) *tau_out = pk == 0u ? 0 : -1;
        }
        return;
    }
    const int e = peak_exp(pk);
    const Layout L = layout_of(W, tau_max);
    unsigned char* base = lds + (size_t)wave * L.total;
    short* raw = reinterpret_cast<short*>(base + L.raw);
    unsigned* ah = reinterpret_cast<unsigned*>(base + L.ah);
    unsigned* al = reinterpret_cast<unsigned*>(base + L.al);
    unsigned* bb = reinterpret_cast<unsigned*>(base + L.bb);
    long long* R = reinterpret_cast<long long*>(base + L.r);   // r(tau), then d(tau), then d'(tau) as float64: [0 .. tau_max + 1]
    double* DP = reinterpret_cast<double*>(base + L.r);

    // ---- the frame, quantised ----
    const float* row = reinterpret_cast<const float*>(side == 0 ? x_rows[b] : y_rows[b]) + t * H;  // reads [0, span) of it
    for (int i = lane; i < span; i += 64) {
        raw[i] = (short)quantise(row[i], e);
    }
    __syncthreads();
    long long e0 = 0;
    for (int k = lane; k < 4 * L.njb; k += 64) {  // window pair k, zero past W
        const int a0 = 2 * k < W ? raw[2 * k] : 0, a1 = 2 * k + 1 < W ? raw[2 * k + 1] : 0;
        const int h0 = (a0 + 128) >> 8, h1 = (a1 + 128) >> 8;
        ah[k] = pack16(h0, h1);
        al[k] = pack16(a0 - 256 * h0, a1 - 256 * h1);
        e0 += (long long)(a0 * a0) + (long long)(a1 * a1);
    }
    for (int k = lane; k < 4 * L.nbb; k += 64) {  // lagged pairs at both alignments, zero past the span
        const int i1 = 2 * k + 1;
        const int q1 = i1 < span ? raw[i1] : 0, q2 = i1 + 1 < span ? raw[i1 + 1] : 0, q3 = i1 + 2 < span ? raw[i1 + 2] : 0;
        unsigned* blk = bb + (k >> 2) * 8 + (k & 3);
        blk[0] = pack16(q1, q2);
        blk[4] = pack16(q2, q3);
    }
    e0 = wave_sum_i64(e0);  // E(0)
    __syncthreads();

    // ---- r(tau) ----
    const int m = lane >> 1, p = lane & 1;
    const uint4* ah4 = reinterpret_cast<const uint4*>(ah);
    const uint4* al4 = reinterpret_cast<const uint4*>(al);
    const uint4* bb4 = reinterpret_cast<const uint4*>(bb);
    for (int pass = 0; pass < L.passes; ++pass) {
        const int kb = 32 * pass + m;  // jb + kb + 1 <= njb - 1 + 32 (passes - 1) + 31 + 1 = nbb - 1
        long long sh[4] = {0, 0, 0, 0}, sl[4] = {0, 0, 0, 0};
        for (int jb0 = 0; jb0 < L.njb; jb0 += PT_SPILL) {
            const int jb1 = jb0 + PT_SPILL < L.njb ? jb0 + PT_SPILL : L.njb;
            int ch[4] = {0, 0, 0, 0}, cl[4] = {0, 0, 0, 0};
            uint4 s0 = bb4[2 * (jb0 + kb) + p];
            for (int jb = jb0; jb < jb1; ++jb) {
                const uint4 s1 = bb4[2 * (jb + 1 + kb) + p];
                const uint4 vh = ah4[jb], vl = al4[jb];
                const unsigned s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
                const unsigned wh[4] = {vh.x, vh.y, vh.z, vh.w}, wl[4] = {vl.x, vl.y, vl.z, vl.w};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        ch[i] = dot2(wh[jj], s[jj + i], ch[i]);
                        cl[i] = dot2(wl[jj], s[jj + i], cl[i]);
                    }
                }
                s0 = s1;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                sh[i] += ch[i];
                sl[i] += cl[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int tau = 1 + 256 * pass + 8 * m + p + 2 * i;
            if (tau <= tau_max) R[tau] = 256 * sh[i] + sl[i];
        }
    }
    __syncthreads();

    // ---- d, S, the choice ----
    const int K = (tau_max + 63) / 64;
    const int ta = 1 + lane * K;
    const int tb = ta + K - 1 < tau_max ? ta + K - 1 : tau_max;  // the lane's lags ta .. tb (none when ta > tau_max)
    long long gsum = 0;
    for (int tau = ta; tau <= tb; ++tau) {
        const int hi = raw[W + tau - 1], lo = raw[tau - 1];
        gsum += (long long)(hi * hi) - (long long)(lo * lo);
    }
    long long E = e0 + wave_scan_excl_i64(gsum, lane);  // E(ta - 1)
    long long dsum = 0;
    for (int tau = ta; tau <= tb; ++tau) {
        const int hi = raw[W + tau - 1], lo = raw[tau - 1];
        E += (long long)(hi * hi) - (long long)(lo * lo);
        const long long d = e0 + E - 2 * R[tau];
        R[tau] = d;
        dsum += d;
    }
    long long S = wave_scan_excl_i64(dsum, lane);  // S(ta - 1)
    int first = 0x7fffffff;
    for (int tau = ta; tau <= tb; ++tau) {
        const long long d = R[tau];
        S += d;
        const long long dt = d * tau;
        if (tau >= tau_min && S > 0 && SWC_PITCH_THRESHOLD_DEN * dt < SWC_PITCH_THRESHOLD_NUM * S && first == 0x7fffffff) first = tau;
        DP[tau] = S > 0 ? __ddiv_rn((double)dt, (double)S) : 1.0;
    }
    first = wave_min_i32(first);
    __syncthreads();
    int c = 0;
    float f0 = 0.0f;
    if (first != 0x7fffffff) {  // uniform over the wave
        int stop = 0x7fffffff;
        for (int tau = ta > first ? ta : first; tau <= tb; ++tau) {
            if (!(tau + 1 <= tau_max && DP[tau + 1] < DP[tau])) {
                stop = tau;
                break;
            }
        }
        c = wave_min_i32(stop);  // (tau_max always stops)
        double off = 0.0;
        if (c + 1 <= tau_max) {
            const double a = DP[c - 1], bq = DP[c], g = DP[c + 1];  // c - 1 >= tau_min - 1 >= 1
            const double den = __dadd_rn(__dsub_rn(a, __dmul_rn(2.0, bq)), g);
            if (den > 0.0) {
                off = __ddiv_rn(__dmul_rn(0.5, __dsub_rn(a, g)), den);
                off = off > 1.0 ? 1.0 : (off < -1.0 ? -1.0 : off);
            }
        }
        f0 = (float)__ddiv_rn((double)sr, __dadd_rn((double)c, off));
    }
    if (active && lane == 0) {
        *f0_ws = f0;
        if (f0_out != nullptr) *f0_out = f0;
        if (tau_out != nullptr) *tau_out = c;
    }
}

// one wave per row: the counts, then the float64 sums over the stored tracks: lane l adds its frames l, l + 64, ... in
// ascending order, lane 0 adds the 64 partial sums in ascending lane order
__global__ __launch_bounds__(64) void pitch_pairs_kernel(const int64_t* __restrict__ n_in, long max_n, int span, int H,
                                                         const unsigned* __restrict__ peaks, const float* __restrict__ ws_f0,
                                                         long ws_T, int pair, float* __restrict__ values,
                                                         int32_t* __restrict__ counts, int B) {
    __shared__ double part[64][4];
    __shared__ double tot[4];
    const int b = blockIdx.x, lane = threadIdx.x;
    const long T = frames_of(clamp_len(n_in, b, max_n), span, H);
    const float* fx = ws_f0 + (long)b * ws_T;
    const float* fy = ws_f0 + ((long)B + b) * ws_T;
    const bool defined = peak_defined(peaks[b]) && (!pair || peak_defined(peaks[(long)B + b]));
    int n_vx = 0, n_vy = 0, n_vv = 0, n_diff = 0, n_gross = 0;
    double s_c2 = 0.0, s_x = 0.0, s_y = 0.0;
    if (defined) {
        for (long t = lane; t < T; t += 64) {
            const double x = (double)fx[t], y = pair ? (double)fy[t] : 0.0;
            const bool vx = x > 0.0, vy = y > 0.0;
            n_vx += vx;
            n_vy += vy;
            n_diff += vx != vy;
            if (vx && vy) {
                ++n_vv;
                const double ratio = __ddiv_rn(y, x);
                const double cents = __dmul_rn(1200.0, log2(ratio));
                s_c2 = __dadd_rn(s_c2, __dmul_rn(cents, cents));
                n_gross += fabs(__dsub_rn(ratio, 1.0)) > 0.2;
                s_x = __dadd_rn(s_x, x);
                s_y = __dadd_rn(s_y, y);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // (integers: any order)
        n_vx += __shfl_xor(n_vx, o);
        n_vy += __shfl_xor(n_vy, o);
        n_vv += __shfl_xor(n_vv, o);
        n_diff += __shfl_xor(n_diff, o);
        n_gross += __shfl_xor(n_gross, o);
    }
    part[lane][0] = s_c2;
    part[lane][1] = s_x;
    part[lane][2] = s_y;
    __syncthreads();
    if (lane < 3) {
        double s = part[0][lane];
        for (int i = 1; i < 64; ++i) s = __dadd_rn(s, part[i][lane]);
        tot[lane] = s;
    }
    __syncthreads();
    const double nan = __builtin_nan("");
    const double mx = n_vv > 0 ? __ddiv_rn(tot[1], (double)n_vv) : 0.0, my = n_vv > 0 ? __ddiv_rn(tot[2], (double)n_vv) : 0.0;
    double s_xx = 0.0, s_yy = 0.0, s_xy = 0.0;
    if (defined && pair) {
        for (long t = lane; t < T; t += 64) {
            const double x = (double)fx[t], y = (double)fy[t];
            if (x > 0.0 && y > 0.0) {
                const double dx = __dsub_rn(x, mx), dy = __dsub_rn(y, my);
                s_xx = __dadd_rn(s_xx, __dmul_rn(dx, dx));
                s_yy = __dadd_rn(s_yy, __dmul_rn(dy, dy));
                s_xy = __dadd_rn(s_xy, __dmul_rn(dx, dy));
            }
        }
    }
    const double c2 = tot[0];
    __syncthreads();  // tot and part are free again
    part[lane][0] = s_xx;
    part[lane][1] = s_yy;
    part[lane][2] = s_xy;
    __syncthreads();
    if (lane < 3) {
        double s = part[0][lane];
        for (int i = 1; i < 64; ++i) s = __dadd_rn(s, part[i][lane]);
        tot[lane] = s;
    }
    __syncthreads();
    if (lane != 0) return;
    if (counts != nullptr) {
        int32_t* c = counts + (long)b * SWC_PITCH_COUNTS;
        c[0] = (int32_t)T;
        c[1] = n_vx;
        c[2] = n_vy;
        c[3] = n_vv;
    }
    if (values != nullptr) {
        float* v = values + (long)b * SWC_PITCH_VALUES;
        const double sxx = tot[0], syy = tot[1], sxy = tot[2];
        const bool ok = defined;
        v[0] = (float)(ok && n_vv > 0 ? sqrt(__ddiv_rn(c2, (double)n_vv)) : nan);
        v[1] = (float)(ok && n_vv >= 2 && sxx > 0.0 && syy > 0.0 ? __ddiv_rn(sxy, sqrt(__dmul_rn(sxx, syy))) : nan);
        v[2] = (float)(ok && n_vv > 0 ? __ddiv_rn((double)n_gross, (double)n_vv) : nan);
        v[3] = (float)(ok && T > 0 ? __ddiv_rn((double)n_diff, (double)T) : nan);
        v[4] = (float)(ok && n_vx + n_vy > 0 ? __ddiv_rn(__dmul_rn(2.0, (double)n_vv), (double)(n_vx + n_vy)) : nan);
        v[5] = (float)(ok && T > 0 ? __ddiv_rn((double)n_vx, (double)T) : nan);
        v[6] = (float)(ok && T > 0 ? __ddiv_rn((double)n_vy, (double)T) : nan);
        v[7] = 0.0f;
    }
}

bool params_ok(int W, int tau_max, int H) {
    return W >= SWC_PITCH_MIN_WIN && W <= SWC_PITCH_MAX_WIN && tau_max > SWC_PITCH_MIN_TAU && tau_max <= SWC_PITCH_MAX_TAU &&
           (long)W * tau_max <= SWC_PITCH_MAX_WORK && H >= 1;
}

// where swc_pitch keeps what inside its workspace (byte offsets): the peaks [2][B] u32 and the f0 tracks [2][B][T] f32
struct WsLayout {
    size_t peaks, f0, total;
};

WsLayout ws_layout(int B, long T) {
    WsLayout P;
    size_t o = 0;
    P.peaks = o; o += up256((size_t)2 * B * sizeof(unsigned));
    P.f0 = o; o += up256((size_t)2 * B * (size_t)T * sizeof(float));
    P.total = o;
    return P;
}

}  // namespace

extern "C" int64_t swc_pitch_workspace_bytes(int32_t B, int64_t max_n_in, int32_t W, int32_t tau_max, int32_t H) {
    if (B < 0 || B > 65535 || max_n_in < 0 || !params_ok(W, tau_max, H)) return -1;
    const long T = frames_of(max_n_in, W + tau_max, H);
    if (T >= 0x7fffffffL) return -1;
    return (int64_t)ws_layout(B, T).total;
}

extern "C" int swc_pitch(const void* const* x_rows, const void* const* y_rows, const int64_t* n_in, int64_t max_n_in, int32_t sr,
                         int32_t W, int32_t tau_min, int32_t tau_max, int32_t H, int32_t* tau_x, float* f0_x, int32_t* tau_y,
                         float* f0_y, int64_t ldt, float* values, int32_t* counts, void* workspace, int64_t workspace_bytes,
                         int32_t B, void* stream) {
    SWC_CHECK_ARG(x_rows && n_in && workspace, "swc_pitch: null pointer");
    SWC_CHECK_ARG(y_rows || !(values || tau_y || f0_y), "swc_pitch: values, tau_y and f0_y need y_rows");
    SWC_CHECK_ARG(tau_x || f0_x || tau_y || f0_y || values || counts, "swc_pitch: no output (every track, values and counts are null)");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_pitch: B=%d (0..65535)", B);
    SWC_CHECK_ARG(max_n_in >= 0, "swc_pitch: max_n_in=%ld out of range", (long)max_n_in);
    SWC_CHECK_ARG(sr >= 1, "swc_pitch: sr=%d", sr);
    SWC_CHECK_ARG(W >= SWC_PITCH_MIN_WIN && W <= SWC_PITCH_MAX_WIN, "swc_pitch: window W=%d (%d..%d)", W, SWC_PITCH_MIN_WIN,
                  SWC_PITCH_MAX_WIN);
    SWC_CHECK_ARG(tau_min >= SWC_PITCH_MIN_TAU && tau_min < tau_max && tau_max <= SWC_PITCH_MAX_TAU,
                  "swc_pitch: lags tau_min=%d, tau_max=%d (%d <= tau_min < tau_max <= %d)", tau_min, tau_max, SWC_PITCH_MIN_TAU,
                  SWC_PITCH_MAX_TAU);
    SWC_CHECK_ARG((long)W * tau_max <= SWC_PITCH_MAX_WORK, "swc_pitch: W * tau_max = %ld (at most %d)", (long)W * tau_max,
                  SWC_PITCH_MAX_WORK);
    SWC_CHECK_ARG(H >= 1, "swc_pitch: hop H=%d", H);
    const int span = W + tau_max;
    const long T = frames_of(max_n_in, span, H);
    SWC_CHECK_ARG(T < 0x7fffffffL, "swc_pitch: max_n_in=%ld gives 2^31 frames or more", (long)max_n_in);
    SWC_CHECK_ARG(!(tau_x || f0_x || tau_y || f0_y) || ldt >= T, "swc_pitch: ldt=%ld, %ld frames at max_n_in", (long)ldt, T);
    const WsLayout P = ws_layout(B, T);
    SWC_CHECK_ARG(workspace_bytes >= (int64_t)P.total, "swc_pitch: workspace of %ld bytes, %ld needed (swc_pitch_workspace_bytes)",
                  (long)workspace_bytes, (long)P.total);
    SWC_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "swc_pitch: workspace must be 256-byte aligned");
    if (B == 0) return SWC_OK;
    hipStream_t st = (hipStream_t)stream;
    const int sides = y_rows != nullptr ? 2 : 1;
    unsigned char* base = reinterpret_cast<unsigned char*>(workspace);
    unsigned* peaks = reinterpret_cast<unsigned*>(base + P.peaks);
    float* ws_f0 = reinterpret_cast<float*>(base + P.f0);
    const long max_n = max_n_in;
    if (hipMemsetAsync(peaks, 0, (size_t)2 * B * sizeof(unsigned), st) != hipSuccess) {
        (void)hipGetLastError();
        swc_set_error("swc_pitch: clearing the peaks failed");
        return SWC_E_LAUNCH;
    }
    if (max_n > 0) {
        const long chunks = (max_n + PK_CHUNK - 1) / PK_CHUNK;
        hipLaunchKernelGGL(pitch_peak_kernel, dim3((unsigned)chunks, (unsigned)B, (unsigned)sides), dim3(PK_THREADS), 0, st, x_rows,
                           y_rows, n_in, max_n, peaks, B);
        SWC_CHECK_LAUNCH("swc_pitch (peak)");
    }
    if (T > 0) {
        const Layout L = layout_of(W, tau_max);
        const int lds_bytes = L.total * PT_WAVES;
        if (lds_bytes > 65536) SWC_ENABLE_LDS(pitch_frames_kernel, 160 * 1024, "swc_pitch");
        const long groups = (T + PT_WAVES - 1) / PT_WAVES;
        hipLaunchKernelGGL(pitch_frames_kernel, dim3((unsigned)groups, (unsigned)B, (unsigned)sides), dim3(PT_THREADS), lds_bytes, st,
                           x_rows, y_rows, n_in, max_n, sr, W, tau_min, tau_max, H, (const unsigned*)peaks, tau_x, f0_x, tau_y, f0_y,
                           (long)ldt, ws_f0, T, B);
        SWC_CHECK_LAUNCH("swc_pitch (frames)");
    }
    if (values != nullptr || counts != nullptr) {
        hipLaunchKernelGGL(pitch_pairs_kernel, dim3((unsigned)B), dim3(64), 0, st, n_in, max_n, span, H, (const unsigned*)peaks,
                           (const float*)ws_f0, T, sides == 2 ? 1 : 0, values, counts, B);
        SWC_CHECK_LAUNCH("swc_pitch (pairs)");
    }
    return SWC_OK;
}
