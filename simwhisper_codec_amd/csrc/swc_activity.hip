// Speech activity on the device (include/swc_activity.h): the ITU-T P.56 active level, the long-term level, the activity
// factor, the sample peak and the runs of active samples of every row of a ragged batch, and the normalising gain computed and
// applied without a read-back.
//
// The envelope is a two-stage recursion with the pole g = exp(-1 / (0.03 fs)) (0.9979 at 16 kHz), so a row cannot simply be
// cut into independent pieces.  It is linear, though: the state (p, q) at the end of a sub-block of AL = 256 samples is
// M s + (the state the sub-block leaves when it starts from zero), M the 2 x 2 transition over AL samples of silence (the
// three-pass structure of swc_loudness.hip).  Nine launches:
//   filter 0 (S/64 x rows)   one lane per sub-block filters |x| from zero state and leaves the final state
//   carry    (rows)          s_{k+1} = M s_k + zs_k along the row: the true state at the start of every sub-block
//   filter 1 (S/64 x rows)   again from the true state: one byte per sample, the number of thresholds c_j = 2^(j - 15) that q
//                            reaches (read off the exponent of q: exact), and the sub-block's sum of squares and peak
//   window 0 (tiles x rows)  the sliding maximum of that byte over I + 1 samples; the thresholds are nested, so the one
//                            maximum gives all fifteen counts a_j of a tile
//   level    (rows)          sq, the peak, the a_j, the walk over j: A, L, the factor, c*
//   filter 2 (S/64 x rows)   once more from the true state (the same arithmetic, the same bits): one byte per sample, q >= c*
//   window 1 (tiles x rows)  the sliding maximum of that mask: starts, ends and active samples of a tile
//   scan     (rows)          exclusive scan of the tiles' starts and ends along the row; the two counts of the row
//   window 2 (tiles x rows)  the same maximum again; every start and end goes to its place in the run list
// The filter passes stage tiles of 64 sub-blocks x 64 samples through LDS as loud_filter_kernel does: the global reads are runs
// of 64 consecutive floats, the lanes then walk their own sub-block out of LDS (stride 65 words: no bank conflict), the bytes
// go back through the same tile and leave as runs of 64 consecutive bytes.  The sliding maximum over W = I + 1 samples is built
// in LDS by doubling (windows of 1, 2, 4, ... samples, then two overlapping windows of the largest power of two under W): every
// step is a byte-wise maximum of two shifted copies, in two buffers that swap roles.  The segmentation is fixed by constants:
// nothing depends on the grid.  No atomic, no scratch.
#include "swc_metric_common.h"
#include "swc_activity.h"
#include <math.h>

namespace {

constexpr int AL = SWC_ACTIVITY_SUBBLOCK;  // samples per sub-block
constexpr int AG = SWC_ACTIVITY_GROUP;     // sub-blocks per workgroup of a filter pass = lanes of its one wave
constexpr int AT = 64;                     // samples of every sub-block per LDS tile
constexpr int AS = AT + 1;                 // LDS row stride in words
constexpr int WT = SWC_ACTIVITY_TILE;      // output samples per workgroup of a window pass
constexpr int WN = SWC_ACTIVITY_THREADS;
constexpr int WP = WT / WN;                // consecutive samples per lane in the run passes
constexpr int NJ = SWC_ACTIVITY_THRESHOLDS;
constexpr int NV = SWC_ACTIVITY_VALUES;
constexpr int NM_THREADS = 256;
constexpr int NM_TILE = 4096;              // output columns per workgroup of the normalise kernel
static_assert(AL % AT == 0 && AG == 64 && AT == 64 && WT % WN == 0, "tile shapes");

struct EnvCoef {
    double g, om;  // the pole and 1 - g
    double M[4];   // the state transition over AL samples of silence, row-major over (p, q)
};

__host__ __device__ __forceinline__ void env_step(double g, double om, double& p, double& q, double ax) {
    p = g * p + om * ax;
    q = g * q + om * p;
}

bool fs_ok(int fs) { return fs >= SWC_ACTIVITY_MIN_FS && fs <= SWC_ACTIVITY_MAX_FS; }

// I = floor(hangover_s fs + 0.5), or -1 for a hangover the header refuses
long hangover_samples(int fs, double hangover_s) {
    if (!(hangover_s >= 0.0 && hangover_s <= 10.0)) return -1;
    const double v = floor(hangover_s * (double)fs + 0.5);
    return v <= (double)SWC_ACTIVITY_MAX_HANGOVER ? (long)v : -1;
}

EnvCoef coefficients(int fs) {
    EnvCoef c;
    c.g = exp(-1.0 / ((double)fs * 0.03));
    c.om = 1.0 - c.g;
    for (int col = 0; col < 2; ++col) {  // column col is what AL silent samples leave of the unit state e_col
        double p = col == 0 ? 1.0 : 0.0, q = col == 1 ? 1.0 : 0.0;
        for (int i = 0; i < AL; ++i) env_step(c.g, c.om, p, q, 0.0);
        c.M[col] = p;
        c.M[2 + col] = q;
    }
    return c;
}

// ---- the three filter passes ----

// MODE 0: from zero state, leaves the final state.  MODE 1: from the true state, leaves the level byte of every sample, the
// sub-block's sum of squares and peak.  MODE 2: from the true state, leaves the byte q >= c* of every sample
template <int MODE>
__global__ __launch_bounds__(AG) void act_filter_kernel(const void* const* __restrict__ rows, const int64_t* __restrict__ n_in,
                                                       long max_n, EnvCoef co, double* __restrict__ states, double* __restrict__ sqk,
                                                       unsigned* __restrict__ pkk, long ld, unsigned char* __restrict__ lev, long ldl,
                                                       const double* __restrict__ values) {
    __shared__ unsigned tile[AG * AS];
    const int lane = threadIdx.x, b = blockIdx.y;
    const long n = clamp_len(n_in, b, max_n);
    const long S = (n + AL - 1) / AL;
    const long k0 = (long)blockIdx.x * AG;
    if (k0 >= S) return;  // (uniform over the workgroup)
    const int nsb = (int)(S - k0 < AG ? S - k0 : AG);
    const bool live = lane < nsb;
    const long rem = n - k0 * AL;  // samples of the row from this workgroup's first sub-block on: 0 < rem, rem <= nsb AL
    const float* x = reinterpret_cast<const float*>(rows[b]) + k0 * AL;  // sub-block k0 + r, sample j: x[r AL + j], read below rem
    double* srow = states + ((long)b * ld + k0 + lane) * 2;
    double p = 0.0, q = 0.0;
    if (MODE != 0 && live) {
        p = srow[0];
        q = srow[1];
    }
    const double cstar = MODE == 2 ? values[(long)b * NV + SWC_ACTIVITY_THRESHOLD] : 0.0;  // (NaN: no sample is at or above it)
    unsigned char* lrow = lev + (long)b * ldl + k0 * AL;
    double acc = 0.0;
    unsigned pk = 0u;
    float pre[AG];
#pragma unroll
    for (int r = 0; r < AG; ++r) pre[r] = (long)r * AL + lane < rem ? x[(long)r * AL + lane] : 0.0f;
    for (int j0 = 0; j0 < AL; j0 += AT) {
        __syncthreads();  // the tile before this one has been walked and written out
#pragma unroll
        for (int r = 0; r < AG; ++r) tile[r * AS + lane] = __float_as_uint(pre[r]);
        __syncthreads();
        const int j1 = j0 + AT;
        if (j1 < AL) {
#pragma unroll
            for (int r = 0; r < AG; ++r) pre[r] = (long)r * AL + j1 + lane < rem ? x[(long)r * AL + j1 + lane] : 0.0f;
        }
        if (live) {
            unsigned* mine = tile + lane * AS;
            for (int j = 0; j < AT; ++j) {
                const float xv = __uint_as_float(mine[j]);
                env_step(co.g, co.om, p, q, (double)fabsf(xv));
                if (MODE == 1) {
                    acc += (double)xv * (double)xv;
                    pk = max(pk, __float_as_uint(fabsf(xv)));
                    // q >= 2^(j - 15) for j = 0 .. e + 15, e the exponent of q: the count of thresholds reached, 0 .. 15
                    const int e = (int)((__double_as_longlong(q) >> 52) & 0x7ff) - 1023 + 16;
                    mine[j] = (unsigned)(e < 0 ? 0 : (e > NJ ? NJ : e));
                }
                if (MODE == 2) mine[j] = q >= cstar ? 1u : 0u;
            }
        }
        if (MODE != 0) {
            __syncthreads();
            for (int r = 0; r < nsb; ++r) {
                const long i = (long)r * AL + j0 + lane;  // (j0 + lane < AL: AL is a multiple of AT)
                if (i < rem) lrow[i] = (unsigned char)tile[r * AS + lane];
            }
        }
    }
    if (!live) return;
    if (MODE == 0) {
        srow[0] = p;
        srow[1] = q;
    }
    if (MODE == 1) {
        sqk[(long)b * ld + k0 + lane] = acc;
        pkk[(long)b * ld + k0 + lane] = pk;
    }
}

// states[b][k] holds the zero-state final state of sub-block k on entry, the true state at its start on exit.  One wave per row:
// 64 sub-blocks at a time through LDS, lane 0 walks them
__global__ __launch_bounds__(64) void act_carry_kernel(const int64_t* __restrict__ n_in, long max_n, EnvCoef co,
                                                      double* __restrict__ states, long ld) {
    __shared__ double buf[AG * 2];
    const int lane = threadIdx.x, b = blockIdx.x;
    const long S = (clamp_len(n_in, b, max_n) + AL - 1) / AL;
    double* row = states + (long)b * ld * 2;
    double p = 0.0, q = 0.0;  // (lane 0's)
    for (long k0 = 0; k0 < S; k0 += AG) {
        const int cnt = (int)(S - k0 < AG ? S - k0 : AG);
        if (lane < cnt) {
            buf[lane * 2] = row[(k0 + lane) * 2];
            buf[lane * 2 + 1] = row[(k0 + lane) * 2 + 1];
        }
        __syncthreads();
        if (lane == 0) {
            for (int k = 0; k < cnt; ++k) {
                const double zp = buf[k * 2], zq = buf[k * 2 + 1];
                buf[k * 2] = p;
                buf[k * 2 + 1] = q;
                const double np = (co.M[0] * p + co.M[1] * q) + zp;
                const double nq = (co.M[2] * p + co.M[3] * q) + zq;
                p = np;
                q = nq;
            }
        }
        __syncthreads();
        if (lane < cnt) {
            row[(k0 + lane) * 2] = buf[lane * 2];
            row[(k0 + lane) * 2 + 1] = buf[lane * 2 + 1];
        }
        __syncthreads();
    }
}

// ---- the sliding-window passes ----

// The maximum of lev over [i - I, i] for the samples i = t0 - 1 .. t0 + WT of the row (bytes outside [0, n) count as 0), in
// LDS: local index u stands for sample t0 - 1 - I + u, u in [0, span), span = WT + I + 2; what comes back holds the maximum at
// every u >= I.  Two buffers of span bytes.
__device__ __forceinline__ const unsigned char* window_max(const unsigned char* __restrict__ lrow, long n, long t0, int I, int span,
                                                           unsigned char* a, unsigned char* bq, int tid) {
    const long base = t0 - 1 - I;
    for (int u = tid; u < span; u += WN) {
        const long i = base + u;
        a[u] = (i >= 0 && i < n) ? lrow[i] : (unsigned char)0;
    }
    __syncthreads();
    const int W = I + 1;
    unsigned char *src = a, *dst = bq;
    int P = 1;  // src[u] = the maximum over the P samples that end at u
    while (2 * P <= W) {
        for (int u = tid; u < span; u += WN) {
            const unsigned char v = src[u], w = u >= P ? src[u - P] : (unsigned char)0;
            dst[u] = v > w ? v : w;
        }
        __syncthreads();
        unsigned char* t = src;
        src = dst;
        dst = t;
        P *= 2;
    }
    const int sh = W - P;  // 0 <= sh < P: two windows of P samples cover the W
    if (sh == 0) return src;
    for (int u = tid; u < span; u += WN) {
        const unsigned char v = src[u], w = u >= sh ? src[u - sh] : (unsigned char)0;
        dst[u] = v > w ? v : w;
    }
    __syncthreads();
    return dst;
}

// MODE 0: the fifteen counts of the tile -> acnt[b][tile][16].  MODE 1: the tile's starts, ends and active samples ->
// rcnt[b][tile][4].  MODE 2: rcnt holds the exclusive scans of the starts and ends; the boundaries go into the run list
template <int MODE>
__global__ __launch_bounds__(WN) void act_window_kernel(const int64_t* __restrict__ n_in, long max_n, int I,
                                                       const unsigned char* __restrict__ lev, long ldl, unsigned* __restrict__ acnt,
                                                       unsigned* __restrict__ rcnt, long NT, int64_t* __restrict__ runs, long ld_runs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wbuf[];
    __shared__ unsigned red[3][WN];
    __shared__ unsigned tot[3];
    const int tid = threadIdx.x, b = blockIdx.y;
    const long n = clamp_len(n_in, b, max_n);
    const long t0 = (long)blockIdx.x * WT;
    if (t0 >= n) return;  // (uniform over the workgroup)
    const int span = WT + I + 2;
    const int half = (span + 15) & ~15;
    const unsigned char* m = window_max(lev + (long)b * ldl, n, t0, I, span, wbuf, wbuf + half, tid);
    const long slot = (long)b * NT + blockIdx.x;
    if (MODE == 0) {
        unsigned c[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) c[j] = 0u;
        for (int o = tid; o < WT; o += WN) {
            if (t0 + o < n) {
                const unsigned v = m[I + 1 + o];
#pragma unroll
                for (int j = 0; j < NJ; ++j) c[j] += v > (unsigned)j ? 1u : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c[j] += (unsigned)__shfl_xor((int)c[j], o);
            if ((tid & 63) == j) red[0][(tid >> 6) * 16 + j] = c[j];
        }
        __syncthreads();
        if (tid < NJ) acnt[slot * 16 + tid] = ((red[0][tid] + red[0][16 + tid]) + red[0][32 + tid]) + red[0][48 + tid];
        return;
    }
    // a lane looks at WP consecutive samples: a start is an active sample behind an inactive one (or at 0), an end an active
    // sample in front of an inactive one (or at n - 1)
    unsigned ns = 0u, ne = 0u, na = 0u;
    unsigned smask = 0u, emask = 0u;
    const int o0 = tid * WP;
#pragma unroll
    for (int k = 0; k < WP; ++k) {
        const long i = t0 + o0 + k;
        const int u = I + 1 + o0 + k;
        const bool act = i < n && m[u] != 0;
        const bool prev = i > 0 && m[u - 1] != 0;
        const bool next = i + 1 < n && m[u + 1] != 0;
        if (act) {
            ++na;
            if (!prev) { ++ns; smask |= 1u << k; }
            if (!next) { ++ne; emask |= 1u << k; }
        }
    }
    red[0][tid] = ns;
    red[1][tid] = ne;
    red[2][tid] = na;
    __syncthreads();
    if (tid < 3) {  // exclusive scan in lane order (WN entries: a few hundred LDS reads, once per tile)
        unsigned s = 0u;
        for (int t = 0; t < WN; ++t) {
            const unsigned v = red[tid][t];
            red[tid][t] = s;
            s += v;
        }
        tot[tid] = s;
    }
    __syncthreads();
    if (MODE == 1) {
        if (tid < 3) rcnt[slot * 4 + tid] = tot[tid];
        return;
    }
    long rs = (long)rcnt[slot * 4] + red[0][tid], re = (long)rcnt[slot * 4 + 1] + red[1][tid];
    int64_t* rrow = runs + (long)b * ld_runs * 2;
#pragma unroll
    for (int k = 0; k < WP; ++k) {
        const long i = t0 + o0 + k;
        if ((smask >> k) & 1u) {
            if (rs < ld_runs) rrow[rs * 2] = i;
            ++rs;
        }
        if ((emask >> k) & 1u) {
            if (re < ld_runs) rrow[re * 2 + 1] = i + 1;
            ++re;
        }
    }
}

// starts and ends of the tiles of a row -> their exclusive scans in place; the row's active samples and runs -> values
__global__ __launch_bounds__(64) void act_scan_kernel(const int64_t* __restrict__ n_in, long max_n, unsigned* __restrict__ rcnt,
                                                     long NT, double* __restrict__ values) {
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    const long tiles = (clamp_len(n_in, b, max_n) + WT - 1) / WT;
    unsigned* r = rcnt + (long)b * NT * 4;
    unsigned os = 0u, oe = 0u;
    long long act = 0;
    for (long t = 0; t < tiles; ++t) {
        const unsigned s = r[t * 4], e = r[t * 4 + 1];
        act += r[t * 4 + 2];
        r[t * 4] = os;
        r[t * 4 + 1] = oe;
        os += s;
        oe += e;
    }
    values[(long)b * NV + SWC_ACTIVITY_ACTIVE_SAMPLES] = (double)act;
    values[(long)b * NV + SWC_ACTIVITY_RUNS] = (double)os;
}

// ---- the levels ----

__global__ __launch_bounds__(WN) void act_level_kernel(const int64_t* __restrict__ n_in, long max_n, double margin,
                                                      const double* __restrict__ sqk, const unsigned* __restrict__ pkk, long ld,
                                                      const unsigned* __restrict__ acnt, long NT, double* __restrict__ values,
                                                      int64_t* __restrict__ counts) {
    __shared__ double sh[WN];
    __shared__ unsigned shp[WN];
    __shared__ long long a_sh[NJ];
    const int tid = threadIdx.x, b = blockIdx.x;
    const long n = clamp_len(n_in, b, max_n);
    const long S = (n + AL - 1) / AL, tiles = (n + WT - 1) / WT;
    double s = 0.0;
    unsigned pk = 0u;
    for (long k = tid; k < S; k += WN) {
        s += sqk[(long)b * ld + k];
        pk = max(pk, pkk[(long)b * ld + k]);
    }
    sh[tid] = s;
    shp[tid] = pk;
    if (tid < NJ) {
        long long a = 0;
        for (long t = 0; t < tiles; ++t) a += acnt[((long)b * NT + t) * 16 + tid];
        a_sh[tid] = a;
        counts[(long)b * NJ + tid] = a;
    }
    __syncthreads();
    if (tid != 0) return;
    double sq = 0.0;
    for (int i = 0; i < WN; ++i) {  // ascending lane order
        sq += sh[i];
        pk = max(pk, shp[i]);
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double A = nan, Lv = nan, fac = nan, cs = nan, jx = nan;
    if (n > 0 && sq > 0.0) {
        Lv = 10.0 * log10(sq / (double)n);
        double Ap = 0.0, Dp = 0.0;
        for (int j = 0; j < NJ; ++j) {
            const long long a = a_sh[j];
            if (a == 0) break;
            const double Aj = 10.0 * log10(sq / (double)a);
            const double Dj = Aj - 20.0 * log10(ldexp(1.0, j - 15));
            if (Dj <= margin) {
                if (j == 0 || Dj == margin) {
                    A = Aj;
                } else {
                    const double t = (Dp - margin) / (Dp - Dj);
                    A = Ap + t * (Aj - Ap);
                }
                jx = (double)j;
                break;
            }
            Ap = Aj;
            Dp = Dj;
        }
        if (A == A) {
            fac = pow(10.0, (Lv - A) / 10.0);
            cs = pow(10.0, (A - margin) / 20.0);
        }
    }
    double* v = values + (long)b * NV;
    v[SWC_ACTIVITY_ACTIVE_LEVEL] = A;
    v[SWC_ACTIVITY_LONG_TERM] = Lv;
    v[SWC_ACTIVITY_FACTOR] = fac;
    v[SWC_ACTIVITY_THRESHOLD] = cs;
    v[SWC_ACTIVITY_SAMPLE_PEAK] = (double)__uint_as_float(pk);
    v[SWC_ACTIVITY_CROSSING] = jx;
}

// ---- normalise ----

__global__ __launch_bounds__(NM_THREADS) void act_normalise_kernel(const void* const* __restrict__ rows, const int64_t* __restrict__ n_in,
                                                                  const double* __restrict__ values, double target,
                                                                  float* __restrict__ out, long ld_out, long cols,
                                                                  float* __restrict__ gains, int* __restrict__ flags) {
    __shared__ float g_sh;
    const int tid = threadIdx.x, b = blockIdx.y;
    if (tid == 0) {
        const double A = values[(long)b * NV + SWC_ACTIVITY_ACTIVE_LEVEL];
        const double pk = values[(long)b * NV + SWC_ACTIVITY_SAMPLE_PEAK];
        double g = 1.0;
        int fl = 0;
        if (A != A || !(pk > 0.0) || pk > 1.7976931348623157e308) {
            fl = SWC_ACTIVITY_UNMEASURED;
        } else {
            const double gt = pow(10.0, (target - A) / 20.0), gc = 1.0 / pk;
            g = gt;
            if (gc < gt) {
                g = gc;
                fl = SWC_ACTIVITY_PEAK_LIMITED;
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
            const float4 v = *reinterpret_cast<const float4*>(x + j);
            *reinterpret_cast<float4*>(orow + j) = make_float4(__fmul_rn(v.x, g), __fmul_rn(v.y, g), __fmul_rn(v.z, g), __fmul_rn(v.w, g));
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (j + i < jend) orow[j + i] = j + i < n ? __fmul_rn(x[j + i], g) : 0.0f;
        }
    }
}

struct WsLayout {
    size_t states, sqk, pkk, lev, acnt, rcnt, total;
    long S, NT, ldl;
};

// the workspace of B rows of at most max_n samples: one place for swc_activity_workspace_bytes and swc_activity
WsLayout ws_layout(int B, long max_n) {
    WsLayout P;
    P.S = (max_n + AL - 1) / AL;
    P.NT = (max_n + WT - 1) / WT;
    P.ldl = (long)up256((size_t)max_n);
    size_t o = 0;
    P.states = o; o += up256((size_t)B * P.S * 2 * sizeof(double));
    P.sqk = o;    o += up256((size_t)B * P.S * sizeof(double));
    P.pkk = o;    o += up256((size_t)B * P.S * sizeof(unsigned));
    P.lev = o;    o += up256((size_t)B * P.ldl);
    P.acnt = o;   o += up256((size_t)B * P.NT * 16 * sizeof(unsigned));
    P.rcnt = o;   o += up256((size_t)B * P.NT * 4 * sizeof(unsigned));
    P.total = o;
    return P;
}

}  // namespace

extern "C" int swc_activity_coefficients(int32_t fs, double hangover_s, double* g, int32_t* hangover, int32_t* subblock, double* m4) {
    if (!fs_ok(fs) || g == nullptr || hangover == nullptr || subblock == nullptr || m4 == nullptr) return -1;
    const long I = hangover_samples(fs, hangover_s);
    if (I < 0) return -1;
    const EnvCoef c = coefficients(fs);
    *g = c.g;
    *hangover = (int32_t)I;
    *subblock = AL;
    for (int i = 0; i < 4; ++i) m4[i] = c.M[i];
    return 0;
}

extern "C" int64_t swc_activity_workspace_bytes(int32_t B, int64_t max_n_in, int32_t fs) {
    if (B < 0 || B > 65535 || max_n_in < 0 || max_n_in > SWC_ACTIVITY_MAX_N || !fs_ok(fs)) return -1;
    return (int64_t)ws_layout(B, (long)max_n_in).total;
}

extern "C" int swc_activity(const void* const* x_rows, const int64_t* n_in, int64_t max_n_in, int32_t fs, double margin_db,
                            double hangover_s, double* values, int64_t* counts, int64_t* runs, int64_t ld_runs, void* workspace,
                            int64_t workspace_bytes, int32_t B, void* stream) {
    SWC_CHECK_ARG(x_rows && n_in && values && counts && runs && workspace, "swc_activity: null pointer");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_activity: B=%d (0..65535)", B);
    SWC_CHECK_ARG(max_n_in >= 0 && max_n_in <= SWC_ACTIVITY_MAX_N, "swc_activity: max_n_in=%ld (0..2^30)", (long)max_n_in);
    SWC_CHECK_ARG(fs_ok(fs), "swc_activity: fs=%d: an integer in %d..%d", fs, SWC_ACTIVITY_MIN_FS, SWC_ACTIVITY_MAX_FS);
    SWC_CHECK_ARG(margin_db > 0.0 && margin_db <= 100.0, "swc_activity: margin_db=%g: a number in (0, 100]", margin_db);
    const long I = hangover_samples(fs, hangover_s);
    SWC_CHECK_ARG(I >= 0, "swc_activity: hangover_s=%g: 0 .. %d samples at fs=%d", hangover_s, SWC_ACTIVITY_MAX_HANGOVER, fs);
    const long max_n = (long)max_n_in;
    SWC_CHECK_ARG(ld_runs >= max_n / (I + 2) + 1, "swc_activity: ld_runs=%ld: at least max_n_in / (I + 2) + 1 = %ld", (long)ld_runs,
                  max_n / (I + 2) + 1);
    const WsLayout P = ws_layout(B, max_n);
    SWC_CHECK_ARG(workspace_bytes >= (int64_t)P.total, "swc_activity: workspace of %ld bytes, %ld needed (swc_activity_workspace_bytes)",
                  (long)workspace_bytes, (long)P.total);
    SWC_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "swc_activity: workspace must be 256-byte aligned");
    SWC_CHECK_ARG(((reinterpret_cast<uintptr_t>(values) | reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(runs)) & 7u) == 0,
                  "swc_activity: values, counts and runs must be 8-byte aligned");
    if (B == 0) return SWC_OK;
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace);
    double* states = reinterpret_cast<double*>(ws + P.states);
    double* sqk = reinterpret_cast<double*>(ws + P.sqk);
    unsigned* pkk = reinterpret_cast<unsigned*>(ws + P.pkk);
    unsigned char* lev = reinterpret_cast<unsigned char*>(ws + P.lev);
    unsigned* acnt = reinterpret_cast<unsigned*>(ws + P.acnt);
    unsigned* rcnt = reinterpret_cast<unsigned*>(ws + P.rcnt);
    const EnvCoef co = coefficients(fs);
    const dim3 fgrid((unsigned)((P.S + AG - 1) / AG), (unsigned)B), wgrid((unsigned)P.NT, (unsigned)B);
    const size_t lds = 2 * (size_t)((WT + I + 2 + 15) & ~15L);  // two buffers of span bytes: at most 56232
    const double* cvalues = values;
    if (P.S > 0) {
        hipLaunchKernelGGL(act_filter_kernel<0>, fgrid, dim3(AG), 0, st, x_rows, n_in, max_n, co, states, sqk, pkk, P.S, lev, P.ldl, cvalues);
        SWC_CHECK_LAUNCH("swc_activity (filter 0)");
        hipLaunchKernelGGL(act_carry_kernel, dim3((unsigned)B), dim3(64), 0, st, n_in, max_n, co, states, P.S);
        SWC_CHECK_LAUNCH("swc_activity (carry)");
        hipLaunchKernelGGL(act_filter_kernel<1>, fgrid, dim3(AG), 0, st, x_rows, n_in, max_n, co, states, sqk, pkk, P.S, lev, P.ldl, cvalues);
        SWC_CHECK_LAUNCH("swc_activity (filter 1)");
        hipLaunchKernelGGL(act_window_kernel<0>, wgrid, dim3(WN), lds, st, n_in, max_n, (int)I, (const unsigned char*)lev, P.ldl, acnt, rcnt,
                           P.NT, runs, (long)ld_runs);
        SWC_CHECK_LAUNCH("swc_activity (window 0)");
    }
    hipLaunchKernelGGL(act_level_kernel, dim3((unsigned)B), dim3(WN), 0, st, n_in, max_n, margin_db, (const double*)sqk,
                       (const unsigned*)pkk, P.S, (const unsigned*)acnt, P.NT, values, counts);
    SWC_CHECK_LAUNCH("swc_activity (level)");
    if (P.S > 0) {
        hipLaunchKernelGGL(act_filter_kernel<2>, fgrid, dim3(AG), 0, st, x_rows, n_in, max_n, co, states, sqk, pkk, P.S, lev, P.ldl, cvalues);
        SWC_CHECK_LAUNCH("swc_activity (filter 2)");
        hipLaunchKernelGGL(act_window_kernel<1>, wgrid, dim3(WN), lds, st, n_in, max_n, (int)I, (const unsigned char*)lev, P.ldl, acnt, rcnt,
                           P.NT, runs, (long)ld_runs);
        SWC_CHECK_LAUNCH("swc_activity (window 1)");
    }
    hipLaunchKernelGGL(act_scan_kernel, dim3((unsigned)B), dim3(64), 0, st, n_in, max_n, rcnt, P.NT, values);
    SWC_CHECK_LAUNCH("swc_activity (scan)");
    if (P.S > 0) {
        hipLaunchKernelGGL(act_window_kernel<2>, wgrid, dim3(WN), lds, st, n_in, max_n, (int)I, (const unsigned char*)lev, P.ldl, acnt, rcnt,
                           P.NT, runs, (long)ld_runs);
        SWC_CHECK_LAUNCH("swc_activity (window 2)");
    }
    return SWC_OK;
}

extern "C" int swc_activity_normalise(const void* const* x_rows, const int64_t* n_in, const double* values, double target_db,
                                      float* out, int64_t ld_out, int64_t cols, float* gains, int32_t* flags, int32_t B, void* stream) {
    SWC_CHECK_ARG(x_rows && n_in && values, "swc_activity_normalise: null pointer");
    SWC_CHECK_ARG(out || gains || flags, "swc_activity_normalise: no output (out, gains and flags are null)");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_activity_normalise: B=%d (0..65535)", B);
    SWC_CHECK_ARG(target_db == target_db && fabs(target_db) <= 1e3, "swc_activity_normalise: target_db=%g: a finite number expected", target_db);
    SWC_CHECK_ARG(!out || (cols >= 0 && cols <= ld_out), "swc_activity_normalise: cols=%ld must be in 0..ld_out=%ld", (long)cols,
                  (long)ld_out);
    if (B == 0) return SWC_OK;
    const long c = out ? (long)cols : 0;
    const long tiles = c > 0 ? (c + NM_TILE - 1) / NM_TILE : 1;
    SWC_CHECK_ARG(tiles <= 0x7fffffffL, "swc_activity_normalise: cols too large");
    hipLaunchKernelGGL(act_normalise_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(NM_THREADS), 0, (hipStream_t)stream, x_rows,
                       n_in, values, target_db, c > 0 ? out : (float*)nullptr, (long)ld_out, c, gains, (int*)flags);
    SWC_CHECK_LAUNCH("swc_activity_normalise");
    return SWC_OK;
}
