// swc_lag_track, swc_lag_fit, swc_warp (include/swc_track.h): the sub-sample lag of every segment of every pair, one line per
// pair through that track, and the degraded row resampled along the line.  This file is compiled with -ffp-contract=off: the
// header fixes every float64 operation's rounding, and the one fused operation it asks for (swc_warp's chain) is written as
// fmaf.  No atomics and no memset: every intermediate word has exactly one writer.
//   track_level_kernel  one workgroup per (pair, side): max |v| of the row as an unsigned maximum over the bit patterns of |v|
//                       (any NaN or Inf wins), then in envelope mode the row's sum of |q|.
//   track_corr_kernel   the hot kernel, after align_corr_kernel (swc_align.hip): a workgroup of 256 threads owns (pair,
//                       segment, a block of SWC_TRACK_LAG_BLOCK lags) and walks the segment in chunks of SWC_TRACK_CHUNK
//                       samples of x.  Per chunk it stages the y span (CHUNK + LAG_BLOCK samples from i0 + d0 + the block's
//                       first lag, zero outside the row) as int16 and writes the packed views: the x chunk as pairs split
//                       into a high and a low digit (s = 256 h + l, |h|, |l| <= 128), the y span at both pair alignments
//                       (E[k] = (y[2k], y[2k+1]), O[k] = (y[2k+1], y[2k+2])) interleaved in blocks of four dwords.  Each of
//                       the four waves takes a quarter of the chunk and all 256 lags; lane (m = lane / 2, p = lane % 2) owns
//                       the lags 8 m + p + 2 i, i < 4; per four x pairs one 16-byte LDS read of each x digit (a broadcast) and
//                       one of y, 32 packed 16-bit dot products.  int32 accumulators are spilled into int64 every
//                       SWC_TRACK_SPILL samples (the bound is a static_assert) and the int64 sums stay in registers over the
//                       chunks.  The four waves' sums meet in LDS and the workgroup stores its 256 c_k[d]: it owns them.
//   track_seg_kernel    one workgroup per (pair, segment): the integer peak (an int64 maximum, then an integer minimum over the
//                       tie rule's key), the two int64 energies over the facing samples, 35 threads run one interpolation
//                       chain each, thread 0 picks j*, the parabola and writes the slot; the copy of c_k into xc.
//   track_fit_kernel    one thread per pair: the two passes of the weighted line in ascending k.
//   track_warp_kernel   one workgroup per SWC_WARP_BLOCK outputs: the y span those outputs read (at most 292 samples) staged
//                       once in LDS, one thread per output, a 32-term fmaf chain.
// Every store to global memory is an ordinary vector store from plain C++.
#include "swc_metric_common.h"
#include "swc_align.h"
#include "swc_track.h"
#include "swc_track_host.h"

namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_WAVES = TR_THREADS / 64;
constexpr int TR_C = SWC_TRACK_CHUNK;
constexpr int TR_G = SWC_TRACK_LAG_BLOCK;
constexpr int TR_XB = TR_C / 8;                 // blocks of four x pairs in a chunk
constexpr int TR_WB = TR_XB / TR_WAVES;         // ... in a wave's quarter
constexpr int TR_YB = TR_XB + TR_G / 8;         // blocks of four y pairs of ONE alignment: the last one read is TR_XB - 1 + 31 + 1
constexpr int TR_RAW = TR_C + TR_G + 8;         // y samples staged: O[4 TR_YB - 1] reads raw[8 TR_YB] = raw[TR_C + TR_G]
constexpr int TR_SPILL = SWC_TRACK_SPILL / 8;   // blocks of four x pairs between two spills
constexpr int TR_W = SWC_TRACK_W;
constexpr int TR_P = SWC_TRACK_P;
constexpr int TR_ROWS = SWC_TRACK_TABLE_ROWS;
constexpr int TR_COLS = SWC_TRACK_TABLE_COLS;
constexpr int WP_THREADS = SWC_WARP_BLOCK;
constexpr int WP_SPAN = 320;                    // y samples staged per workgroup of the warp kernel
static_assert(TR_G == 256 && TR_THREADS == TR_G, "a lane owns four lags of a wave's 256; the final reduce has one thread per lag");
static_assert(TR_WB % TR_SPILL == 0 && TR_XB % TR_WAVES == 0 && TR_C % 8 == 0, "whole spill runs per wave");
static_assert(TR_SPILL * 4 * 2 * 128 * 32767LL < (1LL << 31), "a digit's dot products fit int32 between two spills");
static_assert((long long)SWC_TRACK_MAX_N * 32767LL * 32767LL < (1LL << 53), "c, Sxx, Syy convert to double exactly");
static_assert(8 * TR_YB < TR_RAW, "the packed y views read inside the staged span");
static_assert(TR_ROWS == TR_P + 3 && TR_COLS == 2 * TR_W + 1 && TR_ROWS <= TR_THREADS, "one thread per interpolated position");
// ip moves by at most ceil(255 * 1.01) + 1 = 259 over a workgroup's outputs, and an output reads 32 samples from ip - 15
static_assert(259 + SWC_WARP_TAPS <= WP_SPAN && WP_THREADS == 256, "the warp kernel's outputs read inside the staged span");

__device__ __forceinline__ int sequence(int q, int mode, int mu) { return mode == SWC_ALIGN_ENVELOPE ? (q < 0 ? -q : q) - mu : q; }

// grid (B, 2 sides): peaks[side B + b], sums[side B + b]; 0, 0 for a row of an empty pair (its address is not read)
__global__ __launch_bounds__(TR_THREADS) void track_level_kernel(const void* const* __restrict__ x_rows,
                                                                 const void* const* __restrict__ y_rows,
                                                                 const int64_t* __restrict__ n_x, const int64_t* __restrict__ n_y,
                                                                 long max_nx, long max_ny, int mode, unsigned* __restrict__ peaks,
                                                                 long long* __restrict__ sums, int B) {
    __shared__ unsigned wm[TR_WAVES];
    __shared__ long long wsum[TR_WAVES];
    const int b = blockIdx.x, side = blockIdx.y, tid = threadIdx.x;
    const long nx = clamp_len(n_x, b, max_nx), ny = clamp_len(n_y, b, max_ny);
    unsigned pk = 0;
    long long total = 0;
    if (nx > 0 && ny > 0) {  // uniform over the workgroup
        const long n = side == 0 ? nx : ny;
        const void* row = side == 0 ? x_rows[b] : y_rows[b];
        const unsigned* pu = reinterpret_cast<const unsigned*>(row);
        unsigned m = 0;
#pragma unroll 4
        for (long i = tid; i < n; i += TR_THREADS) {
            const unsigned v = pu[i] & 0x7fffffffu;
            m = v > m ? v : m;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned v = (unsigned)__shfl_xor((int)m, o);
            m = v > m ? v : m;
        }
        if ((tid & 63) == 0) wm[tid >> 6] = m;
        __syncthreads();
        pk = wm[0];
#pragma unroll
        for (int w = 1; w < TR_WAVES; ++w) pk = wm[w] > pk ? wm[w] : pk;
        if (mode == SWC_ALIGN_ENVELOPE && peak_defined(pk)) {
            const int e = peak_exp(pk);
            const float* pf = reinterpret_cast<const float*>(row);
            long long s = 0;
#pragma unroll 4
            for (long i = tid; i < n; i += TR_THREADS) {
                const int q = quantise(pf[i], e);
                s += q < 0 ? -q : q;
            }
            s = wave_sum_i64(s);
            if ((tid & 63) == 0) wsum[tid >> 6] = s;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < TR_WAVES; ++w) total += wsum[w];
        }
    }
    if (tid == 0) {
        peaks[(long)side * B + b] = pk;
        sums[(long)side * B + b] = total;
    }
}

// grid (K * lag_blocks, B): c_k[d] of (pair, segment, lag block) into cws [B][K][2 R + 1]; zeros where nothing is summed
__global__ __launch_bounds__(TR_THREADS) void track_corr_kernel(const void* const* __restrict__ x_rows,
                                                                const void* const* __restrict__ y_rows,
                                                                const int64_t* __restrict__ n_x, const int64_t* __restrict__ n_y,
                                                                long max_nx, long max_ny, const int32_t* __restrict__ d0, long ld_d0,
                                                                int S, int H, int R, int mode, int lag_blocks, int K,
                                                                const unsigned* __restrict__ peaks,
                                                                const long long* __restrict__ sums, long long* __restrict__ cws,
                                                                int B) {
    __shared__ __attribute__((aligned(16))) unsigned xh[TR_C / 2];     // x pairs, high digits
    __shared__ __attribute__((aligned(16))) unsigned xl[TR_C / 2];     // x pairs, low digits
    __shared__ __attribute__((aligned(16))) unsigned yb[TR_YB * 8];    // y pairs: block k = E[4k .. 4k+3], O[4k .. 4k+3]
    __shared__ __attribute__((aligned(16))) long long red[TR_WAVES * TR_G];
    __shared__ short raw[TR_RAW];
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int seg = blockIdx.x / lag_blocks, lb = blockIdx.x - seg * lag_blocks;
    const long nx = clamp_len(n_x, b, max_nx), ny = clamp_len(n_y, b, max_ny);
    const long nl = 2L * R + 1;
    const long dl = (long)lb * TR_G - R;      // the block's first lag
    // everything that decides `live` is uniform over the workgroup
    bool live = nx > 0 && ny > 0;
    unsigned pkx = 0, pky = 0;
    if (live) {
        pkx = peaks[b];
        pky = peaks[(long)B + b];
        live = peak_defined(pkx) && peak_defined(pky) && pkx != 0u && pky != 0u;  // not defined, or a silent side: c stays 0
    }
    long s0 = 0, s1 = 0;
    if (live) {
        live = seg < track_segments(nx, S, H);
        s0 = S == 0 ? 0 : (long)seg * H;
        s1 = S == 0 ? nx : (s0 + S < nx ? s0 + S : nx);
    }
    const int m = lane >> 1, p = lane & 1;
    long long sh[4] = {0, 0, 0, 0}, sl[4] = {0, 0, 0, 0};
    if (live) {
        const int ex = peak_exp(pkx), ey = peak_exp(pky);
        int mux = 0, muy = 0;
        if (mode == SWC_ALIGN_ENVELOPE) {
            mux = (int)(sums[b] / nx);
            muy = (int)(sums[(long)B + b] / ny);
        }
        const float* xrow = reinterpret_cast<const float*>(x_rows[b]);
        const float* yrow = reinterpret_cast<const float*>(y_rows[b]);
        const long dc = d0[(long)b * ld_d0];
        const uint4* xh4 = reinterpret_cast<const uint4*>(xh);
        const uint4* xl4 = reinterpret_cast<const uint4*>(xl);
        const uint4* yb4 = reinterpret_cast<const uint4*>(yb);
        const int jw = wave * TR_WB;  // jw + jb + 1 + m <= TR_XB - 1 + 1 + 31 = TR_YB - 1
        for (long i0 = s0; i0 < s1; i0 += TR_C) {
            const long ys = i0 + dc + dl;            // the y sample that faces x[i0] at the block's first lag
            if (ys >= ny || ys + TR_C + TR_G <= 0) continue;  // the whole span lies outside y: every product is 0
            __syncthreads();                         // the previous chunk's reads are over
            // ---- the y span as int16, the x chunk (cut at the segment's end) as digit pairs ----
            for (int k = tid; k < TR_RAW; k += TR_THREADS) {
                const long g = ys + k;
                raw[k] = (short)((g >= 0 && g < ny) ? sequence(quantise(yrow[g], ey), mode, muy) : 0);
            }
            for (int k = tid; k < TR_C / 2; k += TR_THREADS) {
                const long g = i0 + 2 * k;
                const int a0 = g < s1 ? sequence(quantise(xrow[g], ex), mode, mux) : 0;
                const int a1 = g + 1 < s1 ? sequence(quantise(xrow[g + 1], ex), mode, mux) : 0;
                const int h0 = (a0 + 128) >> 8, h1 = (a1 + 128) >> 8;
                xh[k] = pack16(h0, h1);
                xl[k] = pack16(a0 - 256 * h0, a1 - 256 * h1);
            }
            __syncthreads();
            for (int k = tid; k < 4 * TR_YB; k += TR_THREADS) {  // 2 k + 2 <= 8 TR_YB < TR_RAW
                const int q0 = raw[2 * k], q1 = raw[2 * k + 1], q2 = raw[2 * k + 2];
                unsigned* blk = yb + (k >> 2) * 8 + (k & 3);
                blk[0] = pack16(q0, q1);
                blk[4] = pack16(q1, q2);
            }
            __syncthreads();
            // ---- this wave's quarter of the chunk, four lags per lane ----
            for (int jb0 = 0; jb0 < TR_WB; jb0 += TR_SPILL) {
                int ch[4] = {0, 0, 0, 0}, cl[4] = {0, 0, 0, 0};
                uint4 t0 = yb4[2 * (jw + jb0 + m) + p];
                for (int jb = jb0; jb < jb0 + TR_SPILL; ++jb) {
                    const uint4 t1 = yb4[2 * (jw + jb + 1 + m) + p];
                    const uint4 vh = xh4[jw + jb], vl = xl4[jw + jb];
                    const unsigned s[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
                    const unsigned wh[4] = {vh.x, vh.y, vh.z, vh.w}, wl[4] = {vl.x, vl.y, vl.z, vl.w};
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            ch[i] = dot2(wh[jj], s[jj + i], ch[i]);
                            cl[i] = dot2(wl[jj], s[jj + i], cl[i]);
                        }
                    }
                    t0 = t1;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    sh[i] += ch[i];
                    sl[i] += cl[i];
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave * TR_G + 8 * m + p + 2 * i] = 256 * sh[i] + sl[i];
    __syncthreads();
    long long v = 0;
#pragma unroll
    for (int w = 0; w < TR_WAVES; ++w) v += red[w * TR_G + tid];
    const long col = dl + tid + R;  // d + R
    if (col < nl) cws[((long)b * K + seg) * nl + col] = v;
}

// grid (K, B): one workgroup per segment slot
__global__ __launch_bounds__(TR_THREADS) void track_seg_kernel(const void* const* __restrict__ x_rows,
                                                               const void* const* __restrict__ y_rows,
                                                               const int64_t* __restrict__ n_x, const int64_t* __restrict__ n_y,
                                                               long max_nx, long max_ny, const int32_t* __restrict__ d0, long ld_d0,
                                                               int S, int H, int Rs, int mode, int K,
                                                               const double* __restrict__ table, const unsigned* __restrict__ peaks,
                                                               const long long* __restrict__ sums,
                                                               const long long* __restrict__ cws, double* __restrict__ vals,
                                                               int32_t* __restrict__ status, long ldk, int32_t* __restrict__ nseg,
                                                               int64_t* __restrict__ xc, long ldc, int B) {
    __shared__ long long best_c[TR_THREADS];
    __shared__ int best_d[TR_THREADS];
    __shared__ long long we[TR_WAVES][2];
    __shared__ double ct[TR_ROWS];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int R = Rs + TR_W + 1;
    const long nl = 2L * R + 1;
    const long nx = clamp_len(n_x, b, max_nx), ny = clamp_len(n_y, b, max_ny);
    const unsigned pkx = peaks[b], pky = peaks[(long)B + b];
    const bool ok = nx > 0 && ny > 0 && peak_defined(pkx) && peak_defined(pky);
    const int ns = ok ? (int)track_segments(nx, S, H) : 0;
    const long long* c = cws + ((long)b * K + k) * nl;
    if (xc != nullptr) {
        int64_t* o = xc + ((long)b * ldk + k) * ldc;
        for (long col = tid; col < nl; col += TR_THREADS) o[col] = c[col];
    }
    if (k == 0 && tid == 0 && nseg != nullptr) nseg[b] = ns;
    if (vals == nullptr && status == nullptr) return;
    // the integer peak in two order-free steps (align_pick_kernel): the largest c, then the smallest key 2 |d| + (d < 0)
    long long bc = 0;
    for (int d = -Rs + tid; d <= Rs; d += TR_THREADS) {
        const long long v = c[d + R];
        bc = v > bc ? v : bc;
    }
    best_c[tid] = bc;
    __syncthreads();
    for (int o = TR_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const long long c2 = best_c[tid + o];
            if (c2 > best_c[tid]) best_c[tid] = c2;
        }
        __syncthreads();
    }
    const long long cmax = best_c[0];
    int key = 0x7fffffff;
    if (cmax > 0) {
        for (int d = -Rs + tid; d <= Rs; d += TR_THREADS) {
            if (c[d + R] == cmax) {
                const int kd = d < 0 ? 2 * -d + 1 : 2 * d;
                key = kd < key ? kd : key;
            }
        }
    }
    best_d[tid] = key;
    __syncthreads();
    for (int o = TR_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const int k2 = best_d[tid + o];
            if (k2 < best_d[tid]) best_d[tid] = k2;
        }
        __syncthreads();
    }
    const bool defined = k < ns && cmax > 0;   // uniform
    double* ov = vals != nullptr ? vals + ((long)b * ldk + k) * SWC_TRACK_VALUES : nullptr;
    int32_t* os = status != nullptr ? status + (long)b * ldk + k : nullptr;
    if (!defined) {
        if (tid == 0) {
            const double nan = __builtin_nan("");
            if (ov != nullptr) {
                ov[0] = nan;
                ov[1] = nan;
                ov[2] = 0.0;
                ov[3] = nan;
            }
            if (os != nullptr) *os = 0;
        }
        return;
    }
    const int kbest = best_d[0];
    const int dstar = (kbest & 1) ? -(kbest >> 1) : (kbest >> 1);
    const long dc = d0[(long)b * ld_d0];
    const long dd = dc + dstar;
    const long s0 = S == 0 ? 0 : (long)k * H;
    const long s1 = S == 0 ? nx : (s0 + S < nx ? s0 + S : nx);
    const long lo = s0 > -dd ? s0 : -dd, hi = s1 < ny - dd ? s1 : ny - dd;  // lo < hi: c_k[d*] > 0 has a term
    // ---- the energies over the facing samples ----
    {
        const int ex = peak_exp(pkx), ey = peak_exp(pky);
        int mux = 0, muy = 0;
        if (mode == SWC_ALIGN_ENVELOPE) {
            mux = (int)(sums[b] / nx);
            muy = (int)(sums[(long)B + b] / ny);
        }
        const float* xrow = reinterpret_cast<const float*>(x_rows[b]);        // reads [lo, hi): inside [0, nx)
        const float* yrow = reinterpret_cast<const float*>(y_rows[b]) + dd;   // reads [lo + dd, hi + dd): inside [0, ny)
        long long sxx = 0, syy = 0;
#pragma unroll 4
        for (long i = lo + tid; i < hi; i += TR_THREADS) {
            const int vx = sequence(quantise(xrow[i], ex), mode, mux), vy = sequence(quantise(yrow[i], ey), mode, muy);
            sxx += (long long)(vx * vx);
            syy += (long long)(vy * vy);
        }
        sxx = wave_sum_i64(sxx);
        syy = wave_sum_i64(syy);
        if ((tid & 63) == 0) {
            we[tid >> 6][0] = sxx;
            we[tid >> 6][1] = syy;
        }
    }
    // ---- ct(j), one chain per thread; |d*| <= Rs, so the columns d* + t + R lie in [1, 2 R - 1] ----
    if (tid < TR_ROWS) {
        const double* trow = table + tid * TR_COLS;
        const long long* cc = c + (dstar + R - TR_W);
        double acc = 0.0;
        for (int t = 0; t < TR_COLS; ++t) {
            const double prod = (double)cc[t] * trow[t];
            acc = acc + prod;
        }
        ct[tid] = acc;
    }
    __syncthreads();
    if (tid != 0) return;
    long long sxx = 0, syy = 0;
#pragma unroll
    for (int w = 0; w < TR_WAVES; ++w) {
        sxx += we[w][0];
        syy += we[w][1];
    }
    // j* over the interior: 0, +1, -1, +2, -2, ... with a strict comparison is the tie rule
    const int mid = TR_P / 2 + 1;  // the row of j = 0
    int js = 0;
    double y0 = ct[mid];
    for (int a = 1; a <= TR_P / 2; ++a) {
        if (ct[mid + a] > y0) {
            y0 = ct[mid + a];
            js = a;
        }
        if (ct[mid - a] > y0) {
            y0 = ct[mid - a];
            js = -a;
        }
    }
    const double ym = ct[mid + js - 1], yp = ct[mid + js + 1];
    const double num = ym - yp;
    const double den = (ym - y0) + (yp - y0);
    double delta = 0.0;
    if (den < 0.0) {
        const double quot = num / den;
        delta = 0.5 * quot;
    }
    delta = delta < -0.5 ? -0.5 : (delta > 0.5 ? 0.5 : delta);
    const double fr = ((double)js + delta) / (double)TR_P;
    const double lag = (double)dd + fr;
    const double prod = (double)sxx * (double)syy;
    const double rho = __ddiv_rn((double)cmax, __dsqrt_rn(prod));
    if (ov != nullptr) {
        ov[0] = lag;
        ov[1] = rho;
        ov[2] = (double)sxx;
        ov[3] = (double)(lo + hi - 1) * 0.5;
    }
    if (os != nullptr) *os = SWC_TRACK_DEFINED | ((dstar == Rs || dstar == -Rs) ? SWC_TRACK_EDGE : 0);
}

struct FitLine {
    double a, b, sw;
    int n;
    bool flat;  // a drift fit without two distinct centres
};

// line(U) of the header.  second: U2 (the residual from (a1, b1) at most one sample), else U1
__device__ FitLine fit_line(const double* __restrict__ v, const int32_t* __restrict__ st, int n, double rho_min, int drift, bool second,
                            double a1, double b1) {
    FitLine L = {0.0, 0.0, 0.0, 0, false};
    double sw = 0.0, swt = 0.0, swl = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        double tm = 0.0, lm = 0.0, stt = 0.0, stl = 0.0;
        if (pass == 1) {
            if (L.n == 0) return L;
            tm = swt / sw;
            lm = swl / sw;
        }
        for (int k = 0; k < n; ++k) {
            const double l = v[4 * k], rho = v[4 * k + 1], w = v[4 * k + 2], t = v[4 * k + 3];
            if (!(st[k] & SWC_TRACK_DEFINED) || !(rho >= rho_min)) continue;
            if (second) {
                const double bt = b1 * t;
                const double at = a1 + bt;
                const double r = l - at;
                if (!(fabs(r) <= 1.0)) continue;
            }
            if (pass == 0) {
                const double wt = w * t, wl = w * l;
                sw = sw + w;
                swt = swt + wt;
                swl = swl + wl;
                ++L.n;
            } else {
                const double dt = t - tm, dl = l - lm;
                const double tt = dt * dt, tl = dt * dl;
                const double wtt = w * tt, wtl = w * tl;
                stt = stt + wtt;
                stl = stl + wtl;
            }
        }
        if (pass == 1) {
            L.sw = sw;
            if (drift) {
                if (L.n < 2 || !(stt > 0.0)) {
                    L.flat = true;
                } else {
                    L.b = stl / stt;
                    const double btm = L.b * tm;
                    L.a = lm - btm;
                }
            } else {
                L.a = lm;
            }
        }
    }
    return L;
}

__global__ __launch_bounds__(64) void track_fit_kernel(const double* __restrict__ vals, const int32_t* __restrict__ status, long ldk,
                                                       const int32_t* __restrict__ nseg, int kmax, const int32_t* __restrict__ d0,
                                                       long ld_d0, double rho_min, int drift, double* __restrict__ fit,
                                                       int32_t* __restrict__ counts, int B) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    int n = nseg[b];
    n = n < 0 ? 0 : (n > kmax ? kmax : n);
    const double* v = vals + (long)b * ldk * SWC_TRACK_VALUES;
    const int32_t* st = status + (long)b * ldk;
    int flags = 0, used = 0;
    FitLine L = fit_line(v, st, n, rho_min, drift, false, 0.0, 0.0);
    used = L.n;
    if (L.n == 0) flags |= SWC_FIT_NO_LAG;
    if (drift && (L.n < 2 || L.flat)) flags |= SWC_FIT_NO_DRIFT;
    if (flags == 0) {
        const double a1 = L.a, b1 = L.b;
        L = fit_line(v, st, n, rho_min, drift, true, a1, b1);
        used = L.n;
        if (L.n == 0) flags |= SWC_FIT_NO_LAG;
        if (drift && (L.n < 2 || L.flat)) flags |= SWC_FIT_NO_DRIFT;
        if (flags == 0) {
            double sr = 0.0;
            for (int k = 0; k < n; ++k) {
                const double l = v[4 * k], rho = v[4 * k + 1], w = v[4 * k + 2], t = v[4 * k + 3];
                if (!(st[k] & SWC_TRACK_DEFINED) || !(rho >= rho_min)) continue;
                const double bt1 = b1 * t;
                const double at1 = a1 + bt1;
                const double r1 = l - at1;
                if (!(fabs(r1) <= 1.0)) continue;
                const double bt = L.b * t;
                const double at = L.a + bt;
                const double r = l - at;
                const double rr = r * r;
                const double wrr = w * rr;
                sr = sr + wrr;
                if (st[k] & SWC_TRACK_EDGE) flags |= SWC_FIT_EDGE;
            }
            const double mean = sr / L.sw;
            double* o = fit + (long)b * SWC_FIT_VALUES;
            o[0] = L.a;
            o[1] = L.b;
            o[2] = __dsqrt_rn(mean);
            o[3] = 0.0;
        }
    }
    if (flags & (SWC_FIT_NO_LAG | SWC_FIT_NO_DRIFT)) {
        double* o = fit + (long)b * SWC_FIT_VALUES;
        o[0] = (double)d0[(long)b * ld_d0];
        o[1] = 0.0;
        o[2] = __builtin_nan("");
        o[3] = 0.0;
    }
    if (counts != nullptr) {
        int32_t* o = counts + (long)b * SWC_FIT_COUNTS;
        o[0] = used;
        o[1] = n;
        o[2] = flags;
        o[3] = 0;
    }
}

// grid (ceil(cols / 256), B)
__global__ __launch_bounds__(WP_THREADS) void track_warp_kernel(const void* const* __restrict__ y_rows, const int64_t* __restrict__ n_x,
                                                                const int64_t* __restrict__ n_y, long max_nx, long max_ny,
                                                                const double* __restrict__ fit, long ld_fit,
                                                                const float* __restrict__ table, float* __restrict__ out, long ld_out,
                                                                long cols, int32_t* __restrict__ info) {
    __shared__ float span[WP_SPAN];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long nx = clamp_len(n_x, b, max_nx), ny = clamp_len(n_y, b, max_ny);
    const double a = fit[(long)b * ld_fit], bb = fit[(long)b * ld_fit + 1];
    const bool good = fabs(a) <= (double)SWC_WARP_MAX_LAG && fabs(bb) <= SWC_WARP_MAX_DRIFT;  // a NaN fails
    int64_t A = 0, Q = (int64_t)1 << 32, x0 = 0, m = 0;
    if (good) {
        const double rate = 1.0 + bb;
        A = (int64_t)rint(a * 4294967296.0);
        Q = (int64_t)rint(rate * 4294967296.0);
        if (nx > 0 && ny > 0) warp_bounds(A, Q, nx, ny, cols, &x0, &m);
    }
    if (blockIdx.x == 0 && tid == 0 && info != nullptr) {
        int32_t* o = info + (long)b * SWC_WARP_INFO;
        o[0] = (int32_t)x0;
        o[1] = (int32_t)m;
        o[2] = good ? 0 : 1;
        o[3] = 0;
    }
    const long c0 = (long)blockIdx.x * WP_THREADS, c = c0 + tid;
    float* orow = out + (long)b * ld_out;
    if (c0 >= m) {  // uniform: nothing of the row is read (m == 0 for an empty pair)
        if (c < cols) orow[c] = 0.0f;
        return;
    }
    const int64_t ipf = (A + (x0 + c0) * Q) >> 32;  // >= 0: x0 + c0 is a valid i
    const float* yrow = reinterpret_cast<const float*>(y_rows[b]);
    for (int k = tid; k < WP_SPAN; k += WP_THREADS) {
        const int64_t g = ipf - 15 + k;
        span[k] = (g >= 0 && g < ny) ? yrow[g] : 0.0f;
    }
    __syncthreads();
    if (c >= cols) return;
    float acc = 0.0f;
    if (c < m) {
        const int64_t pos = A + (x0 + c) * Q;
        const int off = (int)((pos >> 32) - ipf);  // 0 .. 259
        const unsigned frac = (unsigned)(pos & 0xffffffffLL);
        const unsigned phase = frac >> 24;
        const float wt = (float)(frac & 0xffffffu) * 5.9604644775390625e-08f;  // 2^-24, exact
        const float* h0 = table + phase * SWC_WARP_TAPS;
        const float* h1 = h0 + SWC_WARP_TAPS;
#pragma unroll 8
        for (int t = 0; t < SWC_WARP_TAPS; ++t) {
            const float a0 = h0[t];
            const float dh = h1[t] - a0;
            const float h = fmaf(wt, dh, a0);
            acc = fmaf(h, span[off + t], acc);
        }
    }
    orow[c] = acc;
}

}  // namespace

extern "C" int64_t swc_track_segments(int64_t n, int32_t S, int32_t H) { return track_segments(n, S, H); }

extern "C" int64_t swc_lag_track_workspace_bytes(int32_t B, int64_t max_nx, int64_t max_ny, int32_t S, int32_t H, int32_t Rs) {
    const TrackLayout P = track_layout(B, max_nx, max_ny, S, H, Rs);
    return P.ok ? (int64_t)P.total : -1;
}

extern "C" int swc_lag_track(const void* const* x_rows, const void* const* y_rows, const int64_t* n_x, const int64_t* n_y,
                             int64_t max_nx, int64_t max_ny, const int32_t* d0, int64_t ld_d0, int32_t S, int32_t H, int32_t Rs,
                             int32_t mode, const double* table, double* vals, int32_t* status, int64_t ldk, int32_t* nseg,
                             int64_t* xc, int64_t ldc, void* workspace, int64_t workspace_bytes, int32_t B, void* stream) {
    SWC_CHECK_ARG(x_rows && y_rows && n_x && n_y && d0 && table && workspace, "swc_lag_track: null pointer");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_lag_track: B=%d (0..65535)", B);
    SWC_CHECK_ARG(max_nx >= 0 && max_nx <= SWC_TRACK_MAX_N && max_ny >= 0 && max_ny <= SWC_TRACK_MAX_N,
                  "swc_lag_track: max_nx=%ld, max_ny=%ld out of range (0..%d)", (long)max_nx, (long)max_ny, SWC_TRACK_MAX_N);
    SWC_CHECK_ARG(ld_d0 >= 1, "swc_lag_track: ld_d0=%ld (>= 1)", (long)ld_d0);
    SWC_CHECK_ARG(S >= 0 && S <= SWC_TRACK_MAX_N, "swc_lag_track: segment length S=%d (0..%d)", S, SWC_TRACK_MAX_N);
    SWC_CHECK_ARG(S == 0 || (H >= 1 && H <= SWC_TRACK_MAX_N), "swc_lag_track: hop H=%d (1..%d)", H, SWC_TRACK_MAX_N);
    SWC_CHECK_ARG(Rs >= 0 && Rs <= SWC_TRACK_MAX_RANGE, "swc_lag_track: search half-range Rs=%d (0..%d)", Rs, SWC_TRACK_MAX_RANGE);
    SWC_CHECK_ARG(mode == SWC_ALIGN_WAVEFORM || mode == SWC_ALIGN_ENVELOPE, "swc_lag_track: mode=%d (0 waveform, 1 envelope)", mode);
    const int64_t K = track_segments(max_nx, S, H);
    SWC_CHECK_ARG(K >= 0 && K <= SWC_TRACK_MAX_SEGMENTS, "swc_lag_track: %ld segments in a row of max_nx samples (at most %d)",
                  (long)K, SWC_TRACK_MAX_SEGMENTS);
    const int R = Rs + SWC_TRACK_W + 1;
    const long nl = 2L * R + 1;
    SWC_CHECK_ARG((vals == nullptr && status == nullptr && xc == nullptr) || ldk >= K, "swc_lag_track: ldk=%ld, %ld segments",
                  (long)ldk, (long)K);
    SWC_CHECK_ARG(xc == nullptr || ldc >= nl, "swc_lag_track: ldc=%ld, %ld lags", (long)ldc, nl);
    const TrackLayout P = track_layout(B, max_nx, max_ny, S, H, Rs);
    SWC_CHECK_ARG(P.ok && workspace_bytes >= (int64_t)P.total,
                  "swc_lag_track: workspace of %ld bytes, %ld needed (swc_lag_track_workspace_bytes)", (long)workspace_bytes,
                  (long)P.total);
    SWC_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "swc_lag_track: workspace must be 256-byte aligned");
    if (B == 0) return SWC_OK;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* base = reinterpret_cast<unsigned char*>(workspace);
    unsigned* peaks = reinterpret_cast<unsigned*>(base + P.peaks);
    long long* sums = reinterpret_cast<long long*>(base + P.sums);
    long long* cws = reinterpret_cast<long long*>(base + P.c);
    const long max_nx_l = max_nx, max_ny_l = max_ny;
    hipLaunchKernelGGL(track_level_kernel, dim3((unsigned)B, 2u), dim3(TR_THREADS), 0, st, x_rows, y_rows, n_x, n_y, max_nx_l, max_ny_l,
                       mode, peaks, sums, B);
    SWC_CHECK_LAUNCH("swc_lag_track (level)");
    if (K > 0) {
        const int lag_blocks = (int)((nl + TR_G - 1) / TR_G);  // <= 9
        hipLaunchKernelGGL(track_corr_kernel, dim3((unsigned)(K * lag_blocks), (unsigned)B), dim3(TR_THREADS), 0, st, x_rows, y_rows,
                           n_x, n_y, max_nx_l, max_ny_l, d0, (long)ld_d0, S, H, R, mode, lag_blocks, (int)K, (const unsigned*)peaks,
                           (const long long*)sums, cws, B);
        SWC_CHECK_LAUNCH("swc_lag_track (corr)");
        if (vals != nullptr || status != nullptr || xc != nullptr || nseg != nullptr) {
            hipLaunchKernelGGL(track_seg_kernel, dim3((unsigned)K, (unsigned)B), dim3(TR_THREADS), 0, st, x_rows, y_rows, n_x, n_y,
                               max_nx_l, max_ny_l, d0, (long)ld_d0, S, H, Rs, mode, (int)K, table, (const unsigned*)peaks,
                               (const long long*)sums, (const long long*)cws, vals, status, (long)ldk, nseg, xc, (long)ldc, B);
            SWC_CHECK_LAUNCH("swc_lag_track (segments)");
        }
    } else if (nseg != nullptr) {  // max_nx == 0: every pair is empty
        if (hipMemsetAsync(nseg, 0, (size_t)B * sizeof(int32_t), st) != hipSuccess) {
            (void)hipGetLastError();
            swc_set_error("swc_lag_track: clearing nseg failed");
            return SWC_E_LAUNCH;
        }
    }
    return SWC_OK;
}

extern "C" int swc_lag_fit(const double* vals, const int32_t* status, int64_t ldk, const int32_t* nseg, int32_t kmax,
                           const int32_t* d0, int64_t ld_d0, double rho_min, int32_t drift, double* fit, int32_t* counts, int32_t B,
                           void* stream) {
    SWC_CHECK_ARG(vals && status && nseg && d0 && fit, "swc_lag_fit: null pointer");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_lag_fit: B=%d (0..65535)", B);
    SWC_CHECK_ARG(kmax >= 0 && kmax <= SWC_TRACK_MAX_SEGMENTS && ldk >= kmax, "swc_lag_fit: kmax=%d, ldk=%ld (0 <= kmax <= %d, ldk >= kmax)",
                  kmax, (long)ldk, SWC_TRACK_MAX_SEGMENTS);
    SWC_CHECK_ARG(ld_d0 >= 1, "swc_lag_fit: ld_d0=%ld (>= 1)", (long)ld_d0);
    SWC_CHECK_ARG(rho_min >= -1.0 && rho_min <= 1.0, "swc_lag_fit: rho_min=%g (-1..1)", rho_min);
    SWC_CHECK_ARG(drift == 0 || drift == 1, "swc_lag_fit: drift=%d (0 or 1)", drift);
    if (B == 0) return SWC_OK;
    hipLaunchKernelGGL(track_fit_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, vals, status, (long)ldk, nseg,
                       (int)kmax, d0, (long)ld_d0, rho_min, (int)drift, fit, counts, B);
    SWC_CHECK_LAUNCH("swc_lag_fit");
    return SWC_OK;
}

extern "C" int swc_warp(const void* const* y_rows, const int64_t* n_x, const int64_t* n_y, int64_t max_nx, int64_t max_ny,
                        const double* fit, int64_t ld_fit, const float* table, float* out, int64_t ld_out, int64_t cols,
                        int32_t* info, int32_t B, void* stream) {
    SWC_CHECK_ARG(y_rows && n_x && n_y && fit && table && out, "swc_warp: null pointer");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_warp: B=%d (0..65535)", B);
    SWC_CHECK_ARG(max_nx >= 0 && max_nx <= SWC_TRACK_MAX_N && max_ny >= 0 && max_ny <= SWC_TRACK_MAX_N,
                  "swc_warp: max_nx=%ld, max_ny=%ld out of range (0..%d)", (long)max_nx, (long)max_ny, SWC_TRACK_MAX_N);
    SWC_CHECK_ARG(ld_fit >= 2, "swc_warp: ld_fit=%ld (>= 2)", (long)ld_fit);
    SWC_CHECK_ARG(cols >= 0 && cols <= SWC_TRACK_MAX_N, "swc_warp: cols=%ld (0..%d)", (long)cols, SWC_TRACK_MAX_N);
    SWC_CHECK_ARG(ld_out >= cols, "swc_warp: ld_out=%ld, %ld columns", (long)ld_out, (long)cols);
    if (B == 0) return SWC_OK;
    hipStream_t st = (hipStream_t)stream;
    if (cols == 0) {  // no output column: only info, from one workgroup per pair
        if (info == nullptr) return SWC_OK;
    }
    const long blocks = cols > 0 ? (cols + WP_THREADS - 1) / WP_THREADS : 1;
    hipLaunchKernelGGL(track_warp_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(WP_THREADS), 0, st, y_rows, n_x, n_y, (long)max_nx,
                       (long)max_ny, fit, (long)ld_fit, table, out, (long)ld_out, (long)cols, info);
    SWC_CHECK_LAUNCH("swc_warp");
    return SWC_OK;
}
