// swc_align (include/swc_align.h): the integer lag, the overlap, the correlation and the level ratio of every pair of a ragged
// batch.  After one memset of the accumulators (peaks, sums of |q|, c[d]) up to six kinds of launch, no workgroup waits for
// another:
//   align_peak_kernel  max |v| of every row as an unsigned maximum over the bit patterns of |v| (the trick of pitch_peak_kernel:
//                      any NaN or Inf wins, exact in any order): one workgroup per 4096 samples of one row, one atomic per workgroup.
//   align_abs_kernel   (envelope mode only) sum |q| of every row: int64 partial sums, one integer atomic add per workgroup.
//   align_corr_kernel  the direct correlation.  A workgroup of 256 threads takes (pair, a chunk of SWC_ALIGN_CHUNK samples of x
//                      from i0, a block of SWC_ALIGN_LAG_BLOCK lags from d0).  It stages the y span ys = i0 + d0 .. of
//                      CHUNK + LAG_BLOCK samples as int16 (zero outside the row), then writes the packed views: the x chunk as
//                      pairs (s[2k], s[2k+1]) split into a high and a low digit (s = 256 h + l, |h|, |l| <= 128), and the y
//                      span at both pair alignments, E[k] = (y[2k], y[2k+1]) and O[k] = (y[2k+1], y[2k+2]), interleaved in
//                      blocks of four dwords.  Each of the four waves takes a quarter of the chunk and all 256 lags: lane
//                      (m = lane / 2, p = lane % 2) owns the four lags t = 8 m + p + 2 i, for which the y pairs of x pair j are
//                      (p ? O : E)[j + 4 m + i]: per four x pairs it reads one 16-byte block of each x digit (the same address
//                      in every lane: a broadcast) and one new 16-byte block of y (consecutive lanes, consecutive blocks), and
//                      issues 32 packed 16-bit dot products.  A digit's products stay below 2^23, so 128 pairs fit an int32
//                      accumulator; then it is spilled into an int64 sum.  The four waves' sums meet in LDS and one int64
//                      integer atomic per lag adds them to c[d] in the workspace.
//   align_pick_kernel  one workgroup per pair: the choice as an int64 maximum and then an integer minimum over the tie rule's
//                      key (any reduction order gives the same d*), the copy of c into xc, and info.
//   align_energy_kernel  (when values are asked for) the four int64 energies over the overlap, one workgroup per 4096 samples,
//                      integer atomics; then align_values_kernel, one thread per pair: the two float64 values.
// Everything up to the two final divisions is integer arithmetic: any order gives the same bits.
// Every store to global memory is an ordinary vector store from plain C++ or an integer atomic.
#include "swc_metric_common.h"
#include "swc_align.h"

namespace {

constexpr int AL_THREADS = 256;
constexpr int AL_WAVES = AL_THREADS / 64;
constexpr int AL_C = SWC_ALIGN_CHUNK;
constexpr int AL_G = SWC_ALIGN_LAG_BLOCK;
constexpr int AL_XB = AL_C / 8;                 // blocks of four x pairs in a chunk
constexpr int AL_WB = AL_XB / AL_WAVES;         // ... in a wave's quarter
constexpr int AL_YB = AL_XB + AL_G / 8;         // blocks of four y pairs of ONE alignment: the last one read is AL_XB - 1 + 31 + 1
constexpr int AL_RAW = AL_C + AL_G + 8;         // y samples staged: O[4 AL_YB - 1] reads raw[8 AL_YB] = raw[AL_C + AL_G]
constexpr int AL_SPILL = SWC_ALIGN_SPILL / 8;   // blocks of four x pairs between two spills
constexpr int PK_THREADS = 256;
constexpr int PK_CHUNK = 4096;                  // samples per workgroup of the peak and abs kernels
constexpr int EN_CHUNK = 4096;                  // samples of the overlap per workgroup of the energy kernel
constexpr int AL_ACC = 8;                       // int64 words per pair: Sxx, Syy, Exx, Eyy, d*, three spare
static_assert(AL_G == 256 && AL_THREADS == AL_G, "a lane owns four lags of a wave's 256; the final reduce has one thread per lag");
static_assert(AL_WB % AL_SPILL == 0 && AL_XB % AL_WAVES == 0 && AL_C % 8 == 0, "whole spill runs per wave");
static_assert(AL_SPILL * 4 * 2 * 128 * 32767LL < (1LL << 31), "a digit's dot products fit int32 between two spills");
static_assert((long long)SWC_ALIGN_MAX_N * 32767LL * 32767LL < (1LL << 53), "c, Sxx, Exx convert to double exactly");
static_assert(8 * AL_YB < AL_RAW, "the packed y views read inside the staged span");

// s of the header from q
__device__ __forceinline__ int sequence(int q, int mode, int mu) { return mode == SWC_ALIGN_ENVELOPE ? (q < 0 ? -q : q) - mu : q; }

__device__ __forceinline__ void atomic_add_i64(long long* p, long long v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);  // two's complement: exact
}

// grid (chunks, B, 2 sides)
__global__ __launch_bounds__(PK_THREADS) void align_peak_kernel(const void* const* __restrict__ x_rows,
                                                                const void* const* __restrict__ y_rows,
                                                                const int64_t* __restrict__ n_x, const int64_t* __restrict__ n_y,
                                                                long max_nx, long max_ny, unsigned* __restrict__ peaks, int B) {
    const int b = blockIdx.y, side = blockIdx.z, tid = threadIdx.x;
    const long nx = clamp_len(n_x, b, max_nx), ny = clamp_len(n_y, b, max_ny);
    if (nx <= 0 || ny <= 0) return;  // an empty pair: its addresses are not read
    const long n = side == 0 ? nx : ny;
    const long i0 = (long)blockIdx.x * PK_CHUNK;
    if (i0 >= n) return;
    const unsigned* p = reinterpret_cast<const unsigned*>(side == 0 ? x_rows[b] : y_rows[b]);
    const long i1 = i0 + PK_CHUNK < n ? i0 + PK_CHUNK : n;
    unsigned m = 0;
#pragma unroll 4
    for (long i = i0 + tid; i < i1; i += PK_THREADS) {
        const unsigned v = p[i] & 0x7fffffffu;
        m = v > m ? v : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned v = (unsigned)__shfl_xor((int)m, o);
        m = v > m ? v : m;
    }
    // one atomic per workgroup, not per wave: the atomics of a row all meet at one address and serialise there
    __shared__ unsigned wm[PK_THREADS / 64];
    if ((tid & 63) == 0) wm[tid >> 6] = m;
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < PK_THREADS / 64; ++w) m = wm[w] > m ? wm[w] : m;
    if (m != 0) atomicMax(peaks + (long)side * B + b, m);
}

// grid (chunks, B, 2 sides): sum |q| of a defined pair's rows
__global__ __launch_bounds__(PK_THREADS) void align_abs_kernel(const void* const* __restrict__ x_rows,
                                                               const void* const* __restrict__ y_rows,
                                                               const int64_t* __restrict__ n_x, const int64_t* __restrict__ n_y,
                                                               long max_nx, long max_ny, const unsigned* __restrict__ peaks,
                                                               long long* __restrict__ sums, int B) {
    const int b = blockIdx.y, side = blockIdx.z, tid = threadIdx.x;
    const long nx = clamp_len(n_x, b, max_nx), ny = clamp_len(n_y, b, max_ny);
    if (nx <= 0 || ny <= 0) return;
    const long n = side == 0 ? nx : ny;
    const long i0 = (long)blockIdx.x * PK_CHUNK;
    if (i0 >= n) return;
    const unsigned pkx = peaks[b], pky = peaks[(long)B + b];
    if (!peak_defined(pkx) || !peak_defined(pky)) return;
    const int e = peak_exp(side == 0 ? pkx : pky);
    const float* p = reinterpret_cast<const float*>(side == 0 ? x_rows[b] : y_rows[b]);
    const long i1 = i0 + PK_CHUNK < n ? i0 + PK_CHUNK : n;
    long long s = 0;
#pragma unroll 4
    for (long i = i0 + tid; i < i1; i += PK_THREADS) {
        const int q = quantise(p[i], e);
        s += q < 0 ? -q : q;
    }
    s = wave_sum_i64(s);
    __shared__ long long wsum[PK_THREADS / 64];
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < PK_THREADS / 64; ++w) s += wsum[w];
    if (s != 0) atomic_add_i64(sums + (long)side * B + b, s);
}

// grid (chunks of x * lag blocks, B)
__global__ __launch_bounds__(AL_THREADS) void align_corr_kernel(const void* const* __restrict__ x_rows,
                                                                const void* const* __restrict__ y_rows,
                                                                const int64_t* __restrict__ n_x, const int64_t* __restrict__ n_y,
                                                                long max_nx, long max_ny, int L, int mode, int lag_blocks,
                                                                const unsigned* __restrict__ peaks,
                                                                const long long* __restrict__ sums, long long* __restrict__ cws,
                                                                int B) {
    __shared__ __attribute__((aligned(16))) unsigned xh[AL_C / 2];     // x pairs, high digits
    __shared__ __attribute__((aligned(16))) unsigned xl[AL_C / 2];     // x pairs, low digits
    __shared__ __attribute__((aligned(16))) unsigned yb[AL_YB * 8];    // y pairs: block k = E[4k .. 4k+3], O[4k .. 4k+3]
    __shared__ __attribute__((aligned(16))) long long red[AL_WAVES * AL_G];
    __shared__ short raw[AL_RAW];
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long nx = clamp_len(n_x, b, max_nx), ny = clamp_len(n_y, b, max_ny);
    if (nx <= 0 || ny <= 0) return;  // uniform over the workgroup, like every return below
    const int chunk = blockIdx.x / lag_blocks, lb = blockIdx.x - chunk * lag_blocks;
    const long i0 = (long)chunk * AL_C;
    if (i0 >= nx) return;
    const long d0 = (long)lb * AL_G - L;     // the block's first lag
    const long ys = i0 + d0;                 // the y sample that faces x[i0] at lag d0
    if (ys >= ny || ys + AL_C + AL_G <= 0) return;  // the whole span lies outside y: every product is 0
    const unsigned pkx = peaks[b], pky = peaks[(long)B + b];
    if (!peak_defined(pkx) || !peak_defined(pky) || pkx == 0u || pky == 0u) return;  // not defined, or a silent side: c stays 0
    const int ex = peak_exp(pkx), ey = peak_exp(pky);
    int mux = 0, muy = 0;
    if (mode == SWC_ALIGN_ENVELOPE) {
        mux = (int)(sums[b] / nx);
        muy = (int)(sums[(long)B + b] / ny);
    }
    const float* xrow = reinterpret_cast<const float*>(x_rows[b]);
    const float* yrow = reinterpret_cast<const float*>(y_rows[b]);

    // ---- the y span as int16, the x chunk as digit pairs ----
    for (int k = tid; k < AL_RAW; k += AL_THREADS) {
        const long g = ys + k;
        raw[k] = (short)((g >= 0 && g < ny) ? sequence(quantise(yrow[g], ey), mode, muy) : 0);
    }
    for (int k = tid; k < AL_C / 2; k += AL_THREADS) {
        const long g = i0 + 2 * k;
        const int a0 = g < nx ? sequence(quantise(xrow[g], ex), mode, mux) : 0;
        const int a1 = g + 1 < nx ? sequence(quantise(xrow[g + 1], ex), mode, mux) : 0;
        const int h0 = (a0 + 128) >> 8, h1 = (a1 + 128) >> 8;
        xh[k] = pack16(h0, h1);
        xl[k] = pack16(a0 - 256 * h0, a1 - 256 * h1);
    }
    __syncthreads();
    for (int k = tid; k < 4 * AL_YB; k += AL_THREADS) {  // 2 k + 2 <= 8 AL_YB < AL_RAW
        const int q0 = raw[2 * k], q1 = raw[2 * k + 1], q2 = raw[2 * k + 2];
        unsigned* blk = yb + (k >> 2) * 8 + (k & 3);
        blk[0] = pack16(q0, q1);
        blk[4] = pack16(q1, q2);
    }
    __syncthreads();

    // ---- c over this wave's quarter of the chunk, four lags per lane ----
    const int m = lane >> 1, p = lane & 1;
    const uint4* xh4 = reinterpret_cast<const uint4*>(xh);
    const uint4* xl4 = reinterpret_cast<const uint4*>(xl);
    const uint4* yb4 = reinterpret_cast<const uint4*>(yb);
    const int jw = wave * AL_WB;  // jw + jb + 1 + m <= AL_XB - 1 + 1 + 31 = AL_YB - 1
    long long sh[4] = {0, 0, 0, 0}, sl[4] = {0, 0, 0, 0};
    for (int jb0 = 0; jb0 < AL_WB; jb0 += AL_SPILL) {
        int ch[4] = {0, 0, 0, 0}, cl[4] = {0, 0, 0, 0};
        uint4 s0 = yb4[2 * (jw + jb0 + m) + p];
        for (int jb = jb0; jb < jb0 + AL_SPILL; ++jb) {
            const uint4 s1 = yb4[2 * (jw + jb + 1 + m) + p];
            const uint4 vh = xh4[jw + jb], vl = xl4[jw + jb];
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
    for (int i = 0; i < 4; ++i) red[wave * AL_G + 8 * m + p + 2 * i] = 256 * sh[i] + sl[i];
    __syncthreads();
    long long v = 0;
#pragma unroll
    for (int w = 0; w < AL_WAVES; ++w) v += red[w * AL_G + tid];
    const long d = d0 + tid;
    if (d <= L && v != 0) atomic_add_i64(cws + (long)b * (2L * L + 1) + (d + L), v);
}

// grid (B): one workgroup per pair
__global__ __launch_bounds__(AL_THREADS) void align_pick_kernel(const int64_t* __restrict__ n_x, const int64_t* __restrict__ n_y,
                                                                long max_nx, long max_ny, int L,
                                                                const unsigned* __restrict__ peaks,
                                                                const long long* __restrict__ cws, long long* __restrict__ acc,
                                                                int32_t* __restrict__ info, int64_t* __restrict__ xc, long ldc,
                                                                int B) {
    __shared__ long long best_c[AL_THREADS];
    __shared__ int best_d[AL_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long nx = clamp_len(n_x, b, max_nx), ny = clamp_len(n_y, b, max_ny);
    const long nl = 2L * L + 1;
    const long long* c = cws + (long)b * nl;
    const bool ok = nx > 0 && ny > 0 && peak_defined(peaks[b]) && peak_defined(peaks[(long)B + b]);
    // c is 0 everywhere for a pair that is empty or not defined: the correlation kernel added nothing.
    // The choice in two order-free steps: the largest c (an int64 maximum), then among the lags that reach it the smallest
    // key 2 |d| + (d < 0) (an integer minimum): the smaller |d| first, then d >= 0.
    long long bc = 0;
    for (long k = tid; k < nl; k += AL_THREADS) {
        const long long v = c[k];
        if (xc != nullptr) xc[(long)b * ldc + k] = v;
        bc = v > bc ? v : bc;
    }
    best_c[tid] = bc;
    __syncthreads();
    for (int o = AL_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const long long c2 = best_c[tid + o];
            if (c2 > best_c[tid]) best_c[tid] = c2;
        }
        __syncthreads();
    }
    const long long cmax = best_c[0];  // 0 without a positive c
    int key = 0x7fffffff;
    if (cmax > 0) {
        for (long k = tid; k < nl; k += AL_THREADS) {
            if (c[k] == cmax) {
                const int d = (int)(k - L);
                const int kd = d < 0 ? 2 * -d + 1 : 2 * d;
                key = kd < key ? kd : key;
            }
        }
    }
    best_d[tid] = key;
    __syncthreads();
    for (int o = AL_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const int k2 = best_d[tid + o];
            if (k2 < best_d[tid]) best_d[tid] = k2;
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const int kbest = best_d[0];
    const int dstar = ok && cmax > 0 ? ((kbest & 1) ? -(kbest >> 1) : (kbest >> 1)) : 0;
    acc[(long)b * AL_ACC + 4] = dstar;  // for the energy and value kernels
    if (info != nullptr) {
        const long x0 = dstar < 0 ? -(long)dstar : 0, y0 = dstar > 0 ? dstar : 0;
        long mlen = nx - x0 < ny - y0 ? nx - x0 : ny - y0;
        mlen = ok && mlen > 0 ? mlen : 0;
        int32_t* o = info + (long)b * SWC_ALIGN_INFO;
        o[0] = dstar;
        o[1] = ok ? (int32_t)x0 : 0;
        o[2] = ok ? (int32_t)y0 : 0;
        o[3] = (int32_t)mlen;
    }
}

// grid (chunks of the overlap, B): the four int64 energies over x[x0 .. x0 + m), y[y0 .. y0 + m), integer atomics into acc
__global__ __launch_bounds__(PK_THREADS) void align_energy_kernel(const void* const* __restrict__ x_rows,
                                                                  const void* const* __restrict__ y_rows,
                                                                  const int64_t* __restrict__ n_x, const int64_t* __restrict__ n_y,
                                                                  long max_nx, long max_ny, int mode,
                                                                  const unsigned* __restrict__ peaks,
                                                                  const long long* __restrict__ sums, long long* __restrict__ acc,
                                                                  int B) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const long nx = clamp_len(n_x, b, max_nx), ny = clamp_len(n_y, b, max_ny);
    if (nx <= 0 || ny <= 0) return;
    const unsigned pkx = peaks[b], pky = peaks[(long)B + b];
    if (!peak_defined(pkx) || !peak_defined(pky)) return;
    const int dstar = (int)acc[(long)b * AL_ACC + 4];
    const long x0 = dstar < 0 ? -(long)dstar : 0, y0 = dstar > 0 ? dstar : 0;
    const long mlen = nx - x0 < ny - y0 ? nx - x0 : ny - y0;
    const long i0 = (long)blockIdx.x * EN_CHUNK;
    if (i0 >= mlen) return;
    const long i1 = i0 + EN_CHUNK < mlen ? i0 + EN_CHUNK : mlen;
    const int ex = peak_exp(pkx), ey = peak_exp(pky);
    int mux = 0, muy = 0;
    if (mode == SWC_ALIGN_ENVELOPE) {
        mux = (int)(sums[b] / nx);
        muy = (int)(sums[(long)B + b] / ny);
    }
    const float* xrow = reinterpret_cast<const float*>(x_rows[b]) + x0;  // reads [i0, i1) of it: inside [0, nx)
    const float* yrow = reinterpret_cast<const float*>(y_rows[b]) + y0;
    long long sxx = 0, syy = 0, exx = 0, eyy = 0;
#pragma unroll 4
    for (long i = i0 + tid; i < i1; i += PK_THREADS) {
        const int qx = quantise(xrow[i], ex), qy = quantise(yrow[i], ey);
        const int vx = sequence(qx, mode, mux), vy = sequence(qy, mode, muy);
        sxx += (long long)(vx * vx);
        syy += (long long)(vy * vy);
        exx += (long long)(qx * qx);
        eyy += (long long)(qy * qy);
    }
    sxx = wave_sum_i64(sxx);
    syy = wave_sum_i64(syy);
    exx = wave_sum_i64(exx);
    eyy = wave_sum_i64(eyy);
    __shared__ long long we[PK_THREADS / 64][4];
    if ((tid & 63) == 0) {
        we[tid >> 6][0] = sxx;
        we[tid >> 6][1] = syy;
        we[tid >> 6][2] = exx;
        we[tid >> 6][3] = eyy;
    }
    __syncthreads();
    if (tid >= 4) return;
    long long v = 0;
#pragma unroll
    for (int w = 0; w < PK_THREADS / 64; ++w) v += we[w][tid];
    if (v != 0) atomic_add_i64(acc + (long)b * AL_ACC + tid, v);
}

// one thread per pair: corr and gain from the energies, each operation rounded on its own
__global__ __launch_bounds__(64) void align_values_kernel(const int64_t* __restrict__ n_x, const int64_t* __restrict__ n_y, long max_nx,
                                                          long max_ny, int L, const unsigned* __restrict__ peaks,
                                                          const long long* __restrict__ cws, const long long* __restrict__ acc,
                                                          float* __restrict__ values, int B) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const long nx = clamp_len(n_x, b, max_nx), ny = clamp_len(n_y, b, max_ny);
    const unsigned pkx = peaks[b], pky = peaks[(long)B + b];
    const bool ok = nx > 0 && ny > 0 && peak_defined(pkx) && peak_defined(pky);
    const long long* a = acc + (long)b * AL_ACC;
    const double nan = __builtin_nan("");
    double corr = nan, gain = nan;
    if (ok) {
        const long long sxx = a[0], syy = a[1], exx = a[2], eyy = a[3];
        const int dstar = (int)a[4];
        const double prod = __dmul_rn((double)sxx, (double)syy);
        if (prod != 0.0) corr = __ddiv_rn((double)cws[(long)b * (2L * L + 1) + (dstar + L)], __dsqrt_rn(prod));
        if (eyy != 0) gain = ldexp(__dsqrt_rn(__ddiv_rn((double)exx, (double)eyy)), peak_exp(pkx) - peak_exp(pky));
    }
    float* o = values + (long)b * SWC_ALIGN_VALUES;
    o[0] = (float)corr;
    o[1] = (float)gain;
    o[2] = 0.0f;
    o[3] = 0.0f;
}

bool limits_ok(int B, long max_nx, long max_ny, int L) {
    return B >= 0 && B <= 65535 && max_nx >= 0 && max_nx <= SWC_ALIGN_MAX_N && max_ny >= 0 && max_ny <= SWC_ALIGN_MAX_N && L >= 0 &&
           L <= SWC_ALIGN_MAX_LAG;
}

// where swc_align keeps what inside its workspace (byte offsets): the peaks [2][B] u32, the sums of |q| [2][B] i64, the
// accumulators [B][AL_ACC] i64 and c [B][2 L + 1] i64
struct WsLayout {
    size_t peaks, sums, acc, c, total;
};

WsLayout ws_layout(int B, int L) {
    WsLayout P;
    size_t o = 0;
    P.peaks = o; o += up256((size_t)2 * B * sizeof(unsigned));
    P.sums = o; o += up256((size_t)2 * B * sizeof(long long));
    P.acc = o; o += up256((size_t)AL_ACC * B * sizeof(long long));
    P.c = o; o += up256((size_t)B * (size_t)(2L * L + 1) * sizeof(long long));
    P.total = o;
    return P;
}

}  // namespace

extern "C" int64_t swc_align_workspace_bytes(int32_t B, int64_t max_nx, int64_t max_ny, int32_t L) {
    if (!limits_ok(B, max_nx, max_ny, L)) return -1;
    return (int64_t)ws_layout(B, L).total;
}

extern "C" int swc_align(const void* const* x_rows, const void* const* y_rows, const int64_t* n_x, const int64_t* n_y,
                         int64_t max_nx, int64_t max_ny, int32_t L, int32_t mode, int32_t* info, float* values, int64_t* xc,
                         int64_t ldc, void* workspace, int64_t workspace_bytes, int32_t B, void* stream) {
    SWC_CHECK_ARG(x_rows && y_rows && n_x && n_y && workspace, "swc_align: null pointer");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_align: B=%d (0..65535)", B);
    SWC_CHECK_ARG(max_nx >= 0 && max_nx <= SWC_ALIGN_MAX_N && max_ny >= 0 && max_ny <= SWC_ALIGN_MAX_N,
                  "swc_align: max_nx=%ld, max_ny=%ld out of range (0..%d)", (long)max_nx, (long)max_ny, SWC_ALIGN_MAX_N);
    SWC_CHECK_ARG(L >= 0 && L <= SWC_ALIGN_MAX_LAG, "swc_align: search range L=%d (0..%d)", L, SWC_ALIGN_MAX_LAG);
    SWC_CHECK_ARG(mode == SWC_ALIGN_WAVEFORM || mode == SWC_ALIGN_ENVELOPE, "swc_align: mode=%d (0 waveform, 1 envelope)", mode);
    const long nl = 2L * L + 1;
    SWC_CHECK_ARG(xc == nullptr || ldc >= nl, "swc_align: ldc=%ld, %ld lags", (long)ldc, nl);
    const WsLayout P = ws_layout(B, L);
    SWC_CHECK_ARG(workspace_bytes >= (int64_t)P.total, "swc_align: workspace of %ld bytes, %ld needed (swc_align_workspace_bytes)",
                  (long)workspace_bytes, (long)P.total);
    SWC_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "swc_align: workspace must be 256-byte aligned");
    if (B == 0) return SWC_OK;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* base = reinterpret_cast<unsigned char*>(workspace);
    unsigned* peaks = reinterpret_cast<unsigned*>(base + P.peaks);
    long long* sums = reinterpret_cast<long long*>(base + P.sums);
    long long* acc = reinterpret_cast<long long*>(base + P.acc);
    long long* cws = reinterpret_cast<long long*>(base + P.c);
    if (hipMemsetAsync(workspace, 0, P.total, st) != hipSuccess) {
        (void)hipGetLastError();
        swc_set_error("swc_align: clearing the accumulators failed");
        return SWC_E_LAUNCH;
    }
    const long max_nx_l = max_nx, max_ny_l = max_ny;
    const long max_n = max_nx_l > max_ny_l ? max_nx_l : max_ny_l;
    if (max_nx_l > 0 && max_ny_l > 0) {
        const long chunks = (max_n + PK_CHUNK - 1) / PK_CHUNK;
        hipLaunchKernelGGL(align_peak_kernel, dim3((unsigned)chunks, (unsigned)B, 2u), dim3(PK_THREADS), 0, st, x_rows, y_rows, n_x,
                           n_y, max_nx_l, max_ny_l, peaks, B);
        SWC_CHECK_LAUNCH("swc_align (peak)");
        if (mode == SWC_ALIGN_ENVELOPE) {
            hipLaunchKernelGGL(align_abs_kernel, dim3((unsigned)chunks, (unsigned)B, 2u), dim3(PK_THREADS), 0, st, x_rows, y_rows,
                               n_x, n_y, max_nx_l, max_ny_l, (const unsigned*)peaks, sums, B);
            SWC_CHECK_LAUNCH("swc_align (abs)");
        }
        const long xchunks = (max_nx_l + AL_C - 1) / AL_C;          // <= 1024
        const int lag_blocks = (int)((nl + AL_G - 1) / AL_G);       // <= 257
        hipLaunchKernelGGL(align_corr_kernel, dim3((unsigned)(xchunks * lag_blocks), (unsigned)B), dim3(AL_THREADS), 0, st, x_rows,
                           y_rows, n_x, n_y, max_nx_l, max_ny_l, L, mode, lag_blocks, (const unsigned*)peaks,
                           (const long long*)sums, cws, B);
        SWC_CHECK_LAUNCH("swc_align (corr)");
    }
    if (info != nullptr || values != nullptr || xc != nullptr) {
        hipLaunchKernelGGL(align_pick_kernel, dim3((unsigned)B), dim3(AL_THREADS), 0, st, n_x, n_y, max_nx_l, max_ny_l, L,
                           (const unsigned*)peaks, (const long long*)cws, acc, info, xc, (long)ldc, B);
        SWC_CHECK_LAUNCH("swc_align (pick)");
    }
    if (values != nullptr) {
        const long min_n = max_nx_l < max_ny_l ? max_nx_l : max_ny_l;  // no overlap is longer
        if (min_n > 0) {
            const long chunks = (min_n + EN_CHUNK - 1) / EN_CHUNK;
            hipLaunchKernelGGL(align_energy_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(PK_THREADS), 0, st, x_rows, y_rows, n_x,
                               n_y, max_nx_l, max_ny_l, mode, (const unsigned*)peaks, (const long long*)sums, acc, B);
            SWC_CHECK_LAUNCH("swc_align (energy)");
        }
        hipLaunchKernelGGL(align_values_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, n_x, n_y, max_nx_l, max_ny_l, L,
                           (const unsigned*)peaks, (const long long*)cws, (const long long*)acc, values, B);
        SWC_CHECK_LAUNCH("swc_align (values)");
    }
    return SWC_OK;
}
