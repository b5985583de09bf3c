// What swc_dtw (swc_mcd.hip) and swc_subdtw (swc_subdtw.hip) share, so that the two calls quantise and charge a pair of frames
// in exactly one way (include/swc_mcd.h "scale" and "cost"): the limits and their bounds, the clamp of a frame count, the 13-bit
// quantisation, the exact integer distance of two quantised frames, and the two kernels that find a pair's peak and write its
// two quantised sides into the workspace.  Everything has internal linkage: each translation unit gets its own copy.
#pragma once
#include "swc_metric_common.h"
#include "swc_mcd.h"

namespace {

typedef unsigned long long u64;

constexpr int DT_THREADS = 256;
constexpr int DT_S = SWC_DTW_STRIP;        // rows of a strip: one per thread
constexpr int DT_QW = SWC_DTW_MAX_D / 2;   // dwords of a quantised frame in the workspace (32 int16)
constexpr int DT_PK_FRAMES = 128;          // frames per workgroup of the peak and quantise kernels
constexpr int DT_NBITS = 14;               // bits of N in a key
constexpr int DT_QMAX = (1 << SWC_DTW_QBITS) - 1;
constexpr u64 DT_INF = ~0ull;              // the key of a cell that is not allowed or not reachable
constexpr long long DT_DMAX = 91LL * 2 * DT_QMAX;  // d <= sqrt(256 * 32) * 16382 < 91 * 16382
static_assert(DT_S == DT_THREADS, "a thread owns one row of a strip");
static_assert(2 * DT_QMAX <= 32767, "a difference of two quantised features fits int16");
static_assert(8LL * (2 * DT_QMAX) * (2 * DT_QMAX) < (1LL << 31), "eight squared differences fit an int32");
static_assert((long long)SWC_DTW_MAX_D * (2 * DT_QMAX) * (2 * DT_QMAX) < (1LL << 33), "s < 2^33, so 256 s < 2^41 is exact in float64");
static_assert(DT_DMAX * DT_DMAX >= 256LL * SWC_DTW_MAX_D * (2 * DT_QMAX) * (2 * DT_QMAX) && DT_DMAX < (1LL << 21), "d < 2^21");
static_assert(2 * SWC_DTW_MAX_FRAMES - 1 < (1 << DT_NBITS), "N <= 16383 fits the key's low bits");
static_assert(DT_DMAX * (2LL * SWC_DTW_MAX_FRAMES - 1) < (1LL << 35), "C < 2^35, so a key is below 2^49");

__device__ __forceinline__ int clamp_frames(const int32_t* t, int b, int t_max) {
    const int v = t[b];
    return v < 0 ? 0 : (v > t_max ? t_max : v);
}

// q = clamp(rint(v 2^(13 - e)), +-8191): the product is exact, one rounding in rint
__device__ __forceinline__ int quantise13(float v, int e) {
    double r = rint(ldexp((double)v, SWC_DTW_QBITS - e));
    r = r > (double)DT_QMAX ? (double)DT_QMAX : (r < -(double)DT_QMAX ? -(double)DT_QMAX : r);
    return (int)r;
}

// c + the two squared differences of a packed pair (no difference leaves int16)
__device__ __forceinline__ int sqdiff2(unsigned a, unsigned b, int c) {
    const i16x2 d = *reinterpret_cast<const i16x2*>(&a) - *reinterpret_cast<const i16x2*>(&b);
    return __builtin_amdgcn_sdot2(d, d, c, false);
}

// floor(sqrt(256 s)) for 0 <= s < 2^33: the float64 root of an exact integer is off by one at most
__device__ __forceinline__ long long root256(long long s) {
    const long long v = s << 8;
    long long r = (long long)__dsqrt_rn((double)v);
    if (r * r > v) --r;
    else if ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

template <int G>
__device__ __forceinline__ long long local_cost(const uint4 (&x)[G], const uint4 (&y)[G]) {
    long long s = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        int a = sqdiff2(x[g].x, y[g].x, 0);
        a = sqdiff2(x[g].y, y[g].y, a);
        a = sqdiff2(x[g].z, y[g].z, a);
        a = sqdiff2(x[g].w, y[g].w, a);
        s += a;
    }
    return root256(s);
}

// grid (chunks of frames, B, 2 sides)
__global__ __launch_bounds__(DT_THREADS) void dtw_peak_kernel(const float* __restrict__ xf, const float* __restrict__ yf,
                                                              const int32_t* __restrict__ tx, const int32_t* __restrict__ ty,
                                                              int tmax_x, int tmax_y, int D, long ldf, unsigned* __restrict__ peaks) {
    const int b = blockIdx.y, side = blockIdx.z, tid = threadIdx.x;
    const int Tx = clamp_frames(tx, b, tmax_x), Ty = clamp_frames(ty, b, tmax_y);
    if (Tx <= 0 || Ty <= 0) return;  // an empty pair
    const int T = side == 0 ? Tx : Ty, t0 = blockIdx.x * DT_PK_FRAMES;
    if (t0 >= T) return;
    const int nfr = T - t0 < DT_PK_FRAMES ? T - t0 : DT_PK_FRAMES;
    const unsigned* p = reinterpret_cast<const unsigned*>(side == 0 ? xf : yf) + ((long)b * (side == 0 ? tmax_x : tmax_y) + t0) * ldf;
    unsigned m = 0;
    for (int idx = tid; idx < nfr * D; idx += DT_THREADS) {
        const int t = idx / D, k = idx - t * D;
        const unsigned v = p[(long)t * ldf + k] & 0x7fffffffu;
        m = v > m ? v : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned v = (unsigned)__shfl_xor((int)m, o);
        m = v > m ? v : m;
    }
    __shared__ unsigned wm[DT_THREADS / 64];
    if ((tid & 63) == 0) wm[tid >> 6] = m;
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < DT_THREADS / 64; ++w) m = wm[w] > m ? wm[w] : m;
    if (m != 0) atomicMax(peaks + b, m);
}

// grid (chunks of frames, B, 2 sides): frame t of a side as 16 dwords of two int16 each, zero from column D on
__global__ __launch_bounds__(DT_THREADS) void dtw_quant_kernel(const float* __restrict__ xf, const float* __restrict__ yf,
                                                               const int32_t* __restrict__ tx, const int32_t* __restrict__ ty,
                                                               int tmax_x, int tmax_y, int D, long ldf,
                                                               const unsigned* __restrict__ peaks, unsigned* __restrict__ xq,
                                                               unsigned* __restrict__ yq) {
    const int b = blockIdx.y, side = blockIdx.z, tid = threadIdx.x;
    const int Tx = clamp_frames(tx, b, tmax_x), Ty = clamp_frames(ty, b, tmax_y);
    if (Tx <= 0 || Ty <= 0) return;
    const unsigned pk = peaks[b];
    if (!peak_defined(pk)) return;
    const int e = peak_exp(pk);
    const int T = side == 0 ? Tx : Ty, t_max = side == 0 ? tmax_x : tmax_y, t0 = blockIdx.x * DT_PK_FRAMES;
    if (t0 >= T) return;
    const int nfr = T - t0 < DT_PK_FRAMES ? T - t0 : DT_PK_FRAMES;
    const float* p = (side == 0 ? xf : yf) + ((long)b * t_max + t0) * ldf;
    unsigned* q = (side == 0 ? xq : yq) + ((long)b * t_max + t0) * DT_QW;
    for (int idx = tid; idx < nfr * DT_QW; idx += DT_THREADS) {
        const int t = idx / DT_QW, k = 2 * (idx - t * DT_QW);
        const int q0 = k < D ? quantise13(p[(long)t * ldf + k], e) : 0;
        const int q1 = k + 1 < D ? quantise13(p[(long)t * ldf + k + 1], e) : 0;
        q[idx] = pack16(q0, q1);
    }
}

}  // namespace
