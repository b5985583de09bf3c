// What the metric calls share (swc_stoi.hip, swc_spectral.hip, swc_pitch.hip, swc_align.hip, swc_mcd.hip): the workspace rounding, the
// clamp of a row's length, the int16 quantisation against a row's peak and the packed 16-bit dot product.  Helpers only: no
// kernel lives here, and nothing is a template over its callers.
//
// pitch_peak_kernel and align_peak_kernel stay two kernels: pitch issues one atomicMax per WAVE, align one per WORKGROUP
// (a row's atomics all meet at one address; measured for swc_align only).  One kernel for both wants
// that measurement for swc_pitch first: it changes device code.
#pragma once
#include "swc_common.h"

typedef short i16x2 __attribute__((ext_vector_type(2)));

// every part of a metric workspace starts on a multiple of 256 bytes
static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// n[b] clamped into [0, max_n]: the device never trusts a length beyond the bound the host sized the launch for
__device__ __forceinline__ long clamp_len(const int64_t* n, int b, long max_n) {
    const long v = n[b];
    return v < 0 ? 0 : (v > max_n ? max_n : v);
}

// a row's peak is the unsigned maximum over the bit patterns of |v|: any NaN or Inf wins, and the row is then not defined.
// One spot keeps the literal: pitch_frames_kernel tests `pk == 0u || pk >= 0x7f800000u`; with `!peak_defined(pk)` there the
// compiler folds the two tests differently and the kernel's code changes (tools/isa_equal.py).
__device__ __forceinline__ bool peak_defined(unsigned pk) { return pk < 0x7f800000u; }

__device__ __forceinline__ int peak_exp(unsigned pk) {
    int e = 0;
    if (pk != 0u) (void)frexpf(__uint_as_float(pk), &e);  // peak = m 2^e, m in [0.5, 1)
    return e;
}

// q = clamp(rint(v 2^(15 - e)), +-32767): the product is exact, one rounding in rint
__device__ __forceinline__ int quantise(float v, int e) {
    double r = rint(ldexp((double)v, 15 - e));
    r = r > 32767.0 ? 32767.0 : (r < -32767.0 ? -32767.0 : r);
    return (int)r;
}

__device__ __forceinline__ unsigned pack16(int lo, int hi) { return ((unsigned)lo & 0xffffu) | ((unsigned)hi << 16); }

__device__ __forceinline__ int dot2(unsigned a, unsigned b, int c) {
    return __builtin_amdgcn_sdot2(*reinterpret_cast<const i16x2*>(&a), *reinterpret_cast<const i16x2*>(&b), c, false);
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
