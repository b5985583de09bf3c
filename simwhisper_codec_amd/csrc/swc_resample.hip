// Sample-rate conversion on the device (include/swc_audio.h): a ragged batch of f32 or interleaved int16 rows ->
// the zero-padded f32 batch at the codec's rate, one launch per (orig, new) pair.
//
// A streaming kernel: a workgroup of 256 threads owns `tile` consecutive output samples of one row (grid = tiles x rows).
// It stages the input span those samples read (down-mixed and scaled to f32 on the way in: 16-byte loads where the
// row's address allows, element loads at ragged edges and odd addresses) and the packed filter phases they use in
// LDS, then every thread computes 4 consecutive outputs, each as ONE ascending fmaf chain over the `run` packed taps
// of its phase, and writes them as one 16-byte store where the output address allows.  The chain is the same whatever
// the tile, the row index or the alignment, so an output sample's bits depend on its row's samples and the table only.
#include "swc_common.h"
#include "swc_audio.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_PER_THREAD = 4;

// MODE 0: f32 mono rows.  MODE 1, 2, 4, 8: int16 rows of MODE interleaved channels (a 16-byte vector holds whole frames
// when the row's address is a multiple of the frame size).  MODE 9: int16, any other channel count (element loads only).
template <int MODE>
__device__ __forceinline__ float mono_at(const void* src, long i, int ch, float scale) {
    if constexpr (MODE == 0) {
        return reinterpret_cast<const float*>(src)[i];
    } else {
        const short* s = reinterpret_cast<const short*>(src) + i * ch;
        int sum = 0;
        for (int c = 0; c < ch; ++c) sum += (int)s[c];
        return __fmul_rn((float)sum, scale);
    }
}

// xs[s] = xpad[lo + s] for s in [0, span): samples of the row inside [0, n), zeros outside
template <int MODE>
__device__ __forceinline__ void stage_span(float* xs, const void* src, long n, long lo, int span, int ch, float scale, int tid) {
    constexpr int VL = MODE == 0 ? 4 : (MODE == 9 ? 1 : 8 / MODE);  // mono samples per 16-byte vector
    const uintptr_t addr = reinterpret_cast<uintptr_t>(src);
    bool vec = MODE != 9;
    int shift = 0;  // the row starts `shift` mono samples behind a 16-byte boundary
    if constexpr (MODE == 0) {
        shift = (int)((addr >> 2) & 3);
    } else if constexpr (MODE != 9) {
        const int a = (int)((addr >> 1) & 7);
        vec = a % MODE == 0;
        shift = a / MODE;
    }
    if (n == 0) vec = false;  // (an empty row's address is not looked at)
    if (!vec) {
        for (int s = tid; s < span; s += RS_THREADS) {
            const long i = lo + s;
            xs[s] = (i >= 0 && i < n) ? mono_at<MODE>(src, i, ch, scale) : 0.0f;
        }
        return;
    }
    if constexpr (MODE != 9) {
        // vector v covers xs[VL v - m, VL v - m + VL): mono samples whose address is 16-byte aligned
        const int m = (int)((lo + shift) & (VL - 1));
        const int nvec = (span - 1 + m) / VL + 1;
        for (int v = tid; v < nvec; v += RS_THREADS) {
            const int s0 = VL * v - m;
            const long i0 = lo + s0;
            float f[VL];
            if (i0 >= 0 && i0 + VL <= n) {
                if constexpr (MODE == 0) {
                    const float4 q = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(src) + i0);
                    f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
                } else {
                    const uint4 q = *reinterpret_cast<const uint4*>(reinterpret_cast<const short*>(src) + i0 * MODE);
                    const unsigned w[4] = {q.x, q.y, q.z, q.w};
                    int h[8];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        h[2 * k] = (int)(short)(w[k] & 0xFFFFu);
                        h[2 * k + 1] = (int)(short)(w[k] >> 16);
                    }
#pragma unroll
                    for (int g = 0; g < VL; ++g) {
                        int sum = 0;
#pragma unroll
                        for (int c = 0; c < MODE; ++c) sum += h[g * MODE + c];
                        f[g] = __fmul_rn((float)sum, scale);
                    }
                }
            } else {
#pragma unroll
                for (int g = 0; g < VL; ++g) {
                    const long i = i0 + g;
                    f[g] = (i >= 0 && i < n) ? mono_at<MODE>(src, i, ch, scale) : 0.0f;
                }
            }
#pragma unroll
            for (int g = 0; g < VL; ++g)
                if (s0 + g >= 0 && s0 + g < span) xs[s0 + g] = f[g];
        }
    }
}

__device__ __forceinline__ void store4(float* orow, long j, long jend, const float (&y)[RS_PER_THREAD]) {
    if (j + RS_PER_THREAD <= jend && (reinterpret_cast<uintptr_t>(orow + j) & 15) == 0) {
        *reinterpret_cast<float4*>(orow + j) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
        for (int i = 0; i < RS_PER_THREAD; ++i)
            if (j + i < jend) orow[j + i] = y[i];
    }
}

template <int MODE>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const void* const* __restrict__ rows, const int64_t* __restrict__ n_in,
                                                              int ch, float scale, int orig, int new_, int width,
                                                              const float* __restrict__ taps_packed,
                                                              const int* __restrict__ tap_start, int run,
                                                              float* __restrict__ out, long ld_out, long cols, int tile,
                                                              int span_max) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const long j0 = (long)blockIdx.x * tile;
    float* orow = out + (long)b * ld_out;
    long n = n_in[b];
    if (n < 0) n = 0;
    const long n_out = (n * new_ + orig - 1) / orig;
    const long jend = j0 + tile < cols ? j0 + tile : cols;  // this tile writes [j0, jend)
    const long jv = jend < n_out ? jend : n_out;            // ... samples in [j0, jv), zeros behind
    if (jv <= j0) {  // (uniform over the workgroup)
        const float z[RS_PER_THREAD] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int u4 = tid * RS_PER_THREAD; j0 + u4 < jend; u4 += RS_THREADS * RS_PER_THREAD) store4(orow, j0 + u4, jend, z);
        return;
    }
    const int taps = 2 * width + orig;
    const int rs = run | 1;  // odd row stride: consecutive phases fall on different LDS banks
    const int nph = new_ < tile ? new_ : tile;
    float* xs = smem;
    float* tab = smem + span_max;
    int* st = reinterpret_cast<int*>(tab + nph * rs);
    const long f0 = j0 / new_;
    const int r0 = (int)(j0 - f0 * new_);
    const int span = (int)((jv - 1) / new_ - f0) * orig + taps;  // <= span_max
    const long lo = f0 * orig - width;                            // xs[s] = x[lo + s]
    // the phases of this tile: all of them, or (new_ > tile) one per output sample, phase (r0 + u) mod new_ in slot u
    for (int idx = tid; idx < nph * run; idx += RS_THREADS) {
        const int s = idx / run, k = idx - s * run;
        int p = s;
        if (new_ > tile) {
            p = r0 + s;
            if (p >= new_) p -= new_;
        }
        tab[s * rs + k] = taps_packed[(long)p * run + k];
    }
    for (int s = tid; s < nph; s += RS_THREADS) {
        int p = s;
        if (new_ > tile) {
            p = r0 + s;
            if (p >= new_) p -= new_;
        }
        st[s] = tap_start[p];
    }
    stage_span<MODE>(xs, rows[b], n, lo, span, ch, scale, tid);
    __syncthreads();
    for (int u4 = tid * RS_PER_THREAD; j0 + u4 < jend; u4 += RS_THREADS * RS_PER_THREAD) {
        const long j = j0 + u4;
        int xb[RS_PER_THREAD], tb[RS_PER_THREAD];
        float acc[RS_PER_THREAD];
#pragma unroll
        for (int i = 0; i < RS_PER_THREAD; ++i) {
            const int u = j + i < jv ? u4 + i : 0;  // (a lane behind the row's end computes sample j0 again and drops it)
            const unsigned t = (unsigned)(r0 + u);
            const unsigned q = t / (unsigned)new_;
            const int p = (int)(t - q * (unsigned)new_);
            const int slot = new_ > tile ? u : p;
            xb[i] = (int)q * orig + st[slot];
            tb[i] = slot * rs;
            acc[i] = 0.0f;
        }
        for (int k = 0; k < run; ++k) {
#pragma unroll
            for (int i = 0; i < RS_PER_THREAD; ++i) acc[i] = fmaf(tab[tb[i] + k], xs[xb[i] + k], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < RS_PER_THREAD; ++i)
            if (j + i >= jv) acc[i] = 0.0f;
        store4(orow, j, jend, acc);
    }
}

// LDS floats of a tile: the input span of `tile` outputs, the phases it uses (odd row stride) and their starts
long tile_floats(int tile, int orig, int new_, int taps, int run) {
    const long nph = new_ < tile ? new_ : tile;
    return ((long)(tile - 1) / new_ + 1) * orig + taps + nph * (run | 1) + nph;
}

}  // namespace

extern "C" int64_t swc_resample_out_len(int64_t n_in, int32_t orig_rate, int32_t new_rate) {
    if (orig_rate < 1 || new_rate < 1) return -1;
    if (n_in <= 0) return 0;
    return (n_in * new_rate + orig_rate - 1) / orig_rate;
}

extern "C" int swc_resample(const void* const* rows, const int64_t* n_in, int32_t in_format, int32_t ch, int32_t orig,
                            int32_t new_, int32_t width, const float* taps_packed, const int32_t* tap_start, int32_t run,
                            float* out, int64_t ld_out, int64_t cols, int32_t B, void* stream) {
    SWC_CHECK_ARG(rows && n_in && taps_packed && tap_start && out, "swc_resample: null pointer");
    SWC_CHECK_ARG(in_format == SWC_PCM_F32 || in_format == SWC_PCM_I16, "swc_resample: in_format must be SWC_PCM_F32 or SWC_PCM_I16");
    SWC_CHECK_ARG(orig >= 1 && new_ >= 1, "swc_resample: rates must be >= 1 (orig=%d new=%d)", orig, new_);
    SWC_CHECK_ARG(ch >= 1 && ch <= 8 && (in_format == SWC_PCM_I16 || ch == 1),
                  "swc_resample: ch=%d (1..8 for int16 rows, 1 for f32 rows)", ch);
    SWC_CHECK_ARG(width >= 0 && width <= (1 << 20) && orig <= (1 << 20) && new_ <= (1 << 20), "swc_resample: width or ratio out of range");
    const int taps = 2 * width + orig;
    SWC_CHECK_ARG(run >= 1 && run <= taps, "swc_resample: table size: run=%d must be in 1..%d (2 width + orig)", run, taps);
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_resample: B=%d (0..65535)", B);
    SWC_CHECK_ARG(cols >= 0 && cols <= ld_out, "swc_resample: cols=%ld must be in 0..ld_out=%ld", (long)cols, (long)ld_out);
    int tile = 2048;
    while (tile > 256 && tile_floats(tile, orig, new_, taps, run) > SWC_RESAMPLE_MAX_LDS_FLOATS) tile >>= 1;
    SWC_CHECK_ARG(tile_floats(tile, orig, new_, taps, run) <= SWC_RESAMPLE_MAX_LDS_FLOATS,
                  "swc_resample: the ratio %d:%d with %d taps (run %d) does not fit the LDS tile", orig, new_, taps, run);
    if (B == 0 || cols == 0) return SWC_OK;
    const long tiles = (cols + tile - 1) / tile;
    SWC_CHECK_ARG(tiles <= 0x7fffffffL, "swc_resample: cols too large");
    const int span_max = (int)(((long)(tile - 1) / new_ + 1) * orig + taps);
    const size_t lds = (size_t)tile_floats(tile, orig, new_, taps, run) * sizeof(float);
    const float scale = (float)(0x1p-15 / (double)ch);
    const dim3 grid((unsigned)tiles, (unsigned)B), block(RS_THREADS);
#define SWC_RS_LAUNCH(MODE)                                                                                            \
    hipLaunchKernelGGL(resample_kernel<MODE>, grid, block, lds, (hipStream_t)stream, rows, n_in, (int)ch, scale, (int)orig, \
                       (int)new_, (int)width, taps_packed, (const int*)tap_start, (int)run, out, (long)ld_out, (long)cols, tile, span_max)
    if (in_format == SWC_PCM_F32) SWC_RS_LAUNCH(0);
    else if (ch == 1) SWC_RS_LAUNCH(1);
    else if (ch == 2) SWC_RS_LAUNCH(2);
    else if (ch == 4) SWC_RS_LAUNCH(4);
    else if (ch == 8) SWC_RS_LAUNCH(8);
    else SWC_RS_LAUNCH(9);
#undef SWC_RS_LAUNCH
    SWC_CHECK_LAUNCH("swc_resample");
    return SWC_OK;
}
