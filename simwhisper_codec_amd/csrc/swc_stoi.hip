// STOI of a ragged batch of (clean, degraded) pairs on the device (include/swc_metrics.h): the contract is stated there.
//
// Five steps, every intermediate in the caller's workspace, no float atomics, every sum in one fixed order:
//   swc_resample (x rows, then y rows) -> x10, y10 [B][ld10]             (skipped at 10 kHz: the rows are read in place)
//   stoi_energy_kernel    one wave per frame of x10: e[b][f] in dB
//   stoi_select_kernel    one workgroup per row: max e, keep flags, exclusive scan -> src[b][0..K), K[b]
//   stoi_spectra_kernel   one workgroup per (16 STFT frames, row, signal): rebuilds the 16 x 256 compacted and twice
//                         windowed samples from the kept frames in LDS, multiplies them with the 256 x (2 x 224) DFT
//                         matrix of bins 7..230 on the f32 MFMA (v_mfma_f32_16x16x4_f32; the matrix is never stored:
//                         its 512 distinct values sit in LDS and are indexed by bin * n mod 512), squares, sums the 15
//                         bands in ascending bin order and writes sqrt -> Xt / Yt [B][15][Mmax].  The complex spectrum
//                         never leaves the chip.
//   stoi_segments_kernel  one workgroup per row: every (band, segment) normalise / clip / correlate, thread-strided in
//                         a fixed order, then a fixed tree over the 256 partial sums -> d[b], segs[b]
// A frame's band values depend on its own 256 samples only (an MFMA row never mixes with another), a row's tiles start
// at frame 0 of that row, and the reductions are ordered by the row's own S: the bits of d[b] do not depend on B, the
// row's index, its address or the grid.
//
// swc_quality (include/swc_quality.h) runs the same front end (resample .. spectra) once and then, as asked for:
//   stoi_segments_kernel  as above, untouched -> stoi[b], segs[b]
//   estoi_segments_kernel one wave per segment, SWC_ESTOI_GROUP segments per workgroup: lane l < 30 holds frame column l
//                         (15 + 15 band values in registers); the 2 x 15 row means and row norms are sums over the wave on
//                         the DPP path (lanes 30..63 hold exact zeros), the column step is lane-local, e_m one more wave sum
//                         -> eseg[b][s]
//   estoi_mean_kernel     one workgroup per row: eseg[b][0..S) thread-strided, then the 256-leaf tree -> estoi[b]
//   sisdr_sums_kernel     one workgroup per (chunk of SWC_SISDR_CHUNK samples, row), float64: pass 1 sums x, y, xx, xy,
//                         pass 2 sums (alpha x')^2 and (y' - alpha x')^2; a thread owns the same samples whatever the
//                         alignment (16-byte loads when both rows allow them, element loads otherwise: same values, same
//                         order); a fixed tree over the workgroup -> one record per (row, chunk)
//   sisdr_finish_kernel   one workgroup per row adds the records in ascending chunk order: after pass 1 -> mx, my, alpha,
//                         after pass 2 -> si_sdr[b]
#include "swc_metric_common.h"
#include "swc_audio.h"
#include "swc_metrics.h"
#include "swc_quality.h"

namespace {

constexpr int ST_FRAME = 256, ST_HOP = 128, ST_NFFT = 512, ST_J = 15, ST_N = 30;
constexpr int ST_BIN0 = 7;            // first bin any band reads
constexpr int ST_BINS = 224;          // bins 7..230 are computed (14 MFMA tiles of 16), 7..218 are used
constexpr int ST_TILE = SWC_STOI_TILE;
constexpr int ST_SPEC_WAVES = 7;      // each wave: two 16-bin tiles, real and imaginary part
constexpr int ST_SPEC_THREADS = 64 * ST_SPEC_WAVES;
constexpr int ST_LDA = 260;           // A row stride in floats: 16 rows x 4 k-columns of one fragment read fall on 64 different banks
constexpr float ST_EPS = 0x1p-52f;
constexpr float ST_CLIP = 6.623413251903491f;  // 1 + 10^(15/20)
__constant__ int c_edges[ST_J + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

struct Layout {
    long n10max, ld10, Fmax, Mmax;
    size_t x10, y10, e, src, K, Xt, Yt, total;
};

Layout layout(long B, long max_n, int orig, int new_) {
    Layout L;
    L.n10max = orig == new_ ? max_n : (max_n * new_ + orig - 1) / orig;
    L.ld10 = (L.n10max + 3) & ~3L;
    L.Fmax = L.n10max >= ST_FRAME ? (L.n10max - ST_FRAME) / ST_HOP + 1 : 0;
    L.Mmax = L.Fmax > 0 ? L.Fmax - 1 : 0;
    size_t o = 0;
    const size_t sig = orig == new_ ? 0 : up256((size_t)B * L.ld10 * 4);
    L.x10 = o; o += sig;
    L.y10 = o; o += sig;
    L.e = o; o += up256((size_t)B * L.Fmax * 4);
    L.src = o; o += up256((size_t)B * L.Fmax * 4);
    L.K = o; o += up256((size_t)B * 4);
    L.Xt = o; o += up256((size_t)B * ST_J * L.Mmax * 4);
    L.Yt = o; o += up256((size_t)B * ST_J * L.Mmax * 4);
    L.total = o;
    return L;
}

constexpr int ES_GROUP = SWC_ESTOI_GROUP;
constexpr int SD_CHUNK = SWC_SISDR_CHUNK, SD_THREADS = 256;
constexpr int SD_GROUPS = SD_CHUNK / (4 * SD_THREADS);  // groups of 4 consecutive samples one thread owns in a chunk
static_assert(SD_GROUPS * 4 * SD_THREADS == SD_CHUNK, "SWC_SISDR_CHUNK is a multiple of 1024 samples");
constexpr double SD_EPS = 0x1p-52;

// swc_quality's workspace: swc_stoi's, then eseg [B][Smax] f32, the SI-SDR records [B][chunks][4] f64 (both passes use
// them in turn), mx / my / alpha [B][4] f64, and a place for segs when the caller passes none
struct QLayout {
    Layout st;
    long Smax, chunks;
    size_t eseg, rec, stat, segs, total;
};

QLayout qlayout(long B, long max_n, int orig, int new_) {
    QLayout Q;
    Q.st = layout(B, max_n, orig, new_);
    Q.Smax = Q.st.Mmax >= ST_N ? Q.st.Mmax - ST_N + 1 : 0;
    Q.chunks = (max_n + SD_CHUNK - 1) / SD_CHUNK;
    size_t o = Q.st.total;
    Q.eseg = o; o += up256((size_t)B * Q.Smax * 4);
    Q.rec = o; o += up256((size_t)B * Q.chunks * 4 * 8);
    Q.stat = o; o += up256((size_t)B * 4 * 8);
    Q.segs = o; o += up256((size_t)B * 4);
    Q.total = o;
    return Q;
}

// w[i] = hanning(258)[1 + i], evaluated in float64 and rounded once
__device__ __forceinline__ float window_at(int i) { return (float)(0.5 - 0.5 * cospi(2.0 * (double)(i + 1) / 257.0)); }

// the row's length at 10 kHz and its number of frames (n_in clamped into [0, max_n])
__device__ __forceinline__ long len10(const int64_t* n_in, int b, long max_n, int orig, int new_) {
    const long n = clamp_len(n_in, b, max_n);
    return orig == new_ ? n : (n * new_ + orig - 1) / orig;
}
__device__ __forceinline__ int frames_of(long n10) { return n10 >= ST_FRAME ? (int)((n10 - ST_FRAME) / ST_HOP) + 1 : 0; }

// the 10 kHz signal of row b: the resampler's output, or the caller's row itself (never looked at for an empty row)
__device__ __forceinline__ const float* signal_of(const void* const* rows, const float* s10, long ld10, int b, long n10) {
    if (s10 != nullptr) return s10 + (long)b * ld10;
    return n10 > 0 ? reinterpret_cast<const float*>(rows[b]) : nullptr;
}

__global__ __launch_bounds__(256) void stoi_energy_kernel(const void* const* __restrict__ x_rows, const int64_t* __restrict__ n_in,
                                                          long max_n, int orig, int new_, const float* __restrict__ x10,
                                                          long ld10, float* __restrict__ e, long Fmax) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long n10 = len10(n_in, b, max_n, orig, new_);
    if (f >= frames_of(n10)) return;  // (uniform over the wave)
    const float* x = signal_of(x_rows, x10, ld10, b, n10) + f * ST_HOP;
    float acc = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lane + 64 * r;
        const float v = window_at(i) * x[i];
        acc = fmaf(v, v, acc);
    }
    const float s = wave_sum_dpp(acc);
    if (lane == 0) e[(long)b * Fmax + f] = 20.0f * log10f(sqrtf(s) + ST_EPS);
}

__global__ __launch_bounds__(256) void stoi_select_kernel(const int64_t* __restrict__ n_in, long max_n, int orig, int new_,
                                                          const float* __restrict__ e, int* __restrict__ src,
                                                          int* __restrict__ K, long Fmax) {
    __shared__ float red[4];
    __shared__ int cnt[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int F = frames_of(len10(n_in, b, max_n, orig, new_));
    const float* er = e + (long)b * Fmax;
    int* sr = src + (long)b * Fmax;
    // (fmaxf drops a NaN energy: such a frame is then never kept, and the row's d comes out of the frames that are)
    float mx = -INFINITY;
    for (int f = tid; f < F; f += 256) mx = fmaxf(mx, er[f]);
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) red[wv] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    int running = 0;
    for (int f0 = 0; f0 < F; f0 += 256) {
        const int f = f0 + tid;
        const bool keep = f < F && (mx - 40.0f - er[f]) < 0.0f;
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        __syncthreads();  // (cnt of the previous chunk has been read)
        if (lane == 0) cnt[wv] = __popcll(m);
        __syncthreads();
        int off = running;
        for (int w = 0; w < wv; ++w) off += cnt[w];
        if (keep) sr[off + before] = f;
        running += cnt[0] + cnt[1] + cnt[2] + cnt[3];
    }
    if (tid == 0) K[b] = running;
}

__global__ __launch_bounds__(ST_SPEC_THREADS) void stoi_spectra_kernel(const void* const* __restrict__ x_rows,
                                                                       const void* const* __restrict__ y_rows,
                                                                       const int64_t* __restrict__ n_in, long max_n, int orig,
                                                                       int new_, const float* __restrict__ x10,
                                                                       const float* __restrict__ y10, long ld10,
                                                                       const int* __restrict__ src, const int* __restrict__ K,
                                                                       float* __restrict__ Xt, float* __restrict__ Yt, long Fmax,
                                                                       long Mmax) {
    __shared__ float win[ST_FRAME];
    __shared__ float tw[ST_NFFT];            // cos(2 pi j / 512)
    __shared__ int srow[ST_TILE + 2];        // src of the compacted frames m0 - 1 .. m0 + 16 (-1: none)
    __shared__ float A[ST_TILE * ST_LDA];
    __shared__ float P[ST_TILE * ST_BINS];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m0 = blockIdx.x * ST_TILE;
    const long n10 = len10(n_in, b, max_n, orig, new_);
    const int F = frames_of(n10);
    int Kb = F > 0 ? K[b] : 0;
    Kb = Kb < 0 ? 0 : (Kb > F ? F : Kb);
    const int M = Kb - 1;
    if (m0 >= M) return;  // (uniform over the workgroup)
    const bool second = blockIdx.z != 0;
    const float* sig = signal_of(second ? y_rows : x_rows, second ? y10 : x10, ld10, b, n10);
    float* out = (second ? Yt : Xt) + (long)b * ST_J * Mmax;

    for (int i = tid; i < ST_FRAME; i += ST_SPEC_THREADS) win[i] = window_at(i);
    for (int j = tid; j < ST_NFFT; j += ST_SPEC_THREADS) tw[j] = (float)cospi((double)j / 256.0);
    if (tid < ST_TILE + 2) {
        const int c = m0 - 1 + tid;
        int s = -1;
        if (c >= 0 && c < Kb) {
            s = src[(long)b * Fmax + c];
            s = s < 0 ? 0 : (s >= F ? F - 1 : s);  // (a frame index always addresses inside the row)
        }
        srow[tid] = s;
    }
    __syncthreads();
    // A[r][i] = w[i] * xs[(m0 + r) 128 + i], xs the overlap-add of the kept windowed frames; rows behind M are zeros
    for (int idx = tid; idx < ST_TILE * ST_FRAME; idx += ST_SPEC_THREADS) {
        const int r = idx >> 8, i = idx & 255;
        float v = 0.0f;
        if (m0 + r < M) {
            v = win[i] * sig[(long)srow[r + 1] * ST_HOP + i];
            if (i < ST_HOP) {
                if (srow[r] >= 0) v += win[i + ST_HOP] * sig[(long)srow[r] * ST_HOP + i + ST_HOP];
            } else {
                v += win[i - ST_HOP] * sig[(long)srow[r + 2] * ST_HOP + i - ST_HOP];  // (m + 1 <= K - 1 always exists)
            }
            v *= win[i];
        }
        A[r * ST_LDA + i] = v;
    }
    __syncthreads();
    // D[frame][bin] += A[frame][n] * cos / sin(2 pi bin n / 512): v_mfma_f32_16x16x4_f32, lane l holds A[l & 15][k = l >> 4],
    // B[k = l >> 4][l & 15] and D[4 (l >> 4) + r][l & 15]
    const int col = lane & 15, kq = lane >> 4;
    // two accumulator sets, even and odd k-steps, added at the end: half the length of every rounding chain, and eight
    // independent MFMA chains in flight
    f32x4 re0[2], im0[2], re1[2], im1[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) re0[h] = im0[h] = re1[h] = im1[h] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int bin_a = ST_BIN0 + (2 * wv) * 16 + col, bin_b = bin_a + 16;
    const float* arow = A + col * ST_LDA + kq;
    for (int k0 = 0; k0 < ST_FRAME; k0 += 8) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = k0 + 4 * h + kq;
            const float a = arow[k0 + 4 * h];
            const int ia = (bin_a * n) & (ST_NFFT - 1), ib = (bin_b * n) & (ST_NFFT - 1);
            re0[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, tw[ia], re0[h], 0, 0, 0);
            im0[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, tw[(ia + 384) & (ST_NFFT - 1)], im0[h], 0, 0, 0);  // sin t = cos(t - pi / 2)
            re1[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, tw[ib], re1[h], 0, 0, 0);
            im1[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, tw[(ib + 384) & (ST_NFFT - 1)], im1[h], 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float* p = P + (4 * kq + r) * ST_BINS + (2 * wv) * 16 + col;
        const float ra = re0[0][r] + re0[1][r], ia = im0[0][r] + im0[1][r];
        const float rb = re1[0][r] + re1[1][r], ib = im1[0][r] + im1[1][r];
        p[0] = fmaf(ra, ra, ia * ia);
        p[16] = fmaf(rb, rb, ib * ib);
    }
    __syncthreads();
    if (tid < ST_J * ST_TILE) {
        const int j = tid >> 4, r = tid & 15;
        if (m0 + r < M) {
            float s = 0.0f;
            for (int k = c_edges[j]; k < c_edges[j + 1]; ++k) s += P[r * ST_BINS + k - ST_BIN0];
            out[(long)j * Mmax + m0 + r] = sqrtf(s);
        }
    }
}

__global__ __launch_bounds__(256) void stoi_segments_kernel(const int64_t* __restrict__ n_in, long max_n, int orig, int new_,
                                                            const int* __restrict__ K, const float* __restrict__ Xt,
                                                            const float* __restrict__ Yt, long Mmax, float* __restrict__ d,
                                                            int* __restrict__ segs) {
    __shared__ float red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int F = frames_of(len10(n_in, b, max_n, orig, new_));
    int Kb = F > 0 ? K[b] : 0;
    Kb = Kb < 0 ? 0 : (Kb > F ? F : Kb);
    const int M = Kb - 1;
    if (M < ST_N) {  // (uniform over the workgroup)
        if (tid == 0) {
            d[b] = SWC_STOI_SHORT;
            segs[b] = 0;
        }
        return;
    }
    const int S = M - ST_N + 1;
    const float* X = Xt + (long)b * ST_J * Mmax;
    const float* Y = Yt + (long)b * ST_J * Mmax;
    float part = 0.0f;
    for (long item = tid; item < (long)ST_J * S; item += 256) {
        const int j = (int)(item / S), s = (int)(item - (long)j * S);
        const float* xa = X + (long)j * Mmax + s;
        const float* ya = Y + (long)j * Mmax + s;
        float a[ST_N], c[ST_N];
        float na = 0.0f, nc = 0.0f;
#pragma unroll
        for (int i = 0; i < ST_N; ++i) {
            a[i] = xa[i];
            c[i] = ya[i];
            na = fmaf(a[i], a[i], na);
            nc = fmaf(c[i], c[i], nc);
        }
        const float scale = sqrtf(na) / (sqrtf(nc) + ST_EPS);
        float ma = 0.0f, mc = 0.0f;
#pragma unroll
        for (int i = 0; i < ST_N; ++i) {
            c[i] = fminf(c[i] * scale, a[i] * ST_CLIP);
            ma += a[i];
            mc += c[i];
        }
        ma *= 1.0f / ST_N;
        mc *= 1.0f / ST_N;
        na = 0.0f;
        nc = 0.0f;
#pragma unroll
        for (int i = 0; i < ST_N; ++i) {
            a[i] -= ma;
            c[i] -= mc;
            na = fmaf(a[i], a[i], na);
            nc = fmaf(c[i], c[i], nc);
        }
        const float ia = 1.0f / (sqrtf(na) + ST_EPS), ic = 1.0f / (sqrtf(nc) + ST_EPS);
        float rho = 0.0f;
#pragma unroll
        for (int i = 0; i < ST_N; ++i) rho = fmaf(a[i] * ia, c[i] * ic, rho);
        part += rho;
    }
    red[tid] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        d[b] = red[0] / (float)((long)ST_J * S);
        segs[b] = S;
    }
}

// M of row b (STFT frames after the silent ones are gone), from what the selection kernel left: clamped into the row
__device__ __forceinline__ int stft_frames_of(const int64_t* n_in, int b, long max_n, int orig, int new_, const int* K) {
    const int F = frames_of(len10(n_in, b, max_n, orig, new_));
    int Kb = F > 0 ? K[b] : 0;
    Kb = Kb < 0 ? 0 : (Kb > F ? F : Kb);
    return Kb - 1;
}

__global__ __launch_bounds__(64 * ES_GROUP) void estoi_segments_kernel(const int64_t* __restrict__ n_in, long max_n, int orig,
                                                                       int new_, const int* __restrict__ K,
                                                                       const float* __restrict__ Xt, const float* __restrict__ Yt,
                                                                       long Mmax, float* __restrict__ eseg, long Smax) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const long s = (long)blockIdx.x * ES_GROUP + (threadIdx.x >> 6);
    const int M = stft_frames_of(n_in, b, max_n, orig, new_, K);
    if (M < ST_N || s >= M - ST_N + 1) return;  // (uniform over the wave; nothing below waits for another wave)
    const bool on = lane < ST_N;
    // frame s + lane <= S - 1 + 29 = M - 1 < Mmax; the lanes behind the segment read frame s and hold zeros
    const float* X = Xt + (long)b * ST_J * Mmax + s + (on ? lane : 0);
    const float* Y = Yt + (long)b * ST_J * Mmax + s + (on ? lane : 0);
    float a[ST_J], c[ST_J];
#pragma unroll
    for (int j = 0; j < ST_J; ++j) {
        const float xv = X[(long)j * Mmax], yv = Y[(long)j * Mmax];
        a[j] = on ? xv : 0.0f;
        c[j] = on ? yv : 0.0f;
    }
    // 4a: every band row minus its mean over the 30 frames, over its norm + EPS
#pragma unroll
    for (int j = 0; j < ST_J; ++j) {
        const float ma = wave_sum_dpp(a[j]) * (1.0f / ST_N), mc = wave_sum_dpp(c[j]) * (1.0f / ST_N);
        a[j] = on ? a[j] - ma : 0.0f;
        c[j] = on ? c[j] - mc : 0.0f;
        const float ia = 1.0f / (sqrtf(wave_sum_dpp(a[j] * a[j])) + ST_EPS);
        const float ic = 1.0f / (sqrtf(wave_sum_dpp(c[j] * c[j])) + ST_EPS);
        a[j] *= ia;
        c[j] *= ic;
    }
    // 4b: every frame column minus its mean over the 15 bands, over its norm + EPS (a lane of zeros stays zeros)
    float ma = 0.0f, mc = 0.0f;
#pragma unroll
    for (int j = 0; j < ST_J; ++j) {
        ma += a[j];
        mc += c[j];
    }
    ma *= 1.0f / ST_J;
    mc *= 1.0f / ST_J;
    float na = 0.0f, nc = 0.0f;
#pragma unroll
    for (int j = 0; j < ST_J; ++j) {
        a[j] -= ma;
        c[j] -= mc;
        na = fmaf(a[j], a[j], na);
        nc = fmaf(c[j], c[j], nc);
    }
    const float ia = 1.0f / (sqrtf(na) + ST_EPS), ic = 1.0f / (sqrtf(nc) + ST_EPS);
    // 4c
    float p = 0.0f;
#pragma unroll
    for (int j = 0; j < ST_J; ++j) p = fmaf(a[j] * ia, c[j] * ic, p);
    const float e = wave_sum_dpp(p) * (1.0f / ST_N);
    if (lane == 0) eseg[(long)b * Smax + s] = e;
}

// estoi[b] = sum of eseg[b][0..S) / S in an order fixed by S; segs[b] too when `segs` is given (the STOI kernel did not run)
__global__ __launch_bounds__(256) void estoi_mean_kernel(const int64_t* __restrict__ n_in, long max_n, int orig, int new_,
                                                         const int* __restrict__ K, const float* __restrict__ eseg, long Smax,
                                                         float* __restrict__ estoi, int* __restrict__ segs) {
    __shared__ float red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int M = stft_frames_of(n_in, b, max_n, orig, new_, K);
    if (M < ST_N) {  // (uniform over the workgroup)
        if (tid == 0) {
            estoi[b] = SWC_STOI_SHORT;
            if (segs != nullptr) segs[b] = 0;
        }
        return;
    }
    const int S = M - ST_N + 1;
    const float* er = eseg + (long)b * Smax;
    float part = 0.0f;
    for (int s = tid; s < S; s += 256) part += er[s];
    red[tid] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        estoi[b] = red[0] / (float)S;
        if (segs != nullptr) segs[b] = S;
    }
}

// PASS 1: record = sum x, sum y, sum x x, sum x y.  PASS 2: record = sum (alpha x')^2, sum (y' - alpha x')^2, 0, 0.
// Thread t owns the samples 4 (256 g + t) .. + 3 of the chunk, g = 0 .. SD_GROUPS - 1, and adds them in ascending order
template <int PASS>
__global__ __launch_bounds__(SD_THREADS) void sisdr_sums_kernel(const void* const* __restrict__ x_rows,
                                                                const void* const* __restrict__ y_rows,
                                                                const int64_t* __restrict__ n_in, long max_n,
                                                                const double* __restrict__ stat, double* __restrict__ rec,
                                                                long chunks) {
    __shared__ double red[SD_THREADS / 64][4];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long n = clamp_len(n_in, b, max_n), c0 = (long)blockIdx.x * SD_CHUNK;
    if (c0 >= n) return;  // (uniform over the workgroup; also every chunk of an empty row, whose addresses are not read)
    const float* x = reinterpret_cast<const float*>(x_rows[b]) + c0;
    const float* y = reinterpret_cast<const float*>(y_rows[b]) + c0;
    const long left = n - c0;
    const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0;
    float xv[SD_GROUPS][4], yv[SD_GROUPS][4];
#pragma unroll
    for (int g = 0; g < SD_GROUPS; ++g) {
        const long i = ((long)g * SD_THREADS + tid) * 4;
        if (vec && i + 4 <= left) {
            const float4 vx = *reinterpret_cast<const float4*>(x + i), vy = *reinterpret_cast<const float4*>(y + i);
            xv[g][0] = vx.x; xv[g][1] = vx.y; xv[g][2] = vx.z; xv[g][3] = vx.w;
            yv[g][0] = vy.x; yv[g][1] = vy.y; yv[g][2] = vy.z; yv[g][3] = vy.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = i + k < left;
                xv[g][k] = in ? x[i + k] : 0.0f;
                yv[g][k] = in ? y[i + k] : 0.0f;
            }
        }
    }
    double mx = 0.0, my = 0.0, al = 0.0;
    if (PASS == 2) {
        mx = stat[(long)b * 4 + 0];
        my = stat[(long)b * 4 + 1];
        al = stat[(long)b * 4 + 2];
    }
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int g = 0; g < SD_GROUPS; ++g) {
        const long i = ((long)g * SD_THREADS + tid) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i + k < left) {
                const double dx = (double)xv[g][k], dy = (double)yv[g][k];
                if (PASS == 1) {
                    s0 += dx;
                    s1 += dy;
                    s2 = fma(dx, dx, s2);
                    s3 = fma(dx, dy, s3);
                } else {
                    const double t = al * (dx - mx);
                    const double e = (dy - my) - t;
                    s0 = fma(t, t, s0);
                    s1 = fma(e, e, s1);
                }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o);
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
        s3 += __shfl_xor(s3, o);
    }
    if (lane == 0) {
        red[wv][0] = s0;
        red[wv][1] = s1;
        red[wv][2] = s2;
        red[wv][3] = s3;
    }
    __syncthreads();
    if (tid < 4) rec[((long)b * chunks + blockIdx.x) * 4 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// the records of row b in ascending chunk order (64 at a time through LDS: the loads in parallel, the adds in order);
// PASS 1 -> stat[b] = mx, my, alpha;  PASS 2 -> out[b] = 10 log10((Et + EPS) / (En + EPS)), NaN for an empty row
template <int PASS>
__global__ __launch_bounds__(64) void sisdr_finish_kernel(const int64_t* __restrict__ n_in, long max_n,
                                                          const double* __restrict__ rec, long chunks, double* __restrict__ stat,
                                                          float* __restrict__ out) {
    __shared__ double tile[64][4];
    __shared__ double tot[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long n = clamp_len(n_in, b, max_n);
    const long C = (n + SD_CHUNK - 1) / SD_CHUNK;  // <= chunks: the chunks of this row that were written
    const double* r = rec + (long)b * chunks * 4;
    double acc = 0.0;
    for (long t0 = 0; t0 < C; t0 += 64) {
        const long c = t0 + tid;
        if (c < C) {
#pragma unroll
            for (int k = 0; k < 4; ++k) tile[tid][k] = r[c * 4 + k];
        }
        __syncthreads();
        if (tid < 4) {
            const int m = (int)(C - t0 < 64 ? C - t0 : 64);
            for (int i = 0; i < m; ++i) acc += tile[i][tid];
        }
        __syncthreads();
    }
    if (tid < 4) tot[tid] = acc;
    __syncthreads();
    if (tid != 0) return;
    if (PASS == 1) {
        double mx = 0.0, my = 0.0, al = 0.0;
        if (n > 0) {
            mx = tot[0] / (double)n;
            my = tot[1] / (double)n;
            const double sxx = fma(-tot[0], mx, tot[2]), sxy = fma(-tot[0], my, tot[3]);  // sum x' x', sum x' y'
            al = sxy / (sxx + SD_EPS);
        }
        stat[(long)b * 4 + 0] = mx;
        stat[(long)b * 4 + 1] = my;
        stat[(long)b * 4 + 2] = al;
        stat[(long)b * 4 + 3] = 0.0;
    } else {
        out[b] = n > 0 ? (float)(10.0 * log10((tot[0] + SD_EPS) / (tot[1] + SD_EPS))) : __builtin_nanf("");
    }
}

}  // namespace

extern "C" int64_t swc_stoi_workspace_bytes(int32_t B, int64_t max_n_in, int32_t orig, int32_t new_) {
    if (B < 0 || B > 65535 || max_n_in < 0 || orig < 1 || new_ < 1) return -1;
    if (max_n_in > (1L << 40) / new_) return -1;
    return (int64_t)layout(B, max_n_in, orig, new_).total;
}

// resample -> energies -> selection -> band spectra on the layout L; `who` names the entry point in a launch error.
// swc_resample checks the table and the LDS limit before it launches anything (with B == 0 or no samples it only checks)
static int front_end(const Layout& L, char* ws, const void* const* x_rows, const void* const* y_rows, const int64_t* n_in,
                     int64_t max_n_in, int32_t orig, int32_t new_, int32_t width, const float* taps_packed,
                     const int32_t* tap_start, int32_t run, int32_t B, hipStream_t st, const char* who) {
    char label[64];
    float* x10 = nullptr;
    float* y10 = nullptr;
    if (orig != new_) {
        x10 = reinterpret_cast<float*>(ws + L.x10);
        y10 = reinterpret_cast<float*>(ws + L.y10);
        int rc = swc_resample(x_rows, n_in, SWC_PCM_F32, 1, orig, new_, width, taps_packed, tap_start, run, x10, L.ld10, L.n10max,
                              B, st);
        if (rc != SWC_OK) return rc;
        rc = swc_resample(y_rows, n_in, SWC_PCM_F32, 1, orig, new_, width, taps_packed, tap_start, run, y10, L.ld10, L.n10max, B,
                          st);
        if (rc != SWC_OK) return rc;
    }
    if (B == 0) return SWC_OK;
    float* e = reinterpret_cast<float*>(ws + L.e);
    int* src = reinterpret_cast<int*>(ws + L.src);
    int* K = reinterpret_cast<int*>(ws + L.K);
    float* Xt = reinterpret_cast<float*>(ws + L.Xt);
    float* Yt = reinterpret_cast<float*>(ws + L.Yt);
    const long max_n = max_n_in;
    if (L.Fmax > 0) {
        hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)((L.Fmax + 3) / 4), (unsigned)B), dim3(256), 0, st, x_rows, n_in, max_n,
                           (int)orig, (int)new_, (const float*)x10, L.ld10, e, L.Fmax);
        snprintf(label, sizeof label, "%s (energies)", who);
        SWC_CHECK_LAUNCH(label);
    }
    hipLaunchKernelGGL(stoi_select_kernel, dim3((unsigned)B), dim3(256), 0, st, n_in, max_n, (int)orig, (int)new_, (const float*)e, src,
                       K, L.Fmax);
    snprintf(label, sizeof label, "%s (frame selection)", who);
    SWC_CHECK_LAUNCH(label);
    if (L.Mmax > 0) {
        hipLaunchKernelGGL(stoi_spectra_kernel, dim3((unsigned)((L.Mmax + ST_TILE - 1) / ST_TILE), (unsigned)B, 2u),
                           dim3(ST_SPEC_THREADS), 0, st, x_rows, y_rows, n_in, max_n, (int)orig, (int)new_, (const float*)x10,
                           (const float*)y10, L.ld10, (const int*)src, (const int*)K, Xt, Yt, L.Fmax, L.Mmax);
        snprintf(label, sizeof label, "%s (band spectra)", who);
        SWC_CHECK_LAUNCH(label);
    }
    return SWC_OK;
}

extern "C" int swc_stoi(const void* const* x_rows, const void* const* y_rows, const int64_t* n_in, int64_t max_n_in,
                        int32_t orig, int32_t new_, int32_t width, const float* taps_packed, const int32_t* tap_start,
                        int32_t run, float* d, int32_t* segs, void* workspace, int64_t workspace_bytes, int32_t B,
                        void* stream) {
    SWC_CHECK_ARG(x_rows && y_rows && n_in && taps_packed && tap_start && d && segs && workspace, "swc_stoi: null pointer");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_stoi: B=%d (0..65535)", B);
    SWC_CHECK_ARG(orig >= 1 && new_ >= 1, "swc_stoi: rates must be >= 1 (orig=%d new=%d)", orig, new_);
    SWC_CHECK_ARG(max_n_in >= 0 && max_n_in <= (1L << 40) / new_, "swc_stoi: max_n_in=%ld out of range", (long)max_n_in);
    const Layout L = layout(B, max_n_in, orig, new_);
    SWC_CHECK_ARG(L.n10max < 0x7fffff00L, "swc_stoi: max_n_in=%ld is 2^31 samples or more at 10 kHz", (long)max_n_in);
    SWC_CHECK_ARG(workspace_bytes >= (int64_t)L.total, "swc_stoi: workspace of %ld bytes, %ld needed (swc_stoi_workspace_bytes)",
                  (long)workspace_bytes, (long)L.total);
    SWC_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "swc_stoi: workspace must be 256-byte aligned");
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const int rc = front_end(L, ws, x_rows, y_rows, n_in, max_n_in, orig, new_, width, taps_packed, tap_start, run, B, st, "swc_stoi");
    if (rc != SWC_OK || B == 0) return rc;
    hipLaunchKernelGGL(stoi_segments_kernel, dim3((unsigned)B), dim3(256), 0, st, n_in, (long)max_n_in, (int)orig, (int)new_,
                       (const int*)(ws + L.K), (const float*)(ws + L.Xt), (const float*)(ws + L.Yt), L.Mmax, d, segs);
    SWC_CHECK_LAUNCH("swc_stoi (segments)");
    return SWC_OK;
}

extern "C" int64_t swc_quality_workspace_bytes(int32_t B, int64_t max_n_in, int32_t orig, int32_t new_) {
    if (B < 0 || B > 65535 || max_n_in < 0 || orig < 1 || new_ < 1) return -1;
    if (max_n_in > (1L << 40) / new_) return -1;
    return (int64_t)qlayout(B, max_n_in, orig, new_).total;
}

extern "C" int swc_quality(const void* const* x_rows, const void* const* y_rows, const int64_t* n_in, int64_t max_n_in,
                           int32_t orig, int32_t new_, int32_t width, const float* taps_packed, const int32_t* tap_start,
                           int32_t run, float* stoi, float* estoi, int32_t* segs, float* si_sdr, void* workspace,
                           int64_t workspace_bytes, int32_t B, void* stream) {
    const bool front = stoi != nullptr || estoi != nullptr;
    SWC_CHECK_ARG(x_rows && y_rows && n_in && workspace, "swc_quality: null pointer");
    SWC_CHECK_ARG(front || si_sdr != nullptr, "swc_quality: no output (stoi, estoi and si_sdr are all null)");
    SWC_CHECK_ARG(!front || (taps_packed && tap_start), "swc_quality: null pointer (stoi and estoi need the 10 kHz table)");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_quality: B=%d (0..65535)", B);
    SWC_CHECK_ARG(orig >= 1 && new_ >= 1, "swc_quality: rates must be >= 1 (orig=%d new=%d)", orig, new_);
    SWC_CHECK_ARG(max_n_in >= 0 && max_n_in <= (1L << 40) / new_, "swc_quality: max_n_in=%ld out of range", (long)max_n_in);
    const QLayout Q = qlayout(B, max_n_in, orig, new_);
    const Layout& L = Q.st;
    SWC_CHECK_ARG(!front || L.n10max < 0x7fffff00L, "swc_quality: max_n_in=%ld is 2^31 samples or more at 10 kHz", (long)max_n_in);
    SWC_CHECK_ARG(workspace_bytes >= (int64_t)Q.total,
                  "swc_quality: workspace of %ld bytes, %ld needed (swc_quality_workspace_bytes)", (long)workspace_bytes, (long)Q.total);
    SWC_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "swc_quality: workspace must be 256-byte aligned");
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const long max_n = max_n_in;
    if (front) {
        const int rc = front_end(L, ws, x_rows, y_rows, n_in, max_n_in, orig, new_, width, taps_packed, tap_start, run, B, st,
                                 "swc_quality");
        if (rc != SWC_OK) return rc;
    }
    if (B == 0) return SWC_OK;
    const int* K = reinterpret_cast<const int*>(ws + L.K);
    const float* Xt = reinterpret_cast<const float*>(ws + L.Xt);
    const float* Yt = reinterpret_cast<const float*>(ws + L.Yt);
    if (stoi != nullptr) {
        int* s = segs != nullptr ? segs : reinterpret_cast<int*>(ws + Q.segs);
        hipLaunchKernelGGL(stoi_segments_kernel, dim3((unsigned)B), dim3(256), 0, st, n_in, max_n, (int)orig, (int)new_, K, Xt, Yt,
                           L.Mmax, stoi, s);
        SWC_CHECK_LAUNCH("swc_quality (STOI segments)");
    }
    if (estoi != nullptr) {
        float* eseg = reinterpret_cast<float*>(ws + Q.eseg);
        if (Q.Smax > 0) {
            hipLaunchKernelGGL(estoi_segments_kernel, dim3((unsigned)((Q.Smax + ES_GROUP - 1) / ES_GROUP), (unsigned)B),
                               dim3(64 * ES_GROUP), 0, st, n_in, max_n, (int)orig, (int)new_, K, Xt, Yt, L.Mmax, eseg, Q.Smax);
            SWC_CHECK_LAUNCH("swc_quality (ESTOI segments)");
        }
        hipLaunchKernelGGL(estoi_mean_kernel, dim3((unsigned)B), dim3(256), 0, st, n_in, max_n, (int)orig, (int)new_, K,
                           (const float*)eseg, Q.Smax, estoi, stoi != nullptr ? (int*)nullptr : segs);
        SWC_CHECK_LAUNCH("swc_quality (ESTOI mean)");
    }
    if (si_sdr != nullptr) {
        double* rec = reinterpret_cast<double*>(ws + Q.rec);
        double* stat = reinterpret_cast<double*>(ws + Q.stat);
        const dim3 grid((unsigned)Q.chunks, (unsigned)B);
        if (Q.chunks > 0) {
            hipLaunchKernelGGL(sisdr_sums_kernel<1>, grid, dim3(SD_THREADS), 0, st, x_rows, y_rows, n_in, max_n, (const double*)stat,
                               rec, Q.chunks);
            SWC_CHECK_LAUNCH("swc_quality (SI-SDR pass 1)");
        }
        hipLaunchKernelGGL(sisdr_finish_kernel<1>, dim3((unsigned)B), dim3(64), 0, st, n_in, max_n, (const double*)rec, Q.chunks, stat,
                           si_sdr);
        SWC_CHECK_LAUNCH("swc_quality (SI-SDR means)");
        if (Q.chunks > 0) {
            hipLaunchKernelGGL(sisdr_sums_kernel<2>, grid, dim3(SD_THREADS), 0, st, x_rows, y_rows, n_in, max_n, (const double*)stat,
                               rec, Q.chunks);
            SWC_CHECK_LAUNCH("swc_quality (SI-SDR pass 2)");
        }
        hipLaunchKernelGGL(sisdr_finish_kernel<2>, dim3((unsigned)B), dim3(64), 0, st, n_in, max_n, (const double*)rec, Q.chunks, stat,
                           si_sdr);
        SWC_CHECK_LAUNCH("swc_quality (SI-SDR result)");
    }
    return SWC_OK;
}
