// swc_stretch (include/swc_stretch.h): WSOLA time stretch of a ragged batch with a least-squares search in exact integer
// arithmetic.  After one memset of the peaks, four kinds of launch; no workgroup waits for another:
//   stretch_peak_kernel   max |x| of every row as an unsigned maximum over the bit patterns of |x| (the pattern of
//                         align_peak_kernel, one side): one workgroup per 4096 samples, one atomic per workgroup.
//   stretch_window_kernel the W window values, float64 cospi rounded to f32 once, into the workspace.
//   stretch_track_kernel  grid (B): one workgroup of 256 threads per row, serial over the frames (frame m needs s_{m-1}).  Per
//                         frame it holds in LDS, as int16 quantised from f32 on the way in, the span Q(a_m - D .. a_m + D + W)
//                         at both pair alignments (ev[k] = (S[2k], S[2k+1]) is the raw span itself, od[k] = (S[2k+1], S[2k+2]))
//                         and the target Q(p .. p + W) as pairs split into a high and a low digit (q = 256 h + l, |h|, |l| <=
//                         128).  Dm(d) = E_target + E_candidate(d) - 2 c(d):
//                           c            work items (lag, segment of 64 samples of the window), item = segment * lags + lag, dealt
//                                        round-robin to the 256 lanes: 32 packed 16-bit dot products per digit into an int32 (a
//                                        digit's pair of products stays below 2^23, so 32 pairs stay below 2^28), then one
//                                        int64 LDS atomic add of 256 ch + cl per item.  Lanes of a wave mostly share the
//                                        segment: the target's 16-byte blocks are broadcasts.
//                           E_candidate  differences of a running (prefix) sum over the span's pair energies: a scan by wave
//                                        shuffles, the four waves' totals through LDS.
//                           E_target     a plain sum while the target is staged.
//                         The choice is ONE unsigned 64-bit minimum over (Dm << 12) | key with key = 2 |d| + (d < 0): Dm < 2^43
//                         and key < 2^12, so the order of the pairs (Dm, key) is the order of the words, and any reduction
//                         order gives the same d.  While the items run, the next frame's span (it depends on m alone, not on
//                         s_m) is already on its way from global memory into registers; only the target's load waits for
//                         the choice.  The kernel is latency-bound by construction: B workgroups, J serial steps each.
//   stretch_synth_kernel  grid (blocks of SWC_STRETCH_CHUNK output samples, B): the two windowed reads per sample from the
//                         positions in the workspace, written under the output contract.
// Everything up to the window and the one fmaf per sample is integer arithmetic: any order gives the same bits.  The file is
// built with -ffp-contract=off: the output expression states its own fma and nothing else may contract.
// Every store to global memory is an ordinary vector store from plain C++ or an integer atomic.
#include "swc_metric_common.h"
#include "swc_stretch.h"

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_WAVES = ST_THREADS / 64;
constexpr int ST_SPAN = 2 * SWC_STRETCH_MAX_D + SWC_STRETCH_MAX_W;  // samples of the longest span
constexpr int ST_PER = ST_SPAN / ST_THREADS;                        // ... per thread
constexpr int ST_LAGS = 2 * SWC_STRETCH_MAX_D + 1;
constexpr int ST_SEG = 8;              // blocks of four target pairs per work item: 64 samples
constexpr int ST_KEY_BITS = 12;
constexpr int PK_CHUNK = 4096;         // samples per workgroup of the peak kernel
constexpr int SY_CHUNK = SWC_STRETCH_CHUNK;
constexpr int SY_PER = SY_CHUNK / ST_THREADS;
static_assert(ST_SPAN % ST_THREADS == 0 && ST_SPAN % 2 == 0, "whole samples per thread, whole pairs");
static_assert(ST_SEG * 4 * 2 * 128 * 32767LL < (1LL << 31), "a digit's dot products of one item fit int32");
static_assert(2 * SWC_STRETCH_MAX_D + 1 < (1 << ST_KEY_BITS), "the tie key fits its bits");
static_assert((long long)SWC_STRETCH_MAX_W * 65534LL * 65534LL < (1LL << (63 - ST_KEY_BITS)), "Dm << 12 fits 63 bits");
static_assert(SWC_STRETCH_MIN_W % 8 == 0 && SWC_STRETCH_MAX_W % 8 == 0, "whole blocks of four pairs");

inline int64_t out_len(int64_t n, int num, int den) { return (n * den + num - 1) / num; }
inline int64_t frames_of(int64_t n_out, int Hs) { return (n_out + Hs - 1) / Hs; }

bool speed_ok(int num, int den) {
    return num >= 1 && num <= SWC_STRETCH_MAX_TERM && den >= 1 && den <= SWC_STRETCH_MAX_TERM &&
           (int64_t)num <= (int64_t)SWC_STRETCH_MAX_RATIO * den && (int64_t)den <= (int64_t)SWC_STRETCH_MAX_RATIO * num;
}
bool window_ok(int W) { return W >= SWC_STRETCH_MIN_W && W <= SWC_STRETCH_MAX_W && W % 8 == 0; }

// grid (chunks, B)
__global__ __launch_bounds__(ST_THREADS) void stretch_peak_kernel(const void* const* __restrict__ x_rows, const int64_t* __restrict__ n,
                                                                  long max_n, unsigned* __restrict__ peaks) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const long nb = clamp_len(n, b, max_n);
    const long i0 = (long)blockIdx.x * PK_CHUNK;
    if (i0 >= nb) return;  // an empty row: its address is not read
    const unsigned* p = reinterpret_cast<const unsigned*>(x_rows[b]);
    const long i1 = i0 + PK_CHUNK < nb ? i0 + PK_CHUNK : nb;
    unsigned m = 0;
#pragma unroll 4
    for (long i = i0 + tid; i < i1; i += ST_THREADS) {
        const unsigned v = p[i] & 0x7fffffffu;
        m = v > m ? v : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned v = (unsigned)__shfl_xor((int)m, o);
        m = v > m ? v : m;
    }
    // one atomic per workgroup: the atomics of a row all meet at one address
    __shared__ unsigned wm[ST_WAVES];
    if ((tid & 63) == 0) wm[tid >> 6] = m;
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < ST_WAVES; ++w) m = wm[w] > m ? wm[w] : m;
    if (m != 0) atomicMax(peaks + b, m);
}

__global__ __launch_bounds__(ST_THREADS) void stretch_window_kernel(float* __restrict__ win, int W) {
    const int k = blockIdx.x * ST_THREADS + threadIdx.x;
    if (k < W) win[k] = (float)(0.5 - 0.5 * cospi(2.0 * (double)k / (double)W));
}

// grid (B)
__global__ __launch_bounds__(ST_THREADS) void stretch_track_kernel(const void* const* __restrict__ x_rows, const int64_t* __restrict__ n,
                                                                   long max_n, int W, int D, int num, int den,
                                                                   const unsigned* __restrict__ peaks, int* __restrict__ posw, long Jmax,
                                                                   int32_t* __restrict__ pos, int64_t* __restrict__ dist, long ldm,
                                                                   int32_t* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) short raw[ST_SPAN];              // the span S; as dwords: the even pair view
    __shared__ __attribute__((aligned(16))) unsigned od[ST_SPAN / 2];        // the odd pair view
    __shared__ __attribute__((aligned(16))) unsigned th[SWC_STRETCH_MAX_W / 2];  // target pairs, high digits
    __shared__ __attribute__((aligned(16))) unsigned tl[SWC_STRETCH_MAX_W / 2];  // target pairs, low digits
    __shared__ long long P2[ST_SPAN / 2 + 1];                                // P2[k] = sum of S[i]^2 over i < 2 k
    __shared__ long long red[ST_LAGS];                                       // c per lag
    __shared__ long long wtot[ST_WAVES], wet[ST_WAVES];
    __shared__ unsigned long long wmin[ST_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long nb = clamp_len(n, b, max_n);
    const int Hs = W / 2;
    const long n_out = (nb * den + num - 1) / num;
    const long J = (n_out + Hs - 1) / Hs;
    const unsigned pk = nb > 0 ? peaks[b] : 0u;
    const bool defined = peak_defined(pk);
    int* pw = posw + (long)b * Jmax;
    int32_t* prow = pos ? pos + (long)b * ldm : nullptr;
    int64_t* drow = dist ? dist + (long)b * ldm : nullptr;
    if (flags != nullptr && tid == 0) flags[b] = defined ? 0 : SWC_STRETCH_UNDEFINED;
    // frame 0 and everything behind the row's frames (every frame of a row that is not defined): zeros
    for (long m = (defined && J > 0 ? J : 0) + tid; m < Jmax; m += ST_THREADS) {
        pw[m] = 0;
        if (prow) prow[m] = 0;
        if (drow) drow[m] = 0;
    }
    if (!defined || J == 0) return;  // uniform over the workgroup, like the return below
    if (tid == 0) {
        pw[0] = 0;
        if (prow) prow[0] = 0;
        if (drow) drow[0] = 0;
    }
    if (J == 1) return;

    const int e = peak_exp(pk);
    const float* x = reinterpret_cast<const float*>(x_rows[b]);  // nb > 0 here
    const int span = 2 * D + W, nl = 2 * D + 1, npairs = span / 2;
    const int blocks = W / 8, nseg = (blocks + ST_SEG - 1) / ST_SEG, nitems = nl * nseg;
    const int cp = (npairs + ST_THREADS - 1) / ST_THREADS;  // pairs of the span per thread of the scan (<= 8)
    const unsigned* ev = reinterpret_cast<const unsigned*>(raw);
    const uint4* th4 = reinterpret_cast<const uint4*>(th);
    const uint4* tl4 = reinterpret_cast<const uint4*>(tl);

    for (int k = tid; k < nl; k += ST_THREADS) red[k] = 0;
    float pf[ST_PER];  // the span on its way in
    {
        const long a1 = ((long)Hs * num) / den - D;
#pragma unroll
        for (int i = 0; i < ST_PER; ++i) {
            const int k = i * ST_THREADS + tid;
            const long g = a1 + k;
            if (k < span) raw[k] = (short)((g >= 0 && g < nb) ? quantise(x[g], e) : 0);
        }
    }
    __syncthreads();

    long s_prev = 0;
#pragma unroll 1
    for (long m = 1; m < J; ++m) {
        const long a_m = (m * Hs * num) / den;
        // ---- the odd view, the scan's partial sums, the target ----
        for (int k = tid; k < npairs - 1; k += ST_THREADS) od[k] = pack16(raw[2 * k + 1], raw[2 * k + 2]);
        long long loc = 0;
        for (int i = 0; i < cp; ++i) {
            const int k = tid * cp + i;
            if (k < npairs) {
                const long long q0 = raw[2 * k], q1 = raw[2 * k + 1];
                loc += q0 * q0 + q1 * q1;
            }
        }
        long long inc = loc;  // inclusive over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wtot[wave] = inc;
        const long p = s_prev + Hs;
        long long et = 0;
        for (int k = tid; k < Hs; k += ST_THREADS) {
            const long g = p + 2 * k;
            const int q0 = (g >= 0 && g < nb) ? quantise(x[g], e) : 0;
            const int q1 = (g + 1 >= 0 && g + 1 < nb) ? quantise(x[g + 1], e) : 0;
            const int h0 = (q0 + 128) >> 8, h1 = (q1 + 128) >> 8;
            th[k] = pack16(h0, h1);
            tl[k] = pack16(q0 - 256 * h0, q1 - 256 * h1);
            et += (long long)(q0 * q0) + (long long)(q1 * q1);
        }
        et = wave_sum_i64(et);
        if (lane == 0) wet[wave] = et;
        __syncthreads();
        long long Et = 0, run = inc - loc;
#pragma unroll
        for (int w = 0; w < ST_WAVES; ++w) {
            Et += wet[w];
            if (w < wave) run += wtot[w];
        }
        if (tid == 0) P2[0] = 0;
        for (int i = 0; i < cp; ++i) {
            const int k = tid * cp + i;
            if (k < npairs) {
                const long long q0 = raw[2 * k], q1 = raw[2 * k + 1];
                run += q0 * q0 + q1 * q1;
                P2[k + 1] = run;
            }
        }
        // ---- the next frame's span sets out (it does not depend on this frame's choice) ----
        const bool more = m + 1 < J;
        if (more) {
            const long a1 = ((m + 1) * Hs * num) / den - D;
#pragma unroll
            for (int i = 0; i < ST_PER; ++i) {
                const int k = i * ST_THREADS + tid;
                const long g = a1 + k;
                pf[i] = (k < span && g >= 0 && g < nb) ? x[g] : 0.0f;
            }
        }
        // ---- c: the items ----
#pragma unroll 1
        for (int item = tid; item < nitems; item += ST_THREADS) {
            const int seg = item / nl, o = item - seg * nl;
            const int blk0 = seg * ST_SEG, blk1 = blk0 + ST_SEG < blocks ? blk0 + ST_SEG : blocks;
            const unsigned* v = (o & 1) ? od : ev;
            int base = (o >> 1) + 4 * blk0;  // base + 3 <= (o >> 1) + W / 2 - 1: inside the view (npairs, or npairs - 1 of od)
            int ch = 0, cl = 0;
            for (int blk = blk0; blk < blk1; ++blk, base += 4) {
                const uint4 h = th4[blk], l = tl4[blk];
                const unsigned s0 = v[base], s1 = v[base + 1], s2 = v[base + 2], s3 = v[base + 3];
                ch = dot2(h.x, s0, ch);
                cl = dot2(l.x, s0, cl);
                ch = dot2(h.y, s1, ch);
                cl = dot2(l.y, s1, cl);
                ch = dot2(h.z, s2, ch);
                cl = dot2(l.z, s2, cl);
                ch = dot2(h.w, s3, ch);
                cl = dot2(l.w, s3, cl);
            }
            atomicAdd(reinterpret_cast<unsigned long long*>(red + o), (unsigned long long)(256LL * ch + cl));  // two's complement: exact
        }
        __syncthreads();
        // ---- the choice ----
        unsigned long long best = ~0ull;
        for (int o = tid; o < nl; o += ST_THREADS) {
            const long long c = red[o];
            red[o] = 0;  // for the next frame
            const int oe = o & ~1;
            long long Ec = P2[(oe + W) >> 1] - P2[oe >> 1];
            if (o & 1) {
                const long long q0 = raw[o - 1], q1 = raw[o - 1 + W];
                Ec += q1 * q1 - q0 * q0;
            }
            const long long Dm = Et + Ec - 2 * c;
            const int d = o - D;
            const unsigned key = d < 0 ? (unsigned)(-2 * d + 1) : (unsigned)(2 * d);
            const unsigned long long word = ((unsigned long long)Dm << ST_KEY_BITS) | key;
            best = word < best ? word : best;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long t = __shfl_xor(best, o);
            best = t < best ? t : best;
        }
        if (lane == 0) wmin[wave] = best;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < ST_WAVES; ++w) best = wmin[w] < best ? wmin[w] : best;
        const int key = (int)(best & ((1u << ST_KEY_BITS) - 1));
        const long s_m = a_m + ((key & 1) ? -(key >> 1) : (key >> 1));
        if (tid == 0) {
            pw[m] = (int)s_m;
            if (prow) prow[m] = (int32_t)s_m;
            if (drow) drow[m] = (int64_t)(best >> ST_KEY_BITS);
        }
        s_prev = s_m;
        // ---- the next span lands: every read of this frame's lies before the barrier above ----
        if (more) {
#pragma unroll
            for (int i = 0; i < ST_PER; ++i) {
                const int k = i * ST_THREADS + tid;
                if (k < span) raw[k] = (short)quantise(pf[i], e);
            }
        }
        __syncthreads();
    }
}

// grid (chunks of the output, B)
__global__ __launch_bounds__(ST_THREADS) void stretch_synth_kernel(const void* const* __restrict__ x_rows, const int64_t* __restrict__ n,
                                                                   long max_n, int W, int num, int den, const unsigned* __restrict__ peaks,
                                                                   const int* __restrict__ posw, long Jmax, const float* __restrict__ win,
                                                                   float* __restrict__ out, long ld, long cols) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const long nb = clamp_len(n, b, max_n);
    const int Hs = W / 2;
    const long n_out = (nb * den + num - 1) / num;
    const bool defined = nb > 0 && peak_defined(peaks[b]);
    const long len = !defined ? 0 : (n_out < cols ? n_out : cols);
    const float* x = defined ? reinterpret_cast<const float*>(x_rows[b]) : nullptr;
    const int* pw = posw + (long)b * Jmax;
    float* o = out + (long)b * ld;
    long t = (long)blockIdx.x * SY_CHUNK + tid;
#pragma unroll 1
    for (int k = 0; k < SY_PER; ++k, t += ST_THREADS) {
        if (t >= cols) break;
        float y = 0.0f;
        if (t < len) {
            const long j = t / Hs;  // j < J <= Jmax
            const int u = (int)(t - j * Hs);
            const long ia = (long)pw[j] + u;
            const long ib = (j > 0 ? (long)pw[j - 1] : -(long)Hs) + Hs + u;
            const float xa = (ia >= 0 && ia < nb) ? x[ia] : 0.0f;
            const float xb = (ib >= 0 && ib < nb) ? x[ib] : 0.0f;
            const float tail = win[u + Hs] * xb;  // rounded to f32 once (no contraction in this file)
            y = fmaf(win[u], xa, tail);
        }
        o[t] = y;
    }
}

// where swc_stretch keeps what inside its workspace (byte offsets): the peaks [B] u32, the window [W] f32, s_m [B][Jmax] i32
struct WsLayout {
    size_t peaks, win, pos, total;
    int64_t Jmax;
};

WsLayout ws_layout(int B, int64_t max_n, int W, int num, int den) {
    WsLayout P;
    P.Jmax = frames_of(out_len(max_n, num, den), W / 2);
    size_t o = 0;
    P.peaks = o; o += up256((size_t)B * sizeof(unsigned));
    P.win = o; o += up256((size_t)W * sizeof(float));
    P.pos = o; o += up256((size_t)B * (size_t)P.Jmax * sizeof(int));
    P.total = o;
    return P;
}

}  // namespace

extern "C" int64_t swc_stretch_out_len(int64_t n, int32_t num, int32_t den) {
    if (n < 0 || n > SWC_STRETCH_MAX_N || !speed_ok(num, den)) return -1;
    return out_len(n, num, den);
}

extern "C" int64_t swc_stretch_workspace_bytes(int32_t B, int64_t max_n, int32_t W, int32_t num, int32_t den) {
    if (B < 0 || B > 65535 || max_n < 0 || max_n > SWC_STRETCH_MAX_N || !window_ok(W) || !speed_ok(num, den)) return -1;
    return (int64_t)ws_layout(B, max_n, W, num, den).total;
}

extern "C" int swc_stretch(const void* const* x_rows, const int64_t* n, int64_t max_n, int32_t W, int32_t D, int32_t num, int32_t den,
                           float* out, int64_t ld, int64_t cols, int32_t* pos, int64_t* dist, int64_t ldm, int32_t* flags, void* workspace,
                           int64_t workspace_bytes, int32_t B, void* stream) {
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_stretch: B=%d (0..65535)", B);
    SWC_CHECK_ARG(window_ok(W), "swc_stretch: W=%d (a multiple of 8 in %d..%d)", W, SWC_STRETCH_MIN_W, SWC_STRETCH_MAX_W);
    SWC_CHECK_ARG(D >= 0 && D <= SWC_STRETCH_MAX_D, "swc_stretch: D=%d (0..%d)", D, SWC_STRETCH_MAX_D);
    SWC_CHECK_ARG(speed_ok(num, den), "swc_stretch: speed %d/%d (terms in 1..%d, 1/%d <= num/den <= %d)", num, den, SWC_STRETCH_MAX_TERM,
                  SWC_STRETCH_MAX_RATIO, SWC_STRETCH_MAX_RATIO);
    SWC_CHECK_ARG(max_n >= 0 && max_n <= SWC_STRETCH_MAX_N, "swc_stretch: max_n=%lld (0..%d)", (long long)max_n, SWC_STRETCH_MAX_N);
    SWC_CHECK_ARG(out == nullptr || (cols >= 0 && cols <= ld), "swc_stretch: cols=%lld, ld=%lld (0 <= cols <= ld)", (long long)cols,
                  (long long)ld);
    SWC_CHECK_ARG(out || pos || dist || flags, "swc_stretch: no output (out, pos, dist and flags are all null)");
    const WsLayout P = ws_layout(B, max_n, W, num, den);
    SWC_CHECK_ARG((pos == nullptr && dist == nullptr) || ldm >= P.Jmax, "swc_stretch: ldm=%lld, %lld frames", (long long)ldm,
                  (long long)P.Jmax);
    if (B == 0) return SWC_OK;
    SWC_CHECK_ARG(x_rows && n && workspace, "swc_stretch: null pointer");
    SWC_CHECK_ARG((((uintptr_t)x_rows | (uintptr_t)n | (uintptr_t)dist) & 7u) == 0 &&
                      (((uintptr_t)out | (uintptr_t)pos | (uintptr_t)flags) & 3u) == 0 && ((uintptr_t)workspace & 255u) == 0,
                  "swc_stretch: misaligned pointer (the workspace is 256-byte aligned)");
    SWC_CHECK_ARG(workspace_bytes >= (int64_t)P.total, "swc_stretch: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                  (long long)P.total);
    SWC_CHECK_ARG(out == nullptr || (cols + SY_CHUNK - 1) / SY_CHUNK <= 0x7fffffffLL, "swc_stretch: cols=%lld", (long long)cols);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* base = reinterpret_cast<unsigned char*>(workspace);
    unsigned* peaks = reinterpret_cast<unsigned*>(base + P.peaks);
    float* win = reinterpret_cast<float*>(base + P.win);
    int* posw = reinterpret_cast<int*>(base + P.pos);
    if (hipMemsetAsync(peaks, 0, (size_t)B * sizeof(unsigned), st) != hipSuccess) {
        (void)hipGetLastError();
        swc_set_error("swc_stretch: clearing the peaks failed");
        return SWC_E_LAUNCH;
    }
    const dim3 block(ST_THREADS);
    if (max_n > 0) {
        hipLaunchKernelGGL(stretch_peak_kernel, dim3((unsigned)((max_n + PK_CHUNK - 1) / PK_CHUNK), (unsigned)B), block, 0, st, x_rows, n,
                           (long)max_n, peaks);
        SWC_CHECK_LAUNCH("swc_stretch (peak)");
    }
    hipLaunchKernelGGL(stretch_track_kernel, dim3((unsigned)B), block, 0, st, x_rows, n, (long)max_n, (int)W, (int)D, (int)num, (int)den,
                       (const unsigned*)peaks, posw, (long)P.Jmax, pos, dist, (long)ldm, flags);
    SWC_CHECK_LAUNCH("swc_stretch (track)");
    if (out != nullptr && cols > 0) {
        hipLaunchKernelGGL(stretch_window_kernel, dim3((unsigned)((W + ST_THREADS - 1) / ST_THREADS)), block, 0, st, win, (int)W);
        SWC_CHECK_LAUNCH("swc_stretch (window)");
        hipLaunchKernelGGL(stretch_synth_kernel, dim3((unsigned)((cols + SY_CHUNK - 1) / SY_CHUNK), (unsigned)B), block, 0, st, x_rows, n,
                           (long)max_n, (int)W, (int)num, (int)den, (const unsigned*)peaks, (const int*)posw, (long)P.Jmax,
                           (const float*)win, out, (long)ld, (long)cols);
        SWC_CHECK_LAUNCH("swc_stretch (synthesis)");
    }
    return SWC_OK;
}
