// swc_code_usage and swc_code_compare (include/swc_units.h): what a ragged batch of code streams uses of its codebooks, and
// how far apart two batches of streams are.  Integer arithmetic only; no workgroup waits for another; no workspace.
//   code_usage_kernel<E>   grid (chunks, B, G): a workgroup of 256 threads takes SWC_UNITS_CHUNK frames of one (utterance,
//                          group), counts them into an LDS histogram of n_codes int32 (LDS atomics) and adds the non-zero
//                          bins to `hist` (64-bit atomicAdd).  Frame t looks at frame t - 1 for the repeat count: the first
//                          frame of every chunk but an utterance's first reads the last frame of the chunk before.  The repeat
//                          and invalid counts are summed over a wave first: one atomic per wave and counter.
//   code_count_kernel<E>   grid (B): the positional counts of a pair.  Thread tid walks t = tid, tid + 256, ... over all G
//                          groups with its 83 counters in registers (the loops over groups and dimensions are unrolled, so
//                          every index is a constant); then a sum over each wave, the four waves through LDS, plain stores.
//                          A code is taken apart into its levels only where the two codes differ.
//   code_edit_kernel<E>    grid (G, B): the edit distance of one (pair, group).  Both streams are staged in LDS as 16-bit
//                          symbols (0xffff = invalid: `differs` makes it unequal to itself), raw into the boundary row's
//                          space first and from there compacted (a ballot scan over "differs from its predecessor", 256
//                          values a round) into their own rows.  The recurrence walks the matrix in strips of
//                          SWC_UNITS_STRIP = 256 rows the way dtw_dp_kernel of swc_mcd.hip does: thread r owns row i0 + r + 1
//                          and is at column s - r + 1 at step s; D(i-1, j) is what thread r - 1 wrote to LDS one step earlier
//                          (two buffers, one barrier per step), D(i-1, j-1) what this thread read one step earlier,
//                          D(i, j-1) its own last value.  Thread 0's neighbour is the last row of the strip before, kept in
//                          LDS IN PLACE: thread 255 writes column s - 254 at the step at which thread 0 reads column s + 1,
//                          and thread 0 has read a column 255 steps before it is overwritten.
//                          LDS: 2 x 16 KB symbols + 32 KB boundary row + 2 KB of keys.
// Every store to global memory is an ordinary vector store or a vector atomic from plain C++.
#include "swc_common.h"
#include "swc_units.h"

namespace {

constexpr int UN_THREADS = 256;
constexpr int UN_WAVES = UN_THREADS / 64;
constexpr int UN_CHUNK = SWC_UNITS_CHUNK;
constexpr int UN_MAXF = SWC_UNITS_MAX_FRAMES;
constexpr int UN_MAXG = SWC_UNITS_MAX_GROUPS;
constexpr int UN_STRIP = SWC_UNITS_STRIP;
constexpr unsigned short UN_INVALID = 0xffffu;
typedef unsigned long long u64;

static_assert(UN_STRIP == UN_THREADS, "one row of a strip per thread");
static_assert(SWC_UNITS_MAX_CODES < UN_INVALID, "a symbol fits 16 bits beside the reserved one");

struct UnLevels { int L[4]; int n_codes; };

__device__ __forceinline__ int clamp_len(const int64_t* n, int b, int max_frames) {
    const long T = n[b];
    return T < 0 ? 0 : (T > max_frames ? max_frames : (int)T);
}

template <typename E>
__device__ __forceinline__ bool code_valid(E v, int n_codes) { return v >= 0 && v < (E)n_codes; }

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---------------------------------------------------------------- swc_code_usage ----

template <typename E>
__global__ __launch_bounds__(UN_THREADS) void code_usage_kernel(const void* const* __restrict__ rows, const int64_t* __restrict__ ldgs,
                                                                const int64_t* __restrict__ n_frames, int max_frames, int n_codes,
                                                                u64* __restrict__ hist, u64* __restrict__ repeats,
                                                                u64* __restrict__ totals) {
    extern __shared__ int s_hist[];  // n_codes
    const int tid = threadIdx.x, b = blockIdx.y, g = blockIdx.z;
    const int T = clamp_len(n_frames, b, max_frames);
    const int t0 = blockIdx.x * UN_CHUNK;
    if (t0 >= T) return;  // (uniform) also every utterance without frames: its row is not read
    if (blockIdx.x == 0 && g == 0 && tid == 0) atomicAdd(totals, (u64)T);
    for (int c = tid; c < n_codes; c += UN_THREADS) s_hist[c] = 0;
    __syncthreads();
    const E* row = reinterpret_cast<const E*>(rows[b]) + (long)g * ldgs[b];
    const int tend = t0 + UN_CHUNK < T ? t0 + UN_CHUNK : T;
    int rep = 0, bad = 0;
    for (int t = t0 + tid; t < tend; t += UN_THREADS) {
        const E v = row[t];
        const bool ok = code_valid(v, n_codes);
        if (ok) atomicAdd(&s_hist[(int)v], 1);
        bad += !ok;
        if (t >= 1) rep += ok && row[t - 1] == v;  // (the frame before is this utterance's, in this chunk or the one before)
    }
    __syncthreads();
    for (int c = tid; c < n_codes; c += UN_THREADS) {
        const int n = s_hist[c];
        if (n) atomicAdd(hist + (long)g * n_codes + c, (u64)n);
    }
    rep = wave_sum_int(rep);
    bad = wave_sum_int(bad);
    if ((tid & 63) == 0) {
        if (rep) atomicAdd(repeats + g, (u64)rep);
        if (bad) atomicAdd(totals + 1, (u64)bad);
    }
}

// ---------------------------------------------------------------- swc_code_compare: positional counts ----

// the counters of one thread: match[8] | both_valid[8] | level_match[8][4] | level_l1[8][4] | frame_match | bad[2]
constexpr int CN_MATCH = 0, CN_VALID = UN_MAXG, CN_LM = 2 * UN_MAXG, CN_L1 = CN_LM + 4 * UN_MAXG, CN_FRAME = CN_L1 + 4 * UN_MAXG,
              CN_BAD = CN_FRAME + 1, CN_ALL = CN_BAD + 2;

template <typename E>
__global__ __launch_bounds__(UN_THREADS) void code_count_kernel(const void* const* __restrict__ rows_a, const int64_t* __restrict__ ldg_a,
                                                                const int64_t* __restrict__ n_a, const void* const* __restrict__ rows_b,
                                                                const int64_t* __restrict__ ldg_b, const int64_t* __restrict__ n_b,
                                                                int max_frames, int G, UnLevels K, int* __restrict__ match,
                                                                int* __restrict__ both_valid, int* __restrict__ level_match,
                                                                int* __restrict__ level_l1, int* __restrict__ frame_match,
                                                                int* __restrict__ bad) {
    __shared__ int s_acc[UN_WAVES][CN_ALL];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int Ta = clamp_len(n_a, b, max_frames), Tb = clamp_len(n_b, b, max_frames);
    const int Tmax = Ta > Tb ? Ta : Tb;
    const E* ra = Ta ? reinterpret_cast<const E*>(rows_a[b]) : nullptr;
    const E* rb = Tb ? reinterpret_cast<const E*>(rows_b[b]) : nullptr;
    const long lda = ldg_a[b], ldb = ldg_b[b];
    int acc[CN_ALL];
#pragma unroll
    for (int k = 0; k < CN_ALL; ++k) acc[k] = 0;
    for (int t = tid; t < Tmax; t += UN_THREADS) {
        const bool ina = t < Ta, inb = t < Tb;
        bool all = ina && inb;
#pragma unroll
        for (int g = 0; g < UN_MAXG; ++g) {
            if (g < G) {
                E va = 0, vb = 0;
                bool oka = false, okb = false;
                if (ina) {
                    va = ra[g * lda + t];
                    oka = code_valid(va, K.n_codes);
                    acc[CN_BAD] += !oka;
                }
                if (inb) {
                    vb = rb[g * ldb + t];
                    okb = code_valid(vb, K.n_codes);
                    acc[CN_BAD + 1] += !okb;
                }
                const bool both = ina && inb && oka && okb;
                const bool eq = both && va == vb;
                all = all && eq;
                acc[CN_MATCH + g] += eq;
                acc[CN_VALID + g] += both;
                if (eq) {
#pragma unroll
                    for (int d = 0; d < 4; ++d) acc[CN_LM + 4 * g + d] += 1;
                } else if (both) {
                    int ca = (int)va, cb = (int)vb;
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const int qa = ca / K.L[d], qb = cb / K.L[d];
                        const int la = ca - qa * K.L[d], lb = cb - qb * K.L[d];
                        acc[CN_LM + 4 * g + d] += la == lb;
                        acc[CN_L1 + 4 * g + d] += la > lb ? la - lb : lb - la;
                        ca = qa;
                        cb = qb;
                    }
                }
            }
        }
        acc[CN_FRAME] += all;
    }
#pragma unroll
    for (int k = 0; k < CN_ALL; ++k) {
        const int v = wave_sum_int(acc[k]);
        if ((tid & 63) == 0) s_acc[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid >= CN_ALL) return;
    int v = 0;
#pragma unroll
    for (int w = 0; w < UN_WAVES; ++w) v += s_acc[w][tid];
    if (tid < CN_VALID) {
        if (tid < G) match[(long)b * G + tid] = v;
    } else if (tid < CN_LM) {
        if (tid - CN_VALID < G) both_valid[(long)b * G + tid - CN_VALID] = v;
    } else if (tid < CN_L1) {
        if (tid - CN_LM < 4 * G) level_match[(long)b * G * 4 + tid - CN_LM] = v;
    } else if (tid < CN_FRAME) {
        if (tid - CN_L1 < 4 * G) level_l1[(long)b * G * 4 + tid - CN_L1] = v;
    } else if (tid == CN_FRAME) {
        frame_match[b] = v;
    } else {
        bad[(long)b * 2 + tid - CN_BAD] = v;
    }
}

// ---------------------------------------------------------------- swc_code_compare: edit distance ----

// symbols differ unless both are valid and the same: the reserved symbol differs from itself
__device__ __forceinline__ int differs(unsigned short x, unsigned short y) { return x != y || x == UN_INVALID; }

// T values of `row` as 16-bit symbols into raw[0, T)  (no barrier)
template <typename E>
__device__ __forceinline__ void stage_raw(const E* __restrict__ row, int T, int n_codes, unsigned short* raw) {
    for (int t = threadIdx.x; t < T; t += UN_THREADS) {
        const E v = row[t];
        raw[t] = code_valid(v, n_codes) ? (unsigned short)v : UN_INVALID;
    }
}

// raw[0, T) -> out[0, len): symbol t is kept when !dedup, t == 0 or it differs from symbol t - 1.  Every thread of the
// workgroup calls it (T is uniform); ends behind a barrier.  -> len
__device__ __forceinline__ int compact(const unsigned short* raw, int T, int dedup, unsigned short* out, int* s_wave) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int base = 0;
    for (int t0 = 0; t0 < T; t0 += UN_THREADS) {
        const int t = t0 + tid;
        const bool in = t < T;
        const unsigned short s = in ? raw[t] : (unsigned short)0;
        const bool keep = in && (!dedup || t == 0 || differs(s, raw[t - 1]));
        const u64 m = __ballot(keep);
        if (lane == 0) s_wave[w] = __popcll(m);
        __syncthreads();
        int off = base;
#pragma unroll
        for (int k = 0; k < UN_WAVES; ++k) {
            if (k < w) off += s_wave[k];
            base += s_wave[k];
        }
        if (keep) out[off + __popcll(m & ((1ull << lane) - 1ull))] = s;
        __syncthreads();
    }
    return base;
}

template <typename E>
__global__ __launch_bounds__(UN_THREADS) void code_edit_kernel(const void* const* __restrict__ rows_a, const int64_t* __restrict__ ldg_a,
                                                               const int64_t* __restrict__ n_a, const void* const* __restrict__ rows_b,
                                                               const int64_t* __restrict__ ldg_b, const int64_t* __restrict__ n_b,
                                                               int max_frames, int G, int n_codes, int dedup, int* __restrict__ edit,
                                                               int* __restrict__ len_a, int* __restrict__ len_b) {
    __shared__ unsigned short s_a[UN_MAXF], s_b[UN_MAXF];
    __shared__ int s_bnd[UN_MAXF + 1];       // D(i0, j), j = 1 .. lb, of the strip before; first the raw symbols of both sides
    __shared__ int s_key[2][UN_STRIP + 1];   // [step parity][1 + thread that wrote it]
    __shared__ int s_wave[UN_WAVES];
    const int tid = threadIdx.x, g = blockIdx.x, b = blockIdx.y;
    const int Ta = clamp_len(n_a, b, max_frames), Tb = clamp_len(n_b, b, max_frames);  // <= UN_MAXF: the host checks max_frames
    unsigned short* raw_a = reinterpret_cast<unsigned short*>(s_bnd);
    unsigned short* raw_b = raw_a + UN_MAXF;
    if (Ta) stage_raw<E>(reinterpret_cast<const E*>(rows_a[b]) + (long)g * ldg_a[b], Ta, n_codes, raw_a);
    if (Tb) stage_raw<E>(reinterpret_cast<const E*>(rows_b[b]) + (long)g * ldg_b[b], Tb, n_codes, raw_b);
    __syncthreads();
    const int la = compact(raw_a, Ta, dedup, s_a, s_wave);
    const int lb = compact(raw_b, Tb, dedup, s_b, s_wave);
    const long o = (long)b * G + g;
    if (tid == 0) {
        len_a[o] = la;
        len_b[o] = lb;
        if (la == 0 || lb == 0) edit[o] = la + lb;
    }
    if (la == 0 || lb == 0) return;  // uniform
    for (int i0 = 0; i0 < la; i0 += UN_STRIP) {
        const int nrows = la - i0 < UN_STRIP ? la - i0 : UN_STRIP, i = i0 + tid + 1;
        const bool mine = tid < nrows;
        const unsigned short x = mine ? s_a[i - 1] : (unsigned short)0;
        const bool writes_bound = tid == UN_STRIP - 1 && i0 + UN_STRIP < la;  // the last row, when another strip follows
        int left = i, diag = i - 1;                                          // D(i, 0) and D(i - 1, 0)
        const int steps = lb + nrows - 1;
        for (int s = 0; s < steps; ++s) {
            __syncthreads();
            const int j = s - tid + 1;
            int val = 0;
            if (mine && j >= 1 && j <= lb) {
                const int up = tid == 0 ? (i0 == 0 ? j : s_bnd[j]) : s_key[(s + 1) & 1][tid];
                const int sub = diag + differs(x, s_b[j - 1]);
                const int ins = (up < left ? up : left) + 1;
                val = sub < ins ? sub : ins;
                left = val;
                diag = up;
                if (writes_bound) s_bnd[j] = val;
                if (i == la && j == lb) edit[o] = val;
            }
            s_key[s & 1][tid + 1] = val;
        }
        __syncthreads();  // the strip's last row is complete, and the keys are free again
    }
}

bool units_levels_ok(const int32_t* lv, UnLevels* K) {
    long prod = 1;
    for (int i = 0; i < 4; ++i) {
        if (lv[i] < 2 || lv[i] > 1024) return false;
        prod *= lv[i];
        K->L[i] = lv[i];
    }
    K->n_codes = (int)prod;
    return prod <= SWC_UNITS_MAX_CODES;
}

}  // namespace

extern "C" int swc_code_usage(const void* const* rows, const int64_t* ldg, const int64_t* n_frames, int32_t elem_size,
                              const int32_t* levels_host4, int32_t G, int32_t max_frames, int64_t* hist, int64_t* repeats,
                              int64_t* totals, int32_t B, void* stream) {
    SWC_CHECK_ARG(rows && ldg && n_frames && levels_host4 && hist && repeats && totals, "swc_code_usage: null pointer");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_code_usage: B=%d (0..65535)", B);
    SWC_CHECK_ARG(elem_size == 4 || elem_size == 8, "swc_code_usage: elem_size=%d (4 = int32 or 8 = int64)", elem_size);
    SWC_CHECK_ARG(G >= 1 && G <= UN_MAXG, "swc_code_usage: G=%d (1..%d)", G, UN_MAXG);
    UnLevels K;
    SWC_CHECK_ARG(units_levels_ok(levels_host4, &K), "swc_code_usage: levels must be 4 values in 2..1024 whose product is at most %d",
                  SWC_UNITS_MAX_CODES);
    SWC_CHECK_ARG(max_frames >= 0 && max_frames <= SWC_UNITS_USAGE_MAX_FRAMES, "swc_code_usage: max_frames=%d (0..%d)", max_frames,
                  SWC_UNITS_USAGE_MAX_FRAMES);
    if (B == 0 || max_frames == 0) return SWC_OK;
    const dim3 grid((unsigned)((max_frames + UN_CHUNK - 1) / UN_CHUNK), (unsigned)B, (unsigned)G), block(UN_THREADS);
    const size_t lds = sizeof(int) * (size_t)K.n_codes;
    if (elem_size == 4)
        hipLaunchKernelGGL(code_usage_kernel<int>, grid, block, lds, (hipStream_t)stream, rows, ldg, n_frames, (int)max_frames, K.n_codes,
                           (u64*)hist, (u64*)repeats, (u64*)totals);
    else
        hipLaunchKernelGGL(code_usage_kernel<long long>, grid, block, lds, (hipStream_t)stream, rows, ldg, n_frames, (int)max_frames,
                           K.n_codes, (u64*)hist, (u64*)repeats, (u64*)totals);
    SWC_CHECK_LAUNCH("swc_code_usage");
    return SWC_OK;
}

extern "C" int swc_code_compare(const void* const* rows_a, const int64_t* ldg_a, const int64_t* n_a, const void* const* rows_b,
                                const int64_t* ldg_b, const int64_t* n_b, int32_t elem_size, const int32_t* levels_host4, int32_t G,
                                int32_t max_frames, int32_t dedup, int32_t* match, int32_t* both_valid, int32_t* level_match,
                                int32_t* level_l1, int32_t* frame_match, int32_t* bad, int32_t* edit, int32_t* len_a, int32_t* len_b,
                                int32_t B, void* stream) {
    SWC_CHECK_ARG(rows_a && ldg_a && n_a && rows_b && ldg_b && n_b && levels_host4 && match && both_valid && level_match && level_l1 &&
                      frame_match && bad && edit && len_a && len_b,
                  "swc_code_compare: null pointer");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_code_compare: B=%d (0..65535)", B);
    SWC_CHECK_ARG(elem_size == 4 || elem_size == 8, "swc_code_compare: elem_size=%d (4 = int32 or 8 = int64)", elem_size);
    SWC_CHECK_ARG(G >= 1 && G <= UN_MAXG, "swc_code_compare: G=%d (1..%d)", G, UN_MAXG);
    UnLevels K;
    SWC_CHECK_ARG(units_levels_ok(levels_host4, &K), "swc_code_compare: levels must be 4 values in 2..1024 whose product is at most %d",
                  SWC_UNITS_MAX_CODES);
    SWC_CHECK_ARG(max_frames >= 0 && max_frames <= UN_MAXF, "swc_code_compare: max_frames=%d (0..%d)", max_frames, UN_MAXF);
    if (B == 0) return SWC_OK;
    const dim3 block(UN_THREADS), grid_c((unsigned)B), grid_e((unsigned)G, (unsigned)B);
    if (elem_size == 4) {
        hipLaunchKernelGGL(code_count_kernel<int>, grid_c, block, 0, (hipStream_t)stream, rows_a, ldg_a, n_a, rows_b, ldg_b, n_b,
                           (int)max_frames, (int)G, K, match, both_valid, level_match, level_l1, frame_match, bad);
        hipLaunchKernelGGL(code_edit_kernel<int>, grid_e, block, 0, (hipStream_t)stream, rows_a, ldg_a, n_a, rows_b, ldg_b, n_b,
                           (int)max_frames, (int)G, K.n_codes, (int)dedup, edit, len_a, len_b);
    } else {
        hipLaunchKernelGGL(code_count_kernel<long long>, grid_c, block, 0, (hipStream_t)stream, rows_a, ldg_a, n_a, rows_b, ldg_b, n_b,
                           (int)max_frames, (int)G, K, match, both_valid, level_match, level_l1, frame_match, bad);
        hipLaunchKernelGGL(code_edit_kernel<long long>, grid_e, block, 0, (hipStream_t)stream, rows_a, ldg_a, n_a, rows_b, ldg_b, n_b,
                           (int)max_frames, (int)G, K.n_codes, (int)dedup, edit, len_a, len_b);
    }
    SWC_CHECK_LAUNCH("swc_code_compare");
    return SWC_OK;
}
