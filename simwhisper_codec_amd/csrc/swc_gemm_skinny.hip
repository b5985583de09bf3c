// swc_gemm, "skinny" geometry: implicit-GEMM Conv1d with few output rows and a long reduction (the k7 convolutions of the two
// samplers at the metric batch: 6048 or 4000 rows x 512 columns, taps x K = 3584), bf16 and split-f16 operands.
//
// The implicit-conv staging of swc_gemm.hip re-derives every lane's source address in every slice (tap, K tail and row tests,
// a 64-bit multiply per 16-byte chunk, six chunks per lane): on its 64 x 128 tile that is more issue time than the slice's 24
// MFMAs per wave, with at most two waves per SIMD to hide it behind.  Here, with K a multiple of the slice:
//   * every lane keeps one source pointer per LDS-DMA instruction and advances it by 128 bytes per slice (W: always; A: re-made
//     when the tap changes, which is also the only time the zero-page lanes of padded taps and rows beyond M change);
//   * the stages form a ring of DEPTH = 3, and the slice fence is a counted vmcnt that leaves one slice in flight behind the
//     one it waits for (LDS-DMA retires in issue order);
//   * the four waves sit side by side along N (64 rows x 32 columns each): every wave stages and reads its own 32 rows of W,
//     all of them read the 64 rows of A.  Same LDS image and swizzle as swc_gemm.hip.
// 24 KiB per stage, < 128 registers: two workgroups per CU, one tile per workgroup.
//
// SWC_SKINNY_WREG=1 (a build option, not shipped) streams W global -> VGPR instead, straight from the row-major operand through
// a register ring, so that only A touches LDS.  It measured SLOWER than the old geometry on every launch with more than 256
// tiles and on every plain GEMM, whatever the ring depth (4, 6) and the waves per workgroup (4, 8): a fragment-shaped load takes
// 16 bytes from each of 16 rows per quarter wave, and the launches are bound by that address path, not by latency
// (profiles/gemm_skinny_ab.txt).
//
// Arithmetic: the products of a slice in the order of swc_gemm.hip (split-f16: W_lo A_hi, W_hi A_lo, W_hi A_hi; bf16: chunk fh,
// chunk fh + 4), slices in ascending k, taps in ascending order, the epilogue expressions of swc_gemm.hip per element — every
// output is bit-identical to what the other geometries give for the same row.
//
// Accumulator tile j of a wave holds weight rows 16j + fr: lane (fr, fh) owns, for activation row 16i + fr, the output columns
// 16j + 4fh + e (with W in registers: rows {8a + 4j + b}, fr = 4a + b, and the 8 contiguous columns 8fh + 4j + e).
#include <type_traits>
#include "swc_mfma.h"
#include "swc_gemm_skinny.h"

// Build options (A/B builds only; the defaults are what was measured fastest, profiles/gemm_skinny_ab.txt)
#ifndef SWC_SKINNY_DEPTH  // stages of the LDS ring (and of the register ring of W)
#define SWC_SKINNY_DEPTH 3
#endif
#ifndef SWC_SKINNY_WREG   // 1: W global -> registers, fragment-shaped loads; 0: W through LDS like A
#define SWC_SKINNY_WREG 0
#endif

namespace {

__device__ __attribute__((aligned(16))) unsigned int g_zero16[4] = {0u, 0u, 0u, 0u};

// the LDS image of swc_gemm.hip: row r (128 bytes) holds logical chunk c at position c ^ swz(r); conflict-free ds_read_b128 of 16
// consecutive rows
__device__ __forceinline__ int swz(int row) { return ((row >> 1) ^ ((row >> 4) << 1)) & 7; }
__device__ __forceinline__ int lds_off(int row, int chunk) { return row * 128 + ((chunk ^ swz(row)) << 4); }

struct SkinnyP {
    const char* A;
    const char* W;
    void* C;
    const float* bias;
    const float* gamma;
    const float* residual;
    long ldc, ldr;                  // elements
    unsigned lda_bytes, ldw_bytes;  // whole operands stay below 2 GiB (gemm_plan): 32-bit lane offsets
    int M, N, K;
    int taps, dil, stride, pad, t_in, t_out;
    int act;
    float alpha, out_scale;
    unsigned* sat;
    int kc_per_tap, n_tiles_n, n_tiles_m;
};

template <typename OutT>
__device__ __forceinline__ float epi_act(float x) {
    return __is_same(OutT, bf16_t) ? gelu_fast(x) : (__is_same(OutT, f16s_t) ? gelu_as(x) : gelu_erf(x));
}

// Lane (fr, fh): rows bm + 16i + fr, columns col0 + CS j + e.  Per element the expressions of gemm_epilogue_direct /
// gemm_epilogue_slab in swc_gemm.hip, in their order: acc * alpha + bias, GELU, * gamma (f32 outputs), + residual, conversion.
template <typename OutT, bool GELU, int NJ, int CS>
__device__ __forceinline__ void skinny_epilogue(const SkinnyP& p, f32x4 (&acc)[4][NJ], int bm, int col0, int fr) {
    constexpr bool F16S_OUT = __is_same(OutT, f16s_t);
    constexpr bool F32_OUT = __is_same(OutT, float);
    float amax = 0.f;
    (void)amax;
    const bool res_vec = !p.residual || ((p.ldr & 3) == 0 && (reinterpret_cast<uintptr_t>(p.residual) & 15) == 0);
    const bool out_vec = F16S_OUT || ((p.ldc & 3) == 0 && (reinterpret_cast<uintptr_t>(p.C) & 15) == 0);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = col0 + CS * j;
        if (col >= p.N) continue;
        const bool vec = col + 4 <= p.N && res_vec && out_vec;
        float bv[4], gv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bv[e] = (p.bias && col + e < p.N) ? p.bias[col + e] : 0.f;
            gv[e] = (F32_OUT && p.gamma && col + e < p.N) ? p.gamma[col + e] : 1.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = bm + 16 * i + fr;
            if (row >= p.M) continue;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = acc[i][j][e] * p.alpha + bv[e];
                if constexpr (GELU) v[e] = epi_act<OutT>(v[e]);
                if constexpr (F32_OUT) v[e] *= gv[e];
            }
            if (vec) {
                if (p.residual) {
                    const float4 r4 = *reinterpret_cast<const float4*>(p.residual + (long)row * p.ldr + col);
                    v[0] += r4.x; v[1] += r4.y; v[2] += r4.z; v[3] += r4.w;
                }
                if constexpr (F16S_OUT) {
                    const float os = p.out_scale;
                    f16s_store4(reinterpret_cast<unsigned short*>(p.C) + (long)row * p.ldc * 2, col, v[0] * os, v[1] * os, v[2] * os,
                                v[3] * os, amax);
                } else if constexpr (F32_OUT) {
                    *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.C) + (long)row * p.ldc + col) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
                    *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(p.C) + (long)row * p.ldc + col) =
                        make_uint2(bf16_pack2(v[0], v[1]), bf16_pack2(v[2], v[3]));
                }
            } else {
                if (p.residual) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (col + e < p.N) v[e] += p.residual[(long)row * p.ldr + col + e];
                }
                if constexpr (F16S_OUT) {  // N % 32 == 0 (swc_gemm checks): a group below N lies inside it
                    const float os = p.out_scale;
                    f16s_store4(reinterpret_cast<unsigned short*>(p.C) + (long)row * p.ldc * 2, col, v[0] * os, v[1] * os, v[2] * os,
                                v[3] * os, amax);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (col + e < p.N) store_out<OutT>(reinterpret_cast<OutT*>(p.C) + (long)row * p.ldc + col + e, v[e]);
                }
            }
        }
    }
    if constexpr (F16S_OUT) sat_commit(p.sat, 0, amax, SWC_F16S_LIMIT);
}

template <int MODE, typename OutT, int D, int NW, bool WREG>
__global__ __launch_bounds__(64 * NW, SWC_SKINNY_WG_PER_CU * NW / 4) void gemm_skinny_kernel(SkinnyP p) {
    static_assert(WREG || NW == 4, "W through LDS: 4 waves");
    static_assert(MODE == SWC_BF16 || MODE == SWC_F16S, "16-bit MFMA operands only");
    static_assert(NW == 4 || NW == 8, "4 waves of 32 columns or 8 waves of 16");
    constexpr bool F16S = MODE == SWC_F16S;
    constexpr int A_BYTES = 64 * 128;                        // one slice of A: 64 rows x 128 bytes
    constexpr int W_WAVE = WREG ? 0 : (128 / NW) * 128;      // one slice of a wave's own W rows (W through LDS)
    constexpr int STAGE = A_BYTES + NW * W_WAVE;
    constexpr int NJ = 8 / NW;       // 16-column accumulator tiles per wave
    constexpr int NA = 8 / NW;       // LDS-DMA wave-instructions (8 rows each) of A per wave and slice
    constexpr int NWD = W_WAVE / 1024;  // LDS-DMA wave-instructions of W per wave and slice
    // vector-memory operations of one slice per wave: NA LDS-DMA + 2 NJ W loads, or NA + NWD LDS-DMA
    constexpr int VM_PER_SLICE = NA + (WREG ? 2 * NJ : NWD);
    static_assert(D >= 2 && VM_PER_SLICE * (D - 2) <= 63, "the slice fence leaves VM_PER_SLICE (D - 2) operations in flight: vmcnt has 6 bits");

    extern __shared__ __attribute__((aligned(16))) char smem[];  // [D][64 rows of A | NW x 32 rows of W][128 B]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fh = lane >> 4;

    // tile order of swc_gemm.hip (band 1): workgroups b and b + 8 share an XCD, every XCD owns a contiguous chunk of the
    // row-major tile sequence; grid == tiles
    const int ntiles = p.n_tiles_m * p.n_tiles_n;
    const int xcd = blockIdx.x & 7;
    const int cq = ntiles >> 3, cr = ntiles & 7;
    const int chunk_start = xcd < cr ? xcd * (cq + 1) : cr * (cq + 1) + (xcd - cr) * cq;
    const int chunk_size = cq + (xcd < cr ? 1 : 0);
    const int tl = blockIdx.x >> 3;
    if (tl >= chunk_size) return;
    const int bid = chunk_start + tl;
    const int tm = bid / p.n_tiles_n;
    const int bm = tm * SWC_SKINNY_TILE_M, bn = (bid - tm * p.n_tiles_n) * SWC_SKINNY_TILE_N;

    // ---- A staging: one LDS-DMA wave-instruction writes 8 rows lane-linearly; thread (ld_row, ld_pos) fetches the chunk that
    // belongs at position ld_pos of row ld_row (and ld_row + 32 with 4 waves)
    const int ld_pos = tid & 7, ld_row = tid >> 3;
    unsigned a_off[NA];
    int a_ts[NA];
    bool a_rowok[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int row = ld_row + 32 * i;
        const int r = bm + row;
        a_rowok[i] = r < p.M;
        const int rr = a_rowok[i] ? r : 0;
        const int b = rr / p.t_out;
        a_ts[i] = (rr - b * p.t_out) * p.stride;
        a_off[i] = (unsigned)(b * p.t_in + a_ts[i]) * p.lda_bytes + ((unsigned)(ld_pos ^ swz(row)) << 4);
    }
    // ---- W: lane (fr, fh) reads chunk fh (and fh + 4) of rows wn0 + 4 NJ (fr >> 2) + 4j + (fr & 3); rows beyond N are clamped
    // (their columns are never stored)
    const int wn0 = bn + 16 * NJ * wave;
    unsigned w_off[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int n = min(wn0 + 4 * NJ * (fr >> 2) + 4 * j + (fr & 3), p.N - 1);
        w_off[j] = (unsigned)n * p.ldw_bytes + 16u * (unsigned)fh;
    }
    const unsigned smem_base = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));

    // ---- W through LDS: every wave stages and reads its own 32 rows (no other wave needs them); rows 16j + fr of accumulator
    // tile j: lane (fr, fh) owns columns 16j + 4fh + e
    const char* w_ptr[NWD ? NWD : 1];
    auto set_w = [&]() {
#pragma unroll
        for (int q = 0; q < NWD; ++q) {
            const int row = (lane >> 3) + 8 * q;
            const int n = min(wn0 + row, p.N - 1);
            w_ptr[q] = p.W + (long)n * p.ldw_bytes + (((lane & 7) ^ swz(row)) << 4);
        }
    };
    set_w();
    u32x4 ring[WREG ? D : 1][2 * NJ];  // [slice % D][2j + (0: chunk fh = hi halves / first k-group, 1: chunk fh + 4 = lo halves / second k-group)]
    // The next slice to issue.  Slices are 128 bytes apart along a row of W through all taps (K is a multiple of the slice) and
    // along a row of A inside a tap; which lanes of A take the zero page (a tap outside [0, t_in), a row beyond M) changes with
    // the tap only: per-lane source pointers, re-made when the tap changes, advanced by 128 or (zero page) by 0
    int is_kc = 0, is_tap = 0;
    const char* wb = p.W;
    const char* a_ptr[NA];
    unsigned a_inc[NA];
    auto set_tap = [&](int tap) {
        const int shift = tap * p.dil - p.pad;
        const char* ab = p.A + (long)shift * p.lda_bytes;  // wave-uniform
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int ts = a_ts[i] + shift;
            const bool ok = a_rowok[i] && ts >= 0 && ts < p.t_in;
            a_ptr[i] = ok ? ab + a_off[i] : reinterpret_cast<const char*>(g_zero16);
            a_inc[i] = ok ? 128u : 0u;
        }
    };
    set_tap(0);
    // the next slice of both operands into stage / ring slot ST: NA LDS-DMA + 2 NJ W loads per wave, which the fence counts on
    auto issue = [&](auto ST) {
        constexpr int st = decltype(ST)::value;
        const unsigned sa = smem_base + st * STAGE + wave * 1024;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            glds16(a_ptr[i], sa + 32 * i * 128);
            a_ptr[i] += a_inc[i];
        }
        if constexpr (WREG) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                ring[st][2 * j] = *reinterpret_cast<const u32x4*>(wb + w_off[j]);
                ring[st][2 * j + 1] = *reinterpret_cast<const u32x4*>(wb + w_off[j] + 64);
            }
            wb += 128;
        } else {
            const unsigned sw = smem_base + st * STAGE + A_BYTES + wave * W_WAVE;
#pragma unroll
            for (int q = 0; q < NWD; ++q) {
                glds16(w_ptr[q], sw + q * 1024);
                w_ptr[q] += 128;
            }
        }
        if (++is_kc == p.kc_per_tap) {  // wave-uniform
            is_kc = 0;
            set_tap(++is_tap);  // behind the last tap: pointers that nothing loads from
        }
    };
    // the LDS-DMA is invisible to the compiler: order it ourselves.  lgkmcnt(0): every fragment read of this wave has returned
    // before another wave may overwrite the stage
    auto fence = [&](auto LEFT) {
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(decltype(LEFT)::value) : "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };

    f32x4 acc[4][NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    auto compute = [&](auto ST) {
        constexpr int st = decltype(ST)::value;
        const char* sa = smem + st * STAGE;
        uint4 a0[4], a1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a0[i] = *reinterpret_cast<const uint4*>(sa + lds_off(16 * i + fr, fh));
#pragma unroll
        for (int i = 0; i < 4; ++i) a1[i] = *reinterpret_cast<const uint4*>(sa + lds_off(16 * i + fr, fh + 4));
        u32x4 wf[2 * NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if constexpr (WREG) {
                wf[2 * j] = ring[st][2 * j];
                wf[2 * j + 1] = ring[st][2 * j + 1];
            } else {
                const char* sw = sa + A_BYTES + wave * W_WAVE;
                wf[2 * j] = *reinterpret_cast<const u32x4*>(sw + lds_off(16 * j + fr, fh));
                wf[2 * j + 1] = *reinterpret_cast<const u32x4*>(sw + lds_off(16 * j + fr, fh + 4));
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                f32x4 c = acc[i][j];
                if constexpr (F16S) {
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<f16x8*>(&wf[2 * j + 1]), *reinterpret_cast<f16x8*>(&a0[i]), c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<f16x8*>(&wf[2 * j]), *reinterpret_cast<f16x8*>(&a1[i]), c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<f16x8*>(&wf[2 * j]), *reinterpret_cast<f16x8*>(&a0[i]), c, 0, 0, 0);
                } else {
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<bf16x8*>(&wf[2 * j]), *reinterpret_cast<bf16x8*>(&a0[i]), c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<bf16x8*>(&wf[2 * j + 1]), *reinterpret_cast<bf16x8*>(&a1[i]), c, 0, 0, 0);
                }
                acc[i][j] = c;
            }
    };
    // slice kt sits in stage kt % D; while it is computed, slice kt + D - 1 is issued into the stage slice kt - 1 has left
    auto step = [&](auto U, auto MORE) {
        constexpr int u = decltype(U)::value;
        if constexpr (decltype(MORE)::value) issue(std::integral_constant<int, (u + D - 1) % D>{});
        compute(U);
        // slice kt + 1 has landed once all but the operations of slices kt + 2 .. kt + D - 1 are done
        if constexpr (decltype(MORE)::value) fence(std::integral_constant<int, VM_PER_SLICE*(D - 2)>{});
        else fence(std::integral_constant<int, 0>{});
    };

    const int nkt = p.taps * p.kc_per_tap;
    // prologue: slices 0 .. D - 2.  Always D - 1 slices and no branch around a load, so that hipcc's own count of the W loads in
    // flight is exact at the head of the loop (behind a conditional load it waits for vmcnt(0) in every round of the loop): a
    // reduction shorter than that loads slice 0 again, into a stage and a ring slot that nothing reads
    auto prologue = [&](auto self, auto S) {
        constexpr int s = decltype(S)::value;
        if constexpr (s < D - 1) {
            if (s >= nkt) {  // wave-uniform
                is_kc = is_tap = 0;
                wb = p.W;
                set_w();
                set_tap(0);
            }
            issue(S);
            self(self, std::integral_constant<int, s + 1>{});
        }
    };
    prologue(prologue, std::integral_constant<int, 0>{});
    fence(std::integral_constant<int, 0>{});

    auto steps = [&](auto self, auto U, int kt0, auto MORE) {
        constexpr int u = decltype(U)::value;
        if constexpr (u < D) {
            if constexpr (decltype(MORE)::value) {
                step(U, std::true_type{});
            } else if (kt0 + u < nkt) {  // wave-uniform
                if (kt0 + u + D - 1 < nkt) step(U, std::true_type{});
                else step(U, std::false_type{});
            }
            self(self, std::integral_constant<int, u + 1>{}, kt0, MORE);
        }
    };
    int kt0 = 0;
    for (; kt0 + 2 * D - 1 <= nkt; kt0 += D) steps(steps, std::integral_constant<int, 0>{}, kt0, std::true_type{});  // every step issues
    for (; kt0 < nkt; kt0 += D) steps(steps, std::integral_constant<int, 0>{}, kt0, std::false_type{});

    // columns of accumulator tile j: W in registers 4 NJ fh + 4j + e, W through LDS 16j + 4fh + e
    const int col0 = wn0 + (WREG ? 4 * NJ : 4) * fh;
    constexpr int CS = WREG ? 4 : 16;
    if (p.act == SWC_ACT_GELU) skinny_epilogue<OutT, true, NJ, CS>(p, acc, bm, col0, fr);
    else skinny_epilogue<OutT, false, NJ, CS>(p, acc, bm, col0, fr);
}

template <int MODE, typename OutT>
int launch(const SkinnyP& p, hipStream_t s) {
    constexpr int D = SWC_SKINNY_DEPTH, NW = SWC_SKINNY_WAVES;
    constexpr bool WREG = SWC_SKINNY_WREG != 0;
    constexpr int LDS = D * (WREG ? 8192 : 8192 + 128 * 128);
    static_assert(SWC_SKINNY_WG_PER_CU * LDS <= 160 * 1024, "the stages of the resident workgroups must fit the CU's LDS");
    auto kern = gemm_skinny_kernel<MODE, OutT, D, NW, WREG>;
    if (LDS > 64 * 1024) SWC_ENABLE_LDS(kern, LDS, "swc_gemm");
    hipLaunchKernelGGL(kern, dim3((unsigned)(p.n_tiles_m * p.n_tiles_n)), dim3(64 * NW), LDS, s, p);
    return SWC_OK;
}

}  // namespace

int swc_gemm_skinny_launch(const swc_gemm_args* a, int n_tiles_m, int n_tiles_n, int kc_per_tap, unsigned* sat, hipStream_t s) {
    const int es = a->a_dtype == SWC_F16S ? 4 : 2;
    SkinnyP p;
    p.A = (const char*)a->A;
    p.W = (const char*)a->W;
    p.C = a->C;
    p.bias = a->bias;
    p.gamma = a->gamma;
    p.residual = a->residual;
    p.ldc = a->ldc; p.ldr = a->ldr;
    p.lda_bytes = (unsigned)(a->lda * es); p.ldw_bytes = (unsigned)(a->ldw * es);
    p.M = a->M; p.N = a->N; p.K = a->K;
    p.taps = a->taps; p.dil = a->dil; p.stride = a->stride; p.pad = a->pad;
    p.t_in = a->t_in; p.t_out = a->t_out;
    p.act = a->act;
    p.alpha = a->alpha == 0.0f ? 1.0f : a->alpha;
    p.out_scale = a->out_scale == 0.0f ? 1.0f : a->out_scale;
    p.sat = sat;
    p.kc_per_tap = kc_per_tap; p.n_tiles_n = n_tiles_n; p.n_tiles_m = n_tiles_m;
    if (a->a_dtype == SWC_F16S) return a->c_dtype == SWC_F16S ? launch<SWC_F16S, f16s_t>(p, s) : launch<SWC_F16S, float>(p, s);
    return a->c_dtype == SWC_BF16 ? launch<SWC_BF16, bf16_t>(p, s) : launch<SWC_BF16, float>(p, s);
}
