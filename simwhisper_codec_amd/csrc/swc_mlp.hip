// swc_mlp_block: the MLP sub-block of one OmniWhisperTransformerLayer in ONE kernel on gfx950 MFMA (modules.py:224-232):
//     x_out[M][D] = x + fc2( GELU( fc1( LayerNorm(x; ln_w, ln_b) ) ) )            residual stream f32, operands bf16
//     y_next[M][D] = LayerNorm(x_out; next_ln_w, next_ln_b) as bf16  (optional)    the NEXT sub-block's GEMM operand
// Neither the normalised operand (M x D bf16) nor the hidden activations (M x F bf16: 98 MB per layer at 32 x 10 s, written
// and read back by the two-GEMM form) nor the two LayerNorm passes around the block exist as launches or HBM traffic.
//
// Decomposition (D = 768, F % 256 == 0; 4 waves, one per SIMD, up to 512 registers each, one workgroup per CU):
//   * a workgroup owns 64 tokens (16 000 tokens at 32 x 10 s = 250 workgroups: one round over 256 CUs; a 128-token tile
//     would need 384 KiB of accumulators and 192 KiB of LDS for y and leave half the chip idle);
//   * prologue: wave w normalises tokens 16 w .. 16 w + 15 (whole 3 KiB rows per wave load, sums on the DPP path: the
//     arithmetic and order of swc_layernorm) and writes them to LDS as MFMA B-operand fragments (96 KiB, resident);
//   * the hidden dimension is walked in slices of 256.  In slice j
//       GEMM1: wave w computes H^T[64 hidden of its own][64 tokens] = W1[256 j + 64 w ..] . y^T     (K = 768, 48 k-steps)
//       GELU + bias on the accumulators, converted to bf16 IN REGISTERS (a 32 x 32 accumulator tile, rows pairwise
//              converted, IS the B operand of the next product; W2 is packed in that k order), exchanged through a 32 KiB
//              LDS buffer because every wave needs all 256 hidden values;
//       GEMM2: wave w accumulates out^T[192 columns of its own][64 tokens] += W2[n][slice j] . H^T  (192 accumulators, AGPRs);
//   * WEIGHTS NEVER TOUCH LDS: every weight fragment has exactly one consumer wave and goes global -> VGPR as one
//     contiguous 1 KiB wave load from a stream swc_mlp_pack lays out in each wave's order of consumption.  A 64-token tile
//     needs twice the weight bytes per flop of the 128-frame ConvNeXt tile (16 B per clock and wave at full MFMA rate), so
//     16 fragments (16 KiB) are in flight per wave;
//   * software pipeline as in swc_convnext.hip: GEMM1(j), then GEMM2(j-1) with the GELU of slice j spread over its 16
//     k-steps, barrier, H_j to LDS, barrier;
//   * epilogue: out^T through LDS (transposed, two passes of 32 tokens) so that the residual stream is read and written in
//     whole 3 KiB rows; the wave that stores a row has all of it in registers and emits LayerNorm_next(row) as well.
// Rows are independent: the kernel may run in place (x_out == x).
//
// swc_layer_tail = the same kernel with the attention out-projection in front (template OPROJ: attention tile to LDS by DMA, x' = x +
// att Wo^T + bo accumulated in GEMM2's registers, LayerNorm(x') taken in the accumulator layout, the MLP's residual add free), and —
// template F8, preset fp8_fc1 — with fc1 on the block-scaled fp8 MFMA.  Measured: 181 us (bf16) / 152 us (fp8 fc1)
// per layer at 16 000 tokens against 238 us for the five launches of round 3.
//
// MFMA: v_mfma_f32_32x32x16_bf16; operand maps in swc_mfma.h.
#include <type_traits>
#include "swc_mfma.h"

namespace {

constexpr int ML_D = 768;         // model width (K of GEMM1, N of GEMM2)
constexpr int ML_BM = 64;         // tokens per workgroup
constexpr int ML_SL = 256;        // hidden values per slice
#ifndef ML_PF
#define ML_PF 16                  // weight fragments in flight per wave (1 KiB each)
#endif
constexpr int ML_KS1 = ML_D / 16;   // k-steps of GEMM1 (48)
constexpr int ML_KS2 = ML_SL / 16;  // k-steps of GEMM2 (16)
constexpr int ML_NB = ML_D / 4 / 32;  // 32-column blocks of out^T per wave (6)
constexpr int ML_FPP = 96;          // fragments per phase and wave: GEMM1 48 x 2, GEMM2 16 x 6
// pitch of one y fragment in LDS: 1 KiB + 16 B.  Fragment READS are lane-linear (conflict-free at any pitch); the prologue
// WRITES 8 bytes per lane with the fragment index in the lane's upper bits: at a pitch of 1024 all 64 lanes of a
// ds_write_b64 fall into 4 banks (32-way conflict), at 1040 into 32 (4-way)
constexpr int ML_YP = 1040;
constexpr int ML_Y_BYTES = 2 * ML_KS1 * ML_YP;  // 97.5 KiB
constexpr int ML_H_BYTES = ML_SL * ML_BM * 2;  // 32 KiB
constexpr int ML_LDS = ML_Y_BYTES + ML_H_BYTES;
constexpr int ML_TLD = ML_D + 4;  // row pitch (floats) of the epilogue transpose buffer: conflict-free b128 writes
static_assert(ML_KS1 * 2 == ML_FPP && ML_KS2 * ML_NB == ML_FPP, "phase length");
static_assert(ML_FPP % ML_PF == 0, "the ring index of a fragment must not depend on the phase");
static_assert(32 * ML_TLD * 4 <= ML_LDS, "epilogue buffer");
// Timing ablations for tuning builds only (-DML_ABL=mask, wrong results): 1 = no barriers in the slice loop, 2 = no GELU
// arithmetic, 4 = no weight loads in the loop (the ring keeps its first fragments), 8 = LDS fragment reads only in the
// first k-steps of a phase, 16 = no epilogue, 32 = no prologue loads (y = garbage)
#ifndef ML_ABL
#define ML_ABL 0
#endif

// GEMM1's MFMAs of one k-step in VGPR form: 2 hidden blocks x 2 token blocks (why asm and not the builtin: see mfma32 in
// swc_mfma.h)
template <bool F16 = false>
__device__ __forceinline__ void ml_mfma2x2_vgpr(const u32x4& a0, const u32x4& a1, const u32x4& b0, const u32x4& b1,
                                                f32x16& c00, f32x16& c01, f32x16& c10, f32x16& c11) {
    if constexpr (F16)
        asm("s_nop 1\n\t"
            "v_mfma_f32_32x32x16_f16 %0, %4, %6, %0\n\t"
            "v_mfma_f32_32x32x16_f16 %1, %4, %7, %1\n\t"
            "v_mfma_f32_32x32x16_f16 %2, %5, %6, %2\n\t"
            "v_mfma_f32_32x32x16_f16 %3, %5, %7, %3"
            : "+v"(c00), "+v"(c01), "+v"(c10), "+v"(c11)
            : "v"(a0), "v"(a1), "v"(b0), "v"(b1));
    else
        asm("s_nop 1\n\t"
            "v_mfma_f32_32x32x16_bf16 %0, %4, %6, %0\n\t"
            "v_mfma_f32_32x32x16_bf16 %1, %4, %7, %1\n\t"
            "v_mfma_f32_32x32x16_bf16 %2, %5, %6, %2\n\t"
            "v_mfma_f32_32x32x16_bf16 %3, %5, %7, %3"
            : "+v"(c00), "+v"(c01), "+v"(c10), "+v"(c11)
            : "v"(a0), "v"(a1), "v"(b0), "v"(b1));
}

// fp8 fc1: one W1 fragment (16 hidden x 128 k, e4m3) against the four token tiles, accumulators in VGPRs (given the builtin, hipcc
// puts these 64 accumulators — and even operands — into AGPRs beside GEMM2's 192 and shuffles: 776 v_accvgpr_* and 250 spills).
// Scales: one VGPR holding 0x7f7f7f7f (E8M0 2^0 for every 32-block; the tensor scales live in alpha1); cbsz / blgp 0 = e4m3.
__device__ __forceinline__ void ml_mfma8_1x4_vgpr(const i32x8& a, const i32x8& b0, const i32x8& b1, const i32x8& b2, const i32x8& b3,
                                                  f32x4& c0, f32x4& c1, f32x4& c2, f32x4& c3, unsigned sc) {
    asm("s_nop 1\n\t"
        "v_mfma_scale_f32_16x16x128_f8f6f4 %0, %4, %5, %0, %9, %9 op_sel_hi:[0,0,0]\n\t"
        "v_mfma_scale_f32_16x16x128_f8f6f4 %1, %4, %6, %1, %9, %9 op_sel_hi:[0,0,0]\n\t"
        "v_mfma_scale_f32_16x16x128_f8f6f4 %2, %4, %7, %2, %9, %9 op_sel_hi:[0,0,0]\n\t"
        "v_mfma_scale_f32_16x16x128_f8f6f4 %3, %4, %8, %3, %9, %9 op_sel_hi:[0,0,0]"
        : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3)
        : "v"(a), "v"(b0), "v"(b1), "v"(b2), "v"(b3), "v"(sc));
}

// F16 (operand_dtype SWC_F16, with OPROJ): every MFMA operand INSIDE the kernel — the attention tile (converted in LDS: bf16 -> f16 is
// exact), LayerNorm(x'), GELU(h) and the three weight matrices of the stream — is IEEE half precision instead of bf16: 11
// significand bits instead of 8 at the same MFMA rate.  f16 has a finite range where bf16 has f32's: conversions saturate at
// +-65504 (one v_med3 per value; LayerNorm outputs and weights cannot get there, a hidden activation could in principle).
template <bool F16>
__device__ __forceinline__ unsigned ml_pack_x2(float lo, float hi) {
    if constexpr (F16) {
        lo = __builtin_amdgcn_fmed3f(lo, -65504.0f, 65504.0f);
        hi = __builtin_amdgcn_fmed3f(hi, -65504.0f, 65504.0f);
        return pack_f16x2(lo, hi);
    } else {
        return pack_bf16x2(lo, hi);
    }
}

struct MlNorm {
    const float* w;  // [D]
    const float* b;  // [D]
};

constexpr int ML_P0 = ML_KS1 * ML_NB;  // fragments per wave of the out-proj phase (OPROJ): 48 k-steps x 6 column blocks
static_assert(ML_P0 % ML_PF == 0, "the ring index of a fragment must not depend on the phase");

// wstream: per wave w (4 of them) [OPROJ: ML_P0 +] NS * 192 + ML_PF fragments of 1 KiB in the order of consumption
// (mlp_pack_kernel).
// OPROJ (swc_layer_tail): the attention out-projection runs in front, in the same kernel: `att` [M][D] bf16 is the
// attention output; the workgroup's tile of it goes to LDS by DMA, x' = x + att Wo^T + bo is accumulated IN the 192
// registers that later accumulate fc2 (so x' never exists in memory and the residual add of the MLP is free), LayerNorm(x')
// is taken in that transposed layout (row statistics across the 4 waves through LDS) and its bf16 fragments replace the
// attention tile in LDS.
// F8 (with OPROJ; preset fp8_fc1): fc1 alone runs on the block-scaled fp8 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4, e4m3 x e4m3,
// K = 128 per instruction at twice the bf16 rate per clock).  LayerNorm(x') is written to LDS as e4m3 at SWC_FP8_ACT_SCALE
// (48 KiB instead of 96: B fragments of 128 channels x 16 tokens, 32 bytes per lane as two lane-linear halves), W1 comes from the
// stream as e4m3 at its per-tensor power-of-two scale (half the bytes per slice), the 16 x 16 accumulator tiles get
// alpha1 = 1 / (act scale x weight scale), bias and GELU and are written to the H buffer in the 32 x 32 x 16 B-fragment layout
// (8 bytes per lane: 4 consecutive hidden values of one token), where fc2 reads them as before — in bf16, natural k order.
template <bool OPROJ, bool F8 = false, bool F16 = false>
__global__ __launch_bounds__(256, 1) void mlp_block_kernel(const float* x, float* xo, MlNorm ln, float eps,
                                                           const u32x4* __restrict__ wstream, const float* __restrict__ b1,
                                                           const float* __restrict__ b2, MlNorm nln,
                                                           bf16_t* __restrict__ y_next, int M, int NS,
                                                           const bf16_t* __restrict__ att, const float* __restrict__ bo,
                                                           float alpha1, unsigned* sat) {
    static_assert(!F8 || OPROJ, "the fp8 fc1 exists for the layer-tail form");
    static_assert(!F16 || (OPROJ && !F8), "half-precision operands exist for the bf16 layer-tail form");
    constexpr int G1F = F8 ? ML_FPP / 2 : ML_FPP;  // 1 KiB stream entries of one GEMM1 phase (e4m3: half the bytes)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lf = lane & 31, lh = lane >> 5;
    const int row0 = blockIdx.x * ML_BM;

    // ---- weight stream of this wave: wave-uniform byte pointer (SGPR pair, advanced once per phase) + one 32-bit lane
    // offset + immediate
    const long per_wave = (OPROJ ? ML_P0 : 0) + (long)NS * (G1F + ML_FPP) + ML_PF;  // fragments
    const char* wbase = reinterpret_cast<const char*>(wstream) + (long)w * per_wave * 1024;
    const unsigned lane_off = (unsigned)lane * 16u;
    auto wfrag = [&](int i) __attribute__((always_inline)) -> u32x4 {  // fragment i of the current phase (i may run ML_PF past its end)
        if (ML_ABL & 4) i &= ML_PF - 1;
        return *reinterpret_cast<const u32x4*>(wbase + (long)i * 1024 + lane_off);
    };
    u32x4 ring[ML_PF];

    const u32x4* ylds = reinterpret_cast<const u32x4*>(smem) + lane;
    u32x4* hlds = reinterpret_cast<u32x4*>(smem + ML_Y_BYTES) + lane;
    auto y_frags = [&](int s, u32x4 (&dst)[2]) {
        if ((ML_ABL & 8) && s > 1) return;
#pragma unroll
        for (int b = 0; b < 2; ++b) dst[b] = ylds[(s * 2 + b) * (ML_YP / 16)];
    };
    f32x16 acc2[ML_NB][2];  // [column block of this wave][token block]: out^T, 192 accumulators (AGPRs)

    // ---- prologue: LayerNorm of this wave's 16 tokens -> LDS as B fragments.  Fragment (s, fb) = k-step s (16 channels) x
    // token block fb (32 tokens) at [(2 s + fb)][lane][16 B]; lane l supplies token 32 fb + (l & 31), channels
    // 16 s + 8 (l >> 5) .. + 7.  A lane owns channels 256 k + 4 l .. + 3 (k = 0..2) of every row.
    if constexpr (!OPROJ) {
        float4 v[16][3];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long row = (long)row0 + 16 * w + i;
            const bool ok = row < M && !(ML_ABL & 32);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                v[i][k] = ok ? *reinterpret_cast<const float4*>(x + row * ML_D + 256 * k + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float4 gw[3], gb[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            gw[k] = *reinterpret_cast<const float4*>(ln.w + 256 * k + 4 * lane);
            gb[k] = *reinterpret_cast<const float4*>(ln.b + 256 * k + 4 * lane);
        }
#pragma unroll
        for (int i0 = 0; i0 < 16; i0 += 4) {
            if (i0 == 12) {
                // the first weight fragments are requested once three quarters of the rows have left their registers (all 16 rows and
                // the ring together do not fit): their latency overlaps the second half and the other waves' tails
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < ML_PF; ++i) ring[i] = wfrag(i);
                __builtin_amdgcn_sched_barrier(0);
            }
            float s[4], q[4], mean[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                s[u] = 0.f;
#pragma unroll
                for (int k = 0; k < 3; ++k) s[u] += (v[i0 + u][k].x + v[i0 + u][k].y) + (v[i0 + u][k].z + v[i0 + u][k].w);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) mean[u] = wave_sum_dpp(s[u]) / (float)ML_D;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                q[u] = 0.f;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float a = v[i0 + u][k].x - mean[u], b_ = v[i0 + u][k].y - mean[u], c = v[i0 + u][k].z - mean[u],
                                d = v[i0 + u][k].w - mean[u];
                    q[u] += (a * a + b_ * b_) + (c * c + d * d);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float rstd = 1.0f / sqrtf(wave_sum_dpp(q[u]) / (float)ML_D + eps);
                const int tok = 16 * w + i0 + u;          // token inside the tile
                const int fb = tok >> 5, fl = tok & 31;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float4 t = v[i0 + u][k];
                    const float o0 = (t.x - mean[u]) * rstd * gw[k].x + gb[k].x, o1 = (t.y - mean[u]) * rstd * gw[k].y + gb[k].y;
                    const float o2 = (t.z - mean[u]) * rstd * gw[k].z + gb[k].z, o3 = (t.w - mean[u]) * rstd * gw[k].w + gb[k].w;
                    // channels c = 256 k + 4 l .. + 3 -> fragment (s = c / 16, fb), lane' = 32 ((c % 16) / 8) + fl, byte (c % 8) * 2
                    const int s_ = 16 * k + (lane >> 2);
                    const int off = (s_ * 2 + fb) * ML_YP + (32 * ((lane >> 1) & 1) + fl) * 16 + (lane & 1) * 8;
                    *reinterpret_cast<uint2*>(smem + off) = make_uint2(bf16_pack2(o0, o1), bf16_pack2(o2, o3));
                }
            }
        }
        __syncthreads();
    #pragma unroll
        for (int a = 0; a < ML_NB; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc2[a][b][r] = 0.f;
    } else {
        // ---- OPROJ prologue.  (1) attention tile -> LDS as B fragments by DMA: fragment (s, fb) = k-step s (16 channels) x
        // token block fb at [(2 s + fb) * ML_YP]; lane l supplies token 32 fb + (l & 31), channels 16 s + 8 (l >> 5) .. + 7
        const unsigned lds0 = lds_addr_of(smem);
#pragma unroll 4
        for (int i = 0; i < 2 * ML_KS1 / 4; ++i) {
            const int frag = w * (2 * ML_KS1 / 4) + i;
            const int s_ = frag >> 1, fb = frag & 1;
            int row = row0 + 32 * fb + lf;
            row = row < M ? row : M - 1;  // rows beyond M are computed on a copy of the last row and never stored
            glds16(att + (long)row * ML_D + 16 * s_ + 8 * lh, lds0 + frag * ML_YP);
        }
        // (2) the accumulators start at the residual stream + out-proj bias, in the accumulator layout: register r = 4 g + e
        // of tile (n, fb) in lane (lf, lh) is token 32 fb + lf, column 192 w + 32 n + 8 g + 4 lh + e
#pragma unroll
        for (int n = 0; n < ML_NB; ++n) {
            if (n == ML_NB / 2) __builtin_amdgcn_sched_barrier(0);  // two halves of 24 loads: all 48 in flight + the ring spill
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = 192 * w + 32 * n + 8 * g + 4 * lh;
                const float4 bv = *reinterpret_cast<const float4*>(bo + col);
#pragma unroll
                for (int fb = 0; fb < 2; ++fb) {
                    const long row = (long)row0 + 32 * fb + lf;
                    const float4 xv = (row < M && !(ML_ABL & 32)) ? *reinterpret_cast<const float4*>(x + row * ML_D + col)
                                                                   : make_float4(0.f, 0.f, 0.f, 0.f);
                    acc2[n][fb][4 * g] = xv.x + bv.x; acc2[n][fb][4 * g + 1] = xv.y + bv.y;
                    acc2[n][fb][4 * g + 2] = xv.z + bv.z; acc2[n][fb][4 * g + 3] = xv.w + bv.w;
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < ML_PF; ++i) ring[i] = wfrag(i);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if constexpr (F16) {
            // the attention tile arrived as bf16: to f16 in place (exact: 8 significand bits into 11; saturating).  A lane rewrites the
            // 16 bytes it read: 24 fragments per wave
#pragma unroll 4
            for (int i = 0; i < 2 * ML_KS1 / 4; ++i) {
                u32x4* fp = reinterpret_cast<u32x4*>(smem + (w * (2 * ML_KS1 / 4) + i) * ML_YP) + lane;
                const u32x4 v = *fp;
                u32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = ml_pack_x2<true>(__uint_as_float(v[e] << 16), __uint_as_float(v[e] & 0xffff0000u));
                *fp = o;
            }
            __syncthreads();
        }
        // (3) x' = x + att Wo^T + bo: 48 k-steps of 12 MFMAs over the attention image
        {
            u32x4 aA[2], aB[2];
            y_frags(0, aA);
            auto step = [&](int s_, u32x4 (&cur)[2], u32x4 (&nxt)[2]) {
                if (s_ + 1 < ML_KS1) y_frags(s_ + 1, nxt);
#pragma unroll
                for (int n = 0; n < ML_NB; ++n) {
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc2[n][b] = mfma32<F16>(ring[(s_ * ML_NB + n) % ML_PF], cur[b], acc2[n][b]);
                    ring[(s_ * ML_NB + n) % ML_PF] = wfrag(s_ * ML_NB + n + ML_PF);
                }
                __builtin_amdgcn_sched_barrier(0);
            };
#pragma unroll
            for (int s_ = 0; s_ < ML_KS1; s_ += 2) {
                step(s_, aA, aB);
                step(s_ + 1, aB, aA);
            }
            wbase += ML_P0 * 1024;
        }
        // (4) LayerNorm(x') in the accumulator layout.  A token's 768 values sit in 2 lanes (lh) of each of the 4 waves:
        // two-pass statistics (mean, then squared deviations), partial sums exchanged through LDS (the H buffer is free)
        float* red = reinterpret_cast<float*>(smem + ML_Y_BYTES);
        float sm[2], mean[2], rstd[2];
#pragma unroll
        for (int fb = 0; fb < 2; ++fb) {
            float t = 0.f;
#pragma unroll
            for (int n = 0; n < ML_NB; ++n)
#pragma unroll
                for (int r = 0; r < 16; r += 4) t += (acc2[n][fb][r] + acc2[n][fb][r + 1]) + (acc2[n][fb][r + 2] + acc2[n][fb][r + 3]);
            sm[fb] = t + __shfl_xor(t, 32);
        }
        if (lh == 0) { red[w * 64 + lf] = sm[0]; red[w * 64 + 32 + lf] = sm[1]; }
        __syncthreads();  // (every wave has also finished reading the attention image)
#pragma unroll
        for (int fb = 0; fb < 2; ++fb) {
            const int tk = 32 * fb + lf;
            mean[fb] = ((red[tk] + red[64 + tk]) + (red[128 + tk] + red[192 + tk])) / (float)ML_D;
            float t = 0.f;
#pragma unroll
            for (int n = 0; n < ML_NB; ++n)
#pragma unroll
                for (int r = 0; r < 16; r += 4) {
                    const float a0 = acc2[n][fb][r] - mean[fb], a1 = acc2[n][fb][r + 1] - mean[fb], a2 = acc2[n][fb][r + 2] - mean[fb],
                                a3 = acc2[n][fb][r + 3] - mean[fb];
                    t += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
                }
            sm[fb] = t + __shfl_xor(t, 32);
        }
        if (lh == 0) { red[256 + w * 64 + lf] = sm[0]; red[256 + w * 64 + 32 + lf] = sm[1]; }
        __syncthreads();
#pragma unroll
        for (int fb = 0; fb < 2; ++fb) {
            const int tk = 256 + 32 * fb + lf;
            rstd[fb] = 1.0f / sqrtf(((red[tk] + red[64 + tk]) + (red[128 + tk] + red[192 + tk])) / (float)ML_D + eps);
        }
        // (5) y = LayerNorm(x') as bf16 B fragments over the attention image: registers 8 t .. 8 t + 7 of tile (n, fb), rows
        // pairwise converted, are the fragment of k-step 12 w + 2 n + t (W1 is packed in that channel order)
        float amax8 = 0.f;
        (void)amax8;
#pragma unroll
        for (int n = 0; n < ML_NB; ++n) {
            float4 gw[4], gb[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                gw[g] = *reinterpret_cast<const float4*>(ln.w + 192 * w + 32 * n + 8 * g + 4 * lh);
                gb[g] = *reinterpret_cast<const float4*>(ln.b + 192 * w + 32 * n + 8 * g + 4 * lh);
            }
#pragma unroll
            for (int fb = 0; fb < 2; ++fb)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    float o[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int r = 8 * t + e;
                        o[e] = (acc2[n][fb][r] - mean[fb]) * rstd[fb] * reinterpret_cast<const float*>(&gw[r >> 2])[r & 3] +
                               reinterpret_cast<const float*>(&gb[r >> 2])[r & 3];
                    }
                    if constexpr (F8) {
                        // e4m3 at the activation scale, B fragments of the 16 x 16 x 128 MFMA: fragment (s = c / 128, tb = token / 16)
                        // = 2 KiB as two lane-linear halves; lane' = 16 ((c % 128) / 32) + token % 16 holds 32 channels
                        // (tokens beyond M run on x = 0 and a copy of the last row's attention and are never stored: what they
                        // convert is not an activation of the call and must not reach the clip counter)
                        float am = 0.f;
#pragma unroll
                        for (int hq = 0; hq < 2; ++hq) {
                            const int c = 192 * w + 32 * n + 8 * (2 * t + hq) + 4 * lh;
                            const int tok = 32 * fb + lf;
                            const int off = (((c >> 7) * 4 + (tok >> 4)) * 2 + ((c & 31) >> 4)) * 1024 +
                                            (16 * ((c & 127) >> 5) + (tok & 15)) * 16 + (c & 15);
                            *reinterpret_cast<unsigned*>(smem + off) =
                                fp8_pack4(o[4 * hq] * SWC_FP8_ACT_SCALE, o[4 * hq + 1] * SWC_FP8_ACT_SCALE, o[4 * hq + 2] * SWC_FP8_ACT_SCALE,
                                          o[4 * hq + 3] * SWC_FP8_ACT_SCALE, am);
                        }
                        if (row0 + 32 * fb + lf < M) amax8 = fmaxf(amax8, am);
                    } else {
                        if constexpr (F16)
                            *reinterpret_cast<u32x4*>(smem + (2 * (12 * w + 2 * n + t) + fb) * ML_YP + lane * 16) =
                                (u32x4){ml_pack_x2<true>(o[0], o[1]), ml_pack_x2<true>(o[2], o[3]), ml_pack_x2<true>(o[4], o[5]),
                                        ml_pack_x2<true>(o[6], o[7])};
                        else
                            *reinterpret_cast<u32x4*>(smem + (2 * (12 * w + 2 * n + t) + fb) * ML_YP + lane * 16) =
                                (u32x4){bf16_pack2(o[0], o[1]), bf16_pack2(o[2], o[3]), bf16_pack2(o[4], o[5]), bf16_pack2(o[6], o[7])};
                    }
                }
        }
        if constexpr (F8) sat_commit(sat, 1, amax8, SWC_FP8_LIMIT);
        __syncthreads();
    }
    f32x16 acc1[2][2];  // [hidden block][token block]: H^T of this wave's 64 hidden rows

    auto h_frags = [&](int q, u32x4 (&dst)[2]) {
        if ((ML_ABL & 8) && q > 1) return;
#pragma unroll
        for (int b = 0; b < 2; ++b) dst[b] = hlds[(q * 2 + b) * 64];
    };
    // b1 of this wave's 64 hidden rows, one slice ahead: register r = 4 g + e of a lane in half lh belongs to row
    // 8 g + 4 lh + e of its 32-row block
    float4 bias_nx[2][4];
    auto load_bias = [&](int j) __attribute__((always_inline)) {
#pragma unroll
        for (int hb = 0; hb < 2; ++hb)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                bias_nx[hb][g] = *reinterpret_cast<const float4*>(b1 + (long)j * ML_SL + 64 * w + 32 * hb + 8 * g + 4 * lh);
    };
    load_bias(0);
    // Every k-step is its own scheduling region (sched_barrier at its end): it issues the LDS reads of the NEXT step's B
    // fragments, its MFMAs and the refill of the ring slots it consumed (see swc_convnext.hip for what hipcc does otherwise)
    auto gemm1 = [&](int j) __attribute__((always_inline)) {
#pragma unroll
        for (int hb = 0; hb < 2; ++hb)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc1[hb][b][r] = reinterpret_cast<const float*>(&bias_nx[hb][r >> 2])[r & 3];
        load_bias(j + 1 < NS ? j + 1 : 0);
        u32x4 yA[2], yB[2];
        y_frags(0, yA);
        // fully unrolled: the ring must not become loop-carried (swc_convnext.hip)
#pragma unroll
        for (int s = 0; s < ML_KS1; s += 2) {
            {
                y_frags(s + 1, yB);
                ml_mfma2x2_vgpr<F16>(ring[(2 * s) % ML_PF], ring[(2 * s + 1) % ML_PF], yA[0], yA[1], acc1[0][0], acc1[0][1], acc1[1][0],
                                acc1[1][1]);
                ring[(2 * s) % ML_PF] = wfrag(2 * s + ML_PF);
                ring[(2 * s + 1) % ML_PF] = wfrag(2 * s + 1 + ML_PF);
                __builtin_amdgcn_sched_barrier(0);
            }
            {
                y_frags((s + 2) % ML_KS1, yA);  // the last step re-reads step 0 (harmless)
                ml_mfma2x2_vgpr<F16>(ring[(2 * s + 2) % ML_PF], ring[(2 * s + 3) % ML_PF], yB[0], yB[1], acc1[0][0], acc1[0][1],
                                acc1[1][0], acc1[1][1]);
                ring[(2 * s + 2) % ML_PF] = wfrag(2 * s + 2 + ML_PF);
                ring[(2 * s + 3) % ML_PF] = wfrag(2 * s + 3 + ML_PF);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // MFMA results in VGPRs -> VALU readers: the wait states hipcc would insert for its own MFMAs
        asm volatile("s_nop 15\n\ts_nop 7" : "+v"(acc1[0][0]), "+v"(acc1[0][1]), "+v"(acc1[1][0]), "+v"(acc1[1][1]));
        wbase += ML_FPP * 1024;
    };
    // GELU of accumulator registers 8 t + 4 h .. + 3 of tile (hb, b) -> two packed dwords of B fragment t, kept IN PLACE:
    // they replace registers 4 t + 2 h, + 1 of the same tile (already consumed when the halves run in order)
    auto gelu_half = [&](int hb, int b, int t, int h) __attribute__((always_inline)) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (ML_ABL & 2) ? acc1[hb][b][8 * t + 4 * h + e] : gelu_fast(acc1[hb][b][8 * t + 4 * h + e]);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc1[hb][b][4 * t + 2 * h + i] = __uint_as_float(ml_pack_x2<F16>(v[2 * i], v[2 * i + 1]));
    };
    auto store_h = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int hb = 0; hb < 2; ++hb)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    hlds[((4 * w + 2 * hb + t) * 2 + b) * 64] =
                        (u32x4){__float_as_uint(acc1[hb][b][4 * t]), __float_as_uint(acc1[hb][b][4 * t + 1]),
                                __float_as_uint(acc1[hb][b][4 * t + 2]), __float_as_uint(acc1[hb][b][4 * t + 3])};
    };
    // GEMM2 over the slice whose H^T is in LDS; `with_gelu`: the GELU of the NEXT slice (acc1) rides along, half a
    // fragment per k-step, in the same scheduling region as that step's 12 MFMAs
    // ---- fp8 fc1 (F8): GEMM1 on the block-scaled MFMA.  Wave w: 4 hidden tiles of 16 x 4 token tiles of 16, 6 k-steps of 128
    f32x4 a8[4][4];   // [hidden tile][token tile]: lane (tok = l & 15, g4 = l >> 4) holds hidden rows 16 ht + 4 g4 + r, r = 0..3
    float4 bias8[4];  // b1 of those rows, loaded at the start of GEMM1(j), consumed by the GELU that rides on GEMM2(j - 1)
    auto gemm1_f8 = [&](int j) __attribute__((always_inline)) {
        if constexpr (F8) {
            const int g4 = lane >> 4;
#pragma unroll
            for (int ht = 0; ht < 4; ++ht) {
                bias8[ht] = *reinterpret_cast<const float4*>(b1 + (long)j * ML_SL + 64 * w + 16 * ht + 4 * g4);
#pragma unroll
                for (int tb = 0; tb < 4; ++tb) a8[ht][tb] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            const u32x4* y8 = reinterpret_cast<const u32x4*>(smem) + lane;
            auto yfr = [&](int s_, i32x8 (&dst)[4]) {
#pragma unroll
                for (int tb = 0; tb < 4; ++tb) {
                    const u32x4 lo = y8[((s_ * 4 + tb) * 2) * 64], hi = y8[((s_ * 4 + tb) * 2 + 1) * 64];
                    dst[tb] = (i32x8){(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
                }
            };
            i32x8 yA[4], yB[4];
            yfr(0, yA);
            auto step8 = [&](int s_, i32x8 (&cur)[4], i32x8 (&nxt)[4]) {
                if (s_ + 1 < ML_D / 128) yfr(s_ + 1, nxt);
#pragma unroll
                for (int ht = 0; ht < 4; ++ht) {
                    const u32x4 lo = ring[(8 * s_ + 2 * ht) % ML_PF], hi = ring[(8 * s_ + 2 * ht + 1) % ML_PF];
                    const i32x8 wa = (i32x8){(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
                    ml_mfma8_1x4_vgpr(wa, cur[0], cur[1], cur[2], cur[3], a8[ht][0], a8[ht][1], a8[ht][2], a8[ht][3], 0x7f7f7f7fu);
                    ring[(8 * s_ + 2 * ht) % ML_PF] = wfrag(8 * s_ + 2 * ht + ML_PF);
                    ring[(8 * s_ + 2 * ht + 1) % ML_PF] = wfrag(8 * s_ + 2 * ht + 1 + ML_PF);
                }
                __builtin_amdgcn_sched_barrier(0);
            };
#pragma unroll
            for (int s_ = 0; s_ < ML_D / 128; s_ += 2) {
                step8(s_, yA, yB);
                step8(s_ + 1, yB, yA);
            }
            // MFMA results in VGPRs -> VALU readers: the wait states hipcc would insert for its own MFMAs
#pragma unroll
            for (int ht = 0; ht < 4; ++ht) asm volatile("s_nop 15\n\ts_nop 7" : "+v"(a8[ht][0]), "+v"(a8[ht][1]), "+v"(a8[ht][2]), "+v"(a8[ht][3]));
            wbase += G1F * 1024;
        }
    };
    // bias + GELU of one 16 x 16 tile -> two packed dwords (4 bf16), kept in place of the tile's first two registers
    auto gelu_tile8 = [&](int q) __attribute__((always_inline)) {
        if constexpr (F8) {
            const int ht = q >> 2, tb = q & 3;
            const float* bb = reinterpret_cast<const float*>(&bias8[ht]);
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = gelu_fast(fmaf(a8[ht][tb][r], alpha1, bb[r]));
            a8[ht][tb][0] = __uint_as_float(bf16_pack2(v[0], v[1]));
            a8[ht][tb][1] = __uint_as_float(bf16_pack2(v[2], v[3]));
        }
    };
    // H^T -> the LDS exchange buffer in the B-fragment layout of GEMM2 (32 x 32 x 16): k-step q = 4 w + ht, token block fb,
    // lane' = 32 (hidden % 16 / 8) + token % 32, 4 consecutive hidden values = 8 bytes
    auto store_h8 = [&]() __attribute__((always_inline)) {
        if constexpr (F8) {
            const int g4 = lane >> 4, tok = lane & 15;
#pragma unroll
            for (int ht = 0; ht < 4; ++ht)
#pragma unroll
                for (int tb = 0; tb < 4; ++tb) {
                    const int off = ((4 * w + ht) * 2 + (tb >> 1)) * 1024 + (32 * (g4 >> 1) + 16 * (tb & 1) + tok) * 16 + 8 * (g4 & 1);
                    *reinterpret_cast<uint2*>(smem + ML_Y_BYTES + off) =
                        make_uint2(__float_as_uint(a8[ht][tb][0]), __float_as_uint(a8[ht][tb][1]));
                }
        }
    };

    auto gemm2 = [&](auto with_gelu) __attribute__((always_inline)) {
        u32x4 hA[2], hB[2];
        h_frags(0, hA);
        auto step = [&](int q, u32x4 (&cur)[2], u32x4 (&nxt)[2]) {
            if (q + 1 < ML_KS2) h_frags(q + 1, nxt);
#pragma unroll
            for (int n = 0; n < ML_NB; ++n) {
#pragma unroll
                for (int b = 0; b < 2; ++b) acc2[n][b] = mfma32<F16>(ring[(q * ML_NB + n) % ML_PF], cur[b], acc2[n][b]);
                ring[(q * ML_NB + n) % ML_PF] = wfrag(q * ML_NB + n + ML_PF);
            }
            if constexpr (decltype(with_gelu)::value) {
                if constexpr (F8) gelu_tile8(q);
                else gelu_half(q >> 3, (q >> 2) & 1, (q >> 1) & 1, q & 1);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
#pragma unroll
        for (int q = 0; q < ML_KS2; q += 2) {
            step(q, hA, hB);
            step(q + 1, hB, hA);
        }
        wbase += ML_FPP * 1024;
    };

    // ---- pipeline over the hidden slices
    auto g1 = [&](int j) __attribute__((always_inline)) {
        if constexpr (F8) gemm1_f8(j);
        else gemm1(j);
    };
    auto sh = [&]() __attribute__((always_inline)) {
        if constexpr (F8) store_h8();
        else store_h();
    };
    g1(0);
#pragma unroll
    for (int q = 0; q < ML_KS2; ++q) {
        if constexpr (F8) gelu_tile8(q);
        else gelu_half(q >> 3, (q >> 2) & 1, (q >> 1) & 1, q & 1);
    }
    sh();
    __syncthreads();
    for (int j = 1; j < NS; ++j) {
        g1(j);
        gemm2(std::true_type{});
        if (!(ML_ABL & 1)) __syncthreads();  // every wave has read H_{j-1}
        sh();
        if (!(ML_ABL & 1)) __syncthreads();  // H_j visible
    }
    gemm2(std::false_type{});
    __syncthreads();  // LDS is free: the epilogue re-uses it

    if (ML_ABL & 16) {  // keep the accumulators alive, store nothing
        float keep = 0.f;
#pragma unroll
        for (int a = 0; a < ML_NB; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) keep += acc2[a][b][0] + acc2[a][b][7];
        if (keep == 12345.678f) xo[0] = keep;
        return;
    }
    // ---- epilogue: x_out[row][n] = x[row][n] + out[row][n] + b2[n] via a transposed f32 image [32 tokens][772]; the wave
    // that owns a row then holds all 768 values of it: LayerNorm_next on the spot
    float* tl = reinterpret_cast<float*>(smem);
    float4 c4[3], nw[3], nb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c4[k] = *reinterpret_cast<const float4*>(b2 + 256 * k + 4 * lane);
        if (y_next) {
            nw[k] = *reinterpret_cast<const float4*>(nln.w + 256 * k + 4 * lane);
            nb[k] = *reinterpret_cast<const float4*>(nln.b + 256 * k + 4 * lane);
        }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        // the residual rows of this pass first: 24 independent 16-byte loads per lane, in flight across the LDS round trip
        float4 rr[8][3];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const long row = (long)row0 + 32 * p + 8 * w + i;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                rr[i][k] = (!OPROJ && row < M) ? *reinterpret_cast<const float4*>(x + row * ML_D + 256 * k + 4 * lane)
                                                : make_float4(0.f, 0.f, 0.f, 0.f);  // (OPROJ: the accumulators hold x' already)
        }
#pragma unroll
        for (int n = 0; n < ML_NB; ++n)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x16& t = acc2[n][p];
                *reinterpret_cast<float4*>(tl + lf * ML_TLD + 32 * (ML_NB * w + n) + 8 * g + 4 * lh) =
                    make_float4(t[4 * g], t[4 * g + 1], t[4 * g + 2], t[4 * g + 3]);
            }
        __syncthreads();
#pragma unroll
        for (int i0 = 0; i0 < 8; i0 += 4) {
            float4 o[4][3];
            float s[4], q[4], mean[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int fl = 8 * w + i0 + u;
                const long row = (long)row0 + 32 * p + fl;
                s[u] = 0.f;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float4 v = *reinterpret_cast<const float4*>(tl + fl * ML_TLD + 256 * k + 4 * lane);
                    float4 r = rr[i0 + u][k];
                    r.x += v.x + c4[k].x; r.y += v.y + c4[k].y; r.z += v.z + c4[k].z; r.w += v.w + c4[k].w;
                    o[u][k] = r;
                    if (row < M) *reinterpret_cast<float4*>(xo + row * ML_D + 256 * k + 4 * lane) = r;
                    s[u] += (r.x + r.y) + (r.z + r.w);
                }
            }
            if (y_next) {
#pragma unroll
                for (int u = 0; u < 4; ++u) mean[u] = wave_sum_dpp(s[u]) / (float)ML_D;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    q[u] = 0.f;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const float a = o[u][k].x - mean[u], b_ = o[u][k].y - mean[u], c = o[u][k].z - mean[u], d = o[u][k].w - mean[u];
                        q[u] += (a * a + b_ * b_) + (c * c + d * d);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float rstd = 1.0f / sqrtf(wave_sum_dpp(q[u]) / (float)ML_D + eps);
                    const long row = (long)row0 + 32 * p + 8 * w + i0 + u;
                    if (row < M) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const float4 t = o[u][k];
                            const float y0 = (t.x - mean[u]) * rstd * nw[k].x + nb[k].x, y1 = (t.y - mean[u]) * rstd * nw[k].y + nb[k].y;
                            const float y2 = (t.z - mean[u]) * rstd * nw[k].z + nb[k].z, y3 = (t.w - mean[u]) * rstd * nw[k].w + nb[k].w;
                            *reinterpret_cast<uint2*>(y_next + row * ML_D + 256 * k + 4 * lane) =
                                make_uint2(bf16_pack2(y0, y1), bf16_pack2(y2, y3));
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

// One thread per 16-byte chunk of the packed stream.  Stream of wave w: [with wo: the out-proj phase P0 of ML_P0 fragments,]
// then phases of 96 fragments in the order of consumption G1(0), G1(1), G2(0), G1(2), G2(1), ..., G1(NS-1), G2(NS-2),
// G2(NS-1), then ML_PF zero fragments (read ahead, never used).
//   P0,    fragment i: k-step s = i / 6, column block n = i % 6: Wo rows 192 w + 32 n + (lane & 31), columns
//                      16 s + 8 (lane >> 5) .. + 7 (the attention tile arrives by DMA in natural channel order)
//   G1(j), fragment i: k-step s = i / 2, hidden block hb = i % 2: W1 rows 256 j + 64 w + 32 hb + (lane & 31), columns
//                      16 s + 8 (lane >> 5) .. + 7, or — with wo, where y comes out of the accumulators —
//                      16 s + 4 (lane >> 5) + {0..3, 8..11}
//   G2(j), fragment i: k-step q = i / 6, column block n = i % 6: W2 rows 192 w + 32 n + (lane & 31), hidden values
//                      256 j + 16 q + 4 (lane >> 5) + {0..3, 8..11}: the order GEMM1's accumulators convert in place
__global__ void mlp_pack_kernel(const bf16_t* __restrict__ wo, const void* __restrict__ w1v, const bf16_t* __restrict__ w2,
                                uint4* __restrict__ out, int NS, int f8) {
    // f8: w1 is e4m3 bytes [F][D]; a GEMM1 phase is then 48 entries: entry i = k-step s = i / 8 (128 columns), hidden tile
    // ht = (i % 8) / 2 (16 rows), half h = i % 2: W1 rows 256 j + 64 w + 16 ht + (lane & 15), columns 128 s + 32 (lane >> 4) + 16 h
    // .. + 15; GEMM2's hidden values are in natural order (H is written to LDS fragment by fragment, not converted in place)
    const bf16_t* w1 = reinterpret_cast<const bf16_t*>(w1v);
    const unsigned char* w1q = reinterpret_cast<const unsigned char*>(w1v);
    const long p0 = wo ? ML_P0 : 0;
    const int g1f = f8 ? ML_FPP / 2 : ML_FPP;
    const long per_slice = g1f + ML_FPP;
    const long per_wave = p0 + (long)NS * per_slice + ML_PF;
    const long total = 4 * per_wave * 64;
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const int lane = (int)(id & 63);
    const long f_all = id >> 6;
    const int w = (int)(f_all / per_wave);
    long f = f_all - (long)w * per_wave;
    const int lf = lane & 31, lh = lane >> 5;
    const long F = (long)NS * ML_SL;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (f < p0) {
        const int s = (int)(f / ML_NB), n = (int)(f % ML_NB);
        v = *reinterpret_cast<const uint4*>(wo + (long)(192 * w + 32 * n + lf) * ML_D + 16 * s + 8 * lh);
    } else if (f - p0 < (long)NS * per_slice) {
        f -= p0;
        // consumption order: G1(0), G1(1), G2(0), G1(2), G2(1), ..., G1(NS-1), G2(NS-2), G2(NS-1)
        int j, i;
        bool is_g1;
        if (f < g1f) { is_g1 = true; j = 0; i = (int)f; }
        else {
            const long r = f - g1f;                       // pairs (G1(k), G2(k-1)) for k = 1 .. NS-1, then G2(NS-1)
            const long pair = r / per_slice, o = r % per_slice;
            if (pair < NS - 1) {
                if (o < g1f) { is_g1 = true; j = (int)pair + 1; i = (int)o; }
                else { is_g1 = false; j = (int)pair; i = (int)(o - g1f); }
            } else { is_g1 = false; j = NS - 1; i = (int)(r - (long)(NS - 1) * per_slice); }
        }
        if (is_g1 && f8) {
            const int s = i >> 3, ht = (i >> 1) & 3, h = i & 1;
            const long row = (long)j * ML_SL + 64 * w + 16 * ht + (lane & 15);
            v = *reinterpret_cast<const uint4*>(w1q + row * ML_D + 128 * s + 32 * (lane >> 4) + 16 * h);
        } else if (is_g1) {
            const int s = i >> 1, hb = i & 1;
            const long row = (long)j * ML_SL + 64 * w + 32 * hb + lf;  // hidden row
            if (wo) {
                const uint2 lo = *reinterpret_cast<const uint2*>(w1 + row * ML_D + 16 * s + 4 * lh);
                const uint2 hi = *reinterpret_cast<const uint2*>(w1 + row * ML_D + 16 * s + 4 * lh + 8);
                v = make_uint4(lo.x, lo.y, hi.x, hi.y);
            } else {
                v = *reinterpret_cast<const uint4*>(w1 + row * ML_D + 16 * s + 8 * lh);
            }
        } else {
            const int q = i / ML_NB, n = i % ML_NB;
            const long nrow = 192 * w + 32 * n + lf;  // output column = row of W2
            if (f8) {
                v = *reinterpret_cast<const uint4*>(w2 + nrow * F + (long)j * ML_SL + 16 * q + 8 * lh);
            } else {
                const long hid = (long)j * ML_SL + 16 * q + 4 * lh;  // elements jj: hid + 8 (jj >> 2) + (jj & 3)
                const uint2 lo = *reinterpret_cast<const uint2*>(w2 + nrow * F + hid);
                const uint2 hi = *reinterpret_cast<const uint2*>(w2 + nrow * F + hid + 8);
                v = make_uint4(lo.x, lo.y, hi.x, hi.y);
            }
        }
    }
    out[id] = v;
}

int ml_pack(const void* wo, const void* w1, const void* w2, void* stream_out, int32_t D, int32_t F, void* stream, const char* who,
            int f8 = 0) {
    SWC_CHECK_ARG(w1 && w2 && stream_out, "%s: null pointer", who);
    SWC_CHECK_ARG(D == ML_D && F > 0 && F % ML_SL == 0, "%s: needs D = %d and F a multiple of %d (D=%d F=%d)", who, ML_D, ML_SL, D, F);
    SWC_CHECK_ARG(aligned16(wo) && aligned16(w1) && aligned16(w2) && aligned16(stream_out), "%s: unaligned", who);
    const int NS = F / ML_SL;
    const long total = 4L * ((wo ? ML_P0 : 0) + (long)NS * ((f8 ? ML_FPP / 2 : ML_FPP) + ML_FPP) + ML_PF) * 64;
    hipLaunchKernelGGL(mlp_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)wo, w1, (const bf16_t*)w2, (uint4*)stream_out, NS, f8);
    SWC_CHECK_LAUNCH(who);
    return SWC_OK;
}

}  // namespace

extern "C" int64_t swc_mlp_stream_bytes(int32_t D, int32_t F) {
    if (D != ML_D || F <= 0 || F % ML_SL != 0) return 0;
    return 4L * ((long)(F / ML_SL) * (2 * ML_FPP) + ML_PF) * 1024;
}

extern "C" int swc_mlp_pack(const void* w1, const void* w2, void* stream_out, int32_t D, int32_t F, void* stream) {
    return ml_pack(nullptr, w1, w2, stream_out, D, F, stream, "swc_mlp_pack");
}

extern "C" int swc_mlp_block(const float* x, float* x_out, const float* ln_w, const float* ln_b, float eps,
                             const void* w_stream, const float* b1, const float* b2, const float* next_ln_w,
                             const float* next_ln_b, void* y_next, int32_t M, int32_t D, int32_t F, void* stream) {
    SWC_CHECK_ARG(x && x_out && ln_w && ln_b && w_stream && b1 && b2, "swc_mlp_block: null pointer");
    SWC_CHECK_ARG(!y_next || (next_ln_w && next_ln_b), "swc_mlp_block: y_next needs next_ln_w / next_ln_b");
    SWC_CHECK_ARG(D == ML_D && F > 0 && F % ML_SL == 0, "swc_mlp_block: needs D = %d and F a multiple of %d (D=%d F=%d)", ML_D,
                  ML_SL, D, F);
    SWC_CHECK_ARG(M >= 0, "swc_mlp_block: bad M");
    SWC_CHECK_ARG(aligned16(x) && aligned16(x_out) && aligned16(ln_w) && aligned16(ln_b) && aligned16(w_stream) && aligned16(b1) &&
                      aligned16(b2) && aligned16(next_ln_w) && aligned16(next_ln_b) && aligned16(y_next),
                  "swc_mlp_block: unaligned");
    if (M == 0) return SWC_OK;
    SWC_ENABLE_LDS((mlp_block_kernel<false, false>), ML_LDS, "swc_mlp_block");
    const unsigned grid = (unsigned)((M + ML_BM - 1) / ML_BM);
    hipLaunchKernelGGL((mlp_block_kernel<false, false>), dim3(grid), dim3(256), ML_LDS, (hipStream_t)stream, x, x_out, MlNorm{ln_w, ln_b},
                       eps, (const u32x4*)w_stream, b1, b2, MlNorm{next_ln_w, next_ln_b}, (bf16_t*)y_next, M, F / ML_SL,
                       (const bf16_t*)nullptr, (const float*)nullptr, 1.0f, (unsigned*)nullptr);
    SWC_CHECK_LAUNCH("swc_mlp_block");
    return SWC_OK;
}

extern "C" int64_t swc_layer_tail_stream_bytes(int32_t D, int32_t F, int32_t fc1_dtype) {
    if (D != ML_D || F <= 0 || F % ML_SL != 0 || (fc1_dtype != SWC_BF16 && fc1_dtype != SWC_FP8)) return 0;
    return 4L * (ML_P0 + (long)(F / ML_SL) * ((fc1_dtype == SWC_FP8 ? ML_FPP / 2 : ML_FPP) + ML_FPP) + ML_PF) * 1024;
}

extern "C" int swc_layer_tail_pack(const void* wo, const void* w1, const void* w2, void* stream_out, int32_t D, int32_t F,
                                   int32_t fc1_dtype, void* stream) {
    SWC_CHECK_ARG(wo, "swc_layer_tail_pack: null pointer");
    SWC_CHECK_ARG(fc1_dtype == SWC_BF16 || fc1_dtype == SWC_FP8, "swc_layer_tail_pack: fc1_dtype must be BF16 or FP8");
    return ml_pack(wo, w1, w2, stream_out, D, F, stream, "swc_layer_tail_pack", fc1_dtype == SWC_FP8);
}

extern "C" int swc_layer_tail(const void* attn, const float* x, float* x_out, const void* w_stream, const float* bo,
                              const float* ln_w, const float* ln_b, float eps, const float* b1, const float* b2,
                              const float* next_ln_w, const float* next_ln_b, void* y_next, int32_t M, int32_t D, int32_t F,
                              int32_t fc1_dtype, float fc1_alpha, int32_t operand_dtype, void* stream) {
    SWC_CHECK_ARG(operand_dtype == SWC_BF16 || (operand_dtype == SWC_F16 && fc1_dtype == SWC_BF16),
                  "swc_layer_tail: operand_dtype must be BF16, or F16 with a 16-bit fc1");
    SWC_CHECK_ARG(attn && x && x_out && bo && ln_w && ln_b && w_stream && b1 && b2, "swc_layer_tail: null pointer");
    SWC_CHECK_ARG(!y_next || (next_ln_w && next_ln_b), "swc_layer_tail: y_next needs next_ln_w / next_ln_b");
    SWC_CHECK_ARG(D == ML_D && F > 0 && F % ML_SL == 0, "swc_layer_tail: needs D = %d and F a multiple of %d (D=%d F=%d)", ML_D,
                  ML_SL, D, F);
    SWC_CHECK_ARG(fc1_dtype == SWC_BF16 || fc1_dtype == SWC_FP8, "swc_layer_tail: fc1_dtype must be BF16 or FP8");
    SWC_CHECK_ARG(M >= 0, "swc_layer_tail: bad M");
    SWC_CHECK_ARG(aligned16(attn) && aligned16(x) && aligned16(x_out) && aligned16(bo) && aligned16(ln_w) && aligned16(ln_b) &&
                      aligned16(w_stream) && aligned16(b1) && aligned16(b2) && aligned16(next_ln_w) && aligned16(next_ln_b) &&
                      aligned16(y_next),
                  "swc_layer_tail: unaligned");
    if (M == 0) return SWC_OK;
    const unsigned grid = (unsigned)((M + ML_BM - 1) / ML_BM);
    if (fc1_dtype == SWC_FP8) {
        SWC_ENABLE_LDS((mlp_block_kernel<true, true>), ML_LDS, "swc_layer_tail");
        hipLaunchKernelGGL((mlp_block_kernel<true, true>), dim3(grid), dim3(256), ML_LDS, (hipStream_t)stream, x, x_out,
                           MlNorm{ln_w, ln_b}, eps, (const u32x4*)w_stream, b1, b2, MlNorm{next_ln_w, next_ln_b}, (bf16_t*)y_next, M,
                           F / ML_SL, (const bf16_t*)attn, bo, fc1_alpha, swc_sat_counter());
    } else if (operand_dtype == SWC_F16) {
        SWC_ENABLE_LDS((mlp_block_kernel<true, false, true>), ML_LDS, "swc_layer_tail");
        hipLaunchKernelGGL((mlp_block_kernel<true, false, true>), dim3(grid), dim3(256), ML_LDS, (hipStream_t)stream, x, x_out,
                           MlNorm{ln_w, ln_b}, eps, (const u32x4*)w_stream, b1, b2, MlNorm{next_ln_w, next_ln_b}, (bf16_t*)y_next, M,
                           F / ML_SL, (const bf16_t*)attn, bo, 1.0f, (unsigned*)nullptr);
    } else {
        SWC_ENABLE_LDS((mlp_block_kernel<true, false>), ML_LDS, "swc_layer_tail");
        hipLaunchKernelGGL((mlp_block_kernel<true, false>), dim3(grid), dim3(256), ML_LDS, (hipStream_t)stream, x, x_out,
                           MlNorm{ln_w, ln_b}, eps, (const u32x4*)w_stream, b1, b2, MlNorm{next_ln_w, next_ln_b}, (bf16_t*)y_next, M,
                           F / ML_SL, (const bf16_t*)attn, bo, 1.0f, (unsigned*)nullptr);
    }
    SWC_CHECK_LAUNCH("swc_layer_tail");
    return SWC_OK;
}
