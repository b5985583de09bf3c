// Device primitives shared by the MFMA kernels (swc_gemm, swc_attention16, swc_convnext, swc_convnext64, swc_mlp, swc_projln):
// fragment types, the LDS-DMA load, the packed 16-bit conversions in asm form, the 32 x 32 x 16 MFMA and the per-wave weight
// stream.  One copy each: M0 handling, the missing wait state after a transcendental and the operand maps are where a
// mistake is silent.
//
// v_mfma_f32_32x32x16_{bf16,f16} operand maps (lane l): A[row l&31][k = 8(l>>5) + j], B[k = 8(l>>5) + j][col l&31],
// D[row (r&3) + 8(r>>2) + 4(l>>5)][col l&31], r = 0..15.
#pragma once
#include "swc_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));   // one 32 x 32 accumulator tile
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // one MFMA operand fragment (8 x 16 bit) as a native vector: asm "v" operand
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// LDS byte address of a __shared__ pointer
__device__ __forceinline__ unsigned lds_addr_of(const void* p) {
    return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}

// 16 bytes per lane, global -> LDS (global_load_lds_dwordx4): 64 lanes x 16 bytes from per-lane global addresses to 1 KiB
// of LDS.  `lds_addr` is the wave-uniform LDS byte address; lane l lands at lds_addr + 16 l.  Written as inline asm on
// purpose: hipcc drains a compiler-visible LDS-DMA (s_waitcnt vmcnt(0)) in front of the next ds_read, which would
// serialise the prefetch of slice t+1 with the MFMAs of slice t.  Hidden in asm, the DMA is ordered by the caller's own
// `s_waitcnt vmcnt(N)` + barrier.  M0 is saved/restored inside the statement.
__device__ __forceinline__ void glds16_uniform(const void* gsrc, unsigned lds_addr) {  // lds_addr ALREADY in an SGPR (readfirstlane'd by the caller)
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(lds_addr)
        : "memory");
}
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_addr) {
    glds16_uniform(gsrc, __builtin_amdgcn_readfirstlane(lds_addr));  // wave-uniform by construction; pin it to an SGPR
}
// same, address = wave-uniform 64-bit base (SGPR pair) + per-lane unsigned 32-bit byte offset: one VGPR per lane
// instead of a 64-bit pointer per staged row
__device__ __forceinline__ void glds16_s(const char* base, unsigned off, unsigned lds_addr) {
    unsigned keep;
    lds_addr = __builtin_amdgcn_readfirstlane(lds_addr);
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(off), "s"(base), "s"(lds_addr)
        : "memory");
}

// two f32 -> one dword of two bf16 / f16 (lo in bits 0..15), RNE, one v_cvt_pk_* as inline asm.  ONLY for operands that a
// plain VALU instruction produced (e.g. the fma that ends gelu_fast): hipcc does not insert, for an asm statement, the wait
// state that a transcendental result needs before its first use (an asm form fed from v_exp_f32 returned NaNs).  Behind a
// transcendental use the vector conversions bf16_pack2 / pack2_f16 of swc_common.h.
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
__device__ __forceinline__ unsigned pack_f16x2(float lo, float hi) {  // does not saturate: +-65504 is the caller's business
    unsigned r;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}

// one 32 x 32 x 16 MFMA through the builtin: hipcc chooses the register file of the accumulator (AGPRs for the large
// second-GEMM tiles) and inserts the hazard padding.
// The kernels ALSO keep groups of MFMAs as inline asm with "v" operands (mfma32x4_vgpr in swc_convnext.hip,
// ml_mfma2x2_vgpr / ml_mfma8_1x4_vgpr in swc_mlp.hip, c6_mfma1x2_vgpr in swc_convnext64.hip, mfma16x8_vgpr / mfma16x4_agpr
// in swc_convnext.hip; their shapes differ per kernel).  Why asm: the accumulators of the second GEMM fill the AGPR half
// of the register file; left to hipcc, the first GEMM's accumulators are also given AGPR-form MFMAs and the two sets are
// shuffled between the halves with ~1500 v_accvgpr_read/write/mov per slice (6 k issue cycles beside 8 k MFMA cycles).
// With "v" operands they stay in VGPRs, where the GELU reads them directly.  One statement per k-step: its leading
// s_nop 1 covers a VALU copy of an operand hipcc may have placed right in front (it pads nothing inside asm), and the
// first VALU reader of the results needs the wait states (s_nop 15, s_nop 7) hipcc would insert for its own MFMAs.
template <bool F16 = false>
__device__ __forceinline__ f32x16 mfma32(const u32x4& a, const u32x4& b, f32x16 c) {
    if constexpr (F16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(&a), *reinterpret_cast<const f16x8*>(&b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&a), *reinterpret_cast<const bf16x8*>(&b),
                                                       c, 0, 0, 0);
}

// The per-wave weight stream of the kernels whose weights never touch LDS: the host packs every wave's 1 KiB fragments
// (64 lanes x 16 bytes) in its order of consumption, the wave keeps PF of them in flight in a register ring `u32x4 ring[PF]`
// of its own.  Address of a fragment = wave-uniform byte pointer `base` (SGPR pair, advanced by the kernel once per phase) +
// one 32-bit lane offset + immediate: per-fragment 64-bit VGPR addresses cost 28 registers and a spill in the slice loop.
// ABL: the kernel's timing-ablation mask; bit 4 = no weight loads in the loop (the ring keeps re-reading its first fragments).
// Used by swc_projln.hip.  swc_convnext.hip, swc_convnext64.hip and swc_mlp.hip write the same form out as locals and a
// `wfrag` lambda: with the pointer a struct member the loop-carried values of their slice loops are numbered in another
// order and hipcc allocates other registers (same instructions; tools/isa_equal.py), so they were left as measured.
template <int PF, int ABL = 0>
struct WeightStream {
    const char* base;
    unsigned lane_off;
    // stream of wave w (wave-uniform); per_wave: fragments per wave
    __device__ __forceinline__ WeightStream(const u32x4* wstream, int w, long per_wave, int lane)
        : base(reinterpret_cast<const char*>(wstream) + (long)w * per_wave * 1024), lane_off((unsigned)lane * 16u) {}
    // fragment i of the current phase (i may run PF past its end: the stream is padded)
    __device__ __forceinline__ u32x4 frag(int i) const {
        if (ABL & 4) i &= PF - 1;
        return *reinterpret_cast<const u32x4*>(base + (long)i * 1024 + lane_off);
    }
};
