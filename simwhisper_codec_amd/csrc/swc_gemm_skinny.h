// The "skinny" geometry of swc_gemm (swc_gemm_skinny.hip): few rows, long reduction.  gemm_plan() in swc_gemm.hip decides
// when it is taken; this header is the seam between the two files.
#pragma once
#include "swc_common.h"

// resident workgroups per CU the kernel is built for (3 stages of 24 KiB each; < 128 registers)
#ifndef SWC_SKINNY_WG_PER_CU
#define SWC_SKINNY_WG_PER_CU 2
#endif
// waves per workgroup, side by side along N: 4 (32 columns each) or 8 (16 columns each)
#ifndef SWC_SKINNY_WAVES
#define SWC_SKINNY_WAVES 4
#endif
constexpr int SWC_SKINNY_TILE_M = 64, SWC_SKINNY_TILE_N = 128;
// smallest reduction length taps x K (logical elements) that takes the geometry
#ifndef SWC_SKINNY_MIN_K
#define SWC_SKINNY_MIN_K 512
#endif

// Launches the kernel for `a` (checked by gemm_check_args, chosen by gemm_plan: bf16 or split-f16 operands, K a multiple of
// the slice, operands below 2 GiB) on one workgroup per tile.  `sat`: the calling thread's saturation counters or nullptr.
int swc_gemm_skinny_launch(const swc_gemm_args* a, int n_tiles_m, int n_tiles_n, int kc_per_tap, unsigned* sat, hipStream_t s);
