"""Every place in simwhisper_codec_amd/csrc/ that converts an ACTIVATION to split-f16 or fp8, read off the source.

COUNTED: one entry per call of sat_commit / sat_commit_out (the range guard, swc_set_saturation_counter in include/swc.h): the
thread keeps the largest |scaled value| it converted and adds one to the caller's counter slot when that left the format's range.
An entry names the site as (file, enclosing function, n-th commit inside that function, text the line must hold) and lists the GPU
tests that hold it to an exact count ("file::test").  Several code paths can share one commit line (the direct GEMM epilogue has
one pair of commits for its vector and scalar bodies and for every geometry): `paths` spells them out, and the GPU cases cover each.

BOUNDED: conversions that do not track the range, each with the reason the value cannot leave it (or, for swc_attention_ex, the
statement that it can and who relies on that).  (file, enclosing function, text of the converting line, reason, GPU tests or ()).

tests/test_sat_sites_cpu.py pins the table to the source: a commit in the source that no entry claims, an entry whose site is
gone, an entry without a GPU test (unless marked unreachable, with the CPU test that pins why), a converting function that neither commits nor is listed as bounded — each fails there.

Out of scope: conversions of WEIGHTS (swc_cast_* called at load time are the same kernels as the activation casts and are
covered as such), and the plain-f16 operands INSIDE swc_layer_tail / swc_mlp_block / swc_convnext_* with operand_dtype SWC_F16
(never stored to memory in a reduced-range format; the decode side, whose packing step checks the range: codec._cx_f16_safe).
"""

RG = "test_range_guard_gpu.py::"

# helpers whose sat_commit lines dispatch on the output type for their callers: not sites themselves
HELPERS = {("swc_common.h", "sat_commit"), ("swc_pointwise.hip", "sat_commit_out")}

# functions that convert (f16s_store4 / f16s_split / f16s_split2 / fp8_pack4 / store_row4 / pack2_f16) for their callers
CONVERTERS = {("swc_common.h", None), ("swc_pointwise.hip", "store_row4")}


def C(id, file, func, nth, text, slot, paths, gpu, unreachable=None):
    """unreachable: the commit is never instantiated, so no GPU test can reach it; names the test of tests/test_sat_sites_cpu.py
    that pins the condition which compiles it out.  Such an entry lists no GPU case."""
    return dict(id=id, file=file, func=func, nth=nth, text=text, slot=slot, paths=tuple(paths), gpu=tuple(gpu), unreachable=unreachable)


COUNTED = [
    C("ln.generic", "swc_pointwise.hip", "layernorm_kernel", 0, "sat_commit_out<OutT>(sat, amax)", "f16s|fp8",
      ["generic LayerNorm, split-f16 output (C not 512 / 768)", "generic LayerNorm, fp8 output (every C, 512 and 768 included)"],
      [RG + "test_layernorm_threshold", RG + "test_layernorm_position_masks_accounting", "test_guards_gpu.py::test_saturation_counter_unit"]),
    C("ln.two_rows", "swc_pointwise.hip", "layernorm2_kernel", 0, "sat_commit_out<OutT>(sat, amax)", "f16s",
      ["layernorm2_kernel C = 512, split-f16 output", "layernorm2_kernel C = 768, split-f16 output"],
      [RG + "test_layernorm_threshold", RG + "test_layernorm_position_masks_accounting"]),
    C("snake.interior", "swc_pointwise.hip", "snake_aa_kernel", 0, "sat_commit_out<OutT>(sat, amax)", "f16s",
      ["snake_aa_kernel, interior-strip exit (no exact threshold case: every output is a filtered sum, no input makes one equal "
       "1023.5 bit for bit; counts are bounded by the float64 reference)"], [RG + "test_snake_exits"]),
    C("snake.generic", "swc_pointwise.hip", "snake_aa_kernel", 1, "sat_commit_out<OutT>(sat, amax)", "f16s",
      ["snake_aa_kernel, generic-strip exit (no exact threshold case, as above)"], [RG + "test_snake_exits"]),
    C("cast.fp8", "swc_pointwise.hip", "cast_fp8_kernel", 0, "sat_commit(sat, 1, amax, SWC_FP8_LIMIT)", "fp8",
      ["swc_cast_fp8 from f32", "swc_cast_fp8 from bf16"],
      [RG + "test_cast_sites", "test_guards_gpu.py::test_saturation_counter_unit"]),
    C("cast.f16s", "swc_pointwise.hip", "cast_f16s_kernel", 0, "sat_commit(sat, 0, amax, SWC_F16S_LIMIT)", "f16s",
      ["swc_cast_f32_f16s"], [RG + "test_cast_sites", "test_guards_gpu.py::test_saturation_counter_unit"]),
    C("gemm.direct.f16s", "swc_gemm.hip", "gemm_epilogue_direct", 0, "sat_commit(p.sat, 0, amax, SWC_F16S_LIMIT)", "f16s",
      ["direct epilogue, split-f16 body: 4-wave 64- and 128-row tiles, 8-wave 128- / 192- / 256-row tiles, plain and implicit-conv "
       "staging, activation bodies 0 / 1 / 2, the single-body 256-row conv kernel"],
      [RG + "test_gemm_sites", "test_work_walk_gpu.py::test_gemm_walk"]),
    C("gemm.direct.fp8", "swc_gemm.hip", "gemm_epilogue_direct", 1, "sat_commit(p.sat, 1, amax, SWC_FP8_LIMIT)", "fp8",
      ["direct epilogue, fp8 vector body: 4-wave 128-row tile, 8-wave 128- / 192- / 256-row tiles, plain and implicit-conv staging, "
       "activation bodies 0 / 1 / 2", "direct epilogue, fp8 scalar tail (N or ldc cuts the lane's 16 columns)"],
      [RG + "test_gemm_sites", "test_work_walk_gpu.py::test_gemm_walk"]),
    # compiled out: `if constexpr (SLAB && sizeof(OutT) == 4 && ...)` admits f32 outputs only, so the fp8 commit behind the slab
    # epilogue is never instantiated; fp8 outputs take the direct epilogue in every geometry (gemm.direct.fp8).  The CPU test pins
    # the gate; should it ever admit fp8_t that test fails and the entry needs GPU cases of its own.
    C("gemm.slab.fp8", "swc_gemm.hip", "gemm_epilogue", 0, "sat_commit(p.sat, 1, amax, SWC_FP8_LIMIT)", "fp8",
      ["slab epilogue, fp8 (unreachable: the slab gate admits 4-byte outputs only)"],
      [], unreachable="test_the_slab_epilogue_admits_f32_outputs_only"),
    C("skinny.f16s", "swc_gemm_skinny.hip", "skinny_epilogue", 0, "sat_commit(p.sat, 0, amax, SWC_F16S_LIMIT)", "f16s",
      ["skinny geometry, vector path", "skinny geometry, tail path (residual pitch or address breaks 16-byte rows)"],
      [RG + "test_skinny_sites"]),
    C("projln.y_next", "swc_projln.hip", "projln_kernel", 0, "if (y_next) sat_commit(sat, 0, amax, SWC_F16S_LIMIT)", "f16s",
      ["swc_proj_ln, LayerNorm output y_next"],
      [RG + "test_proj_ln_y_next", "test_kernels_gpu.py::test_proj_ln_errors_and_saturation"]),
    C("layer_tail.fp8_ln", "swc_mlp.hip", "mlp_block_kernel", 0, "if constexpr (F8) sat_commit(sat, 1, amax8, SWC_FP8_LIMIT)", "fp8",
      ["swc_layer_tail with fp8 fc1: LayerNorm(x') written to LDS as e4m3"], [RG + "test_layer_tail_fp8_ln"]),
]
SLAB_GATE = "if constexpr (SLAB && sizeof(OutT) == 4 && !__is_same(OutT, f16s_t))"


def B(id, file, func, text, reason, gpu=()):
    return dict(id=id, file=file, func=func, text=text, reason=reason, gpu=tuple(gpu))


BOUNDED = [
    B("ln.generic.zero_rows", "swc_pointwise.hip", "layernorm_kernel", "store_row4<OutT>(yr, 4 * i, 0.f, 0.f, 0.f, 0.f, z_)",
      "zero stores of masked rows and of rows in [t_in, t_out)"),
    B("ln.two_rows.zero_rows", "swc_pointwise.hip", "layernorm2_kernel", "0.f, 0.f, 0.f, 0.f, z_)",
      "zero stores of masked rows and of rows in [t_in, t_out)"),
    B("attn16.out", "swc_attention16.hip", "attn16_kernel", "f16s_store4(out + (r0 + q) * 2L * D, head * 64 + d, a, bq, c, e)",
      "split-f16 output of attn16: a convex combination (softmax weights) of v values that were themselves stored in range; "
      "the zero rows of padding queries go through the same line"),
    B("attn16.p", "swc_attention16.hip", "attn16_kernel", "pack2_f16(p0",
      "softmax probabilities in [0, 1], an operand kept in registers"),
    B("gemm.slab.f16s_store", "swc_gemm.hip", "gemm_epilogue_slab", "f16s_store4(reinterpret_cast<unsigned short*>(p.C) + (long)row * p.ldc * 2, col, v0 * os",
      "never instantiated: the slab gate (SLAB_GATE) admits f32 outputs only.  Were it opened to f16s_t, this store would go "
      "UNCOUNTED: gemm_epilogue commits behind the slab for fp8 alone"),
    B("gemm.slab.fp8_store", "swc_gemm.hip", "gemm_epilogue_slab", "fp8_pack4(v0 * os, v1 * os, v2 * os, v3 * os, amax)",
      "never instantiated: the slab gate (SLAB_GATE) admits f32 outputs only (COUNTED gemm.slab.fp8 is its commit)"),
    B("istft.spec", "swc_pointwise.hip", "spec_store", "f16s_split(v * SWC_F16S_ACT_SCALE, hi, lo)",
      "istft_spec2_kernel: |S| <= 100 by the magnitude clip min(exp(.), 100) (value_domain.istft_ref); the zero columns beyond 642"),
    B("attention_ex.zero_rows", "swc_attention.hip", "attn_kernel", "f16s_store4(orow_s, head * HD + dt * 16 + fh * 4, 0.f, 0.f, 0.f, 0.f)",
      "zero stores of query blocks beyond lens[b]"),
    B("attention_ex.out", "swc_attention.hip", "attn_kernel", "f16s_store4(orow_s, head * HD + dt * 16 + fh * 4, v[0] * SWC_F16S_ACT_SCALE",
      "NOT bounded: f32 v is unbounded, the weighted sum saturates at +-65504 / 64 UNCOUNTED (stated in include/swc.h); no caller "
      "inside the package takes this form: `mixed` casts q/k/v to split-f16 in the GEMM epilogue (counted there) and runs attn16",
      [RG + "test_attention_ex_saturates_uncounted"]),
]


def gpu_cases():
    """every "file::test" the table points at"""
    out = set()
    for e in COUNTED + BOUNDED:
        out.update(e["gpu"])
    return sorted(out)
