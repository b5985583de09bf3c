"""swc_gemm and swc_dwconv7_ln in the regime where a workgroup walks several work items (tests/work_walk.py: the case table,
each case checked against the plan functions by tests/test_work_walk_cpu.py).  Per case:

 1. the result against a float64 statement of the op (matmul or conv1d, bias, F.gelu, gamma, residual; conv1d + layer_norm),
    computed on the device and anchored once per kernel against the same statement on the CPU.  Tolerances are those of
    tests/test_kernels_gpu.py for the same operand and output format (named at TOL below), relative to the largest |reference|;
 2. every element of the (M, N) window is written, the columns N..ldc and the rows behind M keep their fill bit for bit;
 3. the result does not depend on the walk: the same rows computed by launches in which every workgroup has exactly one item,
    on the same kernel (both asserted through the plan of the very arguments of each launch), are bit-identical: M is cut at
    tile-row multiples; the cases of one row panel are cut along N.  The in-place-residual cases are also compared with the
    out-of-place result of the same call.  One shape has no cut (work_walk.py, "fp8-192-plus1-1x257": the CPU test shows that
    none exists): it runs 1 and 2 only; the same kernel instance is cut in "fp8-192-band4-m2-inplace";
 4. the saturation counter reads the same for the walked launch and the sum of the one-item launches (split-f16 / fp8 outputs;
    a few bias columns are raised beyond the formats' range so that the count is not zero).
"""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import work_walk as ww  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

# relative to max |reference|.  tests/test_kernels_gpu.py: test_gemm_plain (f32 2e-6, bf16 2e-5: bias only), test_gemm_epilogue /
# test_gemm_conv1d / test_gemm_big_tile_bf16 (f32 3e-6, bf16 3e-5: epilogue inputs, conv taps), test_gemm_f16s_is_f32_class (2e-6;
# 3e-6 with GELU + residual and for the split-f16 output), test_gemm_fp8 (5e-5 against the product of the quantised operands;
# e4m3 output: half an ulp + the subnormal step + 1e-3 per element), bf16 outputs 8e-3 everywhere; test_dwconv7_ln (2e-5
# absolute for f32, 8e-3 relative for bf16)
TOL = {"f32": (2e-6, 3e-6), "bf16": (2e-5, 3e-5), "f16s": (2e-6, 3e-6), "fp8": (5e-5, 5e-5)}   # (bias only, epilogue / conv)
TOL_BF16_OUT, TOL_F16S_OUT = 8e-3, 3e-6
TOL_DW_F32_ABS, TOL_DW_BF16_REL = 2e-5, 8e-3
GUARD_ROWS = 64
CLIP_EVERY = 53          # split-f16 / fp8 outputs: bias of every 53rd column lies beyond the output format's range


def _ops():
    from simwhisper_codec_amd import ops
    return ops


def _unsplit(t, N, scale):
    """split-f16 [rows, 2N] -> float64 [rows, N] (tests/test_kernels_gpu.py::_unsplit, on the device)"""
    v = t.double().view(t.shape[0], N // 32, 2, 32)
    return (v[:, :, 0] + v[:, :, 1]).reshape(t.shape[0], N) / scale


def _filled(rows, cols, dtype):
    """an output buffer of NaN (fp8: the byte 0x7f, e4m3fn's NaN, which the saturating conversions never produce)"""
    if dtype == torch.float8_e4m3fn:
        return torch.full((rows, cols), 0x7F, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)
    return torch.full((rows, cols), float("nan"), dtype=dtype, device=DEV)


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _is_fill(t):
    b = _bits(t)
    return b == _bits(_filled(1, 1, t.dtype))[0, 0]


class GemmRun:
    """operands, epilogue inputs and the float64 reference of one case, on the device"""

    def __init__(self, case):
        ops = _ops()
        self.case, c = case, case
        M, N, K = c["M"], c["N"], c["K"]
        g = torch.Generator(device=DEV).manual_seed(len(c["name"]) * 1000 + M % 997)
        rnd = lambda *s: torch.randn(*s, generator=g, device=DEV)
        if c["conv"] is None:
            self.taps, self.rows_in, self.t_in, self.t_out = 1, M, M, M
        else:
            self.taps, self.dil, self.stride, self.pad, self.t_in, self.t_out = ww.conv_geometry(c["conv"])
            self.rows_in = c["conv"][3] * self.t_in
        A = rnd(self.rows_in, K)
        W = rnd(N, self.taps * K) / math.sqrt(self.taps * K)
        self.alpha = 1.0
        if c["a"] == "f32":
            self.A, self.W, A64, W64 = A, W, A.double(), W.double()
        elif c["a"] == "bf16":
            self.A, self.W = A.bfloat16(), W.bfloat16()
            A64, W64 = self.A.double(), self.W.double()
        elif c["a"] == "f16s":       # f32-class operands: the reference is the product of the f32 values (test_gemm_f16s_is_f32_class)
            sa, sw = 64.0, 2.0 ** 10
            self.A, self.W = ops.cast_f16s(A, K, scale=sa), ops.cast_f16s(W, self.taps * K, scale=sw)
            A64, W64, self.alpha = A.double(), W.double(), 1.0 / (sa * sw)
        else:                        # fp8: the reference is the product of the QUANTISED operands (test_gemm_fp8)
            sa, sw = 16.0, 2.0 ** 6
            self.A, self.W = ops.cast_fp8(A, sa), ops.cast_fp8(W, sw)
            A64, W64, self.alpha = self.A.float().double() / sa, self.W.float().double() / sw, 1.0 / (sa * sw)
        pad1 = rnd(2 * N + 8)
        off = 1 if c["unaligned"] else 0                       # 4-byte aligned views: the direct f32 epilogue path
        self.bias = pad1[off:off + N] if c["bias"] else None
        self.gamma = pad1[N + 4 + off:2 * N + 4 + off] if c["gamma"] else None
        self.clipped = torch.zeros(N, dtype=torch.bool, device=DEV)
        if c["c"] in ("f16s", "fp8"):
            self.clipped[::CLIP_EVERY] = True
            self.bias[::CLIP_EVERY] = 5000.0
        self.ldc = N + c["ldc_pad"]
        self.res = rnd(M + GUARD_ROWS, self.ldc) if c["residual"] else None
        # ---- the op, stated plainly in float64
        if c["conv"] is None:
            ref = A64 @ W64.T
        else:                        # conv1d: output frame t of utterance b reads, for tap j, frame t * stride + j * dil - pad
            B = c["conv"][3]
            x = F.pad(A64.view(B, self.t_in, K), (0, 0, self.pad, self.pad))
            t = torch.arange(self.t_out, device=DEV) * self.stride
            ref = sum(x[:, t + j * self.dil] @ W64[:, j * K:(j + 1) * K].T for j in range(self.taps)).reshape(M, N)
            self.A64, self.W64 = A64, W64
        if c["bias"]:
            ref = ref + self.bias.double()
        if c["gelu"]:
            ref = F.gelu(ref)
        if c["gamma"]:
            ref = ref * self.gamma.double()
        if c["residual"]:
            ref = ref + self.res[:M, :N].double()
        self.ref = ref

    def out_buffer(self):
        c = self.case
        return _filled(c["M"] + GUARD_ROWS, ww.DT[c["c"]] == torch.float16 and 2 * self.ldc or self.ldc, ww.DT[c["c"]])

    def launch(self, out, row0=0, rows=None, col0=0, cols=None, residual="own", plan_only=False):
        """rows [row0, row0 + rows) x columns [col0, col0 + cols) of the case into the same window of `out`; plan_only: launch
        nothing, return the plan of the argument block this very call would pass"""
        ops, c = _ops(), self.case
        rows = c["M"] if rows is None else rows
        cols = c["N"] if cols is None else cols
        res = self.res if residual == "own" else residual
        kw = {}
        a0 = row0
        if c["conv"] is not None:
            assert row0 % self.t_out == 0 and rows % self.t_out == 0
            a0 = row0 // self.t_out * self.t_in
            kw = dict(taps=self.taps, dil=self.dil, stride=self.stride, pad=self.pad, t_in=self.t_in, t_out=self.t_out,
                      ldw=self.taps * c["K"])
        w = 2 if out.dtype == torch.float16 else 1
        call = ops.gemm_call_plan if plan_only else ops.gemm
        got = call(self.A[a0:], self.W[col0:], rows, cols, c["K"], out=out[row0:, w * col0:], ldc=self.ldc,
                   bias=None if self.bias is None else self.bias[col0:], gamma=None if self.gamma is None else self.gamma[col0:],
                   residual=None if res is None else res[row0:, col0:], ldr=self.ldc if res is not None else None,
                   act=ops.ACT_GELU if c["gelu"] else ops.ACT_NONE, alpha=self.alpha, out_scale=c["out_scale"], **kw)
        return got if plan_only else out

    def window(self, out):
        c = self.case
        w = 2 * c["N"] if out.dtype == torch.float16 else c["N"]
        return out[:c["M"], :w]


def _check_against_reference(run, out):
    c, ref = run.case, run.ref
    keep = ~run.clipped
    got = run.window(out)
    if c["c"] == "f16s":
        got = _unsplit(got, c["N"], c["out_scale"])
    elif c["c"] == "fp8":
        got = got.float().double() / c["out_scale"]
    else:
        got = got.double()
    got, want = got[:, keep], ref[:, keep]
    if c["c"] == "fp8":
        tol = want.abs() * 2.0 ** -4 + 2.0 ** -9 / 16 + 1e-3
        worst = float(((got - want).abs() - tol).max())
        print(f"{c['name']}: worst |err| - tol = {worst:.3e}")
        assert worst <= 0
        return
    epilogue = c["gelu"] or c["gamma"] or c["residual"] or c["conv"] is not None
    tol = {"bf16": TOL_BF16_OUT, "f16s": TOL_F16S_OUT}.get(c["c"], TOL[c["a"]][1 if epilogue else 0])
    err = float((got - want).abs().max() / want.abs().max())
    print(f"{c['name']}: rel err {err:.3e} (tol {tol:.0e})")
    assert err < tol, (c["name"], err, tol)


def _check_fill(run, out):
    c = run.case
    win = run.window(out)
    assert not bool(_is_fill(win).any()) and (c["c"] == "fp8" or not bool(torch.isnan(win.float()).any()))
    assert bool(_is_fill(out[:, win.shape[1]:]).all()), "columns N..ldc were written"
    assert bool(_is_fill(out[c["M"]:]).all()), "rows behind M were written"


@pytest.mark.parametrize("case", ww.GEMM_CASES, ids=lambda c: c["name"])
def test_gemm_walk(case):
    ops = _ops()
    run = GemmRun(case)
    first = run.out_buffer()
    plan = run.launch(first, plan_only=True)                   # of the arguments the call below passes
    assert plan == ww.gemm_plan(case)                          # ... which are the ones the CPU test pinned to the regime
    assert (plan["tile_m"], plan["waves"], plan["band"]) == (case["tile"], case["waves"], case["band"])
    assert plan["grid"] == plan["slots"] < plan["n_tiles_m"] * plan["n_tiles_n"] and ww.walk_class(plan) == case["walk"]
    counted = case["c"] in ("f16s", "fp8")
    sat = torch.zeros(2, dtype=torch.int32, device=DEV)
    ops.set_saturation_counter(sat if counted else None)
    try:
        out = run.launch(first)
        sat_walk = sat.clone()
        _check_against_reference(run, out)
        _check_fill(run, out)
        if case["inplace"]:                                    # out is residual: against the out-of-place result of the same call
            r = run.res.clone()
            run.launch(r, residual=r)
            assert torch.equal(r[:case["M"], :case["N"]], out[:case["M"], :case["N"]])
            assert torch.equal(r[case["M"]:], run.res[case["M"]:]) and torch.equal(r[:, case["N"]:], run.res[:, case["N"]:])
        if case["split"] is None:                              # work_walk.py: no cut into one-item launches exists for this shape
            return
        sat.zero_()
        split = run.out_buffer()
        for row0, rows, col0, cols in ww.gemm_chunks(case):
            q = run.launch(split, row0, rows, col0, cols, plan_only=True)
            assert q["grid"] == q["n_tiles_m"] * q["n_tiles_n"] and all(q[k] == plan[k] for k in ww.SAME_KERNEL)
            run.launch(split, row0, rows, col0, cols)
        _check_fill(run, split)
        assert torch.equal(_bits(run.window(out)), _bits(run.window(split))), "the result depends on the walk"
        if counted:
            assert int(sat_walk[0 if case["c"] == "f16s" else 1]) > 0 and torch.equal(sat, sat_walk), (sat, sat_walk)
    finally:
        ops.set_saturation_counter(None)


def test_gemm_device_reference_is_anchored():
    """the float64 statements GemmRun evaluates on the device, evaluated by the CPU: a plain case with every epilogue input
    and a strided conv case"""
    for name in ("bf16-64-plus1", "bf16-128-mixed-conv3s2"):
        case = next(c for c in ww.GEMM_CASES if c["name"] == name)
        run = GemmRun(case)
        M, N, K = case["M"], case["N"], case["K"]
        if case["conv"] is None:
            cpu = run.A.cpu().double() @ run.W.cpu().double().T
            rows = slice(0, M)
        else:                                                  # the first two utterances
            B, T = 2, run.t_in
            x = run.A64[:B * T].cpu().view(B, T, K).transpose(1, 2)
            w = run.W64.cpu().view(N, run.taps, K).permute(0, 2, 1)
            cpu = F.conv1d(x, w, stride=run.stride, padding=run.pad, dilation=run.dil).transpose(1, 2).reshape(-1, N)
            rows = slice(0, B * run.t_out)
        cpu = cpu + run.bias.cpu().double()
        if case["gelu"]:
            cpu = F.gelu(cpu)
        if case["gamma"]:
            cpu = cpu * run.gamma.cpu().double()
        if case["residual"]:
            cpu = cpu + run.res[rows, :N].cpu().double()
        assert float((run.ref[rows].cpu() - cpu).abs().max()) < 1e-12 * float(cpu.abs().max())


# --------------------------------------------------------------------------------------------------------- swc_dwconv7_ln
class DwRun:
    def __init__(self, case):
        B, T, C_ = case["B"], case["T"], case["C"]
        g = torch.Generator(device=DEV).manual_seed(C_ * 7 + T)
        rnd = lambda *s: torch.randn(*s, generator=g, device=DEV)
        self.case, self.x, self.w7 = case, rnd(B, T, C_), rnd(7, C_) / 3
        self.b, self.lw, self.lb = rnd(C_), rnd(C_), rnd(C_)
        x = F.pad(self.x.double(), (0, 0, 3, 3))               # Conv1d(k = 7, padding = 3, groups = C) per utterance
        y = sum(x[:, j:j + T] * self.w7[j].double() for j in range(7)) + self.b.double()
        self.ref = F.layer_norm(y, (C_,), self.lw.double(), self.lb.double(), 1e-6)

    def out_buffer(self):
        c = self.case
        return _filled(c["B"] * c["T"] + GUARD_ROWS, c["C"], ww.DT[c["out"]])

    def launch(self, out, b0=0, nb=None):
        c = self.case
        nb = c["B"] if nb is None else nb
        _ops().dwconv7_ln(self.x[b0:b0 + nb], self.w7, self.b, self.lw, self.lb, 1e-6, B=nb, T=c["T"], C_=c["C"],
                          out=out[b0 * c["T"]:])
        return out


@pytest.mark.parametrize("case", ww.DW_CASES, ids=lambda c: c["name"])
def test_dwconv7_ln_walk(case):
    plan = ww.dw_plan(case)
    assert plan["per"] == case["per"] >= 2 and plan["nstrips"] > plan["slots"] == case["slots"]
    run = DwRun(case)
    rows = case["B"] * case["T"]
    out = run.launch(run.out_buffer())
    got, ref = out[:rows].double(), run.ref.view(rows, -1)
    if case["out"] == "f32":
        err = float((got - ref).abs().max())
        print(f"{case['name']}: abs err {err:.3e}")
        assert err < TOL_DW_F32_ABS
    else:
        err = float((got - ref).abs().max() / ref.abs().max())
        print(f"{case['name']}: rel err {err:.3e}")
        assert err < TOL_DW_BF16_REL
    assert not bool(torch.isnan(out[:rows].float()).any()) and bool(_is_fill(out[rows:]).all())
    split = run.out_buffer()
    for b0, nb in ww.dw_groups(case):
        assert ww.dw_plan(case, nb)["per"] == 1 and ww.dw_plan(case, nb)["S"] == plan["S"]
        run.launch(split, b0, nb)
    assert bool(_is_fill(split[rows:]).all())
    assert torch.equal(_bits(out[:rows]), _bits(split[:rows])), "the result depends on the walk"


def test_dwconv_device_reference_is_anchored():
    case = next(c for c in ww.DW_CASES if c["name"] == "c64-f32-per2")
    run = DwRun(case)
    C_ = case["C"]
    x = run.x.cpu().double().transpose(1, 2)
    y = F.conv1d(x, run.w7.cpu().double().T.reshape(C_, 1, 7), run.b.cpu().double(), padding=3, groups=C_)
    cpu = F.layer_norm(y.transpose(1, 2), (C_,), run.lw.cpu().double(), run.lb.cpu().double(), 1e-6)
    assert float((run.ref.cpu() - cpu).abs().max()) < 1e-12 * float(cpu.abs().max())
