"""Value-domain sweeps: each kernel's in-kernel math over the whole range of values it can be handed, against float64 on the
host (tests/value_domain.py holds the inputs and the references; test_value_domain_cpu.py ties the bounds used here to
float32 emulations of the formulas).  The shape coverage lives in test_kernels_gpu.py; the tensors here are the smallest
that carry a sweep."""
import math

import pytest
import torch

import value_domain as vd

pytestmark = pytest.mark.gpu

DEV = "cuda"
GELU_FAST = 2.8e-4      # gelu_fast: 2.71e-4 by the float32 emulation (test_value_domain_cpu) + one unit for v_exp_f32 / v_rcp_f32
F16S_FLOOR = 2.0 ** -24 / 64   # split-f16 at scale 64: absolute floor of the low half (test_f16s_cast_roundtrip)


def _ops():
    from simwhisper_codec_amd import ops
    return ops


def _d(t):
    return t.to(DEV)


def _unsplit(t, K, scale=64.0):
    """split-f16 [rows, 2K] -> float64 [rows, K]"""
    v = t.cpu().double().view(-1, K // 32, 2, 32)
    return (v[:, :, 0] + v[:, :, 1]).reshape(-1, K) / scale


def _check(name, got, ref, tol, where=None):
    """print the worst figure, then assert |got - ref| <= tol element by element (all float64 host tensors)"""
    err = (got - ref).abs()
    assert torch.isfinite(got).all(), name
    excess = err - tol
    i = int(excess.argmax())
    at = "" if where is None else f" at v={float(where.flatten()[i]):.9g}"
    print(f"[value-domain] {name}: max err {float(err.max()):.3e}, worst err/tol {float((err / tol).max()):.3f}{at} "
          f"(err {float(err.flatten()[i]):.3e}, tol {float(tol.flatten()[i]) if torch.is_tensor(tol) and tol.numel() > 1 else float(tol):.3e})")
    assert float(excess.max()) <= 0, name


# ------------------------------------------------------------------------------------------------------------ 1. GELU
def test_gelu_gemm_bf16_out():
    """gelu_fast in the bf16 epilogue of swc_gemm: A holds the sweep, W = I, so C[m, n] = gelu(A[m, n])."""
    ops = _ops()
    A = vd.pad_to(vd.gelu_sweep("bf16"), 128).view(-1, 128).to(torch.bfloat16)
    M = A.shape[0]
    out = ops.gemm(_d(A), _d(torch.eye(128).to(torch.bfloat16)), M, 128, 128, act=ops.ACT_GELU, out_dtype=torch.bfloat16)
    ref = vd.gelu_ref(A.float())
    _check("gemm bf16", out.float().cpu().double(), ref, GELU_FAST + 2.0 ** -8 * ref.abs(), A.float())


def test_gelu_gemm_f32_out():
    """erff in the f32 epilogue (f32 operands) on the same points."""
    ops = _ops()
    A = vd.pad_to(vd.gelu_sweep("bf16"), 128).view(-1, 128)
    out = ops.gemm(_d(A), _d(torch.eye(128)), A.shape[0], 128, 128, act=ops.ACT_GELU)
    ref = vd.gelu_ref(A)
    _check("gemm f32", out.cpu().double(), ref, 2.0 ** -22 * (1 + ref.abs()), A)


def test_gelu_gemm_f16s_out():
    """gelu_as in the split-f16 epilogue: the operand is the split form of the sweep (values beyond +-1023 saturate in the
    cast; the reference starts from what the operand holds)."""
    ops = _ops()
    A = vd.pad_to(vd.gelu_sweep("bf16"), 128).view(-1, 128)
    M = A.shape[0]
    As, Ws = ops.cast_f16s(_d(A), 128, scale=64.0), ops.cast_f16s(_d(torch.eye(128)), 128, scale=64.0)
    v = _unsplit(As, 128)
    assert float((v - A.double().clamp(-65504 / 64, 65504 / 64)).abs().sub(A.double().abs() * 2.0 ** -21 + F16S_FLOOR).max()) <= 0
    out = ops.gemm(As, Ws, M, 128, 128, alpha=1.0 / 4096, act=ops.ACT_GELU, out_dtype=torch.float16, out_scale=64.0)
    _check("gemm f16s", _unsplit(out, 128), vd.gelu_ref(v), 4e-7 * (1 + v.abs()), v)


def test_gelu_gemm_fp8_out():
    """gelu_fast in the e4m3 epilogue: every finite e4m3 operand value at three operand scales (|v| up to 112; the output
    saturates at 448 / 16)."""
    ops = _ops()
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)
    A8 = vd.pad_to(codes, 128).view(-1, 128).view(ops.FP8_T)
    W8 = ops.cast_fp8(_d(torch.eye(128)), 1.0)
    for alpha in (1.0 / 16, 1.0 / 64, 1.0 / 4):
        out = ops.gemm(_d(A8), W8, A8.shape[0], 128, 128, alpha=alpha, act=ops.ACT_GELU, out_dtype=ops.FP8_T, out_scale=16.0)
        v = A8.float().double() * alpha
        ref = vd.gelu_ref(v).clamp(-28.0, 28.0)
        # the refit's error, half an e4m3 step (3 mantissa bits, round to nearest) and the subnormal step 2^-9 at scale 16
        _check(f"gemm fp8 alpha={alpha}", out.float().cpu().double() / 16.0, ref, GELU_FAST + ref.abs() * 2.0 ** -4 + 2.0 ** -9 / 16, v)


def _eye_stream512(ops, dt, pack):
    eye = _d(torch.eye(512).to(dt))
    return pack(eye, eye, _d(torch.ones(512))) if pack is ops.convnext_pack else pack(eye, eye)


@pytest.mark.parametrize("kernel", ["convnext_mlp", "convnext64_mlp"])
def test_gelu_convnext_mlp(kernel):
    """W1 = W2 = I, zero biases, gamma = 1, x0 = 0: x = bf16(gelu(y)) for every element of y — the lane -> element mapping of
    the in-register GELU -> bf16 pack is pinned with the values."""
    ops = _ops()
    sw = vd.gelu_sweep("bf16")
    assert sw.numel() <= 128 * 512
    y = vd.pad_to(sw, 128 * 512).view(128, 512)
    z = _d(torch.zeros(512))
    x = _d(torch.zeros(128, 512))
    if kernel == "convnext_mlp":
        ops.convnext_mlp(_d(y.to(torch.bfloat16)), _eye_stream512(ops, torch.bfloat16, ops.convnext_pack), z, z, _d(torch.ones(512)), x,
                         M=128, C_=512, I=512)
    else:
        ops.convnext64_mlp(_d(y.to(torch.bfloat16)), _eye_stream512(ops, torch.bfloat16, ops.convnext64_pack), z, z, _d(torch.ones(512)),
                           x, M=128, C_=512, I=512)
    ref = vd.gelu_ref(y)
    _check(kernel, x.cpu().double(), ref, GELU_FAST + vd.ulp16(ref, "bf16"), y)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_gelu_convnext_block(fmt):
    """swc_convnext_block normalises before the MLP, so the sweep enters as the LayerNorm's bias with a zero LayerNorm weight
    (y = 0 * xhat + lb exactly): one call per 512 sweep points, identity centre tap, W1 = W2 = I, x0 = 0."""
    ops = _ops()
    dt = torch.bfloat16 if fmt == "bf16" else torch.float16
    sw = vd.pad_to(vd.gelu_sweep(fmt), 512).view(-1, 512)
    ws = _eye_stream512(ops, dt, ops.convnext_pack)
    z, one = _d(torch.zeros(512)), _d(torch.ones(512))
    w7 = torch.zeros(7, 512)
    w7[3] = 1.0
    w7 = _d(w7)
    x0 = _d(torch.zeros(1, 128, 512))
    swd = _d(sw)
    outs = []
    for i in range(sw.shape[0]):
        out = torch.full_like(x0, float("nan"))
        ops.convnext_block(x0, out, w7, z, z, swd[i], 1e-6, ws, z, z, one, B=1, T=128, C_=512, I=512, operands=dt)
        assert torch.equal(out[0, 1:], out[0, :1].expand(127, 512))          # every frame holds the same row
        outs.append(out[0, 127])
    got = torch.stack(outs).cpu().double()
    ref = vd.gelu_ref(sw)
    _check(f"convnext_block {fmt}", got, ref, GELU_FAST + vd.ulp16(ref, fmt), sw)


@pytest.mark.parametrize("kernel,fmt", [("mlp_block", "bf16"), ("layer_tail", "bf16"), ("layer_tail", "f16"), ("layer_tail", "fp8")])
def test_gelu_mlp_block_and_layer_tail(kernel, fmt):
    """The transformer MLP kernels normalise before fc1: LayerNorm weight 0 and W1 = 0 leave fc1's output equal to b1, which
    carries 768 sweep points per call; W2 = I, everything else zero, x = 0: x_out = round16(gelu(b1))."""
    ops = _ops()
    D = F_ = 768
    M = 64
    f16 = fmt == "f16"
    dt = torch.float16 if f16 else torch.bfloat16
    sw = vd.subsample(vd.gelu_sweep("f16" if f16 else "bf16"), 8 * F_).view(8, F_)
    zD, zw = _d(torch.zeros(D)), _d(torch.zeros(D, D).to(dt))
    eye = _d(torch.eye(D).to(dt))
    kw = {}
    if kernel == "mlp_block":
        ws = ops.mlp_pack(zw, eye)
    elif fmt == "fp8":
        ws = ops.layer_tail_pack(zw, ops.cast_fp8(_d(torch.zeros(F_, D)), 1.0), eye)
        kw = dict(fc1_dtype=ops.FP8_T, fc1_alpha=1.0 / ops.FP8_ACT_SCALE)
    else:
        ws = ops.layer_tail_pack(zw, zw, eye)
        kw = dict(operands=dt)
    att = _d(torch.zeros(M, D).to(torch.bfloat16))
    swd = _d(sw)
    outs = []
    for i in range(sw.shape[0]):
        x = _d(torch.zeros(M, D))
        if kernel == "mlp_block":
            xo, _ = ops.mlp_block(x, zD, zD, 1e-5, ws, swd[i], zD, M=M, D=D, F=F_)
        else:
            xo, _ = ops.layer_tail(att, x, ws, zD, zD, zD, 1e-5, swd[i], zD, M=M, D=D, F=F_, **kw)
        assert torch.equal(xo[1:], xo[:1].expand(M - 1, D))
        outs.append(xo[M - 1])
    got = torch.stack(outs).cpu().double()
    ref = vd.gelu_ref(sw)
    fm = "f16" if f16 else "bf16"
    if f16:
        ref = ref.clamp(-65504.0, 65504.0)
    _check(f"{kernel} {fmt}", got, ref, GELU_FAST + vd.ulp16(ref, fm), sw)


# ----------------------------------------------------------------------------------------------------- 2. sin^2 / snake
# bf16 outputs take the hardware sine (__sinf).  The largest |alpha * up| that swc_snake_aa is handed on the shipped path is 3.31
# (synthetic checkpoint, tiny and real configurations, the `single` and `ragged` golden inputs, every preset and output type; 2.98
# for the bf16 outputs alone).  Measured on an MI355X with this sweep: every point up to |a| = 1e5 stays within the bf16 bound
# below, the first miss is |a| = 1e6 ("Value domain").  The test asserts over 4x the path's range.
SNAKE_PATH_MAX = 3.31


def _snake_sweep(out_dtype):
    ops = _ops()
    f = vd.kaiser_sinc12()
    a_all = vd.pad_to(vd.snake_arguments(), 64)
    got, ref, tol_arg, args, betas = [], [], [], [], []
    for a in a_all.view(-1, 64):
        x, alpha, beta = vd.snake_case(a, f)
        out = ops.snake_aa(_d(x), _d(alpha), _d(beta), f.tolist(), B=1, T=16, C_=64, out_dtype=out_dtype)
        out = _unsplit(out.view(16, -1), 64).view(1, 16, 64) if out_dtype == torch.float16 else out.float().cpu().double()
        got.append(out[0])
        ref.append(vd.snake_ref(x.transpose(1, 2), alpha, beta, f)[0].T)
        args.append((vd.snake_up(x.transpose(1, 2), f)[0].T * alpha.double()).abs().amax(0, keepdim=True).expand(16, 64))
        betas.append(beta.double().expand(16, 64))
    return torch.cat(got), torch.cat(ref), torch.cat(args), torch.cat(betas)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16])
def test_snake_argument_domain(out_dtype):
    """sin2_f32 (f32 and split-f16 outputs): dense band, quadrant edges of both parities up to q = 5000, both sides of the
    switch to libm at 8192, and the libm branch.  Tolerance: the existing 1e-5, four float32 roundings of the argument
    (12-tap sum and the product: |a| 2^-21) and the function's own 1.5e-7, the last two through 1 / beta."""
    got, ref, a, beta = _snake_sweep(out_dtype)
    assert float(a.max()) > 9e5 and ((a > 8191.5) & (a <= 8192)).any()
    _check(f"snake {out_dtype}", got, ref, 1e-5 + (a * 2.0 ** -21 + 1.5e-7) / beta, a)


def test_snake_argument_domain_bf16():
    """__sinf behind the bf16 output: within the bf16 rounding bound over four times the range the path uses."""
    got, ref, a, beta = _snake_sweep(torch.bfloat16)
    tol = 2.0 ** -8 * ref.abs() + 1e-5 / beta
    ok = (got - ref).abs() <= tol
    bad = a[~ok]
    limit = float(a[a < bad.min()].max()) if bad.numel() else float(a.max())
    print(f"[value-domain] snake bf16: every sweep point with |a| <= {limit:.9g} is within the bf16 bound"
          + (f"; first miss at |a| = {float(bad.min()):.9g}" if bad.numel() else ""))
    sel = a <= 4 * SNAKE_PATH_MAX
    assert int(sel.sum()) > 100 * 16
    _check("snake bf16 (4x the path's range)", got[sel], ref[sel], tol[sel], a[sel])
    assert limit >= 4 * SNAKE_PATH_MAX


@pytest.mark.parametrize("C,T", [(512, 125), (64, 1), (64, 3), (32, 40)])
def test_snake_aa_bf16_values(C, T):
    """the bf16 output of swc_snake_aa at the shapes of test_snake_aa, against float64 to the bf16 rounding bound"""
    ops = _ops()
    B = 2
    g = torch.Generator().manual_seed(C * T)
    x = torch.randn(B, C, T, generator=g) * 2
    al, be = torch.randn(C, generator=g) * 0.3, torch.randn(C, generator=g) * 0.3
    f = vd.kaiser_sinc12()
    ref = vd.snake_ref(x, al.exp(), be.exp(), f).transpose(1, 2)      # on the float32 alpha, beta the kernel is handed
    out = ops.snake_aa(_d(x.transpose(1, 2).contiguous()), _d(al.exp()), _d(be.exp()), f.tolist(), B=B, T=T, C_=C,
                       out_dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16
    _check(f"snake_aa bf16 {C}x{T}", out.float().cpu().double(), ref, 2.0 ** -8 * ref.abs() + 1e-5)


# ---------------------------------------------------------------------------------------------------------- 3. ISTFT
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16])
def test_istft_spec_value_domain(out_dtype):
    """expf / cosf / sinf of swc_istft_spec: log-magnitudes from -100 over the clip at ln 100 to 1e4, phases up to 1e7.  Both
    factors are libm-accurate, so |err| <= mag 2^-21; to that comes only what the output format cannot hold at all: a float32
    subnormal step for the f32 output (mag = e^-100 is subnormal), the low half's floor for split-f16."""
    ops = _ops()
    h, _, _ = vd.istft_rows()
    sp = ops.istft_spec(_d(h), 656, 8, 672, out_dtype=out_dtype)
    if out_dtype == torch.float16:
        got, floor = _unsplit(sp, 672), F16S_FLOOR
    else:
        got, floor = sp.cpu().double(), 2.0 ** -149
    c, s, mag = vd.istft_ref(h)
    ph = h[:, 321:642]
    _check(f"istft re {out_dtype}", got[:, :321], c, mag * 2.0 ** -21 + floor, ph)
    _check(f"istft im {out_dtype}", got[:, 321:642], s, mag * 2.0 ** -21 + floor, ph)
    assert (got[:, 642:] == 0).all()


# ------------------------------------------------------------------------------------------------------ 4. LayerNorm
LN_ROWS = 96


def _ln_check(name, got, x, w, b, eps, ulp=None):
    """err_kernel <= 4 err_torch_f32 + 1e-6 (1 + |ref|) (+ one step of a 16-bit output format), element by element against
    the largest float32-torch error on the same rows; constant rows must return the bias."""
    ref = vd.ln_ref(x, w, b, eps)
    e_t = vd.ln_torch_f32_err(x, w, b, eps)
    extra = ulp(ref) if ulp is not None else 0.0
    err = (got - ref).abs()
    print(f"[value-domain] LayerNorm {name}: kernel max err {float(err.max()):.3e}, torch f32 max err {e_t:.3e}")
    assert torch.isfinite(got).all(), name
    assert float((err - (4 * e_t + 1e-6 * (1 + ref.abs()) + extra)).max()) <= 0, name
    if name.endswith("constant"):
        extra_b = ulp(b.double().expand_as(got)) if ulp is not None else 0.0
        assert float(((got - b.double()).abs() - (1e-6 * (1 + b.double().abs()) + extra_b)).max()) <= 0, name


@pytest.mark.parametrize("C", [128, 512, 768])
@pytest.mark.parametrize("family", vd.LN_FAMILIES)
def test_layernorm_hard_rows(family, C):
    """swc_layernorm, f32 output, ragged (lens) and packed (row_start): C = 128 takes layernorm_kernel, 512 / 768 layernorm2_kernel"""
    ops = _ops()
    x = vd.ln_rows(family, LN_ROWS, C)
    w, b = vd.ln_affine(C)
    lens, starts = [50, 46], [0, 50]
    out = ops.layernorm(_d(x), _d(w), _d(b), 1e-5, B=2, t_in=50, C_=C, lens=_d(torch.tensor(lens, dtype=torch.int32)),
                        row_start=_d(torch.tensor(starts, dtype=torch.int32))).cpu()
    assert (out[1, 46:] == 0).all()
    got = torch.cat([out[0, :50], out[1, :46]]).double()
    _ln_check(f"layernorm C={C} {family}", got, x, w, b, 1e-5)


@pytest.mark.parametrize("C", [128, 512, 768])
@pytest.mark.parametrize("family", vd.LN_FAMILIES)
def test_dwconv7_ln_hard_rows(family, C):
    """swc_dwconv7_ln with an identity centre tap (the other taps multiply by an exact zero): its LayerNorm alone"""
    ops = _ops()
    x = vd.ln_rows(family, LN_ROWS, C, seed=1)
    w, b = vd.ln_affine(C, seed=1)
    w7 = torch.zeros(7, C)
    w7[3] = 1.0
    out = ops.dwconv7_ln(_d(x.view(1, LN_ROWS, C)), _d(w7), _d(torch.zeros(C)), _d(w), _d(b), 1e-6, B=1, T=LN_ROWS, C_=C)
    _ln_check(f"dwconv7_ln C={C} {family}", out[0].cpu().double(), x, w, b, 1e-6)


@pytest.mark.parametrize("kernel", ["proj_ln", "mlp_block", "layer_tail"])
@pytest.mark.parametrize("family", vd.LN_FAMILIES)
def test_fused_layernorm_hard_rows(family, kernel):
    """The LayerNorm that closes swc_proj_ln (split-f16 out), swc_mlp_block and swc_layer_tail (bf16 out), with zero weights in
    front of it: x_out = x exactly and y_next = LN(x)."""
    ops = _ops()
    D = 768
    x = vd.ln_rows(family, LN_ROWS, D, seed=2)
    w, b = vd.ln_affine(D, seed=2)
    zD = _d(torch.zeros(D))
    xd = _d(x).clone()
    if kernel == "proj_ln":
        stream = ops.proj_ln_pack(ops.cast_f16s(_d(torch.zeros(D, D)), D, scale=64.0))
        a = _d(torch.zeros(LN_ROWS, 2 * D, dtype=torch.float16))
        xo, y = ops.proj_ln(a, stream, None, 1.0, xd, M=LN_ROWS, N=D, K=D, ln=(_d(w), _d(b)), eps=1e-5)
        got = _unsplit(y, D)
        ulp = lambda r: r.abs() * 2.0 ** -21 + F16S_FLOOR
    else:
        zw = _d(torch.zeros(D, D).to(torch.bfloat16))
        if kernel == "mlp_block":
            xo, y = ops.mlp_block(xd, zD, zD, 1e-5, ops.mlp_pack(zw, zw), zD, zD, M=LN_ROWS, D=D, F=D, next_ln=(_d(w), _d(b)))
        else:
            xo, y = ops.layer_tail(_d(torch.zeros(LN_ROWS, D).to(torch.bfloat16)), xd, ops.layer_tail_pack(zw, zw, zw), zD, zD, zD, 1e-5,
                                   zD, zD, M=LN_ROWS, D=D, F=D, next_ln=(_d(w), _d(b)))
        got = y.float().cpu().double()
        ulp = lambda r: vd.ulp16(r, "bf16")
    assert torch.equal(xo.cpu(), x)
    _ln_check(f"{kernel} {family}", got, x, w, b, 1e-5, ulp)


@pytest.mark.parametrize("family", vd.LN_FAMILIES)
def test_convnext_block_layernorm_hard_rows(family):
    """The LayerNorm inside swc_convnext_block (identity centre tap, W1 = W2 = I, gamma = 1): out = x + bf16(gelu(bf16(LN(x)))).
    The LayerNorm bound (with a bf16 step for y) passes through the GELU, whose slope is at most 1.13, and meets the GELU's own
    bound, a bf16 step of h and the float32 rounding of the residual sum.  For the `huge` family (and the 1e15 constant row)
    that last term, 2^-23 |x| ~ 1e8, hides y: those rows only have to come out finite here; swc_dwconv7_ln, the same front half
    with y as its output, is compared on them directly above."""
    ops = _ops()
    C, T = 512, LN_ROWS
    x = vd.ln_rows(family, T, C, seed=3)
    w, b = vd.ln_affine(C, seed=3)
    w7 = torch.zeros(7, C)
    w7[3] = 1.0
    z, one = _d(torch.zeros(C)), _d(torch.ones(C))
    xd = _d(x.view(1, T, C))
    out = torch.full_like(xd, float("nan"))
    ops.convnext_block(xd, out, _d(w7), z, _d(w), _d(b), 1e-6, _eye_stream512(ops, torch.bfloat16, ops.convnext_pack), z, z, one,
                       B=1, T=T, C_=C, I=C)
    y = vd.ln_ref(x, w, b, 1e-6)
    h = vd.gelu_ref(y)
    ref = x.double() + h
    e_t = vd.ln_torch_f32_err(x, w, b, 1e-6)
    tol = (1.13 * (4 * e_t + 1e-6 * (1 + y.abs()) + vd.ulp16(y, "bf16")) + GELU_FAST + vd.ulp16(h, "bf16") + 2.0 ** -23 * ref.abs())
    print(f"[value-domain] convnext_block LayerNorm {family}: torch f32 max err {e_t:.3e}")
    _check(f"convnext_block LN {family}", out[0].cpu().double(), ref, tol)


@pytest.mark.parametrize("kernel,fmt", [("mlp_block", "bf16"), ("layer_tail", "bf16"), ("layer_tail", "f16")])
@pytest.mark.parametrize("family", vd.LN_FAMILIES)
def test_leading_layernorm_hard_rows(family, kernel, fmt):
    """The LayerNorm in FRONT of fc1: swc_mlp_block's (one wave per row) and swc_layer_tail's (a row's 768 values spread over the
    4 waves in the accumulator layout, statistics exchanged through LDS).  Zero weights would multiply their output away, so fc1
    and fc2 are identities (F = 768, zero biases, Wo = 0): x_out = x + r16(gelu(r16(LN(x)))), r16 the operand format.  The bound
    is that of the ConvNeXt block above.  For the `huge` family the residual x ~ 1e15 hides y: those rows only have to come out
    finite here (the trailing LayerNorm of the same kernels is compared on them directly)."""
    ops = _ops()
    D, M = 768, LN_ROWS
    dt = torch.float16 if fmt == "f16" else torch.bfloat16
    x = vd.ln_rows(family, M, D, seed=4)
    w, b = vd.ln_affine(D, seed=4)
    zD, zw, eye = _d(torch.zeros(D)), _d(torch.zeros(D, D).to(dt)), _d(torch.eye(D).to(dt))
    xd = _d(x).clone()
    if kernel == "mlp_block":
        xo, _ = ops.mlp_block(xd, _d(w), _d(b), 1e-5, ops.mlp_pack(eye, eye), zD, zD, M=M, D=D, F=D)
    else:
        xo, _ = ops.layer_tail(_d(torch.zeros(M, D).to(torch.bfloat16)), xd, ops.layer_tail_pack(zw, eye, eye), zD, _d(w), _d(b), 1e-5,
                               zD, zD, M=M, D=D, F=D, operands=dt)
    y = vd.ln_ref(x, w, b, 1e-5)
    h = vd.gelu_ref(y)
    ref = x.double() + h
    e_t = vd.ln_torch_f32_err(x, w, b, 1e-5)
    tol = (1.13 * (4 * e_t + 1e-6 * (1 + y.abs()) + vd.ulp16(y, fmt)) + GELU_FAST + vd.ulp16(h, fmt) + 2.0 ** -23 * ref.abs())
    print(f"[value-domain] leading LayerNorm {kernel} {fmt} {family}: torch f32 max err {e_t:.3e}")
    _check(f"leading LN {kernel} {fmt} {family}", xo.cpu().double(), ref, tol)
    if family == "constant":   # y = b whatever the row: the residual rounding aside, nothing of the LayerNorm error term is needed
        hb = vd.gelu_ref(b).expand_as(ref)
        tol_b = 1.13 * (1e-6 * (1 + b.double().abs()) + vd.ulp16(b.double(), fmt)) + GELU_FAST + vd.ulp16(hb, fmt) + 2.0 ** -23 * ref.abs()
        _check(f"leading LN {kernel} {fmt} constant rows", xo.cpu().double(), x.double() + hb, tol_b)


# ------------------------------------------------------------------------------------------------------ 5. attention
@pytest.mark.parametrize("mode,tol", [("f32", 1e-5), ("bf16", 1.5e-2), ("f16s", 1e-5)])
@pytest.mark.parametrize("case", vd.ATT_CASES)
def test_attention_score_range(case, mode, tol):
    """Softmax over score ranges the randn tests never reach, through swc_attention (f32), and swc_attention16 (bf16 with its
    lazy rescale; split-f16).  Operands are exact in all three formats, so the three kernels see the same numbers; tolerances
    are those of test_attention / test_attention16, relative to max |v|.
    creeping_max: the bf16 kernel moves its reference maximum when a tile's maximum exceeds it by more than 8 / c_exp =
    8 ln 2 = 5.545 score units (p may exceed 1 by 2^8); the maximum grows by 4 per 128-key tile, so no single tile triggers
    the rescale and the third tile (8 above the first) does."""
    ops = _ops()
    B, H, T, lens = vd.ATT_B, vd.ATT_H, vd.ATT_T, list(vd.ATT_LENS)
    qkv = vd.attention_case(case)
    ld = _d(torch.tensor(lens, dtype=torch.int32))
    if mode == "f32":
        out = ops.attention(_d(qkv), ld, B, T, H).cpu().double()
    elif mode == "bf16":
        out = ops.attention(_d(qkv.to(torch.bfloat16)), ld, B, T, H).float().cpu().double()
    else:
        qd = ops.cast_f16s(_d(qkv.view(B * T, -1)), 3 * H * 64).view(B, T, -1)
        out = _unsplit(ops.attention(qd, ld, B, T, H), H * 64).view(B, T, H * 64)
    assert torch.isfinite(out).all()          # rows >= len included
    vmax = float(qkv[..., 2 * H * 64:].abs().max())
    for b, (L, ref) in enumerate(zip(lens, vd.attention_ref(qkv, lens, H))):
        if case == "equal_keys":
            mean_v = qkv[b, :L, 2 * H * 64:].double().mean(0)
            assert float((ref - mean_v).abs().max()) < 1e-12
        _check(f"attention {mode} {case} b={b}", out[b, :L], ref, torch.tensor(tol * vmax, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------- 6. mel log, FSQ
def test_mel_log_value_domain():
    """log10 with its 1e-10 floor from 0 and the smallest subnormal to 3e38, the per-utterance maximum and the max - 8 floor.
    Utterance 0 holds the whole sweep, utterance 1 only values at or under the floor (its maximum is the incoming -10... or
    the floor's own log), utterance 2 starts from -inf."""
    ops = _ops()
    B, T, n_mel, ld = 3, 4, 80, 96
    vals = vd.mel_values()
    mel = torch.zeros(B, T, ld)
    mel[0, :, :n_mel] = vals.repeat(T * n_mel // vals.numel()).view(T, n_mel)
    mel[1, :, :n_mel] = vals[:6].repeat(T * n_mel // 6 + 1)[:T * n_mel].view(T, n_mel)
    mel[2, :, :n_mel] = vals[[3, 7]].repeat(T * n_mel // 2).view(T, n_mel)
    umax0 = torch.tensor([-10.0, -10.0, float("-inf")])
    md, umax = _d(mel).clone(), _d(umax0).clone()
    ops.mel_logmax(md, ld, umax, B=B, T=T, n_mel=n_mel)
    lg, mx_ref = vd.mel_ref(mel[:, :, :n_mel], umax0)
    got = md[:, :, :n_mel].cpu()
    _check("mel log10", got.double(), lg, 1e-6 * (1 + lg.abs()))
    assert torch.equal(md[:, :, n_mel:].cpu(), mel[:, :, n_mel:])
    # the maximum the kernel left for swc_mel_final: between the two calls umax holds the order-preserving integer form its
    # atomicMax works on (the float's bits, magnitude bits inverted for negative numbers)
    bits = umax.cpu().view(torch.int32)
    kmax = torch.where(bits >= 0, bits, bits ^ 0x7FFFFFFF).view(torch.float32)
    mx = torch.maximum(got.amax(dim=(1, 2)), umax0)                     # exact: the maximum of the kernel's own logs
    assert torch.equal(kmax, mx)
    assert float((kmax.double() - mx_ref.double()).abs().sub(1e-6 * (1 + mx_ref.double().abs())).max()) <= 0   # and the float64 one
    out = ops.mel_final(md, ld, umax, B=B, T=T, n_mel=n_mel, ldo=ld).cpu()
    assert float(mx[1]) == -10.0 and float(mx[0]) > 38 and float(mx[2]) == 0.0
    want = (torch.maximum(got, (mx - 8.0).view(B, 1, 1)) + 4.0) / 4.0
    assert torch.equal(out[:, :, :n_mel], want)
    assert (out[:, :, n_mel:] == 0).all()


@pytest.mark.parametrize("levels", [(8, 7, 6, 6), (16, 3, 2, 9)])
def test_fsq_saturation(levels):
    """tanh saturation of swc_fsq_encode: +-0, +-20, +-88, +-1e30, +-inf and z = -shift (tanh(0), the rounding tie of even
    levels): codes and zq equal the float64-tanh statement bit for bit."""
    from simwhisper_codec_amd import spec
    ops = _ops()
    k12 = spec.fsq_constants(list(levels), 1e-3)
    z = vd.fsq_values(k12[8:12])
    T = z.shape[0]
    zq, codes = ops.fsq_encode(_d(z.view(1, T, 4)), 4, _d(torch.tensor([T], dtype=torch.int32)), k12, B=1, T=T, t_pad=16, G=1,
                               levels=levels)
    want_zq, want_idx = vd.fsq_ref(z, k12, levels)
    print(f"[value-domain] fsq {levels}: codes {codes[0, 0, :T].tolist()}")
    assert torch.equal(codes[0, 0, :T].cpu(), want_idx)
    assert torch.equal(zq[0, :T].cpu().view(torch.int32), want_zq.view(torch.int32))
    assert (codes[:, :, T:] == 0).all() and (zq[:, T:] == 0).all()
    n = 1
    for lv in levels:
        n *= lv
    assert int(want_idx.min()) >= 0 and int(want_idx.max()) < n
