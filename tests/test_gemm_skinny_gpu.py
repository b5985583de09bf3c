"""The skinny geometry of swc_gemm (csrc/swc_gemm_skinny.hip: 64 x 128 tile, four waves side by side along N, a ring of LDS
stages filled through running per-lane pointers) against the other geometries, and against float64.

Every case computes rows [0, M) twice without any switch: alone, at a shape swc_gemm_plan reports as skinny, and as the head of
a call with enough rows that the plan reports another geometry: the 8-wave tile where the chooser can reach it (N >= 256), the
4-wave 128 x 128 tile for the narrower outputs (below 256 columns no row count takes the 8-wave tile).  Both plans are asserted,
and the two results must be equal bit for bit: an output's accumulation chain and epilogue do not depend on the geometry.
f32 outputs are then held to the float64 bounds of tests/test_kernels_gpu.py (test_gemm_f16s_is_f32_class: 2e-6 and 4 x the
exact-f32 kernel's error + 2e-7; test_gemm_plain, bf16: 2e-5), split-f16 outputs to the 3e-6 of test_gemm_f16s_is_f32_class and
bf16 outputs to the 8e-3 of test_gemm_big_tile_bf16.

The geometry takes launches with the implicit-conv staging only (plain GEMMs measured faster on the plain staging and keep it,
profiles/gemm_skinny_ab.txt).  The taps = 1 cases are therefore launches with a row remap, one utterance of t_in = M + 1 input
rows of which the first t_out = M are computed: one tap, no padding, the conv staging; the unused input row is NaN.

All operands sit in buffers whose rows in front, rows behind and leading-dimension padding are NaN, outputs in guarded windows
(poison.guarded) whose previous content is NaN: a read beyond a row or a column shows in the result, a store outside the window
in the guard bands.
"""
import pytest
import torch

import poison

pytestmark = pytest.mark.gpu
DEV = "cuda"
SA, SW = 64.0, 2.0 ** 14          # split-f16 operand scales (activations, weights), as in test_gemm_f16s_is_f32_class
BK = {"f16s": 32, "bf16": 64}     # logical elements of K per slice


def _ops():
    from simwhisper_codec_amd import ops
    return ops


def _embed(data, ld, before, after):
    """data [rows, width] inside an allocation of (before + rows + after) rows of ld elements, NaN everywhere else"""
    rows, width = data.shape
    back = torch.full(((before + rows + after) * ld,), float("nan"), dtype=data.dtype, device=DEV)
    view = back.as_strided((rows, width), (ld, 1), before * ld)
    view.copy_(data)
    return view


def _operand(x, kind, K, scale):
    """f32 [rows, K logical] on the device -> (operand tensor, storage columns per logical column)"""
    if kind == "bf16":
        return x.to(torch.bfloat16), 1
    return _ops().cast_f16s(x, K, scale=scale), 2


def _unsplit(y, cols, scale):
    y = y.cpu().double().view(y.shape[0], cols // 32, 2, 32)
    return (y[:, :, 0] + y[:, :, 1]).reshape(y.shape[0], cols) / scale


def _plan_args(kind, M, N, K, taps, dil, t):
    from simwhisper_codec_amd import _lib
    a = _lib.GemmArgs()
    a.A = a.W = a.C = 0x10000
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc = M, N, K, K, taps * K, N
    a.taps, a.dil, a.stride, a.pad = taps, dil, 1, dil * (taps - 1) // 2
    a.t_out = t if taps > 1 else M
    a.t_in = t if taps > 1 else M + 1
    a.a_dtype = a.c_dtype = {"bf16": _lib.BF16, "f16s": _lib.F16S}[kind]
    return a


def _threshold(kind, taps=1):
    """smallest K (a multiple of the slice) whose taps x K takes the skinny geometry at 640 rows x 128 columns"""
    ops = _ops()
    t = 128 if taps > 1 else None
    for K in range(BK[kind], 4097, BK[kind]):
        if ops.gemm_plan(_plan_args(kind, 640, 128, K, taps, 1, t))["skinny"]:
            return K
    raise AssertionError("no reduction length up to 4096 takes the skinny geometry")


def _big_rows(N, unit):
    """rows (a multiple of `unit`) from which the chooser leaves the few-row regime: 96 tiles of 256 x 256 for the 8-wave
    tile, 384 tiles of 128 x 128 below 256 columns"""
    rows = 96 // (-(-N // 256)) * 256 if N >= 256 else 384 // (-(-N // 128)) * 128
    return -(-rows // unit) * unit


# kind, M (plain) or (B, t) (taps = 7), N, K ("thr": at the selection threshold, "thr+1": one slice above it), dil, epilogue
#   epilogue: "f32-inplace" (f32 output, bias, residual == out), "16" (operand-type output, bias), "16-gelu"
PLAIN = [
    ("f16s", 512, 128, "thr", "f32-inplace"),
    ("f16s", 577, 160, "thr+1", "16-gelu"),
    ("f16s", 641, 512, 3072, "f32-inplace"),
    ("f16s", 577, 32, "thr", "16"),
    ("bf16", 512, 160, "thr+1", "16-gelu"),
    ("bf16", 641, 32, "thr", "f32-inplace"),
    ("bf16", 577, 512, 3072, "16"),
    ("bf16", 641, 128, "thr", "f32-inplace"),
]
CONV = [
    ("f16s", (3, 189), 512, 1, "f32-inplace"),
    ("f16s", (5, 125), 160, 3, "16-gelu"),
    ("f16s", (4, 189), 128, 9, "f32-inplace"),
    ("bf16", (5, 125), 512, 9, "16"),
    ("bf16", (3, 189), 32, 1, "f32-inplace"),
    ("bf16", (6, 125), 160, 3, "16-gelu"),
]


def _reference(A, W, bias, taps, dil, t):
    """float64 A (*) W^T + bias on the host; A [M, K], W [N, taps * K] (tap-major), utterances of t rows"""
    A, W = A.double().cpu(), W.double().cpu()
    M, K = A.shape
    if taps == 1:
        return A @ W.T + bias.double().cpu()
    B, pad = M // t, dil * (taps - 1) // 2
    x = torch.zeros(B, t + 2 * pad, K, dtype=torch.float64)
    x[:, pad:pad + t] = A.view(B, t, K)
    out = torch.zeros(B, t, W.shape[0], dtype=torch.float64)
    for tap in range(taps):
        out += x[:, tap * dil:tap * dil + t] @ W[:, tap * K:(tap + 1) * K].T
    return out.view(M, -1) + bias.double().cpu()


def _rel(a, b):
    return float((a.double().cpu() - b).abs().max() / (b.abs().max() + 1e-30))


def _run_case(kind, M, N, K, taps, dil, t, epi, seed):
    ops = _ops()
    unit = t if taps > 1 else 1
    Mb = _big_rows(N, unit)
    assert Mb > M
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).to(DEV)
    W = (torch.randn(N, taps * K, generator=g) * 0.03).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    res = torch.randn(M, N, generator=g).to(DEV)
    torch.manual_seed(seed)
    A_big = torch.cat([A, torch.randn(Mb - M, K, device=DEV)])
    res_big = torch.cat([res, torch.randn(Mb - M, N, device=DEV)])
    sa, sw = (SA, SW) if kind == "f16s" else (1.0, 1.0)
    Wd, cw = _operand(W, kind, taps * K, sw)
    lpad = 8 if kind == "bf16" else 32          # leading-dimension padding: one 16-byte step (bf16) / one 32-block (split-f16)
    w = _embed(Wd, cw * (taps * K + lpad), 1, 260)
    out_dt = torch.float32 if epi == "f32-inplace" else (torch.float16 if kind == "f16s" else torch.bfloat16)
    co = 2 if out_dt == torch.float16 else 1
    ldc = N + (32 if out_dt == torch.float16 else 16 // torch.empty(0, dtype=out_dt).element_size())
    outs, plans = [], []
    for rows, a_src, r_src in ((M, A, res), (Mb, A_big, res_big)):
        conv = dict(taps=taps, dil=dil, pad=dil * (taps - 1) // 2, t_in=t, t_out=t) if taps > 1 else dict(t_in=rows + 1, t_out=rows)
        Ad, ca = _operand(a_src, kind, K, sa)
        a = _embed(Ad, ca * (K + lpad), 3, 300)
        c, check = poison.guarded((rows, co * N), out_dt, ld=co * ldc, device=DEV)
        kw = dict(out=c, lda=K + lpad, ldw=taps * K + lpad, ldc=ldc, bias=bias, alpha=1.0 / (sa * sw), **conv)
        if epi == "f32-inplace":
            c.copy_(r_src)
            kw.update(residual=c, ldr=ldc)
        else:
            c.fill_(float("nan"))
            kw.update(act=ops.ACT_GELU if epi == "16-gelu" else ops.ACT_NONE, out_scale=64.0 if out_dt == torch.float16 else 1.0)
        plans.append(ops.gemm_call_plan(a, w, rows, N, K, **kw))
        ops.gemm(a, w, rows, N, K, **kw)
        torch.cuda.synchronize()
        check()
        outs.append(c[:M].clone())
    small, big = plans
    assert small["skinny"] == 1 and (small["tile_m"], small["tile_n"], small["waves"], small["plain"]) == (64, 128, 4, 0), small
    assert small["grid"] == small["n_tiles_m"] * small["n_tiles_n"], small
    assert big["skinny"] == 0 and (big["waves"] == 8 if N >= 256 else (big["tile_m"], big["waves"]) == (128, 4)), big
    assert not torch.isnan(outs[0].float()).any()
    assert torch.equal(outs[0], outs[1]), "the skinny geometry and the LDS-staged geometry differ"
    # ---- float64
    ref = _reference(A if kind == "f16s" else A.to(torch.bfloat16), W if kind == "f16s" else W.to(torch.bfloat16), bias, taps, dil, t)
    if epi == "f32-inplace":
        ref = ref + res.double().cpu()
        err = _rel(outs[0], ref)
        if kind == "bf16":
            assert err < 2e-5, err
        else:
            c32 = res.clone()
            conv = dict(taps=taps, dil=dil, pad=dil * (taps - 1) // 2, t_in=t, t_out=t) if taps > 1 else {}
            ops.gemm(A, W, M, N, K, out=c32, bias=bias, residual=c32, ldw=taps * K, **conv)
            e32 = _rel(c32, ref)
            assert err < 2e-6 and err < 4 * e32 + 2e-7, (err, e32)
    else:
        if epi == "16-gelu":
            ref = torch.nn.functional.gelu(ref)
        if kind == "f16s":
            assert float((_unsplit(outs[0], N, 64.0) - ref).abs().max() / ref.abs().max()) < 3e-6
        else:
            assert _rel(outs[0].float(), ref) < 8e-3


@pytest.mark.parametrize("kind,M,N,K,epi", PLAIN, ids=lambda v: str(v))
def test_skinny_plain_equals_lds_geometry(kind, M, N, K, epi):
    thr = _threshold(kind)
    K = {"thr": thr, "thr+1": thr + BK[kind]}.get(K, K)
    _run_case(kind, M, N, K, 1, 1, None, epi, seed=M + N + K)


@pytest.mark.parametrize("kind,Bt,N,dil,epi", CONV, ids=lambda v: str(v))
def test_skinny_conv7_equals_lds_geometry(kind, Bt, N, dil, epi):
    """taps = 7, pad = 3 dil: tiles cross utterance boundaries (t = 189, 125 against 64-row tiles), padded taps at both ends"""
    B, t = Bt
    K = _threshold(kind, taps=7)
    _run_case(kind, B * t, N, K, 7, dil, t, epi, seed=B * t + N + dil)


def test_threshold_is_a_threshold():
    """one slice below the selection threshold the 2 x 2-wave 64-row geometry is kept; the threshold lies in the range the
    design gives (512 .. 3072 logical elements of taps x K)"""
    ops = _ops()
    for kind in ("f16s", "bf16"):
        thr = _threshold(kind)
        assert 512 <= thr <= 3072, thr
        below = ops.gemm_plan(_plan_args(kind, 640, 128, thr - BK[kind], 1, 1, None))
        assert below["skinny"] == 0 and (below["tile_m"], below["waves"], below["slots"]) == (64, 4, 512), below
        plain = _plan_args(kind, 640, 128, 3072, 1, 1, None)
        plain.t_in = plain.t_out
        assert ops.gemm_plan(plain)["skinny"] == 0 and ops.gemm_plan(plain)["plain"] == 1       # plain GEMMs keep the plain staging
        assert _threshold(kind, taps=7) == -(-thr // (7 * BK[kind])) * BK[kind]
