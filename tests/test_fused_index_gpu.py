"""The attention kernels, the front half of swc_convnext_block and the M tail of the layer kernels on every branch of their index
arithmetic, through the C-ABI: tests/fused_index.py holds the cases, the float64 references, the predicates that name each
case's branches and the fault model; test_fused_index_cpu.py holds the tables to the branches and shows that the criteria
below catch each modelled fault.  Criteria: values of the valid rows against float64 within the tolerance the existing test
of the same form uses (fi.ATT_TOL, fi.CX_TOL, fi.TAIL_TOL: no new numbers); bit identities without any tolerance (packed =
padded, an utterance alone = the utterance in its batch, one head alone = the head among H, hostile rows as zeros change
nothing); and the memory contract: every output is a guarded window of tests/poison.py, packed buffers end at their last row.
Rows at and beyond lens[b] hold trap data in every case (fi.with_traps), lengths and row starts are always valid."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_index as fi  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
BOUNDARY_LENS = (1, 15, 16, 63, 64, 65, 127, 128, 129, 191, 192, 193)


def _ops():
    from simwhisper_codec_amd import ops
    return ops


def _d(t):
    return t.to(DEV)


def _unsplit(t, K, scale=64.0):
    """split-f16 [..., 2K] -> float64 [..., K]"""
    v = t.cpu().double().reshape(-1, K // 32, 2, 32)
    return ((v[:, :, 0] + v[:, :, 1]).reshape(-1, K) / scale).view(tuple(t.shape[:-1]) + (K,))


def _bits(t):
    t = t.cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


class Worst:
    """the worst err / tol of a test's cases (the pattern of test_stage_index_gpu.py): printed once, after every assertion"""

    def __init__(self, name):
        self.name, self.err, self.ratio, self.at = name, 0.0, 0.0, ""

    def check(self, what, err, tol):
        """assert err < tol (err: a float, the maximum of the checked rows)"""
        ratio = err / tol
        if ratio > self.ratio:
            self.err, self.ratio, self.at = err, ratio, what
        if not ratio < 1:
            self.report()
        assert ratio < 1, (self.name, what, f"err {err:.3e} tol {tol:.1e}")

    def report(self):
        print(f"[fused-index] {self.name}: worst err/tol {self.ratio:.3f} (err {self.err:.3e}) at {self.at}")


# ------------------------------------------------------------------------------------------------------------ attention
def _device_input(ops, form, qkv):
    """the f32 host tensor [.., T, 3D] as the form's kernel takes it"""
    if form in fi.ATT_BF16_SOURCE:
        return _d(qkv.bfloat16())
    if form == "f16s":
        W = qkv.shape[-1]
        return ops.cast_f16s(_d(qkv.reshape(-1, W)), W).view(tuple(qkv.shape[:-1]) + (2 * W,))
    return _d(qkv)


def _launch(ops, form, dev_in, lens, T, H, row_start=None):
    """one launch into a guarded window -> the raw output (padded [B, T, W] or packed [rows, W]); every row is written and
    nothing outside the window is"""
    D, B = H * 64, len(lens)
    dtype, W = {"f32": (torch.float32, D), "f32->f16s": (torch.float16, 2 * D), "bf16 legacy": (torch.bfloat16, D),
                "bf16": (torch.bfloat16, D), "f16s": (torch.float16, 2 * D)}[form]
    rows = None if row_start is None else fi.row_starts(lens, T)[1]
    out, check = poison.guarded((B, T, W) if row_start is None else (rows, W), dtype, device=DEV)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    rs_d = None if row_start is None else torch.tensor(row_start, dtype=torch.int32, device=DEV)
    ops.LEGACY_ATTENTION = form == "bf16 legacy"
    try:
        ops.attention(dev_in, lens_d, B, T, H, out=out, out_dtype=torch.float16 if form == "f32->f16s" else None,
                      row_start=rs_d, rows=rows)
    finally:
        ops.LEGACY_ATTENTION = False
    torch.cuda.synchronize()
    check()
    raw = out.contiguous()
    untouched = (raw.reshape(-1, W).view(torch.uint8) == poison.SENTINEL).all(dim=-1)
    assert not bool(untouched.any()), (form, "rows never written", int(untouched.sum()))
    return raw


def _f64(form, raw, H):
    return _unsplit(raw, H * 64) if raw.dtype == torch.float16 else raw.double().cpu()


_REF = {}


def _ref(name, form):
    key = (name, form in fi.ATT_BF16_SOURCE)
    if key not in _REF:
        c = fi.att_case(name)
        _REF[key] = fi.attn_ref(fi.source(fi.attn_input(name), form), c["lens"], c["T"], c["H"])
    return _REF[key]


@pytest.mark.parametrize("name", [c["name"] for c in fi.ATT_CASES])
@pytest.mark.parametrize("form", list(fi.ATT_FORMS))
def test_attention(form, name):
    ops = _ops()
    c = fi.att_case(name)
    T, lens, H = c["T"], c["lens"], c["H"]
    B, D, e = len(lens), H * 64, fi.eff_lens(c["lens"], c["T"])
    ok = fi.valid_mask(lens, T)
    w = Worst(f"attention {form} {name}")
    dev_in = _device_input(ops, form, fi.attn_input(name))
    raw = _launch(ops, form, dev_in, lens, T, H)
    got = _f64(form, raw, H)
    assert bool(torch.isfinite(got).all())
    # values of the valid rows against float64
    err = (got - _ref(name, form))[ok].abs()
    w.check("float64", float(err.max()), fi.ATT_TOL[form])
    if form == "f32->f16s":
        o32 = _launch(ops, "f32", dev_in, lens, T, H).double().cpu()
        w.check("the f32 form's output", float((got - o32)[ok].abs().max()), fi.F16S_VS_F32)
    # query blocks wholly beyond the length: zeros
    qb = fi.ATT_FORMS[form]["qb"]
    beyond = (torch.arange(T).view(1, T) // qb * qb) >= torch.tensor(e).view(-1, 1)
    assert bool((got[beyond] == 0).all())
    # the hostile rows as zeros: no bit of a valid row changes
    if T > 1:
        cold = _launch(ops, form, _device_input(ops, form, fi.with_traps(fi.attn_base(name), lens, T, H, zeros=True)), lens, T, H)
        assert torch.equal(_bits(cold)[ok], _bits(raw)[ok]), "rows at and beyond lens[b] change valid rows"
    # packed = padded, bit for bit; both packed buffers end at row sum(lens)
    if form in fi.ATT_PACKED:
        rs, total = fi.row_starts(lens, T)
        packed_in = fi.pack(dev_in, lens, T).contiguous()
        assert packed_in.shape[0] == total
        pk = _launch(ops, form, packed_in, lens, T, H, row_start=rs)
        assert torch.equal(_bits(pk), _bits(fi.pack(raw, lens, T))), "packed differs from padded"
    # an utterance alone (T = its length) = the utterance in its batch
    pick = [b for b in range(B) if e[b] > 0 and (B <= 8 or e[b] in BOUNDARY_LENS)]
    seen = set()
    for b in pick:
        if e[b] in seen or len(seen) == len(BOUNDARY_LENS):
            continue
        seen.add(e[b])
        alone = _launch(ops, form, dev_in[b:b + 1, :e[b]].contiguous(), (e[b],), e[b], H)
        assert torch.equal(_bits(alone)[0], _bits(raw)[b, :e[b]]), (b, e[b], "alone differs from batched")
    # the last head alone = the last head among H
    if H > 1:
        h, hw = H - 1, dev_in.shape[-1] // (3 * H)
        one = torch.cat([dev_in[..., (i * H + h) * hw:(i * H + h + 1) * hw] for i in range(3)], dim=-1).contiguous()
        oh = _launch(ops, form, one, lens, T, 1)
        ow = raw.shape[-1] // H
        assert torch.equal(_bits(oh)[ok], _bits(raw[..., h * ow:(h + 1) * ow])[ok]), "one head alone differs from the head among H"
    w.report()


@pytest.mark.parametrize("form", list(fi.ATT_FORMS))
def test_attention_spike_on_the_last_valid_key_and_the_first_masked_one(form):
    """key len - 1 carries a score spike and key len (masked) the same row: the valid rows equal, bit for bit, the run in which
    row len is zeros, and float64"""
    ops = _ops()
    hot, cold = fi.spike_input()
    T, n, H = fi.SPIKE["T"], fi.SPIKE["n"], fi.SPIKE["H"]
    a = _launch(ops, form, _device_input(ops, form, hot), (n,), T, H)
    b = _launch(ops, form, _device_input(ops, form, cold), (n,), T, H)
    assert torch.equal(_bits(a)[0, :n], _bits(b)[0, :n])
    ref = fi.attn_ref(fi.source(hot, form), (n,), T, H)
    w = Worst(f"attention {form} spike")
    w.check("float64", float((_f64(form, a, H) - ref)[0, :n].abs().max()), fi.ATT_TOL[form])
    w.report()


def test_attention_refuses_65536_utterances():
    ops = _ops()
    from simwhisper_codec_amd._lib import SwcError
    B = 65536
    lens = torch.ones(B, dtype=torch.int32, device=DEV)
    x = torch.zeros(B, 1, 192, device=DEV)
    for form in fi.ATT_FORMS:
        ops.LEGACY_ATTENTION = form == "bf16 legacy"
        try:
            with pytest.raises(SwcError):
                ops.attention(_device_input(ops, form, x.cpu()), lens, B, 1, 1, out_dtype=torch.float16 if form == "f32->f16s" else None)
        finally:
            ops.LEGACY_ATTENTION = False


# ------------------------------------------------------------------------------------------------------- ConvNeXt block
@pytest.mark.parametrize("case", fi.BLOCK_CASES, ids=lambda c: f"B{c['B']}-T{c['T']}-I{c['I']}" + ("" if c["t_limit"] is None else "-limit"))
def test_convnext_block(case):
    """both operand types against float64 (e_ref of test_convnext_block_fused / _f16_operands) and, for bf16, against the two
    kernels the block replaces (e_pair); with t_limit the frames below t_limit[b] - 3, and a tile that returns at once leaves
    its rows as they were; x is read only and nothing outside x_out is written"""
    ops = _ops()
    B, T, I, lim = case["B"], case["T"], case["I"], case["t_limit"]
    C, M = fi.CX_C, B * T
    t = fi.block_input(B, T, I)
    x0 = t["x"]
    xd, w7, db, lw, lb, b1, b2, gam = (_d(t[k]) for k in ("x", "w7", "db", "lw", "lb", "b1", "b2", "gam"))
    lim_d = None if lim is None else torch.tensor(lim, dtype=torch.int32, device=DEV)
    rows, skipped = fi.block_check_rows(B, T, lim), fi.block_skipped_rows(B, T, lim)
    assert bool(rows.any())
    w = Worst(f"convnext_block B={B} T={T} I={I} t_limit={lim}")
    for operands, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        ws = ops.convnext_pack(_d(t["w1"]).to(dt), _d(t["w2"]).to(dt), gam)
        out, check = poison.guarded((B, T, C), torch.float32, device=DEV)
        ops.convnext_block(xd, out, w7, db, lw, lb, 1e-6, ws, b1, b2, gam, B=B, T=T, C_=C, I=I, t_limit=lim_d, operands=dt)
        torch.cuda.synchronize()
        check()
        assert torch.equal(xd.cpu(), x0)
        raw = out.contiguous().view(M, C)
        left = (raw.view(torch.uint8) == poison.SENTINEL).all(dim=-1).cpu()
        assert torch.equal(left, skipped), "the tiles that return at once are not the ones the need loop names"
        got = raw.double().cpu()
        assert bool(torch.isfinite(got[~skipped]).all())
        ref = fi.block_ref(B, T, I, operands)
        scale = float((ref - x0.double().view(M, C)).abs().max())
        w.check(f"{operands} e_ref", float((got - ref)[rows].abs().max()) / scale, fi.CX_TOL[operands]["e_ref"])
        if operands == "bf16":
            y = ops.dwconv7_ln(xd, w7, db, lw, lb, 1e-6, B=B, T=T, C_=C, out_dtype=torch.bfloat16)
            x2 = xd.clone()
            ops.convnext_mlp(y, ws, b1, b2, gam, x2, M=M, C_=C, I=I)
            w.check("bf16 e_pair", float((got - x2.double().cpu().view(M, C))[rows].abs().max()) / scale, fi.CX_TOL["bf16"]["e_pair"])
    w.report()


# ----------------------------------------------------------------------------------------------------------- layer tail
@pytest.mark.parametrize("M", fi.TAIL_M)
def test_layer_tail_and_mlp_block_m_tail(M):
    """swc_layer_tail and swc_mlp_block at M = 1, 63, 64, 65, 129 (64-token tiles; rows beyond M are computed on a copy of the
    last row and never stored), F = 256: the reference and the bounds of test_layer_tail_fused / test_mlp_block_fused, the
    outputs guarded windows"""
    ops = _ops()
    D, F_ = fi.TAIL_D, fi.TAIL_F
    t = {k: _d(v) for k, v in fi.tail_input(M).items()}
    x0 = fi.tail_input(M)["x"].double()
    w = Worst(f"layer tail M={M}")
    for with_attn in (True, False):
        ref = fi.tail_ref(M, with_attn)
        scale = float((ref - x0).abs().max())
        xo, chk_x = poison.guarded((M, D), torch.float32, device=DEV)
        yn, chk_y = poison.guarded((M, D), torch.bfloat16, device=DEV)
        x2 = t["x"].clone()
        ws = ops.mlp_pack(t["w1"], t["w2"])
        if with_attn:
            wts = ops.layer_tail_pack(t["wo"], t["w1"], t["w2"])
            ops.layer_tail(t["att"], t["x"], wts, t["bo"], t["lw"], t["lb"], 1e-5, t["b1"], t["b2"], M=M, D=D, F=F_, x_out=xo,
                           next_ln=(t["nw"], t["nb"]), y_next=yn)
            ops.gemm(t["att"], t["wo"], M, D, D, bias=t["bo"], residual=x2, out=x2)
        else:
            ops.mlp_block(t["x"], t["lw"], t["lb"], 1e-5, ws, t["b1"], t["b2"], M=M, D=D, F=F_, x_out=xo, next_ln=(t["nw"], t["nb"]),
                          y_next=yn)
        if with_attn:                                  # the launches it replaces, as the two existing tests run them
            ops.mlp_block(x2, t["lw"], t["lb"], 1e-5, ws, t["b1"], t["b2"], M=M, D=D, F=F_)
        else:
            y = ops.layernorm(t["x"], t["lw"], t["lb"], 1e-5, B=1, t_in=M, C_=D, out_dtype=torch.bfloat16)
            hh = ops.gemm(y.view(M, D), t["w1"], M, F_, D, bias=t["b1"], act=ops.ACT_GELU, out_dtype=torch.bfloat16)
            ops.gemm(hh, t["w2"], M, D, F_, bias=t["b2"], residual=x2, out=x2)
        torch.cuda.synchronize()
        chk_x()
        chk_y()
        assert torch.equal(t["x"].cpu(), fi.tail_input(M)["x"])
        got, two = xo.contiguous().double().cpu(), x2.double().cpu()
        assert bool(torch.isfinite(got).all())
        what = "layer_tail" if with_attn else "mlp_block"
        e_ref, e_two, e_two_ref = (float(v.abs().max()) / scale for v in (got - ref, got - two, two - ref))
        w.check(f"{what} e_ref", e_ref, fi.TAIL_TOL["e_ref"])
        w.check(f"{what} e_ref against the unfused launches'", e_ref, 2.0 * e_two_ref + 1e-4)
        w.check(f"{what} e_two", e_two, fi.TAIL_TOL["e_two"])
        want = ops.layernorm(xo.contiguous(), t["nw"], t["nb"], 1e-5, B=1, t_in=M, C_=D, out_dtype=torch.bfloat16).view(M, D)
        assert torch.equal(yn.contiguous(), want)
    w.report()
