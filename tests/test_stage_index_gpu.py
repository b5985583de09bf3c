"""The stage kernels of csrc/swc_pointwise.hip on every branch of their index arithmetic, against float64 (or exactly, where a
kernel only copies or the statement is exact): tests/stage_index.py holds the cases, the references and the predicates that
name each case's branches; test_stage_index_cpu.py holds the table to those branches.  The value sweeps live in
test_value_domain_gpu.py and the memory contract in test_memory_contract_gpu.py; the shapes here are the smallest that reach
a branch."""
import pytest
import torch

import stage_index as si
import value_domain as vd

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16s": torch.float16}
BF16_U = 2.0 ** -8            # one bf16 rounding (8 significant bits, round to nearest even)


def _ops():
    from simwhisper_codec_amd import ops
    return ops


def _d(t):
    return t.to(DEV)


def _unsplit(t, K, scale=64.0):
    """split-f16 [rows, 2K] -> float64 [rows, K]"""
    v = t.cpu().double().view(-1, K // 32, 2, 32)
    return (v[:, :, 0] + v[:, :, 1]).reshape(-1, K) / scale


class Worst:
    """the worst err / tol of a test's cases: printed once, after every case has been asserted"""

    def __init__(self, name):
        self.name, self.err, self.ratio, self.at = name, 0.0, 0.0, ""

    def check(self, what, got, ref, tol):
        """assert |got - ref| <= tol element by element (float64 host tensors)"""
        assert torch.isfinite(got).all(), (self.name, what)
        err = (got - ref).abs()
        tol = tol if torch.is_tensor(tol) else torch.full_like(err, tol)
        rel = torch.where(err <= tol, err / tol.clamp(min=1e-300), torch.full_like(err, float("inf")))   # (0 <= 0 passes)
        rel = torch.where(tol > 0, err / tol.clamp(min=1e-300), rel)
        ratio = float(rel.max()) if err.numel() else 0.0
        if ratio > self.ratio:
            self.err, self.ratio, self.at = float(err.flatten()[int(rel.argmax())]), ratio, what
        self.err_max = max(getattr(self, "err_max", 0.0), float(err.max()) if err.numel() else 0.0)
        if ratio > 1:
            self.report()
        assert ratio <= 1, (self.name, what, f"err/tol {ratio:.3f}")

    def report(self):
        print(f"[stage-index] {self.name}: max |err| {getattr(self, 'err_max', 0.0):.3e}; worst err/tol {self.ratio:.3f} "
              f"(err {self.err:.3e}) at {self.at}")


# ----------------------------------------------------------------------------------------------------------- mel_frames
@pytest.mark.parametrize("n_pad", si.MF_NPAD)
def test_mel_frames(n_pad):
    """Twelve lengths from 0 to n_pad in one launch, at the product's T (the last frame reflects at n_pad) and at the largest T
    the launcher accepts, each with wav addressed three ways: rows on 16-byte boundaries (interior quads are one load), ld_wav
    = n_pad + 1, and a view one float into its buffer (both element-wise).  The kernel copies: equality, and the three ways
    agree bit for bit.  Samples at and beyond n[b] hold 7.0, the reference zeros."""
    ops = _ops()
    wav0, n = si.frames_input(n_pad)
    B = len(n)
    nd = _d(torch.tensor(n, dtype=torch.int32))
    filled = wav0.clone()
    for b, nb in enumerate(n):
        filled[b, nb:] = si.MF_FILL
    for T in (si.frames_t_product(n_pad), si.frames_t_max(n_pad)):
        ref = si.frames_ref(wav0, n, n_pad, T)
        got = {}
        for way in si.MF_WAYS:
            off, ld = si.frames_layout(way, n_pad)
            buf = torch.full((off + B * ld,), si.MF_FILL, device=DEV)
            wav = buf[off:].view(B, ld)[:, :n_pad]
            wav.copy_(filled)
            assert (wav.data_ptr() % 16 == 0 and wav.stride(0) % 4 == 0) == si.frames_vec_ok(off, ld)
            got[way] = ops.mel_frames(wav, nd, n_pad, B=B, T=T).cpu()
            assert got[way].shape == (B, T, 400)
            assert torch.equal(got[way], ref), (T, way, [b for b in range(B) if not torch.equal(got[way][b], ref[b])])
        assert torch.equal(got["aligned"], got["ld_odd"]) and torch.equal(got["aligned"], got["offset1"])
        assert bool((got["aligned"][0] == 0).all()) and bool(got["aligned"][-1].any())


# -------------------------------------------------------------------------------------------------------- mel_power
def test_mel_power():
    """|X|^2 as the kernel states it: m = sqrtf(fl(fl(re re) + fl(im im))), v = fl(m m).  Five float32 roundings, each a factor
    (1 + d) with |d| <= 2^-24: both products and their sum (positive terms: the sum's relative error is at most the larger
    term's, times its own rounding) give P (1 + d)^2, the correctly rounded square root sqrt(P) (1 + d)^2, its square
    P (1 + d)^4 and the rounding of that product P (1 + d)^5: |v - P| <= ((1 + 2^-24)^5 - 1) P = 2.98e-7 P, element by
    element (randn inputs: no intermediate is subnormal).  Columns at and beyond 201 are exact zeros."""
    ops = _ops()
    w = Worst("mel_power")
    for c in si.power_cases():
        rows, ld, ldp = c["rows"], c["ld"], c["ldp"]
        dft = torch.randn(rows, ld, generator=si._g("power", rows, ld))
        pw = ops.mel_power(_d(dft), ld, rows, ldp).cpu()
        ref = si.power_ref(dft)
        assert float(ref.min()) > 1e-30
        w.check(f"rows={rows} ld={ld} ldp={ldp}", pw[:, :201].double(), ref, si.POWER_REL * ref)
        assert pw.shape == (rows, ldp) and bool((pw[:, 201:] == 0).all())
        assert float((pw[:, :201].double() - ref).abs().max() / ref.max()) < 1e-6       # the bound of test_mel_frames_and_final
    w.report()


# ------------------------------------------------------------------------------------------------ mel_logmax + mel_final
@pytest.mark.parametrize("case", si.logmax_cases(), ids=lambda c: f"{c['name']}-from{c['umax0']}")
def test_mel_logmax_and_final(case):
    """2 and 3 workgroups per utterance (one atomicMax each), every loop slot of a thread, and one strictly larger value per
    utterance planted where a wrong stride, loop bound or workgroup offset would miss it; the maximum starts from -10 and from
    -inf, and is negative in the last case (the `i ^ 0x7fffffff` side of the ordered-int map decides).  The stored maximum
    equals the maximum of the kernel's own logs exactly and float64 to 1e-6 (1 + |ref|); the padding columns stay as they
    were; swc_mel_final at ldo = n_mel, 96 and 97 equals the float32 statement exactly (f32) and to one bf16 rounding."""
    ops = _ops()
    B, T, n_mel, ld = 3, case["T"], case["n_mel"], case["ld"]
    mel = si.logmax_input(case["name"], T, n_mel, ld, case["peaks"], case["negative"])
    umax0 = torch.full((B,), case["umax0"])
    md, umax = _d(mel).clone(), _d(umax0).clone()
    ops.mel_logmax(md, ld, umax, B=B, T=T, n_mel=n_mel)
    lg, mx_ref = vd.mel_ref(mel[:, :, :n_mel], umax0)
    got = md[:, :, :n_mel].cpu()
    w = Worst(f"mel_logmax {case['name']} from {case['umax0']}")
    w.check("log10", got.double(), lg, 1e-6 * (1 + lg.abs()))
    assert torch.equal(md[:, :, n_mel:].cpu(), mel[:, :, n_mel:])
    bits = umax.cpu().view(torch.int32)           # the order-preserving integer form (test_mel_log_value_domain)
    kmax = torch.where(bits >= 0, bits, bits ^ 0x7FFFFFFF).view(torch.float32)
    mx = torch.maximum(got.amax(dim=(1, 2)), umax0)
    assert torch.equal(kmax, mx), (kmax.tolist(), mx.tolist())
    flat = got.reshape(B, -1)
    for b, p in enumerate(case["peaks"]):
        assert float(kmax[b]) == float(flat[b, p]) and int(flat[b].argmax()) == p
    w.check("maximum", kmax.double(), mx_ref.double(), 1e-6 * (1 + mx_ref.double().abs()))
    assert bool((kmax < 0).all()) == case["negative"]
    want = (torch.maximum(got, (mx - 8.0).view(B, 1, 1)) + 4.0) / 4.0
    assert bool((got < (mx - 8.0).view(B, 1, 1)).any()) == case["negative"]      # the max - 8 floor binds in the negative case
    for ldo in si.final_ldo(n_mel):
        out = ops.mel_final(md, ld, umax, B=B, T=T, n_mel=n_mel, ldo=ldo).cpu()
        assert out.shape == (B, T, ldo) and torch.equal(out[:, :, :n_mel], want) and bool((out[:, :, n_mel:] == 0).all())
        o16 = ops.mel_final(md, ld, umax, B=B, T=T, n_mel=n_mel, ldo=ldo, out_dtype=torch.bfloat16).cpu()
        assert o16.dtype == torch.bfloat16 and bool((o16[:, :, n_mel:] == 0).all())
        w.check(f"mel_final bf16 ldo={ldo}", o16[:, :, :n_mel].double(), want.double(), BF16_U * want.double().abs())
    w.report()


# ---------------------------------------------------------------------------------------------------------------- snake
@pytest.mark.parametrize("case", si.SNAKE_CASES, ids=lambda c: f"C{c['C']}-{c['out']}")
def test_snake_aa(case):
    """Every T from 1 to 35: both sides of the interior condition of the first three interior strips (T = 18 / 19, 26 / 27,
    34 / 35) and every partial last strip, one channel block and two with a tail.  References and tolerances as in
    test_snake_aa / test_snake_aa_bf16_values / test_snake_argument_domain: 1e-5 (f32, split-f16), 2^-8 |ref| + 1e-5 (bf16)."""
    ops = _ops()
    C_, out_dtype = case["C"], DT[case["out"]]
    f = vd.kaiser_sinc12().tolist()
    w = Worst(f"snake_aa C={C_} {case['out']}")
    for T in si.SNAKE_T:
        x, al, be, ref = si.snake_input(C_, T)
        out = ops.snake_aa(_d(x.transpose(1, 2).contiguous()), _d(al), _d(be), f, B=2, T=T, C_=C_, out_dtype=out_dtype)
        if case["out"] == "f16s":
            assert out.shape == (2, T, 2 * C_)
            got = _unsplit(out.view(2 * T, 2 * C_), C_).view(2, T, C_)
        else:
            assert out.shape == (2, T, C_) and out.dtype == out_dtype
            got = out.float().cpu().double()
        tol = BF16_U * ref.abs() + 1e-5 if case["out"] == "bf16" else torch.full_like(ref, 1e-5)
        w.check(f"T={T}", got, ref, tol)
    w.report()


# --------------------------------------------------------------------------------------------------------------- col2im
def _col2im(ops, C_, ldo, s, T, t_out, dtype):
    y3, bias = si.col2im_input(C_, T)
    return ops.deconv_col2im(_d(y3), _d(bias), B=2, T=T, C_=C_, s=s, t_out=t_out, ldo=ldo, out_dtype=dtype).cpu()


@pytest.mark.parametrize("s", si.CI_S)
@pytest.mark.parametrize("C_,ldo", si.CI_SHAPES)
def test_deconv_col2im(C_, ldo, s):
    """The scalar kernel (C or ldo no multiple of 4) and the 4-channel one, strides 1 to 4, T = 1, 2, 17, and t_out = 1, 2, the
    product's crop and the full (T - 1) s + 3, on random taps (no GEMM in front): float64 three-tap sum to 1e-5 (f32), one
    bf16 rounding on top (bf16); the columns from C to ldo are zeros."""
    ops = _ops()
    w = Worst(f"deconv_col2im C={C_} ldo={ldo} s={s}")
    for T in si.CI_T:
        y3, bias = si.col2im_input(C_, T)
        full = si.col2im_ref(y3, bias, s, (T - 1) * s + 3)
        for t_out in si.col2im_t_outs(T, s):
            ref = full[:, :t_out]
            for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
                out = _col2im(ops, C_, ldo, s, T, t_out, dtype)
                assert out.shape == (2, t_out, ldo) and out.dtype == dtype and bool((out[:, :, C_:] == 0).all())
                tol = torch.full_like(ref, 1e-5) if name == "f32" else 1e-5 + BF16_U * (ref.abs() + 1e-5)
                w.check(f"T={T} t_out={t_out} {name}", out[:, :, :C_].double(), ref, tol)
    w.report()


@pytest.mark.parametrize("s", si.CI_S)
@pytest.mark.parametrize("C_,ldo", si.CI_BITEQ)
def test_deconv_col2im_kernels_agree(C_, ldo, s):
    """C % 4 == 0: the 4-channel kernel (ldo % 4 == 0) and the scalar one (ldo + 1) add bias and taps in the same order, so the
    first C columns are the same bits"""
    ops = _ops()
    assert si.col2im_kernel(C_, ldo) == "vec4" and si.col2im_kernel(C_, ldo + 1) == "scalar"
    for T in si.CI_T:
        for t_out in si.col2im_t_outs(T, s):
            for dtype in (torch.float32, torch.bfloat16):
                a, b = _col2im(ops, C_, ldo, s, T, t_out, dtype), _col2im(ops, C_, ldo + 1, s, T, t_out, dtype)
                bits = torch.int32 if dtype == torch.float32 else torch.int16
                assert torch.equal(a[:, :, :C_].contiguous().view(bits), b[:, :, :C_].contiguous().view(bits)), (T, t_out, dtype)


# ---------------------------------------------------------------------------------------------------------------- ISTFT
def test_istft_ola():
    """T = 1 .. 9: fewer than four overlapping frames and both clamps of the frame window (T <= 4), then the steady state,
    against the fold-based statement in float64; 1e-4 as in test_istft"""
    ops = _ops()
    wsq = _d((torch.hann_window(640, dtype=torch.float64) ** 2).float())
    w = Worst("istft_ola")
    for T in si.OLA_T:
        fr = si.ola_input(T)
        wav = ops.istft_ola(_d(fr), wsq, B=2, T=T).cpu()
        assert wav.shape == (2, T * 160)
        ref = si.ola_ref(fr)
        w.check(f"T={T}", wav.double(), ref, torch.full_like(ref, 1e-4))
    w.report()


@pytest.mark.parametrize("out,lds", si.SPEC_OUT)
@pytest.mark.parametrize("ldh", si.SPEC_LDH)
def test_istft_spec(ldh, out, lds):
    """the value check of test_istft (2e-4; one bf16 rounding on top for bf16; split-f16 after un-splitting) at every (ldh,
    format, lds) of the memory-contract test, 3 rows: workgroup boundaries fall inside rows.  The columns beyond 642 are zeros;
    the columns of h beyond 642 hold 1e30 (never read)."""
    ops = _ops()
    h0 = si.spec_input()
    h = torch.full((si.SPEC_ROWS, ldh), 1e30)
    h[:, :642] = h0
    sp = ops.istft_spec(_d(h), ldh, si.SPEC_ROWS, lds, out_dtype=DT[out])
    got = _unsplit(sp, lds) if out == "f16s" else sp.float().cpu().double()
    assert got.shape == (si.SPEC_ROWS, lds)
    re, im, _ = vd.istft_ref(h0)
    ref = torch.cat([re, im], dim=1)
    tol = 2e-4 + BF16_U * (ref.abs() + 2e-4) if out == "bf16" else torch.full_like(ref, 2e-4)
    w = Worst(f"istft_spec ldh={ldh} {out} lds={lds}")
    w.check("re, im", got[:, :642], ref, tol)
    assert bool((got[:, 642:] == 0).all())
    w.report()


# ------------------------------------------------------------------------------------------------------------------ FSQ
@pytest.mark.parametrize("case", si.fsq_encode_cases(), ids=lambda c: f"G{c['G']}-ldz{c['ldz']}-tpad{c['t_pad']}")
def test_fsq_encode(case):
    """codes and zq equal vd.fsq_ref bit for bit (as test_fsq_saturation), rows at and beyond lens[b] and T are zeros; the
    columns of z beyond 4G and its rows beyond lens[b] hold 1e30"""
    ops = _ops()
    G_, ldz, t_pad, T = case["G"], case["ldz"], case["t_pad"], si.FSQ_T
    z, k12, want_zq, want_codes = si.fsq_input(G_)
    zz = torch.full((3, T, ldz), 1e30)
    zz[:, :, :4 * G_] = z.view(3, T, 4 * G_)
    for b, n in enumerate(si.FSQ_LENS):
        zz[b, n:] = 1e30
    lens = _d(torch.tensor(si.FSQ_LENS, dtype=torch.int32))
    zq, codes = ops.fsq_encode(_d(zz), ldz, lens, k12, B=3, T=T, t_pad=t_pad, G=G_, levels=si.FSQ_LEVELS)
    zq, codes = zq.cpu(), codes.cpu()
    assert zq.shape == (3, t_pad, 4 * G_) and codes.shape == (G_, 3, t_pad)
    assert torch.equal(codes[:, :, :T], want_codes)
    assert torch.equal(zq[:, :T].view(torch.int32), want_zq.view(3, T, 4 * G_).view(torch.int32))
    assert bool((codes[:, :, T:] == 0).all()) and bool((zq[:, T:].view(torch.int32) == 0).all())


@pytest.mark.parametrize("case", si.fsq_decode_cases(), ids=lambda c: f"G{c['G']}-ldq{c['ldq']}")
def test_fsq_decode(case):
    """zq of the codes vd.fsq_ref assigns equals its zq bit for bit, except that a level of -0.0 (rintf of a small negative
    number) decodes as +0.0; rows at and beyond lens[b] and the columns from 4G to ldq are zeros.  Codes beyond lens[b] hold
    a valid non-zero code."""
    ops = _ops()
    G_, ldq, T = case["G"], case["ldq"], si.FSQ_T
    _, _, want_zq, want_codes = si.fsq_input(G_)
    codes = want_codes.long()
    for b, n in enumerate(si.FSQ_LENS):
        codes[:, b, n:] = 1234
    lens = _d(torch.tensor(si.FSQ_LENS, dtype=torch.int32))
    zq = ops.fsq_decode(_d(codes), lens, B=3, T=T, G=G_, ldq=ldq, levels=si.FSQ_LEVELS).cpu()
    assert zq.shape == (3, T, ldq)
    want = want_zq.view(3, T, 4 * G_) + 0.0          # -0.0 + 0.0 = +0.0: the decoder computes (n - half) / half from integers
    assert torch.equal(zq[:, :, :4 * G_].view(torch.int32), want.view(torch.int32))
    assert bool((zq[:, :, 4 * G_:].view(torch.int32) == 0).all())
