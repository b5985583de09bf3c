"""The memory contract of every exported kernel (include/swc.h; DESIGN.md "Memory contract"), three checks per entry:
 (a) writes stay inside the declared extent: every output is a poison.guarded window (sentinel bands of 256 rows x ld in
     front and behind, sentinel ld padding) and check() runs after the call;
 (b) what the header says is written is written, and (c) results do not depend on memory the contract calls irrelevant:
     every case runs three times with the previous content of its outputs and all irrelevant input memory (ld padding,
     rows in front of / behind the operand, rows beyond lens) filled with zeros, with NaN and with 6.0e4, and every
     promised output must be BIT-IDENTICAL between the runs (an unwritten element would keep three different fills).
     "Masked but read" memory (attention rows t >= lens[b], ConvNeXt rows beyond t_limit) gets differently seeded finite data
     instead.  The range-guard counters (swc_set_saturation_counter) are installed for every run and must agree as well.
Inputs are checked bit-unchanged after every call.  No tolerances anywhere: the values are tests/test_kernels_gpu.py's job.
Nothing here provokes a fault: all pointers, lengths and starts are valid, poison goes only into memory the test owns.
"""
import ctypes as C
import math

import pytest
import torch

import poison

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILLS = ("zero", "nan", "big")


def covers(*names):
    """names the include/swc.h entry points a test exercises (tests/test_poison_cpu.py greps these against the header)"""
    return lambda fn: fn


def _ops():
    from simwhisper_codec_amd import ops
    return ops


def _lib():
    from simwhisper_codec_amd import _lib
    return _lib.load(), _lib.check


def _fill(t, how):
    if t.numel() == 0:
        return t
    if how == "zero":
        (t.view(torch.uint8) if t.element_size() == 1 else t).zero_()
    else:
        poison.fill_(t, how)
    return t


def _es(dtype):
    return torch.empty(0, dtype=dtype).element_size()


class Arena:
    """the operands of one kernel call under one fill of the irrelevant memory"""

    def __init__(self, fill):
        self.fill, self._inputs, self._checks, self._inouts = fill, [], [], []

    def inp(self, data, ld=None, before=0, after=0, lead=0):
        """read-only operand: data [.., width] as rows of stride ld inside an allocation whose other elements (ld padding,
        `before` / `after` rows, `lead` more elements in front: an unaligned start) carry the fill; must be bit-unchanged
        after the call"""
        view, back = self._embed(data, ld, before, after, lead)
        self._inputs.append((back, back.clone()))
        return view

    def inout(self, data, ld=None, before=0, after=0):
        """in-place operand: as inp(), but only the memory OUTSIDE the window must be unchanged after the call"""
        view, back = self._embed(data, ld, before, after)
        rows, width = data.reshape(-1, data.shape[-1]).shape
        self._inouts.append((back, back.clone(), before, rows, width, ld or width))
        return view

    def _embed(self, data, ld, before, after, lead=0):
        data = data.to(DEV)
        d2 = data.reshape(-1, data.shape[-1])
        rows, width = d2.shape
        ld = width if ld is None else ld
        n = lead + (before + rows + after) * ld
        back = _fill(torch.zeros(n * data.element_size(), dtype=torch.uint8, device=DEV).view(data.dtype), self.fill)
        view = back.as_strided((rows, width), (ld, 1), lead + before * ld)
        (view.view(torch.uint8) if data.element_size() == 1 else view).copy_(d2.view(torch.uint8) if data.element_size() == 1 else d2)
        return view, back

    def out(self, shape, dtype, ld=None, band_rows=256):
        """pure output: a guarded window whose previous content is the fill"""
        view, check = poison.guarded(shape, dtype, ld=ld, band_rows=band_rows, device=DEV)
        _fill(view, self.fill)
        self._checks.append(check)
        return view

    def masked(self, shape, seed, scale=1.0):
        """finite data for memory that is masked but read: another seed per fill, same distribution"""
        g = torch.Generator().manual_seed(seed + 1000 * FILLS.index(self.fill))
        return torch.randn(shape, generator=g) * scale

    def finish(self):
        torch.cuda.synchronize()
        for check in self._checks:
            check()
        for back, snap in self._inputs:
            assert poison.same_bits(back, snap), "a read-only input changed"
        for back, snap, before, rows, width, ld in self._inouts:
            es = back.element_size()
            diff = (back.view(torch.uint8) != snap.view(torch.uint8)).view(-1, ld * es)
            diff[before:before + rows, :width * es] = False
            assert not bool(diff.any()), "an in-place kernel wrote outside its operand"


def same3(case, fills=FILLS):
    """run case(arena) -> {name: promised output} once per fill; all promised outputs and the clip counters bit-identical"""
    ops = _ops()
    res = []
    for f in fills:
        cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
        ops.set_saturation_counter(cnt)
        try:
            ar = Arena(f)
            out = case(ar)
            ar.finish()
        finally:
            ops.set_saturation_counter(None)
        out = {k: v.detach().clone() for k, v in out.items()}
        out["clip counters"] = cnt
        res.append(out)
    for name in res[0]:
        for f, r in zip(fills[1:], res[1:]):
            assert poison.same_bits(res[0][name], r[name]), f"{name}: differs between the zero fill and the {f} fill"
    return res[0]


def _slack(i, es):
    """leading-dimension slack number i in elements: tight, + 16 bytes, + one more odd multiple of 16 bytes (48)"""
    return (0, 16 // es, 48 // es)[i]


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# ------------------------------------------------------------------------------------------------------------ swc_gemm
_EPC = {"f32": 4, "bf16": 8, "f16s": 32, "fp8": 16}     # elements per lda / ldw step (16-byte rows; split-f16: one 32-column block)


def _operand(ops, x, kind, scale):
    """f32 [rows, K] -> (tensor in the operand type, storage columns per logical column)"""
    if kind == "f32":
        return x.to(DEV), 1
    if kind == "bf16":
        return x.to(DEV, torch.bfloat16), 1
    if kind == "f16s":
        return ops.cast_f16s(x.to(DEV), x.shape[-1], scale=scale), 2
    return ops.cast_fp8(x.to(DEV), scale), 1


@covers("swc_gemm", "swc_set_saturation_counter")
@pytest.mark.parametrize("slack", [0, 1, 2])
@pytest.mark.parametrize("M,N,K", [(300, 200, 256), (513, 770, 768), (257, 96, 3072)])
@pytest.mark.parametrize("kind", ["f32", "bf16", "f16s", "fp8"])
def test_gemm_plain(kind, M, N, K, slack):
    ops = _ops()
    sa, sw = {"f16s": (64.0, 2.0 ** 12), "fp8": (16.0, 2.0 ** 10)}.get(kind, (1.0, 1.0))
    A, ca = _operand(ops, _rand((M, K), M + K), kind, sa)
    W, _ = _operand(ops, _rand((N, K), N + K, 0.05), kind, sw)
    bias, gamma, res = _rand((N,), 1).to(DEV), _rand((N,), 2).to(DEV), _rand((M, N), 3)
    pad = _EPC[kind] * (0, 1, 3)[slack]
    out_types = [torch.float32]
    if N % 32 == 0:
        out_types.append({"f32": torch.float16, "bf16": torch.bfloat16, "f16s": torch.float16, "fp8": ops.FP8_T}[kind])
    if kind == "fp8" and N % 32 == 0:
        out_types.append(torch.bfloat16)
    for od in out_types:
        f32_out = od == torch.float32
        cw = 2 if od == torch.float16 else 1
        ldc = N + (32 * (0, 1, 3)[slack] if od == torch.float16 else _slack(slack, _es(od)))

        def case(ar):
            a = ar.inp(A, ld=ca * (K + pad), before=3, after=300)          # rows in front of row 0 and behind row M - 1
            w = ar.inp(W, ld=ca * (K + pad), before=1, after=260)
            r = ar.inp(res, ld=N + _slack(slack, 4), after=300)            # residual rows >= M
            c = ar.out((M, cw * N), od, ld=cw * ldc)                       # previous content of C; rows >= M are the band
            ops.gemm(a, w, M, N, K, out=c, lda=K + pad, ldw=K + pad, ldc=ldc, bias=bias, gamma=gamma if f32_out else None,
                     residual=r, ldr=N + _slack(slack, 4), act=ops.ACT_GELU, alpha=1.0 / (sa * sw),
                     out_scale={torch.float16: 64.0, ops.FP8_T: 16.0}.get(od, 1.0))
            return {"C": c}
        same3(case)


@covers("swc_gemm")
@pytest.mark.parametrize("slack", [0, 1, 2])
@pytest.mark.parametrize("cin,cout,k,stride,dil,pad,T", [(32, 32, 7, 1, 3, 9, 77), (64, 40, 3, 2, 1, 1, 100), (64, 96, 7, 1, 9, 27, 60)])
@pytest.mark.parametrize("kind", ["f32", "bf16", "f16s", "fp8"])
def test_gemm_conv_taps(kind, cin, cout, k, stride, dil, pad, T, slack):
    """taps > 1: the rows in front of utterance 0 and behind utterance B - 1 are outside [0, t_in) of every tap: zero, never read"""
    ops = _ops()
    B = 3
    To = (T + 2 * pad - dil * (k - 1) - 1) // stride + 1
    sa, sw = {"f16s": (64.0, 2.0 ** 10), "fp8": (16.0, 2.0 ** 8)}.get(kind, (1.0, 1.0))
    X, ca = _operand(ops, _rand((B * T, cin), cin + T), kind, sa)
    W, _ = _operand(ops, _rand((cout, k * cin), cout + k, 0.05), kind, sw)
    bias = _rand((cout,), 4).to(DEV)
    lpad = _EPC[kind] * (0, 1, 3)[slack]

    def case(ar):
        x = ar.inp(X, ld=ca * (cin + lpad), before=40, after=300)
        w = ar.inp(W, ld=ca * (k * cin + lpad), after=130)
        c = ar.out((B * To, cout), torch.float32, ld=cout + _slack(slack, 4))
        ops.gemm(x, w, B * To, cout, cin, out=c, lda=cin + lpad, ldw=k * cin + lpad, ldc=cout + _slack(slack, 4), bias=bias, taps=k,
                 dil=dil, stride=stride, pad=pad, t_in=T, t_out=To, alpha=1.0 / (sa * sw))
        return {"C": c}
    same3(case)


# ------------------------------------------------------------------- plan functions (host structs; run here because
# tests/test_poison_cpu.py looks for the @covers of every include/swc.h output entry point in this module; no GPU is used)
@covers("swc_gemm_plan", "swc_dwconv7_ln_plan")
def test_plan_functions_write_their_host_struct_only():
    """the plan functions are host arithmetic: they fill the caller's HOST struct and nothing around it, and follow none of the
    device pointers of the argument block (placeholders here, which a dereference would fault on the host)"""
    from simwhisper_codec_amd import _lib
    lib = _lib.load()
    a = _lib.GemmArgs()
    a.A = a.W = a.C = 0x10000
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc = 70000, 512, 64, 64, 64, 512
    a.taps = a.dil = a.stride = 1
    a.t_in = a.t_out = a.M
    a.a_dtype, a.c_dtype = _lib.BF16, _lib.F32
    for struct, call in ((_lib.GemmPlan, lambda p: lib.swc_gemm_plan(C.byref(a), p)),
                         (_lib.Dwconv7LnPlan, lambda p: lib.swc_dwconv7_ln_plan(3, 2750, 512, _lib.F32, p))):
        n, band = C.sizeof(struct), 64
        raw = (C.c_ubyte * (n + 2 * band))(*([0xA5] * (n + 2 * band)))
        plan = struct.from_buffer(raw, band)
        assert call(C.byref(plan)) == 0 and plan.grid > 0 and plan.slots >= plan.grid
        assert bytes(raw[:band]) == bytes([0xA5] * band) and bytes(raw[band + n:]) == bytes([0xA5] * band)


# ----------------------------------------------------------------------------------------------------------- attention
def _qkv(ar, ops, mode, B, T, H, lens, seed):
    """[B, T, 3 H 64] in the operand type; rows t >= lens[b] are masked but READ (keys are masked by score, rows are computed):
    finite data of another seed per fill"""
    q = _rand((B, T, 3 * H * 64), seed, 0.7)
    other = ar.masked((B, T, 3 * H * 64), seed + 1, 0.7)
    for b, L in enumerate(lens):
        q[b, L:] = other[b, L:]
    if mode == "f32":
        return q
    if mode == "bf16":
        return q.to(torch.bfloat16)
    return ops.cast_f16s(q.view(B * T, -1).to(DEV), 3 * H * 64).view(B, T, -1)


def _valid_rows(out, lens):
    return torch.cat([out[b, :L] for b, L in enumerate(lens)])


@covers("swc_attention", "swc_attention_ex", "swc_attention16")
@pytest.mark.parametrize("T,lens", [(64, [64, 1]), (100, [100, 37, 0]), (130, [65, 130, 64]), (500, [500, 431])])
@pytest.mark.parametrize("mode", ["f32", "f32->f16s", "bf16 legacy", "bf16", "f16s"])
def test_attention_padded(mode, T, lens):
    """promised: rows t < lens[b]; rows t >= lens[b] hold finite don't-care values but stay inside the [B][T] extent"""
    ops = _ops()
    B, H = len(lens), 3
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    in_mode = {"f32->f16s": "f32", "bf16 legacy": "bf16"}.get(mode, mode)
    od = {"f32": torch.float32, "f32->f16s": torch.float16, "bf16 legacy": torch.bfloat16, "bf16": torch.bfloat16,
          "f16s": torch.float16}[mode]
    cw = 2 if od == torch.float16 else 1

    def case(ar):
        qkv = ar.inp(_qkv(ar, ops, in_mode, B, T, H, lens, T), before=2, after=140).view(B, T, -1)
        out = ar.out((B, T, cw * H * 64), od)
        ops.LEGACY_ATTENTION = mode == "bf16 legacy"
        try:
            ops.attention(qkv, ld, B, T, H, out=out, out_dtype=od)
        finally:
            ops.LEGACY_ATTENTION = False
        assert bool(torch.isfinite(out.float()).all())          # "finite don't-care values"
        return {"valid rows of out": _valid_rows(out, lens)}
    same3(case)


@covers("swc_attention16")
@pytest.mark.parametrize("T,lens", [(64, [64, 1]), (100, [100, 37, 0]), (130, [65, 130, 64]), (500, [500, 431]), (129, [129])])
@pytest.mark.parametrize("mode", ["bf16", "f16s"])
def test_attention16_packed(mode, T, lens):
    """valid-token packing: utterance b's lens[b] rows start at row_start[b], nothing follows the last utterance — the rows
    behind it (poison here, qkv and out) are neither read nor written; every packed row of out is promised, and equals
    the padded layout's row bit for bit"""
    ops = _ops()
    B, H = len(lens), 3
    total = sum(lens)
    starts = [sum(lens[:b]) for b in range(B)]
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    rs = torch.tensor(starts, dtype=torch.int32, device=DEV)
    od = torch.bfloat16 if mode == "bf16" else torch.float16
    cw = 2 if mode == "f16s" else 1

    def case(ar):
        q = _qkv(ar, ops, mode, B, T, H, lens, T + 7)
        packed = torch.cat([q[b, :L].to(DEV) for b, L in enumerate(lens)])
        qp = ar.inp(packed, before=2, after=140)
        out = ar.out((total, cw * H * 64), od)
        ops.attention(qp, ld, B, T, H, out=out, row_start=rs, rows=total)
        ref = ar.out((B, T, cw * H * 64), od)
        ops.attention(ar.inp(q, after=140).view(B, T, -1), ld, B, T, H, out=ref)
        assert poison.same_bits(out, _valid_rows(ref, lens)), "packed and padded layouts differ"
        return {"out": out}
    same3(case)


# ------------------------------------------------------------------------------------------- layernorm / pack_rows
_LN_T = {"f32": torch.float32, "bf16": torch.bfloat16, "f16s": torch.float16, "fp8": torch.float8_e4m3fn}


@covers("swc_layernorm")
@pytest.mark.parametrize("layout", ["padded", "padded no lens", "packed"])
@pytest.mark.parametrize("C_", [768, 512, 128])
@pytest.mark.parametrize("y", ["f32", "bf16", "f16s", "fp8"])
def test_layernorm(y, C_, layout):
    """every output row is written: zeros for t >= t_in and for t >= lens[b]; x rows >= lens[b] are never read (NaN there)"""
    ops = _ops()
    B, t_in, t_out = 3, 50, 60
    lens = [50, 20, 0]
    od = _LN_T[y]
    cw = 2 if od == torch.float16 else 1
    w, b = _rand((C_,), 5).to(DEV), _rand((C_,), 6).to(DEV)
    x0 = _rand((B, t_in, C_), C_, 3.0) + 1
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    rs = torch.tensor([0, 50, 70], dtype=torch.int32, device=DEV)

    def case(ar):
        if layout == "packed":
            x = ar.inp(torch.cat([x0[i, :L] for i, L in enumerate(lens)]), before=2, after=300)    # nothing follows the last utterance
        else:
            xx = x0.clone().to(DEV)
            if layout == "padded":
                for i, L in enumerate(lens):
                    _fill(xx[i, L:], ar.fill)
            x = ar.inp(xx, before=2, after=300)
        out = ar.out((B, t_out, cw * C_), od)
        ops.layernorm(x, w, b, 1e-5, B=B, t_in=t_in, t_out=t_out, C_=C_, lens=None if layout == "padded no lens" else ld, out=out,
                      row_start=rs if layout == "packed" else None)
        return {"y": out}
    got = same3(case)["y"]
    z = got.view(torch.uint8) if od == torch.float8_e4m3fn else got
    assert bool((z[:, t_in:] == 0).all())
    if layout != "padded no lens":
        for i, L in enumerate(lens):
            assert bool((z[i, L:] == 0).all())


@covers("swc_pack_rows")
@pytest.mark.parametrize("row_bytes", [16, 3072, 4 * 772])
def test_pack_rows(row_bytes):
    lib, check = _lib()
    ops = _ops()
    B, T, lens = 4, 50, [50, 20, 0, 7]
    total, Cw = sum(lens), row_bytes // 4
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    rs = torch.tensor([0, 50, 70, 70], dtype=torch.int32, device=DEV)
    src0 = _rand((B, T, Cw), row_bytes)

    def case(ar):
        s = src0.clone().to(DEV)
        for i, L in enumerate(lens):
            _fill(s[i, L:], ar.fill)                      # padded rows: never read
        src = ar.inp(s, before=1, after=60)
        dst = ar.out((total, Cw), torch.float32)          # dst beyond `total` is the band
        check(lib.swc_pack_rows(_p(src), _p(dst), _p(rs), _p(ld), B, T, row_bytes, ops._stream()), "swc_pack_rows")
        return {"dst": dst}
    got = same3(case)["dst"]
    assert torch.equal(got.cpu(), torch.cat([src0[i, :L] for i, L in enumerate(lens)]))


# ------------------------------------------------------------------------------- packed operand streams and their kernels
def _pack3(pack, nbytes):
    """(b) + (c) of a pack kernel: every byte of the stream is written whatever it held before (0x00 / 0xA5 / 0xA5 prefill),
    nothing outside it; returns the stream"""
    def case(ar):
        s = ar.out((nbytes,), torch.uint8, band_rows=2)
        pack(s)
        return {"stream": s}
    return same3(case)["stream"]


def _poison_tail(stream):
    """a copy of a packed stream whose prefetch tails are NaN: the stream is four per-wave quarters, each ending in the
    fragments the register ring loads past the last one it consumes — the pack kernels write zeros there (random weights
    leave no other run of zero KiB).  0xFF bytes are NaN as bf16, f16 and e4m3."""
    s = stream.clone()
    q = s.view(4, -1)
    for w in range(4):
        nz = (q[w] != 0).nonzero()
        last = int(nz[-1]) + 1 if nz.numel() else 0
        tail = q.shape[1] - last
        assert tail >= 1024, f"wave {w}: the stream ends in {tail} zero bytes, expected at least one 1 KiB prefetch fragment"
        q[w, q.shape[1] - (tail // 1024) * 1024:] = 0xFF
    return s


def _tail_is_dead(run, stream):
    """prefetched, never consumed: the fused kernel's outputs are bit-identical with a NaN prefetch tail"""
    a, b = run(stream), run(_poison_tail(stream))
    torch.cuda.synchronize()
    for name in a:
        assert poison.same_bits(a[name], b[name]), f"{name} depends on the prefetch tail of the operand stream"


@covers("swc_convnext_pack", "swc_convnext_mlp", "swc_convnext_stream_bytes")
@pytest.mark.parametrize("M,I", [(300, 256), (128, 128), (77, 512)])
def test_convnext_mlp(M, I):
    ops = _ops()
    lib, check = _lib()
    Cc = 512
    w1 = _rand((I, Cc), I, Cc ** -0.5).to(DEV, torch.bfloat16)
    w2 = _rand((Cc, I), I + 1, I ** -0.5).to(DEV, torch.bfloat16)
    b1, b2, gam = _rand((I,), 1, 0.3).to(DEV), _rand((Cc,), 2, 0.3).to(DEV), _rand((Cc,), 3).to(DEV)
    n = lib.swc_convnext_stream_bytes(Cc, I)
    ws = _pack3(lambda s: check(lib.swc_convnext_pack(_p(w1), _p(w2), _p(gam), _p(s), Cc, I, ops._stream()), "swc_convnext_pack"), n)
    assert poison.same_bits(ws, ops.convnext_pack(w1, w2, gam))
    y0, x0 = _rand((M, Cc), M).to(torch.bfloat16), _rand((M, Cc), M + 1)

    def run(stream):
        def case(ar):
            y = ar.inp(y0, before=2, after=200)              # rows >= M
            x = ar.inout(x0, before=256, after=256)          # in place: the rows around x must not change
            ops.convnext_mlp(y, stream, b1, b2, gam, x, M=M, C_=Cc, I=I)
            return {"x": x}
        return same3(case)
    _tail_is_dead(run, ws.clone())


@covers("swc_convnext64_pack", "swc_convnext64_mlp", "swc_convnext64_stream_bytes")
@pytest.mark.parametrize("M,I", [(300, 256), (64, 128)])
def test_convnext64_mlp(M, I):
    ops = _ops()
    lib, check = _lib()
    Cc = 512
    w1 = _rand((I, Cc), I, Cc ** -0.5).to(DEV, torch.bfloat16)
    w2 = _rand((Cc, I), I + 1, I ** -0.5).to(DEV, torch.bfloat16)
    b1, b2, gam = _rand((I,), 1, 0.3).to(DEV), _rand((Cc,), 2, 0.3).to(DEV), _rand((Cc,), 3).to(DEV)
    n = lib.swc_convnext64_stream_bytes(Cc, I)
    ws = _pack3(lambda s: check(lib.swc_convnext64_pack(_p(w1), _p(w2), _p(s), Cc, I, ops._stream()), "swc_convnext64_pack"), n)
    y0, x0 = _rand((M, Cc), M).to(torch.bfloat16), _rand((M, Cc), M + 1)

    def run(stream):
        def case(ar):
            y = ar.inp(y0, before=2, after=200)
            x = ar.inout(x0, before=256, after=256)
            ops.convnext64_mlp(y, stream, b1, b2, gam, x, M=M, C_=Cc, I=I)
            return {"x": x}
        return same3(case)
    _tail_is_dead(run, ws.clone())


@covers("swc_convnext_block", "swc_convnext_pack")
@pytest.mark.parametrize("limits", [None, "t_limit"])
@pytest.mark.parametrize("B,T,I", [(3, 100, 256), (2, 300, 512), (1, 5, 128)])
@pytest.mark.parametrize("operands", [torch.bfloat16, torch.float16])
def test_convnext_block(operands, B, T, I, limits):
    """taps do not cross utterances: the memory in front of utterance 0 and behind utterance B - 1 is never read; x_out's
    previous content is irrelevant.  With t_limit the promised output is the frames below t_limit[b] - 3 (the header's
    receptive-field rule for one block); rows of x at or beyond the limit are masked but may be read (finite other data)."""
    ops = _ops()
    Cc = 512
    w1 = _rand((I, Cc), I, Cc ** -0.5).to(DEV, operands)
    w2 = _rand((Cc, I), I + 1, I ** -0.5).to(DEV, operands)
    b1, b2, gam = _rand((I,), 1, 0.3).to(DEV), _rand((Cc,), 2, 0.3).to(DEV), _rand((Cc,), 3).to(DEV)
    w7, db = _rand((7, Cc), 4, 0.3).to(DEV), _rand((Cc,), 5, 0.1).to(DEV)
    lw, lb = (1 + 0.2 * _rand((Cc,), 6)).to(DEV), (0.1 * _rand((Cc,), 7)).to(DEV)
    ws = ops.convnext_pack(w1, w2, gam)
    lim = [T, max(T // 3, 1), 4][:B] if limits else None
    lim_dev = torch.tensor(lim, dtype=torch.int32, device=DEV) if lim else None
    x0 = _rand((B, T, Cc), B * T)

    def run(stream):
        def case(ar):
            xx = x0.clone()
            if lim:
                other = ar.masked((B, T, Cc), 99)
                for b, L in enumerate(lim):
                    xx[b, L:] = other[b, L:]
            x = ar.inp(xx, before=8, after=200)
            out = ar.out((B, T, Cc), torch.float32)
            ops.convnext_block(x, out, w7, db, lw, lb, 1e-6, stream, b1, b2, gam, B=B, T=T, C_=Cc, I=I, t_limit=lim_dev,
                               operands=operands)
            if lim:
                return {f"x_out[{b}, :t_limit - 3]": out[b, :max(L - 3, 0)] for b, L in enumerate(lim)}
            return {"x_out": out}
        return same3(case)
    _tail_is_dead(run, ws)


def _tail_weights(F_, wdt, seed):
    D = 768
    return (_rand((D, D), seed, D ** -0.5).to(DEV, wdt), _rand((F_, D), seed + 1, D ** -0.5).to(DEV, wdt),
            _rand((D, F_), seed + 2, F_ ** -0.5).to(DEV, wdt))


@covers("swc_mlp_pack", "swc_mlp_block", "swc_mlp_stream_bytes")
@pytest.mark.parametrize("M,F_,with_next", [(64, 256, True), (300, 512, True), (77, 256, False)])
def test_mlp_block(M, F_, with_next):
    ops = _ops()
    lib, check = _lib()
    D = 768
    _, w1, w2 = _tail_weights(F_, torch.bfloat16, F_)
    n = lib.swc_mlp_stream_bytes(D, F_)
    ws = _pack3(lambda s: check(lib.swc_mlp_pack(_p(w1), _p(w2), _p(s), D, F_, ops._stream()), "swc_mlp_pack"), n)
    v = [(_rand((k,), 10 + i, 0.2) + (1 if i in (0, 2) else 0)).to(DEV) for i, k in enumerate((D, D, D, D, F_, D))]
    x0 = _rand((M, D), M, 1.5) + 0.1

    def run(stream):
        def case(ar):
            x = ar.inp(x0, before=2, after=100)                  # rows >= M
            xo = ar.out((M, D), torch.float32)
            yn = ar.out((M, D), torch.bfloat16) if with_next else None
            ops.mlp_block(x, v[0], v[1], 1e-5, stream, v[4], v[5], M=M, D=D, F=F_, x_out=xo,
                          next_ln=(v[2], v[3]) if with_next else None, y_next=yn)
            return {"x_out": xo, **({"y_next": yn} if with_next else {})}
        return same3(case)
    _tail_is_dead(run, ws.clone())


@covers("swc_layer_tail_pack", "swc_layer_tail", "swc_layer_tail_stream_bytes")
@pytest.mark.parametrize("M,F_,with_next", [(64, 256, True), (300, 512, True), (77, 256, False)])
@pytest.mark.parametrize("variant", ["bf16", "f16", "fp8_fc1"])
def test_layer_tail(variant, M, F_, with_next):
    ops = _ops()
    lib, check = _lib()
    D = 768
    wdt = torch.float16 if variant == "f16" else torch.bfloat16
    wo, w1, w2 = _tail_weights(F_, wdt, F_ + 3)
    alpha, f1 = 1.0, ops.BF16
    if variant == "fp8_fc1":
        w1f = _rand((F_, D), F_ + 4, D ** -0.5)
        sw = 2.0 ** math.floor(math.log2(448.0 / float(w1f.abs().max())))
        w1, alpha, f1 = ops.cast_fp8(w1f.to(DEV), sw), 1.0 / (ops.FP8_ACT_SCALE * sw), ops.FP8
    n = lib.swc_layer_tail_stream_bytes(D, F_, f1)
    ws = _pack3(lambda s: check(lib.swc_layer_tail_pack(_p(wo), _p(w1), _p(w2), _p(s), D, F_, f1, ops._stream()),
                                "swc_layer_tail_pack"), n)
    assert poison.same_bits(ws, ops.layer_tail_pack(wo, w1, w2))
    v = [(_rand((k,), 20 + i, 0.2) + (1 if i in (1, 3) else 0)).to(DEV) for i, k in enumerate((D, D, D, D, D, F_, D))]
    x0, att0 = _rand((M, D), M, 1.5) + 0.1, _rand((M, D), M + 1, 0.7).to(torch.bfloat16)

    def run(stream):
        def case(ar):
            att = ar.inp(att0, before=2, after=100)              # rows >= M of attn / x
            x = ar.inp(x0, before=2, after=100)
            xo = ar.out((M, D), torch.float32)
            yn = ar.out((M, D), torch.bfloat16) if with_next else None
            ops.layer_tail(att, x, stream, v[0], v[1], v[2], 1e-5, v[5], v[6], M=M, D=D, F=F_, x_out=xo,
                           next_ln=(v[3], v[4]) if with_next else None, y_next=yn,
                           fc1_dtype=ops.FP8_T if variant == "fp8_fc1" else torch.bfloat16, fc1_alpha=alpha,
                           operands=torch.float16 if variant == "f16" else torch.bfloat16)
            return {"x_out": xo, **({"y_next": yn} if with_next else {})}
        return same3(case)
    _tail_is_dead(run, ws.clone())


@covers("swc_proj_ln_pack", "swc_proj_ln", "swc_proj_ln_stream_bytes")
@pytest.mark.parametrize("slack", [0, 1, 2])
@pytest.mark.parametrize("M,K,with_ln", [(64, 768, True), (300, 3072, True), (77, 768, False), (1000, 256, True)])
def test_proj_ln(M, K, with_ln, slack):
    ops = _ops()
    lib, check = _lib()
    N = 768
    sa, sw = 64.0, 2.0 ** 12
    As = ops.cast_f16s(_rand((M, K), M + K, 0.7).to(DEV), K, scale=sa)
    Ws = ops.cast_f16s(_rand((N, K), K, K ** -0.5).to(DEV), K, scale=sw)
    n = lib.swc_proj_ln_stream_bytes(N, K)
    ws = _pack3(lambda s: check(lib.swc_proj_ln_pack(_p(Ws), _p(s), N, K, ops._stream()), "swc_proj_ln_pack"), n)
    bias, lw, lb = _rand((N,), 1, 0.2).to(DEV), (1 + 0.2 * _rand((N,), 2)).to(DEV), (0.1 * _rand((N,), 3)).to(DEV)
    x0 = _rand((M, N), M, 1.5) + 0.1
    lda = K + 32 * (0, 1, 3)[slack]            # split-f16 rows move in 32-column blocks (128 bytes)

    def run(stream):
        def case(ar):
            a = ar.inp(As, ld=2 * lda, before=2, after=100)
            x = ar.inp(x0, before=2, after=100)
            xo = ar.out((M, N), torch.float32)
            yn = ar.out((M, 2 * N), torch.float16) if with_ln else None
            ops.proj_ln(a, stream, bias, 1.0 / (sa * sw), x, M=M, N=N, K=K, lda=lda, x_out=xo, ln=(lw, lb) if with_ln else None,
                        y_next=yn)
            return {"x_out": xo, **({"y_next": yn} if with_ln else {})}
        return same3(case)
    _tail_is_dead(run, ws.clone())


# ------------------------------------------------------------------------------------------------- Vocos pointwise kernels
@covers("swc_dwconv7_ln")
@pytest.mark.parametrize("C_,T", [(512, 100), (64, 9), (512, 1), (260, 33), (1024, 37)])
@pytest.mark.parametrize("y", [torch.float32, torch.bfloat16])
def test_dwconv7_ln(y, C_, T):
    ops = _ops()
    B = 2
    w7, db, lw, lb = _rand((7, C_), 1, 0.3).to(DEV), _rand((C_,), 2).to(DEV), _rand((C_,), 3).to(DEV), _rand((C_,), 4).to(DEV)
    x0 = _rand((B, T, C_), C_ + T)

    def case(ar):
        x = ar.inp(x0, before=8, after=40)
        out = ar.out((B, T, C_), y)
        ops.dwconv7_ln(x, w7, db, lw, lb, 1e-6, B=B, T=T, C_=C_, out=out)
        return {"y": out}
    same3(case)


@covers("swc_snake_aa")
@pytest.mark.parametrize("C_,T", [(512, 125), (64, 1), (64, 3), (32, 40)])
@pytest.mark.parametrize("y", [torch.float32, torch.bfloat16, torch.float16])
def test_snake_aa(y, C_, T):
    ops = _ops()
    B = 2
    al, be = _rand((C_,), 1, 0.3).exp().to(DEV), _rand((C_,), 2, 0.3).exp().to(DEV)
    filt = [0.002, -0.01, 0.03, -0.08, 0.2, 0.358, 0.358, 0.2, -0.08, 0.03, -0.01, 0.002]
    x0 = _rand((B, T, C_), C_ * T, 2.0)
    cw = 2 if y == torch.float16 else 1

    def case(ar):
        x = ar.inp(x0, before=16, after=40)                 # replicate padding: nothing in front of / behind an utterance is read
        out = ar.out((B, T, cw * C_), y)
        ops.snake_aa(x, al, be, filt, B=B, T=T, C_=C_, out=out)
        return {"y": out}
    same3(case)


# ----------------------------------------------------------------------------------------------------------------- FSQ
def _fsq_consts(levels):
    from simwhisper_codec_amd import spec
    return spec.fsq_constants(list(levels), 1e-3)


@covers("swc_fsq_encode", "swc_fsq_encode_levels")
@pytest.mark.parametrize("slack", [0, 1, 2])
@pytest.mark.parametrize("levels", [None, (8, 7, 6, 6), (16, 3, 2, 9)])
def test_fsq_encode(levels, slack):
    """zq and codes are written up to t_pad: zeros for t >= lens[b] and t >= T; z rows >= lens[b] and the ldz padding are never read"""
    lib, check = _lib()
    ops = _ops()
    B, T, G, t_pad = 3, 50, 8, 64
    lens = [50, 13, 0]
    ldz = 4 * G + _slack(slack, 4)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    k12 = (C.c_float * 12)(*_fsq_consts(levels or (8, 7, 6, 6)))
    lv = (C.c_int32 * 4)(*(levels or (8, 7, 6, 6)))
    z0 = _rand((B, T, 4 * G), 3, 1.5)

    def case(ar):
        zz = z0.clone().to(DEV)
        for i, L in enumerate(lens):
            _fill(zz[i, L:], ar.fill)
        z = ar.inp(zz, ld=ldz, before=1, after=40)
        zq = ar.out((B, t_pad, 4 * G), torch.float32)
        codes = ar.out((G, B, t_pad), torch.int32)
        if levels is None:
            check(lib.swc_fsq_encode(_p(z), ldz, _p(zq), _p(codes), _p(ld), k12, B, T, t_pad, G, ops._stream()), "swc_fsq_encode")
        else:
            check(lib.swc_fsq_encode_levels(_p(z), ldz, _p(zq), _p(codes), _p(ld), k12, lv, B, T, t_pad, G, ops._stream()),
                  "swc_fsq_encode_levels")
        return {"zq": zq, "codes": codes}
    got = same3(case)
    for i, L in enumerate(lens):
        assert bool((got["zq"][i, L:] == 0).all()) and bool((got["codes"][:, i, L:] == 0).all())
    assert bool(got["codes"][:, 0, :50].any())


@covers("swc_fsq_decode", "swc_fsq_decode_levels")
@pytest.mark.parametrize("slack", [0, 1, 2])
@pytest.mark.parametrize("levels", [None, (8, 7, 6, 6), (16, 3, 2, 9)])
def test_fsq_decode(levels, slack):
    """zq rows are written whole (ldq columns: cols >= 4G zero) and masked by lens; codes at t >= lens[b] are irrelevant"""
    lib, check = _lib()
    ops = _ops()
    B, T, G = 3, 50, 8
    lens = [50, 13, 0]
    ldq = 4 * G + _slack(slack, 4)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    lv = (C.c_int32 * 4)(*(levels or (8, 7, 6, 6)))
    n_codes = math.prod(levels or (8, 7, 6, 6))
    c0 = torch.randint(0, n_codes, (G, B, T), generator=torch.Generator().manual_seed(9), dtype=torch.int64)

    def case(ar):
        cc = c0.clone().to(DEV)
        for i, L in enumerate(lens):
            _fill(cc[:, i, L:], ar.fill)                 # integer poison: the small wrong value 1, a valid code
        codes = ar.inp(cc, before=1, after=4)
        zq = ar.out((B, T, ldq), torch.float32)
        if levels is None:
            check(lib.swc_fsq_decode(_p(codes), _p(zq), ldq, _p(ld), B, T, G, ops._stream()), "swc_fsq_decode")
        else:
            check(lib.swc_fsq_decode_levels(_p(codes), _p(zq), ldq, _p(ld), lv, B, T, G, ops._stream()), "swc_fsq_decode_levels")
        return {"zq": zq}
    got = same3(case)["zq"]
    assert bool((got[:, :, 4 * G:] == 0).all()) and bool(got[0].any())
    for i, L in enumerate(lens):
        assert bool((got[i, L:] == 0).all())


# ------------------------------------------------------------------------------------------------------- log-mel front end
@covers("swc_mel_frames")
@pytest.mark.parametrize("slack", [0, 1, 2])
def test_mel_frames(slack):
    """wav samples >= n[b] are virtually zero: never read; the ld_wav padding neither"""
    lib, check = _lib()
    ops = _ops()
    B, n_pad = 3, 2000
    n = [2000, 1234, 0]
    T = n_pad // 160
    ldw = n_pad + _slack(slack, 4)
    nd = torch.tensor(n, dtype=torch.int32, device=DEV)
    w0 = _rand((B, n_pad), 0)

    def case(ar):
        ww = w0.clone().to(DEV)
        for i, L in enumerate(n):
            _fill(ww[i, L:], ar.fill)
        wav = ar.inp(ww, ld=ldw, before=1, after=2)
        fr = ar.out((B, T, 400), torch.float32)
        check(lib.swc_mel_frames(_p(wav), ldw, _p(nd), n_pad, _p(fr), B, T, ops._stream()), "swc_mel_frames")
        return {"frames": fr}
    got = same3(case)["frames"]
    assert bool((got[2] == 0).all()) and bool(got[0].any())


@covers("swc_mel_power", "swc_mel_logmax", "swc_mel_final")
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("slack", [0, 1, 2])
def test_mel_power_logmax_final(slack, out_dtype):
    """power: dft columns >= 402 never read, pw rows written whole (cols >= 201 zero).  logmax: in place on the first n_mel
    columns, the mel padding columns (80 -> 96) neither read (the max / abs reduction must not see them) nor written.
    final: out rows written whole (cols n_mel .. ldo zero)."""
    lib, check = _lib()
    ops = _ops()
    B, T, n_mel = 3, 12, 80
    rows = B * T
    ld, ldp = 402 + 2 + _slack(slack, 4), 201 + 3 + _slack(slack, 4)
    dft0 = _rand((rows, 402), 1)
    mel0 = torch.rand((B, T, n_mel), generator=torch.Generator().manual_seed(2)) * 5
    mel0[2] = 0.0
    ldm = 96 + _slack(slack, 4)
    od = out_dtype
    ldo = 96 + _slack(slack, _es(od))

    def case(ar):
        dft = ar.inp(dft0, ld=ld, before=1, after=8)
        pw = ar.out((rows, ldp), torch.float32)
        check(lib.swc_mel_power(_p(dft), ld, _p(pw), ldp, rows, ops._stream()), "swc_mel_power")
        mel = ar.inout(mel0, ld=ldm, before=4, after=4)
        umax = ar.inout(torch.tensor([[-10.0, float("-inf"), -10.0]]), before=1, after=1)
        check(lib.swc_mel_logmax(_p(mel), ldm, _p(umax), B, T, n_mel, ops._stream()), "swc_mel_logmax")
        out = ar.out((B, T, ldo), od)
        check(lib.swc_mel_final(_p(mel), ldm, _p(umax), _p(out), ldo, B, T, n_mel, ops._DT[od], ops._stream()), "swc_mel_final")
        return {"pw": pw, "log mel": mel, "umax": umax, "out": out}
    got = same3(case)
    assert bool((got["pw"][:, 201:] == 0).all()) and bool(got["pw"][:, :201].any())
    assert bool((got["out"][:, :, n_mel:] == 0).all()) and bool(got["out"][:, :, :n_mel].float().any())


# ------------------------------------------------------------------------------------------- up-sampler tail, ISTFT head
@covers("swc_deconv_col2im")
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("slack", [0, 1, 2])
@pytest.mark.parametrize("s", [2, 1])
def test_deconv_col2im(s, slack, out_dtype):
    lib, check = _lib()
    ops = _ops()
    B, T, Co = 2, 17, 24
    t_out = (T - 1) * s + 3 - (1 if s == 2 else 3)
    ldo = 32 + _slack(slack, _es(out_dtype))
    y0, bias = _rand((B * T, 3 * Co), 9), _rand((Co,), 1).to(DEV)

    def case(ar):
        y3 = ar.inp(y0, before=2, after=20)
        out = ar.out((B, t_out, ldo), out_dtype)
        check(lib.swc_deconv_col2im(_p(y3), _p(bias), _p(out), ldo, B, T, Co, s, t_out, ops._DT[out_dtype], ops._stream()),
              "swc_deconv_col2im")
        return {"out": out}
    got = same3(case)["out"]
    assert bool((got[:, :, Co:] == 0).all()) and bool(got[:, :, :Co].any())


@covers("swc_istft_spec")
@pytest.mark.parametrize("s_dtype,lds", [(torch.float32, 642), (torch.float32, 648), (torch.float32, 672), (torch.bfloat16, 648),
                                         (torch.bfloat16, 672), (torch.float16, 672), (torch.float16, 704)])
@pytest.mark.parametrize("ldh", [642, 648, 656, 668])
def test_istft_spec(ldh, s_dtype, lds):
    """the head GEMM writes 642 columns into rows of 648: columns 642 .. ldh are never read; s rows are written whole (pad zero)"""
    lib, check = _lib()
    ops = _ops()
    rows = 46
    h0 = _rand((rows, 642), 11)
    h0[0, 3] = 9.0
    cw = 2 if s_dtype == torch.float16 else 1

    def case(ar):
        h = ar.inp(h0, ld=ldh, before=1, after=8)
        s = ar.out((rows, cw * lds), s_dtype)
        check(lib.swc_istft_spec(_p(h), ldh, _p(s), lds, rows, ops._DT[s_dtype], ops._stream()), "swc_istft_spec")
        return {"s": s}
    got = same3(case)["s"]
    if s_dtype != torch.float16:
        assert bool((got[:, 642:] == 0).all()) and bool(got[:, :642].any())


@covers("swc_istft_ola")
@pytest.mark.parametrize("B,T", [(2, 23), (1, 1), (3, 5)])
def test_istft_ola(B, T):
    lib, check = _lib()
    ops = _ops()
    wsq = (torch.hann_window(640) ** 2).to(DEV)
    f0 = _rand((B * T, 640), T)

    def case(ar):
        fr = ar.inp(f0, before=4, after=8)                       # frames in front of utterance 0 / behind utterance B - 1
        wav = ar.out((B, T * 160), torch.float32)
        check(lib.swc_istft_ola(_p(fr), _p(wsq), _p(wav), B, T, ops._stream()), "swc_istft_ola")
        return {"wav": wav}
    same3(case)


# ------------------------------------------------------------------------------------------ bitstream, casts, batch assembly
@covers("swc_codes_pack", "swc_codes_unpack")
@pytest.mark.parametrize("slack", [0, 1, 2])
@pytest.mark.parametrize("T", [1, 7, 1000])
def test_codes_pack_unpack(T, slack):
    lib, check = _lib()
    ops = _ops()
    ldg = T + _slack(slack, 4)
    c0 = torch.randint(0, 2016, (8, T), generator=torch.Generator().manual_seed(T), dtype=torch.int32)

    def case(ar):
        codes = ar.inp(c0, ld=ldg, before=1, after=1)
        by = ar.out((11 * T,), torch.uint8, band_rows=2)
        check(lib.swc_codes_pack(_p(codes), ldg, _p(by), T, ops._stream()), "swc_codes_pack")
        back = ar.out((8, T), torch.int32, ld=ldg)
        check(lib.swc_codes_unpack(_p(ar.inp(by.clone().view(1, -1), before=1, after=1)), _p(back), ldg, T, ops._stream()),
              "swc_codes_unpack")
        return {"bytes": by, "codes": back}
    got = same3(case)
    assert torch.equal(got["codes"].cpu(), c0)


@covers("swc_cast_f32_bf16", "swc_cast_f32_f16s", "swc_cast_fp8")
@pytest.mark.parametrize("slack", [0, 1, 2])
@pytest.mark.parametrize("rows,K", [(37, 96), (1, 32), (300, 768)])
def test_casts(rows, K, slack):
    lib, check = _lib()
    ops = _ops()
    x0 = _rand((rows, K), rows + K) * torch.logspace(-3, 1.5, K)[None, :]
    ldx = K + _slack(slack, 4)
    n = rows * K

    def case(ar):
        xs = ar.inp(x0, ld=ldx, before=1, after=3)               # f16s: f32 [rows][ldx], first K columns
        y16 = ar.out((rows, 2 * K), torch.float16)
        check(lib.swc_cast_f32_f16s(_p(xs), ldx, _p(y16), rows, K, 64.0, ops._stream()), "swc_cast_f32_f16s")
        xc = ar.inp(x0.view(1, -1), before=1, after=1)
        yb = ar.out((n,), torch.bfloat16, band_rows=2)
        check(lib.swc_cast_f32_bf16(_p(xc), _p(yb), n, ops._stream()), "swc_cast_f32_bf16")
        y8 = ar.out((n,), torch.float8_e4m3fn, band_rows=2)
        check(lib.swc_cast_fp8(_p(xc), ops.F32, _p(y8), n, 16.0, ops._stream()), "swc_cast_fp8")
        xb = ar.inp(x0.to(torch.bfloat16).view(1, -1), before=1, after=1)
        y8b = ar.out((n,), torch.float8_e4m3fn, band_rows=2)
        check(lib.swc_cast_fp8(_p(xb), ops.BF16, _p(y8b), n, 16.0, ops._stream()), "swc_cast_fp8")
        return {"f16s": y16, "bf16": yb, "fp8": y8, "fp8 from bf16": y8b}
    got = same3(case)
    assert int(got["clip counters"][1]) > 0          # the logspace tail exceeds 28: the counter comparison is not vacuous


@covers("swc_gather_rows")
@pytest.mark.parametrize("slack", [0, 1, 2])
def test_gather_rows(slack):
    """out rows are written whole: zero-filled beyond each row's length up to ld_bytes"""
    lib, check = _lib()
    ops = _ops()
    lens = [0, 1, 5, 1000, 777, 4096, 3]
    L = max(lens) + 5 + _slack(slack, 4)
    rows0 = [_rand((1, max(n, 1)), n, 100.0) for n in lens]

    def case(ar):
        srcs = [ar.inp(r, before=1, after=1) for r in rows0]
        ptrs = torch.tensor([s.data_ptr() for s in srcs], dtype=torch.int64, device=DEV)
        nb = torch.tensor([4 * n for n in lens], dtype=torch.int64, device=DEV)
        out = ar.out((len(lens), L), torch.float32)
        check(lib.swc_gather_rows(_p(ptrs), _p(nb), _p(out), 4 * L, len(lens), ops._stream()), "swc_gather_rows")
        return {"out": out}
    got = same3(case)["out"].cpu()
    for i, n in enumerate(lens):
        assert torch.equal(got[i, :n], rows0[i][0, :n]) and bool((got[i, n:] == 0).all())


@covers("swc_pcm16_to_f32", "swc_f32_to_pcm16")
@pytest.mark.parametrize("n,off", [(1, 0), (7, 0), (8, 0), (4099, 3), (65536, 5), (160003, 0)])
def test_pcm16(n, off):
    """unaligned starts take the scalar head / tail: nothing in front of or behind the n samples is read or written"""
    lib, check = _lib()
    ops = _ops()
    g = torch.Generator().manual_seed(n)
    pcm0 = torch.randint(-32768, 32768, (1, n), generator=g, dtype=torch.int32).to(torch.int16)
    x0 = torch.rand((1, n), generator=g) * 2.6 - 1.3

    def case(ar):
        # `off` elements of fill in front of the data: an unaligned start that is still the test's memory
        pcm = ar.inp(pcm0, after=1, lead=off)
        f = ar.out((n,), torch.float32, band_rows=1 if off else 2)
        check(lib.swc_pcm16_to_f32(_p(pcm), _p(f), n, ops._stream()), "swc_pcm16_to_f32")
        x = ar.inp(x0, after=1, lead=off)
        p = ar.out((n,), torch.int16, band_rows=1 if off else 2)
        check(lib.swc_f32_to_pcm16(_p(x), _p(p), n, ops._stream()), "swc_f32_to_pcm16")
        return {"f32": f, "pcm": p}
    got = same3(case)
    assert torch.equal(got["f32"].cpu(), pcm0[0].float() / 32768.0)
