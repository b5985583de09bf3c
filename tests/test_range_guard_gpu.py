"""The range guard at kernel level: every producer of a split-f16 / fp8 activation counts its clips, and only those.

One test per counted site of tests/sat_sites.py (tests/test_sat_sites_cpu.py pins that table to the kernel sources), through
`ops`, at the smallest shape that reaches the code path; GEMM cases assert the path with ops.gemm_call_plan.  Every assertion is
an integer count or a bit pattern:

  threshold   the largest representable magnitude (+-1023.5 at scale 64, +-28 at scale 16) is stored exactly and leaves the
              counters at 0; the next float32 beyond it, and +-Inf, are stored as the finite limit and count; the other slot of
              the pair never moves.  The value reaches the conversion exactly (a residual / bias added to an exact zero).
              swc_layer_tail keeps its e4m3 operand in LDS: there the counts alone are asserted.  The snake has no exact
              threshold (every output is a filtered sum: test_snake_exits says why); its counts are bounded by the reference.
  position    one output beyond the range counts exactly 1 wherever it sits (a thread commits once), k outputs in k different
              tiles / rows count k.  The float64 restatement of the kernel decides which outputs lie beyond the range; the
              inputs keep every reference output a relative 1e-3 away from the limit (asserted), so no count is ambiguous.
  silence     out-of-range, finite data wherever the kernel must not convert: rows >= M, rows >= lens[b], the rows before and
              behind the operands, leading-dimension padding.  A false positive costs a permanent fall-back to exact f32.
  accounting  a NULL pointer changes nothing, counts add up across launches, one call counts what the same rows count as
              separate launches.
"""
import contextlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import poison
import stage_index as si
import value_domain as vd

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE = {"f16s": 64.0, "fp8": 16.0}
LIM = {"f16s": 65504.0 / 64.0, "fp8": 448.0 / 16.0}       # 1023.5, 28
SLOT = {"f16s": 0, "fp8": 1}
OUTLIER = {"f16s": 4096.0, "fp8": 112.0}                   # 4 x the limit: far from it whatever in-range value it is added to
MARGIN = 1e-3


def _ops():
    from simwhisper_codec_amd import ops
    return ops


def _dt(kind):
    return torch.float16 if kind == "f16s" else _ops().FP8_T


def _next(v):
    """the float32 next to v, away from zero"""
    return float(np.nextafter(np.float32(v), np.float32(math.copysign(math.inf, v))))


@contextlib.contextmanager
def counting():
    """a zeroed counter pair installed for the calling thread; uninstalled afterwards"""
    ops = _ops()
    cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
    ops.set_saturation_counter(cnt)
    try:
        yield cnt
    finally:
        ops.set_saturation_counter(None)


def _count(cnt, kind, reset=True):
    """this kind's count since the last reset; the other slot must not have moved"""
    v = cnt.tolist()
    assert v[1 - SLOT[kind]] == 0, v
    if reset:
        cnt.zero_()
    return v[SLOT[kind]]


def _at(y, kind, r, c):
    """the value stored at logical (row, column) of a [rows, storage columns] output, as a Python float (exact)"""
    if kind == "f16s":
        h = (c // 32) * 64 + c % 32
        return (float(y[r, h]) + float(y[r, h + 32])) / 64.0
    return float(y[r, c].float()) / 16.0


def _finite(y):
    return bool(torch.isfinite(y.float()).all())


def _clear_of_the_limit(ref, kind):
    """the issue's margin: no reference output within a relative 1e-3 of the limit -> the mask of outputs beyond the range"""
    a = ref.abs()
    near = (a > LIM[kind] * (1 - MARGIN)) & (a < LIM[kind] * (1 + MARGIN))
    assert not bool(near.any()), a[near]
    return a > LIM[kind]


def _embed(data, ld, before, after):
    """data [rows, width] inside (before + rows + after) rows of ld elements; everything else holds the `big` poison
    (6e4 in f32 / f16 halves, 448 in e4m3): finite, and out of range wherever it would be converted"""
    rows, width = data.shape
    back = poison.fill_(torch.empty((before + rows + after) * ld, dtype=data.dtype, device=DEV), "big")
    view = back.as_strided((rows, width), (ld, 1), before * ld)
    if data.dtype == _ops().FP8_T:
        view.view(torch.uint8).copy_(data.view(torch.uint8))
    else:
        view.copy_(data)
    return view


def _threshold_series(kind, bf16_input=False):
    """(value, counted, stored): +-limit exact and silent; the next number beyond it and +-Inf stored as the finite limit"""
    lim = LIM[kind]
    nxt = 28.125 if bf16_input else _next(lim)             # bf16 has 8 significand bits: 28 + 2^-3
    out = []
    for s in (1.0, -1.0):
        out += [(s * lim, 0, s * lim), (s * nxt, 1, s * lim), (s * math.inf, 1, s * lim)]
    return out


# ------------------------------------------------------------------------------------------------------------- casts
def _cast(kind, x, K=None, ldx=None):
    ops = _ops()
    if kind == "f16s":
        return ops.cast_f16s(x, K, ldx=ldx)
    return ops.cast_fp8(x)


@pytest.mark.parametrize("kind,src", [("f16s", torch.float32), ("fp8", torch.float32), ("fp8", torch.bfloat16)],
                         ids=["f16s", "fp8-from-f32", "fp8-from-bf16"])
def test_cast_sites(kind, src):
    """swc_cast_f32_f16s (rows of a wider matrix: ldx > K, big values in the padding and around the matrix) and swc_cast_fp8
    from f32 and from bf16 (a contiguous run inside a larger buffer of big values).  One thread converts 4 elements."""
    rows, K = 5, 96
    g = torch.Generator().manual_seed(11)
    base = (torch.randn(rows, K, generator=g) * 0.5).to(src)
    if kind == "f16s":
        def run(x):
            return _cast(kind, _embed(x.to(DEV), K + 4, 2, 3), K, K + 4)
    else:
        def run(x):
            back = poison.fill_(torch.empty(rows * K + 64, dtype=src, device=DEV), "big")
            inner = back[32:32 + rows * K]
            inner.copy_(x.reshape(-1))
            return _cast(kind, inner.view(rows, K)).view(rows, K)
    _clear_of_the_limit(base.double(), kind)
    with counting() as cnt:
        y = run(base)
        assert _count(cnt, kind) == 0 and _finite(y)
        # threshold, both signs
        for v, counted, stored in _threshold_series(kind, src == torch.bfloat16):
            x = base.clone()
            x[2, 41] = v
            y = run(x)
            assert _count(cnt, kind) == counted, v
            assert _at(y, kind, 2, 41) == stored and _finite(y), (v, _at(y, kind, 2, 41))
        # position: exactly 1 wherever the element sits; k elements in k threads count k, two in one thread count 1
        spots = [(0, 0), (0, 3), (0, 4), (0, 31), (0, 32), (2, 63), (2, 64), (rows - 1, K - 1), (rows - 1, K - 4), (3, 95), (4, 0)]
        for i, (r, c) in enumerate(spots):
            x = base.clone()
            x[r, c] = OUTLIER[kind] * (-1) ** i
            y = run(x)
            assert _count(cnt, kind) == 1, (r, c)
            assert _at(y, kind, r, c) == LIM[kind] * (-1) ** i and _finite(y)
        x = base.clone()
        for r, c in spots[::2]:                            # (0,0) (0,4) (0,32) (2,64) (4,92) (4,0): six different 4-groups
            x[r, c] = OUTLIER[kind]
        many = run(x)
        assert _count(cnt, kind) == len(spots[::2]) and _finite(many)
        x = base.clone()
        x[1, 8:12] = -OUTLIER[kind]
        run(x)
        assert _count(cnt, kind) == 1
        # accounting: counts add up; the rows as separate launches count the same
        x = base.clone()
        x[0, 5], x[3, 7], x[4, 90] = OUTLIER[kind], -OUTLIER[kind], math.inf
        run(x)
        run(x)
        assert _count(cnt, kind) == 6
        for r in range(rows):
            if kind == "f16s":
                _cast(kind, _embed(x[r:r + 1].to(DEV), K + 4, 1, 1), K, K + 4)
            else:
                _cast(kind, x[r:r + 1].to(DEV))
        assert _count(cnt, kind) == 3
        keep = cnt.clone()
    run(x)                                                 # the pointer is NULL again: nothing changes
    torch.cuda.synchronize()
    assert torch.equal(cnt, keep)


# --------------------------------------------------------------------------------------------------------- LayerNorm
LN_CASES = [("f16s", 128), ("fp8", 128), ("fp8", 512), ("f16s", 512), ("f16s", 768)]
LN_IDS = ["generic-f16s-128", "generic-fp8-128", "generic-fp8-512", "two-rows-f16s-512", "two-rows-f16s-768"]


def _ln(x, w, b, kind, **kw):
    C = x.shape[-1]
    return _ops().layernorm(x, w, b, 1e-5, C_=C, out_dtype=_dt(kind), **kw)


@pytest.mark.parametrize("kind,C", LN_CASES, ids=LN_IDS)
def test_layernorm_threshold(kind, C):
    """weight 0 and bias v on one channel: the output there is 0 * xhat + v = v exactly.  One live row = one thread converts it
    (layernorm2_kernel: the wave's second row lies beyond `rows`)."""
    g = torch.Generator().manual_seed(C)
    x = torch.randn(1, 1, C, generator=g).to(DEV)
    w = torch.zeros(C, device=DEV)
    with counting() as cnt:
        for col in (0, 3, 255 % C, C // 2, C - 1):
            for v, counted, stored in _threshold_series(kind):
                b = torch.zeros(C, device=DEV)
                b[col] = v
                y = _ln(x, w, b, kind, B=1, t_in=1).view(1, -1)
                assert _count(cnt, kind) == counted, (col, v)
                assert _at(y, kind, 0, col) == stored and _finite(y), (col, v, _at(y, kind, 0, col))


def _ln_inputs(kind, C, rows, spikes, seed):
    """rows of N(0, 1) noise; a spike of 1e4 at (row, col) makes xhat there sqrt(C - 1) (11 ... 28) and ~0 elsewhere in that row,
    and the gain on a spiked column is large enough that spike x gain leaves the range while noise x gain (|xhat| < 5) stays inside"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g)
    gain = {"f16s": 150.0, "fp8": 4.0}[kind]
    w, b = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    for i, (r, c) in enumerate(spikes):
        x[r, c] = 1e4 * (-1) ** i
        w[c] = gain
    return x, w, b


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("kind,C", LN_CASES, ids=LN_IDS)
def test_layernorm_position_masks_accounting(kind, C, packed):
    """B = 3 utterances of t_in = 5 input rows, lens = (5, 3, 0), t_out = 7 output rows each (21 output rows: three blocks of the
    generic kernel, two and a half of layernorm2_kernel, whose waves take the output rows pairwise).  Packed: the input holds
    the valid rows only, at row_start, with a gap row between the utterances.  Every input row that is NOT converted (rows >=
    lens[b], the gap, the rows before and behind the input) carries the same spike that counts in a live row."""
    ops = _ops()
    B, t_in, t_out, lens = 3, 5, 7, [5, 3, 0]
    cols = [0, 3, 255 % C, 256 % C, C - 4, C - 1]
    live = [(b, t) for b in range(B) for t in range(lens[b])]                   # (utterance, frame) that are converted
    swept = [(0, 0), (0, 1), (0, 4), (1, 0), (1, 1), (1, 2)]
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    start = [0, 6, 10]                                                           # packed: a gap row behind utterance 0
    rs = torch.tensor(start, dtype=torch.int32, device=DEV) if packed else None
    n_in = 10 if packed else B * t_in

    def in_row(b, t):
        return start[b] + t if packed else b * t_in + t

    dead = [r for r in range(n_in) if r not in {in_row(b, t) for b, t in live}]

    def run(spikes, seed=0, utterances=None):
        """spikes: [(utterance, frame, col)] in live rows -> (output [B * t_out, storage columns], float64 reference, beyond)"""
        sp = [(in_row(b, t), c) for b, t, c in spikes] + [(r, cols[i % len(cols)]) for i, r in enumerate(dead)]
        x, w, bb = _ln_inputs(kind, C, n_in, sp, seed)
        ref = torch.zeros(B, t_out, C, dtype=torch.float64)
        full = vd.ln_ref(x, w, bb, 1e-5)
        for b, t in live:
            ref[b, t] = full[in_row(b, t)]
        beyond = _clear_of_the_limit(ref, kind)
        xd = _embed(x.to(DEV), C, 2, 2)
        sel = range(B) if utterances is None else utterances
        outs = []
        for b in sel if utterances is not None else [None]:
            if b is None:
                y = _ln(xd, w.to(DEV), bb.to(DEV), kind, B=B, t_in=t_in, t_out=t_out, lens=ld, row_start=rs)
            elif packed:
                y = _ln(xd, w.to(DEV), bb.to(DEV), kind, B=1, t_in=t_in, t_out=t_out, lens=ld[b:b + 1], row_start=rs[b:b + 1])
            else:
                y = _ln(xd[b * t_in:(b + 1) * t_in], w.to(DEV), bb.to(DEV), kind, B=1, t_in=t_in, t_out=t_out, lens=ld[b:b + 1])
            outs.append(y.view(-1, y.shape[-1]))
        return torch.cat(outs), ref.view(B * t_out, C), beyond.view(B * t_out, C)

    with counting() as cnt:
        # silence: spikes in every dead row only
        y, ref, beyond = run([])
        assert not bool(beyond.any()) and _count(cnt, kind) == 0 and _finite(y)
        # masked rows and the rows in [t_in, t_out) are zeros, bit for bit
        zero_rows = [b * t_out + t for b in range(B) for t in range(t_out) if (b, t) not in live]
        assert not bool(y[zero_rows].view(torch.uint8 if kind == "fp8" else torch.int16).any())
        # position: first / last live row of an utterance, the first row of utterance 1 (packed: behind the gap), both rows
        # of a wave's pair (output rows 0|1, 4, 7|8|9), every lane end and both sides of the 256-column step
        for i, (b, t) in enumerate(swept):
            for c in (cols[i % len(cols)], cols[(i + 3) % len(cols)]):
                y, ref, beyond = run([(b, t, c)], seed=i)
                assert int(beyond.sum()) == 1 and bool(beyond[b * t_out + t, c])
                assert _count(cnt, kind) == 1, (b, t, c)
                assert abs(_at(y, kind, b * t_out + t, c)) == LIM[kind] and _finite(y)
        # k outliers in k different rows of different waves / blocks
        many = [(0, 0, cols[0]), (0, 4, cols[1]), (1, 0, cols[2]), (1, 2, cols[3])]      # output rows 0, 4, 7, 9
        y, ref, beyond = run(many)
        assert int(beyond.sum()) == 4 and _count(cnt, kind) == 4 and _finite(y)
        # accounting: twice the launch, twice the count; utterance by utterance, the same count
        run(many)
        run(many)
        assert _count(cnt, kind) == 8
        y2, _, _ = run(many, utterances=[0, 1, 2])
        assert _count(cnt, kind) == 4 and torch.equal(y2.view(torch.uint8), y.view(torch.uint8))
        keep = cnt.clone()
    run(many)
    torch.cuda.synchronize()
    assert torch.equal(cnt, keep)


# ------------------------------------------------------------------------------------------------------------- snake
@pytest.mark.parametrize("T,t_spike,path,amp", [(24, 11, "fast", 2500.0), (24, 12, "fast", 12000.0), (3, 1, "generic", 2500.0),
                                                 (3, 1, "generic", 12000.0), (24, 1, "generic", 2500.0), (24, 22, "generic", 12000.0)],
                         ids=["interior-t11", "interior-t12-wide", "T3", "T3-wide", "first-strip", "last-strip-wide"])
def test_snake_exits(T, t_spike, path, amp):
    """snake_aa_kernel, split-f16 output: one input sample of +-2500 pushes one output frame of its channel beyond the
    range, one of +-12000 three neighbouring ones (a thread owns a strip of 8 frames of one channel).
    value_domain.snake_ref decides which outputs lie beyond 1023.5; they must all lie in strips of the exit under test; then 1 <= count <= their number, and 0 when there is none.
    No exact threshold here: every output is a 12-tap filter of the activation of a 12-tap filter of the input (f32 sums of
    products with the kaiser-sinc taps, plus sin^2 / beta), so no input makes an output equal 1023.5 or its neighbour bit for
    bit; and an Inf input meets taps of both signs (Inf - Inf = NaN: out of scope).  The conversion behind it is f16s_split,
    whose threshold the cast / LayerNorm / GEMM sites pin.  Accounting: twice the launch counts twice; the two utterances as
    separate launches count what the one call counts and give the same bits."""
    ops = _ops()
    C, B = 288, 2
    f = vd.kaiser_sinc12()
    g = torch.Generator().manual_seed(T + t_spike)
    x0 = torch.randn(B, C, T, generator=g) * 0.5
    al, be = (torch.randn(C, generator=g) * 0.3).exp(), (torch.randn(C, generator=g) * 0.3).exp()

    def launch(x):
        nb = x.shape[0]
        y = ops.snake_aa(x.transpose(1, 2).contiguous().to(DEV), al.to(DEV), be.to(DEV), f.tolist(), B=nb, T=T, C_=C,
                         out_dtype=torch.float16)
        return y.view(nb * T, 2 * C)

    def run(x):
        ref = vd.snake_ref(x, al, be, f).transpose(1, 2).contiguous()           # [B, T, C]
        beyond = _clear_of_the_limit(ref, "f16s")
        beyond = beyond * torch.sign(ref).to(torch.int64)                       # 0: in range, +-1: beyond it on that side
        return launch(x), beyond

    with counting() as cnt:
        y, beyond = run(x0)
        assert not bool(beyond.any()) and _count(cnt, "f16s") == 0 and _finite(y)
        for sign in (1.0, -1.0):
            for b, c in ((0, 0), (1, 257), (1, C - 1)):
                x = x0.clone()
                x[b, c, t_spike] = sign * amp
                y, beyond = run(x)
                where = beyond.nonzero().tolist()
                assert where and all(bb == b and cc == c for bb, _, cc in where), where
                strips = {t // si.SN_TS for _, t, _ in where}
                assert {si.snake_strip_path(T, s) for s in strips} == {"fast" if path == "fast" else "generic"}, (strips, where)
                n = _count(cnt, "f16s")
                assert len(strips) <= n <= len(where), (n, where)
                assert _finite(y)
                for bb, t, cc in where:
                    assert _at(y, "f16s", bb * T + t, cc) == int(beyond[bb, t, cc]) * LIM["f16s"]
                assert int(beyond[b, t_spike, c]) == int(sign)
        # accounting
        x = x0.clone()
        x[0, 0, t_spike], x[1, 257, t_spike], x[1, 5, t_spike] = amp, -amp, amp
        y, beyond = run(x)
        n = _count(cnt, "f16s")
        assert 3 <= n <= int(beyond.abs().sum())
        launch(x)
        launch(x)
        assert _count(cnt, "f16s") == 2 * n
        parts = torch.cat([launch(x[0:1]), launch(x[1:2])])
        assert _count(cnt, "f16s") == n and torch.equal(parts.view(torch.uint8), y.view(torch.uint8))
        keep = cnt.clone()
    launch(x)
    torch.cuda.synchronize()
    assert torch.equal(cnt, keep)


# -------------------------------------------------------------------------------------------------------------- GEMM
def G(name, kind, M, N, K, *, tile, waves, plain, body, act=False, taps=1, t=None, skinny=0, ldc_pad=None, ldr_pad=4):
    return dict(name=name, kind=kind, M=M, N=N, K=K, tile=tile, waves=waves, plain=plain, body=body, act=act, taps=taps, t=t,
                skinny=skinny, ldc_pad=ldc_pad, ldr_pad=ldr_pad)


# tile = rows of the geometry; body = the epilogue body compiled in (0 none, 1 GELU, 2 chosen by `act` at run time: the
# implicit-conv staging); K = one slice (plain) or a shape the plain staging refuses (taps = 3, or fp8 K % 128 != 0)
GEMM_CASES = [
    G("f16s-128x128-plain", "f16s", 200, 160, 32, tile=128, waves=4, plain=1, body=0),
    G("f16s-128x128-plain-gelu", "f16s", 200, 160, 32, tile=128, waves=4, plain=1, body=1, act=True),
    G("f16s-128x128-conv-gelu", "f16s", 200, 160, 32, tile=128, waves=4, plain=0, body=2, act=True, taps=3, t=100),
    G("f16s-64x128-plain", "f16s", 600, 160, 32, tile=64, waves=4, plain=1, body=0),
    G("f16s-64x128-conv", "f16s", 600, 160, 32, tile=64, waves=4, plain=0, body=2, taps=3, t=100),
    G("f16s-128x256-plain", "f16s", 2850, 2048, 32, tile=128, waves=8, plain=1, body=0),
    G("f16s-192x256-plain", "f16s", 32800, 256, 32, tile=192, waves=8, plain=1, body=0),
    G("f16s-256x256-plain-gelu", "f16s", 16330, 768, 32, tile=256, waves=8, plain=1, body=1, act=True),
    G("f16s-256x256-conv-gelu", "f16s", 16330, 768, 32, tile=256, waves=8, plain=0, body=2, act=True, taps=3, t=115),
    G("f16s-256x256-conv", "f16s", 16330, 768, 32, tile=256, waves=8, plain=0, body=2, taps=3, t=115),
    G("fp8-128x128-plain", "fp8", 200, 160, 128, tile=128, waves=4, plain=1, body=0),
    G("fp8-128x128-plain-gelu", "fp8", 200, 160, 128, tile=128, waves=4, plain=1, body=1, act=True),
    G("fp8-128x128-ktail-gelu", "fp8", 200, 160, 64, tile=128, waves=4, plain=0, body=2, act=True),
    G("fp8-128x128-conv", "fp8", 200, 160, 128, tile=128, waves=4, plain=0, body=2, taps=3, t=100),
    G("fp8-128x128-scalar-tail", "fp8", 200, 152, 128, tile=128, waves=4, plain=1, body=0, ldc_pad=8),    # N cuts a lane's 16 columns
    G("fp8-128x128-scalar-ldc", "fp8", 200, 160, 128, tile=128, waves=4, plain=1, body=0, ldc_pad=8),     # ldc % 16 != 0: all scalar
    G("fp8-128x256-plain", "fp8", 2850, 2048, 128, tile=128, waves=8, plain=1, body=0),
    G("fp8-192x256-plain", "fp8", 32800, 256, 128, tile=192, waves=8, plain=1, body=0),
    G("fp8-256x256-plain-gelu", "fp8", 16330, 768, 128, tile=256, waves=8, plain=1, body=1, act=True),
    G("fp8-256x256-conv", "fp8", 16330, 768, 128, tile=256, waves=8, plain=0, body=2, taps=3, t=115),
]
SKINNY_CASES = [
    G("skinny-vector", "f16s", 1200, 160, 192, tile=64, waves=4, plain=0, body=2, taps=3, t=100, skinny=1),
    G("skinny-vector-gelu", "f16s", 1200, 160, 192, tile=64, waves=4, plain=0, body=2, act=True, taps=3, t=100, skinny=1),
    G("skinny-tail", "f16s", 1200, 160, 192, tile=64, waves=4, plain=0, body=2, taps=3, t=100, skinny=1, ldr_pad=1),   # ldr % 4 != 0
]


class _Gemm:
    """one case's operands on the device and its float64 reference without the residual"""

    def __init__(self, case):
        ops = _ops()
        self.c = c = case
        kind, M, N, K, taps = c["kind"], c["M"], c["N"], c["K"], c["taps"]
        g = torch.Generator().manual_seed(M + N + K + taps)
        A = torch.randn(M, K, generator=g) * 0.5
        W = torch.randn(N, taps * K, generator=g) * (taps * K) ** -0.5
        self.bias = (torch.randn(N, generator=g) * 0.3).to(DEV)
        self.res0 = torch.randn(M, N, generator=g) * 0.5
        self.ldr = N + c["ldr_pad"]
        self.resd = _embed(self.res0.to(DEV), self.ldr, 2, 260)            # rows behind, padding columns: big values
        self.resz = _embed(torch.zeros(M, N, device=DEV), self.ldr, 2, 260)
        if kind == "f16s":
            sa, sw, lpad, cw = 64.0, 2.0 ** 12, 32, 2
            Ad, Wd = ops.cast_f16s(A.to(DEV), K, scale=sa), ops.cast_f16s(W.to(DEV), taps * K, scale=sw)
            Aq, Wq = _unsplit(Ad, K, sa), _unsplit(Wd, taps * K, sw)
        else:
            sa, lpad, cw = 16.0, 16, 1
            sw = 2.0 ** math.floor(math.log2(448.0 / float(W.abs().max())))
            Ad, Wd = ops.cast_fp8(A.to(DEV), sa), ops.cast_fp8(W.to(DEV), sw)
            Aq, Wq = Ad.float().cpu().double() / sa, Wd.float().cpu().double() / sw
        self.lda, self.ldw = K + lpad, taps * K + lpad
        self.a = _embed(Ad, cw * self.lda, 3, 260)
        self.a0 = _embed(torch.zeros_like(Ad), cw * self.lda, 3, 260)       # exact zeros: the output is the residual, exactly
        self.w = _embed(Wd, cw * self.ldw, 1, 260)
        self.alpha = 1.0 / (sa * sw)
        self.ldc = N + (c["ldc_pad"] if c["ldc_pad"] is not None else (32 if kind == "f16s" else 16))
        self.conv = dict(taps=taps, pad=(taps - 1) // 2, t_in=c["t"], t_out=c["t"]) if taps > 1 else {}
        base = self._product(Aq, Wq) + self.bias.double().cpu()
        self.base = F.gelu(base) if c["act"] else base

    def _product(self, A, W):
        c = self.c
        M, K, taps, t = c["M"], c["K"], c["taps"], c["t"]
        if taps == 1:
            return A @ W.T
        B, pad = M // t, (taps - 1) // 2
        x = torch.zeros(B, t + 2 * pad, K, dtype=torch.float64)
        x[:, pad:pad + t] = A.view(B, t, K)
        out = torch.zeros(B, t, W.shape[0], dtype=torch.float64)
        for tap in range(taps):
            out += x[:, tap:tap + t] @ W[:, tap * K:(tap + 1) * K].T
        return out.view(M, -1)

    def launch(self, edits=(), *, zero=False, rows=None, check_plan=False, guard=False):
        """One swc_gemm call on rows [first, end) (default: all).  The residual is the case's in-range one with `edits`
        [(row, col, value)] written over it; zero: exact zeros for A, no bias and a residual of zeros + edits, so that the edited
        values reach the conversion exactly.  -> the output window [rows, storage columns]"""
        ops = _ops()
        c = self.c
        kind, N, K = c["kind"], c["N"], c["K"]
        r0, r1 = rows or (0, c["M"])
        n = r1 - r0
        cw = 2 if kind == "f16s" else 1
        res = self.resz if zero else self.resd
        for r, col, v in edits:
            res[r, col] = v
        out, check = poison.guarded((n, cw * N), _dt(kind), ld=cw * self.ldc, device=DEV)
        kw = dict(out=out, lda=self.lda, ldw=self.ldw, ldc=self.ldc, alpha=self.alpha, residual=res[r0:r1], ldr=self.ldr,
                  act=ops.ACT_GELU if c["act"] else ops.ACT_NONE, out_scale=SCALE[kind], **self.conv)
        if not zero:
            kw["bias"] = self.bias
        a = (self.a0 if zero else self.a)[r0:r1]
        if check_plan:
            p = ops.gemm_call_plan(a, self.w, n, N, K, **kw)
            got = (p["tile_m"], p["waves"], p["plain"], p["act_body"], p["skinny"])
            assert got == (c["tile"], c["waves"], c["plain"], c["body"], c["skinny"]), p
            assert p["tile_n"] == (128 if c["waves"] == 4 else 256), p
        ops.gemm(a, self.w, n, N, K, **kw)
        for r, col, _ in edits:                           # (stream order: behind the launch)
            res[r, col] = 0.0 if zero else float(self.res0[r, col])
        if guard:
            torch.cuda.synchronize()
            check()
        return out

    def reference(self, edits):
        """float64 act(A W^T + bias) + residual with the edits, on the operands as stored"""
        res = self.res0.double()
        for r, col, v in edits:
            res[r, col] = v
        return self.base + res


def _unsplit(y, cols, scale):
    y = y.cpu().double().view(y.shape[0], cols // 32, 2, 32)
    return (y[:, :, 0] + y[:, :, 1]).reshape(y.shape[0], cols) / scale


def _gemm_site(case):
    kind, M, N = case["kind"], case["M"], case["N"]
    BM, BN = case["tile"], 128 if case["waves"] == 4 else 256
    lim, big = LIM[kind], OUTLIER[kind]
    gm = _Gemm(case)
    assert float(gm.reference([]).abs().max()) < lim * (1 - MARGIN) / 2     # in range; 4 x the limit on top of it stays beyond

    def spiked(spots):
        edits = [(r, c, big * (-1) ** i) for i, (r, c) in enumerate(spots)]
        beyond = _clear_of_the_limit(gm.reference(edits), kind)
        assert beyond.nonzero().tolist() == sorted([r, c] for r, c in spots)
        return edits

    with counting() as cnt:
        # silence: big finite values before / behind A, W and the residual and in their padding columns, none inside
        y = gm.launch(check_plan=True, guard=True)
        assert _count(cnt, kind) == 0 and _finite(y)
        # position: first / last row of a tile, the tail rows of M % tile, each wave's columns, each quarter of a wave's 64
        # columns, the last 32-block of N
        tail0 = (M // BM) * BM if M % BM else M - BM
        rows = sorted({0, BM - 1, min(BM, M - 1), tail0, M - 1, tail0 - 1})
        cols = sorted({0, 17, 34, 51, 64 + 3, 127, min(BN - 1, N - 1), min(BN, N - 1), N - 32, N - 17, N - 1} & set(range(N)))
        spots = [(rows[i % len(rows)], c) for i, c in enumerate(cols)] + [(r, cols[(3 * i) % len(cols)]) for i, r in enumerate(rows)]
        for i, (r, c) in enumerate(dict.fromkeys(spots)):
            v = big * (-1) ** i
            assert abs(float(gm.base[r, c]) + v) > lim * (1 + MARGIN)
            y = gm.launch([(r, c, v)])
            assert _count(cnt, kind) == 1, (r, c)
            assert _at(y, kind, r, c) == lim * (-1) ** i, (r, c, _at(y, kind, r, c))
        # k outliers in k different tiles
        tiles = [(0, 0), ((M - 1) // BM, (N - 1) // BN), ((M - 1) // BM, 0), (min(1, (M - 1) // BM), (N - 1) // BN)]
        spots = sorted({(min(i * BM + 5, M - 1), min(j * BN + 7, N - 1)) for i, j in dict.fromkeys(tiles)})
        edits = spiked(spots)
        y = gm.launch(edits)
        assert _count(cnt, kind) == len(spots) and _finite(y)
        # accounting: the count adds up over launches, and over the same rows run as separate launches
        gm.launch(edits)
        gm.launch(edits)
        assert _count(cnt, kind) == 2 * len(spots)
        cut = (M // 2 // (case["t"] or 1)) * (case["t"] or 1)
        for e in edits:
            gm.resd[e[0], e[1]] = e[2]
        ya = gm.launch(rows=(0, cut), check_plan=bool(case["skinny"]))
        yb = gm.launch(rows=(cut, M), check_plan=bool(case["skinny"]))
        for r, c, _ in edits:
            gm.resd[r, c] = float(gm.res0[r, c])
        assert _count(cnt, kind) == len(spots)
        assert torch.equal(torch.cat([ya, yb]).view(torch.uint8), y.contiguous().view(torch.uint8))
        # threshold: exact zeros for A and no bias, so (GELU of) 0 + residual reaches the conversion exactly
        r, c = M - 1, N - 1
        for v, counted, stored in _threshold_series(kind):
            mate = [(0, 0, -v)] if counted == 0 else []                        # the limit of the other sign beside it
            y = gm.launch([(r, c, v)] + mate, zero=True)
            assert _count(cnt, kind) == counted, v
            assert _at(y, kind, r, c) == stored and _finite(y), (v, _at(y, kind, r, c))
            assert not mate or _at(y, kind, 0, 0) == -stored
        keep = cnt.clone()
    gm.launch(edits)
    torch.cuda.synchronize()
    assert torch.equal(cnt, keep)


@pytest.mark.parametrize("case", GEMM_CASES, ids=lambda c: c["name"])
def test_gemm_sites(case):
    """swc_gemm's direct epilogue with split-f16 and fp8 outputs in each geometry the chooser has (asserted from the plan).  The
    outlier rides on the f32 residual, which is added after bias and activation and before the conversion: the float64
    reference is act(A W^T + bias) + residual on the operands as stored.  The slab epilogue is compiled for f32 outputs only
    (tests/test_sat_sites_cpu.py pins the gate): fp8 outputs of every geometry pass here through the direct one."""
    _gemm_site(case)


@pytest.mark.parametrize("case", SKINNY_CASES, ids=lambda c: c["name"])
def test_skinny_sites(case):
    """the skinny geometry (swc_gemm_skinny.hip, k3 convolution of 3 x 192 = 576 >= 512 reduction elements over 1200 rows, whose halves
    of 600 rows take it as well): its vector path and, with a residual pitch that breaks 16-byte rows, its tail path"""
    _gemm_site(case)


# ----------------------------------------------------------------------------------------------------------- proj_ln
def test_proj_ln_y_next():
    """swc_proj_ln: LayerNorm(x + alpha A W^T + bias) -> split-f16.  M = 77: one full 64-token tile and a tail of 13; a thread
    owns 4 columns (256 k + 4 lane) of the rows 8 w + i and 32 + 8 w + i of its wave w."""
    ops = _ops()
    M, N, K = 77, 768, 64
    g = torch.Generator().manual_seed(5)
    A, W = torch.randn(M, K, generator=g) * 0.5, torch.randn(N, K, generator=g) * K ** -0.5
    bias = torch.randn(N, generator=g) * 0.2
    sa, sw = 64.0, 2.0 ** 12
    As, Ws = ops.cast_f16s(A.to(DEV), K, scale=sa), ops.cast_f16s(W.to(DEV), K, scale=sw)
    stream = ops.proj_ln_pack(Ws)
    prod = _unsplit(As, K, sa) @ _unsplit(Ws, K, sw).T + bias.double()
    a = _embed(As, 2 * (K + 64), 2, 70)
    cols = [0, 3, 255, 256, 511, 764, 767]

    def launch(x, w, b, rows=(0, M)):
        r0, r1 = rows
        xd = _embed(x[r0:r1].to(DEV), N, 1, 70)                              # rows behind x: big values
        out = torch.empty(r1 - r0, N, device=DEV)
        _, y = ops.proj_ln(a[r0:r1], stream, bias.to(DEV), 1.0 / (sa * sw), xd, M=r1 - r0, N=N, K=K, lda=K + 64, x_out=out,
                           ln=(w.to(DEV), b.to(DEV)))
        return y

    def run(spikes, seed=0, parts=((0, M),)):
        x, w, b = _ln_inputs("f16s", N, M, spikes, seed)
        ref = vd.ln_ref((x.double() + prod).float(), w, b, 1e-5)            # LayerNorm of the f32 x_out the kernel stores
        beyond = _clear_of_the_limit(ref, "f16s")
        assert beyond.nonzero().tolist() == sorted([r, c] for r, c in spikes)
        return torch.cat([launch(x, w, b, rows) for rows in parts])

    with counting() as cnt:
        y = run([])
        assert _count(cnt, "f16s") == 0 and _finite(y)
        # threshold: weight 0 and bias v on one column give 0 * xhat + v = v exactly; one row = one thread converts it
        x1 = torch.randn(M, N, generator=g)
        for col in (0, 255, 256, N - 1):
            for v, counted, stored in _threshold_series("f16s"):
                b = torch.zeros(N)
                b[col] = v
                y = launch(x1, torch.zeros(N), b, rows=(0, 1))
                assert _count(cnt, "f16s") == counted, (col, v)
                assert _at(y, "f16s", 0, col) == stored and _finite(y), (col, v, _at(y, "f16s", 0, col))
        for i, r in enumerate((0, 7, 8, 31, 32, 63, 64, 76)):
            c = cols[i % len(cols)]
            y = run([(r, c)], seed=i)
            assert _count(cnt, "f16s") == 1, (r, c)
            assert abs(_at(y, "f16s", r, c)) == LIM["f16s"] and _finite(y)
        many = [(0, 0), (8, 255), (16, 256), (24, 767), (70, 4)]                   # five waves' rows: five threads
        y = run(many)
        assert _count(cnt, "f16s") == 5
        run(many)
        run(many)
        assert _count(cnt, "f16s") == 10
        # the same rows as three launches (cuts inside a tile and inside a wave's rows): the same count, the same bits
        y3 = run(many, parts=((0, 12), (12, 40), (40, M)))
        assert _count(cnt, "f16s") == 5 and torch.equal(y3.view(torch.uint8), y.view(torch.uint8))
        keep = cnt.clone()
    run(many)
    torch.cuda.synchronize()
    assert torch.equal(cnt, keep)


# -------------------------------------------------------------------------------------------------------- layer_tail
def test_layer_tail_fp8_ln():
    """swc_layer_tail with fp8 fc1: LayerNorm(x'), x' = x + attn Wo^T + bo, goes to LDS as e4m3 at scale 16.  M = 77 (a tail of 13
    tokens in the second 64-token tile).  Tokens >= M are computed on x = 0 and a copy of the last row's attention and never
    stored; they must not count either: `silent` gives exactly those tokens an out-of-range LayerNorm output (a column where
    bo = 1e4 and every live row of x holds -1e4)."""
    ops = _ops()
    M, D, F_ = 77, 768, 256
    g = torch.Generator().manual_seed(9)
    att = (torch.randn(M, D, generator=g) * 0.7).to(torch.bfloat16)
    wo = (torch.randn(D, D, generator=g) * D ** -0.5).to(torch.bfloat16)
    w1f = torch.randn(F_, D, generator=g) * D ** -0.5
    w2 = (torch.randn(D, F_, generator=g) * F_ ** -0.5).to(torch.bfloat16)
    b1, b2 = torch.randn(F_, generator=g) * 0.3, torch.randn(D, generator=g) * 0.3
    sw = 2.0 ** math.floor(math.log2(448.0 / float(w1f.abs().max())))
    wts = ops.layer_tail_pack(wo.to(DEV), ops.cast_fp8(w1f.to(DEV), sw), w2.to(DEV))
    proj = att.double() @ wo.double().T
    cols = [0, 3, 4, 191, 192, 763, 767]

    def launch(x, w, b, bo, rows=(0, M)):
        r0, r1 = rows
        xd = _embed(x[r0:r1].to(DEV), D, 1, 70)
        ad = _embed(att[r0:r1].to(DEV), D, 1, 70)
        out = torch.empty(r1 - r0, D, device=DEV)
        ops.layer_tail(ad, xd, wts, bo.to(DEV), w.to(DEV), b.to(DEV), 1e-5, b1.to(DEV), b2.to(DEV), M=r1 - r0, D=D, F=F_, x_out=out,
                       fc1_dtype=ops.FP8_T, fc1_alpha=1.0 / (ops.FP8_ACT_SCALE * sw))
        assert _finite(out)
        return out

    def run(spikes, seed=0, silent=False, parts=((0, M),)):
        x, w, b = _ln_inputs("fp8", D, M, spikes, seed)
        bo = torch.randn(D, generator=torch.Generator().manual_seed(seed + 100)) * 0.2
        if silent:
            bo[100], x[:, 100], w[100] = 1e4, -1e4, 4.0
            pad_row = F.layer_norm(proj[M - 1] + bo.double(), (D,), w.double(), b.double(), 1e-5)
            assert float(pad_row.abs().max()) > LIM["fp8"] * 2                     # what a token >= M would convert
        ref = vd.ln_ref((x.double() + proj + bo.double()).float(), w, b, 1e-5)
        beyond = _clear_of_the_limit(ref, "fp8")
        assert beyond.nonzero().tolist() == sorted([r, c] for r, c in spikes)
        return torch.cat([launch(x, w, b, bo, rows) for rows in parts])

    with counting() as cnt:
        run([])
        assert _count(cnt, "fp8") == 0
        run([], silent=True)
        assert _count(cnt, "fp8") == 0, "tokens beyond M were counted"
        # threshold: weight 0 and bias v on one column make LayerNorm(x') = v there exactly.  The e4m3 operand stays in LDS, so
        # only the count is visible: +-28 silent, the next float32 and +-Inf counted once — by the ONE live token of an M = 1
        # call, whose 63 padding tokens convert the same v and must stay silent
        x1 = torch.randn(M, D, generator=g)
        for col in (0, 191, 192, D - 1):
            for v, counted, _ in _threshold_series("fp8"):
                b = torch.zeros(D)
                b[col] = v
                launch(x1, torch.zeros(D), b, torch.zeros(D), rows=(0, 1))
                assert _count(cnt, "fp8") == counted, (col, v)
        for i, r in enumerate((0, 15, 16, 31, 32, 63, 64, 76)):
            run([(r, cols[i % len(cols)])], seed=i)
            assert _count(cnt, "fp8") == 1, (r, cols[i % len(cols)])
        many = [(0, 0), (1, 192), (40, 384), (70, 767)]
        out = run(many)
        assert _count(cnt, "fp8") == 4
        run(many)
        run(many)
        assert _count(cnt, "fp8") == 8
        # the same rows as three launches, each with padding tokens behind its last row: the same count, the same bits
        out3 = run(many, parts=((0, 1), (1, 50), (50, M)))
        assert _count(cnt, "fp8") == 4 and torch.equal(out3, out)
        keep = cnt.clone()
    run(many)
    torch.cuda.synchronize()
    assert torch.equal(cnt, keep)


# ------------------------------------------------------------------------------------------------------ attention_ex
def test_attention_ex_saturates_uncounted():
    """swc_attention_ex with split-f16 output (include/swc.h): the weighted sum of f32 v is not bounded, is stored as the
    finite limit +-65504 / 64 and is NOT counted; nothing in the package takes this form."""
    ops = _ops()
    B, T, H = 1, 16, 1
    qkv = torch.zeros(B, T, 3 * 64, device=DEV)
    qkv[:, :, 128:160] = 5000.0
    qkv[:, :, 160:192] = -5000.0
    lens = torch.tensor([T], dtype=torch.int32, device=DEV)
    with counting() as cnt:
        y = ops.attention(qkv, lens, B, T, H, out_dtype=torch.float16).view(T, 128)
        torch.cuda.synchronize()
        assert cnt.tolist() == [0, 0]
    assert _finite(y)
    for r in (0, T - 1):
        assert _at(y, "f16s", r, 0) == LIM["f16s"] and _at(y, "f16s", r, 63) == -LIM["f16s"]
