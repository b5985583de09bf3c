"""The index-math case tables of the fused kernels, shared by tests/test_fused_index_cpu.py and tests/test_fused_index_gpu.py:
the attention kernels (csrc/swc_attention.hip: f32, legacy bf16, f32 -> split-f16; csrc/swc_attention16.hip: bf16 and
split-f16, padded and packed), the front half of swc_convnext_block (csrc/swc_convnext.hip: depthwise k7 + LayerNorm inside
the fused kernel, with its window, its utterance test and its t_limit loop) and the M tail of swc_layer_tail / swc_mlp_block.

Laid out like tests/stage_index.py: per kernel a table of the smallest shapes that reach each branch of its index arithmetic,
a float64 reference, and predicates that restate the kernel's own conditions (source lines quoted in the docstrings) and so
name the branches a case takes.  REQUIRED lists every branch per kernel form; the CPU test fails when one has no case, and
when a case could be deleted without uncovering a branch.

On top of that a FAULT MODEL: a float64 restatement of each kernel's walk (attn_walk, block_walk) with switchable faults.
The CPU test runs the criteria of the GPU test on the faulty walks and shows that the case named for the branch fails.

Host only: nothing here touches a device.
"""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

from simwhisper_codec_amd import spec


def _g(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


# =========================================================================================================== attention
KT = 64                         # `constexpr int KT = 64;` / `KT16` = 64 in both launches of swc_attention16: keys per tile
# queries per workgroup, per wave, and 16-query MFMA tiles per wave, of every form ops.attention can reach
ATT_FORMS = {
    "f32":         dict(qb=64, qw=16, sixteen=False),      # attn_kernel<false>
    "f32->f16s":   dict(qb=64, qw=16, sixteen=False),      # attn_kernel<false, true> (swc_attention_ex)
    "bf16 legacy": dict(qb=64, qw=16, sixteen=False),      # attn_kernel<true> (ops.LEGACY_ATTENTION)
    "bf16":        dict(qb=128, qw=32, sixteen=True),      # attn16_kernel<1, 64, 2>
    "f16s":        dict(qb=128, qw=32, sixteen=True),      # attn16_kernel<2, 64, 2>
}
ATT_PACKED = ("bf16", "f16s")   # the forms that take row_start
ATT_BF16_SOURCE = ("bf16 legacy", "bf16")       # forms whose q/k/v are rounded to bf16 (the reference is taken on the rounded values)
LARGEST_T = spec.token_len(spec.CHUNK_SAMPLES)  # the encoder's tokens of a 30 s window: the longest row the codec launches

TRAP_MULT = 8.0                 # trap key and query rows: this multiple of a valid row
TRAP_V = 500.0                  # trap value rows: a constant far from every valid value (|v| < 4), exact in bf16
TRAP_LIMIT = 1023.0             # everything stays below the split-f16 range (include/swc.h: |x| <= 1023.5)
TRAP_MARGIN = 40.0


def A(name, T, lens, H, model=True):
    return dict(name=name, T=T, lens=tuple(int(v) for v in lens), H=H, model=model)


ATT_CASES = [
    A("dense", 193, range(194), 2),                       # B = T + 1 utterances of lengths 0 .. T: every length at once
    A("T128", 128, (128, 127, 1, 0, 70), 3),
    A("T63", 63, (63, 0, 0, 62, 17), 2),
    A("T192", 192, (0, 192, 191, 5), 2),
    A("T127", 127, (127, 126, 0), 2),
    A("T15", 15, (15, 14, 1, 0, 7), 2),
    A("T1", 1, (1, 0, 1), 1),
    A("T-largest", LARGEST_T, (LARGEST_T,), 2),
    A("H12", 70, (70, 33), 12),
    A("clamp", 65, (-3, 70, 65), 2),
    A("B65535", 1, [b % 3 != 1 for b in range(65535)], 2, model=False),    # (the walk model adds nothing to T1 here)
]


def att_case(name):
    return next(c for c in ATT_CASES if c["name"] == name)


def eff_lens(lens, T):
    """`len = len < 0 ? 0 : (len > T ? T : len);` (both kernels)"""
    return [0 if n < 0 else (T if n > T else n) for n in lens]


def row_starts(lens, T):
    """the packed layout: utterance b's valid rows follow those of b - 1 -> (row_start, total rows)"""
    e = eff_lens(lens, T)
    rs, total = [], 0
    for n in e:
        rs.append(total)
        total += n
    return rs, total


def attn_branches(form, T, lens, H, packed=False):
    """The branches one launch takes.
    `if (q0 >= len) {  // whole block is padding` (both kernels); `const int ntile = (len + KT16 - 1) / KT16;`;
    `if (LAST) v = key < len ? v : -INFINITY;` on tile ntile - 1 only; `const int st = RES ? kt : (kt & 1);`;
    `q = q < len ? q : len - 1;` (16-bit kernel: query columns beyond the length inside a valid block);
    `const long r0 = row_start ? (long)row_start[b] : (long)b * T;` and `const int qlim = row_start ? len : T;`"""
    f = ATT_FORMS[form]
    qb, qw = f["qb"], f["qw"]
    out = {f"H={H}"} if H in (1, 3, 12) else set()
    if T % 128 == 0:
        out.add("T%128=0")
    elif T % 64 == 0:
        out.add("T%128=64")
    if T % 64 in (1, 63):
        out.add(f"T%64={T % 64}")
    if 1 < T < 16:
        out.add("T<16")
    if T == 1:
        out.add("T=1")
    if T == LARGEST_T:
        out.add("T=largest")
    if len(lens) == 65535:
        out.add("B=65535")
    for raw, n in sorted(set(zip(lens, eff_lens(lens, T)))):
        if raw < 0:
            out.add("len<0")
        if raw > T:
            out.add("len>T")
        if n in (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193):
            out.add(f"len={n}")
        if 1 < n < 16:
            out.add("len<16")
        if n == T - 1:
            out.add("len=T-1")
        if n == T:
            out.add("len=T")
        if n == 0:
            continue
        ntile = (n + KT - 1) // KT
        out.add(f"ntile={min(ntile, 4)}" + ("+" if ntile > 4 else ""))
        if n % KT == 0:
            out.add("last-tile-full")
        if n % KT == 1:
            out.add("last-tile-one-key")
        for q0 in range(0, T, qb):
            if q0 >= n:
                out.add("block-beyond-len")
                continue
            for w in range(4):
                qw0 = q0 + w * qw
                if qw0 >= T:
                    continue
                if qw0 >= n:
                    out.add("wave-beyond-len")
                elif f["sixteen"] and qw0 + 16 >= n and qw0 + 16 < T:
                    out.add("tile16-beyond-len")
    if packed:
        e = eff_lens(lens, T)
        rs, _ = row_starts(lens, T)
        out.add("ends-at-last-row")
        if e[0] == 0:
            out.add("empty-first")
        if e[-1] == 0:
            out.add("empty-last")
        if any(e[b] == 0 and e[b + 1] == 0 for b in range(len(e) - 1)):
            out.add("empty-twice")
        if any(e[b] > 0 and rs[b] != b * T for b in range(len(e))):
            out.add("packed-rows-shifted")
    return out


_ATT_COMMON = ({f"len={n}" for n in (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193)}
               | {"len<16", "len=T-1", "len=T", "len<0", "len>T", "ntile=1", "ntile=2", "ntile=3", "ntile=4", "ntile=4+",
                  "last-tile-full", "last-tile-one-key", "block-beyond-len", "wave-beyond-len", "T%128=0", "T%128=64",
                  "T%64=1", "T%64=63", "T<16", "T=1", "T=largest", "H=1", "H=3", "H=12", "B=65535"})
_ATT_PACKED = {"ends-at-last-row", "empty-first", "empty-last", "empty-twice", "packed-rows-shifted"}


@functools.lru_cache(maxsize=None)
def attn_base(name):
    """(read-only: cached) the f32 q | k | v of a case before the traps: [B, T, 3 * H * 64], the distribution of test_attention"""
    c = att_case(name)
    return torch.randn(len(c["lens"]), c["T"], 3 * c["H"] * 64, generator=_g("attn", name)) * 0.7


def with_traps(qkv, lens, T, H, zeros=False):
    """Rows at and beyond the (clamped) length of the padded layout as hostile data (zeros=True: as zeros).  Trap key row t is
    TRAP_MULT x the valid QUERY row t % len, head by head (its score beats every valid score of that query by more than
    TRAP_MARGIN: a masked key that leaked would own the softmax); trap query row t is TRAP_MULT x the LAST VALID KEY row (its
    maximum jumps in the last key tile: read by a wave, it triggers the bf16 kernel's wave-uniform rescale); trap value rows
    hold TRAP_V.  An empty utterance (never read) holds TRAP_MULT, TRAP_MULT, TRAP_V."""
    out = qkv.clone()
    D = H * 64
    for b, n in enumerate(eff_lens(lens, T)):
        if n == T:
            continue
        if zeros:
            out[b, n:] = 0
        elif n == 0:
            out[b, :, :2 * D] = TRAP_MULT
            out[b, :, 2 * D:] = TRAP_V
        else:
            j = torch.arange(n, T) % n
            out[b, n:, D:2 * D] = TRAP_MULT * qkv[b, j, :D]
            out[b, n:, :D] = TRAP_MULT * qkv[b, n - 1, D:2 * D]
            out[b, n:, 2 * D:] = TRAP_V
    return out


@functools.lru_cache(maxsize=None)
def attn_input(name):
    """(read-only: cached) the f32 input of a case, traps in place"""
    c = att_case(name)
    if c["T"] == 1:                 # (B = 65535: vectorised)
        out = attn_base(name).clone()
        D = c["H"] * 64
        empty = torch.tensor(eff_lens(c["lens"], 1)) == 0
        out[empty, :, :2 * D] = TRAP_MULT
        out[empty, :, 2 * D:] = TRAP_V
        return out
    return with_traps(attn_base(name), c["lens"], c["T"], c["H"])


def source(qkv, form):
    """what the form's kernel is handed, as float64: rounded to bf16 for the bf16 forms (as test_attention / test_attention16)"""
    return (qkv.bfloat16() if form in ATT_BF16_SOURCE else qkv).double()


def attn_ref(src, lens, T, H):
    """float64 [B, T, H * 64]: row t < len of utterance b is sum_k p[t, k] v[k] over the keys k < len, p = e^(s - max) / sum;
    rows at and beyond the length are zeros (they are don't-care, or not stored)"""
    B, D = src.shape[0], H * 64
    out = torch.zeros(B, T, D, dtype=torch.float64)
    e = eff_lens(lens, T)
    if T == 1:
        return src[:, :, 2 * D:] * (torch.tensor(e) > 0).view(B, 1, 1)
    for b, n in enumerate(e):
        if n == 0:
            continue
        q, k, v = (src[b, :n, i * D:(i + 1) * D].reshape(n, H, 64).transpose(0, 1) for i in range(3))
        s = q @ k.transpose(1, 2)
        p = (s - s.amax(-1, keepdim=True)).exp()
        out[b, :n] = ((p / p.sum(-1, keepdim=True)) @ v).transpose(0, 1).reshape(n, D)
    return out


def trap_margin(src, lens, T, H):
    """min over (utterance, head, trapped query) of [score against its trap key] - [its largest valid score] (inf: no trap)"""
    D, worst = H * 64, float("inf")
    for b, n in enumerate(eff_lens(lens, T)):
        if n == 0 or n == T:
            continue
        q, k = (src[b, :, i * D:(i + 1) * D].reshape(T, H, 64).transpose(0, 1) for i in range(2))
        j = torch.arange(n, T) % n
        trap = (q[:, j] * k[:, n:]).sum(-1)                                   # [H, T - n]
        valid = (q[:, :n] @ k[:, :n].transpose(1, 2)).amax(-1)[:, j]          # [H, T - n]
        worst = min(worst, float((trap - valid).min()))
    return worst


SPIKE = dict(T=200, n=150, H=1, query=10, mult=40.0)


@functools.lru_cache(maxsize=None)
def spike_input():
    """(read-only: cached) one utterance of 150 of 200 rows, as test_attention_spike builds it: key len - 1 is 40 x query 10,
    and key len (masked) is the same row; rows beyond are traps.  -> (with the spike on row len, with row len as zeros)"""
    T, n = SPIKE["T"], SPIKE["n"]
    base = torch.randn(1, T, 192, generator=_g("attn-spike")) * 0.3
    base[0, n - 1, 64:128] = base[0, SPIKE["query"], 0:64] * SPIKE["mult"]
    hot = with_traps(base, (n,), T, 1)
    hot[0, n, 64:128] = base[0, n - 1, 64:128]
    cold = hot.clone()
    cold[0, n] = 0
    return hot, cold


# ------------------------------------------------------------------------------------------- the attention walk, in float64
ATT_FAULTS = {
    # fault: (what it does, the branch whose cases must catch it)
    "mask<=": ("the staging guard `const bool ok = key < len;` and the mask `key < len ? v : -INFINITY` (one condition, stated "
               "twice) read `key <= len`", "len=T-1"),
    "ntile-floor": ("`ntile = len / 64` (floor): the partly filled tile is never walked", "last-tile-one-key"),
    "slot-reuse": ("tile kt >= 2 is computed from the data of tile kt - 2 (its double-buffer slot was not staged again)", "ntile=3"),
    "clamp-len": ("`q = q < len ? q : len` (the first row beyond the length, not the last valid one)", "tile16-beyond-len"),
    "packed-r0": ("packed layout addressed as padded: `r0 = b * T`", "packed-rows-shifted"),
    "head-offset": ("every head reads the keys of head 0", "H=12"),
}
RESCALE_STEP = 8.0 * math.log(2.0)      # `mt > m_run[qt] + 8.0f / c_exp` with c_exp = log2 e: 2^8 in natural-log units


def attn_walk(buf, lens, T, H, form, fault=None, row_start=None):
    """The kernels' walk in float64.  buf: what the kernel is handed, [B, T, 3D] (padded) or [rows, 3D] (packed, with
    row_start).  -> the output buffer of the same layout, NaN where nothing is stored.  A row read beyond the buffer is zeros
    (the model never faults).  Per (utterance, query block of qb, head): key tiles of 64, zero rows staged for keys beyond the
    length, the mask in the last tile only, online softmax.  16-bit forms clamp the query row to len - 1; the f32 forms read
    the query row itself (`q_in ? q : T - 1`).  Form "bf16" moves the reference maximum only when a 16-query tile's ballot
    fires and rounds P to bf16, as the kernel does: that is what makes a don't-care query row visible in a valid one."""
    f = ATT_FORMS[form]
    qb, sixteen, lazy = f["qb"], f["sixteen"], form == "bf16"
    D = H * 64
    flat = buf.reshape(-1, 3 * D)
    nrows = flat.shape[0]
    out = torch.full((nrows, D), float("nan"), dtype=torch.float64)
    packed = row_start is not None

    def rows(idx, c0):          # [n, H, 64] at column c0 of rows idx; rows outside the buffer read as zeros
        ok = (idx >= 0) & (idx < nrows)
        r = flat[idx.clamp(0, nrows - 1)][:, c0:c0 + D] * ok.view(-1, 1)
        return r.view(-1, H, 64).transpose(0, 1)          # [H, n, 64]

    ar = torch.arange(KT)
    for b, n in enumerate(eff_lens(lens, T)):
        r0 = row_start[b] if packed and fault != "packed-r0" else b * T
        qlim = n if packed else T
        for q0 in range(0, T, qb):
            qs = torch.arange(q0, min(q0 + qb, max(qlim, q0)))
            qs = qs[qs < qlim]                             # the rows this block stores
            if q0 >= n:
                qs = qs[r0 + qs < nrows]
                if len(qs):
                    out[r0 + qs] = 0.0
                continue
            allq = torch.arange(q0, q0 + qb)
            if sixteen:
                qrow = torch.where(allq < n, allq, torch.full_like(allq, n if fault == "clamp-len" else n - 1))
            else:
                qrow = torch.where(allq < T, allq, torch.full_like(allq, T - 1))
            Q = rows(r0 + qrow, 0)                         # [H, qb, 64]
            m = torch.full((H, qb), float("-inf"), dtype=torch.float64)
            l = torch.zeros(H, qb, dtype=torch.float64)
            O = torch.zeros(H, qb, 64, dtype=torch.float64)
            ntile = n // KT if fault == "ntile-floor" else (n + KT - 1) // KT
            for kt in range(ntile):
                data = kt - 2 if (fault == "slot-reuse" and kt >= 2) else kt
                keys = data * KT + ar
                ok = (keys <= n) if fault == "mask<=" else (keys < n)
                K = rows(r0 + keys, D) * ok.view(1, -1, 1)
                V = rows(r0 + keys, 2 * D) * ok.view(1, -1, 1)
                if fault == "head-offset":
                    K = K[:1].expand(H, -1, -1)
                S = Q @ K.transpose(1, 2)                  # [H, qb, 64]
                if kt == ntile - 1:
                    mk = kt * KT + ar
                    S = S.masked_fill(~((mk <= n) if fault == "mask<=" else (mk < n)).view(1, 1, -1), float("-inf"))
                mt = S.amax(-1)
                if lazy:                                   # the ballot of one 16-query tile
                    fire = (mt > m + RESCALE_STEP).view(H, qb // 16, 16).any(-1, keepdim=True).expand(-1, -1, 16).reshape(H, qb)
                else:
                    fire = torch.ones(H, qb, dtype=torch.bool)
                m_new = torch.where(fire, torch.maximum(m, mt), m)
                alpha = torch.where(fire, (m - m_new).exp(), torch.ones(()).double())
                alpha = torch.where(torch.isnan(alpha), torch.zeros(()).double(), alpha)
                m = m_new
                P = (S - m.unsqueeze(-1)).exp()
                if lazy:
                    P = P.bfloat16().double()
                l = l * alpha + P.sum(-1)
                O = O * alpha.unsqueeze(-1) + P @ V
            inv = torch.where(l > 0, 1.0 / l, torch.zeros(()).double())
            res = (O * inv.unsqueeze(-1)).transpose(0, 1).reshape(qb, D)
            qs = qs[r0 + qs < nrows]                       # (a store beyond the buffer is dropped: the model never faults)
            if len(qs):
                out[r0 + qs] = res[qs - q0]
    return out.view(buf.shape[:-1] + (D,))


def pack(padded, lens, T):
    """padded [B, T, W] -> packed [sum(lens), W]: the buffer ends at its last row"""
    e = eff_lens(lens, T)
    return torch.cat([padded[b, :n] for b, n in enumerate(e)] + [padded[0, :0]])


def valid_mask(lens, T):
    return torch.arange(T).view(1, T) < torch.tensor(eff_lens(lens, T)).view(-1, 1)


def attn_criteria(run, form, name, packed_too=True):
    """The criteria of the GPU test on a function run(buf, lens, T, H, row_start) -> output buffer in float64 (NaN = not
    stored): values of the valid rows against attn_ref within the form's tolerance, zeros in query blocks wholly beyond the
    length, traps as zeros change nothing in a valid row, packed equals padded.  -> list of the criteria that FAIL."""
    c = att_case(name)
    T, lens, H = c["T"], c["lens"], c["H"]
    src = source(attn_input(name), form)
    cold = source(with_traps(attn_base(name), lens, T, H, zeros=True), form)
    ref, ok = attn_ref(src, lens, T, H), valid_mask(lens, T)
    failed = []
    got = run(src, lens, T, H, None)
    err = (got - ref)[ok]
    if not bool(torch.isfinite(got).all()) or float(err.abs().max() if err.numel() else 0.0) >= ATT_TOL[form]:
        failed.append("values")
    qb = ATT_FORMS[form]["qb"]
    beyond = (torch.arange(T).view(1, T) // qb * qb) >= torch.tensor(eff_lens(lens, T)).view(-1, 1)
    if bool((got[beyond] != 0).any()):
        failed.append("zeros-in-blocks-beyond-len")
    if not torch.equal(run(cold, lens, T, H, None)[ok], got[ok]):
        failed.append("traps-as-zeros")
    if packed_too and form in ATT_PACKED:
        rs, total = row_starts(lens, T)
        gp = run(pack(src, lens, T), lens, T, H, rs)
        if gp.shape[0] != total or not torch.equal(gp, pack(got, lens, T)):
            failed.append("packed-equals-padded")
    return failed


# the tolerances of the existing tests of the same form (tests/test_kernels_gpu.py); no new numbers
ATT_TOL = {
    "f32": 1e-5,           # test_attention: `assert err < (1e-5 if dtype == torch.float32 else 1e-2), (b, L, err)`
    "bf16 legacy": 1e-2,   # test_attention (the same line; runs the legacy kernel when ops.LEGACY_ATTENTION is set)
    "bf16": 1.5e-2,        # test_attention16: `src, tol = qd.float(), 1.5e-2`
    "f16s": 1e-5,          # test_attention16: `src, tol = qkv, 1e-5`
    "f32->f16s": 1e-5,     # (the f32 bound against float64; and within F16S_VS_F32 of the f32 form's output)
}
F16S_VS_F32 = 2e-6         # test_f16s_producers: `assert (a[i, :L] - bb[i, :L]).abs().max().item() < 2e-6`


# ====================================================================================================== ConvNeXt block
CX_BM, CX_C = 128, 512          # frames per workgroup (4 waves x 32 frames, groups of 4), channels
CX_I = (128, 256)               # one and two hidden slices (`I % CX_SL == 0`, CX_SL = 128)
CX_OPERANDS = ("bf16", "f16")
# test_convnext_block_fused: `assert e_ref < 1.5e-2, e_ref` and `assert e_pair < 2e-3, e_pair`;
# test_convnext_block_f16_operands: `assert e16 < 3e-3 and eb < 2e-2, (e16, eb)` (f64 on the UNROUNDED weights there)
CX_TOL = {"bf16": dict(e_ref=1.5e-2, e_pair=2e-3), "f16": dict(e_ref=3e-3)}
BIG_LIMIT = 1 << 30


def X(B, T, I, t_limit=None):
    return dict(B=B, T=T, I=I, t_limit=None if t_limit is None else tuple(t_limit))


BLOCK_CASES = [
    # the utterance border at a wave edge and at the tile edge
    X(3, 124, 128), X(3, 125, 256), X(3, 127, 128), X(3, 128, 256), X(3, 129, 128), X(3, 131, 256), X(3, 132, 128), X(2, 256, 256),
    # T < 7 (and 7, 8): the 10-row window of a group spans several utterances; two tiles and a tail
    X(383, 1, 128), X(130, 2, 256), X(96, 3, 128), X(66, 4, 256), X(44, 6, 128), X(41, 7, 256), X(33, 8, 128),
    X(17, 17, 256), X(1, 257, 128),
    # t_limit
    X(3, 100, 128, (100, 150, BIG_LIMIT)), X(2, 300, 128, (100, 130)), X(2, 200, 256, (200, 0)),
    X(2, 128, 128, (128, 0)), X(8, 40, 256, (0, 0, 0, 5, 0, 0, 40, 40)),
]


def block_tiles(B, T, t_limit, fault=None):
    """the tiles that compute: `for (int b = row0 / fr.T; b <= last / fr.T; ++b) { const int t_lo = (row0 > b * fr.T ? row0 :
    b * fr.T) - b * fr.T;  need = need || t_lo < fr.t_limit[b]; }  if (!need) return;` -> [(tile, needed, utterances, who needs)]"""
    M = B * T
    out = []
    for tile in range((M + CX_BM - 1) // CX_BM):
        row0 = tile * CX_BM
        last = min(row0 + CX_BM - 1, M - 1)
        utts = list(range(row0 // T, last // T + 1))
        if t_limit is None:
            out.append((tile, True, utts, utts))
            continue
        look = utts[:1] if fault == "need-first-only" else utts
        lt = (lambda a, b: a <= b) if fault == "limit<=" else (lambda a, b: a < b)
        who = [b for b in look if lt(max(row0, b * T) - b * T, t_limit[b])]
        out.append((tile, bool(who), utts, who))
    return out


def block_interior(f0w, M, T):
    """`const bool interior = f0w - 3 >= 0 && f0w + 35 < M && (f0w - 3) / fr.T == (f0w + 35) / fr.T;`"""
    return f0w - 3 >= 0 and f0w + 35 < M and (f0w - 3) // T == (f0w + 35) // T


def block_branches(B, T, I, t_limit):
    """The branches one launch takes: per wave `interior` (block_interior); per border row b * T its place in the 4-frame group
    and against the wave (32 frames) and tile (128) edges, which is where `const bool ok = interior || ur[p] == uf[u];` with
    `ur[p] = r < 0 ? -1 : r / fr.T;` decides; `const bool ok = interior || (r >= 0 && r < M);` in load_row; the tail
    `M % 128`; and the outcomes of the `need` loop (block_tiles)."""
    M = B * T
    out = {f"I={I}", f"Mtail={M % CX_BM}" if M % CX_BM in (1, 31, 32, 33, 127) else "Mtail=other"}
    if t_limit is None and T in (1, 2, 3, 4, 6, 7, 8, 124, 125, 127, 128, 129, 131, 132, 256):
        out.add(f"T={T}")                            # (every tile computes: both sides of every border are checked)
    for f0w in range(0, M, 32):
        out.add("interior" if block_interior(f0w, M, T) else "boundary-wave")
    out.add("rows<0-zero-taps")                      # the first wave: `ur[p] = r < 0 ? -1 : r / fr.T;` and load_row's `r >= 0`
    out.add("rows>=M-zero-taps")                     # the last frame's taps 4 .. 6: load_row's `r < M`
    for b in range(1, B):
        r = b * T                                    # the first row of utterance b: a border inside the tensor
        out.add(f"border%4={r % 4}")                 # its place in the 4-frame group (f0w is a multiple of 32)
        for d in (0, 1, -1):
            if (r - d) % 32 == 0:
                out.add(f"border-at-wave-edge{d:+d}" if d else "border-at-wave-edge")
        for d in (0, 1, -1, 3, -3, 4, -4):
            if (r - d) % CX_BM == 0:
                out.add(f"border-at-tile-edge{d:+d}" if d else "border-at-tile-edge")
    if B > 1 and T <= 4:
        out.add("window-spans>=3-utterances")        # 10 rows: `ur[p] == uf[u]` has three or more values in one group
    if t_limit is None:
        out.add("t_limit-absent")
        return out
    if all(v >= T for v in t_limit):
        out.add("t_limit-all>=T")
    if any(v == 0 for v in t_limit):
        out.add("t_limit=0")
    for tile, need, utts, who in block_tiles(B, T, t_limit):
        if not need:
            out.add("tile-skipped")
            if len(utts) == 1 and t_limit[utts[0]] == tile * CX_BM - utts[0] * T:
                out.add("tile-starts-at-its-limit")  # t_lo == t_limit[b]: `<` and `<=` differ
        if len(utts) == 2 and who == utts[:1]:
            out.add("tile-two-utterances-first-needs")
        if len(utts) == 2 and who == utts[1:]:
            out.add("tile-two-utterances-second-needs")
        if len(utts) >= 3:
            out.add("tile-three-utterances")
            if need and utts[0] not in who:
                out.add("tile-three-utterances-a-later-one-needs")
    return out


REQUIRED_BLOCK = ({f"T={T}" for T in (1, 2, 3, 4, 6, 7, 8, 124, 125, 127, 128, 129, 131, 132, 256)}
                  | {f"Mtail={r}" for r in (1, 31, 32, 33, 127)} | {f"border%4={r}" for r in range(4)}
                  | {"interior", "boundary-wave", "rows<0-zero-taps", "rows>=M-zero-taps", "border-at-wave-edge",
                     "border-at-wave-edge+1", "border-at-wave-edge-1", "border-at-tile-edge", "border-at-tile-edge+1",
                     "border-at-tile-edge-1", "border-at-tile-edge+3", "border-at-tile-edge-3", "border-at-tile-edge+4",
                     "border-at-tile-edge-4", "window-spans>=3-utterances", "I=128", "I=256", "t_limit-absent", "t_limit-all>=T",
                     "t_limit=0", "tile-skipped", "tile-starts-at-its-limit", "tile-two-utterances-first-needs",
                     "tile-two-utterances-second-needs", "tile-three-utterances", "tile-three-utterances-a-later-one-needs"})


@functools.lru_cache(maxsize=None)
def block_input(B, T, I):
    """(read-only: cached) the f32 tensors of test_convnext_block_f16_operands (weights unrounded), by name"""
    g = _g("block", B, T, I)
    C = CX_C
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(B, T, C), w7=r(7, C) * 0.3, db=r(C) * 0.1, lw=1 + 0.2 * r(C), lb=0.1 * r(C), w1=r(I, C) * C ** -0.5,
                w2=r(C, I) * I ** -0.5, b1=r(I) * 0.3, b2=r(C) * 0.3, gam=r(C))


def block_weights(t, operands):
    """the float64 pwconv weights the reference uses: rounded to bf16 for the bf16 form (test_convnext_block_fused), unrounded
    for the f16 form (test_convnext_block_f16_operands)"""
    if operands == "bf16":
        return t["w1"].bfloat16().double(), t["w2"].bfloat16().double()
    return t["w1"].double(), t["w2"].double()


def block_back(t, conv, operands):
    """float64 LayerNorm (eps 1e-6, two-pass) + pwconv1 + GELU (erf) + pwconv2 + gamma + residual of conv rows [M, C]; x [M, C]"""
    w1, w2 = block_weights(t, operands)
    x = t["x"].double().reshape(-1, CX_C)
    d = conv - conv.mean(-1, keepdim=True)
    yn = d / (d.pow(2).mean(-1, keepdim=True) + 1e-6).sqrt() * t["lw"].double() + t["lb"].double()
    h = yn @ w1.T + t["b1"].double()
    h = 0.5 * h * (1 + torch.erf(h / math.sqrt(2.0)))
    return x + t["gam"].double() * (h @ w2.T + t["b2"].double())


def block_ref(B, T, I, operands):
    """float64 [M, C]: y[b, t] = bias + sum_j w7[j] x[b, t + j - 3] over 0 <= t + j - 3 < T, then block_back"""
    t = block_input(B, T, I)
    x = t["x"].double()
    conv = t["db"].double().expand(B, T, CX_C).clone()
    for j in range(7):
        lo, hi = max(0, 3 - j), min(T, T + 3 - j)          # frames whose tap j lies inside the utterance
        if lo < hi:
            conv[:, lo:hi] += t["w7"][j].double() * x[:, lo + j - 3:hi + j - 3]
    return block_back(t, conv.reshape(B * T, CX_C), operands)


BLOCK_FAULTS = {
    "taps-cross-border": ("`const bool ok = interior || ur[p] == uf[u];` always true: taps read the neighbouring utterance",
                          "border%4=1"),
    "beyond-M-last-row": ("a tap at a row >= M takes the last row (load_row's `r < M` and the `ur` test both let it through; "
                          "either guard alone still gives zero)", "rows>=M-zero-taps"),
    "need-first-only": ("`need` looks at the tile's first utterance only", "tile-two-utterances-second-needs"),
    "limit<=": ("`need = need || t_lo <= fr.t_limit[b]`", "tile-starts-at-its-limit"),
}


def block_walk(B, T, I, t_limit, operands, fault=None):
    """The fused kernel's front half as it walks: per tile the `need` loop, per wave `interior`, per group of 4 frames the 10-row
    window, `load_row`'s zero rows and the per-(frame, row) utterance test; then block_back.  -> (out [M, C] float64 with NaN in
    the rows of tiles that returned at once, the tiles that computed)"""
    t = block_input(B, T, I)
    M = B * T
    x = t["x"].double().reshape(M, CX_C)
    w7, zero = t["w7"].double(), torch.zeros(CX_C, dtype=torch.float64)
    conv = torch.full((M, CX_C), float("nan"), dtype=torch.float64)
    done = []
    for tile, need, _, _ in block_tiles(B, T, t_limit, fault):
        if not need:
            continue
        done.append(tile)
        for w in range(4):
            f0w = tile * CX_BM + 32 * w
            interior = block_interior(f0w, M, T)
            for g in range(8):
                win, ur = [], []
                for p in range(10):
                    r = f0w + 4 * g - 3 + p
                    if fault == "beyond-M-last-row" and r >= M:
                        r = M - 1
                    win.append(x[r] if interior or 0 <= r < M else zero)       # load_row
                    ur.append(-1 if r < 0 else r // T)
                for u in range(4):
                    row = f0w + 4 * g + u
                    if row >= M:
                        continue                                               # computed on zeros, never stored
                    v = t["db"].double().clone()
                    for j in range(7):
                        p = u + j
                        if interior or ur[p] == ur[u + 3] or fault == "taps-cross-border":
                            v = v + win[p] * w7[j]
                    conv[row] = v
    out = block_back(t, torch.nan_to_num(conv), operands)
    out[torch.isnan(conv[:, 0])] = float("nan")
    return out, done


def block_check_rows(B, T, t_limit):
    """the rows a value check covers: all without t_limit; with it the frames t < t_limit[b] - 3 (include/swc.h: the caller's
    limit covers what it keeps plus the receptive field, 3 frames per block)"""
    tt = torch.arange(T).view(1, T).expand(B, T)
    if t_limit is None:
        return torch.ones(B * T, dtype=torch.bool)
    return (tt < torch.tensor(t_limit).view(B, 1) - 3).reshape(-1)


def block_skipped_rows(B, T, t_limit):
    """the rows of tiles that return at once (they keep what x_out held)"""
    m = torch.zeros(B * T, dtype=torch.bool)
    for tile, need, _, _ in block_tiles(B, T, t_limit):
        if not need:
            m[tile * CX_BM:(tile + 1) * CX_BM] = True
    return m


def block_criteria(out, B, T, I, t_limit, operands):
    """the criteria of the GPU test on an output [M, C] float64 (NaN = the row was left alone) -> list of those that FAIL"""
    ref = block_ref(B, T, I, operands)
    x = block_input(B, T, I)["x"].double().reshape(-1, CX_C)
    scale = float((ref - x).abs().max())
    rows = block_check_rows(B, T, t_limit)
    failed = []
    got = out[rows]
    if not bool(torch.isfinite(got).all()) or float((got - ref[rows]).abs().max() if got.numel() else 0.0) / scale >= CX_TOL[operands]["e_ref"]:
        failed.append("values")
    if not bool(torch.isnan(out[block_skipped_rows(B, T, t_limit)]).all()):
        failed.append("skipped-tiles-left-alone")
    return failed


# ========================================================================================================= layer tail
TAIL_M = (1, 63, 64, 65, 129)      # `rows beyond M are computed on a copy of the last row and never stored`: 64-token tiles
TAIL_D, TAIL_F = 768, 256
# test_layer_tail_fused / test_mlp_block_fused: `assert e_ref < 1e-2`, `assert e_ref < 2.0 * e_two_ref + 1e-4`, `assert e_two < 5e-3`
TAIL_TOL = dict(e_ref=1e-2, e_two=5e-3)


def tail_branches(M):
    """`row = row < M ? row : M - 1;  // rows beyond M are computed on a copy of the last row and never stored` (the form the
    64-token tiles of swc_mlp_block / swc_layer_tail share with swc_convnext_mlp)"""
    out = {f"M={M}", "partial-tile" if M % 64 else "full-tiles", "one-tile" if M <= 64 else "tiles>=2"}
    if M % 64 == 1:
        out.add("tile-of-one-row")
    return out


REQUIRED_TAIL = {f"M={M}" for M in TAIL_M} | {"partial-tile", "full-tiles", "one-tile", "tiles>=2", "tile-of-one-row"}


@functools.lru_cache(maxsize=None)
def tail_input(M):
    """(read-only: cached) the tensors of test_layer_tail_fused at F = 256 (weights and att already rounded to bf16), by name"""
    D, F_ = TAIL_D, TAIL_F
    g = _g("tail", M)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(M, D) * 1.5 + 0.1, att=(r(M, D) * 0.7).bfloat16(), wo=(r(D, D) * D ** -0.5).bfloat16(), bo=r(D) * 0.2,
                lw=1 + 0.2 * r(D), lb=0.1 * r(D), nw=1 + 0.2 * r(D), nb=0.1 * r(D), w1=(r(F_, D) * D ** -0.5).bfloat16(),
                w2=(r(D, F_) * F_ ** -0.5).bfloat16(), b1=r(F_) * 0.3, b2=r(D) * 0.3)


def tail_ref(M, with_attn):
    """float64 of test_layer_tail_fused (with_attn) / test_mlp_block_fused -> (ref, residual-in x')"""
    t = tail_input(M)
    xp = t["x"].double()
    if with_attn:
        xp = xp + t["att"].double() @ t["wo"].double().T + t["bo"].double()
    yr = F.layer_norm(xp, (TAIL_D,), t["lw"].double(), t["lb"].double(), 1e-5)
    h = F.gelu(yr @ t["w1"].double().T + t["b1"].double())
    return xp + h @ t["w2"].double().T + t["b2"].double()


# ======================================================================================================= the case list
@functools.lru_cache(maxsize=None)
def all_cases():
    """(read-only: cached) every case with the branches its predicate assigns it: [(kernel form, case text, sorted branches)]"""
    rows = []
    for form in ATT_FORMS:
        for layout in (("padded", "packed") if form in ATT_PACKED else ("padded",)):
            for c in ATT_CASES:
                lens = c["lens"]
                text = (f"{c['name']}: T={c['T']} H={c['H']} B={len(lens)} lens="
                        + (str(list(lens)) if len(lens) <= 8 else f"[{lens[0]}, {lens[1]}, {lens[2]}, ... {lens[-1]}]"))
                br = attn_branches(form, c["T"], lens, c["H"], packed=layout == "packed")
                if layout == "packed":
                    br &= _ATT_PACKED                  # (the packed launch repeats the padded one's branches: list its own)
                rows.append((f"attention {form} {layout}", text, br))
    for c in BLOCK_CASES:
        rows.append(("convnext_block", f"B={c['B']} T={c['T']} M={c['B'] * c['T']} I={c['I']} t_limit="
                     f"{None if c['t_limit'] is None else list(c['t_limit'])} bf16+f16",
                     block_branches(c["B"], c["T"], c["I"], c["t_limit"])))
    for M in TAIL_M:
        rows.append(("layer_tail", f"M={M} D={TAIL_D} F={TAIL_F} swc_layer_tail+swc_mlp_block", tail_branches(M)))
    return [(k, s, sorted(b)) for k, s, b in rows]


REQUIRED = {"convnext_block": REQUIRED_BLOCK, "layer_tail": REQUIRED_TAIL}
for _form, _f in ATT_FORMS.items():
    REQUIRED[f"attention {_form} padded"] = _ATT_COMMON | ({"tile16-beyond-len"} if _f["sixteen"] else set())
    if _form in ATT_PACKED:
        REQUIRED[f"attention {_form} packed"] = set(_ATT_PACKED)


def uncovered(rows):
    """{kernel form: the REQUIRED branches no row of `rows` takes}"""
    seen = {}
    for kernel, _, branches in rows:
        seen.setdefault(kernel, set()).update(branches)
    return {k: sorted(need - seen.get(k, set())) for k, need in REQUIRED.items() if need - seen.get(k, set())}


def cases_text():
    """profiles/fused_index_cases.txt"""
    lines = ["The cases of tests/fused_index.py: one line per case with its shape and the branches its predicate assigns it",
             "(host arithmetic, no GPU; tests/test_fused_index_cpu.py compares this file with what the table computes).", ""]
    for k, s, b in all_cases():
        lines.append(f"{k:28s} {s}  ->  {' '.join(b)}")
    return "\n".join(lines) + "\n"
