"""The index-math case tables of the stage kernels (csrc/swc_pointwise.hip), shared by tests/test_stage_index_cpu.py and
tests/test_stage_index_gpu.py: the log-mel front end, the samplers' snake activation, the FSQ, the deconvolution's col2im and
the ISTFT head.

Per kernel there is a table of the smallest shapes that reach each branch of its index arithmetic, a float64 (or, for pure
copies, exact) reference of the operation, and a short predicate that restates the kernel's own condition (the source line is
quoted in its docstring) and so names the branches a case takes.  The CPU test holds the tables to the branches (REQUIRED
below: a branch without a case fails it), pins the references against independent statements and compares
profiles/stage_index_cases.txt with cases_text(); the GPU test runs every case.

Host only: nothing here touches a device.
"""
import functools
import itertools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import value_domain as vd

FSQ_LEVELS = (8, 7, 6, 6)


def nblk(n, bs):
    """workgroups of bs threads for n items (csrc: `inline unsigned nblk(long n, int bs)`)"""
    return (n + bs - 1) // bs


def _g(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


# ------------------------------------------------------------------------------------------------------- mel_frames
MF_NPAD = (400, 640, 1000)
MF_WAYS = ("aligned", "ld_odd", "offset1")     # how wav is addressed: see frames_layout
MF_FILL = 7.0                                  # what the samples at and beyond n[b] hold (a missed length check shows)


def frames_lengths(n_pad):
    return [0, 1, 3, 4, 5, 199, 200, 201, n_pad - 3, n_pad - 2, n_pad - 1, n_pad]


def frames_t_product(n_pad):
    """the product's relation (spec.mel_len + centre padding): the last frame reflects at n_pad"""
    return n_pad // 160 + 1


def frames_t_max(n_pad):
    """the largest T swc_mel_frames accepts: `SWC_CHECK_ARG((long)(T - 1) * 160 + 199 < 2L * n_pad - 1, ...)`"""
    return (2 * n_pad - 2 - 199) // 160 + 1


def frames_layout(way, n_pad):
    """(floats in front of row 0 inside the buffer, ld_wav) of an addressing way"""
    return {"aligned": (0, n_pad), "ld_odd": (0, n_pad + 1), "offset1": (1, n_pad)}[way]


def frames_vec_ok(offset, ld_wav):
    """`const int vec_ok = aligned16(wav) && ld_wav % 4 == 0;` with the buffer itself 16-byte aligned"""
    return offset % 4 == 0 and ld_wav % 4 == 0


def frames_branches(n_pad, T, lengths, vec_ok):
    """The branches the quads of one launch take.  The kernel, per quad at s0 = t * 160 + 4 * j - 200:
    `if (vec_ok && s0 >= 0 && s0 + 3 < nb && s0 + 3 < n_pad)` one 16-byte load, else per element
    `if (s < 0) s = -s;  if (s >= n_pad) s = 2 * (n_pad - 1) - s;  e[i] = s < nb ? wb[s] : 0.f;`"""
    out = {"vec_ok=1" if vec_ok else "vec_ok=0"}
    s0 = (np.arange(T)[:, None] * 160 + 4 * np.arange(100)[None, :] - 200).reshape(-1)
    s = s0[:, None] + np.arange(4)[None, :]
    for nb in lengths:
        vec = vec_ok & (s0 >= 0) & (s0 + 3 < nb) & (s0 + 3 < n_pad)
        if vec.any():
            out.add("quad-load")
        se = s[~vec]
        left, right = se < 0, se >= n_pad
        r = np.where(left, -se, np.where(right, 2 * (n_pad - 1) - se, se))
        assert (r >= 0).all() and (r < n_pad).all()
        if (~left & ~right & (r < nb)).any():
            out.add("element-load")
        if (left & (r < nb)).any():
            out.add("left-reflect")
        if (left & (r >= nb)).any() and nb < 200:
            out.add("left-reflect-beyond-length")
        if (right & (r < nb)).any():
            out.add("right-reflect")
        if (right & (r >= nb)).any():
            out.add("right-reflect-beyond-length")
        if (~left & ~right & (r >= nb)).any():
            out.add("beyond-length")
        if nb > 0:
            out.add(f"length-mod4={nb % 4}")     # 1..3: the length ends inside a quad (s0 < nb <= s0 + 3); 0: on a quad boundary
        if nb < 200:
            out.add("length<200")
    return out


def frames_cases():
    return [dict(kernel="mel_frames", n_pad=n_pad, T=T, way=way) for n_pad in MF_NPAD
            for T in (frames_t_product(n_pad), frames_t_max(n_pad)) for way in MF_WAYS]


@functools.lru_cache(maxsize=None)
def frames_input(n_pad):
    """(read-only: cached) the 12 rows (no fill yet) and their lengths"""
    n = frames_lengths(n_pad)
    return torch.randn(len(n), n_pad, generator=_g("frames", n_pad)), n


def frames_ref(wav, n, n_pad, T):
    """zero-extend to n_pad, reflect-pad, unfold(400, 160): torch.stft's centre padding as feature_extractor.py applies it.
    The right pad is the 200 of that statement, or as many samples as frame T - 1 reaches beyond it (the reflection about
    sample n_pad - 1 continued; the argument check keeps it under n_pad - 1, F.pad's own limit)."""
    right = max(200, (T - 1) * 160 + 400 - 200 - n_pad)
    rows = []
    for b in range(wav.shape[0]):
        x = wav[b, :n_pad].clone()
        x[int(n[b]):] = 0
        xp = F.pad(x.view(1, 1, -1), (200, right), mode="reflect").view(-1)
        rows.append(xp.unfold(0, 400, 160)[:T])
    return torch.stack(rows)


# -------------------------------------------------------------------------------------------------------- mel_power
def power_cases():
    return [dict(kernel="mel_power", rows=rows, ld=ld, ldp=ldp) for rows in (1, 3) for ld in (402, 403, 416)
            for ldp in (201, 208)]


def power_branches(rows, ld, ldp):
    """`if (i >= rows * ldp) return;` ... `if (k < 201) {` (else the zero columns up to ldp)"""
    out = {"bin", "one-workgroup" if rows * ldp <= 256 else "workgroups>=2"}
    if ldp > 201:
        out.add("zero-column")
    out.add("rows-16B-aligned" if ld % 4 == 0 else "rows-unaligned")
    return out


U32 = 2.0 ** -24
POWER_REL = (1 + U32) ** 5 - 1   # five float32 roundings, each (1 + d), |d| <= 2^-24, on positive terms: see test_mel_power


def power_ref(dft):
    d = dft.double()
    return d[:, :201] ** 2 + d[:, 201:402] ** 2


# ---------------------------------------------------------------------------------------------- mel_logmax + mel_final
LM_WG = 4096                     # `256 * LM_PER_THREAD` elements per workgroup
LM_SHAPES = ((52, 80, 96), (103, 80, 96), (1400, 3, 7))


def logmax_owner(p):
    """(workgroup, loop slot k, thread) of flat element p of an utterance:
    `const long base = (long)blockIdx.x * (256 * LM_PER_THREAD) + threadIdx.x;` and `const long i = base + 256L * k;`"""
    return p // LM_WG, (p % LM_WG) // 256, p % 256


def L(name, T, n_mel, ld, peaks, umax0, negative=False):
    total = T * n_mel
    peaks = tuple(total - 1 if p == "last" else p for p in peaks)
    assert len(set(peaks)) == len(peaks) == 3 and max(peaks) < total
    return dict(kernel="mel_logmax", name=name, T=T, n_mel=n_mel, ld=ld, peaks=peaks, umax0=umax0, negative=negative)


def logmax_cases():
    out = []
    peaks = {LM_SHAPES[0]: (0, 256 * 15 + 7, 4096), LM_SHAPES[1]: (255, 4096, "last"), LM_SHAPES[2]: (256, 4095, "last")}
    for shape in LM_SHAPES:
        for u0 in (-10.0, float("-inf")):
            out.append(L("x".join(map(str, shape)), *shape, peaks[shape], u0))
    out.append(L("52x80x96-negative", 52, 80, 96, ("last", 0, 4096), float("-inf"), negative=True))
    return out


LM_PEAKS = (0, 255, 256, 256 * 15 + 7, 4095, 4096, "last")


def logmax_branches(case):
    """one `atomicMax(umax_ord + b, f32_ordered(v))` per workgroup; `return i >= 0 ? i : i ^ 0x7fffffff;` in f32_ordered"""
    total = case["T"] * case["n_mel"]
    out = {f"workgroups={nblk(total, LM_WG)}", "start=-inf" if case["umax0"] == float("-inf") else "start=-10"}
    for p in case["peaks"]:
        wg, k, tid = logmax_owner(p)
        out.add(f"peak-in-workgroup-{wg}")
        out.add(f"peak-in-slot-{k}")
        if p == total - 1:
            out.add("peak-at-last-element")
    if total % LM_WG and (total % LM_WG) % 256:
        out.add("last-slot-partly-filled")
    if case["ld"] > case["n_mel"]:
        out.add("padding-columns")
    if case["n_mel"] < 16:
        out.add("many-rows-per-thread-stride")
    out.add("negative-maximum" if case["negative"] else "positive-maximum")
    return out


@functools.lru_cache(maxsize=None)
def logmax_input(name, T, n_mel, ld, peaks, negative):
    """(read-only: cached) mel powers [3, T, ld] f32: every log below the planted peak of its utterance, one strictly larger
    value at flat index peaks[b]; the padding columns hold -3 (neither read nor written by the kernels)"""
    g = _g("logmax", name)
    if negative:
        mel = 10.0 ** (torch.rand(3, T, ld, generator=g) * 9.0 - 9.5)       # (1e-10, 1): logs in (-9.5, -0.5)
        peak = [0.9, 0.8, 0.7]
    else:
        mel = torch.rand(3, T, ld, generator=g) * 0.999 + 1e-3              # logs in (-3, 0)
        peak = [50.0, 60.0, 70.0]
    mel = mel.float()
    for b, p in enumerate(peaks):
        mel[b, p // n_mel, p % n_mel] = peak[b]
    mel[:, :, n_mel:] = -3.0
    return mel


def final_ldo(n_mel):
    return (n_mel, 96, 97)


# ------------------------------------------------------------------------------------------------------------ snake
SN_TS = 8                               # `snake_aa_kernel<.., 8>`: outputs per thread strip
SNAKE_T = tuple(range(1, 36))
SNAKE_CASES = [dict(kernel="snake_aa", C=C_, out=out) for C_, out in
               ((32, "f32"), (260, "f32"), (32, "bf16"), (260, "bf16"), (32, "f16s"), (288, "f16s"))]


def snake_strip_path(T, strip):
    """`if (t0 >= 3 && t0 + SN_TS + 2 <= T - 1) {  // block-uniform` with `t0 = blockIdx.y * SN_TS`: "fast" (the strip's 20
    inputs at once) or "generic" (pair by pair, clamped)"""
    t0 = strip * SN_TS
    assert t0 < T
    return "fast" if t0 >= 3 and t0 + SN_TS + 2 <= T - 1 else "generic"


def snake_branches(T, C_):
    out = {f"channel-blocks={nblk(C_, 256)}"}
    if C_ % 256:
        out.add("channel-tail")
    for strip in range(nblk(T, SN_TS)):
        path = snake_strip_path(T, strip)
        out.add(f"strip{min(strip, 4)}-{path}")
        if strip * SN_TS + SN_TS > T:
            out.add("partial-last-strip")
    return out


@functools.lru_cache(maxsize=None)
def snake_input(C_, T):
    """(read-only: cached) x (B=2, C, T), alpha, beta (already exponentiated) and the float64 reference [B, T, C]"""
    g = _g("snake", C_, T)
    x = torch.randn(2, C_, T, generator=g) * 2
    al, be = (torch.randn(C_, generator=g) * 0.3).exp(), (torch.randn(C_, generator=g) * 0.3).exp()
    ref = vd.snake_ref(x, al, be, vd.kaiser_sinc12()).transpose(1, 2).contiguous()
    return x, al, be, ref


# ----------------------------------------------------------------------------------------------------------- col2im
CI_SHAPES = ((24, 32), (24, 33), (23, 23), (6, 8), (260, 260))
CI_S = (1, 2, 3, 4)
CI_T = (1, 2, 17)
CI_BITEQ = ((24, 32), (24, 24), (260, 260))   # vector-kernel launches whose first C columns must equal the scalar kernel's at ldo + 1


def col2im_t_outs(T, s):
    """1, 2, the product's crop (decode: `t_out=Tv + 1` at s = 2; the reference's trim of 3 otherwise) and the full length"""
    full = (T - 1) * s + 3
    crop = full - (1 if s == 2 else 3)
    return sorted({t for t in (1, 2, crop, full) if 0 < t <= full})


def col2im_kernel(C_, ldo, aligned=True):
    """`if (C % 4 == 0 && ldo % 4 == 0 && aligned16(y3) && aligned16(bias) && aligned16(out)) {` -> deconv_col2im4_kernel,
    else deconv_col2im_kernel (the scalar one)"""
    return "vec4" if C_ % 4 == 0 and ldo % 4 == 0 and aligned else "scalar"


def col2im_branches(C_, ldo, s, T, t_out):
    """per output frame `to` and tap j: `const int d = to - j;  if (d >= 0 && d % s == 0) { const int ti = d / s;
    if (ti < T) v += ...`"""
    out = {col2im_kernel(C_, ldo)}
    if ldo > C_:
        out.add("zero-column")
    for to, j in itertools.product(range(t_out), range(3)):
        d = to - j
        if d < 0:
            out.add("d<0")
        elif d % s:
            out.add("d%s!=0")
        elif d // s >= T:
            out.add("ti>=T")
        else:
            out.add("tap")
    n = sum((to - j) >= 0 and (to - j) % s == 0 and (to - j) // s < T for to in range(t_out) for j in range(3))
    if any(sum((to - j) >= 0 and (to - j) % s == 0 and (to - j) // s < T for j in range(3)) == 0 for to in range(t_out)):
        out.add("frame-without-tap")
    assert n > 0
    per = t_out * (ldo // 4 if col2im_kernel(C_, ldo) == "vec4" else ldo)
    out.add("one-workgroup" if per <= 256 else "workgroups>=2")
    return out


def col2im_cases():
    return [dict(kernel="deconv_col2im", C=C_, ldo=ldo, s=s, T=T, t_out=t_out) for (C_, ldo) in CI_SHAPES for s in CI_S
            for T in CI_T for t_out in col2im_t_outs(T, s)]


@functools.lru_cache(maxsize=None)
def col2im_input(C_, T):
    """(read-only: cached) y3 [B=2, T, 3, C] f32 (random: no GEMM in front) and bias [C]"""
    g = _g("col2im", C_, T)
    return torch.randn(2, T, 3, C_, generator=g), torch.randn(C_, generator=g)


def col2im_ref(y3, bias, s, t_out):
    """float64 ConvTranspose1d(k = 3, stride s) tail: out[b, ti * s + j, c] += y3[b, ti, j, c], plus the bias; first t_out frames"""
    B, T, _, C_ = y3.shape
    out = bias.double().expand(B, (T - 1) * s + 3, C_).clone()
    for ti in range(T):
        for j in range(3):
            out[:, ti * s + j] += y3[:, ti, j].double()
    return out[:, :t_out]


# -------------------------------------------------------------------------------------------------------- istft_ola
OLA_T = tuple(range(1, 10))


def ola_window(T, n):
    """(tlo, thi, clamps) of the quad at output sample n: `const long p = n + 240;  long tlo = (p - 639 + 159) / 160;
    if (p - 639 < 0) tlo = 0;  long thi = p / 160;  if (thi > T - 1) thi = T - 1;`"""
    p = n + 240
    clamps = set()
    tlo = (p - 639 + 159) // 160
    if p - 639 < 0:
        tlo = 0
        clamps.add("tlo-clamp")
    thi = p // 160
    if thi > T - 1:
        thi = T - 1
        clamps.add("thi-clamp")
    return tlo, thi, clamps


def ola_branches(T):
    out = set()
    for n in range(0, T * 160, 4):
        tlo, thi, clamps = ola_window(T, n)
        assert 0 <= tlo <= thi < T
        out |= clamps
        out.add(f"overlap={thi - tlo + 1}")
        if clamps == {"tlo-clamp", "thi-clamp"}:
            out.add("both-clamps")
    return out


@functools.lru_cache(maxsize=None)
def ola_input(T):
    """(read-only: cached) frames [B=2, T, 640] f32 (already windowed inverse-DFT rows)"""
    return torch.randn(2, T, 640, generator=_g("ola", T))


def ola_ref(frames):
    """the fold-based statement of test_istft (modules.py:861-884) in float64 on the float32 window the kernel is handed"""
    B, T, _ = frames.shape
    wsq = (torch.hann_window(640, dtype=torch.float64) ** 2).float().double()
    size = (T - 1) * 160 + 640
    fold = lambda v: F.fold(v.transpose(1, 2), output_size=(1, size), kernel_size=(1, 640), stride=(1, 160))[:, 0, 0, 240:-240]
    return fold(frames.double()) / fold(wsq.expand(1, T, -1))


# ------------------------------------------------------------------------------------------------------- istft_spec
SPEC_ROWS = 3
SPEC_OUT = (("f32", 642), ("f32", 648), ("f32", 672), ("bf16", 648), ("bf16", 672), ("f16s", 672), ("f16s", 704))
SPEC_LDH = (642, 648, 656, 668)            # the lists of test_memory_contract_gpu.test_istft_spec


def spec_cases():
    return [dict(kernel="istft_spec", ldh=ldh, out=o, lds=lds) for ldh in SPEC_LDH for o, lds in SPEC_OUT]


def spec_branches(ldh, lds, rows=SPEC_ROWS):
    """`const int per = 321 + (int)(lds - 642);` threads per row; `if (k >= 321) {` writes the zero column 642 + (k - 321)"""
    per = 321 + (lds - 642)
    out = {"bin", "product-ldh=648" if ldh == 648 else f"ldh={ldh}"}
    if lds > 642:
        out.add("zero-column")
    if any((r * per) % 256 for r in range(1, rows)) and rows * per > 256:
        out.add("workgroup-boundary-inside-a-row")
    return out


@functools.lru_cache(maxsize=None)
def spec_input():
    """(read-only: cached) h [SPEC_ROWS, 642] f32: log-magnitudes (one above the clip at ln 100) and phases"""
    h = torch.randn(SPEC_ROWS, 642, generator=_g("spec"))
    h[0, 3] = 9.0
    return h


# -------------------------------------------------------------------------------------------------------------- FSQ
FSQ_T, FSQ_LENS = 17, (17, 13, 0)


def fsq_encode_cases():
    return [dict(kernel="fsq_encode", G=G_, ldz=4 * G_ + dz, t_pad=FSQ_T + dt) for G_ in (1, 3, 8) for dz in (0, 4)
            for dt in (0, 14)]


def fsq_decode_cases():
    return [dict(kernel="fsq_decode", G=G_, ldq=4 * G_ + dq) for G_ in (1, 3, 8) for dq in (0, 8)]


def fsq_encode_branches(G_, ldz, t_pad):
    """`const bool valid = t < T && t < lens[b];` over `total = (long)B * t_pad * G` threads"""
    out = {"valid", "t>=lens[b]", f"G={G_}"}
    if t_pad > FSQ_T:
        out.add("t>=T")
    if ldz > 4 * G_:
        out.add("ldz>4G")
    out.add("one-workgroup" if 3 * t_pad * G_ <= 256 else "workgroups>=2")
    return out


def fsq_decode_branches(G_, ldq):
    """`const int ng = (int)(ldq / 4);  // groups incl. zero padding columns` and `if (g < G && t < lens[b]) {`"""
    out = {"valid", "t>=lens[b]", f"G={G_}"}
    if ldq > 4 * G_:
        out.add("g>=G")
    out.add("one-workgroup" if 3 * FSQ_T * (ldq // 4) <= 256 else "workgroups>=2")
    return out


@functools.lru_cache(maxsize=None)
def fsq_input(G_):
    """(read-only: cached) z [3, T, G, 4] f32, the constants, and vd.fsq_ref of it masked by the lengths:
    (z, k12, zq [3, T, G, 4] f32, codes [G, 3, T] int32)"""
    from simwhisper_codec_amd import spec
    k12 = spec.fsq_constants(list(FSQ_LEVELS), 1e-3)
    z = torch.randn(3, FSQ_T, G_, 4, generator=_g("fsq", G_)) * 1.5
    zq, idx = vd.fsq_ref(z, k12, FSQ_LEVELS)
    mask = torch.arange(FSQ_T)[None, :] < torch.tensor(FSQ_LENS)[:, None]
    zq = torch.where(mask[:, :, None, None], zq, torch.zeros(()))
    idx = torch.where(mask[:, :, None], idx, torch.zeros((), dtype=torch.int32))
    return z, k12, zq, idx.permute(2, 0, 1).contiguous()


# ------------------------------------------------------------------------------------------------------ the case list
def all_cases():
    """every case with the branches its predicate assigns it: [(kernel, shape text, sorted branches)]"""
    rows = []
    for c in frames_cases():
        off, ld = frames_layout(c["way"], c["n_pad"])
        br = frames_branches(c["n_pad"], c["T"], frames_lengths(c["n_pad"]), frames_vec_ok(off, ld))
        if c["T"] > frames_t_product(c["n_pad"]):
            br.add("largest-T")
        rows.append(("mel_frames", f"n_pad={c['n_pad']} T={c['T']} B=12 wav={c['way']} ld_wav={ld}", br))
    for c in power_cases():
        rows.append(("mel_power", f"rows={c['rows']} ld={c['ld']} ldp={c['ldp']}", power_branches(c["rows"], c["ld"], c["ldp"])))
    for c in logmax_cases():
        rows.append(("mel_logmax", f"B=3 T={c['T']} n_mel={c['n_mel']} ld={c['ld']} peaks={list(c['peaks'])} umax0={c['umax0']}"
                     f" mel_final ldo={list(final_ldo(c['n_mel']))} f32+bf16", logmax_branches(c)))
    for c in SNAKE_CASES:
        for T in SNAKE_T:
            rows.append(("snake_aa", f"B=2 T={T} C={c['C']} out={c['out']}", snake_branches(T, c["C"])))
    for c in col2im_cases():
        rows.append(("deconv_col2im", f"B=2 T={c['T']} C={c['C']} ldo={c['ldo']} s={c['s']} t_out={c['t_out']} f32+bf16",
                     col2im_branches(c["C"], c["ldo"], c["s"], c["T"], c["t_out"])))
    for T in OLA_T:
        rows.append(("istft_ola", f"B=2 T={T}", ola_branches(T)))
    for c in spec_cases():
        rows.append(("istft_spec", f"rows={SPEC_ROWS} ldh={c['ldh']} out={c['out']} lds={c['lds']}", spec_branches(c["ldh"], c["lds"])))
    for c in fsq_encode_cases():
        rows.append(("fsq_encode", f"B=3 T={FSQ_T} lens={list(FSQ_LENS)} G={c['G']} ldz={c['ldz']} t_pad={c['t_pad']}",
                     fsq_encode_branches(c["G"], c["ldz"], c["t_pad"])))
    for c in fsq_decode_cases():
        rows.append(("fsq_decode", f"B=3 T={FSQ_T} lens={list(FSQ_LENS)} G={c['G']} ldq={c['ldq']}",
                     fsq_decode_branches(c["G"], c["ldq"])))
    return [(k, s, sorted(b)) for k, s, b in rows]


# the branches no value test reached before (what "every index branch" means here): each needs at least one case
REQUIRED = {
    "mel_logmax": {"workgroups=2", "workgroups=3", "peak-in-workgroup-1", "peak-in-workgroup-2", "peak-in-slot-15",
                   "peak-in-slot-0", "peak-in-slot-1", "peak-at-last-element", "negative-maximum", "start=-inf", "start=-10",
                   "many-rows-per-thread-stride", "last-slot-partly-filled"},
    "mel_frames": {"right-reflect", "right-reflect-beyond-length", "vec_ok=0", "vec_ok=1", "quad-load", "length<200",
                   "left-reflect-beyond-length", "largest-T"} | {f"length-mod4={r}" for r in range(4)},
    "mel_power": {"rows-unaligned", "rows-16B-aligned", "one-workgroup", "workgroups>=2", "zero-column"},
    "snake_aa": {f"strip{k}-{p}" for k in (1, 2, 3) for p in ("fast", "generic")} | {"partial-last-strip", "channel-tail",
                                                                                      "channel-blocks=2"},
    "deconv_col2im": {"scalar", "vec4", "d%s!=0", "ti>=T", "d<0", "tap", "zero-column", "frame-without-tap"},
    "istft_ola": {"overlap=1", "overlap=2", "overlap=3", "overlap=4", "tlo-clamp", "thi-clamp", "both-clamps"},
    "istft_spec": {"product-ldh=648", "zero-column", "workgroup-boundary-inside-a-row"},
    "fsq_encode": {"G=1", "G=3", "G=8", "ldz>4G", "t>=T", "t>=lens[b]"},
    "fsq_decode": {"G=1", "G=3", "G=8", "g>=G", "t>=lens[b]"},
}


def cases_text():
    """profiles/stage_index_cases.txt"""
    lines = ["The cases of tests/stage_index.py: one line per case with its shape and the branches its predicate assigns it",
             "(host arithmetic, no GPU; tests/test_stage_index_cpu.py compares this file with what the table computes).", ""]
    for k, s, b in all_cases():
        lines.append(f"{k:14s} {s}  ->  {' '.join(b)}")
    return "\n".join(lines) + "\n"
