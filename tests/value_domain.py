"""Value-domain sweeps: input generators, float64 references and float32 emulations of the in-kernel approximations.

Shared by test_value_domain_cpu.py (which pins the generators, the emulated error bounds and the agreement of the references
with those of test_kernels_gpu.py) and test_value_domain_gpu.py (which runs the kernels on them).  Host-only: nothing here
touches a device."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

# ----------------------------------------------------------------------------------------------------- 16-bit grids
GELU_EXTREMES = (30.0, 100.0, 1e4, 1e20)


@functools.lru_cache(maxsize=None)
def bf16_grid(limit=16.0):
    """(read-only: cached) every bf16 value with |v| <= limit, both signs, +0 and -0 (as float32)"""
    bits = torch.arange(0, 0x7F80, dtype=torch.int32)                       # non-negative finite bf16 patterns
    pos = (bits << 16).view(torch.float32)
    pos = pos[pos <= limit]
    return torch.cat([pos, -pos])


@functools.lru_cache(maxsize=None)
def f16_grid(limit=16.0):
    """(read-only: cached) every IEEE half value with |v| <= limit, both signs, +0 and -0 (as float32)"""
    bits = torch.arange(0, 0x7C00, dtype=torch.int32).to(torch.int16)
    pos = bits.view(torch.float16).float()
    pos = pos[pos <= limit]
    return torch.cat([pos, -pos])


def gelu_sweep(fmt="bf16"):
    """the GELU pre-activations of the sweep: the complete 16-bit grid on |v| <= 16 and the far points of both signs
    (values the format cannot hold are left out: 1e20 has no half-precision form)"""
    grid = bf16_grid() if fmt == "bf16" else f16_grid()
    ext = [e for e in GELU_EXTREMES if fmt == "bf16" or e < 65504.0]
    far = torch.tensor([s * e for e in ext for s in (1.0, -1.0)])
    far = far.to(torch.bfloat16 if fmt == "bf16" else torch.float16).float()
    return torch.cat([grid, far])


def pad_to(v, n, fill=0.0):
    """v padded with `fill` to a multiple of n"""
    r = (-v.numel()) % n
    return torch.cat([v, torch.full((r,), fill, dtype=v.dtype)]) if r else v


def subsample(v, n):
    """n points of the 1-D sweep v: an even stride through it, its last 16 points (the far values) and the neighbourhood of
    the refit's worst point v ~ -2.92 always included"""
    v = v.flatten()
    keep = torch.zeros(v.numel(), dtype=torch.bool)
    keep[-16:] = True
    keep |= (v + 2.92).abs() < 0.05
    keep |= v == 0
    rest = n - int(keep.sum())
    idx = torch.nonzero(~keep).flatten()
    keep[idx[torch.linspace(0, idx.numel() - 1, rest).round().long()]] = True
    out = v[keep]
    return pad_to(out, n)[:n]


def gelu_ref(v):
    """exact GELU in float64: v Phi(v) with Phi through erfc (no cancellation in the negative tail)"""
    v = v.double()
    return 0.5 * v * torch.special.erfc(-v * math.sqrt(0.5))


def ulp16(x, fmt):
    """spacing of the 16-bit format at |x| (float64 tensor): bf16 (8 significand bits) or IEEE half (11 bits)"""
    x = x.double().abs()
    p, emin = (7, -126) if fmt == "bf16" else (10, -14)
    e = torch.floor(torch.log2(x.clamp(min=2.0 ** emin))).clamp(min=emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - p)


def round16(x, fmt):
    """float64 -> nearest value of the 16-bit format (saturating for half, as the kernels' packs do) -> float64"""
    if fmt == "bf16":
        return x.float().to(torch.bfloat16).double()
    return x.clamp(-65504.0, 65504.0).float().to(torch.float16).double()


# ------------------------------------------------------------------------------------------- float32 emulations
def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _fma(a, b, c):
    """fmaf of float32 arrays: the exact product and sum in float64 (53 bits hold a 24 x 24 bit product), rounded once"""
    return _f32(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))


def emu_gelu_fast(x):
    """gelu_fast of swc_common.h in float32 steps (exp2 and the reciprocal correctly rounded: the hardware's are within 1 ulp)"""
    x = _f32(x)
    c0, lg = np.float32(0.80015708), np.float32(2.885390081777927)
    k0 = np.float32(c0 * lg)
    k1 = np.float32(np.float32(c0 * np.float32(0.0433676)) * lg)
    with np.errstate(over="ignore"):
        t = _f32(x * _fma(np.full_like(x, k1), _f32(x * x), np.full_like(x, k0)))
        e = _f32(np.exp2(t.astype(np.float64)))
        r = _f32(1.0 / (np.float32(1.0) + e).astype(np.float64))
    return _fma(-x, r, x)


def emu_gelu_as(x):
    """gelu_as of swc_common.h (Abramowitz-Stegun 7.1.26 erf) in float32 steps"""
    x = _f32(x)
    one = np.ones_like(x)
    z = _f32(np.abs(x) * np.float32(0.70710678118654752440))
    d = _fma(np.full_like(x, np.float32(0.3275911)), z, one)
    t = _f32(1.0 / d.astype(np.float64))
    t = _fma(t, _fma(-d, t, one), t)
    poly = _fma(np.full_like(x, np.float32(1.061405429)), t, np.full_like(x, np.float32(-1.453152027)))
    for c in (1.421413741, -0.284496736, 0.254829592):
        poly = _fma(poly, t, np.full_like(x, np.float32(c)))
    e = _f32(np.exp2(_f32(_f32(x * x) * np.float32(-0.72134752044448170368)).astype(np.float64)))
    erf_abs = _fma(-_f32(poly * t), e, one)
    return _f32(_f32(np.float32(0.5) * x) * (one + np.copysign(erf_abs, x)))


def emu_sin2(a):
    """sin2_f32 of swc_pointwise.hip in float32 steps, for |a| <= 8192 (the Cody-Waite branch)"""
    a = _f32(a)
    q = np.rint(_f32(a * np.float32(0.63661977236758134308))).astype(np.float32)
    r = _fma(-q, np.full_like(a, np.float32(1.5703125)), a)
    r = _fma(-q, np.full_like(a, np.float32(4.837512969970703125e-4)), r)
    r = _fma(-q, np.full_like(a, np.float32(7.54978995489188216e-8)), r)
    u = _f32(r * r)
    p = _fma(u, np.full_like(a, np.float32(-4.2755787e-6)), np.full_like(a, np.float32(1.4109347e-4)))
    for c in (-3.1746032e-3, 4.4444444e-2, -3.3333334e-1, 1.0):
        p = _fma(p, u, np.full_like(a, np.float32(c)))
    s2 = _f32(u * p)
    return np.where(q.astype(np.int64) & 1, np.float32(1.0) - s2, s2).astype(np.float32)


# --------------------------------------------------------------------------------------------------- snake / sin^2
SIN2_LIMIT = 8192.0   # sin2_f32: Cody-Waite reduction up to here, libm beyond


def kaiser_sinc12():
    """alias_free_torch/filter.py:25-54 with cutoff 0.25, half_width 0.3, kernel 12 (restated)"""
    ks, cutoff, hw = 12, 0.25, 0.3
    half = ks // 2
    A = 2.285 * (half - 1) * math.pi * 4 * hw + 7.95
    beta = 0.1102 * (A - 8.7) if A > 50 else (0.5842 * (A - 21) ** 0.4 + 0.07886 * (A - 21.0) if A >= 21 else 0.0)
    win = torch.kaiser_window(ks, beta=beta, periodic=False)
    t = torch.arange(-half, half) + 0.5
    f = 2 * cutoff * win * torch.sinc(2 * cutoff * t)
    return f / f.sum()


def snake_ref(x, alpha, beta, f):
    """x (B, C, T); plain float64 statement of Activation1d(SnakeBeta) with alpha, beta given directly (already exponentiated)"""
    x = x.double()
    C = x.shape[1]
    f = f.double()
    xp = F.pad(x, (5, 5), mode="replicate")
    up = 2 * F.conv_transpose1d(xp, f.view(1, 1, -1).expand(C, -1, -1), stride=2, groups=C)[..., 15:-15]
    a, b = alpha.double().view(1, -1, 1), beta.double().view(1, -1, 1)
    act = up + (1.0 / (b + 1e-9)) * torch.sin(up * a) ** 2
    ap = F.pad(act, (5, 6), mode="replicate")
    return F.conv1d(ap, f.view(1, 1, -1).expand(C, -1, -1), stride=2, groups=C)


def snake_up(x, f):
    """the up-sampled signal of snake_ref alone (float64): the sine's argument is alpha * this"""
    x = x.double()
    C = x.shape[1]
    xp = F.pad(x, (5, 5), mode="replicate")
    return 2 * F.conv_transpose1d(xp, f.double().view(1, 1, -1).expand(C, -1, -1), stride=2, groups=C)[..., 15:-15]


def _ulp_steps(v, ks):
    """the float32 numbers k steps above (k > 0) / below (k < 0) v"""
    out = []
    for k in ks:
        x = np.float32(v)
        for _ in range(abs(k)):
            x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
        out.append(float(x))
    return out


def snake_arguments():
    """the sine arguments a of the sweep (float32 tensor, both signs): a dense band on [-40, 40], pairs straddling odd
    multiples of pi/4 (where the reduction's quadrant q changes) at q ~ 10, 1000 and 5000 with q of both parities, the
    switch to libm at 8192 from both sides, and 1e4, 1e5, 1e6 beyond it"""
    pts = list(np.linspace(0.0, 40.0, 321)[1:])                       # step 0.125
    for q in (10, 11, 1000, 1001, 5000, 5001):
        edge = (2 * q + 1) * math.pi / 4                                 # between quadrant q and q + 1
        pts += [edge * (1 - 3e-7), edge * (1 + 3e-7), q * math.pi / 2, q * math.pi / 2 + 0.4]
    pts += [8191.0, 8193.0, 8192.0] + _ulp_steps(8192.0, (-4, -3, -2, -1, 1, 2, 3, 4))
    pts += [1e4, 1e5, 1e6]
    a = torch.tensor(pts, dtype=torch.float64).float()
    return torch.cat([a, -a, torch.zeros(1)])


def snake_case(a, f):
    """inputs that make the kernel's sine argument hit `a` (to an f32 rounding or two): x = 1 on every frame, so the
    up-sampled signal is the constant 2 sum(f[odd]) ~ 1, and alpha = a / that; beta cycles through 0.5, 1, 2.
    -> x [1, T=16, C] f32 (frame-major), alpha [C], beta [C]"""
    C = a.numel()
    x = torch.ones(1, 16, C)
    up = float(snake_up(torch.ones(1, 1, 16), f)[0, 0, 8])
    alpha = (a.double() / up).float()
    beta = torch.tensor([0.5, 1.0, 2.0]).repeat((C + 2) // 3)[:C]
    return x, alpha, beta


# ------------------------------------------------------------------------------------------------------ ISTFT head
def istft_rows():
    """h [8, 656]: 321 log-magnitudes and 321 phases per row (the layout of swc_istft_spec), every log-magnitude of the
    sweep against every phase"""
    ln100 = math.log(100.0)
    logmag = [-100.0, -20.0, 0.0, ln100 - 1e-3, ln100, ln100 + 1e-3, 10.0, 88.0, 89.0, 1e4]
    ph = [0.0]
    for v in (math.pi / 2, math.pi, 100.0, 1e3, 1e5, 1e7):
        ph += [v, -v]
    pairs = [(m, p) for m in logmag for p in ph]
    g = torch.Generator().manual_seed(21)
    h = torch.randn(8, 656, generator=g)
    h[:, 642:] = 0
    for i, (m, p) in enumerate(pairs):
        r, k = i % 8, 7 + 19 * (i // 8)
        h[r, k], h[r, 321 + k] = m, p
    return h, logmag, ph


def istft_ref(h):
    """float64 statement of the ISTFT head on the float32 inputs: (mag cos, mag sin, mag), mag = min(exp, 100)"""
    mag = torch.exp(h[:, :321].double()).clamp(max=100.0)
    ph = h[:, 321:642].double()
    return mag * torch.cos(ph), mag * torch.sin(ph), mag


# ------------------------------------------------------------------------------------------------------- LayerNorm
LN_FAMILIES = ("offset", "constant", "outlier", "tiny", "huge", "alternating")


def ln_rows(family, rows, C, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + C + 17 * LN_FAMILIES.index(family))
    r = torch.randn(rows, C, generator=g)
    if family == "offset":
        return 1000.0 + 0.1 * r
    if family == "constant":
        return torch.tensor([0.0, 1.0, -3.5, 1000.0, 1e-20, 1e15, -1e4, 0.1]).repeat((rows + 7) // 8)[:rows, None].expand(rows, C).contiguous()
    if family == "outlier":
        col = torch.randint(0, C, (rows,), generator=g)
        r[torch.arange(rows), col] = torch.where(torch.arange(rows) % 2 == 0, 1e4, -1e4)
        return r
    if family == "tiny":
        return 1e-20 * r
    if family == "huge":
        return 1e15 * r
    if family == "alternating":
        return torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).expand(rows, C).contiguous()
    raise ValueError(family)


def ln_affine(C, seed=0):
    g = torch.Generator().manual_seed(77 + C + seed)
    return 1 + 0.3 * torch.randn(C, generator=g), torch.randn(C, generator=g)


def ln_ref(x, w, b, eps):
    return F.layer_norm(x.double(), (x.shape[-1],), w.double(), b.double(), eps)


def ln_torch_f32_err(x, w, b, eps):
    """largest error of float32 F.layer_norm on the host against float64, on the same rows: the yardstick of the LayerNorm
    tests (float32 loses precision on offset rows itself, so no absolute figure is fixed)"""
    return float((F.layer_norm(x, (x.shape[-1],), w, b, eps).double() - ln_ref(x, w, b, eps)).abs().max())


# ------------------------------------------------------------------------------------------------------- attention
ATT_B, ATT_H, ATT_T, ATT_LENS = 2, 2, 330, (330, 129)
ATT_CASES = ("equal_keys", "all_minus_5000", "all_plus_5000", "creeping_max", "one_key_minus_1e4")
ATT_RESCALE_THRESHOLD = 8.0 * math.log(2.0)   # bf16 kernel: the reference maximum moves when a tile's grows by more than 8 / c_exp


def _q32(t):
    """round to multiples of 1/32 inside [-2, 2]: exact in bf16, in half precision at scale 64, and such that every product
    with another such number or with +-70 is a multiple of 2^-10: dot products near 5000 are exact in float32 in any order"""
    return (t.clamp(-2, 2) * 32).round() / 32


def attention_case(name):
    """qkv [B, T, 3 * H * 64] float32 whose values are exact in bf16 and in split-f16 (|.| <= 1023)"""
    B, H, T = ATT_B, ATT_H, ATT_T
    g = torch.Generator().manual_seed(ATT_CASES.index(name) + 5)
    q = _q32(0.3 * torch.randn(B, T, H, 64, generator=g))
    k = _q32(0.3 * torch.randn(B, T, H, 64, generator=g))
    v = _q32(torch.randn(B, T, H, 64, generator=g))
    if name == "equal_keys":                    # every key is the same row: uniform softmax whatever the query
        k = k[:, :1].expand(B, T, H, 64).clone()
    elif name == "all_minus_5000":              # q and k anti-aligned along dim 0: 70 * -70 = -4900, the rest O(1)
        q[..., 0], k[..., 0] = 70.0, -70.0
    elif name == "all_plus_5000":
        q[..., 0], k[..., 0] = 70.0, 70.0
    elif name == "creeping_max":                # the maximum grows by 4 score units per 128-key tile: under the threshold
        q[..., 0] = 2.0                         # (5.545) tile by tile, over it after two tiles
        q[..., 1:] = _q32(0.05 * torch.randn(B, T, H, 63, generator=g))
        k[..., 0] = (2.0 * (torch.arange(T) // 128)).view(1, T, 1)
    elif name == "one_key_minus_1e4":
        q[..., 0] = 100.0
        k[..., 0] = 0.0
        k[:, 77, :, 0] = -100.0
    else:
        raise ValueError(name)
    return torch.cat([t.reshape(B, T, H * 64) for t in (q, k, v)], dim=-1)


def attention_ref(qkv, lens, H):
    """float64 softmax(q k^T) v (no score scale: the projections carry it) for the valid rows of every utterance"""
    B, T, _ = qkv.shape
    q, k, v = [t.reshape(B, T, H, 64).transpose(1, 2).double() for t in qkv.float().chunk(3, dim=-1)]
    out = []
    for b, L in enumerate(lens):
        s = q[b, :, :L] @ k[b, :, :L].transpose(-1, -2)
        out.append((torch.softmax(s, -1) @ v[b, :, :L]).transpose(0, 1).reshape(L, H * 64))
    return out


# ------------------------------------------------------------------------------------------------------- mel / FSQ
def mel_values():
    f = np.float32
    lo, hi = np.nextafter(f(1e-10), f(0)), np.nextafter(f(1e-10), f(1))
    return torch.tensor(np.array([0.0, 1.401298464324817e-45, 1e-38, 1e-11, lo, 1e-10, hi, 1.0, 1e10, 3e38], dtype=np.float32))


def mel_ref(mel, umax0):
    """float64 log10(max(x, 1e-10)) of float32 inputs [B, T, n]; per-utterance maximum (with the incoming umax0) in float32 as
    the kernel keeps it; -> (log float64, max float32 [B])"""
    lg = torch.log10(mel.double().clamp(min=float(np.float32(1e-10))))
    mx = torch.maximum(lg.float().amax(dim=(1, 2)), umax0)
    return lg, mx


def fsq_values(shift):
    """z inputs for one group of 4 dimensions: every special value in every dimension; shift: the 4 per-dimension shifts"""
    inf = float("inf")
    vals = [0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 1e30, -1e30, inf, -inf]
    rows = [[v] * 4 for v in vals] + [[-float(s) for s in shift]]
    return torch.tensor(rows, dtype=torch.float32)


def fsq_ref(z, k12, levels):
    """the kernel's statement with tanh in float64: z [..., 4] float32 -> (zq float32 [..., 4], index int32 [...])"""
    scale, offset, shift = (torch.tensor(k12[i:i + 4], dtype=torch.float32) for i in (0, 4, 8))
    lv = torch.tensor(levels)
    half = (lv // 2).float()
    base = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.long), lv[:-1]]), 0)
    th = torch.tanh((z + shift).double()).float()
    c = torch.round(scale * th - offset)
    return c / half, ((c + half).long() * base).sum(-1).to(torch.int32)
