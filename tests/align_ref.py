"""The numpy restatement of include/swc_align.h: the level, the sequence of either mode, the direct int64 correlation (one dot
product per lag: no FFT, which is not exact at 2^52), the choice under the tie rule, the overlap and the two values.  The GPU
tests compare swc_align with this bit for bit (xc, info) and within one f32 ulp (values)."""
import math

import numpy as np

WAVEFORM, ENVELOPE = 0, 1
MODES = {"waveform": WAVEFORM, "envelope": ENVELOPE}
MAX_LAG = 32768
MAX_N = 1 << 22


def quantise(v):
    """-> (q int64 [n], e, state): state "ok" or "undefined" (a NaN or Inf peak); peak == 0 gives e = 0 and q = 0"""
    v = np.asarray(v, dtype=np.float32)
    if len(v) == 0:
        return np.zeros(0, np.int64), 0, "ok"
    peak = np.abs(v).max()
    if not np.isfinite(peak):
        return np.zeros(len(v), np.int64), 0, "undefined"
    e = int(np.frexp(np.float32(peak))[1]) if peak != 0 else 0
    q = np.clip(np.rint(np.ldexp(v.astype(np.float64), 15 - e)), -32767, 32767).astype(np.int64)
    return q, e, "ok"


def sequence(q, mode):
    """s of the header: q itself, or |q| minus the floor of its mean"""
    if mode == WAVEFORM or len(q) == 0:
        return q.copy()
    a = np.abs(q)
    return a - int(a.sum()) // len(q)


def xcorr(sx, sy, L):
    """c[d] for d = -L .. L at index d + L: sum over the i with 0 <= i < nx and 0 <= i + d < ny, int64"""
    nx, ny = len(sx), len(sy)
    c = np.zeros(2 * L + 1, np.int64)
    for d in range(-L, L + 1):
        lo, hi = max(0, -d), min(nx, ny - d)
        if hi > lo:
            c[d + L] = np.dot(sx[lo:hi], sy[lo + d:hi + d])
    return c


def choose(c, L):
    """d*: the largest c among the positive ones; ties to the smaller |d|, then to d >= 0; 0 without a positive c"""
    best = None
    for k in range(2 * L + 1):
        d, v = k - L, int(c[k])
        if v <= 0:
            continue
        key = (-v, abs(d), 0 if d >= 0 else 1)
        if best is None or key < best[0]:
            best = (key, d)
    return 0 if best is None else best[1]


def overlap(d, nx, ny):
    x0, y0 = max(0, -d), max(0, d)
    return x0, y0, max(0, min(nx - x0, ny - y0))


def align(x, y, L, mode):
    """-> dict(info int32 [4], values float32 [4], xc int64 [2 L + 1])"""
    mode = MODES.get(mode, mode)
    assert 0 <= L <= MAX_LAG and mode in (WAVEFORM, ENVELOPE)
    nan = np.float32(np.nan)
    empty = dict(info=np.zeros(4, np.int32), values=np.array([nan, nan, 0, 0], np.float32), xc=np.zeros(2 * L + 1, np.int64))
    if len(x) == 0 or len(y) == 0:
        return empty
    qx, ex, stx = quantise(x)
    qy, ey, sty = quantise(y)
    if stx != "ok" or sty != "ok":
        return empty
    sx, sy = sequence(qx, mode), sequence(qy, mode)
    c = xcorr(sx, sy, L)
    d = choose(c, L)
    x0, y0, m = overlap(d, len(x), len(y))
    ox, oy = slice(x0, x0 + m), slice(y0, y0 + m)
    Sxx, Syy = int(np.dot(sx[ox], sx[ox])), int(np.dot(sy[oy], sy[oy]))
    Exx, Eyy = int(np.dot(qx[ox], qx[ox])), int(np.dot(qy[oy], qy[oy]))
    prod = float(Sxx) * float(Syy)
    corr = float(int(c[d + L])) / math.sqrt(prod) if prod != 0.0 else math.nan
    gain = math.ldexp(math.sqrt(float(Exx) / float(Eyy)), ex - ey) if Eyy != 0 else math.nan
    return dict(info=np.array([d, x0, y0, m], np.int32), values=np.array([corr, gain, 0, 0], np.float64).astype(np.float32), xc=c)


def delayed(x, d, n=None):
    """x cut d samples later: y[i] = x[i - d], zeros shifted in (not np.roll), n samples (default len(x))"""
    n = len(x) if n is None else n
    y = np.zeros(n, dtype=x.dtype)
    lo, hi = max(0, d), min(n, len(x) + d)
    if hi > lo:
        y[lo:hi] = x[lo - d:hi - d]
    return y


def envelope_pair(seed, d, n=32000):
    """x = env noise_1, y = 0.5 env noise_2 delayed by d: one envelope (the square of white noise smoothed by an 801-tap Hann
    window), two independent carriers"""
    rng = np.random.default_rng(seed)
    env = np.convolve(rng.standard_normal(n + 800), np.hanning(801) / np.hanning(801).sum(), mode="valid") ** 2
    x = (env * rng.standard_normal(n)).astype(np.float32)
    y = delayed((0.5 * env * rng.standard_normal(n)).astype(np.float32), d)
    return x, y
