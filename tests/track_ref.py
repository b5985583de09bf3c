"""The numpy restatement of include/swc_track.h, from its text alone: the two host-built tables, the segments, the direct int64
correlation of every segment, the integer peak under swc_align.h's tie rule, the sub-sample peak (one individually rounded
float64 chain per position, then the parabola), the per-segment values, the two-pass weighted line, and the Q32 warp in
float64.  The GPU tests compare swc_lag_track with this bit for bit (c, d*, status) and within 1e-12 relative (lag, rho, t),
swc_lag_fit within 1e-12 relative, swc_warp within the bound of its f32 chain.  Also here: the analytic pairs (sums of
amplitude-modulated sinusoids evaluated in float64 at the sample instants of either clock: no resampler takes part)."""
import math

import numpy as np

import align_ref

W, P = 16, 32
ROWS, COLS = P + 3, 2 * W + 1
MAX_RANGE = 1024
MAX_N = 1 << 22
MAX_SEGMENTS = 4096
DEFINED, EDGE = 1, 2
NO_DRIFT, NO_LAG, FIT_EDGE = 1, 2, 4
TAPS, PHASES = 32, 256
MAX_DRIFT = 0.01
MAX_LAG = float(1 << 23)


def _sinc(u):
    u = np.asarray(u, np.float64)
    safe = np.where(u == 0, 1.0, u)
    return np.where(u == 0, 1.0, np.sin(np.pi * safe) / (np.pi * safe))


def track_table():
    """T[j + P/2 + 1][t + W] = sinc(t - j / P) (0.5 + 0.5 cos(pi (t - j / P) / (W + 1))), float64 [35][33]"""
    j = np.arange(-P // 2 - 1, P // 2 + 2, dtype=np.float64)[:, None]
    t = np.arange(-W, W + 1, dtype=np.float64)[None, :]
    u = t - j / P
    return _sinc(u) * (0.5 + 0.5 * np.cos(np.pi * u / (W + 1)))


def warp_table():
    """H[p][t + 15] = float32(sinc(t - p / 256) (0.5 + 0.5 cos(pi (t - p / 256) / 16))), [257][32]"""
    p = np.arange(PHASES + 1, dtype=np.float64)[:, None]
    t = np.arange(-15, 17, dtype=np.float64)[None, :]
    u = t - p / PHASES
    return (_sinc(u) * (0.5 + 0.5 * np.cos(np.pi * u / 16))).astype(np.float32)


def segments(n, S, H):
    if n <= 0:
        return 0
    if S == 0 or n <= S:
        return 1
    return -((S - n) // H) + 1


def _sequences(x, y, mode):
    """-> (sx, sy) int64, or None for an empty or not-defined pair"""
    if len(x) == 0 or len(y) == 0:
        return None
    qx, _, stx = align_ref.quantise(x)
    qy, _, sty = align_ref.quantise(y)
    if stx != "ok" or sty != "ok":
        return None
    return align_ref.sequence(qx, mode), align_ref.sequence(qy, mode)


def seg_corr(sx, sy, lo_x, hi_x, dc, R):
    """c_k[d], d = -R .. R at index d + R: sum over lo_x <= i < hi_x with 0 <= i + dc + d < ny"""
    ny = len(sy)
    c = np.zeros(2 * R + 1, np.int64)
    for d in range(-R, R + 1):
        s = dc + d
        lo, hi = max(lo_x, -s), min(hi_x, ny - s)
        if hi > lo:
            c[d + R] = np.dot(sx[lo:hi], sy[lo + s:hi + s])
    return c


def peak(c, Rs, R):
    """d* over |d| <= Rs, or None"""
    inner = c[R - Rs:R + Rs + 1]
    if inner.max(initial=0) <= 0:
        return None
    return align_ref.choose(inner, Rs)


def sub_sample(c, dstar, R, table):
    """-> (j*, delta): the chains in ascending t, the product rounded, then the sum"""
    cc = c[dstar + R - W:dstar + R + W + 1].astype(np.float64)
    ct = np.zeros(ROWS, np.float64)
    for t in range(COLS):
        ct = ct + cc[t] * table[:, t]
    mid = P // 2 + 1
    js, y0 = 0, ct[mid]
    for a in range(1, P // 2 + 1):
        if ct[mid + a] > y0:
            y0, js = ct[mid + a], a
        if ct[mid - a] > y0:
            y0, js = ct[mid - a], -a
    ym, yp = ct[mid + js - 1], ct[mid + js + 1]
    num = ym - yp
    den = (ym - y0) + (yp - y0)
    delta = 0.5 * (num / den) if den < 0 else 0.0
    return js, min(max(delta, -0.5), 0.5)


def lag_track(x, y, d0, S, H, Rs, mode, table=None):
    """-> dict(vals float64 [K][4], status int32 [K], xc int64 [K][2 R + 1], dstar list); K = 0 for an empty / undefined pair"""
    mode = align_ref.MODES.get(mode, mode)
    table = track_table() if table is None else table
    R = Rs + W + 1
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    seq = _sequences(x, y, mode)
    K = segments(len(x), S, H) if seq is not None else 0
    vals = np.tile(np.array([np.nan, np.nan, 0.0, np.nan]), (K, 1))
    status = np.zeros(K, np.int32)
    xc = np.zeros((K, 2 * R + 1), np.int64)
    dstars = [None] * K
    if K == 0:
        return dict(vals=vals, status=status, xc=xc, dstar=dstars)
    sx, sy = seq
    nx, ny = len(sx), len(sy)
    for k in range(K):
        s0 = 0 if S == 0 else k * H
        s1 = nx if S == 0 else min(s0 + S, nx)
        c = seg_corr(sx, sy, s0, s1, d0, R)
        xc[k] = c
        ds = peak(c, Rs, R)
        if ds is None:
            continue
        dstars[k] = ds
        dd = d0 + ds
        lo, hi = max(s0, -dd), min(s1, ny - dd)
        Sxx = int(np.dot(sx[lo:hi], sx[lo:hi]))
        Syy = int(np.dot(sy[lo + dd:hi + dd], sy[lo + dd:hi + dd]))
        js, delta = sub_sample(c, ds, R, table)
        vals[k, 0] = float(dd) + (float(js) + delta) / P
        vals[k, 1] = float(int(c[ds + R])) / math.sqrt(float(Sxx) * float(Syy))
        vals[k, 2] = float(Sxx)
        vals[k, 3] = float(lo + hi - 1) * 0.5
        status[k] = DEFINED | (EDGE if abs(ds) == Rs else 0)
    return dict(vals=vals, status=status, xc=xc, dstar=dstars)


def _line(vals, use, drift):
    """line(U) of the header -> (a, b, sw, n, flat)"""
    ks = [k for k in range(len(vals)) if use[k]]
    if not ks:
        return 0.0, 0.0, 0.0, 0, False
    sw = swt = swl = 0.0
    for k in ks:
        l, _, w, t = vals[k]
        sw = sw + w
        swt = swt + w * t
        swl = swl + w * l
    tm, lm = swt / sw, swl / sw
    stt = stl = 0.0
    for k in ks:
        l, _, w, t = vals[k]
        dt, dl = t - tm, l - lm
        stt = stt + w * (dt * dt)
        stl = stl + w * (dt * dl)
    if not drift:
        return lm, 0.0, sw, len(ks), False
    if len(ks) < 2 or not stt > 0.0:
        return 0.0, 0.0, sw, len(ks), True
    b = stl / stt
    return lm - b * tm, b, sw, len(ks), False


def lag_fit(vals, status, d0, rho_min=0.3, drift=True):
    """-> dict(a, b, rms, used, offered, flags)"""
    vals = [tuple(float(v) for v in row) for row in vals]
    K = len(vals)
    u1 = [bool(status[k] & DEFINED) and vals[k][1] >= rho_min for k in range(K)]

    def flags_of(n, flat):
        return (NO_LAG if n == 0 else 0) | (NO_DRIFT if drift and (n < 2 or flat) else 0)

    a1, b1, sw, n, flat = _line(vals, u1, drift)
    flags, used = flags_of(n, flat), n
    a = b = rms = None
    if flags == 0:
        u2 = [u1[k] and abs(vals[k][0] - (a1 + b1 * vals[k][3])) <= 1.0 for k in range(K)]
        a, b, sw, n, flat = _line(vals, u2, drift)
        flags, used = flags_of(n, flat), n
        if flags == 0:
            sr = 0.0
            for k in range(K):
                if u2[k]:
                    r = vals[k][0] - (a + b * vals[k][3])
                    sr = sr + vals[k][2] * (r * r)
                    if status[k] & EDGE:
                        flags |= FIT_EDGE
            rms = math.sqrt(sr / sw)
    if flags & (NO_LAG | NO_DRIFT):
        a, b, rms = float(d0), 0.0, math.nan
    return dict(a=a, b=b, rms=rms, used=used, offered=K, flags=flags)


def warp_q32(a, b):
    """-> (A, Q) as Python ints, or None for a pair that is not warped"""
    if not (abs(a) <= MAX_LAG and abs(b) <= MAX_DRIFT):
        return None
    return int(np.rint(np.float64(a) * 4294967296.0)), int(np.rint((np.float64(1.0) + np.float64(b)) * 4294967296.0))


def warp_bounds(A, Q, nx, ny, cols):
    """x0, m in Python integers (floor division is exact)"""
    if nx <= 0 or ny <= 0:
        return 0, 0
    first = -((A) // Q)                      # ceil(-A / Q)
    last = ((ny << 32) - 1 - A) // Q
    lo = max(first, 0)
    m = max(0, min(min(last + 1, nx) - lo, cols))
    return (lo if m > 0 else 0), m


def warp(y, a, b, nx, cols, table=None):
    """-> dict(out float64 [cols], bound float64 [cols] = sum_t |h_t y_t|, x0, m, flag): the float64 evaluation of the same
    table and the same positions (h itself as the kernel rounds it: two f32 roundings; the chain in float64)"""
    table = warp_table() if table is None else table
    y = np.asarray(y, np.float32)
    ny = len(y)
    out, bound = np.zeros(cols, np.float64), np.zeros(cols, np.float64)
    q = warp_q32(a, b)
    if q is None:
        return dict(out=out, bound=bound, x0=0, m=0, flag=1)
    A, Q = q
    x0, m = warp_bounds(A, Q, nx, ny, cols)
    ypad = np.concatenate([np.zeros(16, np.float64), y.astype(np.float64), np.zeros(17, np.float64)])   # ypad[g + 16] = y[g]
    taps = np.arange(1, TAPS + 1, dtype=np.int64)[None, :]                                              # g = ip + t, t = -15 .. 16
    for c0 in range(0, m, 32768):
        c = np.arange(c0, min(c0 + 32768, m), dtype=np.int64)
        pos = A + (x0 + c) * Q                                  # below 2^56: exact in int64
        ip, frac = pos >> 32, pos & 0xffffffff
        phase = frac >> 24
        wt = (frac & 0xffffff).astype(np.float32) * np.float32(2.0 ** -24)
        h0, h1 = table[phase], table[phase + 1]
        dh = (h1 - h0).astype(np.float32)
        # fmaf(wt, dh, h0): the product is exact in float64, the sum rounds to 53 bits and then to 24
        h = (wt.astype(np.float64)[:, None] * dh.astype(np.float64) + h0.astype(np.float64)).astype(np.float32).astype(np.float64)
        ys = ypad[ip[:, None] + taps]
        out[c] = (h * ys).sum(axis=1)
        bound[c] = (np.abs(h) * np.abs(ys)).sum(axis=1)
    return dict(out=out, bound=bound, x0=x0, m=m, flag=0)


# ---- analytic pairs ----

def tones(seed, n_tones=60, fmax=0.4):
    """the parameters of a sum of amplitude-modulated sinusoids: carrier frequencies up to fmax cycles per sample (0.8 Nyquist),
    slow modulators"""
    rng = np.random.default_rng(seed)
    return dict(f=rng.uniform(0.005, fmax, n_tones), ph=rng.uniform(0, 2 * np.pi, n_tones), amp=rng.uniform(0.2, 1.0, n_tones),
                fm=rng.uniform(1e-5, 2e-4, n_tones), pm=rng.uniform(0, 2 * np.pi, n_tones))


def evaluate(par, t):
    """x_cont at the (fractional) instants t, float64"""
    t = np.asarray(t, np.float64)[:, None]
    v = par["amp"] * (1.0 + 0.5 * np.sin(2 * np.pi * par["fm"] * t + par["pm"])) * np.sin(2 * np.pi * par["f"] * t + par["ph"])
    return v.sum(axis=1) / len(par["f"]) * 4.0


def analytic_pair(seed, n, a, b, g=0.5, noise=0.0, ny=None, n_tones=60):
    """x[i] = x_cont(i), y[j] = g x_cont((j - a) / (1 + b)) (+ white noise at `noise` times y's rms) -> float32 rows"""
    par = tones(seed, n_tones)
    ny = n if ny is None else ny
    x = evaluate(par, np.arange(n, dtype=np.float64))
    y = g * evaluate(par, (np.arange(ny, dtype=np.float64) - a) / (1.0 + b))
    if noise:
        rng = np.random.default_rng(seed + 1000)
        y = y + noise * math.sqrt(float(np.mean(y * y))) * rng.standard_normal(ny)
    return x.astype(np.float32), y.astype(np.float32)


def si_sdr(x, y):
    """of the estimate y against the target x, float64, dB"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    al = np.dot(x, y) / np.dot(x, x)
    e = y - al * x
    return 10.0 * math.log10(np.dot(al * x, al * x) / np.dot(e, e))


def pipeline(x, y, L, S, H, Rs, mode="waveform", drift=True, rho_min=0.3):
    """align -> lag_track -> lag_fit -> warp, as metrics.aligned(fine=...) chains them -> dict"""
    d0 = int(align_ref.align(x, y, L, mode)["info"][0])
    tr = lag_track(x, y, d0, S, H, Rs, mode)
    ft = lag_fit(tr["vals"], tr["status"], d0, rho_min, drift)
    wp = warp(y, ft["a"], ft["b"], len(x), len(x))
    return dict(d0=d0, track=tr, fit=ft, warp=wp)
