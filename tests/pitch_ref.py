"""A numpy restatement of include/swc_pitch.h, written from the header's text alone: int64 for d and S, float64 beyond.  Not
derived from the kernel: it takes the difference function as written (a sum of squared differences), one frame at a time."""
import math

import numpy as np

NUM, DEN = 3, 20     # 20 d tau < 3 S: threshold 0.15


def params(sample_rate, f_min=62.5, f_max=500.0):
    """-> dict(sr, W, tau_min, tau_max, H) as the Python layer derives them from the rate"""
    sr = int(sample_rate)
    tau_min, tau_max = int(math.floor(sr / f_max)), int(math.ceil(sr / f_min))
    return dict(sr=sr, W=2 * tau_max, tau_min=tau_min, tau_max=tau_max, H=int(round(sr / 100.0)))


def n_frames(n, W, tau_max, H):
    span = W + tau_max
    return 0 if n < span else 1 + (n - span) // H


def quantise(x):
    """-> (q int64 [n], state) with state "ok", "zero" (q is None) or "nan" (q is None)"""
    x = np.asarray(x, dtype=np.float32)
    if x.size == 0:
        return None, "zero"
    peak = np.max(np.abs(x))
    if not np.isfinite(peak):
        return None, "nan"
    if peak == 0:
        return None, "zero"
    _, e = np.frexp(np.float32(peak))
    q = np.rint(np.ldexp(x.astype(np.float64), 15 - int(e)))     # exact: a power of two
    return np.clip(q, -32767, 32767).astype(np.int64), "ok"


def difference(s, W, tau_max):
    """d(tau), tau = 0 .. tau_max, of one frame s = q[t H .. t H + span) in int64, as the header writes it"""
    a = s[:W]
    lagged = np.lib.stride_tricks.sliding_window_view(s, W)[:tau_max + 1]
    return ((a[None, :] - lagged) ** 2).sum(axis=1, dtype=np.int64)


def frame(s, sr, W, tau_min, tau_max, detail=None):
    """-> (tau, f0 float64) of one frame"""
    d = difference(s, W, tau_max)
    S = np.cumsum(d) - d[0]
    k = np.arange(tau_max + 1, dtype=np.int64)
    dk = d * k
    dp = np.ones(tau_max + 1, dtype=np.float64)
    nz = S > 0
    nz[0] = False
    dp[nz] = dk[nz].astype(np.float64) / S[nz].astype(np.float64)
    if detail is not None:
        detail.update(d=d, S=S, dk=dk, dp=dp)
    below = (S > 0) & (DEN * dk < NUM * S) & (k >= tau_min)
    if not below.any():
        return 0, 0.0
    c = int(np.argmax(below))
    while c + 1 <= tau_max and dp[c + 1] < dp[c]:
        c += 1
    off = 0.0
    if c + 1 <= tau_max:
        a, b, g = dp[c - 1], dp[c], dp[c + 1]
        den = (a - 2.0 * b) + g
        if den > 0:
            off = min(1.0, max(-1.0, (0.5 * (a - g)) / den))
        if detail is not None:
            detail.update(off=off)
    return c, float(sr) / (float(c) + off)


def track(x, sr=16000, W=512, tau_min=32, tau_max=256, H=160):
    """-> (tau int32 [T], f0 float32 [T]) of one row; a row that is not defined has tau -1 and f0 NaN"""
    x = np.asarray(x, dtype=np.float32)
    T = n_frames(len(x), W, tau_max, H)
    tau, f0 = np.zeros(T, np.int32), np.zeros(T, np.float32)
    q, state = quantise(x)
    if state == "nan":
        tau[:] = -1
        f0[:] = np.nan
    if state != "ok":
        return tau, f0
    span = W + tau_max
    for t in range(T):
        c, f = frame(q[t * H:t * H + span], sr, W, tau_min, tau_max)
        tau[t], f0[t] = c, np.float32(f)
    return tau, f0


def pair_values(f0_x, f0_y):
    """the header's pair formulas on two STORED tracks (f32) -> (values float64 [8], counts int [4])"""
    fx, fy = np.asarray(f0_x, np.float32).astype(np.float64), np.asarray(f0_y, np.float32).astype(np.float64)
    T = len(fx)
    nan = float("nan")
    if np.isnan(fx).any() or np.isnan(fy).any():
        return np.array([nan] * 7 + [0.0]), np.array([T, 0, 0, 0])
    vx, vy = fx > 0, fy > 0
    vv = vx & vy
    n_vx, n_vy, n_vv = int(vx.sum()), int(vy.sum()), int(vv.sum())
    v = np.full(8, nan)
    v[7] = 0.0
    if n_vv > 0:
        ratio = fy[vv] / fx[vv]
        cents = 1200.0 * np.log2(ratio)
        v[0] = math.sqrt(float(np.sum(cents * cents)) / n_vv)
        v[2] = float(np.sum(np.abs(ratio - 1.0) > 0.2)) / n_vv
    if n_vv >= 2:
        dx, dy = fx[vv] - fx[vv].sum() / n_vv, fy[vv] - fy[vv].sum() / n_vv
        sxx, syy = float(np.sum(dx * dx)), float(np.sum(dy * dy))
        if sxx > 0 and syy > 0:
            v[1] = float(np.sum(dx * dy)) / math.sqrt(sxx * syy)
    if T > 0:
        v[3] = float(np.sum(vx != vy)) / T
        v[5], v[6] = n_vx / T, n_vy / T
    if n_vx + n_vy > 0:
        v[4] = 2.0 * n_vv / (n_vx + n_vy)
    return v, np.array([T, n_vx, n_vy, n_vv])


def pitch(x, y, **p):
    """a pair -> dict(tau_x, f0_x, tau_y, f0_y, values, counts)"""
    n = min(len(x), len(y))
    tx, fx = track(np.asarray(x)[:n], **p)
    ty, fy = track(np.asarray(y)[:n], **p)
    v, c = pair_values(fx, fy)
    return dict(tau_x=tx, f0_x=fx, tau_y=ty, f0_y=fy, values=v, counts=c)


# ---- signals ----

def harmonic_complex(f, n, sr, harmonics=5, amp=0.3):
    t = np.arange(n, dtype=np.float64) / sr
    f = np.broadcast_to(np.asarray(f, dtype=np.float64), t.shape)
    phase = 2.0 * np.pi * np.cumsum(f) / sr
    return (amp * sum(np.sin(h * phase + h) / h for h in range(1, harmonics + 1))).astype(np.float32)


TOP = np.float32(1.0) - np.float32(2.0 ** -24)      # the largest f32 below 1: quantises to 32768 and is clamped to 32767


def alternating(n, amp=1.0):
    """the full-scale +amp / -amp row of the limit configuration: amp = 1 quantises to +-16384 (1 = 0.5 * 2^1), amp = TOP to
    +-32767, the largest |q| there is"""
    x = np.full(n, amp, np.float32)
    x[1::2] = -x[1::2]
    return x


def test_signal(seed, sr=16000, shift=1.0, noise=0.0):
    """about 2 s: harmonic glides, noise, a stretch of exact zeros, a full-scale clipped square wave and a quiet (peak 1e-4)
    voiced stretch.  shift: the factor on the pitch of the second glide; noise: white noise added to everything"""
    rng = np.random.default_rng(seed)
    seg = lambda sec: int(round(sec * sr))
    parts = [
        harmonic_complex(np.linspace(100.0, 250.0, seg(0.45)), seg(0.45), sr),
        (0.1 * rng.standard_normal(seg(0.25))).astype(np.float32),
        harmonic_complex(shift * np.linspace(220.0, 140.0, seg(0.4)), seg(0.4), sr),
        np.zeros(seg(0.2), np.float32),
        np.clip(40.0 * harmonic_complex(125.0, seg(0.3), sr, harmonics=1, amp=1.0), -1.0, 1.0).astype(np.float32),
        (1e-4 / 0.45) * harmonic_complex(180.0, seg(0.41) + 37, sr),
    ]
    x = np.concatenate(parts)
    if noise:
        x = x + (noise * np.random.default_rng(seed + 1000).standard_normal(len(x))).astype(np.float32)
    return x.astype(np.float32)
