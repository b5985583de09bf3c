"""include/swc_stretch.h restated in numpy, from the header's text alone: the level, the lengths, the positions by the
least-squares search in exact int64, and the output in f32 with one rounded product and one fused multiply-add per sample
(fmaf of tests/degrade_ref.py).  stretch64 evaluates the same output in float64 from the same positions."""
import numpy as np

from degrade_ref import fmaf

MIN_W, MAX_W, MAX_D, MAX_TERM, MAX_RATIO, MAX_N, CHUNK, UNDEFINED = 16, 2048, 1024, 65535, 4, 1 << 22, 4096, 1


def speed_ok(num, den):
    return 1 <= num <= MAX_TERM and 1 <= den <= MAX_TERM and num <= MAX_RATIO * den and den <= MAX_RATIO * num


def window_ok(W):
    return MIN_W <= W <= MAX_W and W % 8 == 0


def out_len(n, num, den):
    """ceil(n den / num); -1 outside the limits"""
    if not 0 <= n <= MAX_N or not speed_ok(num, den):
        return -1
    return -(-n * den // num)


def frames(n, W, num, den):
    return -(-out_len(n, num, den) // (W // 2))


def up256(v):
    return (v + 255) // 256 * 256


def workspace_bytes(B, max_n, W, num, den):
    if not 0 <= B <= 65535 or not 0 <= max_n <= MAX_N or not window_ok(W) or not speed_ok(num, den):
        return -1
    return up256(4 * B) + up256(4 * W) + up256(4 * B * frames(max_n, W, num, den))


def quantise(x):
    """-> (q int64 [n], defined)"""
    x = np.asarray(x, dtype=np.float32)
    if len(x) == 0:
        return np.zeros(0, np.int64), True
    peak = np.abs(x).max()
    if not np.isfinite(peak):
        return np.zeros(len(x), np.int64), False
    e = int(np.frexp(np.float32(peak))[1]) if peak != 0 else 0
    return np.clip(np.rint(np.ldexp(x.astype(np.float64), 15 - e)), -32767, 32767).astype(np.int64), True


def take(v, start, count):
    """v[start .. start + count) with zeros outside [0, len(v))"""
    out = np.zeros(count, dtype=v.dtype)
    lo, hi = max(start, 0), min(start + count, len(v))
    if hi > lo:
        out[lo - start:hi - start] = v[lo:hi]
    return out


def window(W):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W, dtype=np.float64) / W)).astype(np.float32)


def track(x, W, D, num, den, count_ties=False):
    """-> (pos int32 [J], dist int64 [J], defined) and, with count_ties, the number of frames whose smallest Dm is reached by
    more than one d"""
    assert window_ok(W) and 0 <= D <= MAX_D and speed_ok(num, den)
    x = np.asarray(x, dtype=np.float32)
    n, Hs = len(x), W // 2
    J = frames(n, W, num, den)
    pos, dist = np.zeros(J, np.int32), np.zeros(J, np.int64)
    q, defined = quantise(x)
    ties = 0
    if defined:
        s = 0
        for m in range(1, J):
            a = (m * Hs * num) // den
            target = take(q, s + Hs, W)
            span = take(q, a - D, 2 * D + W)
            cand = np.lib.stride_tricks.sliding_window_view(span, W)          # [2 D + 1][W], row o is d = o - D
            Dm = ((cand - target[None, :]) ** 2).sum(axis=1)
            best = None
            for o in np.flatnonzero(Dm == Dm.min()):
                d = int(o) - D
                key = (abs(d), 0 if d >= 0 else 1)
                if best is None or key < best[0]:
                    best = (key, d)
            ties += int((Dm == Dm.min()).sum() > 1)
            s = a + best[1]
            pos[m], dist[m] = s, Dm.min()
    return (pos, dist, defined, ties) if count_ties else (pos, dist, defined)


def _reads(x, pos, W, count):
    """the two samples every output sample t < count is made of, and their window values' indices"""
    Hs = W // 2
    t = np.arange(count)
    j, u = t // Hs, t % Hs
    s = pos.astype(np.int64)
    prev = np.concatenate([[-Hs], s[:-1]]) if len(s) else s
    ia, ib = s[j] + u, prev[j] + Hs + u

    def X(i):
        ok = (i >= 0) & (i < len(x))
        out = np.zeros(len(i), dtype=x.dtype)
        out[ok] = x[i[ok]]
        return out
    return X(ia), X(ib), u


def synthesise(x, pos, defined, W, num, den, cols=None):
    """-> y f32 [cols]: the output contract (samples below min(n_out, cols), zeros behind); cols defaults to n_out"""
    x = np.asarray(x, dtype=np.float32)
    n_out = out_len(len(x), num, den)
    cols = n_out if cols is None else cols
    y = np.zeros(cols, np.float32)
    count = min(n_out, cols) if defined else 0
    if count:
        xa, xb, u = _reads(x, pos, W, count)
        w = window(W)
        y[:count] = fmaf(w[u], xa, w[u + W // 2] * xb)      # f32 * f32 -> f32: the product rounded once
    return y


def stretch64(x, pos, W, num, den):
    """the same output in float64 with the float64 window: what the f32 form is measured against"""
    x = np.asarray(x, dtype=np.float64)
    n_out = out_len(len(x), num, den)
    xa, xb, u = _reads(x, pos, W, n_out)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W, dtype=np.float64) / W)
    return w[u] * xa + w[u + W // 2] * xb


def stretch(x, W, D, num, den, cols=None):
    """-> dict(out f32 [cols], pos int32 [J], dist int64 [J], flag)"""
    pos, dist, defined = track(x, W, D, num, den)
    return dict(out=synthesise(x, pos, defined, W, num, den, cols), pos=pos, dist=dist, flag=0 if defined else UNDEFINED)

