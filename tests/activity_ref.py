"""The definition of include/swc_activity.h restated in float64 numpy from the header's text alone (ITU-T P.56 method B with the
closed form of the interpolation), and the host policy of metrics.speech_segments / trimmed / split_at_pauses restated in plain
integer Python.  The yardstick of tests/test_activity_cpu.py and tests/test_activity_gpu.py: nothing here calls the library."""
import math

import numpy as np
from scipy.signal import lfilter

T = 0.03
MARGIN_DB = 15.9
HANGOVER_S = 0.2
THRESHOLDS = 15
KEYS = ("active_level", "long_term", "activity", "threshold", "sample_peak", "active_samples", "runs", "crossing")
UNMEASURED, PEAK_LIMITED = 1, 2


def rate_ok(fs):
    return fs == int(fs) and 8000 <= fs <= 48000


def pole(fs):
    return math.exp(-1.0 / (fs * T))


def hangover(fs, hangover_s=HANGOVER_S):
    return int(math.floor(hangover_s * fs + 0.5))


def envelope(x, fs):
    """q of the header: two one-pole stages over |x| from zero state, float64, the whole row"""
    g = pole(fs)
    ax = np.abs(np.asarray(x, dtype=np.float64))
    if len(ax) == 0:
        return ax
    p = lfilter([1.0 - g], [1.0, -g], ax)
    return lfilter([1.0 - g], [1.0, -g], p)


def active_mask(q, c, I):
    """sample i is active iff i - last(i) <= I, last(i) the largest i' <= i with q[i'] >= c"""
    n = len(q)
    idx = np.arange(n, dtype=np.int64)
    last = np.maximum.accumulate(np.where(q >= c, idx, np.int64(-(1 << 40))))
    return idx - last <= I


def runs_of(mask):
    """the maximal intervals [s, e) of True, ascending"""
    m = np.concatenate([[False], np.asarray(mask, dtype=bool), [False]])
    d = np.diff(m.astype(np.int8))
    return list(zip((int(v) for v in np.flatnonzero(d == 1)), (int(v) for v in np.flatnonzero(d == -1))))


def measure(x, fs, margin_db=MARGIN_DB, hangover_s=HANGOVER_S):
    """-> dict: the KEYS (floats; NaN where undefined), "counts" (the fifteen a_j), "run_list" [(s, e)], "q" (the envelope)"""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    I = hangover(fs, hangover_s)
    q = envelope(x, fs)
    xd = x.astype(np.float64)
    sq = float(np.sum(xd * xd))
    nan = math.nan
    res = dict.fromkeys(KEYS, nan)
    res["sample_peak"] = float(np.max(np.abs(x))) if n else 0.0
    counts = [int(active_mask(q, 2.0 ** (j - 15), I).sum()) for j in range(THRESHOLDS)]
    res.update(counts=counts, run_list=[], q=q, active_samples=0.0, runs=0.0)
    if n == 0 or not sq > 0.0:
        return res
    L = 10.0 * math.log10(sq / n)
    res["long_term"] = L
    A = nan
    Ap = Dp = 0.0
    for j in range(THRESHOLDS):
        a = counts[j]
        if a == 0:
            break
        Aj = 10.0 * math.log10(sq / a)
        Dj = Aj - 20.0 * math.log10(2.0 ** (j - 15))
        if Dj <= margin_db:
            if j == 0 or Dj == margin_db:
                A = Aj
            else:
                t = (Dp - margin_db) / (Dp - Dj)
                A = Ap + t * (Aj - Ap)
            res["crossing"] = float(j)
            break
        Ap, Dp = Aj, Dj
    if math.isnan(A):
        return res
    c = 10.0 ** ((A - margin_db) / 20.0)
    mask = active_mask(q, c, I)
    rl = runs_of(mask)
    res.update(active_level=A, activity=10.0 ** ((L - A) / 10.0), threshold=c, active_samples=float(mask.sum()), runs=float(len(rl)),
               run_list=rl)
    return res


def margin(x, fs, margin_db=MARGIN_DB, hangover_s=HANGOVER_S, every_threshold=False):
    """the smallest |q_i - c| / c over all samples and all thresholds used: the c_j up to the one the walk stops at, and c*.
    every_threshold: all fifteen c_j (what a test that compares all fifteen counts needs).  inf for an empty row."""
    r = measure(x, fs, margin_db, hangover_s)
    q = r["q"]
    if len(q) == 0:
        return math.inf
    if every_threshold:
        last = THRESHOLDS - 1
    elif not math.isnan(r["crossing"]):
        last = int(r["crossing"])
    else:
        last = next((j for j, a in enumerate(r["counts"]) if a == 0), THRESHOLDS - 1)
    cs = [2.0 ** (j - 15) for j in range(last + 1)]
    if not math.isnan(r["threshold"]):
        cs.append(r["threshold"])
    return min(float(np.min(np.abs(q - c))) / c for c in cs)


def gain(active_level, peak, target_db=-26.0):
    """-> (gain in float64, flags)"""
    if math.isnan(active_level) or not peak > 0.0 or math.isinf(peak):
        return 1.0, UNMEASURED
    gt, gc = 10.0 ** ((target_db - active_level) / 20.0), 1.0 / peak
    return (gc, PEAK_LIMITED) if gc < gt else (gt, 0)


def f32_margin(g):
    """how far g is from the nearest boundary between two f32 roundings, relative to g"""
    f = np.float32(g)
    lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
    return min(abs(g - 0.5 * (float(f) + float(lo))), abs(g - 0.5 * (float(f) + float(hi)))) / abs(g)


# ---- the host policy on the run list ----

def ms_samples(ms, fs):
    return int(math.floor(ms * fs / 1000.0 + 0.5))


def segments(run_list, fs, hangover_ms=200, min_speech_ms=50, pre_ms=60):
    """drop a run whose e - s - I is under min_speech_ms, move every start back by pre_ms (clamped at 0), merge what touches"""
    I = hangover(fs, hangover_ms / 1000.0)
    keep, pre = ms_samples(min_speech_ms, fs), ms_samples(pre_ms, fs)
    out = []
    for s, e in run_list:
        if e - s - I < keep:
            continue
        s = max(0, s - pre)
        if out and s <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], e))
        else:
            out.append((s, e))
    return out


def trim(segs):
    return (segs[0][0], segs[-1][1]) if segs else (0, 0)


def split(segs, max_len):
    """the pieces of [first start, last end): a piece longer than max_len is cut at its longest interior pause (ties: the pause
    whose midpoint is nearest the piece's midpoint, then the earlier one), the left piece ends at the pause's start, the right
    one begins at its end; a piece with no pause is cut evenly"""
    if not segs:
        return []
    s, e = segs[0][0], segs[-1][1]
    if e - s <= max_len:
        return [(s, e)]
    if len(segs) == 1:
        parts = -(-(e - s) // max_len)
        cuts = [s + (k * (e - s)) // parts for k in range(parts + 1)]
        return list(zip(cuts[:-1], cuts[1:]))
    best = None
    for k in range(len(segs) - 1):
        a, b = segs[k][1], segs[k + 1][0]
        key = (-(b - a), abs((a + b) - (s + e)), k)
        if best is None or key < best[0]:
            best = (key, k)
    k = best[1]
    return split(segs[:k + 1], max_len) + split(segs[k + 1:], max_len)
