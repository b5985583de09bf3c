"""A float64 numpy restatement of include/swc_loudness.h: K-weighting, sub-block energies, momentary and short-term loudness, the
gates of BS.1770-4 (integrated loudness) and EBU Tech 3342 (loudness range), the peaks, and the normalising gain.  Nothing here
is shared with the kernels; the true peak alone is taken from the project's host resampler (wavio.resample), as the header
defines it."""
import math

import numpy as np

try:
    from scipy.signal import lfilter
except ImportError:   # a plain loop: the same recursion, slowly
    def lfilter(b, a, x):
        y = np.zeros(len(x))
        x1 = x2 = y1 = y2 = 0.0
        for i, v in enumerate(x):
            y[i] = b[0] * v + b[1] * x1 + b[2] * x2 - a[1] * y1 - a[2] * y2
            x2, x1, y2, y1 = x1, v, y1, y[i]
        return y

ABS_GATE = -70.0
KEYS = ("integrated", "range", "momentary_max", "short_term_max", "sample_peak", "true_peak", "blocks", "blocks_kept")
UNMEASURED, PEAK_LIMITED = 1, 2


def rate_ok(fs):
    return isinstance(fs, int) and 8000 <= fs <= 48000 and fs % 10 == 0


def coefficients(fs):
    """-> (b_shelf, a_shelf, b_hp, a_hp), float64, from the header's text"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return b1, a1, b2, a2


def loud(e):
    """-0.691 + 10 log10(e), -inf at 0, elementwise"""
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(np.asarray(e, dtype=np.float64))


def energies(x, fs):
    """z_k of the K-weighted row over its whole sub-blocks of fs / 10 samples"""
    x = np.asarray(x, dtype=np.float64)
    L = fs // 10
    S = len(x) // L
    if S == 0:
        return np.zeros(0)
    b1, a1, b2, a2 = coefficients(fs)
    y = lfilter(b2, a2, lfilter(b1, a1, x))
    return (y[:S * L].reshape(S, L) ** 2).mean(axis=1)


def block_energies(z, m):
    """the mean of z_j .. z_j+m-1 for every j that has them"""
    n = len(z) - m + 1
    if n <= 0:
        return np.zeros(0)
    return np.array([z[j:j + m].sum() / m for j in range(n)])


def gates(e, rel):
    """e = block energies -> (their loudness, the relative gate or None when nothing passes the absolute one, the kept mask)"""
    l = loud(e)
    a = l > ABS_GATE
    if not a.any():
        return l, None, a
    gamma = float(loud(e[a].mean())) + rel
    return l, gamma, a & (l > gamma)


def percentile_indices(n):
    """the two ranks of EBU Tech 3342 among n kept values in ascending order: (10 %, 95 %)"""
    return int(math.floor(0.10 * (n - 1) + 0.5)), int(math.floor(0.95 * (n - 1) + 0.5))


def true_peak(x, fs):
    """max |wavio.resample(x, fs, 4 fs)| (f32), 0 for an empty row"""
    import torch
    from simwhisper_codec_amd import wavio
    x = np.asarray(x, dtype=np.float32)
    if len(x) == 0:
        return 0.0
    return float(wavio.resample(torch.from_numpy(x), 1, 4).abs().max())


def measure(x, fs, with_true_peak=True):
    """-> dict of the eight values (KEYS), NaN where the header says so; with_true_peak=False leaves "true_peak" NaN"""
    assert rate_ok(fs)
    x = np.asarray(x, dtype=np.float32)
    z = energies(x, fs)
    em, es = block_energies(z, 4), block_energies(z, 30)
    res = dict.fromkeys(KEYS, math.nan)
    lm, _, keep = gates(em, -10.0)
    res["blocks"], res["blocks_kept"] = float(len(em)), float(keep.sum())
    if keep.any():
        res["integrated"] = float(loud(em[keep].mean()))
    if len(em):
        res["momentary_max"] = float(lm.max())
    ls, _, keep3 = gates(es, -20.0)
    if len(es):
        res["short_term_max"] = float(ls.max())
    if keep3.any():
        v = np.sort(ls[keep3])
        lo, hi = percentile_indices(len(v))
        res["range"] = float(v[hi] - v[lo])
    res["sample_peak"] = float(np.abs(x).max()) if len(x) else 0.0
    if with_true_peak:
        res["true_peak"] = true_peak(x, fs)
    return res


def gate_margin(x, fs):
    """the smallest |l_j - gate| over all blocks and both gates, for both I and LRA (inf when there is nothing to compare): a
    case with a margin well above the arithmetic's error cannot have a block flipped by it"""
    z = energies(np.asarray(x, dtype=np.float32), fs)
    m = math.inf
    for width, rel in ((4, -10.0), (30, -20.0)):
        e = block_energies(z, width)
        if len(e) == 0:
            continue
        l, gamma, _ = gates(e, rel)
        fin = l[np.isfinite(l)]
        if len(fin):
            m = min(m, float(np.abs(fin - ABS_GATE).min()))
            if gamma is not None:
                m = min(m, float(np.abs(fin - gamma).min()))
    return m


def gain(integrated, true_peak, target=-23.0, ceiling=-1.0):
    """-> (g float64, flags) of swc_loudness_normalise"""
    if math.isnan(integrated) or not (true_peak > 0.0) or math.isinf(true_peak):
        return 1.0, UNMEASURED
    gt = 10.0 ** ((target - integrated) / 20.0)
    gc = 10.0 ** (ceiling / 20.0) / true_peak
    return (gc, PEAK_LIMITED) if gc < gt else (gt, 0)


def f32_margin(g):
    """the relative distance of g to the nearest point where its rounding to f32 changes (the middle of two neighbouring f32)"""
    f = np.float32(g)
    mids = [(float(f) + float(np.nextafter(f, np.float32(s)))) / 2.0 for s in (-np.inf, np.inf)]
    return min(abs(g - m) for m in mids) / abs(g)
