"""ESTOI (Jensen and Taal 2016) and SI-SDR (Le Roux et al. 2019) restated in float64 numpy from the contract in
include/swc_quality.h: THE reference of tests/test_quality_cpu.py and tests/test_quality_gpu.py.  Steps 1 - 3 of ESTOI (10 kHz,
silent-frame removal, band spectra) and the test signals are those of tests/stoi_ref.py.  Nothing here imports the package.

estoi(x, y, fs) -> dict(d, segs, kept, margin as stoi_ref.stoi gives them, min_col_norm = the smallest norm a frame column is
divided by in step 4b, over both signals, all segments and all frames; inf without a segment).
si_sdr(x, y) -> dB, NaN for an empty pair."""
import math

import numpy as np

import stoi_ref
from stoi_ref import EPS, J, N, SHORT_D


def _normalise(a, axis):
    """minus the mean along `axis`, over (the norm along it + EPS) -> (result, the norms)"""
    a = a - a.mean(axis=axis, keepdims=True)
    nrm = np.linalg.norm(a, axis=axis, keepdims=True)
    return a / (nrm + EPS), nrm


def estoi(x, y, fs):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = min(len(x), len(y))
    short = dict(d=SHORT_D, segs=0, kept=np.zeros(0, dtype=np.int64), margin=math.inf, min_col_norm=math.inf)
    if n <= 0:
        return short
    x10, y10 = stoi_ref.resample(x[:n], fs), stoi_ref.resample(y[:n], fs)
    xs, ys, kept, margin = stoi_ref.remove_silent(x10, y10)
    short.update(kept=kept, margin=margin)
    if len(kept) <= 1:
        return short
    Xt, Yt = stoi_ref.band_spectra(xs), stoi_ref.band_spectra(ys)
    M = Xt.shape[1]
    assert M == len(kept) - 1 and Xt.shape[0] == J
    if M < N:
        return short
    S = M - N + 1
    total, smallest = 0.0, math.inf
    for m in range(N, M + 1):
        a, _ = _normalise(Xt[:, m - N:m], axis=1)        # 4a: band rows over the 30 frames
        b, _ = _normalise(Yt[:, m - N:m], axis=1)
        a, na = _normalise(a, axis=0)                    # 4b: frame columns over the 15 bands
        b, nb = _normalise(b, axis=0)
        smallest = min(smallest, float(na.min()), float(nb.min()))
        total += float((a * b).sum()) / N                # 4c
    return dict(d=total / S, segs=S, kept=kept, margin=margin, min_col_norm=smallest)


def si_sdr(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = min(len(x), len(y))
    if n <= 0:
        return math.nan
    xc, yc = x[:n] - x[:n].mean(), y[:n] - y[:n].mean()
    alpha = float(xc @ yc) / (float(xc @ xc) + EPS)
    t = alpha * xc
    e = yc - t
    return 10.0 * math.log10((float(t @ t) + EPS) / (float(e @ e) + EPS))
