"""swc_cepstra of include/swc_mcd.h restated in float64, and the chain up to the mel-cepstral distortion in dB: THE reference of
tests/test_mcd_cpu.py and tests/test_mcd_gpu.py.  Nothing here imports the package: the tables (the packed mel bank and the
DCT rows, as the kernel gets them: f32) are arguments.

    cep = cepstra(x, W, H, bank, dct)      x f32 [n] -> float64 [T][K], T = 1 + n // H (0 rows for an empty x)
"""
import math

import numpy as np

CLAMP = 1e-5
MCD_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)


def dense_bank(first, count, off, w, F):
    """the packed bank as float64 [M][F], every filter's range cut into [0, F) and into the weight array, as the kernel cuts it"""
    fb = np.zeros((len(first), F), np.float64)
    for m, (a, c, o) in enumerate(zip(first, count, off)):
        for f in range(max(int(a), 0), min(int(a) + int(c), F)):
            wi = int(o) + f - int(a)
            if 0 <= wi < len(w):
                fb[m, f] = np.float64(w[wi])
    return fb


def frames(x, W, H):
    """float64 [T][W]: frame t = w[i] x[t H - W / 2 + i], zero outside [0, n), periodic Hann"""
    x = np.asarray(x, np.float32).astype(np.float64)
    n = len(x)
    if n == 0:
        return np.zeros((0, W))
    T = 1 + n // H
    idx = np.arange(T)[:, None] * H - W // 2 + np.arange(W)[None, :]
    ok = (idx >= 0) & (idx < n)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / W)
    return np.where(ok, x[np.clip(idx, 0, n - 1)], 0.0) * win[None, :]


def cepstra(x, W, H, bank, dct):
    """bank float64 [M][W / 2 + 1] (dense_bank), dct [K][M] -> float64 [T][K]"""
    v = frames(x, W, H)
    if len(v) == 0:
        return np.zeros((0, len(dct)))
    X = np.abs(np.fft.rfft(v, axis=1))
    A = X @ np.asarray(bank, np.float64).T
    L = np.log(np.where(A < CLAMP, CLAMP, A))       # a NaN stays a NaN
    return L @ np.asarray(dct, np.float64).T


def mcd_float64(cx, cy, path):
    """the all-float64 distortion in dB along a path [N][2]: (10 sqrt 2 / ln 10) mean_k |cx[i_k] - cy[j_k]|"""
    d = cx[path[:, 0]] - cy[path[:, 1]]
    return MCD_DB * float(np.sqrt((d * d).sum(1)).mean())


def dtw_float64(cx, cy):
    """the recurrence of include/swc_mcd.h on float64 Euclidean distances, no band -> (total, N): smallest total, then smallest
    N, then the diagonal, (i-1, j), (i, j-1); one anti-diagonal at a time"""
    Tx, Ty = len(cx), len(cy)
    d = np.sqrt(((cx[:, None, :] - cy[None, :, :]) ** 2).sum(2))
    C = np.full((Tx + 1, Ty + 1), np.inf)
    N = np.zeros((Tx + 1, Ty + 1), np.int64)
    for s in range(Tx + Ty - 1):
        i = np.arange(max(0, s - Ty + 1), min(Tx - 1, s) + 1)
        j = s - i
        bc, bn = C[i, j].copy(), N[i, j].copy()
        for pc, pn in ((C[i, j + 1], N[i, j + 1]), (C[i + 1, j], N[i + 1, j])):
            m = (pc < bc) | ((pc == bc) & (pn < bn))
            bc[m], bn[m] = pc[m], pn[m]
        if s == 0:
            bc[:], bn[:] = 0.0, 0
        C[i + 1, j + 1], N[i + 1, j + 1] = bc + d[i, j], bn + 1
    return float(C[-1, -1]), int(N[-1, -1])
