"""float64 numpy restatement of include/swc_segmental.h, written from the header's text: LLR, Itakura-Saito, LPC cepstral
distance, segmental SNR and frequency-weighted segmental SNR of one pair.  Sums whose order the header fixes are formed in that
order (np.add.accumulate is sequential); the band energies come from a float64 FFT where the device runs an f32 one, which is
the one deliberate difference (the tolerance of fwsegsnr in tests/test_segmental_gpu.py measures it).  Vectorised over the
frames of a row, never over the steps of a recursion."""
import math

import numpy as np

CORR = 1.0 + 2.0 ** -20
DB = 4.342944819032518                       # 10 / ln 10, the header's literal
VALUES = ("llr", "is", "cd", "segsnr", "fwsegsnr", "frames", "frames_lpc", "frames_fw")


def frames(n, W):
    return 1 + (n - W) // (W // 4) if n >= W else 0


def window(W):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W, dtype=np.float64) / W)).astype(np.float32)


def workspace_bytes(B, max_n, W, P):
    up = lambda v: (v + 255) & ~255
    T = frames(max_n, W)
    return up(B * T * (2 * (P + 1) + 2) * 8) + up(B * T * 5 * 8)


def k95(T):
    return (19 * T + 10) // 20


def framed(x, W):
    """-> float64 [T][W]: v[t][i] = fl32(w[i] x[t H + i])"""
    x = np.asarray(x, dtype=np.float32)
    T, H = frames(len(x), W), W // 4
    idx = np.arange(T)[:, None] * H + np.arange(W)[None, :]
    return (window(W)[None, :] * x[idx]).astype(np.float64) if T else np.zeros((0, W))


def _seq(a):
    """the sequential sum along the last axis, from 0.0"""
    return np.add.accumulate(a, axis=-1)[..., -1] if a.shape[-1] else np.zeros(a.shape[:-1])


def four_part(terms, W):
    """the header's sum of terms[..., 0 .. L): four parts of W / 4 indices, ((p0 + p1) + p2) + p3"""
    Q, L = W // 4, terms.shape[-1]
    p = [_seq(terms[..., c * Q:min((c + 1) * Q, L)]) for c in range(4)]
    return ((p[0] + p[1]) + p[2]) + p[3]


def autocorr(v, P):
    """-> float64 [T][P + 1], uncorrected"""
    W = v.shape[-1]
    return np.stack([four_part(v[..., :W - k] * v[..., k:], W) for k in range(P + 1)], axis=-1)


def levinson(R, P):
    """R [..., P + 1] (R[0] corrected) -> (a [..., P + 1], E [...]): the header's recursion"""
    R = np.asarray(R, dtype=np.float64)
    a = np.zeros(R.shape[:-1] + (P + 1,))
    a[..., 0] = 1.0
    with np.errstate(all="ignore"):
        E = R[..., 0].copy()
        for m in range(1, P + 1):
            acc = R[..., m].copy()
            for i in range(1, m):
                acc = acc + a[..., i] * R[..., m - i]
            k = -acc / E
            new = [a[..., i] + k * a[..., m - i] for i in range(1, m)]
            for i in range(1, m):
                a[..., i] = new[i - 1]
            a[..., m] = k
            E = E * (1.0 - k * k)
    return a, E


def quad(a, R, P):
    with np.errstate(all="ignore"):
        q = np.zeros(a.shape[:-1])
        for i in range(P + 1):
            s = np.zeros(a.shape[:-1])
            for j in range(P + 1):
                s = s + R[..., abs(i - j)] * a[..., j]
            q = q + a[..., i] * s
    return q


def cepstrum(a, P):
    """c[..., 1 .. P] of the predictor p = -a (c[..., 0] is not used and 0)"""
    c = np.zeros(a.shape)
    with np.errstate(all="ignore"):
        for m in range(1, P + 1):
            acc = -a[..., m]
            for k in range(1, m):
                acc = acc + ((k / m) * c[..., k]) * (-a[..., m - k])
            c[..., m] = acc
    return c


def lo(v, c):
    return np.where(v < c, c, v)


def hi(v, c):
    return np.where(v > c, c, v)


def snr_db(num, den):
    """-10 where num == 0, else 35 where den == 0, else hi(lo(10 log10(num / den), -10), 35); num, den as the header names them"""
    with np.errstate(all="ignore"):
        return np.where(num == 0.0, -10.0, np.where(den == 0.0, 35.0, hi(lo(10.0 * np.log10(num / den), -10.0), 35.0)))


def band_energies(mag, table):
    """mag float64 [T][F] -> float64 [T][K]: the mel_band sums over the packed table, with its two cuts"""
    first, count, off, w = (np.asarray(t) for t in table)
    T, F = mag.shape
    E = np.zeros((T, len(first)))
    for j in range(len(first)):
        a, b = max(int(first[j]), 0), min(int(first[j]) + int(count[j]), F)
        for f in range(a, b):
            wi = int(off[j]) + (f - int(first[j]))
            if 0 <= wi < len(w):
                E[:, j] = E[:, j] + np.float64(w[wi]) * mag[:, f]
    return E


def fw_frames(vx, vy, table):
    """-> (fw float64 [T], kept bool [T])"""
    Ex = band_energies(np.abs(np.fft.rfft(vx, axis=-1)), table)
    Ey = band_energies(np.abs(np.fft.rfft(vy, axis=-1)), table)
    return fw_from_bands(Ex, Ey)


def fw_from_bands(Ex, Ey):
    T, K = Ex.shape
    with np.errstate(all="ignore"):
        emax = np.zeros(T)
        for j in range(K):
            emax = np.where((Ex[:, j] > emax) | np.isnan(Ex[:, j]), Ex[:, j], emax)
        su, sus = np.zeros(T), np.zeros(T)
        for j in range(K):
            ex, d = Ex[:, j], Ex[:, j] - Ey[:, j]
            u = (ex / emax) ** 0.2
            s = np.where(ex == 0.0, -10.0, np.where(d == 0.0, 35.0, hi(lo(10.0 * np.log10((ex * ex) / (d * d)), -10.0), 35.0)))
            su = su + u
            sus = sus + u * (35.0 - s)
        fw = 35.0 - sus / su
    kept = emax != 0.0
    return np.where(kept, fw, np.nan), kept


def select_mean(values):
    """the header's mean of the K95 smallest of `values` (float64, >= 0 or NaN; frame order); NaN for none or with a NaN"""
    v = np.asarray(values, dtype=np.float64)
    if len(v) == 0 or np.isnan(v).any():
        return math.nan
    n = k95(len(v))
    keys = v.view(np.uint64)
    order = np.sort(keys)
    star_key, star = order[n - 1], order[n - 1:n].view(np.float64)[0]
    below = v[keys < star_key]
    return float((_seq(below) + float(n - len(below)) * star) / float(n))


def seq_mean(values):
    v = np.asarray(values, dtype=np.float64)
    return float(_seq(v) / float(len(v))) if len(v) else math.nan


def measure(x, y, W, P, table=None):
    """-> dict: the eight row values by name, "vals" (float64 [8]) and "track" (float64 [T][5], NaN where a frame is left out)"""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    assert len(x) == len(y)
    vx, vy = framed(x, W), framed(y, W)
    T = vx.shape[0]
    track = np.full((T, 5), np.nan)
    if T:
        with np.errstate(all="ignore"):
            Rx, Ry = autocorr(vx, P), autocorr(vy, P)
            S = Rx[:, 0].copy()
            D = four_part((vx - vy) * (vx - vy), W)
            track[:, 3] = snr_db(S, D)
            lpc = (Rx[:, 0] > 0.0) & (Ry[:, 0] > 0.0)
            if lpc.any():
                Rx, Ry = Rx[lpc].copy(), Ry[lpc].copy()
                Rx[:, 0] = Rx[:, 0] * CORR
                Ry[:, 0] = Ry[:, 0] * CORR
                ax, ay = levinson(Rx, P)[0], levinson(Ry, P)[0]
                num, den, gy = quad(ay, Rx, P), quad(ax, Rx, P), quad(ay, Ry, P)
                track[lpc, 0] = hi(lo(np.log(num / den), 0.0), 2.0)
                track[lpc, 1] = hi(((den / gy) * (num / den) + np.log(gy / den)) - 1.0, 100.0)
                cx, cy = cepstrum(ax, P), cepstrum(ay, P)
                acc = np.zeros(len(num))
                for m in range(1, P + 1):
                    d = cx[:, m] - cy[:, m]
                    acc = acc + d * d
                track[lpc, 2] = hi(DB * np.sqrt(2.0 * acc), 10.0)
            if table is not None and len(table[0]):
                fw, kept = fw_frames(vx, vy, table)
                track[:, 4] = fw
            else:
                kept = np.zeros(T, dtype=bool)
    else:
        lpc = kept = np.zeros(0, dtype=bool)
    vals = np.array([select_mean(track[lpc, 0]), seq_mean(track[lpc, 1]), select_mean(track[lpc, 2]), seq_mean(track[:, 3]),
                     seq_mean(track[kept, 4]), float(T), float(lpc.sum()), float(kept.sum())])
    res = dict(zip(VALUES, vals.tolist()))
    res.update(vals=vals, track=track, lpc=lpc, kept=kept)
    return res
