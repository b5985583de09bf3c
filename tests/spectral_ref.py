"""The spectral distances of include/swc_spectral.h (multi-scale mel, multi-resolution STFT, log-spectral distance) restated
in float64 numpy from the header's text: THE reference of tests/test_spectral_cpu.py and tests/test_spectral_gpu.py.  Nothing
here imports the package.  Dense DFT matrices: small, and slow is fine.

spectral(x, y, sample_rate, scales=None, dtype=np.float64) -> dict(mel, stft, lsd, parts [S][4], clamped, T).  dtype=np.float32
runs the same steps in float32 (window, DFT matrices and mel weights rounded once, every product and sum in float32): the
measure of how well an input is conditioned for ANY float32 implementation, not a model of the kernel."""
import math

import numpy as np

import stoi_ref

MEL, STFT, LSD = 1, 2, 4
WINDOWS = (32, 64, 128, 256, 512, 1024, 2048)
MELS = (5, 10, 20, 40, 80, 160, 320)
CLAMP = 1e-5
RATES = (8000, 16000, 24000, 48000)


def default_scales():
    """[(W, n_mels, flags)]: every window flagged MEL, STFT on 512 and 2048, LSD on 2048"""
    return [(W, M, MEL | (STFT if W in (512, 2048) else 0) | (LSD if W == 2048 else 0)) for W, M in zip(WINDOWS, MELS)]


def window(W):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / W)


_DFT = {}


def dft(W):
    """-> (cos, sin) [W][F] float64 of 2 pi f i / W"""
    if W not in _DFT:
        a = 2.0 * np.pi * ((np.arange(W)[:, None] * np.arange(W // 2 + 1)[None, :]) % W) / W
        _DFT[W] = (np.cos(a), np.sin(a))
    return _DFT[W]


def frames(x, W, dtype=np.float64):
    """-> [T][W]: frame t = w[i] x[t H - W / 2 + i], zero outside [0, n), T = 1 + n // H"""
    x = np.asarray(x, dtype=dtype)
    n, H = len(x), W // 4
    T = 1 + n // H
    pad = np.concatenate([np.zeros(W // 2, dtype), x, np.zeros(W, dtype)])
    idx = np.arange(T)[:, None] * H + np.arange(W)[None, :]
    return pad[idx] * window(W).astype(dtype)[None, :]


def stft_complex(x, W, dtype=np.float64):
    c, s = dft(W)
    v = frames(x, W, dtype)
    return v @ c.astype(dtype), -(v @ s.astype(dtype))


def stft_mag(x, W, dtype=np.float64):
    re, im = stft_complex(x, W, dtype)
    return np.sqrt(re * re + im * im)


def hz_of_mel(m):
    return m * (200.0 / 3.0) if m < 15.0 else 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0))


def mel_of_hz(f):
    return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


_FB = {}


def mel_filterbank(sample_rate, W, n_mels):
    """-> float64 [n_mels][F], one filter and one bin at a time"""
    key = (int(sample_rate), W, n_mels)
    if key not in _FB:
        top = mel_of_hz(sample_rate / 2.0)
        edge = [hz_of_mel(top * k / (n_mels + 1)) for k in range(n_mels + 2)]
        edge[0], edge[-1] = 0.0, sample_rate / 2.0              # the end points as given
        fb = np.zeros((n_mels, W // 2 + 1))
        for m in range(n_mels):
            lo, mid, hi = edge[m], edge[m + 1], edge[m + 2]
            for f in range(W // 2 + 1):
                hz = f * sample_rate / W
                fb[m, f] = max(0.0, min((hz - lo) / (mid - lo), (hi - hz) / (hi - mid))) * 2.0 / (hi - lo)
        _FB[key] = fb
    return _FB[key]


def _c(v, dtype):
    return np.where(v < dtype(CLAMP), dtype(CLAMP), v)      # a NaN stays a NaN


def spectral(x, y, sample_rate, scales=None, dtype=np.float64, banks=None):
    """banks: {scale index: dense bank} to use instead of mel_filterbank (a test's own table)"""
    scales = default_scales() if scales is None else scales
    n = min(len(x), len(y))
    S = len(scales)
    parts = np.zeros((S, 4))
    res = dict(mel=0.0, stft=0.0, lsd=0.0, parts=parts, clamped=0, T=[])
    if n <= 0:
        for s, (_, _, fl) in enumerate(scales):
            parts[s] = [math.nan if fl & MEL else 0.0, math.nan if fl & STFT else 0.0, math.nan if fl & STFT else 0.0,
                        math.nan if fl & LSD else 0.0]
        res.update(mel=math.nan, stft=math.nan, lsd=math.nan)
        return res
    x, y = np.asarray(x[:n], dtype=dtype), np.asarray(y[:n], dtype=dtype)
    two = dtype(2.0)
    for s, (W, M, fl) in enumerate(scales):
        if not fl:
            res["T"].append(1 + n // (W // 4))
            continue
        X, Y = stft_mag(x, W, dtype), stft_mag(y, W, dtype)
        T, F = X.shape
        res["T"].append(T)
        if fl & MEL:
            fb = (mel_filterbank(sample_rate, W, M) if banks is None or s not in banks else banks[s])
            fb = fb.astype(np.float32).astype(dtype)
            Mx, My = X @ fb.T, Y @ fb.T
            res["clamped"] += int((Mx < CLAMP).sum() + (My < CLAMP).sum())
            parts[s, 0] = float(np.abs(np.log10(_c(Mx, dtype)) - np.log10(_c(My, dtype))).sum(dtype=dtype) / dtype(T * M))
            res["mel"] += parts[s, 0]
        if fl & (STFT | LSD):
            res["clamped"] += int((X < CLAMP).sum() + (Y < CLAMP).sum())
            d = two * np.log10(_c(X, dtype)) - two * np.log10(_c(Y, dtype))
            if fl & STFT:
                parts[s, 1] = float(np.abs(d).sum(dtype=dtype) / dtype(T * F))
                parts[s, 2] = float(np.abs(X - Y).sum(dtype=dtype) / dtype(T * F))
                res["stft"] += parts[s, 1] + parts[s, 2]
            if fl & LSD:
                parts[s, 3] = float(np.sqrt((d * d).sum(axis=1, dtype=dtype) / dtype(F)).sum(dtype=dtype) / dtype(T))
                res["lsd"] = parts[s, 3]
    return res


def white(n, sigma=0.1, seed=0):
    return (sigma * np.random.default_rng(4000 + seed).standard_normal(n)).astype(np.float32)


def pair(n, fs, snr, seed=0):
    x = stoi_ref.harmonic(n, fs, seed)
    return x, stoi_ref.add_noise(x, snr, seed)


VALUE_LENGTHS = (1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 8191, 8192, 8193)   # 8192 = R_W H for every W
CONDITION_LENGTHS = (1, 7, 8, 2047, 2048, 18000)


def case_table():
    """name -> (sample_rate, x, y): the cases whose float32 restatement must lie within 1e-5 relative of float64"""
    cases = {}
    for snr in (40, 20, 0):
        for k, n in enumerate(CONDITION_LENGTHS):
            # 40 dB at n = 1, 7, 8 failed the condition and is replaced by 10 dB (tests/test_spectral_cpu.py says why)
            snr_n = 10 if (snr == 40 and n <= 8) else snr
            cases[f"harmonic_{snr_n}dB_{n}"] = (16000,) + pair(n, 16000, snr_n, seed=k % 3)
    for fs in (8000, 16000):
        x = white(6000, seed=fs // 8000)
        cases[f"white_x10_{fs}"] = (fs, x, (10.0 * x.astype(np.float64)).astype(np.float32))
    return cases
