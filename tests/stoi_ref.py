"""STOI (Taal et al. 2011, the non-extended form) restated in float64 numpy from the contract in include/swc_metrics.h /
DESIGN.md "STOI": THE reference of tests/test_stoi_cpu.py and tests/test_stoi_gpu.py.  Nothing here imports the package.

stoi(x, y, fs) -> dict(d, segs, kept = indices of the frames that survive silent-frame removal, margin = the smallest
distance in dB of a frame energy from the removal threshold max - 40)."""
import math

import numpy as np

FS, FRAME, HOP, NFFT, J, N, BETA, DYN = 10000, 256, 128, 512, 15, 30, -15.0, 40.0
EPS = 2.0 ** -52
SHORT_D = 1e-5
MARGIN_DB = 0.05          # every test signal keeps its frame energies at least this far from the threshold
SNRS = (40, 20, 10, 0, -10)

WINDOW = np.hanning(FRAME + 2)[1:-1]


def resample_filter(fs):
    """-> (h float64 [2L + 1], p, q): step 1 of the contract (h already normalised to sum 1)"""
    g = math.gcd(FS, int(fs))
    p, q = FS // g, int(fs) // g
    fc = 1.0 / (2 * max(p, q))
    L = int(math.ceil(52.0 / (28.714 * fc / 10.0)))
    t = np.arange(-L, L + 1, dtype=np.float64)
    h = 2 * p * fc * np.sinc(2 * fc * t) * np.kaiser(2 * L + 1, 0.1102 * (60 - 8.7))
    return h / h.sum(), p, q


def resample(x, fs):
    """x10[k] = p sum_j h[k q - j p + L] x[j], k in [0, ceil(n p / q))"""
    x = np.asarray(x, dtype=np.float64)
    if int(fs) == FS:
        return x.copy()
    h, p, q = resample_filter(fs)
    L = (len(h) - 1) // 2
    n = len(x)
    n_out = -(-n * p // q)
    up = np.zeros(n * p + 2 * L + q)           # up[L + j p] = x[j]; out[k] = p sum_i h[i] up[k q + 2 L - i] ...
    up[L + np.arange(n) * p] = x
    full = np.convolve(up, h)                  # full[m] = sum_i h[i] up[m - i];  want index k q - j p + L = i  ->  m = k q + 2 L
    return p * full[2 * L + np.arange(n_out) * q]


def band_edges():
    """bins [lo_j, hi_j) of the 15 one-third octave bands as 16 edges"""
    f = np.arange(NFFT // 2 + 1) * (FS / NFFT)
    k = np.arange(J, dtype=np.float64)
    cf = 150.0 * 2.0 ** (k / 3.0)
    lo = np.array([int(np.argmin((f - c * 2.0 ** (-1.0 / 6.0)) ** 2)) for c in cf])
    hi = np.array([int(np.argmin((f - c * 2.0 ** (1.0 / 6.0)) ** 2)) for c in cf])
    assert (lo[1:] == hi[:-1]).all()
    return [int(v) for v in lo] + [int(hi[-1])]


EDGES = band_edges()


def frame_energies(x10):
    starts = range(0, len(x10) - FRAME + 1, HOP)
    return np.array([20.0 * np.log10(np.linalg.norm(WINDOW * x10[s:s + FRAME]) + EPS) for s in starts])


def remove_silent(x10, y10):
    """-> (xs, ys, kept, margin)"""
    e = frame_energies(x10)
    if len(e) == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int64), math.inf
    gap = e.max() - DYN - e
    kept = np.nonzero(gap < 0)[0]
    margin = float(np.abs(gap).min())
    K = len(kept)
    xs, ys = np.zeros((K - 1) * HOP + FRAME), np.zeros((K - 1) * HOP + FRAME)
    for c, f in enumerate(kept):
        xs[c * HOP:c * HOP + FRAME] += WINDOW * x10[f * HOP:f * HOP + FRAME]
        ys[c * HOP:c * HOP + FRAME] += WINDOW * y10[f * HOP:f * HOP + FRAME]
    return xs, ys, kept, margin


def band_spectra(s):
    """-> Xt [J, M], M frames starting at 0, 128, ... < len - 256"""
    starts = list(range(0, len(s) - FRAME, HOP))
    if not starts:
        return np.zeros((J, 0))
    fr = np.stack([WINDOW * s[a:a + FRAME] for a in starts])
    P = np.abs(np.fft.rfft(fr, n=NFFT, axis=1)) ** 2           # [M, 257]
    return np.stack([np.sqrt(P[:, EDGES[j]:EDGES[j + 1]].sum(axis=1)) for j in range(J)])


def stoi(x, y, fs):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = min(len(x), len(y))
    short = dict(d=SHORT_D, segs=0, kept=np.zeros(0, dtype=np.int64), margin=math.inf)
    if n <= 0:
        return short
    x10, y10 = resample(x[:n], fs), resample(y[:n], fs)
    xs, ys, kept, margin = remove_silent(x10, y10)
    short.update(kept=kept, margin=margin)
    if len(kept) <= 1:
        return short
    Xt, Yt = band_spectra(xs), band_spectra(ys)
    M = Xt.shape[1]
    assert M == len(kept) - 1
    if M < N:
        return short
    clip = 1.0 + 10.0 ** (-BETA / 20.0)
    total = 0.0
    S = M - N + 1
    for m in range(N, M + 1):
        a, b = Xt[:, m - N:m], Yt[:, m - N:m]
        b = b * (np.linalg.norm(a, axis=1, keepdims=True) / (np.linalg.norm(b, axis=1, keepdims=True) + EPS))
        b = np.minimum(b, a * clip)
        a = a - a.mean(axis=1, keepdims=True)
        b = b - b.mean(axis=1, keepdims=True)
        a = a / (np.linalg.norm(a, axis=1, keepdims=True) + EPS)
        b = b / (np.linalg.norm(b, axis=1, keepdims=True) + EPS)
        total += float((a * b).sum())
    return dict(d=total / (J * S), segs=S, kept=kept, margin=margin)


def frames_at_10k(n, fs):
    """M (STFT frames) of a row of n samples at fs when no frame is removed"""
    g = math.gcd(FS, int(fs))
    n10 = -(-n * (FS // g) // (int(fs) // g))
    F = (n10 - FRAME) // HOP + 1 if n10 >= FRAME else 0
    return max(F - 1, 0)


def boundary_lengths(fs):
    """(n29, n30): the longest length with M = 29 and the shortest with M = 30, found by search"""
    n = 1
    while frames_at_10k(n, fs) < N:
        n += 1
    assert frames_at_10k(n - 1, fs) == N - 1 and frames_at_10k(n, fs) == N
    return n - 1, n


BAND_RANGE_DB = 45.0      # every test signal keeps each band of the clean side within this of its strongest band


def harmonic(n, fs, seed=0):
    """the clean test signal: the harmonics of a slowly gliding pitch up to the top band, under a syllable-rate envelope, over
    a weak broadband floor (-30 dB: breath noise), float32 in (-1, 1).
    Loud everywhere (the envelope never falls below 0.35): no frame comes near the -40 dB removal threshold.
    Full-band on purpose: STOI normalises every band by its own norm, while an f32 resampler and an f32 DFT err relative to
    the level of the whole frame (2^-24 = -144 dB per operation, times the square root of a few hundred terms).  A band that
    is empty in the clean signal (a harmonic series stopped at 2.7 kHz leaves the top band 80 dB under the others) turns that
    floor into a 1e-3 error of the band and 1e-5 of d in ANY f32 implementation; band_range_db() states the condition and the
    tests assert it about their inputs."""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(n) / float(fs)
    f0 = 110.0 + 25.0 * seed + 20.0 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / float(fs)
    x = np.zeros(n)
    k = 1
    while k * f0.max() < 0.46 * min(fs, FS):
        x += np.sin(k * ph + rng.uniform(0, 2 * np.pi)) / k ** 0.8
        k += 1
    env = 0.35 + 0.65 * (0.5 + 0.5 * np.sin(2 * np.pi * 3.1 * t + seed)) ** 2
    x = x * env
    floor = rng.standard_normal(n)
    x = x + floor * (np.sqrt((x ** 2).mean() / (floor ** 2).mean()) * 10.0 ** (-30.0 / 20.0))
    return (0.5 * x / np.abs(x).max()).astype(np.float32)


def band_range_db(x, fs):
    """level of the strongest band over the weakest, in dB, of the clean signal's band spectra (silent frames removed)"""
    x10 = resample(x, fs)
    xs, _, kept, _ = remove_silent(x10, x10)
    if len(kept) <= 1:
        return 0.0
    lev = 20.0 * np.log10(np.sqrt((band_spectra(xs) ** 2).mean(axis=1)) + EPS)
    return float(lev.max() - lev.min())


def add_noise(x, snr_db, seed=0):
    rng = np.random.default_rng(2000 + seed)
    nz = rng.standard_normal(len(x))
    x64 = x.astype(np.float64)
    nz *= np.sqrt((x64 ** 2).mean() / (nz ** 2).mean()) * 10.0 ** (-snr_db / 20.0)
    return np.clip(x64 + nz, -1.0, 1.0).astype(np.float32)


def with_gaps(x, fs, gaps):
    """exact zeros over the [start, stop) second spans of `gaps`"""
    x = x.copy()
    for a, b in gaps:
        x[int(a * fs):int(b * fs)] = 0.0
    return x
