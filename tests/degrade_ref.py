"""include/swc_degrade.h restated in numpy from the header's text alone: Philox4x32-10 and the noise sample, the mixing gain and
the fused multiply-add, the convolution by definition in float64, and the header's partitioned overlap-save method in complex64 /
float32 (whose distance from the float64 definition sets the tolerance of the device test)."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
N = 1024   # SWC_CONV_BLOCK
MAX_TAPS = 131072
UNMIXED, OVER = 1, 2


def philox4x32_10(counter, key):
    """-> the four output words of one block (plain Python integers)"""
    c0, c1, c2, c3 = (int(v) & MASK for v in counter)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def noise_v(seed, stream_id, j):
    """V of sample j: 2 h - 8 * 65535 with h the sum of the eight 16-bit halves"""
    seed, s, j = int(seed) & (2**64 - 1), int(stream_id) & (2**64 - 1), int(j) & (2**64 - 1)
    w = philox4x32_10((j & MASK, j >> 32, s & MASK, s >> 32), (seed & MASK, seed >> 32))
    h = sum((x & 0xFFFF) + (x >> 16) for x in w)
    return 2 * h - 8 * 65535


def _philox_vec(j, s, seed):
    """the same over a numpy array of uint64 indices j -> int64 V"""
    j = np.asarray(j, dtype=np.uint64)
    c0, c1 = j & np.uint64(MASK), j >> np.uint64(32)
    c2 = np.full_like(j, int(s) & MASK)
    c3 = np.full_like(j, (int(s) & (2**64 - 1)) >> 32)
    k0, k1 = int(seed) & MASK, (int(seed) & (2**64 - 1)) >> 32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & np.uint64(MASK), (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), \
            p0 & np.uint64(MASK)
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    h = np.zeros(j.shape, dtype=np.int64)
    for c in (c0, c1, c2, c3):
        h += (c & np.uint64(0xFFFF)).astype(np.int64) + (c >> np.uint64(16)).astype(np.int64)
    return 2 * h - 8 * 65535


def noise(seed, stream_id, n, first=0):
    """f32 [n]: samples first .. first + n - 1 of the stream"""
    if n <= 0:
        return np.zeros(0, dtype=np.float32)
    v = _philox_vec(np.arange(first, first + n, dtype=np.uint64), stream_id, seed)
    return (v.astype(np.float64) * 2.0 ** -19).astype(np.float32)   # exact: |V| < 2^20


def noise_batch(seed, stream_ids, lengths, cols, first=0):
    out = np.zeros((len(lengths), cols), dtype=np.float32)
    for b, (s, n) in enumerate(zip(stream_ids, lengths)):
        k = min(max(int(n), 0), cols)
        out[b, :k] = noise(seed, s, k, first)
    return out


def gain(lx, ln, snr, m):
    """-> (g as np.float32, mixed)"""
    if not (math.isfinite(lx) and math.isfinite(ln) and math.isfinite(snr)) or m <= 0:
        return np.float32(0.0), False
    with np.errstate(over="ignore"):
        return np.float32(np.float64(10.0) ** np.float64((lx - ln - snr) / 20.0)), True


def fmaf(a, b, c):
    """one f32 fused multiply-add of finite f32 arrays.  The product of two f32 is exact in float64; where the float64 sum is
    exact too (TwoSum says so), its rounding to f32 is the fused result.  The remaining elements (a double rounding could
    land on the wrong side of a tie) are redone in rationals"""
    from fractions import Fraction
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    r = s.astype(np.float32)
    for i in np.flatnonzero(err != 0):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = np.float32(s[i])
        cands = [near, np.nextafter(near, np.float32(-np.inf)), np.nextafter(near, np.float32(np.inf))]
        # nearest, ties to the even mantissa
        r[i] = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
    return r


def mix(x, v, g, mixed):
    """out = fmaf(v[i mod m], g, x[i]) (or x where not mixed) -> (out f32, flag)"""
    x = np.asarray(x, dtype=np.float32)
    if not mixed:
        out = x.copy()
    else:
        idx = np.arange(len(x)) % len(v)
        out = fmaf(np.asarray(v, dtype=np.float32)[idx], np.full(len(x), g, dtype=np.float32), x)
    with np.errstate(invalid="ignore"):
        over = bool((np.abs(out) > 1).any())
    return out, (0 if mixed else UNMIXED) | (OVER if over else 0)


def convolve64(x, h, d, extra, cols=None):
    """the definition in float64: y[i] = sum_k h[k] x[i + d - k], 0 <= i < min(n + extra, cols)"""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    n = len(x)
    length = n + extra if cols is None else min(n + extra, cols)
    if n == 0 or length <= 0:
        return np.zeros(max(length, 0))
    full = np.convolve(x, h)                       # full[t] = sum_k h[k] x[t - k], t < n + L - 1
    full = np.concatenate([full, np.zeros(max(0, d + length - len(full)))])
    return full[d:d + length]


def _twiddles():
    q = np.arange(N, dtype=np.float64)
    return (np.cos(-np.pi * q / N) + 1j * np.sin(-np.pi * q / N)).astype(np.complex64)


def _network(z, tw, inverse):
    """radix-2 decimation in time over N complex64 points: bit-reversed input, natural output"""
    logn = N.bit_length() - 1
    rev = np.array([int(format(k, f"0{logn}b")[::-1], 2) for k in range(N)])
    a = np.empty(N, dtype=np.complex64)
    a[rev] = z
    for lh in range(logn):
        h = 1 << lh
        a = a.reshape(-1, 2, h)
        w = tw[(np.arange(h) << (logn - lh))]
        if inverse:
            w = np.conj(w)
        t = (w[None, :] * a[:, 1, :]).astype(np.complex64)
        a = np.stack([a[:, 0, :] + t, a[:, 0, :] - t], axis=1).astype(np.complex64).reshape(-1)
    return a


def _forward(v, tw):
    """2 N real f32 samples -> N packed complex64 bins (Nyquist beside DC)"""
    v = np.asarray(v, dtype=np.float32)
    Z = _network((v[0::2] + 1j * v[1::2]).astype(np.complex64), tw, False)
    Bc = np.conj(Z[(N - np.arange(N)) % N])
    E = (np.complex64(0.5) * (Z + Bc)).astype(np.complex64)
    O = (np.complex64(-0.5j) * (Z - Bc)).astype(np.complex64)
    S = (E + tw * O).astype(np.complex64)
    S[0] = np.complex64(complex(np.float32(Z[0].real + Z[0].imag), np.float32(Z[0].real - Z[0].imag)))
    return S


def _inverse(Y, tw):
    """N packed complex64 bins -> 2 N real f32 samples"""
    Bc = np.conj(Y[(N - np.arange(N)) % N])
    E, P = (Y + Bc).astype(np.complex64), (Y - Bc).astype(np.complex64)
    O = (np.conj(tw) * P).astype(np.complex64)
    Z = (E + np.complex64(1j) * O).astype(np.complex64)
    Z[0] = np.complex64(complex(np.float32(Y[0].real + Y[0].imag), np.float32(Y[0].real - Y[0].imag)))
    z = _network(Z, tw, True)
    v = np.empty(2 * N, dtype=np.float32)
    v[0::2], v[1::2] = z.real, z.imag
    return v * np.float32(1.0 / (2 * N))


def convolve_partitioned(x, h, d, extra, cols=None):
    """the header's method, in complex64 / float32 -> f32 [min(n + extra, cols)]"""
    x, h = np.asarray(x, dtype=np.float32), np.asarray(h, dtype=np.float32)
    n, L = len(x), len(h)
    length = n + extra if cols is None else min(n + extra, cols)
    out = np.zeros(max(length, 0), dtype=np.float32)
    if length <= 0:
        return out
    tw = _twiddles()
    P = (L + N - 1) // N
    H = []
    for p in range(P):
        part = np.zeros(2 * N, dtype=np.float32)
        seg = h[N * p:N * p + N]
        part[:len(seg)] = seg
        H.append(_forward(part, tw))

    def sample(i):
        return x[i] if 0 <= i < n else np.float32(0)

    X = {}
    for j in range((length + N - 1) // N):
        Y = np.zeros(N, dtype=np.complex64)
        for p in range(P):
            w = j - p
            if n == 0 or N * (w + 1) + d <= 0 or N * (w - 1) + d >= n:
                continue
            if w not in X:
                s0 = N * (w - 1) + d
                lo, hi = max(s0, 0), min(s0 + 2 * N, n)
                win = np.zeros(2 * N, dtype=np.float32)
                win[lo - s0:hi - s0] = x[lo:hi]
                X[w] = _forward(win, tw)
            prod = (X[w] * H[p]).astype(np.complex64)
            prod[0] = np.complex64(complex(np.float32(X[w][0].real * H[p][0].real), np.float32(X[w][0].imag * H[p][0].imag)))
            Y = (Y + prod).astype(np.complex64)
        v = _inverse(Y, tw)
        k = min(N, length - N * j)
        out[N * j:N * j + k] = v[N:N + k]
    return out


def workspace_bytes(B, max_n, R, max_L):
    return 8 * N * (B * ((max_n + N - 1) // N + 2) + R * ((max_L + N - 1) // N))
