"""Test infrastructure: the case table of the FLAC encoder tests (include/swc_flac_enc.h).  Seeded int16 signals, each built
to force one choice of the exhaustive search; tests/test_flac_enc_cpu.py asserts on the reference's plans that the table
covers CONSTANT, VERBATIM, FIXED of every order 0-4, every partition order 0-6, Rice parameter 0 and one >= 12, and a tie
taken by the smaller order, so the table cannot thin out silently.  The GPU tests encode the same signals."""
import functools

import numpy as np

BLOCK_SIZES = (256, 512, 1024, 2048, 4096)
LENGTHS = (1, 2, 4, 5, 27, 28, 31, 32, 255, 256, 257)   # + BS and BS + 1; 27/28 and 31/32: the MD5 padding boundaries


def _rng(seed):
    return np.random.default_rng(seed)


def noise(n, amp, seed):
    return _rng(seed).integers(-amp, amp + 1, n).astype(np.int16)


def stepped_noise(bs, porder, seed, amps=(3, 2500)):
    """noise whose level changes every bs >> porder samples: partitions of exactly that length pay"""
    seg = bs >> porder
    level = np.where((np.arange(bs) // seg) % 2 == 0, amps[0], amps[1])
    return np.round(_rng(seed).uniform(-1, 1, bs) * level).astype(np.int16)


def sine(n, amp, omega, seed=None, jitter=0):
    x = amp * np.sin(omega * np.arange(n) + 0.3)
    if jitter:
        x = x + _rng(seed).integers(-jitter, jitter + 1, n)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def ramp(n, step=3, start=-200):
    return (start + step * np.arange(n)).astype(np.int16)


def alternation(n):
    """+ / - full scale: nothing predicts it, no Rice parameter below 15 pays -> VERBATIM"""
    return np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)


def speech_like(n, seed):
    """a modulated tone with noise and clipped samples (several blocks)"""
    t = np.arange(n)
    x = 9000 * np.sin(0.031 * t) * (0.6 + 0.4 * np.sin(0.0007 * t)) + 2500 * np.sin(0.27 * t + 1.0)
    x = x + _rng(seed).normal(0, 120, n)
    x[n // 3: n // 3 + 40] *= 8
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def coverage_cases():
    """name -> (samples, blocksize): the signals that make the search take every branch"""
    c = {}
    c["constant_zero"] = (np.zeros(256, dtype=np.int16), 256)
    c["constant_min"] = (np.full(300, -32768, dtype=np.int16), 256)
    c["constant_but_last"] = (np.concatenate([np.full(255, 77), [78]]).astype(np.int16), 256)
    c["alternation"] = (alternation(256), 256)
    c["ramp"] = (ramp(256), 256)                                   # order 2 leaves zeros: Rice parameter 0
    c["noise_loud"] = (noise(256, 6000, 1), 256)                   # order 0, parameter 12
    c["walk"] = (np.cumsum(noise(256, 40, 2)).astype(np.int16), 256)
    c["sine_slow"] = (sine(512, 30000, 0.01), 512)
    c["sine_mid"] = (sine(512, 30000, 0.05), 512)
    c["sine_fast"] = (sine(512, 30000, 0.2), 512)
    c["sine_jitter"] = (sine(1024, 12000, 0.02, seed=3, jitter=6), 1024)
    for p in range(7):
        bs = (256, 512, 1024, 2048, 4096, 256, 4096)[p]
        c[f"stepped_p{p}"] = (stepped_noise(bs, p, 10 + p), bs)
    c["stepped_p6_short"] = (stepped_noise(192, 6, 20), 256)       # a short block, 64 partitions of 3
    # orders 0 and 1 cost the same number of bits here (found by search over seeded random blocks): order 0 is taken
    c["tie"] = (np.array([4, -3, -10, -20, -19, -10, 0, -5, 10, 6, 13, 13, -8, -17, -18, -14, -10, -11, -1, -9], dtype=np.int16), 256)
    c["speech"] = (speech_like(2 * 1024 + 333, 4), 1024)
    return c


def length_cases(blocksize, seed=0):
    """the issue's lengths for one block size: name -> samples"""
    out = {}
    for n in LENGTHS + (blocksize, blocksize + 1):
        out[f"n{n}"] = speech_like(n, seed + n)
    return out


def plan_summary(plans):
    """what the coverage assertion looks at"""
    kinds = {p["kind"] for p in plans}
    fixed = [p for p in plans if p["kind"] == "fixed"]
    return dict(kinds=kinds, orders={p["order"] for p in fixed}, porders={p["porder"] for p in fixed},
                ks={k for p in fixed for k in p["ks"]},
                ties_to_smaller_order=sum(1 for p in fixed if any(o > p["order"] for o, _ in p["tied"])))
