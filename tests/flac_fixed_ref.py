"""Test infrastructure: the FLAC encoder of include/swc_flac_enc.h restated in numpy from that header's contract text alone —
mono int16, block sizes 256 .. 4096, one subframe per frame chosen by exhaustive search over CONSTANT, VERBATIM and every
FIXED (predictor order 0-4, partition order 0-6) candidate with per-partition Rice parameters 0-14.  Exact integers (int64)
throughout.  encode() gives the file's bytes, plans() what was chosen per frame (the CPU tests assert the case table's coverage
on them).  Only the bit helpers come from tests/flac_encode.py."""
import hashlib

import numpy as np

from flac_encode import crc8, crc16, utf8_number  # noqa: F401  (crc16: the tests pin _crc16 below against it)

BLOCK_SIZES = (256, 512, 1024, 2048, 4096)
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
MAX_HEADER = 14
_K = np.arange(15, dtype=np.int64)
_BIG = np.int64(1) << 60

_CRC16_TABLE = []
for _b in range(256):
    _c = _b << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x8005) & 0xFFFF if _c & 0x8000 else (_c << 1) & 0xFFFF
    _CRC16_TABLE.append(_c)


def _crc16(data):
    """flac_encode.crc16, a table step per byte"""
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _CRC16_TABLE[(c >> 8) ^ b]
    return c


def rate_code(rate):
    if rate in RATE_CODES:
        return RATE_CODES[rate]
    if 1 <= rate <= 65535:
        return 13
    raise ValueError(f"rate {rate}")


def _zigzag(e):
    return np.where(e >= 0, 2 * e, -2 * e - 1)


def _residual(x, o):
    """o-th finite difference along the last axis: (..., bs) -> (..., bs - o)"""
    for _ in range(o):
        x = x[..., 1:] - x[..., :-1]
    return x


def plan_blocks(X):
    """X int64 (F, bs): F blocks of one size -> a list of F plans, dict(kind='constant' | 'verbatim' | 'fixed', bits=, and for
    fixed: order=, porder=, ks=[k_j], tied=[(o, p) of every FIXED candidate of the same size])"""
    X = np.asarray(X, dtype=np.int64)
    F, bs = X.shape
    verbatim = 8 + 16 * bs
    bits = np.full((F, 5, 7), _BIG, dtype=np.int64)
    ks = {}
    for o in range(min(4, bs - 1) + 1):
        zz = np.concatenate([np.zeros((F, o), dtype=np.int64), _zigzag(_residual(X, o))], axis=1)  # (F, bs), i < o not coded
        sh = zz[None, :, :] >> _K[:, None, None]                                                    # (15, F, bs)
        for p in range(7):
            L = bs >> p
            if bs % (1 << p) or L <= o:
                continue
            count = np.full(1 << p, L, dtype=np.int64)
            count[0] -= o
            cost = sh.reshape(15, F, 1 << p, L).sum(axis=3) + (_K + 1)[:, None, None] * count[None, None, :]
            kj = cost.argmin(axis=0)                      # the first = smallest k of the minimum
            bits[:, o, p] = 8 + 16 * o + 6 + (4 + cost.min(axis=0)).sum(axis=1)
            ks[o, p] = kj
    flat = bits.reshape(F, 35)
    idx = flat.argmin(axis=1)                             # the first minimum: smaller o, then smaller p
    const = (X == X[:, :1]).all(axis=1)
    out = []
    for f in range(F):
        best = int(flat[f, idx[f]])
        o, p = divmod(int(idx[f]), 7)
        if const[f] and 24 <= min(best, verbatim):
            out.append(dict(kind="constant", bits=24))
        elif best < verbatim:
            out.append(dict(kind="fixed", bits=best, order=o, porder=p, ks=[int(k) for k in ks[o, p][f]],
                            tied=[divmod(int(i), 7) for i in np.nonzero(flat[f] == best)[0]]))
        else:
            out.append(dict(kind="verbatim", bits=verbatim))
    return out


def plans(samples, blocksize):
    x = np.asarray(samples, dtype=np.int64).reshape(-1)
    n = len(x)
    full = n // blocksize
    out = plan_blocks(x[: full * blocksize].reshape(full, blocksize)) if full else []
    if n % blocksize:
        out += plan_blocks(x[full * blocksize:].reshape(1, -1))
    return out


def _field(values, width):
    """values (m,) -> m * width bits, MSB first (two's complement for negative values)"""
    v = np.asarray(values, dtype=np.int64).reshape(-1, 1)
    return ((v >> np.arange(width - 1, -1, -1, dtype=np.int64)) & 1).astype(np.uint8).reshape(-1)


def subframe_bits(s, plan):
    s = np.asarray(s, dtype=np.int64)
    bs = len(s)
    if plan["kind"] == "constant":
        return np.concatenate([_field([0x00], 8), _field(s[:1], 16)])
    if plan["kind"] == "verbatim":
        return np.concatenate([_field([0x02], 8), _field(s, 16)])
    o, p, ks = plan["order"], plan["porder"], np.asarray(plan["ks"], dtype=np.int64)
    L = bs >> p
    zz = _zigzag(_residual(s, o))                        # samples o .. bs - 1
    part = np.arange(o, bs) // L
    k = ks[part]
    q = zz >> k
    length = q + 1 + k
    start = np.cumsum(length) - length + 4 * (part + 1)  # behind the parameters of partitions 0 .. part
    body = np.zeros(int(length.sum()) + 4 * (1 << p), dtype=np.uint8)
    body[start + q] = 1
    for bit in range(int(k.max()) if len(k) else 0):
        m = k > bit
        body[(start + q + k - bit)[m]] = ((zz >> bit) & 1)[m].astype(np.uint8)
    firsts = np.concatenate([[0], np.arange(1, 1 << p) * L - o])    # index in zz of every partition's first sample
    ppos = start[firsts] - 4
    for j in range(1 << p):
        body[ppos[j]:ppos[j] + 4] = _field([ks[j]], 4)
    bits = np.concatenate([_field([(8 + o) << 1], 8), _field(s[:o], 16), _field([p], 6), body])
    assert len(bits) == plan["bits"], (len(bits), plan)
    return bits


def frame_header(number, bs, blocksize, rate):
    if bs == blocksize:
        bcode = 8 + BLOCK_SIZES.index(blocksize)
    else:
        bcode = 6 if bs <= 256 else 7
    rcode = rate_code(rate)
    h = bytes([0xFF, 0xF8, (bcode << 4) | rcode, 0x08]) + utf8_number(number)
    if bcode == 6:
        h += bytes([bs - 1])
    elif bcode == 7:
        h += (bs - 1).to_bytes(2, "big")
    if rcode == 13:
        h += rate.to_bytes(2, "big")
    h += bytes([crc8(h)])
    assert len(h) <= MAX_HEADER
    return h


def encode(samples, rate, blocksize=4096, md5=True):
    """int16 samples (n >= 1,) -> the .flac file's bytes"""
    x16 = np.ascontiguousarray(np.asarray(samples).reshape(-1), dtype="<i2")
    x = x16.astype(np.int64)
    n = len(x)
    assert n >= 1 and blocksize in BLOCK_SIZES
    frames = []
    for k, plan in enumerate(plans(x, blocksize)):
        s = x[k * blocksize:(k + 1) * blocksize]
        body = np.packbits(subframe_bits(s, plan)).tobytes()          # zero bits up to the byte boundary
        fr = frame_header(k, len(s), blocksize, rate) + body
        frames.append(fr + _crc16(fr).to_bytes(2, "big"))
    sizes = [len(f) for f in frames]
    sig = hashlib.md5(x16.tobytes()).digest() if md5 else bytes(16)
    word = (rate << 44) | (0 << 41) | (15 << 36) | n
    info = (blocksize.to_bytes(2, "big") * 2 + min(sizes).to_bytes(3, "big") + max(sizes).to_bytes(3, "big")
            + word.to_bytes(8, "big") + sig)
    assert len(info) == 34
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + info + b"".join(frames)


def worst_case_bytes(n, blocksize):
    return 0 if n <= 0 else 42 + -(-n // blocksize) * (MAX_HEADER + 1 + 2) + 2 * n
