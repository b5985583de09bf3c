"""Test infrastructure of the FLAC device path: the streams the index, the shared frame decoder and the GPU kernels are tested
on, all written by tests/flac_encode.py (imported, not edited) and all short (the encoder is Python ints).

matrix()       valid streams covering every subframe kind, 1 / 2 channels, 8 / 12 / 16 bits, wasted bits, Rice and Rice2, escape
               partitions, partition orders 0 .. max, LPC orders 1 / 12 / 32 and the four channel assignments.
damaged_set()  streams with bits flipped, frames cut short, or reserved / inconsistent codes patched in, whose CRC-16 was then
               recomputed so that they PASS swc_flac_index: what the frame decoder must answer with a status (or with the
               host decoder's samples), never with an access outside the frame or its planes.  Deterministic (seeded).
Everything is cached per process."""
import functools
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_encode as fe  # noqa: E402

V, K = "verbatim", "constant"


def F(o):
    return ("fixed", o)


def L(o):
    return ("lpc", o)


def signal(n, ch, bps, seed):
    g = np.random.default_rng(seed)
    t = np.arange(n)[:, None]
    amp = (1 << (bps - 1)) * 0.4
    x = amp * (np.sin(2 * np.pi * (220.0 + 37 * np.arange(ch)) * t / 16000.0) * 0.6 + 0.1 * g.standard_normal((n, ch)))
    if ch == 2:
        x[:, 1] = 0.7 * x[:, 0] + 0.3 * x[:, 1]
    return np.clip(np.round(x), -(1 << (bps - 1)), (1 << (bps - 1)) - 1).astype(np.int64)


def encode(x, sr, bps, **kw):
    """fe.encode, and what it wrote where: -> (stream bytes, [(frame offset, frame bytes, first sample, blocksize)]).  The
    encoder calls its crc16 once per frame, on the frame's bytes in front of the CRC: that call is listened to."""
    sizes = []
    real = fe.crc16

    def spy(data):
        sizes.append(len(data) + 2)
        return real(data)
    fe.crc16 = spy
    try:
        raw = fe.encode(x, sr, bps, **kw)
    finally:
        fe.crc16 = real
    bs = kw.get("blocksize", 1024)
    pos = len(raw) - sum(sizes)
    table = []
    for k, sz in enumerate(sizes):
        table.append((pos, sz, k * bs, min(bs, len(x) - k * bs)))
        pos += sz
    return raw, table


# ---------------------------------------------------------------------------------------------------- the valid matrix
KINDS0 = [V, K, F(0), F(1), F(2), F(3), F(4), L(1), L(12), L(32), L(8), F(2)]
KINDS1 = [L(32), K, L(12), L(1), F(4), F(3), F(2), F(1), F(0), V, F(3), L(12)]
PORDER = [0, 0, 2, 3, 1, 4, 0, 2, 3, 1, 2, 0]
MODES = [0, 8, 9, 10]


def _kinds_plan(bps):
    def plan(fi, c):
        if c is None:   # (mid = (l + r) >> 1 loses a wasted bit: the second wasted-bits frame is coded independently)
            return 0 if fi % 12 == 11 else MODES[fi % 4]
        po = PORDER[fi % 12]
        return dict(kind=(KINDS0 if c == 0 else KINDS1)[fi % 12], porder=po, rice2=fi % 2 == 1,
                    escape_part=((1 if po else 0) if fi % 3 == 2 else None), wasted=(3 if fi % 12 >= 10 else 0))
    return plan


@functools.lru_cache(maxsize=None)
def matrix():
    """-> [(name, x int64 [n, ch], rate, bps, stream bytes, frame table)]"""
    out = []
    bs = 256
    for ch in (1, 2):
        for bps in (8, 12, 16):
            x = signal(12 * bs + 77, ch, bps, seed=10 * ch + bps)
            x[bs:2 * bs] = x[bs]                       # frame 1: CONSTANT
            x[10 * bs:12 * bs] &= ~np.int64(7)         # frames 10, 11: three wasted bits
            raw, tab = encode(x, 16000 if ch == 1 else 48000, bps, blocksize=bs, plan=_kinds_plan(bps))
            out.append((f"kinds_c{ch}_b{bps}", x, 16000 if ch == 1 else 48000, bps, raw, tab))
    # partition orders 0 .. 8 (block size 256: partitions of one sample at the top), Rice and Rice2, with and without escape
    x = signal(18 * bs, 1, 16, seed=3)
    raw, tab = encode(x, 16000, 16, blocksize=bs, plan=lambda fi, c: 0 if c is None else dict(
        kind=(F(1) if fi % 2 else L(1)), porder=fi // 2, rice2=fi % 4 >= 2, escape_part=(fi // 2 and 1) if fi % 3 == 0 else None))
    out.append(("porders", x, 16000, 16, raw, tab))
    # every stereo mode with every predictor family, 12 bits
    x = signal(16 * 192 + 5, 2, 12, seed=4)
    raw, tab = encode(x, 44100, 12, blocksize=192, plan=lambda fi, c: MODES[fi % 4] if c is None else dict(
        kind=[V, F(2), L(12), L(32)][(fi // 4) % 4], porder=fi % 3, rice2=bool(fi & 1)))
    out.append(("stereo_modes", x, 44100, 12, raw, tab))
    return out


# ---------------------------------------------------------------------------------------------------- the damaged set
def reseal(raw, table, k, frame):
    """the stream with frame k replaced by `frame` (bytes in front of the CRC-16) and that frame's CRC-16 recomputed"""
    off, size = table[k][0], table[k][1]
    return raw[:off] + bytes(frame) + fe.crc16(bytes(frame)).to_bytes(2, "big") + raw[off + size:]


def _hdr_len(raw, off):
    """length of the frame header at off (through its CRC-8), for streams of this module: frame numbers below 128"""
    code = raw[off + 2] >> 4
    return 4 + 1 + (1 if code == 6 else 2 if code == 7 else 0) + 1


def _set_bits(frame, bitpos, nbits, value):
    v = int.from_bytes(frame, "big")
    total = 8 * len(frame)
    mask = ((1 << nbits) - 1) << (total - bitpos - nbits)
    v = (v & ~mask) | ((value << (total - bitpos - nbits)) & mask)
    return v.to_bytes(len(frame), "big")


@functools.lru_cache(maxsize=None)
def damaged_set():
    """-> [(name, stream bytes)], every stream without an MD5 signature (the host decoder then answers for the samples alone)"""
    g = np.random.default_rng(2024)
    bases = []
    x = signal(4 * 256, 1, 16, seed=31)
    bases.append(("m16",) + encode(x, 16000, 16, blocksize=256, md5=False, plan=lambda fi, c: 0 if c is None else dict(
        kind=[F(2), L(8), F(4), L(12)][fi], porder=[2, 0, 3, 1][fi], rice2=fi % 2 == 1, escape_part=1 if fi == 2 else None)))
    x = signal(4 * 192 + 50, 2, 12, seed=32)
    bases.append(("s12",) + encode(x, 48000, 12, blocksize=192, md5=False, plan=lambda fi, c: [10, 8, 9, 0, 10][fi] if c is None else dict(
        kind=[L(6), F(3), L(2), V, F(1)][fi], porder=fi % 3, rice2=fi % 2 == 0)))
    x = signal(6 * 16, 1, 8, seed=33)
    bases.append(("m8",) + encode(x, 16000, 8, blocksize=16, md5=False, plan=lambda fi, c: 0 if c is None else dict(
        kind=[F(2), L(4), F(0), V, F(1), L(1)][fi], porder=fi % 3)))
    out = []
    for name, raw, tab in bases:
        for t in range(10):                                  # one to three flipped bits inside a frame's subframes
            k = int(g.integers(0, len(tab)))
            off, size = tab[k][0], tab[k][1]
            h = _hdr_len(raw, off)
            frame = bytearray(raw[off:off + size - 2])
            for _ in range(1 + t % 3):
                frame[int(g.integers(h, len(frame)))] ^= 1 << int(g.integers(0, 8))
            out.append((f"{name}_flip{t}", reseal(raw, tab, k, frame)))
        for t, cut in enumerate((1, 2, 7)):                  # a frame cut short
            k = t % len(tab)
            off, size = tab[k][0], tab[k][1]
            h = _hdr_len(raw, off)
            keep = max(h + 1, size - 2 - cut)
            out.append((f"{name}_cut{t}", reseal(raw, tab, k, raw[off:off + keep])))
        k = 0                                                 # patched codes in the first subframe of frame 0
        off, size = tab[k][0], tab[k][1]
        h = _hdr_len(raw, off)
        frame = raw[off:off + size - 2]
        out.append((f"{name}_type_reserved", reseal(raw, tab, k, _set_bits(frame, 8 * h + 1, 6, 2))))
        out.append((f"{name}_type_reserved13", reseal(raw, tab, k, _set_bits(frame, 8 * h + 1, 6, 13))))
        out.append((f"{name}_padding_bit", reseal(raw, tab, k, _set_bits(frame, 8 * h, 1, 1))))
        out.append((f"{name}_lpc32", reseal(raw, tab, k, _set_bits(frame, 8 * h + 1, 6, 63))))       # order 32 (> a 16-sample block)
        out.append((f"{name}_wasted", reseal(raw, tab, k, _set_bits(frame, 8 * h + 7, 9, 0x100))))  # wasted flag, then zeros
    # the residual header of a FIXED order-2 subframe sits behind 8 + 2 bps bits: method and partition order patched
    name, raw, tab = bases[0]
    off, size = tab[0][0], tab[0][1]
    h = _hdr_len(raw, off)
    frame = raw[off:off + size - 2]
    at = 8 * h + 8 + 2 * 16
    out.append(("m16_method2", reseal(raw, tab, 0, _set_bits(frame, at, 2, 2))))
    out.append(("m16_method3", reseal(raw, tab, 0, _set_bits(frame, at, 2, 3))))
    out.append(("m16_porder15", reseal(raw, tab, 0, _set_bits(frame, at + 2, 4, 15))))
    out.append(("m16_porder8", reseal(raw, tab, 0, _set_bits(frame, at + 2, 4, 8))))      # 256 >> 8 = 1 < order 2
    out.append(("m16_porder9", reseal(raw, tab, 0, _set_bits(frame, at + 2, 4, 9))))      # 256 % 512 != 0
    name, raw, tab = bases[2]
    off, size = tab[0][0], tab[0][1]
    h = _hdr_len(raw, off)
    frame = raw[off:off + size - 2]
    at = 8 * h + 8 + 2 * 8
    out.append(("m8_porder4", reseal(raw, tab, 0, _set_bits(frame, at + 2, 4, 4))))       # 16 >> 4 = 1 < order 2
    out.append(("m8_porder5", reseal(raw, tab, 0, _set_bits(frame, at + 2, 4, 5))))
    return out


# the dozen the GPU status test uses (tests/test_flac_gpu.py), all part of what tests/test_flac_frame_cpu.py runs under the sanitizers
GPU_DAMAGED = ("m16_flip0", "m16_flip4", "m16_cut0", "m16_cut2", "m16_type_reserved", "m16_method2", "m16_porder15", "m16_porder8",
               "s12_flip1", "s12_cut1", "s12_lpc32", "m8_porder4")


def run_check(paths, dump=None, sanitize=True):
    """simwhisper_codec_amd/swc_flac_check (built on demand) over `paths` -> (returncode, {path: dict(index, host, status list,
    verdict)}, stderr).  Nothing is preloaded: the program is a stand-alone host binary."""
    from simwhisper_codec_amd import build
    exe = build.build_flac_check(sanitize=sanitize)
    r = subprocess.run([exe] + (["--dump", str(dump)] if dump else []) + [str(p) for p in paths], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    res = {}
    for line in r.stdout.splitlines():
        parts = line.rsplit(" ", 4)
        if len(parts) != 5:
            continue
        f = {p.split("=", 1)[0]: p.split("=", 1)[1] for p in parts[1:]}
        res[parts[0]] = dict(index=int(f["index"]), host=f["host"], verdict=f["verdict"],
                             status=[int(v) for v in f["status"].split(",")] if f["status"] else [])
    return r.returncode, res, r.stderr
