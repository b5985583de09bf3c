"""SWC2 in plain Python, restated from the text of include/swc_entropy.h alone: the image, the three stream modes, the adaptive
model, the carry-less range coder and the CRC.  Slow and obvious on purpose; the kernels and the shared C++ header are tested
against it bit for bit (tests/test_entropy_cpu.py, tests/test_entropy_gpu.py)."""
import struct
import zlib

MAGIC = b"SWC2"
TOP, BOT, M32 = 1 << 24, 1 << 16, 0xFFFFFFFF
INC, LIMIT = 24, 8192
MAX_FRAMES = 65536
HEADER = 24


def n_codes(levels):
    return levels[0] * levels[1] * levels[2] * levels[3]


def width(levels):
    return (n_codes(levels) - 1).bit_length()


def raw_bytes(T, levels):
    return (T * width(levels) + 7) // 8


def split(c, levels):
    out = []
    for L in levels:
        out.append(c % L)
        c //= L
    return out


def join(lv, levels):
    c, base = 0, 1
    for s, L in zip(lv, levels):
        c += s * base
        base *= L
    return c


class Model:
    def __init__(self, levels, order):
        self.levels, self.order = levels, order
        self.rows = [[[1] * L for _ in range(L if order else 1)] for L in levels]
        self.prev = [0, 0, 0, 0]

    def row(self, d):
        return self.rows[d][self.prev[d] if self.order else 0]

    def update(self, d, s):
        row = self.row(d)
        row[s] += INC
        if sum(row) > LIMIT:
            row[:] = [(x + 1) >> 1 for x in row]

    def end_frame(self, lv):
        self.prev = list(lv)


class Encoder:
    def __init__(self):
        self.low, self.range, self.out, self.most = 0, M32, bytearray(), 0

    def encode(self, cum, f, tot):
        assert self.range >= BOT and 0 < f and cum + f <= tot <= LIMIT
        self.range //= tot
        self.low = (self.low + cum * self.range) & M32
        self.range = (self.range * f) & M32
        k = 0
        while True:
            if (self.low ^ ((self.low + self.range) & M32)) >= TOP:
                if self.range >= BOT:
                    break
                self.range = (0 - self.low) & (BOT - 1)
            self.out.append(self.low >> 24)
            self.low = (self.low << 8) & M32
            self.range = (self.range << 8) & M32
            k += 1
        self.most = max(self.most, k)

    def finish(self):
        self.out += struct.pack(">I", self.low)
        return bytes(self.out)


class Decoder:
    def __init__(self, data):
        self.data, self.pos = data, 4
        self.low, self.range = 0, M32
        self.code = int.from_bytes((bytes(data[:4]) + b"\0\0\0\0")[:4], "big")

    def decode(self, row):
        tot = sum(row)
        self.range //= tot
        v = min(((self.code - self.low) & M32) // self.range, tot - 1)
        s, cum = 0, 0
        while cum + row[s] <= v:
            cum += row[s]
            s += 1
        self.low = (self.low + cum * self.range) & M32
        self.range = (self.range * row[s]) & M32
        while True:
            if (self.low ^ ((self.low + self.range) & M32)) >= TOP:
                if self.range >= BOT:
                    break
                self.range = (0 - self.low) & (BOT - 1)
            nxt = self.data[self.pos] if self.pos < len(self.data) else 0
            self.pos += 1
            self.code = ((self.code << 8) | nxt) & M32
            self.low = (self.low << 8) & M32
            self.range = (self.range << 8) & M32
        return s


def encode_adaptive(codes, levels, order):
    m, e = Model(levels, order), Encoder()
    for c in codes:
        lv = split(c, levels)
        for d in range(4):
            row = m.row(d)
            e.encode(sum(row[:lv[d]]), row[lv[d]], sum(row))
            m.update(d, lv[d])
        m.end_frame(lv)
    return e.finish(), e.most


def decode_adaptive(data, T, levels, order):
    m, dec, out = Model(levels, order), Decoder(data), []
    for _ in range(T):
        lv = []
        for d in range(4):
            s = dec.decode(m.row(d))
            m.update(d, s)
            lv.append(s)
        m.end_frame(lv)
        out.append(join(lv, levels))
    return out


def encode_raw(codes, levels):
    w, acc = width(levels), 0
    for t, c in enumerate(codes):
        acc |= (c & ((1 << w) - 1)) << (w * t)
    return acc.to_bytes(raw_bytes(len(codes), levels), "little")


def decode_raw(data, T, levels):
    w = width(levels)
    acc = int.from_bytes(bytes(data) + b"\0" * raw_bytes(T, levels), "little")
    return [(acc >> (w * t)) & ((1 << w) - 1) for t in range(T)]


def encode_stream(codes, levels):
    """one (utterance, group) row -> (mode, bytes, number of invalid values)"""
    codes = [int(c) for c in codes]
    bad = sum(1 for c in codes if not 0 <= c < n_codes(levels))
    raw = encode_raw(codes, levels)
    if bad or not codes:
        return 0, raw, bad
    best = (len(raw), 0, raw)
    for order in (0, 1):
        s, _ = encode_adaptive(codes, levels, order)
        best = min(best, (len(s), order + 1, s))
    return best[1], best[2], 0


def encode_image(rows, levels):
    """rows: G sequences of T codes -> (image bytes, modes, bad)"""
    G, T = len(rows), len(rows[0])
    assert 1 <= G <= 8 and T <= MAX_FRAMES and all(len(r) == T for r in rows)
    assert all(2 <= L <= 16 for L in levels) and n_codes(levels) <= 16384
    streams = [encode_stream(r, levels) for r in rows]
    table = b"".join(struct.pack("<I", (m << 24) | len(s)) for m, s, _ in streams)
    body = table + b"".join(s for _, s, _ in streams)
    head = MAGIC + struct.pack("<IBB4BHI", T, G, 0, *levels, 0, len(body))
    crc = zlib.crc32(body, zlib.crc32(head))
    return head + struct.pack("<I", crc) + body, [m for m, _, _ in streams], sum(b for _, _, b in streams)


def parse_image(image, check_crc=True):
    """-> (T, G, levels, [(mode, offset in the image, length)]); ValueError for anything the text refuses"""
    if len(image) < HEADER or bytes(image[:4]) != MAGIC:
        raise ValueError("not a SWC2 image")
    T, G, ver, l0, l1, l2, l3, zero, body, crc = struct.unpack_from("<IBB4BHII", image, 4)
    levels = (l0, l1, l2, l3)
    if ver != 0 or zero != 0:
        raise ValueError("unsupported version")
    if not 1 <= G <= 8 or T > MAX_FRAMES or any(not 2 <= L <= 16 for L in levels) or n_codes(levels) > 16384:
        raise ValueError("limits")
    if body < 4 * G or len(image) < HEADER + body:
        raise ValueError("truncated")
    table, pos = [], HEADER + 4 * G
    for g in range(G):
        (e,) = struct.unpack_from("<I", image, HEADER + 4 * g)
        mode, ln = e >> 24, e & 0xFFFFFF
        if mode > 2 or (mode == 0 and ln != raw_bytes(T, levels)) or (mode and (T == 0 or ln < 4 or ln >= raw_bytes(T, levels))):
            raise ValueError("stream table")
        table.append((mode, pos, ln))
        pos += ln
    if pos != HEADER + body:
        raise ValueError("table sum")
    if check_crc and zlib.crc32(bytes(image[24:24 + body]), zlib.crc32(bytes(image[:20]))) != crc:
        raise ValueError("crc")
    return T, G, levels, table


def decode_image(image, check_crc=True):
    T, G, levels, table = parse_image(image, check_crc)
    rows = []
    for mode, off, ln in table:
        data = bytes(image[off:off + ln])
        rows.append(decode_raw(data, T, levels) if mode == 0 else decode_adaptive(data, T, levels, mode - 1))
    return rows
