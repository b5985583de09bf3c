"""SWC2 (include/swc_entropy.h) without a GPU: the ABI (declarations == bindings == exports, a table apart from the others, the
limits), every argument check before any launch, the plain-Python restatement (tests/entropy_ref.py) on the issue's known
answers and its round trips, the shared header's host encode / decode against it bit for bit (through the check program),
swc_entropy_parse against zlib.crc32 and on every refusal, the check program's own verdict, and the CLI flag."""
import ctypes as C
import os
import random
import re
import struct
import subprocess
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import entropy_ref as ref  # noqa: E402

NAMES = {"swc_entropy_worst_bytes", "swc_entropy_workspace_bytes", "swc_entropy_encode_batch", "swc_entropy_decode_batch",
         "swc_entropy_parse"}
SHIPPED = (8, 7, 6, 6)
LEVEL_SETS = [SHIPPED, (2, 2, 2, 2), (16, 16, 8, 8), (16, 16, 16, 4)]


def _header(name="swc_entropy.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


def _lib():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    return _lib, _lib.load()


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


# ---- the generated streams of the issue (shared with the GPU tests) ----

def stream(kind, T, levels, seed):
    """uniform -> raw; iid geometric levels -> order 0; sticky (keeps its value with p = 0.8) -> order 1; constant"""
    rng = random.Random(f"{kind}-{T}-{levels}-{seed}")
    n = ref.n_codes(levels)
    if kind == "uniform":
        return [rng.randrange(n) for _ in range(T)]
    if kind == "constant":
        return [seed % n] * T
    if kind == "geometric":
        return [ref.join([min(int(rng.expovariate(1.2)), L - 1) for L in levels], levels) for _ in range(T)]
    out, c = [], rng.randrange(n)
    for _ in range(T):
        if rng.random() >= 0.8:
            c = rng.randrange(n)
        out.append(c)
    return out


# ---- ABI ----

def test_entropy_header_declarations_are_bound():
    _l, lib = _lib()
    declared = _declared("swc_entropy.h")
    assert declared == NAMES == set(_l.ENTROPY_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)
        argtypes, restype = _l.ENTROPY_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    seen = {}
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        seen[m.group(1)] = len(m.group(2).split(","))
    assert seen == {n: len(_l.ENTROPY_SIGNATURES[n][0]) for n in NAMES}
    assert [seen[n] for n in sorted(NAMES)] == [16, 16, 9, 5, 3]


def test_entropy_table_is_apart_from_the_others():
    from simwhisper_codec_amd import _lib
    mine = set(_lib.ENTROPY_SIGNATURES)
    assert not mine & set(_lib.exported_symbols())
    others = {k: v for k, v in vars(_lib).items() if (k.endswith("SIGNATURES") or k == "PLAIN") and k != "ENTROPY_SIGNATURES"}
    assert len(others) >= 18
    for other in others.values():
        assert not mine & set(other)
    text = re.sub(r"swc_entropy\w*", " ", _header())
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "swc_entropy.h":
            assert not mine & _declared(h)
            assert "swc_entropy" not in _header(h), h
            for name in _declared(h):   # the new header's text names no function that another table owns
                assert name not in text, (h, name)
    for other in others.values():
        for name in other:
            assert name not in text, name


def test_constants_agree_with_the_header_and_the_reference():
    from simwhisper_codec_amd import _lib
    hdr = _header()
    d = {k: int(v) for k, v in re.findall(r"#define (SWC_ENTROPY_\w+) \(?(-?\d+)\)?", hdr)}
    assert d["SWC_ENTROPY_HEADER_BYTES"] == _lib.ENTROPY_HEADER_BYTES == ref.HEADER == 24
    assert d["SWC_ENTROPY_MAX_FRAMES"] == _lib.ENTROPY_MAX_FRAMES == ref.MAX_FRAMES == 65536
    assert d["SWC_ENTROPY_MAX_GROUPS"] == _lib.ENTROPY_MAX_GROUPS == 8
    assert (d["SWC_ENTROPY_MIN_LEVEL"], d["SWC_ENTROPY_MAX_LEVEL"], d["SWC_ENTROPY_MAX_CODES"]) == \
        (_lib.ENTROPY_MIN_LEVEL, _lib.ENTROPY_MAX_LEVEL, _lib.ENTROPY_MAX_CODES) == (2, 16, 16384)
    assert (d["SWC_ENTROPY_INC"], d["SWC_ENTROPY_LIMIT"]) == (_lib.ENTROPY_INC, _lib.ENTROPY_LIMIT) == (ref.INC, ref.LIMIT) == (24, 8192)
    assert d["SWC_ENTROPY_MAX_RENORM"] == _lib.ENTROPY_MAX_RENORM == 3
    assert {d[k] for k in d if k.startswith("SWC_ENTROPY_E_")} == set(_lib.ENTROPY_E) == {-1, -2, -3, -4, -5, -6}


def test_sizes_are_host_arithmetic():
    _l, lib = _lib()
    for lv in LEVEL_SETS:
        for G in (1, 3, 8):
            for T in (0, 1, 125, 65536):
                assert lib.swc_entropy_worst_bytes(T, G, _i32(*lv)) == 24 + 4 * G + G * ref.raw_bytes(T, lv)
    assert ref.width(SHIPPED) == 11 and ref.width((2, 2, 2, 2)) == 4 and ref.width((16, 16, 8, 8)) == 14
    for T, G, lv in ((-1, 8, SHIPPED), (65537, 8, SHIPPED), (5, 0, SHIPPED), (5, 9, SHIPPED), (5, 8, (8, 7, 6, 17)), (5, 8, (8, 7, 6, 1)),
                     (5, 8, (16, 16, 16, 16))):
        assert lib.swc_entropy_worst_bytes(T, G, _i32(*lv)) == -1
    assert lib.swc_entropy_worst_bytes(5, 8, None) == -1
    cap = C.c_int64(-7)
    n = (C.c_int64 * 3)(0, 125, 37)
    ws = lib.swc_entropy_workspace_bytes(n, 3, 8, _i32(*SHIPPED), C.byref(cap))
    slot = (ref.raw_bytes(125, SHIPPED) + 3) // 4 * 4
    up = lambda v: (v + 255) // 256 * 256   # noqa: E731
    assert ws == up(3 * 8 * 2 * 4) + up(3 * 8 * 4) + up(3 * 8 * 2 * slot) and ws % 256 == 0
    assert cap.value == sum(24 + 32 + 8 * ref.raw_bytes(t, SHIPPED) for t in (0, 125, 37))
    assert lib.swc_entropy_workspace_bytes(None, 0, 8, _i32(*SHIPPED), None) == 0
    assert lib.swc_entropy_workspace_bytes(None, 1, 8, _i32(*SHIPPED), None) == -1
    assert lib.swc_entropy_workspace_bytes(n, 65536, 8, _i32(*SHIPPED), None) == -1
    assert lib.swc_entropy_workspace_bytes((C.c_int64 * 1)(65537), 1, 8, _i32(*SHIPPED), None) == -1
    assert lib.swc_entropy_workspace_bytes((C.c_int64 * 1)(-1), 1, 8, _i32(*SHIPPED), None) == -1
    assert lib.swc_entropy_workspace_bytes(n, 3, 9, _i32(*SHIPPED), None) == -1


def test_every_argument_check_comes_before_any_launch():
    """host memory stands in for device memory: a call that got as far as a launch would not return SWC_E_ARG"""
    _l, lib = _lib()
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    p = p + (-p) % 16
    lv = _i32(*SHIPPED)
    worst = lib.swc_entropy_worst_bytes(10, 8, lv)
    ws = lib.swc_entropy_workspace_bytes((C.c_int64 * 2)(10, 10), 2, 8, lv, None)
    good = dict(rows=p, ldg=p + 64, n=p + 128, es=4, lv=lv, G=8, mf=10, out=p + 1024, ob=2 * worst, off=p + 256, sz=p + 320, bad=p + 384,
                ws=p + 512, wsb=ws, B=2)

    def enc(**kw):
        a = dict(good, **kw)
        return lib.swc_entropy_encode_batch(a["rows"], a["ldg"], a["n"], a["es"], a["lv"], a["G"], a["mf"], a["out"], a["ob"], a["off"],
                                            a["sz"], a["bad"], a["ws"], a["wsb"], a["B"], None)

    cases = [dict(B=-1), dict(B=65536), dict(es=2), dict(es=16), dict(lv=None), dict(G=0), dict(G=9), dict(lv=_i32(8, 7, 6, 17)),
             dict(lv=_i32(1, 7, 6, 6)), dict(lv=_i32(16, 16, 16, 16)), dict(mf=-1), dict(mf=65537), dict(rows=None), dict(ldg=None),
             dict(n=None), dict(out=None), dict(off=None), dict(sz=None), dict(ws=None), dict(rows=p + 4), dict(ldg=p + 68),
             dict(n=p + 132), dict(off=p + 260), dict(sz=p + 324), dict(ws=p + 520), dict(bad=p + 386), dict(ob=2 * worst - 1),
             dict(wsb=ws - 1)]
    for kw in cases:
        assert enc(**kw) == -1, kw
        assert b"swc_entropy_encode_batch" in lib.swc_last_error()
    assert enc(B=0) == 0 and enc(B=0, rows=None, out=None, ws=None) == 0        # nothing to do: no launch either

    gd = dict(by=p, ib=100, so=p + 64, sl=p + 128, sm=p + 192, n=p + 256, lv=lv, G=8, codes=p + 1024, ldg=20, ldb=10, L=10, B=2, nc=2016,
              bad=None)

    def dec(**kw):
        a = dict(gd, **kw)
        return lib.swc_entropy_decode_batch(a["by"], a["ib"], a["so"], a["sl"], a["sm"], a["n"], a["lv"], a["G"], a["codes"], a["ldg"],
                                            a["ldb"], a["L"], a["B"], a["nc"], a["bad"], None)

    for kw in [dict(by=None), dict(so=None), dict(sl=None), dict(sm=None), dict(n=None), dict(codes=None), dict(B=-1), dict(B=65536),
               dict(lv=None), dict(G=0), dict(G=9), dict(lv=_i32(8, 7, 6, 0)), dict(L=-1), dict(L=65537), dict(ldb=9), dict(ldg=19),
               dict(ib=-1), dict(nc=0)]:
        assert dec(**kw) == -1, kw
        assert b"swc_entropy_decode_batch" in lib.swc_last_error()
    assert dec(B=0) == 0 and dec(L=0, ldb=0, ldg=0) == 0


# ---- the reference ----

KNOWN_1 = ("535743320c00000002000807060600001e0000005011c4820500000111000000a007f49a4600f83efa223080f3054000032040010c00")
KNOWN_4 = "53574332000000000200080706060000080000008f0a341e0000000000000000"


def _known():
    return [([[5] * 12, [0, 2015, 1000, 17, 3, 999, 1, 2, 3, 4, 5, 6]], 54, [1, 0]),
            ([[((t // (g + 1)) * 9 + g) % 2016 for t in range(300)] for g in range(8)], 843, [2] * 8),
            ([[(37 * t * t + 101 * g + 5) % 2016 for t in range(40)] for g in range(3)], 201, [0] * 3),
            ([[], []], 32, [0, 0])]


def test_the_four_known_answers():
    images = []
    for rows, size, modes in _known():
        image, got, bad = ref.encode_image(rows, SHIPPED)
        assert (len(image), got, bad) == (size, modes, 0)
        assert ref.decode_image(image) == rows
        images.append(image)
    assert images[0].hex() == KNOWN_1 and images[3].hex() == KNOWN_4
    assert "%08x" % zlib.crc32(images[1]) == "71cbd4de" and "%08x" % zlib.crc32(images[2]) == "d58ac186"
    assert 12 + 11 * 300 == 3312       # what SWC1 spends on the second


@pytest.mark.parametrize("levels", LEVEL_SETS)
def test_reference_round_trips(levels):
    most = 0
    for T in (0, 1, 2, 3, 37, 125):
        for kind in ("uniform", "geometric", "sticky", "constant"):
            c = stream(kind, T, levels, 3)
            for order in (0, 1):
                s, k = ref.encode_adaptive(c, levels, order)
                most = max(most, k)
                assert ref.decode_adaptive(s, T, levels, order) == c
            assert ref.decode_raw(ref.encode_raw(c, levels), T, levels) == c
            image, modes, _ = ref.encode_image([c, c[::-1]], levels)
            assert ref.decode_image(image) == [c, c[::-1]]
            assert len(image) <= 24 + 8 + 2 * ref.raw_bytes(T, levels)          # never larger than raw plus the header
    assert most <= 3


def test_both_halving_branches_run(monkeypatch):
    """T = 400 constant: an order-1 row passes 8192 (1 + 24 k > 8192 - L after 341 symbols); T = 1500: the order-0 rows do"""
    halved = []
    orig = ref.Model.update

    def spy(self, d, s):
        before = sum(self.row(d))
        orig(self, d, s)
        if sum(self.row(d)) < before:
            halved.append(self.order)
    monkeypatch.setattr(ref.Model, "update", spy)
    c = stream("constant", 400, SHIPPED, 77)
    for order in (0, 1):
        s, _ = ref.encode_adaptive(c, SHIPPED, order)
    assert set(halved) == {0, 1}
    del halved[:]
    c = stream("sticky", 1500, SHIPPED, 1)
    s, _ = ref.encode_adaptive(c, SHIPPED, 0)
    assert halved and ref.decode_adaptive(s, 1500, SHIPPED, 0) == c
    s, _ = ref.encode_adaptive(c, SHIPPED, 1)
    assert ref.decode_adaptive(s, 1500, SHIPPED, 1) == c


def test_generated_streams_reach_all_three_modes():
    for levels in LEVEL_SETS:
        for T in (37, 125, 400):
            got = {kind: ref.encode_stream(stream(kind, T, levels, 5), levels)[0] for kind in ("uniform", "geometric", "sticky")}
            if levels == (2, 2, 2, 2) and T < 400:   # 4-bit codes: an order-0 stream this short does not beat raw by its 4 end bytes
                del got["geometric"]
            assert got == {k: m for k, m in (("uniform", 0), ("geometric", 1), ("sticky", 2)) if k in got}, (levels, T, got)


def test_invalid_values_go_raw_and_are_counted():
    rows = [[5, -1, 2016, 7], [1, 2, 3, 4], [1 << 40, 0, 0, 0]]
    image, modes, bad = ref.encode_image(rows, SHIPPED)
    assert modes[0] == 0 and modes[2] == 0 and bad == 3
    back = ref.decode_image(image)
    assert back[0] == [5, 2047, 2016, 7] and back[2] == [0, 0, 0, 0] and back[1] == rows[1]


# ---- the shared header's host code, through the check program ----

def _check_program():
    from simwhisper_codec_amd import build
    return build.build_entropy_check()


def test_check_program_passes():
    r = subprocess.run([_check_program()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert "swc_entropy_check: ok" in r.stdout


@pytest.mark.parametrize("levels", LEVEL_SETS)
def test_host_encode_decode_match_the_reference_bit_for_bit(levels):
    exe = _check_program()
    cases = [(kind, T) for T in (0, 1, 2, 3, 37, 125) for kind in ("uniform", "geometric", "sticky")]
    cases += [("constant", 400), ("sticky", 1500)]
    for kind, T in cases:
        rows = [stream(kind, T, levels, g) for g in range(2)]
        if kind == "uniform" and T == 37:
            rows[1][5] = -1                     # an invalid value: raw, low bits
        want, modes, _ = ref.encode_image(rows, levels)
        text = " ".join(str(c) for r in rows for c in r)
        r = subprocess.run([exe, "encode", *map(str, levels), "2", str(T)], input=text, stdout=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip() == want.hex(), (kind, T)
        r = subprocess.run([exe, "decode"], input=want.hex(), stdout=subprocess.PIPE, text=True, timeout=120)
        lines = r.stdout.splitlines()
        assert r.returncode == 0 and lines[0].split() == [str(T), "2", *map(str, levels)]
        assert [int(m) for m in lines[1].split()] == modes
        assert [[int(c) for c in ln.split()] for ln in lines[2:4]] == ref.decode_image(want)
    for rows, size, modes in _known():
        if levels == SHIPPED:
            text = " ".join(str(c) for r in rows for c in r)
            r = subprocess.run([exe, "encode", "8", "7", "6", "6", str(len(rows)), str(len(rows[0]))], input=text, stdout=subprocess.PIPE,
                               text=True, timeout=120)
            assert r.stdout.strip() == ref.encode_image(rows, SHIPPED)[0].hex()


# ---- swc_entropy_parse ----

def _parse(lib, image, check_crc=1):
    T, G = C.c_int32(-1), C.c_int32(-1)
    lv, off, ln, mode = (C.c_int32 * 4)(), (C.c_int64 * 8)(), (C.c_int64 * 8)(), (C.c_int32 * 8)()
    data = bytes(image)
    rc = lib.swc_entropy_parse(data, len(data), check_crc, C.byref(T), C.byref(G), lv, off, ln, mode)
    return rc, (T.value, G.value, tuple(lv), [(mode[g], off[g], ln[g]) for g in range(max(G.value, 0))])


def test_parse_agrees_with_the_reference_and_zlib():
    _l, lib = _lib()
    for levels in LEVEL_SETS:
        for kind, T in (("uniform", 37), ("sticky", 125), ("geometric", 64), ("constant", 0), ("constant", 1)):
            rows = [stream(kind, T, levels, g) for g in range(3)]
            image, modes, _ = ref.encode_image(rows, levels)
            rc, got = _parse(lib, image)
            assert rc == 0 and got == ref.parse_image(image)
            body = struct.unpack_from("<I", image, 16)[0]
            assert struct.unpack_from("<I", image, 20)[0] == zlib.crc32(image[24:24 + body], zlib.crc32(image[:20]))
            assert _parse(lib, image + b"\xff" * 7)[0] == 0                       # bytes behind the image are not looked at
            assert lib.swc_entropy_parse(image, len(image), 1, None, None, None, None, None, None) == 0


def test_parse_refusals():
    _l, lib = _lib()
    rows = [stream("sticky", 37, SHIPPED, g) for g in range(8)]
    image, _, _ = ref.encode_image(rows, SHIPPED)

    def lie(pos, value, image=image):
        """one byte changed, the CRC made right again: what only the other checks can catch"""
        b = bytearray(image)
        b[pos] = value
        body = struct.unpack_from("<I", image, 16)[0]
        struct.pack_into("<I", b, 20, zlib.crc32(bytes(b[24:24 + body]), zlib.crc32(bytes(b[:20]))))
        return bytes(b)
    assert _parse(lib, lie(0, ord("X")))[0] == -1                              # wrong magic
    assert _parse(lib, b"SWC1" + image[4:])[0] == -1
    assert _parse(lib, lie(9, 1))[0] == -2                                      # version 1
    assert _parse(lib, lie(14, 1))[0] == -2
    assert _parse(lib, lie(10, 17))[0] == -3                                    # a level of 17
    assert _parse(lib, lie(10, 1))[0] == -3
    assert _parse(lib, lie(8, 9))[0] == -3 and _parse(lib, lie(8, 0))[0] == -3
    assert _parse(lib, lie(7, 1))[0] == -3                                      # T = 2^24 + 37
    assert _parse(lib, lie(16, image[16] - 1))[0] == -5                         # a table sum != body_bytes
    assert _parse(lib, lie(16, image[16] + 1) + b"\0")[0] == -5
    assert _parse(lib, lie(16, image[16] + 1))[0] == -4
    assert _parse(lib, lie(27, 3))[0] == -5                                     # mode 3
    raw3, modes3, _ = ref.encode_image(_known()[2][0], SHIPPED)
    assert modes3 == [0, 0, 0] and _parse(lib, lie(4, 39, raw3))[0] == -5       # a T that does not fit the raw lengths
    for cut in list(range(0, 64)) + [len(image) - 1]:
        assert _parse(lib, image[:cut])[0] in (-4, -1) and _parse(lib, image[:cut])[0] < 0, cut
        with pytest.raises(ValueError):
            ref.parse_image(image[:cut])
    assert _parse(lib, b"")[0] == -4
    for bit in range(8 * len(image)):                                            # one flipped bit, anywhere
        b = bytearray(image)
        b[bit >> 3] ^= 1 << (bit & 7)
        assert _parse(lib, b)[0] < 0, bit
    b = bytearray(image)
    b[len(image) - 3] ^= 0x10
    assert _parse(lib, b)[0] == -6 and _parse(lib, b, check_crc=0)[0] == 0     # the CRC is what catches a flip inside a stream
    for pos, value in ((0, ord("X")), (9, 1), (10, 17), (16, image[16] - 1)):
        with pytest.raises(ValueError):
            ref.parse_image(lie(pos, value))


def test_parse_image2_names_the_file():
    from simwhisper_codec_amd import bitstream
    rows = [stream("sticky", 37, SHIPPED, g) for g in range(8)]
    image, modes, _ = ref.encode_image(rows, SHIPPED)
    T, G, lv, table = bitstream.parse_image2(image, "a.swc")
    assert (T, G, lv) == (37, 8, SHIPPED) and table == ref.parse_image(image)[3]
    T, G, lv, table = bitstream.parse_image2(b"xyz" + image + b"tail", "a.swc", offset=3)
    assert table == [(m, o + 3, k) for m, o, k in ref.parse_image(image)[3]]
    b = bytearray(image)
    b[60] ^= 4
    with pytest.raises(ValueError, match=r"^dir/b\.swc: not a sound SWC2 code file \(CRC mismatch\)"):
        bitstream.parse_image2(b, "dir/b.swc")
    assert bitstream.parse_image2(b, "dir/b.swc", check_crc=False)[0] == 37
    with pytest.raises(ValueError, match=r"^c\.swc: .*truncated"):
        bitstream.parse_image2(image[:-1], "c.swc")
    assert bitstream.is_image2(image) and not bitstream.is_image2(b"SWC1" + image[4:]) and not bitstream.is_image2(b"SW")
    # SWC1 stays what it was
    assert bitstream.MAGIC == b"SWC1" and bitstream.parse_header(bitstream.header(3) + bytes(33)) == 3
    with pytest.raises(ValueError, match="x: not a SWC1 code file"):
        bitstream.parse_header(image, "x")


# ---- the CLI flag and the Python surface ----

def test_code_format_flag_parses_and_is_refused_outside_encode():
    import inference
    p = inference.build_parser()
    assert p.parse_args([]).code_format == "swc1"
    assert p.parse_args(["--mode", "encode", "--code_format", "swc2"]).code_format == "swc2"
    with pytest.raises(SystemExit):
        p.parse_args(["--code_format", "swc3"])
    for mode in ("roundtrip", "decode"):
        with pytest.raises(SystemExit, match="--code_format names the container --mode encode writes"):
            inference.main(["--mode", mode, "--code_format", "swc2", "--device", "cpu"])


def test_python_refusals():
    import torch
    from simwhisper_codec_amd import bitstream
    from simwhisper_codec_amd._lib import SwcError
    from simwhisper_codec_amd.pipeline import HostStager
    good = [torch.zeros(8, 5, dtype=torch.int32)]
    with pytest.raises(SwcError, match="0 utterances"):
        bitstream.compress_batch([], SHIPPED)
    with pytest.raises(SwcError, match="four FSQ levels"):
        bitstream.compress_batch(good, (8, 7, 6))
    with pytest.raises(SwcError, match="one HIP device"):
        bitstream.compress_batch(good, SHIPPED)
    with pytest.raises(ValueError, match="format 'swc3'"):
        bitstream.write_codes_batch(["x"], good, format="swc3")
    with pytest.raises(ValueError, match="needs the FSQ levels"):
        bitstream.write_codes_batch(["x"], good, format="swc2")
    with pytest.raises(ValueError, match="format 'flat'"):
        HostStager().codes_to_host(good, format="flat")
    with pytest.raises(ValueError, match="needs the FSQ levels"):
        HostStager().codes_to_host(good, format="swc2")
    assert bitstream.worst_bytes2(125, SHIPPED) == 24 + 32 + 8 * 172
    with pytest.raises(SwcError, match="outside SWC2's limits"):
        bitstream.worst_bytes2(65537, SHIPPED)
