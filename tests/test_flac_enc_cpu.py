"""The FLAC encoder (include/swc_flac_enc.h, csrc/swc_flac_enc.hip), everything that needs no GPU: the C-ABI of the header
(declarations == bindings == exported symbols), the argument checks that return before any launch, the workspace arithmetic,
the CLI flags — and the numpy reference tests/flac_fixed_ref.py against the project's own host decoder and frame index, over
a case table whose coverage of the encoder's choices is asserted here."""
import ctypes as C
import hashlib
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_enc_cases as cases  # noqa: E402
import flac_encode as fe  # noqa: E402
import flac_fixed_ref as ref  # noqa: E402

from simwhisper_codec_amd import _lib, wavio  # noqa: E402


def _header_text():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "swc_flac_enc.h")).read(), flags=re.S)


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_header_declarations_are_bound_and_exported():
    from simwhisper_codec_amd import build
    build.build_library()
    lib = _lib.load()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(swc_\w+)\s*\(", _header_text(), flags=re.M))
    assert declared == {"swc_flac_encode_workspace_bytes", "swc_flac_encode_batch"}
    assert declared == set(_lib.FLAC_ENC_SIGNATURES)
    for name, (argtypes, restype) in _lib.FLAC_ENC_SIGNATURES.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", _header_text(), flags=re.S):
        assert len(m.group(2).split(",")) == len(_lib.FLAC_ENC_SIGNATURES[m.group(1)][0]), m.group(1)
    # a table of its own: disjoint from every other one and from exported_symbols()
    others = [_lib.SIGNATURES, _lib.PLAIN, _lib.AUDIO_SIGNATURES, _lib.CODES_SIGNATURES, _lib.METRICS_SIGNATURES,
              _lib.QUALITY_SIGNATURES, _lib.FLAC_SIGNATURES, _lib.FLAC_IO_SIGNATURES]
    assert not any(declared & set(t) for t in others) and not declared & set(_lib.exported_symbols())
    assert "swc_flac_enc.hip" in build.SOURCES
    text = _header_text()
    from simwhisper_codec_amd import ops
    for name, val in (("SWC_FLAC_ENC_STREAM_HEADER", ops.FLAC_ENC_STREAM_HEADER), ("SWC_FLAC_ENC_MAX_HEADER", ops.FLAC_ENC_MAX_HEADER),
                      ("SWC_FLAC_ENC_MAX_HEADER", ref.MAX_HEADER)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", text).group(1)) == val


P = C.c_void_p


def _call(lib, **kw):
    n_max = kw.get("max_n", 1000)
    a = dict(rows=P(16), n=P(16), rate=16000, bs=4096, md5=1, out=P(16), out_bytes=None, off=P(16), sizes=P(16), ws=P(16),
             ws_bytes=1 << 30, max_n=n_max, B=2)
    a.update(kw)
    if a["out_bytes"] is None:
        a["out_bytes"] = a["B"] * ref.worst_case_bytes(a["max_n"], a["bs"] if a["bs"] in ref.BLOCK_SIZES else 4096)
    return lib.swc_flac_encode_batch(a["rows"], a["n"], a["rate"], a["bs"], a["md5"], a["out"], a["out_bytes"], a["off"], a["sizes"],
                                     a["ws"], a["ws_bytes"], a["max_n"], a["B"], P(0))


def test_encode_batch_checks_its_arguments_before_any_launch():
    """no GPU here: every call below must return in the argument checks (a launch would fail differently)"""
    lib = _lib.load()
    worst = 2 * ref.worst_case_bytes(1000, 4096)
    for bad in (dict(rows=P(0)), dict(n=P(0)), dict(out=P(0)), dict(off=P(0)), dict(sizes=P(0)), dict(ws=P(0)),
                dict(bs=300), dict(bs=0), dict(bs=8192), dict(rate=0), dict(rate=70000), dict(rate=-16000),
                dict(out_bytes=worst - 1), dict(B=65536), dict(B=-1), dict(max_n=-1), dict(max_n=1 << 31),
                dict(ws_bytes=255), dict(ws=P(8)), dict(off=P(4)), dict(sizes=P(4)), dict(rows=P(4)), dict(n=P(4)),
                dict(B=65535, max_n=(1 << 24) // 65535 * 4096 + 4096 * 2)):
        assert _call(lib, **bad) != 0, bad
        assert b"swc_flac_encode_batch" in lib.swc_last_error()
    # the table rates and any rate up to 65535 pass the rate check (the call then stops at the workspace size)
    for rate in list(ref.RATE_CODES) + [1, 11025, 65535]:
        assert _call(lib, rate=rate, ws_bytes=0) != 0 and b"workspace_bytes" in lib.swc_last_error(), rate
    # B == 0 launches nothing, whatever the pointers are
    assert lib.swc_flac_encode_batch(P(0), P(0), 16000, 4096, 1, P(0), 0, P(0), P(0), P(0), 0, 0, 0, P(0)) == 0


def test_workspace_layout_mirrors_the_c_arithmetic():
    from simwhisper_codec_amd import ops
    for ns in ([], [0], [1], [255, 256, 257], [160000] * 32, [4096, 0, 4097, 77], [1 << 20], [(1 << 31) - 1]):
        for bs in ref.BLOCK_SIZES:
            assert ops.flac_encode_workspace_layout(ns, bs) == ops.flac_encode_workspace_bytes(ns, bs), (ns, bs)
            ws, cap = ops.flac_encode_workspace_layout(ns, bs)
            assert ws % 256 == 0 and cap == sum(ref.worst_case_bytes(n, bs) for n in ns)
    assert ref.worst_case_bytes(1, 256) == 42 + 17 + 2
    for bad in (([10], 300), ([-1], 256), ([1 << 31], 256), ([4096 * 300] * 65535, 256)):
        with pytest.raises(_lib.SwcError):
            ops.flac_encode_workspace_bytes(*bad)
        with pytest.raises(_lib.SwcError):
            ops.flac_encode_workspace_layout(*bad)
    assert _lib.load().swc_flac_encode_workspace_bytes(None, 1, 256, None) == -1
    assert _lib.load().swc_flac_encode_workspace_bytes(None, 65536, 256, None) == -1


def test_cli_flags(monkeypatch, tmp_path):
    """--output_format: wav by default; flac needs a CUDA device and one process (refused before any process group or model)"""
    import inference
    args = inference.build_parser().parse_args([])
    assert args.output_format == "wav" and args.flac_md5 == "device"
    args = inference.build_parser().parse_args(["--output_format", "flac", "--flac_md5", "none"])
    assert args.output_format == "flac" and args.flac_md5 == "none"
    for bad in (["--output_format", "ogg"], ["--flac_md5", "host"]):
        with pytest.raises(SystemExit):
            inference.build_parser().parse_args(bad)
    io = ["--synthetic_checkpoint", "--input_dir", str(tmp_path), "--output_dir", str(tmp_path)]
    with pytest.raises(SystemExit, match="CUDA"):
        inference.main(["--output_format", "flac", "--device", "cpu"] + io)
    with pytest.raises(SystemExit, match="CUDA"):
        inference.main(["--output_format", "flac", "--mode", "decode", "--device", "cpu"] + io)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="torch.distributed.run"):
        inference.main(["--output_format", "flac"] + io)


# ------------------------------------------------------------------------------------------------ the reference
def _all_cases():
    out = {name: (x, bs, 16000) for name, (x, bs) in cases.coverage_cases().items()}
    for bs in (256, 4096):
        for name, x in cases.length_cases(bs).items():
            out[f"len_bs{bs}_{name}"] = (x, bs, 11025 if bs == 256 else 16000)
    return out


def test_reference_helpers():
    data = bytes(range(256)) * 3 + b"\x00\xff\x80"
    assert ref._crc16(data) == fe.crc16(data)
    assert ref.rate_code(16000) == 5 and ref.rate_code(11025) == 13 and ref.rate_code(65535) == 13
    for bad in (0, 65536, 70000):
        with pytest.raises(ValueError):
            ref.rate_code(bad)
    # a short frame never uses a table code
    assert ref.frame_header(3, 256, 512, 16000)[2] >> 4 == 6 and ref.frame_header(3, 257, 512, 16000)[2] >> 4 == 7
    assert ref.frame_header(3, 512, 512, 16000)[2] >> 4 == 9
    assert len(ref.frame_header((1 << 24) - 1, 4095, 4096, 11025)) == ref.MAX_HEADER


def test_the_case_table_covers_every_choice():
    plans = []
    for name, (x, bs, rate) in _all_cases().items():
        plans += ref.plans(x, bs)
    s = cases.plan_summary(plans)
    assert s["kinds"] == {"constant", "verbatim", "fixed"}
    assert s["orders"] == {0, 1, 2, 3, 4}
    assert s["porders"] == {0, 1, 2, 3, 4, 5, 6}
    assert 0 in s["ks"] and max(s["ks"]) >= 12 and max(s["ks"]) <= 14
    assert s["ties_to_smaller_order"] >= 1
    # the signals named for a choice make it
    c = cases.coverage_cases()
    kind = lambda name: ref.plans(*c[name])[0]   # noqa: E731
    assert kind("constant_zero")["kind"] == kind("constant_min")["kind"] == "constant"
    assert kind("alternation")["kind"] == "verbatim"
    assert kind("constant_but_last")["kind"] == "fixed"
    assert (kind("ramp")["order"], kind("ramp")["ks"]) == (2, [0])
    assert kind("noise_loud")["ks"] == [12]
    for p in range(7):
        assert kind(f"stepped_p{p}")["porder"] == p
    assert kind("stepped_p6_short")["porder"] == 6
    assert kind("tie")["order"] == 0 and (1, 0) in kind("tie")["tied"]


@pytest.mark.parametrize("name", sorted(_all_cases()))
def test_reference_streams_decode_through_the_host_code(name, tmp_path, caplog):
    x, bs, rate = _all_cases()[name]
    for md5 in (True, False):
        raw = ref.encode(x, rate, bs, md5=md5)
        assert len(raw) <= ref.worst_case_bytes(len(x), bs)
        path = tmp_path / f"{int(md5)}.flac"
        path.write_bytes(raw)
        caplog.clear()
        with caplog.at_level("WARNING"):
            pcm, sr, bits = wavio._decode_flac(str(path))                    # raises on a CRC or MD5 mismatch
        assert ("carries no MD5 signature" in caplog.text) == (not md5)
        assert sr == rate and bits == 16 and pcm.shape == (len(x), 1)
        assert np.array_equal(pcm.reshape(-1), x.astype(np.int32)), name
        assert _decode(path)[3] == int(md5)                                  # 1 = verified, 0 = "carries no signature"
        got = wavio.read_flac_raw(str(path))                                 # the index re-checks CRC-8, CRC-16, numbers, total
        assert got is not None and got.total == len(x) and got.blocksize == bs and len(got.frames) == -(-len(x) // bs)
    a, b = ref.encode(x, rate, bs, md5=True), ref.encode(x, rate, bs, md5=False)
    assert len(a) == len(b) and a[:26] == b[:26] and a[42:] == b[42:] and b[26:42] == bytes(16)
    assert a[26:42] == hashlib.md5(np.asarray(x, dtype="<i2").tobytes()).digest()


def _decode(path):
    """csrc/swc_flac.c on the file -> (int32 samples, rate, bits, md5 state)"""
    lib = wavio._io()
    data = open(path, "rb").read()
    sr, ch, bits, total = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    assert lib.swc_flac_info(data, len(data), C.byref(sr), C.byref(ch), C.byref(bits), C.byref(total)) == 0
    assert ch.value == 1
    out = np.empty(max(int(total.value), 1), dtype=np.int32)
    md5 = C.c_int32(-1)
    n = lib.swc_flac_decode(data, len(data), out.ctypes.data_as(C.c_void_p), int(total.value), C.byref(md5))
    assert n == total.value, n
    return out[:n], sr.value, bits.value, md5.value


# ------------------------------------------------------------------------------------------------ the kernels' serial pieces
def test_serial_pieces_under_the_sanitizers():
    """csrc/swc_flac_enc_bits.h (MD5, the shared CRC-16, frame and stream headers: what the kernels run) as a stand-alone host
    program built with ASan and UBSan, against hashlib and the reference"""
    import subprocess
    from simwhisper_codec_amd import build
    exe = build.build_flac_enc_check()

    def run(*a):
        r = subprocess.run([exe] + [str(v) for v in a], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert r.returncode == 0, r.stdout
        return r.stdout.split()
    ns = [1, 2, 4, 5, 27, 28, 29, 31, 32, 33, 59, 60, 63, 64, 255, 256, 257, 4097]   # around the padding boundaries at 56 and 64 bytes
    for n, got in zip(ns, run("md5", *ns)):
        s = ((np.arange(n, dtype=np.int64) * 7919 + 13) & 0xFFFF).astype("<u2")
        assert got == hashlib.md5(s.tobytes()).hexdigest(), n
    nbs = [1, 3, 4, 5, 17, 100, 1023, 1024, 1025, 4999, 8211]
    out = run("crc", *nbs)
    for i, nb in enumerate(nbs):
        b = bytes((31 * j + 7) & 0xFF for j in range(nb))
        assert out[2 * i] == out[2 * i + 1] == f"{fe.crc16(b) if nb < 2000 else ref._crc16(b):04x}", nb
    for k, bs, log2, rate in ((0, 256, 0, 16000), (127, 256, 0, 16000), (128, 256, 0, 16000), (2047, 512, 1, 11025), (2048, 100, 1, 11025),
                              (65535, 300, 4, 16000), (65536, 4096, 4, 44100), ((1 << 21) - 1, 256, 2, 8000), (1 << 21, 257, 2, 65535),
                              ((1 << 24) - 1, 4095, 4, 1)):
        assert run("hdr", k, bs, log2, rate) == [ref.frame_header(k, bs, 256 << log2, rate).hex()], (k, bs)
    x = cases.speech_like(5000, 1)
    want = ref.encode(x, 22050, 2048)
    sizes = [17, 4000]
    word = (22050 << 44) | (15 << 36) | 5000
    info = b"fLaC" + bytes([0x80, 0, 0, 34]) + (2048).to_bytes(2, "big") * 2 + sizes[0].to_bytes(3, "big") + sizes[1].to_bytes(3, "big") \
        + word.to_bytes(8, "big") + bytes(range(16))
    assert run("info", 2048, sizes[0], sizes[1], 22050, 5000) == [info.hex()]
    assert want[:12] == info[:12] and want[18:26] == info[18:26]     # the reference lays STREAMINFO out the same way
