"""Batched code files, the parts that need no GPU: the C-ABI of include/swc_codes.h (declarations == bindings == exported
symbols, kept apart from swc.h's table; argument checks before any launch), bitstream.parse_header against images built from
the numpy oracle (oracle/bitstream_np.py) plus the documented header, and the CLI's --mode flag."""
import ctypes as C
import os
import re
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _header_text():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "swc_codes.h")).read(), flags=re.S)


def _declared():
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", _header_text(), flags=re.M))


def oracle_image(codes, groups=8, bits=11, magic=b"SWC1"):
    """the documented file image: b"SWC1" | u32 n_frames | u8 groups | u8 bits | u16 0 | the oracle's payload"""
    from oracle import bitstream_np
    codes = np.asarray(codes)
    return magic + struct.pack("<IBBH", codes.shape[1], groups, bits, 0) + bitstream_np.pack(codes).tobytes()


def random_codes(T, seed, hi=2016):
    return np.random.default_rng(seed).integers(0, hi, size=(8, T), dtype=np.int64)


def test_codes_header_declarations_are_bound_and_exported():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    declared = _declared()
    assert declared == {"swc_codefile_bytes", "swc_codes_pack_batch", "swc_codes_unpack_batch"}
    assert declared == set(_lib.CODES_SIGNATURES), declared ^ set(_lib.CODES_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)   # exported by the built library
        argtypes, restype = _lib.CODES_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    # the headers stay apart: swc.h's and swc_audio.h's tables (and the tests that pin them) do not know these symbols
    assert not declared & set(_lib.exported_symbols()) and not declared & set(_lib.AUDIO_SIGNATURES)
    for other in ("swc.h", "swc_audio.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(name in text for name in declared), other
    assert "swc_codes.hip" in build.SOURCES


def test_the_new_header_makes_the_library_stale(tmp_path):
    """build._stale() watches include/swc_codes.h like the other two headers"""
    from simwhisper_codec_amd import build
    build.build_library()
    assert not build._stale()
    hdr = os.path.join(ROOT, "include", "swc_codes.h")
    st = os.stat(hdr)
    try:
        os.utime(hdr, (st.st_atime, os.path.getmtime(build.LIB_PATH) + 10))
        assert build._stale()
    finally:
        os.utime(hdr, (st.st_atime, st.st_mtime))
    assert not build._stale()


def test_every_codes_output_entry_point_has_a_memory_contract_test():
    """the guarantee tests/test_poison_cpu.py gives include/swc.h, for include/swc_codes.h: every declaration with a device
    output pointer is exercised in a guarded window by tests/test_codefile_gpu.py"""
    outs = []
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", _header_text(), flags=re.S):
        params = [p.strip() for p in m.group(2).split(",")]
        if any("*" in p and not re.search(r"\bstream$", p) and not p.startswith("const") for p in params):
            outs.append(m.group(1))
    assert outs == ["swc_codes_pack_batch", "swc_codes_unpack_batch"]
    src = open(os.path.join(ROOT, "tests", "test_codefile_gpu.py")).read()
    assert "poison.guarded" in src and "bitstream.pack_batch(" in src and "bitstream.unpack_batch(" in src
    assert "def test_memory_contract_pack" in src and "def test_memory_contract_unpack" in src


def test_codefile_bytes():
    from simwhisper_codec_amd import _lib, bitstream
    lib = _lib.load()
    for n in (0, 1, 2, 125, 126, 375, 10 ** 6, 2 ** 40):
        assert lib.swc_codefile_bytes(n) == 12 + 11 * n == bitstream.image_bytes(n)
    assert lib.swc_codefile_bytes(125) == 1387            # 10 s of audio
    assert lib.swc_codefile_bytes(-1) == -1 and lib.swc_codefile_bytes(-2 ** 40) == -1


def test_arg_checks_without_gpu():
    """every check happens before any launch: host pointers that are never dereferenced stand in for device memory"""
    from simwhisper_codec_amd import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)

    def pack(rows=p, ldg=p, n=p, off=p, es=4, out=p, out_bytes=512, max_frames=10, B=2):
        return lib.swc_codes_pack_batch(rows, ldg, n, off, es, out, out_bytes, max_frames, B, None)

    for kw, word in [(dict(rows=None), b"null"), (dict(ldg=None), b"null"), (dict(n=None), b"null"), (dict(off=None), b"null"),
                     (dict(out=None), b"null"), (dict(B=-1), b"B="), (dict(B=65536), b"B="), (dict(es=2), b"elem_size"),
                     (dict(es=0), b"elem_size"), (dict(es=16), b"elem_size"), (dict(out_bytes=-1), b"out_bytes"),
                     (dict(out_bytes=23), b"out_bytes"), (dict(max_frames=-1), b"max_frames"),
                     (dict(max_frames=(1 << 24) + 1), b"max_frames")]:
        assert pack(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    assert pack(B=0, out_bytes=0) == 0            # nothing to do: no launch, no device needed

    def unpack(src=p, in_bytes=512, off=p, n=p, codes=p, ldg=64, ldb=16, L=16, B=4, n_codes=2016, bad=None):
        return lib.swc_codes_unpack_batch(src, in_bytes, off, n, codes, ldg, ldb, L, B, n_codes, bad, None)

    for kw, word in [(dict(src=None), b"null"), (dict(off=None), b"null"), (dict(n=None), b"null"), (dict(codes=None), b"null"),
                     (dict(B=-1), b"B="), (dict(B=65536, ldg=1 << 40), b"B="), (dict(L=-1), b"L="), (dict(L=(1 << 24) + 1), b"L="),
                     (dict(ldb=15), b"strides"), (dict(ldg=63), b"strides"), (dict(in_bytes=-1), b"in_bytes"),
                     (dict(n_codes=0), b"n_codes")]:
        assert unpack(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    assert unpack(B=0) == 0 and unpack(L=0, ldb=0, ldg=0) == 0


@pytest.mark.parametrize("T", [0, 1, 2, 125, 333])
def test_parse_header_accepts_the_documented_image(T):
    from simwhisper_codec_amd import bitstream
    img = oracle_image(random_codes(T, T))
    assert len(img) == bitstream.image_bytes(T) and img[:12] == bitstream.header(T)
    for data in (img, bytearray(img), memoryview(img), img + b"trailing bytes are someone else's"):
        assert bitstream.parse_header(data, "a.swc") == T
    assert bitstream.parse_header(b"xyz" + img, "a.swc", offset=3) == T


def test_parse_header_rejects_what_it_must():
    from simwhisper_codec_amd import bitstream
    codes = random_codes(7, 1)
    good = oracle_image(codes)
    for bad, word in [(oracle_image(codes, magic=b"SWC2"), "not a SWC1"), (b"RIFF" + good[4:], "not a SWC1"), (good[:11], "not a SWC1"),
                      (b"", "not a SWC1"), (oracle_image(codes, groups=4), "unsupported"), (oracle_image(codes, groups=9), "unsupported"),
                      (oracle_image(codes, bits=10), "unsupported"), (oracle_image(codes, bits=12), "unsupported"),
                      (good[:-1], "truncated"), (good[:12], "truncated")]:
        with pytest.raises(ValueError, match=word) as e:
            bitstream.parse_header(bad, "dir/utt_17.swc")
        assert "dir/utt_17.swc" in str(e.value)          # the file is named
    with pytest.raises(ValueError, match="truncated"):   # one byte short at an offset, too
        bitstream.parse_header(good + good[:-1], "x", offset=len(good))


def test_a_concatenation_of_images_parses_sequentially():
    from oracle import bitstream_np
    from simwhisper_codec_amd import bitstream
    parts = [random_codes(5, 2), random_codes(0, 3), random_codes(131, 4)]
    shard = b"".join(oracle_image(c) for c in parts)
    pos, seen = 0, []
    while pos < len(shard):
        n = bitstream.parse_header(shard, "shard", offset=pos)
        payload = shard[pos + bitstream.HEADER_BYTES: pos + bitstream.image_bytes(n)]
        seen.append(bitstream_np.unpack(np.frombuffer(payload, dtype=np.uint8), n))
        pos += bitstream.image_bytes(n)
    assert pos == len(shard) and [s.shape[1] for s in seen] == [5, 0, 131]
    assert all(np.array_equal(s, c) for s, c in zip(seen, parts))


def test_cli_mode_flag():
    import inference
    p = inference.build_parser()
    assert vars(p.parse_args([]))["mode"] == "roundtrip"
    for mode in ("roundtrip", "encode", "decode"):
        assert vars(p.parse_args(["--mode", mode]))["mode"] == mode
    with pytest.raises(SystemExit):
        p.parse_args(["--mode", "transcode"])
    # every other default is what it was
    d = vars(p.parse_args([]))
    assert (d["batch_size"], d["in_flight"], d["resample"], d["precision"], d["device"]) == (8, 2, "host", "mixed", "cuda")


@pytest.mark.parametrize("mode", ["encode", "decode"])
def test_cli_single_gpu_modes_refuse_a_distributed_launch(mode, monkeypatch, tmp_path):
    """under torch.distributed.run a mode other than roundtrip exits with a message before any process group exists"""
    import torch.distributed as dist
    import inference
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(inference, "load_model", lambda *a, **k: pytest.fail("a model was loaded"))
    monkeypatch.setattr(inference, "main_distributed", lambda *a, **k: pytest.fail("the distributed loop was entered"))
    with pytest.raises(SystemExit) as e:
        inference.main(["--mode", mode, "--input_dir", str(tmp_path), "--output_dir", str(tmp_path / "out")])
    assert f"--mode {mode}" in str(e.value.code) and "one GPU" in str(e.value.code) and "WORLD_SIZE=2" in str(e.value.code)
    assert not dist.is_initialized() and not (tmp_path / "out").exists()
