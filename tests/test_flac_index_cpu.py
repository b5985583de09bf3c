"""swc_flac_index (csrc/swc_flac.c, include/swc_flac.h): the host half of the FLAC device path.  No entropy decoding — frames are
found by their headers and proved by CRC-8, CRC-16, frame number and the sample total — against what tests/flac_encode.py
wrote, plus the C-ABI of include/swc_flac.h (declarations == bindings == exported symbols, in the two libraries)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_encode as fe  # noqa: E402
import flac_streams as fs  # noqa: E402

from simwhisper_codec_amd import _lib, wavio  # noqa: E402

E_FORMAT, E_CRC, E_UNSUP, E_SPACE, E_HOSTONLY = -1, -2, -3, -4, -6


def _check_table(raw, tab, x, sr, bps, blocksize):
    got = wavio.flac_index(raw)
    assert not isinstance(got, int), got
    info, frames = got
    assert (info.rate, info.channels, info.bps, info.total, info.blocksize) == (sr, x.shape[1], bps, len(x), blocksize)
    assert len(frames) == len(tab)
    assert [(int(f["byte_off"]), int(f["n_bytes"]), int(f["first_sample"]), int(f["blocksize"])) for f in frames] == tab
    assert int(frames["blocksize"].sum()) == len(x) and not frames["file"].any() and not frames["reserved"].any()
    if len(tab):
        assert info.first_frame == tab[0][0]
    return info, frames


@pytest.mark.parametrize("blocksize", [16, 192, 1024, 4096])
def test_index_equals_what_the_encoder_wrote(blocksize):
    """offsets, lengths, first samples and block sizes, a short last block, 1 and 2 channels; the header fields that are
    passed on instead of re-parsed on the device"""
    for ch in (1, 2):
        x = fs.signal(3 * blocksize + min(17, blocksize - 1), ch, 16, seed=blocksize + ch)
        modes = [0, 8, 9, 10]
        raw, tab = fs.encode(x, 22050, 16, blocksize=blocksize,
                             plan=lambda fi, c: (modes[fi % 4] if c is None else dict(kind=("fixed", 2), porder=fi % 2)))
        info, frames = _check_table(raw, tab, x, 22050, 16, blocksize)
        assert len(frames) == 4 and int(frames["blocksize"][-1]) == min(17, blocksize - 1)
        assert list(frames["chan_assign"]) == ([0] * 4 if ch == 1 else [1, 8, 9, 10])
        for f in frames:   # hdr_bytes: sync 2 + codes 2 + number 1 + explicit block size 0 / 1 / 2 + CRC-8
            code = raw[int(f["byte_off"]) + 2] >> 4
            assert int(f["hdr_bytes"]) == 6 + (1 if code == 6 else 2 if code == 7 else 0)


def test_index_matrix_streams_and_id3_prefix():
    for name, x, sr, bps, raw, tab in fs.matrix():
        _check_table(raw, tab, x, sr, bps, 256 if name != "stereo_modes" else 192)
    x = fs.signal(1000, 2, 16, seed=1)
    raw, tab = fs.encode(x, 8000, 16, blocksize=256, id3=True)
    assert raw[:3] == b"ID3"
    _check_table(raw, tab, x, 8000, 16, 256)


def test_index_one_frame_and_zero_frames():
    x = fs.signal(100, 1, 16, seed=2)
    raw, tab = fs.encode(x, 16000, 16, blocksize=1024)
    info, frames = _check_table(raw, tab, x, 16000, 16, 1024)
    assert len(frames) == 1 and frames["byte_off"][0] + frames["n_bytes"][0] == len(raw)
    raw, tab = fs.encode(np.zeros((0, 1), dtype=np.int64), 16000, 16, blocksize=1024)
    info, frames = _check_table(raw, tab, np.zeros((0, 1), dtype=np.int64), 16000, 16, 1024)
    assert len(frames) == 0 and info.total == 0


def test_index_more_than_127_frames_uses_the_multi_byte_frame_number():
    x = fs.signal(16 * 140, 1, 8, seed=6)
    raw, tab = fs.encode(x, 16000, 8, blocksize=16, plan=lambda fi, c: 0 if c is None else dict(kind="verbatim"))
    info, frames = _check_table(raw, tab, x, 16000, 8, 16)
    assert int(frames["hdr_bytes"][127]) == 7 and int(frames["hdr_bytes"][128]) == 8


def test_a_false_sync_with_valid_crc8_and_frame_number_is_skipped():
    """a complete frame header — sync, valid codes, the FOLLOWING frame number, a correct CRC-8 — planted inside a VERBATIM
    subframe.  Only the running CRC-16 tells it from a frame start: the index must not cut the frame there."""
    bs = 64
    hdr = bytes([0xFF, 0xF8, (6 << 4) | 5, (0 << 4) | (4 << 1), 1, bs - 1])   # block size 8-bit explicit, 16 kHz, mono, 16 bit, frame 1
    hdr += bytes([fe.crc8(hdr)])
    x = fs.signal(3 * bs, 1, 16, seed=8)
    words = np.frombuffer(hdr + b"\x00", dtype=">i2").astype(np.int64)          # 4 samples that spell the header
    x[8:8 + len(words), 0] = words
    raw, tab = fs.encode(x, 16000, 16, blocksize=bs, plan=lambda fi, c: 0 if c is None else dict(kind="verbatim"))
    at = raw.find(hdr)
    assert tab[0][0] < at < tab[0][0] + tab[0][1], "the planted header must lie inside frame 0"
    _check_table(raw, tab, x, 16000, 16, bs)
    # and the host decoder agrees on the samples
    lib = wavio._io()
    out = np.empty((len(x), 1), dtype=np.int32)
    md5 = C.c_int32()
    assert lib.swc_flac_decode(raw, len(raw), out.ctypes.data_as(C.c_void_p), len(x), C.byref(md5)) == len(x)
    assert np.array_equal(out.astype(np.int64), x)


def test_a_flipped_bit_is_a_crc_error():
    x = fs.signal(4 * 256, 2, 16, seed=9)
    raw, tab = fs.encode(x, 16000, 16, blocksize=256)
    for k, where in ((0, 3), (1, tab[1][1] // 2), (3, tab[3][1] - 1), (2, 2)):   # header, subframes, the CRC-16 itself, header codes
        bad = bytearray(raw)
        bad[tab[k][0] + where] ^= 0x10
        assert wavio.flac_index(bytes(bad)) == E_CRC, (k, where)
    assert wavio.flac_index(raw[:-1]) == E_CRC and wavio.flac_index(raw[: tab[2][0] + 9]) in (E_CRC, E_FORMAT)
    assert wavio.flac_index(b"fLaC") == E_FORMAT and wavio.flac_index(b"RIFF" + bytes(64)) == E_FORMAT
    # a lost frame: every frame checks out, the total does not
    assert wavio.flac_index(raw[: tab[3][0]]) == E_FORMAT


def test_streams_that_stay_with_the_host_decoder(tmp_path):
    x = fs.signal(600, 1, 24, seed=3)
    raw = fe.encode(x, 16000, 24, blocksize=256)
    assert wavio.flac_index(raw) == E_HOSTONLY
    p = tmp_path / "a24.flac"
    p.write_bytes(raw)
    assert wavio.read_flac_raw(str(p)) is None
    pcm, sr, bits = wavio._decode_flac(str(p))                    # the host decoder takes it
    assert bits == 24 and np.array_equal(pcm.astype(np.int64), x)
    # STREAMINFO of a variable-block-size stream (min != max), and the blocking-strategy bit of a frame header
    x = fs.signal(512, 1, 16, seed=4)
    raw, tab = fs.encode(x, 16000, 16, blocksize=256)
    var = bytearray(raw); var[8:10] = (16).to_bytes(2, "big")
    assert wavio.flac_index(bytes(var)) == E_HOSTONLY
    var = bytearray(raw); var[tab[0][0] + 1] |= 1
    hl = tab[0][0] + 5
    var[hl] = fe.crc8(bytes(var[tab[0][0]:hl]))
    assert wavio.flac_index(bytes(var)) == E_HOSTONLY
    # a stream cut out of another: its frames are sound but do not count from 0 (frame k must carry the number k)
    x3 = fs.signal(3 * 256, 1, 16, seed=12)
    raw3, tab3 = fs.encode(x3, 16000, 16, blocksize=256, md5=False)
    cut = bytearray(raw3[: tab3[0][0]] + raw3[tab3[1][0]:])
    cut[8 + 14:8 + 18] = (2 * 256).to_bytes(4, "big")
    assert wavio.flac_index(bytes(cut)) == E_HOSTONLY
    p = tmp_path / "cut.flac"
    p.write_bytes(bytes(cut))
    pcm, sr, bits = wavio._decode_flac(str(p))                    # (the host decoder does not look at the numbers)
    assert np.array_equal(pcm.astype(np.int64), x3[256:])
    # a good 16-bit file comes back whole
    p = tmp_path / "ok.flac"
    p.write_bytes(raw)
    r = wavio.read_flac_raw(str(p))
    assert (r.rate, r.channels, r.bps, r.total, r.blocksize, len(r)) == (16000, 1, 16, 512, 256, 512)
    assert bytes(r.data) == raw and len(r.frames) == 2 and wavio.read_flac_raw(str(tmp_path / "x.wav")) is None


def test_a_crafted_total_cannot_size_anything(tmp_path, monkeypatch):
    """STREAMINFO's 36-bit total is attacker-controlled: beyond the ceiling of _decode_flac it is refused before any record
    buffer exists; under it, the buffers are sized by the FILE and the walk finds the stream short."""
    x = fs.signal(4096, 1, 16, seed=5)
    raw = bytearray(fe.encode(x, 16000, 16, blocksize=1024))
    q = 8
    raw[q + 13] |= 0x0F
    raw[q + 14:q + 18] = b"\xff\xff\xff\xff"
    sizes = []
    real = np.zeros
    monkeypatch.setattr(np, "zeros", lambda shape, *a, **k: (sizes.append(int(np.prod(shape))), real(shape, *a, **k))[1])
    p = tmp_path / "crafted.flac"
    p.write_bytes(bytes(raw))
    with pytest.raises(ValueError, match="ceiling"):
        wavio.read_flac_raw(str(p))
    assert not sizes
    assert wavio.flac_index(bytes(raw), max_samples=1 << 20) == E_SPACE                   # the C function refuses on its own, too
    assert max(sizes) <= max(16, len(raw) // 9 + 1)                                       # records sized by the file
    raw[q + 13] &= 0xF0
    raw[q + 14:q + 18] = (1 << 30).to_bytes(4, "big")
    p.write_bytes(bytes(raw))
    assert wavio.read_flac_raw(str(p)) is None and wavio.flac_index(bytes(raw)) == E_FORMAT
    assert sizes and max(sizes) <= max(16, len(raw) // 9 + 1)
    monkeypatch.setenv("SWC_FLAC_MAX_SECONDS", "0.1")             # 1 600 samples at 16 kHz
    p.write_bytes(fe.encode(x, 16000, 16, blocksize=1024))
    with pytest.raises(ValueError, match="ceiling"):
        wavio.read_flac_raw(str(p))
    # an undeclared total (0): the frames are counted against the ceiling as they come
    raw = bytearray(fe.encode(x, 16000, 16, blocksize=1024))
    raw[q + 13] &= 0xF0
    raw[q + 14:q + 18] = bytes(4)
    assert wavio.flac_index(bytes(raw)) == E_SPACE
    monkeypatch.delenv("SWC_FLAC_MAX_SECONDS")
    info, frames = wavio.flac_index(bytes(raw))
    assert info.total == 4096 and len(frames) == 4


def test_record_buffer_grows_from_the_count_the_walk_returns():
    x = fs.signal(16 * 60, 1, 8, seed=7)                          # 60 tiny frames: more than the first guess of 16 records
    raw, tab = fs.encode(x, 16000, 8, blocksize=16)
    assert len(raw) // 256 < 60
    info, frames = _check_table(raw, tab, x, 16000, 8, 16)
    lib = wavio._io()
    st = _lib.FlacStream()
    few = np.zeros(3, dtype=np.dtype(_lib.FlacFrame))
    assert lib.swc_flac_index(raw, len(raw), 1 << 20, C.byref(st), few.ctypes.data_as(C.c_void_p), 3) == 60
    assert np.array_equal(few, frames[:3])
    assert lib.swc_flac_index(raw, len(raw), 1 << 20, C.byref(st), None, 0) == 60


# ------------------------------------------------------------------------------------------------ the C-ABI of swc_flac.h
def _header_text():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "swc_flac.h")).read(), flags=re.S)


def test_flac_header_declarations_are_bound_and_exported():
    from simwhisper_codec_amd import build
    build.build_library()
    lib, io = _lib.load(), wavio._io()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(swc_\w+)\s*\(", _header_text(), flags=re.M))
    assert declared == {"swc_flac_index", "swc_flac_decode_workspace_bytes", "swc_flac_decode_batch", "swc_flac_decode_batch_ex"}
    assert declared == set(_lib.FLAC_SIGNATURES) | set(_lib.FLAC_IO_SIGNATURES)
    for table, so in ((_lib.FLAC_SIGNATURES, lib), (_lib.FLAC_IO_SIGNATURES, io)):
        for name, (argtypes, restype) in table.items():
            fn = getattr(so, name)
            assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    # parameter counts of the declarations equal the bindings'
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", _header_text(), flags=re.S):
        table = _lib.FLAC_SIGNATURES if m.group(1) in _lib.FLAC_SIGNATURES else _lib.FLAC_IO_SIGNATURES
        assert len(m.group(2).split(",")) == len(table[m.group(1)][0]), m.group(1)
    # the structs: field for field, and the sizes the tables are laid out with
    for cname, cls in (("swc_flac_frame", _lib.FlacFrame), ("swc_flac_file", _lib.FlacFile), ("swc_flac_stream", _lib.FlacStream)):
        body = re.search(r"typedef struct " + cname + r"\s*\{(.*?)\}\s*" + cname + r"\s*;", _header_text(), flags=re.S).group(1)
        fields = []
        for typ, names in re.findall(r"\b(int32_t|int64_t)\s+([\w\s,]+);", body):
            fields += [(n.strip(), C.c_int64 if typ == "int64_t" else C.c_int32) for n in names.split(",")]
        assert fields == list(cls._fields_), cname
    assert C.sizeof(_lib.FlacFrame) == 40 and C.sizeof(_lib.FlacFile) == 48
    # the header stays apart from the other tables; the new translation unit is part of the build and makes the library stale
    assert not declared & set(_lib.exported_symbols()) and not declared & set(_lib.CODES_SIGNATURES) and not declared & set(_lib.AUDIO_SIGNATURES)
    assert "swc_flac_gpu.hip" in build.SOURCES and "swc_flac.c" in build.IO_SOURCES
    text = _header_text()
    for name, val in (("SWC_FLAC_E_HOSTONLY", _lib.FLAC_E_HOSTONLY), ("SWC_FLAC_PLANE_ALIGN", _lib.FLAC_PLANE_ALIGN)):
        assert int(re.search(r"#define\s+" + name + r"\s+\(?(-?\d+)\)?", text).group(1)) == val
    assert {int(v) for v in re.findall(r"#define\s+SWC_FLAC_ST_\w+\s+(\d+)", text)} == set(_lib.FLAC_ST)


def test_workspace_layout_mirrors_the_c_arithmetic():
    from simwhisper_codec_amd import ops
    for ns, cs in (([], []), ([0], [1]), ([1], [1]), ([63, 64, 65], [1, 2, 8]), ([160000] * 5, [1, 2, 1, 2, 1]), ([4097, 0, 77], [2, 2, 1])):
        assert ops.flac_workspace_layout(ns, cs) == ops.flac_workspace_bytes(ns, cs)
        offs, total = ops.flac_workspace_layout(ns, cs)
        assert total % 256 == 0 and all(o % 64 == 0 for o in offs)
    with pytest.raises(_lib.SwcError):
        ops.flac_workspace_bytes([10], [9])
    with pytest.raises(_lib.SwcError):
        ops.flac_workspace_layout([10], [0])


def test_decode_batch_checks_its_arguments_before_any_launch():
    """no GPU here: every call below must return in the argument checks (a launch would fail differently)"""
    lib = _lib.load()
    P = C.c_void_p
    ok = dict(bytes=P(16), n_bytes=100, frames=P(16), n_frames=1, files=P(16), B=1, out=P(16), out_elems=10, status=P(16),
              ws=P(16), ws_bytes=256, fpw=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.swc_flac_decode_batch_ex(a["bytes"], a["n_bytes"], a["frames"], a["n_frames"], a["files"], a["B"], a["out"],
                                            a["out_elems"], a["status"], a["ws"], a["ws_bytes"], a["fpw"], P(0))
    for bad in (dict(n_frames=-1), dict(n_frames=(1 << 24) + 1), dict(B=-1), dict(B=65536), dict(n_bytes=-1), dict(out_elems=-1),
                dict(ws_bytes=-1), dict(fpw=3), dict(fpw=128), dict(fpw=-1), dict(ws=P(8)), dict(status=P(2)), dict(out=P(1)),
                dict(frames=P(4)), dict(files=P(4)), dict(bytes=P(0)), dict(frames=P(0)), dict(files=P(0)), dict(out=P(0)),
                dict(status=P(0)), dict(ws=P(0)), dict(B=0)):
        assert call(**bad) != 0, bad
        assert b"swc_flac_decode_batch" in lib.swc_last_error()
    # n_frames == 0 launches nothing, whatever the pointers are
    assert call(n_frames=0, bytes=P(0), frames=P(0), files=P(0), out=P(0), status=P(0), ws=P(0), B=0) == 0
    assert lib.swc_flac_decode_batch(P(0), 0, P(0), 0, P(0), 0, P(0), 0, P(0), P(0), 0, P(0)) == 0


def test_cli_flag(monkeypatch, tmp_path):
    """--flac: host by default; gpu needs a CUDA device and one process (refused before any process group or model exists)"""
    import inference
    args = inference.build_parser().parse_args([])
    assert args.flac == "host"
    assert inference.build_parser().parse_args(["--flac", "gpu"]).flac == "gpu"
    with pytest.raises(SystemExit):
        inference.build_parser().parse_args(["--flac", "device"])
    with pytest.raises(SystemExit, match="CUDA"):
        inference.main(["--flac", "gpu", "--device", "cpu", "--synthetic_checkpoint", "--input_dir", str(tmp_path), "--output_dir", str(tmp_path)])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="torch.distributed.run"):
        inference.main(["--flac", "gpu", "--synthetic_checkpoint", "--input_dir", str(tmp_path), "--output_dir", str(tmp_path)])
    # a loader thread hands FLAC files over raw only when asked to and when there is a device to decode them
    x = fs.signal(700, 1, 16, seed=11)
    p = tmp_path / "a.flac"
    p.write_bytes(fe.encode(x, 16000, 16, blocksize=256))
    assert isinstance(inference.load_file(str(p), 16000, True, "host", "gpu"), wavio.FlacRaw)
    for args in ((True, "host", "host"), (False, "host", "gpu"), (True, "gpu", "host")):
        got = inference.load_file(str(p), 16000, *args)
        assert isinstance(got, __import__("torch").Tensor) and got.shape == (700,)
    assert isinstance(inference.load_file(str(p), 16000, True, "host"), __import__("torch").Tensor)   # the signature of before
