"""The shared FLAC frame decoder (csrc/swc_flac_frame.h — the text the GPU kernel runs) compiled for the host and run as a
stand-alone program under AddressSanitizer and UBSan (simwhisper_codec_amd/build.py build_flac_check; a subprocess, nothing
preloaded).  Every frame is decoded from a heap block of exactly its bytes into planes of exactly its size, so a read outside
the frame or a store outside the planes ends the program with a report: this is where out-of-bounds behaviour is found, before
anything runs on a GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_streams as fs  # noqa: E402

REPORTS = ("AddressSanitizer", "runtime error", "LeakSanitizer", "UndefinedBehaviorSanitizer")


def _clean(rc, err):
    assert not any(r in err for r in REPORTS), err[-4000:]
    assert rc == 0, (rc, err[-2000:])


def test_the_program_is_built_with_the_sanitizers():
    from simwhisper_codec_amd import build
    exe = build.build_flac_check()
    blob = open(exe, "rb").read()
    assert b"__asan_init" in blob and b"__ubsan_handle" in blob
    assert b"__asan_init" not in open(build.build_flac_check(sanitize=False), "rb").read()


def test_valid_matrix_equals_the_host_decoder_and_the_original_pcm(tmp_path):
    """every subframe kind, 1 / 2 channels, 8 / 12 / 16 bits, wasted bits, Rice / Rice2, escape partitions, partition orders
    0 .. 8, LPC orders 1 / 12 / 32, every stereo mode: the planes (stereo undone) equal swc_flac_decode's samples (the
    program's verdict) and the PCM that was encoded (the dump), bit for bit, with every frame's status 0"""
    paths = {}
    for name, x, sr, bps, raw, tab in fs.matrix():
        p = tmp_path / f"{name}.flac"
        p.write_bytes(raw)
        paths[str(p)] = (name, x, tab)
    rc, res, err = fs.run_check(list(paths), dump=tmp_path)
    _clean(rc, err)
    assert set(res) == set(paths)
    for p, (name, x, tab) in paths.items():
        r = res[p]
        assert r["verdict"] == "equal" and r["index"] == len(tab) and r["status"] == [0] * len(tab) and int(r["host"]) == len(x), (name, r)
        got = np.fromfile(p + ".i32", dtype=np.int32).reshape(-1, x.shape[1])
        assert np.array_equal(got.astype(np.int64), x), name


def _first_subframe(raw, off, size, bps):
    """what the first subframe of the frame at raw[off] says of itself, read back bit by bit: -> dict(type, wasted, stereo,
    and for FIXED / LPC: method, porder, escape = the first partition is an escape partition)"""
    h = fs._hdr_len(raw, off)
    ca = raw[off + 3] >> 4
    bits = int.from_bytes(raw[off + h:off + size - 2], "big")
    total = 8 * (size - 2 - h)
    pos = 0

    def take(n):
        nonlocal pos
        v = (bits >> (total - pos - n)) & ((1 << n) - 1)
        pos += n
        return v
    assert take(1) == 0
    typ, wasted = take(6), 0
    if take(1):
        wasted = 1
        while not take(1):
            wasted += 1
    out = dict(type=typ, wasted=wasted, stereo=ca)
    width = bps + (1 if ca == 9 else 0) - wasted            # channel 0 is the side channel in side/right only
    order = typ - 8 if 8 <= typ <= 12 else (typ & 31) + 1 if typ >= 32 else None
    if order is None:
        return out
    take(order * width)
    if typ >= 32:
        prec = take(4) + 1
        take(5)
        take(order * prec)
    out["method"], out["porder"] = take(2), take(4)
    out["escape"] = take(5 if out["method"] else 4) == (31 if out["method"] else 15)
    return out


def test_the_matrix_holds_what_it_claims():
    """the plans reach the encoder as asked (it falls back to VERBATIM when a plan does not fit the block, without a word):
    subframe type codes, wasted-bit counts, channel assignments, and behind the warm-up samples of every FIXED / LPC
    subframe the residual method (Rice / Rice2), the partition order and whether the first partition is an escape partition
    are read back from the first subframe of every frame"""
    seen = []
    for name, x, sr, bps, raw, tab in fs.matrix():
        for off, size, first, bs in tab:
            if raw[off + 4] < 0x80:                           # (frame numbers below 128: the header length fs._hdr_len knows)
                seen.append(_first_subframe(raw, off, size, bps))
    types = {f["type"] for f in seen}
    assert {0, 1, 8, 9, 10, 11, 12, 32, 32 + 11, 32 + 31} <= types                       # every kind; LPC orders 1, 12, 32
    assert {f["wasted"] for f in seen} >= {0, 3} and {f["stereo"] for f in seen} >= {0, 1, 8, 9, 10}
    coded = [f for f in seen if "method" in f]
    assert {f["method"] for f in coded} == {0, 1}                                        # Rice and Rice2
    assert {f["porder"] for f in coded} >= set(range(9))                                 # partition orders 0 .. 8 (block size 256)
    assert {(f["method"], f["escape"]) for f in coded} == {(0, False), (0, True), (1, False), (1, True)}
    assert any(f["wasted"] and f["escape"] for f in coded) and any(f["type"] >= 32 and f["escape"] for f in coded)


def test_damaged_streams_end_with_a_status_or_the_host_samples(tmp_path):
    """bits flipped, frames cut short, reserved and inconsistent codes patched in — all resealed with a fresh CRC-16 so that
    the index accepts them.  Each must end with a non-zero status, or with the host decoder's samples; never with a
    sanitizer report (rc 0 also says: no stream had all statuses 0 and other samples than the host decoder)."""
    paths = {}
    for name, raw in fs.damaged_set():
        p = tmp_path / f"{name}.flac"
        p.write_bytes(raw)
        paths[str(p)] = name
    assert len(paths) >= 60 and set(fs.GPU_DAMAGED) <= set(paths.values())
    rc, res, err = fs.run_check(list(paths))
    _clean(rc, err)
    assert set(res) == set(paths)
    verdicts = {paths[p]: r["verdict"] for p, r in res.items()}
    assert set(verdicts.values()) <= {"status", "equal"}, {k: v for k, v in verdicts.items() if v not in ("status", "equal")}
    by = {paths[p]: r for p, r in res.items()}
    # the patched codes get the status the header documents (SWC_FLAC_ST_*), in frame 0, and the other frames stay 0
    for name, want in (("m16_type_reserved", 2), ("m16_type_reserved13", 2), ("m16_padding_bit", 2), ("m16_method2", 2), ("m16_method3", 2),
                       ("m16_porder15", 3), ("m16_porder8", 3), ("m16_porder9", 3), ("m8_porder4", 3), ("m8_porder5", 3), ("m8_lpc32", 3),
                       ("s12_type_reserved", 2)):
        assert by[name]["status"][0] == want and not any(by[name]["status"][1:]), (name, by[name])
    for name in ("m16_cut0", "m16_cut1", "m16_cut2", "s12_cut0", "s12_cut1", "s12_cut2"):
        assert by[name]["verdict"] == "status", (name, by[name])
    assert sum(v == "status" for v in verdicts.values()) >= 40
    # the sanitizer-free host build (what the GPU tests compare with) says the same, word for word
    rc2, res2, _ = fs.run_check(list(paths), sanitize=False)
    assert rc2 == 0 and {p: r["status"] for p, r in res2.items()} == {p: r["status"] for p, r in res.items()}
