"""swc_flac_encode_batch on the device (include/swc_flac_enc.h, csrc/swc_flac_enc.hip): the file bytes equal those of the numpy
reference tests/flac_fixed_ref.py (which tests/test_flac_enc_cpu.py proves against the host decoder), for every length, block
size, choice of the search, frame-number width and rate; batches, alignments and the memory contract; every image decodes
through swc_flac_index + the device decoder; HostStager.flac_to_host and `inference.py --output_format flac`."""
import functools
import hashlib
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_enc_cases as cases  # noqa: E402
import flac_fixed_ref as ref  # noqa: E402
import poison  # noqa: E402
from common import PARAMS  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def expected(key, rate, bs, md5=True):
    """the reference's bytes of signal `key`, computed once and shared"""
    return ref.encode(signal(key), rate, bs, md5=md5)


@functools.lru_cache(maxsize=None)
def signal(key):
    kind, arg = key
    if kind == "cov":
        return cases.coverage_cases()[arg][0]
    if kind == "len":
        return cases.speech_like(arg, arg) if arg else np.zeros(0, dtype=np.int16)
    if kind == "long":
        return cases.speech_like(arg, 5)
    raise KeyError(key)


def place(x, shift=0):
    """the samples on the device, `shift` elements behind a 16-byte boundary"""
    buf = torch.zeros(len(x) + 8 + shift, dtype=torch.int16, device=DEV)
    assert buf.data_ptr() % 16 == 0
    row = buf[shift:shift + len(x)]
    row.copy_(torch.from_numpy(np.asarray(x, dtype=np.int16)))
    return row


def encode(xs, rate=16000, bs=256, md5=True, shifts=None, **kw):
    """-> (list of file bytes, offsets, sizes, buffer)"""
    from simwhisper_codec_amd import ops
    rows = [place(x, 0 if shifts is None else shifts[i]) for i, x in enumerate(xs)]
    buf, off, sizes = ops.flac_encode(rows, rate, blocksize=bs, md5=md5, **kw)
    torch.cuda.synchronize()
    off, sizes, host = off.cpu().tolist(), sizes.cpu().tolist(), buf.cpu().numpy()
    return [host[o:o + s].tobytes() for o, s in zip(off, sizes)], off, sizes, buf


def check(keys, rate=16000, bs=256, md5=True, **kw):
    files, off, sizes, _ = encode([signal(k) for k in keys], rate, bs, md5, **kw)
    pos = 0
    for k, f, o, s in zip(keys, files, off, sizes):
        want = expected(k, rate, bs, md5) if len(signal(k)) else b""
        assert (o, s) == (pos, len(want)), (k, o, s)                   # back to back, in row order
        assert f == want, (k, next(i for i in range(len(f)) if f[i] != want[i]))
        pos += s
    return files


@pytest.mark.parametrize("bs", cases.BLOCK_SIZES)
def test_lengths_at_every_block_size(bs):
    keys = [("len", n) for n in cases.LENGTHS + (bs, bs + 1)]
    files = check(keys, bs=bs)
    for k, f in zip(keys, files):   # 27/28 and 31/32 samples: the MD5 padding boundaries at 54/56 and 62/64 bytes
        assert f[26:42] == hashlib.md5(np.asarray(signal(k), dtype="<i2").tobytes()).digest(), k


def test_every_choice_of_the_search():
    c = cases.coverage_cases()
    for bs in cases.BLOCK_SIZES:
        names = [n for n in c if c[n][1] == bs]
        check([("cov", n) for n in names], bs=bs)


@pytest.mark.parametrize("n", [129 * 256 + 1, 2049 * 256])
def test_frame_numbers_across_the_coding_widths(n):
    """frame numbers 127 / 128 (one and two bytes) and 2047 / 2048 (two and three)"""
    check([("long", n)], bs=256)


def test_rates_and_the_md5_switch():
    keys = [("len", n) for n in (1, 27, 28, 257)] + [("cov", "speech")]
    for rate in (16000, 11025):   # a table code, and the 16-bit field
        with_md5 = check(keys, rate=rate, bs=1024)
        without = check(keys, rate=rate, bs=1024, md5=False)
        for a, b in zip(with_md5, without):   # exactly the 16 signature bytes change
            assert len(a) == len(b) and a[:26] == b[:26] and a[42:] == b[42:] and b[26:42] == bytes(16) and a[26:42] != bytes(16)
    from simwhisper_codec_amd import _lib
    for bad in (0, 70000):
        with pytest.raises(_lib.SwcError):
            encode([signal(("len", 5))], rate=bad)
    with pytest.raises(_lib.SwcError):
        encode([signal(("len", 5))], bs=300)


MIXED = [("len", 257), ("len", 1), ("cov", "stepped_p5"), ("len", 0), ("len", 31), ("cov", "alternation"), ("len", 256),
         ("len", 2), ("cov", "constant_zero"), ("len", 28), ("cov", "ramp")]


@pytest.mark.parametrize("B", [1, 3, 33])
def test_batches_with_mixed_lengths_and_an_empty_row(B):
    keys = [MIXED[(i * 4 + 3) % len(MIXED)] for i in range(B)] if B > 1 else [("len", 257)]
    assert B == 1 or ("len", 0) in keys
    check(keys, bs=256)


def test_a_file_does_not_depend_on_its_place_alignment_or_max_n():
    keys = [("cov", "speech"), ("len", 255), ("cov", "sine_mid"), ("len", 5)]
    want = [expected(k, 16000, 512) for k in keys]
    for shift in range(8):   # rows 0 .. 7 elements behind a 16-byte boundary
        files = encode([signal(k) for k in keys], bs=512, shifts=[shift, (shift + 3) % 8, (shift + 5) % 8, 7 - shift])[0]
        assert files == want, shift
    assert encode([signal(k) for k in keys[::-1]], bs=512)[0] == want[::-1]
    for i, k in enumerate(keys):
        assert encode([signal(k)], bs=512)[0] == [want[i]]
        assert encode([signal(k)], bs=512, max_n=10000)[0] == [want[i]]
    assert encode([signal(k) for k in keys], bs=512, max_n=5 * 512 + 1)[0] == want


def test_memory_contract():
    """out and the workspace in guarded windows, two fills: nothing outside [0, total) and the workspace is written, and the
    bytes do not depend on what the buffers held"""
    from simwhisper_codec_amd import ops
    keys = [("len", 257), ("cov", "stepped_p6_short"), ("len", 4), ("cov", "alternation")]
    xs = [signal(k) for k in keys]
    want = b"".join(expected(k, 16000, 256) for k in keys)
    max_n = max(len(x) for x in xs)
    ws_bytes, cap = ops.flac_encode_workspace_layout([max_n] * len(xs), 256)
    assert len(want) < cap
    for fill in (0x00, 0xFF):
        out, check_out = poison.guarded((cap,), torch.uint8, device=DEV)
        ws, check_ws = poison.guarded((ws_bytes,), torch.uint8, device=DEV)
        out.fill_(fill)
        ws.fill_(fill)
        assert ws.data_ptr() % 16 == 0
        rows = [place(x, i) for i, x in enumerate(xs)]
        buf, off, sizes = ops.flac_encode(rows, 16000, blocksize=256, out=out, workspace=ws)
        torch.cuda.synchronize()
        check_out()
        check_ws()
        host = out.cpu().numpy()
        total = int(sizes.sum())
        assert host[:total].tobytes() == want, fill
        assert (host[total:] == fill).all(), "a store behind the last image"
        assert off.cpu().tolist() == np.cumsum([0] + sizes.cpu().tolist()[:-1]).tolist()
    # too small a buffer or workspace is refused before any launch
    from simwhisper_codec_amd import _lib
    with pytest.raises(_lib.SwcError):
        ops.flac_encode([place(xs[0])], 16000, blocksize=256, out=torch.zeros(ref.worst_case_bytes(257, 256) - 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.SwcError):
        ops.flac_encode([place(xs[0])], 16000, blocksize=256, workspace=torch.zeros(256, dtype=torch.uint8, device=DEV))


def test_images_decode_on_the_device(tmp_path):
    """every image through swc_flac_index + ops.flac_decode (HostStager.to_device_flac), the device decoder"""
    from simwhisper_codec_amd import wavio
    from simwhisper_codec_amd.pipeline import HostStager
    c = cases.coverage_cases()
    keys = [("cov", n) for n in c] + [("len", n) for n in (1, 2, 5, 255, 257)]
    raws = []
    for bs in cases.BLOCK_SIZES:
        ks = [k for k in keys if (c[k[1]][1] if k[0] == "cov" else 256) == bs]
        for k, f in zip(ks, encode([signal(k) for k in ks], bs=bs)[0]):
            p = tmp_path / f"{len(raws)}.flac"
            p.write_bytes(f)
            raw = wavio.read_flac_raw(str(p))
            assert raw is not None and raw.total == len(signal(k)), k
            raws.append((k, raw))
    views, failed = HostStager().to_device_flac([r for _, r in raws], torch.device("cuda", torch.cuda.current_device()), 16000)
    torch.cuda.synchronize()
    assert failed() == []
    for (k, _), v in zip(raws, views):
        assert torch.equal(v.cpu(), torch.from_numpy(signal(k).astype(np.float32) / 32768.0)), k


def test_flac_to_host():
    from simwhisper_codec_amd.pipeline import HostStager
    keys = [("cov", "speech"), ("len", 257), ("len", 27)]
    padded = torch.zeros(3, 3000, dtype=torch.int16, device=DEV)   # rows of one padded buffer, as pcm16_on_device returns them
    rows = []
    for i, k in enumerate(keys):
        x = signal(k)
        padded[i, :len(x)].copy_(torch.from_numpy(x))
        rows.append(padded[i, :len(x)])
    stager = HostStager()
    for md5 in (True, False):
        images = stager.flac_to_host(rows, 16000, md5=md5)
        assert [bytes(im.numpy()) for im in images] == [expected(k, 16000, 4096, md5) for k in keys]
        assert all(im.is_pinned() or im._base.is_pinned() for im in images)
    assert stager.flac_to_host([], 16000) == []
    with pytest.raises(ValueError, match="empty"):
        stager.flac_to_host([rows[0], padded[1, :0]], 16000)


def _write_wav(path, pcm, sr):
    raw = np.asarray(pcm, dtype="<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16)
                + b"data" + struct.pack("<I", len(raw)) + raw)


def test_cli_output_format_flac(tmp_path):
    """--output_format flac in --mode roundtrip and --mode decode: the decoded samples of the .flac files are the data of the
    .wav files of the same run with --output_format wav, which are the files the default writes"""
    import yaml
    import inference
    from simwhisper_codec_amd import wavio
    cfg = tmp_path / "tiny.yaml"
    cfg.write_text(yaml.safe_dump({"generator_params": PARAMS["tiny"]()}))
    ind = tmp_path / "in"
    ind.mkdir()
    names = ["a", "b", "c"]
    for i, (name, n) in enumerate(zip(names, [9000, 5000, 7777])):
        _write_wav(str(ind / f"{name}.wav"), cases.speech_like(n, 80 + i), 16000)
    common = ["--config_path", str(cfg), "--synthetic_checkpoint", "--device", "cuda", "--batch_size", "2", "--precision", "mixed"]
    out = {k: tmp_path / k for k in ("rt_default", "rt_wav", "rt_flac", "rt_nomd5", "swc", "dec_default", "dec_wav", "dec_flac")}
    inference.main(common + ["--input_dir", str(ind), "--output_dir", str(out["rt_default"])])
    inference.main(common + ["--output_format", "wav", "--input_dir", str(ind), "--output_dir", str(out["rt_wav"])])
    inference.main(common + ["--output_format", "flac", "--input_dir", str(ind), "--output_dir", str(out["rt_flac"])])
    inference.main(common + ["--output_format", "flac", "--flac_md5", "none", "--input_dir", str(ind), "--output_dir", str(out["rt_nomd5"])])
    inference.main(common + ["--mode", "encode", "--input_dir", str(ind), "--output_dir", str(out["swc"])])
    inference.main(common + ["--mode", "decode", "--input_dir", str(out["swc"]), "--output_dir", str(out["dec_default"])])
    inference.main(common + ["--mode", "decode", "--output_format", "wav", "--input_dir", str(out["swc"]), "--output_dir", str(out["dec_wav"])])
    inference.main(common + ["--mode", "decode", "--output_format", "flac", "--input_dir", str(out["swc"]), "--output_dir", str(out["dec_flac"])])
    for mode in ("rt", "dec"):
        assert sorted(os.listdir(out[f"{mode}_flac"])) == [f"{n}.flac" for n in names]
        assert sorted(os.listdir(out[f"{mode}_wav"])) == sorted(os.listdir(out[f"{mode}_default"])) == [f"{n}.wav" for n in names]
        for n in names:
            wav = (out[f"{mode}_wav"] / f"{n}.wav").read_bytes()
            assert wav == (out[f"{mode}_default"] / f"{n}.wav").read_bytes(), n
            pcm, sr = wavio.read_pcm(str(out[f"{mode}_wav"] / f"{n}.wav"))
            got, rate, bits = wavio._decode_flac(str(out[f"{mode}_flac"] / f"{n}.flac"))   # checks both CRCs and the MD5
            assert rate == sr and bits == 16 and np.array_equal(got.reshape(-1), pcm.numpy().reshape(-1).astype(np.int32)), (mode, n)
    for n in names:
        a, b = (out["rt_flac"] / f"{n}.flac").read_bytes(), (out["rt_nomd5"] / f"{n}.flac").read_bytes()
        assert a[:26] == b[:26] and a[42:] == b[42:] and b[26:42] == bytes(16) and a[26:42] != bytes(16)
    with pytest.raises(SystemExit, match="code files"):
        inference.main(common + ["--mode", "encode", "--output_format", "flac", "--input_dir", str(ind), "--output_dir", str(out["swc"])])
