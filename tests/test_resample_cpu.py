"""Sample-rate conversion, the parts that need no GPU: the C-ABI of include/swc_audio.h (declarations == bindings ==
exported symbols, argument checks before any launch), the filter table wavio.resample_taps / its packed form, the float64
reference every value check of tests/test_resample_gpu.py uses (resample_reference below), and wavio.read_pcm."""
import ctypes as C
import math
import os
import re
import struct
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PAIRS = [(8000, 16000), (11025, 16000), (22050, 16000), (24000, 16000), (32000, 16000), (44100, 16000), (48000, 16000),
         (16000, 24000), (16000, 48000)]


def resample_reference(x, orig_freq, new_freq):
    """THE reference: the formula of include/swc_audio.h evaluated in float64 from the f32 table and f32 mono input.
    -> (y64 [n_out] float64, mag [n_out] float64 = sum_t |K[p][t]| |xpad[...]|, nnz = largest non-zero tap count of a phase)"""
    from simwhisper_codec_amd import wavio
    K, orig, new, width = wavio.resample_taps(orig_freq, new_freq)
    taps = K.shape[1]
    assert taps == 2 * width + orig and K.dtype == torch.float32 and K.shape[0] == new
    x = x.reshape(-1)
    assert x.dtype == torch.float32
    n = x.numel()
    n_out = -(-new * n // orig)
    frames = -(-n_out // new) if n_out else 0
    xpad = torch.zeros(width + max(n, 0) + frames * orig + taps, dtype=torch.float64)
    xpad[width:width + n] = x.double()
    K64 = K.double()
    y = torch.zeros(frames, new, dtype=torch.float64)
    mag = torch.zeros(frames, new, dtype=torch.float64)
    if frames:
        win = xpad[: (frames - 1) * orig + taps].unfold(0, taps, orig)      # [frames, taps]: xpad[f * orig + t]
        assert win.shape[0] == frames
        y = win @ K64.T
        mag = win.abs() @ K64.abs().T
    nnz = int((K != 0).sum(dim=1).max())
    return y.reshape(-1)[:n_out], mag.reshape(-1)[:n_out], nnz


def bound(mag, nnz):
    """|y - y64| <= (nnz + 1) 2^-24 sum |K| |x|: an f32 dot product of nnz terms in any order, fused or not"""
    return (nnz + 1) * 2.0 ** -24 * mag


def _declared():
    hdr = open(os.path.join(ROOT, "include", "swc_audio.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


def test_audio_header_declarations_are_bound_and_exported():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    declared = _declared()
    assert declared and "swc_resample" in declared
    assert declared == set(_lib.AUDIO_SIGNATURES), declared ^ set(_lib.AUDIO_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)
        argtypes, restype = _lib.AUDIO_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    # the two headers stay apart: swc.h's table (and the tests that pin it) do not know the audio symbols
    assert not declared & set(_lib.exported_symbols())
    swc_h = open(os.path.join(ROOT, "include", "swc.h")).read()
    assert "swc_resample" not in swc_h


def test_every_audio_output_entry_point_has_a_memory_contract_test():
    """the guarantee tests/test_poison_cpu.py gives include/swc.h, for include/swc_audio.h: every declaration with a device
    output pointer is exercised in a guarded window by tests/test_resample_gpu.py"""
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "swc_audio.h")).read(), flags=re.S)
    outs = []
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        params = [p.strip() for p in m.group(2).split(",")]
        if any("*" in p and not re.search(r"\bstream$", p) and not p.startswith("const") for p in params):
            outs.append(m.group(1))
    assert outs == ["swc_resample"]
    src = open(os.path.join(ROOT, "tests", "test_resample_gpu.py")).read()
    assert "poison.guarded" in src and "ops.resample(" in src and "def test_memory_contract" in src


def test_out_len_helper():
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    for n, o, w in [(0, 3, 2), (1, 3, 2), (2, 3, 2), (3, 3, 2), (240001, 24000, 16000), (5, 1, 3), (441, 441, 160), (442, 441, 160)]:
        assert lib.swc_resample_out_len(n, o, w) == math.ceil(w * n / o) == ops.resample_out_len(n, o, w)
    assert lib.swc_resample_out_len(-5, 3, 2) == 0 and lib.swc_resample_out_len(5, 0, 2) == -1


def test_arg_checks_without_gpu():
    """every check happens before any launch: host pointers that are never dereferenced stand in for device memory"""
    from simwhisper_codec_amd import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p)

    def call(rows=p, n_in=p, fmt=_lib.PCM_F32, ch=1, orig=3, new=2, width=10, taps=p, start=p, run=19, out=p, ld=64, cols=64, B=1):
        return lib.swc_resample(rows, n_in, fmt, ch, orig, new, width, taps, start, run, out, ld, cols, B, None)

    for kw, word in [(dict(rows=None), b"null"), (dict(n_in=None), b"null"), (dict(taps=None), b"null"), (dict(start=None), b"null"),
                     (dict(out=None), b"null"), (dict(orig=0), b"rates"), (dict(new=0), b"rates"), (dict(fmt=7), b"in_format"),
                     (dict(fmt=_lib.PCM_I16, ch=0), b"ch="), (dict(fmt=_lib.PCM_I16, ch=9), b"ch="), (dict(ch=2), b"ch="),
                     (dict(cols=65), b"cols"), (dict(cols=-1), b"cols"), (dict(run=0), b"table size"), (dict(run=24), b"table size"),
                     (dict(B=-1), b"B="), (dict(B=65536), b"B="), (dict(width=-1), b"out of range"),
                     (dict(orig=30011, new=30013, width=7, run=13), b"does not fit")]:
        assert call(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    # nothing to do: no launch, no device needed
    assert call(B=0) == 0 and call(cols=0) == 0


@pytest.mark.parametrize("orig_freq,new_freq", PAIRS)
def test_taps_feed_resample_and_the_packed_table(orig_freq, new_freq):
    from simwhisper_codec_amd import ops, wavio
    K, orig, new, width = wavio.resample_taps(orig_freq, new_freq)
    g = math.gcd(orig_freq, new_freq)
    assert (orig, new) == (orig_freq // g, new_freq // g) and width == math.ceil(6 * orig / (min(orig, new) * 0.99))
    assert K.shape == (new, 2 * width + orig) and K.dtype == torch.float32
    # resample == a direct restatement with this table (same bits)
    x = torch.randn(3 * orig_freq // 10 + 7, generator=torch.Generator().manual_seed(orig_freq))
    padded = torch.nn.functional.pad(x.reshape(1, 1, -1), (width, width + orig))
    want = torch.nn.functional.conv1d(padded, K[:, None, :], stride=orig).transpose(1, 2).reshape(-1)
    want = want[: math.ceil(new * x.numel() / orig)]
    got = wavio.resample(x, orig_freq, new_freq)
    assert torch.equal(got, want)
    # the packed table holds every non-zero tap at its place, and only zeros are left out
    t = ops.resample_table(orig_freq, new_freq, "cpu")
    assert (t["orig"], t["new"], t["width"]) == (orig, new, width) and t["taps"].shape == (new, t["run"])
    R = torch.zeros_like(K)
    for p in range(new):
        s = int(t["start"][p])
        assert 0 <= s <= K.shape[1] - t["run"]
        R[p, s:s + t["run"]] = t["taps"][p]
    assert torch.equal(R, K)
    assert t["nnz"] == int((K != 0).sum(1).max()) <= t["run"]
    assert ops.resample_table(orig_freq, new_freq, "cpu") is t        # built once


@pytest.mark.parametrize("orig_freq,new_freq", PAIRS)
def test_host_resample_is_inside_the_derived_bound_of_the_reference(orig_freq, new_freq):
    """the float64 reference and its bound, checked against the host implementation (which sums ALL taps, zeros included):
    the bound the GPU kernel is held to is not a measured tolerance, and the reference is not the kernel's own output"""
    from simwhisper_codec_amd import wavio
    g = torch.Generator().manual_seed(new_freq + orig_freq)
    x = (torch.randn(2 * orig_freq // 5 + 13, generator=g) * 0.3).clamp(-1, 1)
    y64, mag, nnz = resample_reference(x, orig_freq, new_freq)
    y = wavio.resample(x, orig_freq, new_freq)
    assert y.shape == y64.shape and y.numel() == math.ceil(new_freq * x.numel() / orig_freq)
    taps = wavio.resample_taps(orig_freq, new_freq)[0].shape[1]
    assert ((y.double() - y64).abs() <= bound(mag, taps)).all()
    # and the bound has teeth: a dropped tap is outside it almost everywhere
    K, orig, new, width = wavio.resample_taps(orig_freq, new_freq)
    Kd = K.clone()
    Kd[torch.arange(new), K.abs().argmax(dim=1)] = 0
    padded = torch.nn.functional.pad(x.reshape(1, 1, -1), (width, width + orig))
    bad = torch.nn.functional.conv1d(padded, Kd[:, None, :], stride=orig).transpose(1, 2).reshape(-1)[: y.numel()]
    assert ((bad.double() - y64).abs() > bound(mag, nnz)).float().mean() > 0.9


def _wav_bytes(tag, ch, sr, bits, raw):
    return (b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
            struct.pack("<IHHIIHH", 16, tag, ch, sr, sr * ch * bits // 8, ch * bits // 8, bits) + b"data" + struct.pack("<I", len(raw)) + raw)


@pytest.mark.parametrize("sr", [24000, 44100])
@pytest.mark.parametrize("ch", [1, 2])
def test_read_pcm_returns_the_files_integers(tmp_path, sr, ch):
    from simwhisper_codec_amd import wavio
    rng = np.random.default_rng(sr + ch)
    pcm = rng.integers(-32768, 32768, size=(1237, ch), dtype=np.int16)
    path = str(tmp_path / "a.wav")
    open(path, "wb").write(_wav_bytes(1, ch, sr, 16, pcm.astype("<i2").tobytes()))
    got = wavio.read_pcm(path)
    assert got is not None
    x, rate = got
    assert rate == sr and x.dtype == torch.int16 and tuple(x.shape) == (1237, ch) and np.array_equal(x.numpy(), pcm)
    if ch == 1:
        assert torch.equal(wavio.read_pcm16(path, sr), x[:, 0]) and wavio.read_pcm16(path, 16000) is None
    else:
        assert wavio.read_pcm16(path, sr) is None


def test_read_pcm_leaves_other_formats_to_the_host(tmp_path):
    import flac_encode
    from simwhisper_codec_amd import wavio
    f = str(tmp_path / "f.wav")
    open(f, "wb").write(_wav_bytes(3, 1, 24000, 32, np.linspace(-1, 1, 100, dtype="<f4").tobytes()))
    b24 = str(tmp_path / "b24.wav")
    open(b24, "wb").write(_wav_bytes(1, 1, 24000, 24, bytes(300)))
    fl = str(tmp_path / "c.flac")
    open(fl, "wb").write(flac_encode.encode(np.arange(-500, 500, dtype=np.int64).reshape(-1, 1), 24000, 16, blocksize=256))
    notwav = str(tmp_path / "junk.wav")
    open(notwav, "wb").write(b"not a riff file at all")
    for path in (f, b24, fl, notwav):
        assert wavio.read_pcm(path) is None
    assert wavio.load_audio(f, 24000).shape == (1, 1, 100)             # ... and the host path still reads them
    assert wavio.load_audio(fl, 24000).shape == (1, 1, 1000)


def test_cli_has_the_resample_flag_with_the_host_default():
    import inference
    p = inference.build_parser()
    assert vars(p.parse_args([]))["resample"] == "host"
    assert vars(p.parse_args(["--resample", "gpu"]))["resample"] == "gpu"
    with pytest.raises(SystemExit):
        p.parse_args(["--resample", "elsewhere"])
