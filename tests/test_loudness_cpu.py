"""swc_loudness and swc_loudness_normalise (BS.1770 / R128 loudness), the parts that need no GPU: the C-ABI of
include/swc_loudness.h (declarations == bindings == exports, a table apart from the other ten; every argument check before any
launch; the workspace arithmetic against its documented formula), the K-weighting against the table of BS.1770, properties of
the numpy restatement (tests/loudness_ref.py) on signals whose answer is known, the refusals of the Python surface and the flags
of the tools."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loudness_ref as ref  # noqa: E402

NAMES = {"swc_loudness", "swc_loudness_normalise", "swc_loudness_workspace_bytes", "swc_loudness_coefficients"}
BS1770_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              -1.99004745483398, 0.99007225036621)   # shelf b0 b1 b2 a1 a2, high-pass a1 a2


def _header(name="swc_loudness.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


def test_loudness_header_declarations_are_bound():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    declared = _declared("swc_loudness.h")
    assert declared == NAMES == set(_lib.LOUDNESS_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)                       # exported by the library
        argtypes, restype = _lib.LOUDNESS_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    seen = set()
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        assert len(m.group(2).split(",")) == len(_lib.LOUDNESS_SIGNATURES[m.group(1)][0]), m.group(1)
        seen.add(m.group(1))
    assert seen == declared
    assert [len(_lib.LOUDNESS_SIGNATURES[n][0]) for n in sorted(NAMES)] == [13, 2, 12, 3]


def test_loudness_table_is_apart_from_the_other_ten():
    from simwhisper_codec_amd import _lib
    mine = set(_lib.LOUDNESS_SIGNATURES)
    assert not mine & set(_lib.exported_symbols())
    for other in (_lib.SIGNATURES, _lib.PLAIN, _lib.AUDIO_SIGNATURES, _lib.CODES_SIGNATURES, _lib.METRICS_SIGNATURES,
                  _lib.QUALITY_SIGNATURES, _lib.FLAC_SIGNATURES, _lib.FLAC_IO_SIGNATURES, _lib.FLAC_ENC_SIGNATURES,
                  _lib.SPECTRAL_SIGNATURES, _lib.PITCH_SIGNATURES, _lib.ALIGN_SIGNATURES, _lib.MCD_SIGNATURES):
        assert not mine & set(other)
    for h in ("swc.h", "swc_audio.h", "swc_codes.h", "swc_metrics.h", "swc_quality.h", "swc_flac.h", "swc_flac_enc.h", "swc_spectral.h",
              "swc_pitch.h", "swc_align.h", "swc_mcd.h"):
        assert not mine & _declared(h)
        assert "swc_loudness" not in _header(h)


def test_constants_agree_with_the_header_and_the_reference():
    from simwhisper_codec_amd import _lib, metrics, ops
    hdr = _header()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert (val("SWC_LOUDNESS_MIN_FS"), val("SWC_LOUDNESS_MAX_FS")) == (_lib.LOUDNESS_MIN_FS, _lib.LOUDNESS_MAX_FS) == (8000, 48000)
    assert val("SWC_LOUDNESS_MAX_N") == _lib.LOUDNESS_MAX_N == 1 << 30
    assert val("SWC_LOUDNESS_VALUES") == _lib.LOUDNESS_VALUES == len(ops.LOUDNESS_VALUES) == len(ref.KEYS) == len(metrics.LOUDNESS_KEYS) == 8
    assert val("SWC_LOUDNESS_MAX_WIDTH") == _lib.LOUDNESS_MAX_WIDTH and val("SWC_LOUDNESS_GROUP") == _lib.LOUDNESS_GROUP == 64
    assert (val("SWC_LOUDNESS_UNMEASURED"), val("SWC_LOUDNESS_PEAK_LIMITED")) == (_lib.LOUDNESS_UNMEASURED, _lib.LOUDNESS_PEAK_LIMITED) \
        == (ref.UNMEASURED, ref.PEAK_LIMITED) == (1, 2)
    assert ops.LOUDNESS_VALUES == ref.KEYS
    for i, k in enumerate(("I", "LRA", "MOMENTARY_MAX", "SHORT_TERM_MAX", "SAMPLE_PEAK", "TRUE_PEAK", "BLOCKS", "BLOCKS_KEPT")):
        assert val("SWC_LOUDNESS_" + k) == i
    assert "Bits" in hdr and "depend on its samples, fs and the table only" in hdr


def test_build_sees_the_new_object_and_a_touched_header(monkeypatch):
    from simwhisper_codec_amd import build
    build.build_library()
    assert not build._stale()
    assert "swc_loudness.hip" in build.SOURCES
    hdr = os.path.join(ROOT, "include", "swc_loudness.h")
    real = os.path.getmtime
    newer = real(build.LIB_PATH) + 10
    monkeypatch.setattr(os.path, "getmtime", lambda p: newer if os.path.abspath(p) == hdr else real(p))
    assert build._stale()


def _aligned_buffer():
    raw = (C.c_char * 1024)()
    base = C.addressof(raw)
    return raw, C.c_void_p((base + 255) & ~255)


def test_loudness_arg_checks_without_gpu():
    """every check happens before any launch: host pointers that are never dereferenced stand in for device memory"""
    from simwhisper_codec_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_buffer()

    def call(rows=p, n_in=p, max_n=160000, fs=16000, width=7, taps=p, start=p, run=15, values=p, ws=p, ws_bytes=1 << 50, B=2):
        return lib.swc_loudness(rows, n_in, max_n, fs, width, taps, start, run, values, ws, ws_bytes, B, None)

    need = lib.swc_loudness_workspace_bytes(2, 160000, 16000)
    up = lambda v: (v + 255) & ~255
    assert need == up(2 * 2 * 4) + up(2 * 100 * 4 * 8) + 2 * up(2 * 100 * 8)
    assert lib.swc_loudness_workspace_bytes(0, 0, 8000) == 0 and lib.swc_loudness_workspace_bytes(1, 1599, 16000) == up(8)
    for bad in ((-1, 10, 16000), (65536, 10, 16000), (1, -1, 16000), (1, (1 << 30) + 1, 16000), (1, 10, 11025), (1, 10, 7990),
                (1, 10, 48010), (1, 10, 0)):
        assert lib.swc_loudness_workspace_bytes(*bad) == -1, bad
    odd = C.c_void_p(p.value + 4)
    for kw, word in [(dict(rows=None), b"null"), (dict(n_in=None), b"null"), (dict(taps=None), b"null"), (dict(start=None), b"null"),
                     (dict(values=None), b"null"), (dict(ws=None), b"null"), (dict(B=65536), b"B="), (dict(B=-1), b"B="),
                     (dict(max_n=-1), b"max_n_in"), (dict(max_n=(1 << 30) + 1), b"max_n_in"),
                     (dict(fs=11025), b"fs="), (dict(fs=7990), b"fs="), (dict(fs=48010), b"fs="), (dict(fs=16001), b"fs="),
                     (dict(width=-1), b"width"), (dict(width=65), b"width"), (dict(run=0), b"run="), (dict(run=16), b"run="),
                     (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"), (dict(ws=odd), b"aligned")]:
        assert call(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    # nothing to do: no launch, no device needed; 22050 and 44100 pass where 11025 does not
    for fs in (8000, 16000, 22050, 44100, 48000):
        assert call(B=0, fs=fs) == 0
    assert call(B=0, max_n=0, ws_bytes=0) == 0 and call(B=0, max_n=1 << 30) == 0

    def norm(rows=p, n_in=p, values=p, target=-23.0, ceiling=-1.0, out=p, ld=100, cols=100, gains=p, flags=p, B=2):
        return lib.swc_loudness_normalise(rows, n_in, values, target, ceiling, out, ld, cols, gains, flags, B, None)

    for kw, word in [(dict(rows=None), b"null"), (dict(n_in=None), b"null"), (dict(values=None), b"null"),
                     (dict(out=None, gains=None, flags=None), b"no output"), (dict(B=65536), b"B="), (dict(B=-1), b"B="),
                     (dict(target=math.nan), b"finite"), (dict(ceiling=math.inf), b"finite"), (dict(cols=101), b"cols"),
                     (dict(cols=-1), b"cols")]:
        assert norm(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    assert norm(B=0) == 0 and norm(B=0, out=None) == 0 and norm(B=0, gains=None, flags=None, cols=0) == 0
    del keep


def test_python_surface_refuses_what_it_cannot_do():
    from simwhisper_codec_amd import _lib, metrics, ops
    x = torch.zeros(9000)
    for fs in (11025, 7990, 48010, 96000, 16000.5, "fast"):
        with pytest.raises(_lib.SwcError, match="sample_rate"):
            metrics.loudness([x], sample_rate=fs)
        with pytest.raises(_lib.SwcError, match="sample_rate"):
            metrics.normalised([x], fs)
        with pytest.raises(_lib.SwcError, match="sample_rate"):
            metrics.level_matched([x], [x], fs)
        with pytest.raises(_lib.SwcError, match="sample_rate"):
            metrics.spectral([x], [x], sample_rate=fs, level="loudness")
    with pytest.raises(_lib.SwcError, match="want="):
        metrics.loudness([x], want=("pesq",))
    with pytest.raises(_lib.SwcError, match="CPU"):
        metrics.loudness([x], device="cpu")
    with pytest.raises(_lib.SwcError, match="CPU"):
        metrics.normalised([x], 16000, device="cpu")
    with pytest.raises(_lib.SwcError, match="level="):
        metrics.spectral([x], [x], level="rms")
    with pytest.raises(_lib.SwcError, match="rows"):
        ops.loudness([], 16000)                 # B = 0 is refused before anything is launched
    with pytest.raises(_lib.SwcError, match="rows"):
        ops.loudness_normalise([], torch.zeros(0, 8, dtype=torch.float64))
    for fs in (22050, 44100, 8000, 48000):
        assert ops.loudness_check_rate(fs) == fs and ref.rate_ok(fs)
    assert not ref.rate_ok(11025) and not ref.rate_ok(7990)


# ---- the definition ----

def test_coefficients_at_48_khz_are_the_table_of_bs1770():
    from simwhisper_codec_amd import ops
    k = ops.loudness_coefficients(48000)
    got = k[:5] + k[8:]
    assert max(abs(a - b) for a, b in zip(got, BS1770_48K)) <= 1e-12
    assert k[5:8] == [1.0, -2.0, 1.0]
    b1, a1, b2, a2 = ref.coefficients(48000)
    mine = list(b1) + list(a1[1:]) + list(a2[1:])
    assert max(abs(a - b) for a, b in zip(mine, BS1770_48K)) <= 1e-12 and a1[0] == a2[0] == 1.0 and list(b2) == [1.0, -2.0, 1.0]
    # the library's host arithmetic and the reference's: two statements of one text
    for fs in (8000, 16000, 22050, 44100, 48000):
        kk = ops.loudness_coefficients(fs)
        b1, a1, b2, a2 = ref.coefficients(fs)
        assert np.allclose(kk, np.concatenate([b1, a1[1:], b2, a2[1:]]), rtol=0, atol=1e-14)
    # the pole radius of the high-pass the header quotes: no short lead-in can stand for the filter's memory
    assert abs(math.sqrt(ref.coefficients(48000)[3][2]) - 0.9950) < 1e-4 and abs(math.sqrt(ref.coefficients(8000)[3][2]) - 0.9705) < 1e-4


def _sine(fs, seconds, freq, amp=1.0, phase=0.0):
    t = np.arange(int(round(seconds * fs)), dtype=np.float64) / fs
    return (amp * np.sin(2.0 * math.pi * freq * t + phase)).astype(np.float32)


def test_full_scale_997_hz_sine_reads_minus_3_01():
    r = ref.measure(_sine(48000, 5.0, 997.0), 48000, with_true_peak=False)
    assert abs(r["integrated"] - (-3.01)) <= 0.01
    assert r["blocks"] == 47 and r["blocks_kept"] == 47 and abs(r["momentary_max"] + 3.01) <= 0.01 and abs(r["short_term_max"] + 3.01) <= 0.01
    assert abs(r["range"]) < 1e-6 and abs(r["sample_peak"] - 1.0) < 1e-3


def test_relative_gate_drops_the_quiet_half():
    fs = 16000
    x = np.concatenate([_sine(fs, 4.0, 1000.0, 10 ** (-26 / 20)), _sine(fs, 4.0, 1000.0, 10 ** (-46 / 20))])
    z = ref.energies(x, fs)
    e = ref.block_energies(z, 4)
    l, gamma, keep = ref.gates(e, -10.0)
    assert len(e) == 77 and (l > ref.ABS_GATE).all()          # every block passes the absolute gate: the relative one decides
    quiet = np.arange(len(e)) >= 40                             # blocks made of the second half only
    assert not keep[quiet].any() and keep[:37].all()
    assert l[quiet].max() < gamma < l[:37].min()
    r = ref.measure(x, fs, with_true_peak=False)
    assert r["blocks_kept"] == keep.sum() < r["blocks"] == 77
    assert r["integrated"] == float(ref.loud(e[keep].mean()))   # the loudness of the kept blocks alone
    assert abs(r["integrated"] - float(ref.loud(e[:37].mean()))) < 0.2 and r["integrated"] > float(ref.loud(e.mean())) + 2.0
    assert ref.gate_margin(x, fs) > 1e-6


def test_percentile_indices():
    assert [ref.percentile_indices(n) for n in (1, 2, 10, 11)] == [(0, 0), (0, 1), (1, 9), (1, 10)]
    for n in range(1, 400):
        lo, hi = ref.percentile_indices(n)
        assert 0 <= lo <= hi <= n - 1


def test_edges_of_the_reference():
    fs = 8000
    L = fs // 10
    x = _sine(fs, 4.0, 440.0, 0.1)
    for n, blocks in ((0, 0), (L - 1, 0), (4 * L - 1, 0), (4 * L, 1), (30 * L - 1, 26), (30 * L, 27)):
        r = ref.measure(x[:n], fs, with_true_peak=False)
        assert r["blocks"] == blocks
        assert math.isnan(r["integrated"]) == (blocks == 0) and math.isnan(r["momentary_max"]) == (blocks == 0)
        assert math.isnan(r["range"]) == (n < 30 * L) and math.isnan(r["short_term_max"]) == (n < 30 * L)
    r = ref.measure(np.zeros(4 * fs, np.float32), fs, with_true_peak=False)    # every block fails the absolute gate
    assert r["blocks"] == 37 and r["blocks_kept"] == 0 and math.isnan(r["integrated"]) and math.isnan(r["range"])
    assert r["momentary_max"] == -math.inf and r["sample_peak"] == 0.0
    assert ref.gain(math.nan, 0.5) == (1.0, 1) and ref.gain(-20.0, 0.0) == (1.0, 1)
    g, f = ref.gain(-30.0, 0.5)
    assert f == 2 and g == 10 ** (-1 / 20) / 0.5 and ref.gain(-20.0, 0.5) == (10 ** (-3 / 20), 0)


# ---- tools ----

def test_cli_flags_parse_and_defaults_are_unchanged():
    import inference
    a = vars(inference.build_parser().parse_args([]))
    assert a["loudness"] is None and a["true_peak_db"] == -1.0
    assert a["mode"] == "roundtrip" and a["resample"] == "host" and a["flac"] == "host" and a["output_format"] == "wav" and a["in_flight"] == 2
    a = vars(inference.build_parser().parse_args(["--loudness", "-23", "--true_peak_db", "-2.5", "--mode", "encode"]))
    assert a["loudness"] == -23.0 and a["true_peak_db"] == -2.5 and a["mode"] == "encode"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_spectral
    import measure_loudness
    base = ["--original_dir", "A", "--synthesized_dir", "B"]
    assert vars(evaluate_spectral.build_parser().parse_args(base))["level_match"] is False
    assert vars(evaluate_spectral.build_parser().parse_args(base + ["--level_match"]))["level_match"] is True
    a = vars(measure_loudness.build_parser().parse_args(["--input_dir", "D"]))
    assert a["sample_rate"] == 16000 and a["batch_size"] == 32
    with pytest.raises(SystemExit):
        measure_loudness.build_parser().parse_args([])
    nan = math.nan
    rows = [dict.fromkeys(measure_loudness.COLUMNS, -20.0), dict(dict.fromkeys(measure_loudness.COLUMNS, nan), true_peak_db=-60.0),
            dict.fromkeys(measure_loudness.COLUMNS, -30.0)]
    means, out = measure_loudness.summarise(["a", "b", "c"], rows)
    assert out == ["b"] and means["integrated"] == -25.0
    assert "not measured" in measure_loudness.format_line("b", rows[1]) and "-20.00 LUFS" in measure_loudness.format_line("a", rows[0])
    readme = open(os.path.join(ROOT, "tools", "README.md")).read()
    assert "measure_loudness.py" in readme and "bench_loudness.py" in readme
