"""swc_quality (STOI + ESTOI + SI-SDR in one call), the parts that need no GPU: the C-ABI of include/swc_quality.h (declarations
== bindings, a table apart from the other four; argument checks before any launch), the workspace layout against its Python
mirror, and the properties of the float64 restatement (tests/quality_ref.py) that tests/test_quality_gpu.py holds the kernels
to."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quality_ref  # noqa: E402
import stoi_ref  # noqa: E402


def _header(name="swc_quality.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


def test_quality_header_declarations_are_bound():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    declared = _declared("swc_quality.h")
    assert declared == {"swc_quality", "swc_quality_workspace_bytes"} == set(_lib.QUALITY_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)
        argtypes, restype = _lib.QUALITY_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    seen = set()
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        assert len(m.group(2).split(",")) == len(_lib.QUALITY_SIGNATURES[m.group(1)][0]), m.group(1)
        seen.add(m.group(1))
    assert seen == declared
    # swc_metrics.h keeps declaring swc_stoi alone
    assert _declared("swc_metrics.h") == {"swc_stoi", "swc_stoi_workspace_bytes"} == set(_lib.METRICS_SIGNATURES)


def test_quality_table_is_apart_from_the_other_four():
    from simwhisper_codec_amd import _lib
    mine = set(_lib.QUALITY_SIGNATURES)
    assert not mine & set(_lib.exported_symbols())
    for other in (_lib.SIGNATURES, _lib.PLAIN, _lib.AUDIO_SIGNATURES, _lib.CODES_SIGNATURES, _lib.METRICS_SIGNATURES):
        assert not mine & set(other)
    for h in ("swc.h", "swc_audio.h", "swc_codes.h", "swc_metrics.h"):
        assert not mine & _declared(h)
        assert "swc_quality" not in _header(h)


def test_constants_agree_with_the_header():
    from simwhisper_codec_amd import _lib
    hdr = _header()
    assert int(re.search(r"#define SWC_ESTOI_GROUP (\d+)", hdr).group(1)) == _lib.ESTOI_GROUP >= 1
    chunk = int(re.search(r"#define SWC_SISDR_CHUNK (\d+)", hdr).group(1))
    assert chunk == _lib.SISDR_CHUNK and chunk % 1024 == 0      # 256 threads x groups of 4 samples


def test_build_sees_a_touched_quality_header(monkeypatch):
    from simwhisper_codec_amd import build
    build.build_library()
    assert not build._stale()
    hdr = os.path.join(ROOT, "include", "swc_quality.h")
    real = os.path.getmtime
    newer = real(build.LIB_PATH) + 10
    monkeypatch.setattr(os.path, "getmtime", lambda p: newer if os.path.abspath(p) == hdr else real(p))
    assert build._stale()


def _aligned_buffer():
    raw = (C.c_char * 1024)()
    base = C.addressof(raw)
    return raw, C.c_void_p((base + 255) & ~255)


def test_arg_checks_without_gpu():
    """every check happens before any launch: host pointers that are never dereferenced stand in for device memory"""
    from simwhisper_codec_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_buffer()
    need = lib.swc_quality_workspace_bytes(2, 9000, 8, 5)
    assert need > lib.swc_stoi_workspace_bytes(2, 9000, 8, 5) > 0

    def call(x=p, y=p, n_in=p, max_n=9000, orig=8, new=5, width=58, taps=p, start=p, run=117, stoi=p, estoi=p, segs=p, si_sdr=p,
             ws=p, ws_bytes=need, B=2):
        return lib.swc_quality(x, y, n_in, max_n, orig, new, width, taps, start, run, stoi, estoi, segs, si_sdr, ws, ws_bytes, B, None)

    odd = C.c_void_p(p.value + 4)
    need441 = lib.swc_quality_workspace_bytes(2, 9000, 441, 100)
    assert need441 > 0
    for kw, word in [(dict(x=None), b"null"), (dict(y=None), b"null"), (dict(n_in=None), b"null"), (dict(taps=None), b"null"),
                     (dict(start=None), b"null"), (dict(ws=None), b"null"),
                     (dict(taps=None, estoi=None, si_sdr=None), b"null"), (dict(start=None, stoi=None, si_sdr=None), b"null"),
                     (dict(stoi=None, estoi=None, si_sdr=None), b"no output"),
                     (dict(B=-1), b"B="), (dict(B=65536), b"B="), (dict(orig=0), b"rates"), (dict(new=0), b"rates"),
                     (dict(stoi=None, estoi=None, orig=0), b"rates"),
                     (dict(max_n=-1), b"max_n_in"), (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"),
                     (dict(stoi=None, estoi=None, ws_bytes=need - 1), b"workspace"),
                     (dict(ws=odd), b"aligned"), (dict(run=0), b"table size"),
                     (dict(orig=441, new=100, width=160, run=320, ws_bytes=need441), b"does not fit"),
                     (dict(orig=441, new=100, width=160, run=320, ws_bytes=need441, stoi=None, si_sdr=None), b"does not fit"),
                     (dict(orig=441, new=100, width=160, run=320, ws_bytes=need441, B=0), b"does not fit")]:
        assert call(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    # nothing to do: no launch, no device needed.  Each output alone, segs or not; SI-SDR alone needs neither the table nor
    # a ratio the resampler can do
    assert call(B=0) == 0
    assert call(B=0, segs=None) == 0
    assert call(B=0, estoi=None, si_sdr=None) == 0 and call(B=0, stoi=None, si_sdr=None) == 0
    assert call(B=0, stoi=None, estoi=None, segs=None, taps=None, start=None) == 0
    assert call(B=0, stoi=None, estoi=None, segs=None, taps=None, start=None, orig=441, new=100, width=160, run=320,
                ws_bytes=need441) == 0
    del keep


def test_workspace_bytes_and_its_python_mirror():
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    chunk = _lib.SISDR_CHUNK
    for B, n, o, w in [(1, 0, 8, 5), (1, 255, 1, 1), (1, 256, 1, 1), (3, 9000, 8, 5), (32, 160000, 8, 5), (4, 48000, 24, 5),
                       (2, 7000, 4, 5), (2, chunk, 1, 1), (2, chunk + 1, 1, 1), (5, 441000, 441, 100), (1, 3968, 1, 1), (1, 4096, 1, 1)]:
        Q = ops.quality_workspace_layout(B, n, o, w)
        S = ops.stoi_workspace_layout(B, n, o, w)
        assert lib.swc_quality_workspace_bytes(B, n, o, w) == Q["total"] == ops.quality_workspace_bytes(B, n, o, w)
        for k, v in S.items():                                   # the names it shares with the STOI layout keep their offsets
            if k != "total":
                assert Q[k] == v, k
        assert Q["eseg"] == S["total"] and Q["Smax"] == max(S["Mmax"] - 29, 0) and Q["chunks"] == math.ceil(n / chunk)
        order = [Q[k] for k in ("eseg", "rec", "stat", "segs", "total")]
        assert order == sorted(order) and all(v % 256 == 0 for v in order)
        assert Q["rec"] - Q["eseg"] >= 4 * B * Q["Smax"] and Q["stat"] - Q["rec"] >= 32 * B * Q["chunks"]
        assert Q["segs"] - Q["stat"] >= 32 * B and Q["total"] - Q["segs"] >= 4 * B
    for bad in [(-1, 10, 8, 5), (65536, 10, 8, 5), (1, -1, 8, 5), (1, 10, 0, 5), (1, 10, 8, 0)]:
        assert lib.swc_quality_workspace_bytes(*bad) == -1
        with pytest.raises(_lib.SwcError):
            ops.quality_workspace_bytes(*bad)


# ---- the float64 restatement ----

X = stoi_ref.harmonic(18000, 16000)


def test_estoi_identity_and_scale_invariance():
    r = quality_ref.estoi(X, X, 16000)
    assert abs(r["d"] - 1.0) <= 1e-9 and r["segs"] == stoi_ref.frames_at_10k(18000, 16000) - 29
    y = stoi_ref.add_noise(X, 5).astype(np.float64)
    base = quality_ref.estoi(X, y, 16000)
    assert 0.0 < base["d"] < 1.0 and base["min_col_norm"] > 0
    for c in (0.25, 3.0):
        assert abs(quality_ref.estoi(X, c * y, 16000)["d"] - base["d"]) <= 1e-12


def test_estoi_decreases_with_the_snr_and_stays_under_stoi():
    ds = []
    for snr in stoi_ref.SNRS:
        y = stoi_ref.add_noise(X, snr)
        e, s = quality_ref.estoi(X, y, 16000), stoi_ref.stoi(X, y, 16000)
        assert e["segs"] == s["segs"] and np.array_equal(e["kept"], s["kept"]) and e["margin"] == s["margin"]
        assert e["d"] <= s["d"], (snr, e["d"], s["d"])
        ds.append(e["d"])
    print("ESTOI over", stoi_ref.SNRS, "dB:", ["%.4f" % d for d in ds])
    assert all(a > b for a, b in zip(ds, ds[1:])), ds
    assert ds[0] < 1.0 and ds[-1] > 0.0


@pytest.mark.parametrize("fs", [8000, 10000, 16000])
def test_estoi_boundary_lengths(fs):
    n29, n30 = stoi_ref.boundary_lengths(fs)
    x = stoi_ref.harmonic(n30, fs)
    y = stoi_ref.add_noise(x, 10)
    short, one = quality_ref.estoi(x[:n29], y[:n29], fs), quality_ref.estoi(x, y, fs)
    assert (short["segs"], short["d"]) == (0, 1e-5) and len(short["kept"]) == 30 and short["min_col_norm"] == math.inf
    assert one["segs"] == 1 and 0.0 < one["d"] < 1.0 and len(one["kept"]) == 31 and one["min_col_norm"] < math.inf
    assert quality_ref.estoi(x[:0], y[:0], fs)["segs"] == 0 and quality_ref.estoi(x[:100], y[:100], fs)["d"] == 1e-5


def test_si_sdr_of_a_scaled_and_shifted_copy():
    """y = c x + d is x up to what the measure ignores.  The contract's ratio is (Et + EPS) / (En + EPS), so the value cannot
    exceed 10 log10(Et / EPS + 1): 250 dB needs Et > 2.2e9.  The property is therefore checked on the signal at a scale of
    2^20, where that cap is ~296 dB; at unit scale (Et ~ 1e2, cap ~177 dB) the value must sit on the cap."""
    x = X.astype(np.float64)
    for c, d in ((0.25, 0.1), (3.0, -0.2)):
        big = x * 2.0 ** 20
        assert quality_ref.si_sdr(big, c * big + d * 2.0 ** 20) > 250.0
        xc = x - x.mean()
        cap = 10.0 * math.log10((c * c * float(xc @ xc) + stoi_ref.EPS) / stoi_ref.EPS)
        v = quality_ref.si_sdr(x, c * x + d)
        assert 150.0 < v <= cap + 1e-9 and cap - v <= 1e-6, (v, cap)


def test_si_sdr_of_an_orthogonal_distortion_is_its_level():
    x = X.astype(np.float64)
    xc = x - x.mean()
    z = np.random.default_rng(5).standard_normal(len(x))
    basis = np.stack([np.ones(len(x)) / math.sqrt(len(x)), xc / np.linalg.norm(xc)])
    for _ in range(2):                                    # twice: what the first round leaves is rounding
        z = z - basis.T @ (basis @ z)
    assert abs(z.sum()) <= 1e-9 and abs(z @ xc) <= 1e-9
    for c, d, k in ((0.25, 0.1, 0.1), (3.0, -0.2, 1e-3), (1.0, 0.0, 2.0)):
        want = -20.0 * math.log10(k * np.linalg.norm(z) / np.linalg.norm(xc))
        assert abs(quality_ref.si_sdr(x, c * (x + k * z) + d) - want) <= 1e-9, (c, d, k)


def test_si_sdr_of_an_empty_pair_is_nan():
    assert math.isnan(quality_ref.si_sdr(np.zeros(0), np.zeros(0)))
    assert math.isnan(quality_ref.si_sdr(X, np.zeros(0)))
    assert math.isfinite(quality_ref.si_sdr(X[:1], X[:1]))     # one sample: x' = 0, the ratio is EPS / EPS


def test_python_surface_refuses_what_it_cannot_do():
    import torch
    from simwhisper_codec_amd import _lib, metrics
    x = torch.zeros(9000)
    with pytest.raises(_lib.SwcError, match="CPU"):
        metrics.quality([x], [x], device="cpu")
    with pytest.raises(_lib.SwcError, match="1 reference and 2"):
        metrics.quality([x], [x, x], device="cuda")
    with pytest.raises(_lib.SwcError, match="44100"):
        metrics.stoi_table(44100, "cpu")


def test_tool_parser_and_summary():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_quality
    a = vars(evaluate_quality.build_parser().parse_args(["--original_dir", "A", "--synthesized_dir", "B"]))
    assert a["sample_rate"] == 16000 and a["batch_size"] >= 1 and a["verbose"] is False
    nan = float("nan")
    m = evaluate_quality.summarise(["a", "b", "c", "d"], [0.5, 1e-5, 0.7006, 1e-5], [0.25, 1e-5, 0.5, 1e-5], [3, 0, 1, 0],
                                   [10.0, 20.0, -4.0, nan])
    assert m["stoi"] == pytest.approx(0.6003, abs=1e-12) and m["estoi"] == pytest.approx(0.375, abs=1e-12)
    assert m["si_sdr"] == pytest.approx(26.0 / 3, abs=1e-12) and m["short"] == ["b", "d"] and m["empty"] == ["d"]
    m = evaluate_quality.summarise(["a"], [1e-5], [1e-5], [0], [nan])
    assert (m["stoi"], m["estoi"], m["si_sdr"], m["short"], m["empty"]) == (None, None, None, ["a"], ["a"])
