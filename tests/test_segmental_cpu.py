"""swc_segmental (include/swc_segmental.h), the parts that need no GPU: the C-ABI (declarations == bindings == exports, a table
apart from every other; every argument check before any launch; the workspace arithmetic against its documented formula), the
numpy restatement (tests/segmental_ref.py) against independent closed forms (Levinson against a Toeplitz solver, the LPC
cepstrum against the real cepstrum of 1 / A(z) from a long FFT, the two segmental SNRs of a scaled copy, the power-of-two
scalings, K95, the selection formula, frames with digital silence), the refusals of the Python surface and the tool's flags."""
import ctypes as C
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import segmental_ref as ref  # noqa: E402

NAMES = {"swc_segmental_workspace_bytes", "swc_segmental"}


# ---- ABI and arguments ----

def _header(name="swc_segmental.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


def test_segmental_header_declarations_are_bound():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    declared = _declared("swc_segmental.h")
    assert declared == NAMES == set(_lib.SEGMENTAL_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)                       # exported by the library
        argtypes, restype = _lib.SEGMENTAL_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    seen = set()
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        assert len(m.group(2).split(",")) == len(_lib.SEGMENTAL_SIGNATURES[m.group(1)][0]), m.group(1)
        seen.add(m.group(1))
    assert seen == declared
    assert [len(_lib.SEGMENTAL_SIGNATURES[n][0]) for n in sorted(NAMES)] == [19, 5]


def test_segmental_table_is_apart_from_every_other():
    from simwhisper_codec_amd import _lib
    mine = set(_lib.SEGMENTAL_SIGNATURES)
    assert not mine & set(_lib.exported_symbols())
    others = [v for k, v in vars(_lib).items() if (k.endswith("SIGNATURES") or k == "PLAIN") and k != "SEGMENTAL_SIGNATURES"]
    assert len(others) >= 15
    for other in others:
        assert not mine & set(other)
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "swc_segmental.h":
            assert not mine & _declared(h), h
            assert "swc_segmental" not in _header(h), h
    assert _declared("swc_spectral.h") == {"swc_spectral", "swc_spectral_workspace_bytes"}      # nothing was added there


def test_constants_agree_with_the_header_and_the_reference():
    from simwhisper_codec_amd import _lib, ops
    hdr = _header()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert (val("SWC_SEGMENTAL_MIN_WIN"), val("SWC_SEGMENTAL_MAX_WIN")) == (_lib.SEGMENTAL_MIN_WIN, _lib.SEGMENTAL_MAX_WIN) == (64, 2048)
    assert ops.SEGMENTAL_WINDOWS == tuple(w for w in _lib.SPECTRAL_WINDOWS if w >= 64)
    assert (val("SWC_SEGMENTAL_MAX_ORDER"), val("SWC_SEGMENTAL_MAX_BANDS")) == (_lib.SEGMENTAL_MAX_ORDER, _lib.SEGMENTAL_MAX_BANDS) == (32, 64)
    assert (val("SWC_SEGMENTAL_VALUES"), val("SWC_SEGMENTAL_MEASURES")) == (_lib.SEGMENTAL_VALUES, _lib.SEGMENTAL_MEASURES) == (8, 5)
    order = ("LLR", "IS", "CD", "SEGSNR", "FWSEGSNR", "FRAMES", "FRAMES_LPC", "FRAMES_FW")
    assert [val("SWC_SEGMENTAL_" + n) for n in order] == list(range(8))
    assert tuple(n.lower() for n in order) == ops.SEGMENTAL_VALUES == ref.VALUES
    assert "4.342944819032518" in hdr and ref.DB == 4.342944819032518 and abs(ref.DB - 10.0 / math.log(10.0)) < 1e-15
    assert ref.CORR == 1.0 + 1.0 / 1048576.0
    flat = " ".join(hdr.replace(" *", " ").split())
    for words in ("NOT normalised to unit sum", "the window is a power of two", "2^-20 correction", "depend on its samples, W, P, K and the band table only",
                  "Identical rows give exactly llr 0, is 0, cd 0, segsnr 35 and fwsegsnr 35", "NOT Levinson's E"):
        assert words in flat, words


def test_build_sees_a_touched_segmental_header(monkeypatch):
    from simwhisper_codec_amd import build
    build.build_library()
    assert not build._stale()
    assert "swc_segmental.hip" in build.SOURCES and build.EXTRA_FLAGS["swc_segmental.hip"] == ["-ffp-contract=off"]
    hdr = os.path.join(ROOT, "include", "swc_segmental.h")
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
    err = lib.swc_last_error

    def seg(x=p, y=p, n=p, max_n=9000, W=512, P=16, K=25, first=p, count=p, off=p, w=p, w_len=100, vals=p, track=p, ld_t=70, ws=p,
            ws_bytes=1 << 40, B=2):
        return lib.swc_segmental(x, y, n, max_n, W, P, K, first, count, off, w, w_len, vals, track, ld_t, ws, ws_bytes, B, None)

    need = lib.swc_segmental_workspace_bytes(2, 9000, 512, 16, 25)
    assert need == ref.workspace_bytes(2, 9000, 512, 16) > 0
    odd = C.c_void_p(p.value + 4)
    for kw, word in [(dict(x=None), b"null"), (dict(y=None), b"null"), (dict(n=None), b"null"), (dict(vals=None), b"null"), (dict(ws=None), b"null"),
                     (dict(B=65536), b"B="), (dict(B=-1), b"B="), (dict(max_n=-1), b"out of range"),
                     (dict(W=32), b"window"), (dict(W=4096), b"window"), (dict(W=500), b"window"), (dict(W=0), b"window"),
                     (dict(P=0), b"order"), (dict(P=33), b"order"), (dict(K=-1), b"bands"), (dict(K=65), b"bands"),
                     (dict(w_len=-1), b"fb_w_len"), (dict(ld_t=-1), b"ld_t"), (dict(max_n=1 << 44, W=64), b"frames"),
                     (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"), (dict(ws=odd), b"aligned")]:
        assert seg(**kw) == -1, kw
        assert word in err(), (kw, err())
    assert seg(B=0) == 0 and seg(B=0, ws_bytes=lib.swc_segmental_workspace_bytes(0, 9000, 512, 16, 25)) == 0
    assert seg(B=0, track=None, ld_t=-5) == 0                            # the stride does not matter without its output
    assert seg(B=0, K=0, first=None, count=None, off=None, w=None, w_len=0) == 0
    assert seg(B=0, first=None) == 0                                     # a null band table: no fwSegSNR work, not an error
    assert seg(B=0, W=64, P=1, K=64, max_n=0) == 0 and seg(B=0, W=2048, P=32) == 0
    del keep


LAYOUT_CASES = [(1, 0, 64, 1, 0), (1, 63, 64, 1, 0), (1, 64, 64, 1, 1), (3, 9000, 512, 16, 25), (32, 160000, 512, 16, 25), (33, 48000, 2048, 32, 64),
                (0, 5000, 256, 10, 0), (65535, 1 << 22, 64, 32, 64), (5, 2047, 2048, 10, 3), (2, 2048 + 511, 2048, 10, 3), (2, 2048 + 512, 2048, 10, 3)]


def test_workspace_bytes_and_frame_counts_against_the_documented_formula():
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    for B, n, W, P, K in LAYOUT_CASES:
        assert lib.swc_segmental_workspace_bytes(B, n, W, P, K) == ref.workspace_bytes(B, n, W, P) == ops.segmental_workspace_bytes(B, n, W, P, K), (B, n, W)
        assert ops.segmental_frames(n, W) == ref.frames(n, W) == (0 if n < W else len(range(0, n - W + 1, W // 4)))
    for bad in [(-1, 10, 64, 1, 0), (65536, 10, 64, 1, 0), (1, -1, 64, 1, 0), (1, 10, 32, 1, 0), (1, 10, 96, 1, 0), (1, 10, 4096, 1, 0), (1, 10, 64, 0, 0),
                (1, 10, 64, 33, 0), (1, 10, 64, 1, -1), (1, 10, 64, 1, 65), (1, (1 << 31) * 16 + 64, 64, 1, 0)]:
        assert lib.swc_segmental_workspace_bytes(*bad) == -1, bad
    assert lib.swc_segmental_workspace_bytes(1, ((1 << 31) - 3) * 16 + 64, 64, 1, 0) > 0       # 2^31 - 2 frames still fit


# ---- the reference against independent closed forms ----

FS, W, P = 16000, 512, 16


def noise_like(n, seed):
    from scipy.signal import lfilter
    rng = np.random.default_rng(seed)
    x = lfilter([1.0], [1.0, -1.3, 0.6], rng.standard_normal(n + 200))[200:]
    return (0.3 * x / np.abs(x).max()).astype(np.float32)


def tone(n, f, amp=0.4):
    return (amp * np.sin(2.0 * math.pi * f * np.arange(n) / FS)).astype(np.float32)


def mel_table(fs=FS, w=W, K=25):
    from simwhisper_codec_amd import metrics
    return metrics.pack_filterbanks([metrics.mel_filterbank(fs, w, K)])


def corrected_R(x):
    R = ref.autocorr(ref.framed(x, W), P)
    R[:, 0] *= ref.CORR
    return R


def test_levinson_against_a_toeplitz_solver_on_noise_and_on_pure_tones():
    from scipy.linalg import solve_toeplitz
    worst = {}
    for name, x, tol in (("noise", noise_like(6000, 1), 1e-12), ("tone", tone(6000, 437.0), 1e-7), ("tone2", tone(6000, 3000.0) + tone(6000, 1234.5, 0.1), 1e-7)):
        R = corrected_R(x)
        a, E = ref.levinson(R, P)
        assert (E > 0).all() and (E / R[:, 0] > 1e-7).all(), name                 # the recursion never loses positivity
        d = max(float(np.abs(solve_toeplitz(R[t, :P], -R[t, 1:]) - a[t, 1:]).max()) for t in range(len(R)))
        worst[name] = (d, float((E / R[:, 0]).min()))
        assert d <= tol, (name, d)
        # E is the prediction error: the quadratic form of a, to rounding (and not bit for bit: the header says so)
        q = ref.quad(a, R, P)
        assert np.allclose(q, E, rtol=1e-6) and (q > 0).all()
    print("levinson - solve_toeplitz, smallest E / R[0]:", worst)
    assert worst["noise"][0] < 1e-13 < 1e-2 < worst["noise"][1]


def test_the_autocorrelation_is_the_plain_one_in_the_headers_order():
    v = ref.framed(noise_like(3 * W, 2), W)
    R = ref.autocorr(v, P)
    for k in (0, 1, P):
        want = np.array([math.fsum(v[t, :W - k] * v[t, k:]) for t in range(len(v))])
        assert np.allclose(R[:, k], want, rtol=0, atol=1e-13 * abs(want).max())
    t, k, Q = 1, 5, W // 4
    parts = []
    for c in range(4):
        acc = 0.0
        for i in range(c * Q, min((c + 1) * Q, W - k)):
            acc = acc + v[t, i] * v[t, i + k]
        parts.append(acc)
    assert R[t, k] == ((parts[0] + parts[1]) + parts[2]) + parts[3]               # bit for bit: four parts, in order


def test_lpc_cepstrum_against_the_real_cepstrum_of_the_all_pole_filter():
    a, _ = ref.levinson(corrected_R(noise_like(4000, 3)), P)
    c = ref.cepstrum(a, P)
    N = 1 << 14
    for t in range(0, len(a), 5):
        want = np.fft.irfft(-np.log(np.fft.rfft(a[t], N)))[1:P + 1].real           # log(1 / A(z)) = sum_m c[m] z^-m
        assert np.abs(c[t, 1:] - want).max() < 1e-9, t
    assert abs(ref.cepstrum(np.array([1.0, -0.5]), 1)[1] - 0.5) == 0.0              # 1 / (1 - z^-1 / 2): c[1] = 1 / 2


def test_both_segmental_snrs_of_a_scaled_copy_are_20_k_log10_2():
    x = noise_like(FS // 2, 4) + tone(FS // 2, 300.0, 0.05)
    for K in (1, 25, 64):
        table = mel_table(K=K)
        for k, want in ((1, 20.0 * math.log10(2.0)), (2, 40.0 * math.log10(2.0)), (3, 60.0 * math.log10(2.0)), (6, 35.0), (9, 35.0)):
            y = (x.astype(np.float64) * (1.0 - 2.0 ** -k)).astype(np.float32)
            r = ref.measure(x, y, W, P, table)
            # y is rounded to f32: a relative error of 2^-24 of y in a difference of 2^-k x moves a dB value by < 9 2^(k-24)
            assert abs(r["segsnr"] - want) < 1e-5 and abs(r["fwsegsnr"] - want) < 1e-5, (K, k, r["segsnr"], r["fwsegsnr"])
            assert np.abs(r["track"][:, 3:] - want).max() < 1e-4
    assert abs(40.0 * math.log10(2.0) - 12.04) < 0.005


def test_power_of_two_scalings_are_bit_identical():
    x = noise_like(FS // 2, 5) + tone(FS // 2, 200.0, 0.05)
    rng = np.random.default_rng(6)
    y = (x + 0.02 * rng.standard_normal(len(x))).astype(np.float32)
    table = mel_table()
    base = ref.measure(x, y, W, P, table)
    assert base["llr"] > 0 and base["cd"] > 0 and base["frames_lpc"] == base["frames"] > 10
    for s in (2.0 ** -7, 0.5, 16.0):
        r = ref.measure(x, y * np.float32(s), W, P, table)                           # y alone: llr and cd
        assert r["llr"] == base["llr"] and r["cd"] == base["cd"] and np.array_equal(r["track"][:, [0, 2]], base["track"][:, [0, 2]])
        assert r["segsnr"] != base["segsnr"]
        r = ref.measure(x * np.float32(s), y * np.float32(s), W, P, table)           # both: all five
        assert np.array_equal(r["vals"], base["vals"]) and np.array_equal(r["track"], base["track"]), s


def test_identical_rows_give_exactly_0_0_0_35_35():
    x = noise_like(FS // 3, 7)
    r = ref.measure(x, x.copy(), W, P, mel_table())
    T = float(ref.frames(len(x), W))
    assert r["vals"].tolist() == [0.0, 0.0, 0.0, 35.0, 35.0, T, T, T]


def test_k95_is_the_rounded_95_percent():
    for T in range(1, 401):
        assert ref.k95(T) == math.floor(Fraction(19, 20) * T + Fraction(1, 2)) and 1 <= ref.k95(T) <= T
    assert [ref.k95(T) for T in (1, 10, 19, 20, 21, 30)] == [1, 10, 18, 19, 20, 29]


def test_the_selection_formula_is_the_sorted_prefix_mean_also_with_ties():
    rng = np.random.default_rng(8)
    for T in (1, 2, 19, 20, 21, 57, 400):
        for ties in (False, True):
            v = rng.random(T) * 2.0
            if ties:
                v = np.round(v * 4.0) / 4.0                                          # many equal values, exact in binary
                v[rng.integers(0, T, size=max(T // 3, 1))] = np.sort(v)[ref.k95(T) - 1]   # and a crowd at v* itself
            got = ref.select_mean(v)
            want = np.sort(v)[:ref.k95(T)]
            assert abs(got - want.mean()) < 1e-14 * max(1.0, want.mean())
            if ties:
                assert got == math.fsum(want) / ref.k95(T)                         # quarters add exactly
    assert math.isnan(ref.select_mean([])) and math.isnan(ref.select_mean([0.1, math.nan, 0.2]))


def test_frames_with_digital_silence_on_one_side():
    n = 12 * W
    x = noise_like(n, 9)
    rng = np.random.default_rng(10)
    y = (x + 0.01 * rng.standard_normal(n)).astype(np.float32)
    xs, ys = x.copy(), y.copy()
    xs[2 * W:2 * W + W + W // 4] = 0.0                                               # exactly two frames of clean silence
    ys[7 * W:8 * W] = 0.0                                                            # exactly one frame of degraded silence
    r = ref.measure(xs, ys, W, P, mel_table())
    T = ref.frames(n, W)
    clean_out, deg_out = [8, 9], [28]
    assert r["frames"] == T and r["frames_lpc"] == T - 3 and r["frames_fw"] == T - 2
    assert np.flatnonzero(np.isnan(r["track"][:, 0])).tolist() == clean_out + deg_out
    assert np.flatnonzero(np.isnan(r["track"][:, 4])).tolist() == clean_out
    assert (r["track"][clean_out, 3] == -10.0).all() and r["track"][deg_out, 3] == 0.0 and r["track"][deg_out, 4] == 0.0
    assert not np.isnan(r["vals"]).any()
    both = ref.measure(np.zeros(n, np.float32), np.zeros(n, np.float32), W, P, mel_table())
    assert both["frames"] == T and both["frames_lpc"] == 0 == both["frames_fw"] and both["segsnr"] == -10.0
    assert math.isnan(both["llr"]) and math.isnan(both["is"]) and math.isnan(both["cd"]) and math.isnan(both["fwsegsnr"])


def test_bad_band_tables_are_cut_not_followed():
    x = noise_like(3 * W, 11)
    y = (x * np.float32(0.9)).astype(np.float32)
    first, count, off, w = (v.copy() for v in mel_table(K=8))
    good = ref.measure(x, y, W, P, (first, count, off, w))
    first[0], count[7], off[5] = -3, 400, len(w) - 2
    cut = ref.measure(x, y, W, P, (first, count, off, w))
    assert cut["frames_fw"] == good["frames_fw"] and not math.isnan(cut["fwsegsnr"])
    count[:] = 0
    assert ref.measure(x, y, W, P, (first, count, off, w))["frames_fw"] == 0


# ---- the Python surface ----

def test_defaults_from_the_rate_and_refusals_without_a_gpu():
    from simwhisper_codec_amd import _lib, metrics, ops
    assert [metrics.segmental_params(fs) for fs in (8000, 16000, 22050, 44100, 48000)] == [(256, 10), (512, 16), (1024, 16), (2048, 16), (2048, 16)]
    for fs in (8000, 16000, 48000):
        W_, _ = metrics.segmental_params(fs)
        assert W_ >= 0.030 * fs > W_ // 2
    for bad in (0, -1, 96000, "x", 1000):
        with pytest.raises(_lib.SwcError):
            metrics.segmental_params(bad)
    x = [torch.zeros(1000)]
    with pytest.raises(_lib.SwcError, match="no CPU fallback"):
        metrics.segmental(x, x, device="cpu")
    with pytest.raises(_lib.SwcError, match="align="):
        metrics.segmental(x, x, align="phase")
    with pytest.raises(_lib.SwcError, match="needs align="):
        metrics.llr(x, x, fine="lag")
    with pytest.raises(_lib.SwcError):
        ops.segmental_workspace_bytes(1, 1000, 500, 16)
    with pytest.raises(_lib.SwcError):
        ops.segmental_workspace_bytes(1, 1000, 512, 33)
    t = metrics.segmental_table(16000, "cpu")
    assert (t["W"], t["P"], t["K"]) == (512, 16, 25) and t["first"].numel() == 25 and t["w"].dtype == torch.float32
    assert metrics.segmental_table(16000, "cpu") is t
    for name in ("llr", "itakura_saito", "lpc_cd", "seg_snr", "fw_seg_snr", "segmental"):
        assert callable(getattr(metrics, name))
    from simwhisper_codec_amd.codec import AudioCodec
    assert callable(AudioCodec.segmental)


def test_the_tool_has_the_common_flags():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_segmental
    a = evaluate_segmental.build_parser().parse_args(["--original_dir", "a", "--synthesized_dir", "b", "--align", "waveform", "--align_fine", "drift",
                                                      "--max_lag_ms", "20", "--batch_size", "4", "--sample_rate", "8000", "--verbose"])
    assert (a.align, a.align_fine, a.max_lag_ms, a.batch_size, a.sample_rate, a.verbose) == ("waveform", "drift", 20.0, 4, 8000, True)
    m = evaluate_segmental.summarise(["a", "b", "c"], {"frames": [3, 0, 5], "llr": [0.5, math.nan, math.nan], "is": [1.0, math.nan, 3.0],
                                                       "cd": [2.0, math.nan, 4.0], "segsnr": [10.0, math.nan, 20.0], "fwsegsnr": [11.0, math.nan, 21.0]})
    assert m["empty"] == ["b"] and m["llr"] == (0.5, 1) and m["is"] == (2.0, 2) and m["segsnr"] == (15.0, 2)
