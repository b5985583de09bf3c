"""swc_pitch (YIN F0 tracks and the pair measures in one call), the parts that need no GPU: the C-ABI of include/swc_pitch.h
(declarations == bindings == exports, a table apart from the other seven; every argument check before any launch; the
workspace arithmetic against its documented formula), and properties of the numpy restatement (tests/pitch_ref.py): integer
periods, noise and silence, level invariance, frame counts, the int64 / 2^53 bounds at the limit configuration."""
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

import pitch_ref as ref  # noqa: E402

P16 = dict(sr=16000, W=512, tau_min=32, tau_max=256, H=160)


# ---- ABI and arguments ----

def _header(name="swc_pitch.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


def test_pitch_header_declarations_are_bound():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    declared = _declared("swc_pitch.h")
    assert declared == {"swc_pitch", "swc_pitch_workspace_bytes"} == set(_lib.PITCH_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)                       # exported by the library
        argtypes, restype = _lib.PITCH_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    seen = set()
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        assert len(m.group(2).split(",")) == len(_lib.PITCH_SIGNATURES[m.group(1)][0]), m.group(1)
        seen.add(m.group(1))
    assert seen == declared
    assert len(_lib.PITCH_SIGNATURES["swc_pitch"][0]) == 20 and len(_lib.PITCH_SIGNATURES["swc_pitch_workspace_bytes"][0]) == 5


def test_pitch_table_is_apart_from_the_other_seven():
    from simwhisper_codec_amd import _lib
    mine = set(_lib.PITCH_SIGNATURES)
    assert not mine & set(_lib.exported_symbols())
    for other in (_lib.SIGNATURES, _lib.PLAIN, _lib.AUDIO_SIGNATURES, _lib.CODES_SIGNATURES, _lib.METRICS_SIGNATURES,
                  _lib.QUALITY_SIGNATURES, _lib.FLAC_SIGNATURES, _lib.FLAC_IO_SIGNATURES, _lib.FLAC_ENC_SIGNATURES,
                  _lib.SPECTRAL_SIGNATURES):
        assert not mine & set(other)
    for h in ("swc.h", "swc_audio.h", "swc_codes.h", "swc_metrics.h", "swc_quality.h", "swc_flac.h", "swc_flac_enc.h", "swc_spectral.h"):
        assert not mine & _declared(h)
        assert "swc_pitch" not in _header(h)


def test_constants_agree_with_the_header():
    from simwhisper_codec_amd import _lib
    hdr = _header()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert (val("SWC_PITCH_MIN_TAU"), val("SWC_PITCH_MAX_TAU")) == (_lib.PITCH_MIN_TAU, _lib.PITCH_MAX_TAU) == (2, 1024)
    assert (val("SWC_PITCH_MIN_WIN"), val("SWC_PITCH_MAX_WIN")) == (_lib.PITCH_MIN_WIN, _lib.PITCH_MAX_WIN) == (16, 2048)
    assert val("SWC_PITCH_MAX_WORK") == _lib.PITCH_MAX_WORK == 1 << 21
    assert (val("SWC_PITCH_THRESHOLD_NUM"), val("SWC_PITCH_THRESHOLD_DEN")) == (ref.NUM, ref.DEN) == (3, 20)
    assert val("SWC_PITCH_FRAMES_PER_GROUP") == _lib.PITCH_FRAMES_PER_GROUP
    assert (val("SWC_PITCH_VALUES"), val("SWC_PITCH_COUNTS")) == (_lib.PITCH_VALUES, _lib.PITCH_COUNTS) == (8, 4)


def test_build_sees_a_touched_pitch_header(monkeypatch):
    from simwhisper_codec_amd import build
    build.build_library()
    assert not build._stale()
    assert "swc_pitch.hip" in build.SOURCES
    hdr = os.path.join(ROOT, "include", "swc_pitch.h")
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

    def call(x=p, y=p, n_in=p, max_n=9000, sr=16000, W=512, tau_min=32, tau_max=256, H=160, tau_x=p, f0_x=p, tau_y=p, f0_y=p,
             ldt=None, values=p, counts=p, ws=p, ws_bytes=None, B=2):
        T = ref.n_frames(max(max_n, 0), W, tau_max, max(H, 1))
        ldt = T if ldt is None else ldt
        if ws_bytes is None:
            ws_bytes = max(lib.swc_pitch_workspace_bytes(max(min(B, 65535), 0), max(max_n, 0), W, tau_max, H), 1 << 20)
        return lib.swc_pitch(x, y, n_in, max_n, sr, W, tau_min, tau_max, H, tau_x, f0_x, tau_y, f0_y, ldt, values, counts, ws, ws_bytes,
                             B, None)

    need = lib.swc_pitch_workspace_bytes(2, 9000, 512, 256, 160)
    assert need > 0
    odd = C.c_void_p(p.value + 4)
    no_y = dict(y=None, tau_y=None, f0_y=None, values=None)
    for kw, word in [(dict(x=None), b"null"), (dict(n_in=None), b"null"), (dict(ws=None), b"null"),
                     (dict(y=None, tau_y=None, f0_y=None), b"need y_rows"), (dict(y=None, tau_y=None, values=None), b"need y_rows"),
                     (dict(y=None, f0_y=None, values=None), b"need y_rows"),
                     (dict(tau_x=None, f0_x=None, tau_y=None, f0_y=None, values=None, counts=None), b"no output"),
                     (dict(B=-1), b"B="), (dict(B=65536), b"B="), (dict(max_n=-1), b"max_n_in"), (dict(sr=0), b"sr="),
                     (dict(W=15), b"window"), (dict(W=2049), b"window"),
                     (dict(tau_min=1), b"lags"), (dict(tau_min=256), b"lags"), (dict(tau_min=300), b"lags"),
                     (dict(tau_max=1025, W=1024), b"lags"), (dict(tau_min=0, tau_max=1), b"lags"),
                     (dict(H=0), b"hop"), (dict(H=-5), b"hop"), (dict(W=2048, tau_max=1024, H=0), b"hop"),
                     (dict(max_n=1 << 40, H=1), b"2^31 frames"),
                     (dict(ldt=ref.n_frames(9000, 512, 256, 160) - 1), b"ldt"), (dict(ldt=0), b"ldt"),
                     (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"),
                     (dict(ws_bytes=need - 1, **no_y), b"workspace"),
                     (dict(ws=odd), b"aligned")]:
        assert call(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    # W * tau_max <= 2^21 cannot be missed alone (2048 * 1024 = 2^21: the two largest values meet it with equality); the call
    # checks the product all the same, and the largest configuration passes
    assert call(W=2048, tau_max=1024, tau_min=2, B=0) == 0
    # nothing to do: no launch, no device needed.  Each output alone; ldt does not matter without a track; x alone
    assert call(B=0) == 0
    outs = ("tau_x", "f0_x", "tau_y", "f0_y", "values", "counts")
    for only in outs:
        assert call(B=0, **{k: None for k in outs if k != only}) == 0, only
    assert call(B=0, ldt=0, tau_x=None, f0_x=None, tau_y=None, f0_y=None) == 0
    assert call(B=0, **no_y) == 0 and call(B=0, counts=None, tau_x=None, **no_y) == 0
    assert call(B=0, W=16, tau_min=2, tau_max=3, H=1, max_n=0) == 0
    assert call(B=0, ws_bytes=need) == 0
    del keep


def test_workspace_bytes_against_the_documented_formula():
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    up = lambda v: (v + 255) & ~255
    for B, n, W, tmax, H in [(1, 0, 512, 256, 160), (1, 767, 512, 256, 160), (1, 768, 512, 256, 160), (3, 927, 512, 256, 160),
                             (3, 928, 512, 256, 160), (32, 160000, 512, 256, 160), (33, 40000, 256, 128, 80), (0, 5000, 512, 256, 160),
                             (65535, 3072, 2048, 1024, 1), (2, 48000, 1536, 768, 480), (5, 100, 16, 3, 1)]:
        T = 0 if n < W + tmax else 1 + (n - W - tmax) // H
        want = up(2 * B * 4) + up(2 * B * T * 4)
        assert lib.swc_pitch_workspace_bytes(B, n, W, tmax, H) == want, (B, n, W, tmax, H)
        assert ops.pitch_workspace_bytes(B, n, dict(W=W, tau_max=tmax, H=H)) == want and want % 256 == 0
        assert ops.pitch_frames(n, dict(W=W, tau_max=tmax, H=H)) == T == ref.n_frames(n, W, tmax, H)
    for bad in [(-1, 10, 512, 256, 160), (65536, 10, 512, 256, 160), (1, -1, 512, 256, 160), (1, 10, 15, 8, 160), (1, 10, 2049, 256, 160),
                (1, 10, 512, 1025, 160), (1, 10, 512, 2, 160), (1, 10, 512, 256, 0), (1, 1 << 40, 512, 256, 1)]:
        assert lib.swc_pitch_workspace_bytes(*bad) == -1, bad
        with pytest.raises(_lib.SwcError):
            ops.pitch_workspace_bytes(bad[0], bad[1], dict(W=bad[2], tau_max=bad[3], H=bad[4]))


def test_parameters_from_the_rate():
    from simwhisper_codec_amd import _lib, ops
    assert ops.pitch_params(16000) == dict(sr=16000, W=512, tau_min=32, tau_max=256, H=160) == ref.params(16000)
    for sr in (8000, 11025, 22050, 24000, 32000, 44100, 48000):
        p = ops.pitch_params(sr)
        assert p == ref.params(sr)
        assert p["tau_min"] == sr // 500 and p["tau_max"] == math.ceil(sr / 62.5) and p["W"] == 2 * p["tau_max"]
        assert 2 <= p["tau_min"] < p["tau_max"] <= 1024 and p["W"] <= 2048 and p["W"] * p["tau_max"] <= 1 << 21
    for bad in (0, -16000, 96000):
        with pytest.raises(_lib.SwcError):
            ops.pitch_params(bad)
    with pytest.raises(_lib.SwcError):
        ops.pitch_params(16000, f_min=500.0, f_max=62.5)


def test_python_surface_refuses_what_it_cannot_do():
    from simwhisper_codec_amd import _lib, metrics
    x = torch.zeros(9000)
    with pytest.raises(_lib.SwcError, match="CPU"):
        metrics.pitch([x], [x], device="cpu")
    with pytest.raises(_lib.SwcError, match="CPU"):
        metrics.f0([x], device="cpu")
    with pytest.raises(_lib.SwcError, match="1 reference and 2"):
        metrics.pitch([x], [x, x], device="cuda")
    with pytest.raises(_lib.SwcError, match="want"):
        metrics.pitch([x], [x], device="cuda", want=("pesq",))
    with pytest.raises(_lib.SwcError, match="want"):
        metrics.pitch([x], [x], device="cuda", want=())


def test_tool_parser_and_summary():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_pitch
    a = vars(evaluate_pitch.build_parser().parse_args(["--original_dir", "A", "--synthesized_dir", "B"]))
    assert a["sample_rate"] == 16000 and a["batch_size"] >= 1 and a["verbose"] is False
    nan = float("nan")
    cols = {k: [1.0, nan, 2.0] for k in evaluate_pitch.KEYS}
    cols["vde"] = [0.25, 0.5, 0.75]
    m = evaluate_pitch.summarise(["a", "b", "c"], cols)
    assert m["f0_rmse_cents"] == (pytest.approx(1.5, abs=1e-12), ["b"]) and m["vde"] == (pytest.approx(0.5, abs=1e-12), [])
    text = "\n".join(evaluate_pitch.format_summary(m, 3))
    assert "mean F0 RMSE (cents): 1.500000 over 2 of 3 files (1 skipped" in text and "mean voicing decision error: 0.500000 over 3 of 3" in text
    m = evaluate_pitch.summarise(["a"], {k: [nan] for k in evaluate_pitch.KEYS})
    assert all(m[k] == (None, ["a"]) for k in evaluate_pitch.KEYS)
    assert "not defined over 0 of 1 files" in evaluate_pitch.format_summary(m, 1)[0]


# ---- properties of the reference ----

@pytest.mark.parametrize("tau", [32, 80, 160, 256])
def test_an_integer_period_is_found_in_every_frame(tau):
    sr = 16000
    x = ref.harmonic_complex(sr / tau, 4000, sr)
    q, state = ref.quantise(x)
    assert state == "ok" and np.abs(q).max() <= 32767
    T = ref.n_frames(len(x), 512, 256, 160)
    assert T == 21
    for t in range(T):
        detail = {}
        c, f = ref.frame(q[t * 160:t * 160 + 768], sr, 512, 32, 256, detail=detail)
        assert c == tau, (t, c)
        off = detail.get("off", 0.0)
        assert abs(off) < 0.05 and abs(sr / f - (tau + off)) < 1e-9
        if tau == 256:
            assert "off" not in detail and f == sr / 256      # c == tau_max: no refinement
    tr_tau, tr_f0 = ref.track(x, **P16)
    assert (tr_tau == tau).all() and tr_f0.dtype == np.float32 and (tr_f0 > 0).all()


def test_harmonic_complexes_are_voiced_and_close():
    sr = 16000
    for f in (62.5, 100.0, 333.3, 500.0):
        tau, f0 = ref.track(ref.harmonic_complex(f, 3000, sr), **P16)
        assert (tau > 0).all()
        assert np.abs(1200.0 * np.log2(f0.astype(np.float64) / f)).max() < 0.9, f


def test_noise_and_silence_are_unvoiced():
    x = (0.1 * np.random.default_rng(0).standard_normal(8000)).astype(np.float32)
    tau, f0 = ref.track(x, **P16)
    assert len(tau) == 46 and not tau.any() and not f0.any()
    tau, f0 = ref.track(np.zeros(4000, np.float32), **P16)
    assert len(tau) == 21 and not tau.any() and not f0.any()
    tau, f0 = ref.track(np.full(4000, np.nan, np.float32), **P16)
    assert len(tau) == 21 and (tau == -1).all() and np.isnan(f0).all()
    x[17] = np.inf
    tau, f0 = ref.track(x, **P16)
    assert (tau == -1).all() and np.isnan(f0).all()


def test_scaling_by_a_power_of_two_changes_no_bit():
    x = ref.test_signal(3)[:12000]     # the first glide and the noise after it
    base = ref.track(x, **P16)
    assert 0 < (base[0] > 0).sum() < len(base[0])
    for s in (2.0 ** -7, 2.0 ** 3):
        got = ref.track((x * np.float32(s)).astype(np.float32), **P16)
        assert np.array_equal(base[0], got[0]) and np.array_equal(base[1].view(np.uint32), got[1].view(np.uint32)), s


def test_frame_counts_at_the_edges():
    span, H = 768, 160
    for n, T in ((0, 0), (1, 0), (span - 1, 0), (span, 1), (span + H - 1, 1), (span + H, 2), (span + 2 * H - 1, 2), (32000, 196)):
        assert ref.n_frames(n, 512, 256, 160) == T
        tau, f0 = ref.track(np.zeros(n, np.float32), **P16)
        assert len(tau) == len(f0) == T


@pytest.mark.parametrize("amp, level", [(1.0, 16384), (ref.TOP, 32767)])
def test_the_bounds_hold_at_the_limit_configuration(amp, level):
    """W = 2048, tau_max = 1024 on the full-scale alternating row: d is 0 at even lags and W (2 level)^2 at odd lags; with
    |q| = 32767 that is the largest value a difference function can take"""
    W, tmax = 2048, 1024
    q, state = ref.quantise(ref.alternating(W + tmax, amp))
    assert state == "ok" and set(np.unique(q)) == {-level, level}
    detail = {}
    c, f = ref.frame(q, 16000, W, 2, tmax, detail=detail)
    d, S, dk = detail["d"], detail["S"], detail["dk"]
    assert d.dtype == S.dtype == dk.dtype == np.int64
    assert (d[0::2] == 0).all() and (d[1::2] == W * (2 * level) ** 2).all()
    assert d.max() > 2 ** 32 and dk.max() < 2 ** 53 and S.max() < 2 ** 53 and (ref.DEN * dk).max() < 2 ** 63 and ref.NUM * S.max() < 2 ** 63
    assert (dk.astype(np.float64).astype(np.int64) == dk).all() and (S.astype(np.float64).astype(np.int64) == S).all()
    if level == 32767:
        assert dk.max() > 2 ** 52
    # the first even lag, d = 0 there: a, b, g = 1, 0, 1.5, so off = 0.5 (1 - 1.5) / 2.5 = -0.1
    assert c == 2 and abs(detail["off"] + 0.1) < 1e-15 and abs(f - 16000.0 / 1.9) < 1e-9


def test_pair_values_of_identical_and_of_different_tracks():
    x = ref.test_signal(5)
    r = ref.pitch(x, x, **P16)
    T, n_vx, n_vy, n_vv = r["counts"]
    assert 0 < n_vv == n_vx == n_vy < T
    v = r["values"]
    assert v[0] == 0.0 and v[2] == 0.0 and v[3] == 0.0 and v[4] == 1.0 and abs(v[1] - 1.0) < 1e-12 and v[7] == 0.0
    v, c = ref.pair_values(np.array([100.0, 0.0, 200.0, 150.0], np.float32), np.array([100.0, 120.0, 260.0, 0.0], np.float32))
    assert list(c) == [4, 3, 3, 2] and v[2] == 0.5 and v[3] == 0.5 and abs(v[4] - 4.0 / 6.0) < 1e-15
    assert abs(v[0] - math.sqrt((1200.0 * math.log2(1.3)) ** 2 / 2.0)) < 1e-9 and abs(v[1] - 1.0) < 1e-12
    v, c = ref.pair_values(np.zeros(0, np.float32), np.zeros(0, np.float32))
    assert np.isnan(v[:7]).all() and v[7] == 0.0 and list(c) == [0, 0, 0, 0]
    v, c = ref.pair_values(np.array([100.0, 0.0], np.float32), np.array([100.0, 0.0], np.float32))
    assert v[0] == 0.0 and np.isnan(v[1]) and v[3] == 0.0 and v[4] == 1.0     # one both-voiced frame: no correlation
