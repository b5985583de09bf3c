"""swc_spectral (mel, STFT and log-spectral distances in one call), the parts that need no GPU: the float64 restatement
(tests/spectral_ref.py) against torch.stft and against closed forms, the conditioning of the test inputs, the mel filter bank
and its packed table, the C-ABI of include/swc_spectral.h (declarations == bindings, a table apart from the other six;
argument checks before any launch), the workspace arithmetic against its Python mirror, and the tool's parser and summary."""
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

import spectral_ref as ref  # noqa: E402
import stoi_ref  # noqa: E402

CONDITION = 1e-5     # |f32 restatement - f64| / |f64| over the case table (the GPU bound is ten times this)


# ---- the float64 restatement ----

@pytest.mark.parametrize("W", [32, 512, 2048])
def test_reference_stft_equals_torch_stft(W):
    x = stoi_ref.harmonic(5000, 16000).astype(np.float64)
    re, im = ref.stft_complex(x, W)
    want = torch.stft(torch.from_numpy(x), n_fft=W, hop_length=W // 4, win_length=W, window=torch.hann_window(W, periodic=True, dtype=torch.float64),
                      center=True, pad_mode="constant", return_complex=True).numpy().T          # [T][F]
    assert want.shape == re.shape == (1 + 5000 // (W // 4), W // 2 + 1)
    err = max(np.abs(re - want.real).max(), np.abs(im - want.imag).max())
    print(f"W={W}: max |ref - torch.stft| = {err:.2e}")
    assert err <= 1e-10


def test_identical_rows_give_exactly_zero():
    x = stoi_ref.harmonic(6000, 16000)
    r = ref.spectral(x, x, 16000)
    assert r["mel"] == 0.0 and r["stft"] == 0.0 and r["lsd"] == 0.0 and not r["parts"].any()
    r = ref.spectral(x, x, 16000, dtype=np.float32)
    assert r["mel"] == 0.0 and r["stft"] == 0.0 and r["lsd"] == 0.0 and not r["parts"].any()


@pytest.mark.parametrize("fs", [8000, 16000])
def test_ten_times_the_signal(fs):
    x = ref.white(6000, seed=fs // 8000).astype(np.float64)
    r = ref.spectral(x, 10.0 * x, fs)
    assert r["clamped"] == 0                                     # no cell is clamped: the closed form holds
    assert abs(r["mel"] - 7.0) <= 1e-12 and abs(r["lsd"] - 2.0) <= 1e-12
    for s, (W, M, fl) in enumerate(ref.default_scales()):
        assert abs(r["parts"][s, 0] - 1.0) <= 1e-12, W
        if fl & ref.STFT:
            assert abs(r["parts"][s, 1] - 2.0) <= 1e-12, W
            X = ref.stft_mag(x, W)
            assert abs(r["parts"][s, 2] - 9.0 * X.mean()) <= 1e-12 * 9.0 * X.mean(), W
        else:
            assert r["parts"][s, 1] == 0.0 and r["parts"][s, 2] == 0.0 and r["parts"][s, 3] == 0.0


def test_a_silent_reconstruction_is_the_clamp_on_one_side():
    x = ref.white(6000).astype(np.float64)
    r = ref.spectral(x, np.zeros(6000), 16000)
    for s, (W, M, fl) in enumerate(ref.default_scales()):
        X = ref.stft_mag(x, W)
        Mx = X @ ref.mel_filterbank(16000, W, M).astype(np.float32).astype(np.float64).T
        assert (Mx > ref.CLAMP).all() and (X > ref.CLAMP).all()
        assert abs(r["parts"][s, 0] - (np.log10(Mx) + 5.0).mean()) <= 1e-12
        if fl & ref.STFT:
            assert abs(r["parts"][s, 1] - (2.0 * np.log10(X) + 10.0).mean()) <= 1e-12
            assert abs(r["parts"][s, 2] - X.mean()) <= 1e-12
        if fl & ref.LSD:
            assert abs(r["parts"][s, 3] - np.sqrt(((2.0 * np.log10(X) + 10.0) ** 2).mean(axis=1)).mean()) <= 1e-12


def test_an_empty_row_gives_nan():
    x = ref.white(100)
    for a, b in ((x[:0], x[:0]), (x, x[:0])):
        r = ref.spectral(a, b, 16000)
        assert math.isnan(r["mel"]) and math.isnan(r["stft"]) and math.isnan(r["lsd"])
        for s, (_, _, fl) in enumerate(ref.default_scales()):
            assert math.isnan(r["parts"][s, 0])
            assert [math.isnan(v) for v in r["parts"][s, 1:]] == [bool(fl & ref.STFT), bool(fl & ref.STFT), bool(fl & ref.LSD)]


def test_frame_counts():
    for n, W, T in ((1, 32, 1), (7, 32, 1), (8, 32, 2), (9, 32, 2), (511, 2048, 1), (512, 2048, 2), (2049, 2048, 5), (18000, 32, 2251)):
        assert ref.frames(np.zeros(n), W).shape == (T, W)


@pytest.mark.parametrize("name", sorted(ref.case_table()))
def test_the_inputs_are_conditioned_for_float32(name):
    """a condition on the inputs, not a measurement of the kernel.  Harmonic + noise at 40 / 20 / 0 dB with n in {1, 7, 8, 2047,
    2048, 18000} and the two white-noise rows; the 40 dB rows of 1, 7 and 8 samples failed it (1.1e-5 .. 4.5e-5 over eight seeds:
    the mean of at most twenty log differences of 1.5e-3 each sits on the float32 rounding of log10 in any implementation) and
    were replaced by 10 dB rows of the same lengths"""
    fs, x, y = ref.case_table()[name]
    a, b = ref.spectral(x, y, fs), ref.spectral(x, y, fs, dtype=np.float32)
    worst = 0.0
    for k in ("mel", "stft", "lsd"):
        worst = max(worst, abs(b[k] - a[k]) / abs(a[k]))
    nz = a["parts"] != 0
    worst = max(worst, float((np.abs(b["parts"] - a["parts"])[nz] / np.abs(a["parts"][nz])).max()))
    print(f"{name}: worst relative |f32 - f64| = {worst:.2e}")
    assert worst <= CONDITION


# ---- the mel filter bank ----

@pytest.mark.parametrize("fs", ref.RATES)
def test_mel_filterbank_equals_the_reference(fs):
    from simwhisper_codec_amd import metrics
    for W, M in zip(ref.WINDOWS, ref.MELS):
        got, want = metrics.mel_filterbank(fs, W, M), ref.mel_filterbank(fs, W, M)
        assert got.shape == want.shape == (M, W // 2 + 1) and got.dtype == np.float64
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        assert (got >= 0).all()


@pytest.mark.parametrize("fs", ref.RATES)
def test_packed_table_unpacks_to_the_dense_bank(fs):
    from simwhisper_codec_amd import metrics
    t = metrics.spectral_table(fs, "cpu")
    assert metrics.spectral_table(fs, "cpu") is t                       # kept per (rate, device)
    assert t["win"] == list(ref.WINDOWS) and t["n_mels"] == list(ref.MELS)
    assert list(zip(t["win"], t["n_mels"], t["flags"])) == ref.default_scales()
    first, count, off, w = (t[k].numpy() for k in ("first", "count", "off", "w"))
    assert first.dtype == count.dtype == off.dtype == np.int32 and w.dtype == np.float32
    assert len(first) == len(count) == len(off) == sum(ref.MELS)
    k, empty = 0, {}
    for W, M in zip(ref.WINDOWS, ref.MELS):
        dense = ref.mel_filterbank(fs, W, M).astype(np.float32)
        for m in range(M):
            row = np.zeros(W // 2 + 1, np.float32)
            assert 0 <= first[k] and first[k] + count[k] <= W // 2 + 1 and 0 <= off[k] and off[k] + count[k] <= len(w)
            row[first[k]:first[k] + count[k]] = w[off[k]:off[k] + count[k]]
            assert np.array_equal(row, dense[m]), (W, m)
            if count[k] == 0:
                empty[W] = empty.get(W, 0) + 1
            else:
                assert row[first[k]] != 0 and row[first[k] + count[k] - 1] != 0
            k += 1
    assert off[-1] + count[-1] == len(w)
    print(f"{fs} Hz: empty filters per window {empty}")
    if fs == 48000:
        assert empty == {32: 1, 64: 1}
    if fs == 16000:
        assert empty == {}


# ---- ABI and arguments ----

def _header(name="swc_spectral.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


def test_spectral_header_declarations_are_bound():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    declared = _declared("swc_spectral.h")
    assert declared == {"swc_spectral", "swc_spectral_workspace_bytes"} == set(_lib.SPECTRAL_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)
        argtypes, restype = _lib.SPECTRAL_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    seen = set()
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        assert len(m.group(2).split(",")) == len(_lib.SPECTRAL_SIGNATURES[m.group(1)][0]), m.group(1)
        seen.add(m.group(1))
    assert seen == declared


def test_spectral_table_is_apart_from_the_other_six():
    from simwhisper_codec_amd import _lib
    mine = set(_lib.SPECTRAL_SIGNATURES)
    assert not mine & set(_lib.exported_symbols())
    for other in (_lib.SIGNATURES, _lib.PLAIN, _lib.AUDIO_SIGNATURES, _lib.CODES_SIGNATURES, _lib.METRICS_SIGNATURES,
                  _lib.QUALITY_SIGNATURES, _lib.FLAC_SIGNATURES, _lib.FLAC_IO_SIGNATURES, _lib.FLAC_ENC_SIGNATURES):
        assert not mine & set(other)
    for h in ("swc.h", "swc_audio.h", "swc_codes.h", "swc_metrics.h", "swc_quality.h", "swc_flac.h", "swc_flac_enc.h"):
        assert not mine & _declared(h)
        assert "swc_spectral" not in _header(h)


def test_constants_agree_with_the_header():
    from simwhisper_codec_amd import _lib
    hdr = _header()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert val("SWC_SPECTRAL_MAX_SCALES") == _lib.SPECTRAL_MAX_SCALES == 8
    assert (val("SWC_SPECTRAL_MEL"), val("SWC_SPECTRAL_STFT"), val("SWC_SPECTRAL_LSD")) == \
        (_lib.SPECTRAL_MEL, _lib.SPECTRAL_STFT, _lib.SPECTRAL_LSD) == (ref.MEL, ref.STFT, ref.LSD)
    assert _lib.SPECTRAL_WINDOWS == ref.WINDOWS
    for W in ref.WINDOWS:
        assert val(f"SWC_SPECTRAL_RUN_{W}") == _lib.SPECTRAL_RUN[W] and _lib.SPECTRAL_RUN[W] * (W // 4) == 8192


def test_build_sees_a_touched_spectral_header(monkeypatch):
    from simwhisper_codec_amd import build
    build.build_library()
    assert not build._stale()
    assert "swc_spectral.hip" in build.SOURCES
    hdr = os.path.join(ROOT, "include", "swc_spectral.h")
    real = os.path.getmtime
    newer = real(build.LIB_PATH) + 10
    monkeypatch.setattr(os.path, "getmtime", lambda p: newer if os.path.abspath(p) == hdr else real(p))
    assert build._stale()


def _aligned_buffer():
    raw = (C.c_char * 1024)()
    base = C.addressof(raw)
    return raw, C.c_void_p((base + 255) & ~255)


def _i32(values):
    return (C.c_int32 * len(values))(*values)


def test_arg_checks_without_gpu():
    """every check happens before any launch: host pointers that are never dereferenced stand in for device memory"""
    from simwhisper_codec_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_buffer()
    scales = ref.default_scales()
    WIN, MELS, FLAGS = [s[0] for s in scales], [s[1] for s in scales], [s[2] for s in scales]
    need = lib.swc_spectral_workspace_bytes(2, 9000, _i32(WIN), 7)
    assert need > 0

    def call(x=p, y=p, n_in=p, max_n=9000, win=WIN, mels=MELS, flags=FLAGS, n_scales=None, first=p, count=p, off=p, w=p, w_len=100,
             mel=p, stft=p, lsd=p, parts=p, ws=p, ws_bytes=None, B=2):
        n_scales = len(win) if n_scales is None else n_scales
        if ws_bytes is None:
            ws_bytes = lib.swc_spectral_workspace_bytes(max(min(B, 65535), 0), max(max_n, 0), _i32(win), min(n_scales, 8))
            ws_bytes = max(ws_bytes, 0)
        arr = lambda v: _i32(v) if v is not None else None
        return lib.swc_spectral(x, y, n_in, max_n, arr(win), arr(mels), arr(flags), n_scales, first, count, off, w, w_len, mel, stft, lsd,
                                parts, ws, ws_bytes, B, None)

    odd = C.c_void_p(p.value + 4)
    one = lambda W, M, fl: dict(win=[W], mels=[M], flags=[fl])
    nine = dict(win=[32] * 9, mels=[5] * 9, flags=[ref.MEL] * 9, ws_bytes=1 << 20)
    for kw, word in [(dict(x=None), b"null"), (dict(y=None), b"null"), (dict(n_in=None), b"null"), (dict(ws=None), b"null"),
                     (dict(win=None, n_scales=7, ws_bytes=need), b"null"), (dict(mels=None), b"null"), (dict(flags=None), b"null"),
                     (dict(first=None), b"mel table"), (dict(count=None), b"mel table"), (dict(off=None), b"mel table"),
                     (dict(w=None), b"mel table"), (dict(w=None, stft=None, lsd=None, parts=None), b"mel table"),
                     (dict(mel=None, stft=None, lsd=None, parts=None), b"no output"),
                     (dict(B=-1), b"B="), (dict(B=65536), b"B="), (dict(max_n=-1), b"max_n_in"),
                     (dict(ws_bytes=1 << 20, **one(48, 5, ref.MEL)), b"window"), (dict(ws_bytes=1 << 20, **one(4096, 5, ref.MEL)), b"window"),
                     (dict(ws_bytes=1 << 20, **one(16, 5, ref.MEL)), b"window"), (dict(ws_bytes=1 << 20, **one(0, 5, ref.MEL)), b"window"),
                     (nine, b"n_scales"), (dict(n_scales=0, ws_bytes=need), b"n_scales"),
                     (one(64, 0, ref.MEL), b"n_mels"), (one(64, 34, ref.MEL), b"n_mels"), (one(64, 34, ref.STFT), b"n_mels"),
                     (one(64, -1, ref.STFT), b"n_mels"), (one(64, 5, 8), b"flags"),
                     (dict(win=[512, 2048], mels=[80, 320], flags=[ref.LSD, ref.LSD]), b"LSD"),
                     (dict(max_n=1 << 40, ws_bytes=1 << 20), b"2^31 frames"),
                     (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"),
                     (dict(mel=None, stft=None, parts=None, ws_bytes=need - 1), b"workspace"),
                     (dict(ws=odd), b"aligned"), (dict(w_len=-1), b"fb_w_len")]:
        assert call(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    # nothing to do: no launch, no device needed.  Each output alone; without MEL work the table may be null; n_mels = F and
    # n_mels = 0 without the MEL flag are fine
    assert call(B=0) == 0
    for only in ("mel", "stft", "lsd", "parts"):
        assert call(B=0, **{k: None for k in ("mel", "stft", "lsd", "parts") if k != only}) == 0
    assert call(B=0, mel=None, parts=None, first=None, count=None, off=None, w=None) == 0
    assert call(B=0, **one(64, 33, ref.MEL)) == 0 and call(B=0, **one(64, 0, ref.STFT | ref.LSD)) == 0
    assert call(B=0, first=None, count=None, off=None, w=None, **one(64, 0, ref.STFT)) == 0
    del keep


def test_workspace_bytes_and_its_python_mirror():
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    for B, n, win in [(1, 0, [32]), (1, 8191, list(ref.WINDOWS)), (1, 8192, list(ref.WINDOWS)), (3, 18000, list(ref.WINDOWS)),
                      (32, 160000, list(ref.WINDOWS)), (33, 8193, [2048, 512]), (0, 100, [64]), (65535, 1, [32, 32]), (2, 9000, [])]:
        L = ops.spectral_workspace_layout(B, n, win)
        assert lib.swc_spectral_workspace_bytes(B, n, _i32(win) if win else None, len(win)) == L["total"] == ops.spectral_workspace_bytes(B, n, win)
        assert L["runs"] == [math.ceil((1 + n // (w // 4)) / _lib.SPECTRAL_RUN[w]) for w in win]
        assert L["rec"] == sorted(L["rec"]) and all(v % 256 == 0 for v in L["rec"] + [L["total"]])
        for s in range(len(win)):
            end = L["rec"][s + 1] if s + 1 < len(win) else L["total"]
            assert end - L["rec"][s] >= 32 * B * L["runs"][s]
    assert ops.spectral_workspace_layout(1, 8191, [32])["runs"] == [1] and ops.spectral_workspace_layout(1, 8192, [32])["runs"] == [2]
    for bad in [(-1, 10, [32]), (65536, 10, [32]), (1, -1, [32]), (1, 10, [48]), (1, 10, [4096]), (1, 1 << 40, [32])]:
        assert lib.swc_spectral_workspace_bytes(bad[0], bad[1], _i32(bad[2]), len(bad[2])) == -1
        with pytest.raises(_lib.SwcError):
            ops.spectral_workspace_bytes(*bad)
    assert lib.swc_spectral_workspace_bytes(1, 10, _i32([32] * 9), 9) == -1 and lib.swc_spectral_workspace_bytes(1, 10, None, 1) == -1
    with pytest.raises(_lib.SwcError):
        ops.spectral_workspace_bytes(1, 10, [32] * 9)


def test_python_surface_refuses_what_it_cannot_do():
    from simwhisper_codec_amd import _lib, metrics
    x = torch.zeros(9000)
    with pytest.raises(_lib.SwcError, match="CPU"):
        metrics.spectral([x], [x], device="cpu")
    with pytest.raises(_lib.SwcError, match="1 reference and 2"):
        metrics.spectral([x], [x, x], device="cuda")
    with pytest.raises(_lib.SwcError, match="want"):
        metrics.spectral([x], [x], device="cuda", want=("pesq",))
    with pytest.raises(_lib.SwcError, match="want"):
        metrics.spectral([x], [x], device="cuda", want=())


def test_tool_parser_and_summary():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_spectral
    a = vars(evaluate_spectral.build_parser().parse_args(["--original_dir", "A", "--synthesized_dir", "B"]))
    assert a["sample_rate"] == 16000 and a["batch_size"] >= 1 and a["verbose"] is False
    nan = float("nan")
    m = evaluate_spectral.summarise(["a", "b", "c"], [1.0, nan, 2.0], [3.0, nan, 5.0], [0.5, nan, 1.0])
    assert m["mel"] == pytest.approx(1.5, abs=1e-12) and m["stft"] == pytest.approx(4.0, abs=1e-12)
    assert m["lsd"] == pytest.approx(0.75, abs=1e-12) and m["empty"] == ["b"]
    m = evaluate_spectral.summarise(["a"], [nan], [nan], [nan])
    assert (m["mel"], m["stft"], m["lsd"], m["empty"]) == (None, None, None, ["a"])
