"""swc_activity and swc_activity_normalise (ITU-T P.56 active level, the runs of active samples), the parts that need no GPU: the
C-ABI of include/swc_activity.h (declarations == bindings == exports, a table apart from the other eleven; every argument check
before any launch; the workspace arithmetic against its documented formula), the constants of a rate against exp(-1 / (fs T))
and the recursion run on the unit states, the numpy restatement (tests/activity_ref.py) on signals whose answer is known, the
host policy on hand-written run lists, the refusals of the Python surface and the flags of the tools."""
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

import activity_ref as ref  # noqa: E402

NAMES = {"swc_activity", "swc_activity_normalise", "swc_activity_workspace_bytes", "swc_activity_coefficients"}
OTHER_HEADERS = ("swc.h", "swc_audio.h", "swc_codes.h", "swc_metrics.h", "swc_quality.h", "swc_flac.h", "swc_flac_enc.h", "swc_spectral.h",
                 "swc_pitch.h", "swc_align.h", "swc_mcd.h", "swc_loudness.h")


def _header(name="swc_activity.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


def test_activity_header_declarations_are_bound():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    declared = _declared("swc_activity.h")
    assert declared == NAMES == set(_lib.ACTIVITY_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)                       # exported by the library
        argtypes, restype = _lib.ACTIVITY_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    seen = set()
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        assert len(m.group(2).split(",")) == len(_lib.ACTIVITY_SIGNATURES[m.group(1)][0]), m.group(1)
        seen.add(m.group(1))
    assert seen == declared
    assert [len(_lib.ACTIVITY_SIGNATURES[n][0]) for n in sorted(NAMES)] == [14, 6, 11, 3]


def test_activity_table_is_apart_from_the_other_eleven():
    from simwhisper_codec_amd import _lib
    mine = set(_lib.ACTIVITY_SIGNATURES)
    assert not mine & set(_lib.exported_symbols())
    for other in (_lib.SIGNATURES, _lib.PLAIN, _lib.AUDIO_SIGNATURES, _lib.CODES_SIGNATURES, _lib.METRICS_SIGNATURES,
                  _lib.QUALITY_SIGNATURES, _lib.FLAC_SIGNATURES, _lib.FLAC_IO_SIGNATURES, _lib.FLAC_ENC_SIGNATURES,
                  _lib.SPECTRAL_SIGNATURES, _lib.PITCH_SIGNATURES, _lib.ALIGN_SIGNATURES, _lib.MCD_SIGNATURES, _lib.LOUDNESS_SIGNATURES):
        assert not mine & set(other)
    for h in OTHER_HEADERS:
        assert not mine & _declared(h)
        assert "swc_activity" not in _header(h)


def test_constants_agree_with_the_header_and_the_reference():
    from simwhisper_codec_amd import _lib, metrics, ops
    hdr = _header()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert (val("SWC_ACTIVITY_MIN_FS"), val("SWC_ACTIVITY_MAX_FS")) == (_lib.ACTIVITY_MIN_FS, _lib.ACTIVITY_MAX_FS) == (8000, 48000)
    assert val("SWC_ACTIVITY_MAX_N") == _lib.ACTIVITY_MAX_N == 1 << 30 and val("SWC_ACTIVITY_MAX_HANGOVER") == _lib.ACTIVITY_MAX_HANGOVER
    assert val("SWC_ACTIVITY_VALUES") == _lib.ACTIVITY_VALUES == len(ops.ACTIVITY_VALUES) == len(ref.KEYS) == 8
    assert val("SWC_ACTIVITY_THRESHOLDS") == _lib.ACTIVITY_THRESHOLDS == ref.THRESHOLDS == 15
    assert (val("SWC_ACTIVITY_SUBBLOCK"), val("SWC_ACTIVITY_GROUP")) == (_lib.ACTIVITY_SUBBLOCK, _lib.ACTIVITY_GROUP) == (256, 64)
    assert (val("SWC_ACTIVITY_TILE"), val("SWC_ACTIVITY_THREADS")) == (_lib.ACTIVITY_TILE, _lib.ACTIVITY_THREADS) == (4096, 256)
    assert (val("SWC_ACTIVITY_UNMEASURED"), val("SWC_ACTIVITY_PEAK_LIMITED")) == (_lib.ACTIVITY_UNMEASURED, _lib.ACTIVITY_PEAK_LIMITED) \
        == (ref.UNMEASURED, ref.PEAK_LIMITED) == (1, 2)
    assert ops.ACTIVITY_VALUES == ref.KEYS and len(metrics.ACTIVE_LEVEL_KEYS) == 5
    for i, k in enumerate(("ACTIVE_LEVEL", "LONG_TERM", "FACTOR", "THRESHOLD", "SAMPLE_PEAK", "ACTIVE_SAMPLES", "RUNS", "CROSSING")):
        assert val("SWC_ACTIVITY_" + k) == i
    assert "Bits" in hdr and "closed form" in hdr and "bisection" in hdr and "samples, fs, margin_db and hangover_s only" in hdr


def test_build_sees_the_new_object_and_a_touched_header(monkeypatch):
    from simwhisper_codec_amd import build
    build.build_library()
    assert not build._stale()
    assert "swc_activity.hip" in build.SOURCES
    hdr = os.path.join(ROOT, "include", "swc_activity.h")
    real = os.path.getmtime
    newer = real(build.LIB_PATH) + 10
    monkeypatch.setattr(os.path, "getmtime", lambda p: newer if os.path.abspath(p) == hdr else real(p))
    assert build._stale()


def _aligned_buffer():
    raw = (C.c_char * 1024)()
    base = C.addressof(raw)
    return raw, C.c_void_p((base + 255) & ~255)


def test_activity_arg_checks_without_gpu():
    """every check happens before any launch: host pointers that are never dereferenced stand in for device memory"""
    from simwhisper_codec_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_buffer()

    def call(rows=p, n_in=p, max_n=160000, fs=16000, margin=15.9, hang=0.2, values=p, counts=p, runs=p, ld_runs=100, ws=p,
             ws_bytes=1 << 50, B=2):
        return lib.swc_activity(rows, n_in, max_n, fs, margin, hang, values, counts, runs, ld_runs, ws, ws_bytes, B, None)

    need = lib.swc_activity_workspace_bytes(2, 160000, 16000)
    up = lambda v: (v + 255) & ~255
    S, NT = 625, 40
    assert need == up(2 * S * 16) + up(2 * S * 8) + up(2 * S * 4) + up(2 * up(160000)) + up(2 * NT * 64) + up(2 * NT * 16)
    assert lib.swc_activity_workspace_bytes(0, 0, 8000) == 0 and lib.swc_activity_workspace_bytes(1, 1, 44100) == 5 * 256 + 256
    for bad in ((-1, 10, 16000), (65536, 10, 16000), (1, -1, 16000), (1, (1 << 30) + 1, 16000), (1, 10, 7999), (1, 10, 48001), (1, 10, 0)):
        assert lib.swc_activity_workspace_bytes(*bad) == -1, bad
    odd = C.c_void_p(p.value + 4)
    for kw, word in [(dict(rows=None), b"null"), (dict(n_in=None), b"null"), (dict(values=None), b"null"), (dict(counts=None), b"null"),
                     (dict(runs=None), b"null"), (dict(ws=None), b"null"), (dict(B=65536), b"B="), (dict(B=-1), b"B="),
                     (dict(max_n=-1), b"max_n_in"), (dict(max_n=(1 << 30) + 1), b"max_n_in"),
                     (dict(fs=7999), b"fs="), (dict(fs=48001), b"fs="), (dict(fs=0), b"fs="),
                     (dict(margin=0.0), b"margin_db"), (dict(margin=math.nan), b"margin_db"), (dict(margin=101.0), b"margin_db"),
                     (dict(hang=-0.1), b"hangover_s"), (dict(hang=math.nan), b"hangover_s"), (dict(hang=1.6), b"hangover_s"),
                     (dict(ld_runs=49), b"ld_runs"), (dict(ld_runs=99, fs=8000), b"ld_runs"), (dict(ld_runs=0), b"ld_runs"),
                     (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"), (dict(ws=odd), b"aligned"),
                     (dict(values=odd), b"8-byte"), (dict(runs=odd), b"8-byte")]:
        assert call(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    # nothing to do: no launch, no device needed; any integer rate in the range passes (no multiple-of-10 rule)
    for fs in (8000, 11025, 16000, 22050, 44100, 48000, 8001):
        assert call(B=0, fs=fs) == 0
    assert call(B=0, max_n=0, ws_bytes=0, ld_runs=1) == 0 and call(B=0, max_n=1 << 30, ld_runs=1 << 30) == 0
    assert call(B=0, ld_runs=160000 // 3202 + 1) == 0 and call(B=0, ld_runs=100, fs=8000) == 0

    def norm(rows=p, n_in=p, values=p, target=-26.0, out=p, ld=100, cols=100, gains=p, flags=p, B=2):
        return lib.swc_activity_normalise(rows, n_in, values, target, out, ld, cols, gains, flags, B, None)

    for kw, word in [(dict(rows=None), b"null"), (dict(n_in=None), b"null"), (dict(values=None), b"null"),
                     (dict(out=None, gains=None, flags=None), b"no output"), (dict(B=65536), b"B="), (dict(B=-1), b"B="),
                     (dict(target=math.nan), b"finite"), (dict(target=math.inf), b"finite"), (dict(cols=101), b"cols"),
                     (dict(cols=-1), b"cols")]:
        assert norm(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    assert norm(B=0) == 0 and norm(B=0, out=None) == 0 and norm(B=0, gains=None, flags=None, cols=0) == 0
    del keep


def test_python_surface_refuses_what_it_cannot_do():
    from simwhisper_codec_amd import _lib, metrics, ops
    x = torch.zeros(9000)
    for fs in (7999, 48001, 96000, 16000.5, "fast"):
        for call in (lambda: metrics.active_level([x], sample_rate=fs), lambda: metrics.speech_segments([x], fs),
                     lambda: metrics.trimmed([x], fs), lambda: metrics.split_at_pauses([x], fs), lambda: metrics.level_normalised([x], fs)):
            with pytest.raises(_lib.SwcError, match="sample_rate"):
                call()
    for call in (lambda: metrics.active_level([x], device="cpu"), lambda: metrics.speech_segments([x], device="cpu"),
                 lambda: metrics.level_normalised([x], 16000, device="cpu")):
        with pytest.raises(_lib.SwcError, match="CPU"):
            call()
    with pytest.raises(_lib.SwcError, match="rows"):
        ops.activity([], 16000)                 # B = 0 is refused before anything is launched
    with pytest.raises(_lib.SwcError, match="rows"):
        ops.activity_normalise([], torch.zeros(0, 8, dtype=torch.float64))
    with pytest.raises(_lib.SwcError, match="hangover"):
        ops.activity_coefficients(48000, 0.6)
    for fs in (8000, 11025, 22050, 44100, 48000):
        assert ops.activity_check_rate(fs) == fs and ref.rate_ok(fs)
    assert not ref.rate_ok(7999) and not ref.rate_ok(48001)
    assert ops.activity_run_capacity(160000, 3200) == 160000 // 3202 + 1


# ---- the definition ----

def test_coefficients_against_the_text_and_the_recursion_on_the_unit_states():
    from simwhisper_codec_amd import ops
    rel = lambda a, b: abs(a - b) / abs(b)
    for fs in (8000, 11025, 16000, 22050, 44100, 48000):
        c = ops.activity_coefficients(fs)
        g = math.exp(-1.0 / (fs * 0.03))
        assert rel(c["g"], g) <= 1e-15 and c["g"] == ref.pole(fs)
        assert c["hangover"] == ref.hangover(fs) == int(math.floor(0.2 * fs + 0.5)) and c["subblock"] == 256
        want = []
        for p, q in ((1.0, 0.0), (0.0, 1.0)):                   # the recursion on silence from a unit state
            for _ in range(c["subblock"]):
                p = g * p + (1.0 - g) * 0.0
                q = g * q + (1.0 - g) * p
            want.append((p, q))
        m = c["transition"]                                      # row-major over (p, q): column c is what e_c becomes
        assert rel(m[0], want[0][0]) <= 1e-15 and rel(m[2], want[0][1]) <= 1e-15 and rel(m[3], want[1][1]) <= 1e-15 and m[1] == 0.0 == want[1][0]
        # carrying the state through the transition is the filter: 3 sub-blocks in one go against block by block from zero state
        x = np.random.default_rng(fs).standard_normal(3 * 256)
        whole = ref.envelope(x, fs)[-1]
        s = np.zeros(2)
        M = np.array(m).reshape(2, 2)
        for k in range(3):
            ax = np.abs(x[k * 256:(k + 1) * 256])
            from scipy.signal import lfilter
            p = lfilter([1.0 - g], [1.0, -g], ax)
            q = lfilter([1.0 - g], [1.0, -g], p)
            s = M @ s + np.array([p[-1], q[-1]])
        assert rel(s[1], whole) <= 1e-12
    assert abs(ref.pole(16000) - 0.9979) < 1e-4
    assert ops.activity_coefficients(16000, 0.1)["hangover"] == 1600 and ops.activity_coefficients(44100, 0.2)["hangover"] == 8820


def _tone(fs, seconds, amp=0.5, freq=997.0):
    t = np.arange(int(round(seconds * fs)), dtype=np.float64) / fs
    return (amp * np.sin(2.0 * math.pi * freq * t)).astype(np.float32)


def test_a_steady_tone_is_active_all_along():
    fs = 16000
    r = ref.measure(_tone(fs, 5.0), fs)
    assert abs(r["long_term"] - (-9.0309)) <= 1e-3
    assert 0.0 < r["active_level"] - r["long_term"] < 0.03 and r["activity"] > 0.99
    assert r["runs"] == 1 and len(r["run_list"]) == 1 and r["run_list"][0][1] == 5 * fs and r["run_list"][0][0] < 0.030 * fs
    assert abs(r["threshold"] / 0.5 - 0.113) < 0.002                  # c* = 0.113 x amplitude: reached after 0.73 T = 22 ms
    assert r["run_list"][0][0] == 366 and abs(r["active_level"] - r["long_term"] - 0.020) < 1e-3 and abs(r["activity"] - 0.9954) < 1e-4
    assert r["active_samples"] == 5 * fs - 366 and r["counts"][int(r["crossing"])] <= r["active_samples"] <= r["counts"][int(r["crossing"]) - 1]
    assert ref.margin(_tone(fs, 5.0), fs) > 1e-6


def test_a_gated_tone_has_three_runs_and_a_higher_active_level():
    fs = 16000
    on, off = _tone(fs, 1.0), np.zeros(fs, np.float32)
    x = np.concatenate([on, off, on, off, on, off])                    # 1 s on / 1 s off, 1 s of silence appended: 6 s
    r = ref.measure(x, fs)
    assert r["runs"] == 3 and all(1.2 <= (e - s) / fs <= 1.35 for s, e in r["run_list"])
    assert 0.60 <= r["activity"] <= 0.675
    assert abs(r["activity"] - r["active_samples"] / len(x)) < 0.005 and abs(r["activity"] - 0.639) < 1e-3
    assert abs((r["run_list"][0][1] - r["run_list"][0][0]) / fs - 1.278) < 1e-3
    assert abs(r["long_term"] + 12.04) < 0.005 and abs(r["active_level"] + 10.09) < 0.005
    assert ref.margin(x, fs) > 1e-6


def test_silence_an_empty_row_and_a_click_have_no_level_and_no_runs():
    fs = 16000
    click = np.zeros(fs, np.float32)
    click[100] = 1.0
    for x in (np.zeros(fs, np.float32), np.zeros(0, np.float32), click):
        r = ref.measure(x, fs)
        assert math.isnan(r["active_level"]) and math.isnan(r["activity"]) and math.isnan(r["threshold"]) and math.isnan(r["crossing"])
        assert r["run_list"] == [] and r["runs"] == 0 and r["active_samples"] == 0
    r = ref.measure(click, fs)
    assert r["sample_peak"] == 1.0 and not math.isnan(r["long_term"]) and r["counts"][0] > 0 and r["counts"][-1] == 0
    assert math.isnan(ref.measure(np.zeros(fs, np.float32), fs)["long_term"])
    assert ref.gain(math.nan, 0.5) == (1.0, 1) and ref.gain(-20.0, 0.0) == (1.0, 1)
    g, f = ref.gain(-60.0, 0.5)
    assert f == 2 and g == 2.0 and ref.gain(-20.0, 0.5) == (10 ** (-6 / 20), 0)


def test_the_hangover_bridges_short_gaps_and_the_walk_interpolates():
    q = np.array([0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0])
    assert ref.active_mask(q, 0.5, 3).tolist() == [False] + [True] * 8 + [False]
    assert ref.active_mask(q, 0.5, 2).tolist() == [False, True, True, True, False, True, True, True, False, False]
    assert ref.runs_of(ref.active_mask(q, 0.5, 2)) == [(1, 4), (5, 8)] and ref.runs_of(ref.active_mask(q, 2.0, 2)) == []
    assert ref.runs_of([True, True]) == [(0, 2)] and ref.runs_of([]) == []


# ---- the host policy ----

def test_policy_on_hand_written_run_lists():
    from simwhisper_codec_amd import metrics
    fs = 8000                                                           # I = 1600, min speech 400, pre 480 samples
    runs = [(100, 2500), (4000, 5999), (9000, 11000), (11400, 14000), (20000, 21999 + 1)]
    want = [(0, 2500), (8520, 14000), (19520, 22000)]                  # pre_ms clamped at 0; 399 < 400 dropped; two runs merged; 400 kept
    for seg in (metrics.segment_policy, ref.segments):
        assert seg(runs, fs) == want
        assert seg(runs, fs, min_speech_ms=0, pre_ms=0) == runs and seg([], fs) == []
        assert seg([(0, 3000), (3480, 6000)], fs) == [(0, 6000)]       # touching after the start moved back
    assert ref.trim(want) == (0, 22000) and ref.trim([]) == (0, 0)
    for split in (metrics.split_policy, ref.split):
        assert split([], 100) == [] and split([(5, 50), (70, 90)], 100) == [(5, 90)]
        # the longest pause wins; the left piece ends at its start, the right piece begins at its end
        assert split([(0, 40), (50, 90), (120, 160)], 100) == [(0, 90), (120, 160)]
        # two pauses of one length: the one whose midpoint is nearest the piece's midpoint (80 here: 85 against 45)
        assert split([(0, 40), (50, 80), (90, 160)], 100) == [(0, 80), (90, 160)]
        # ... and at equal distance the earlier one
        assert split([(0, 60), (70, 90), (100, 160)], 100) == [(0, 60), (70, 160)]
        # recursion on both pieces
        assert split([(0, 30), (40, 70), (100, 130), (135, 170)], 60) == [(0, 30), (40, 70), (100, 130), (135, 170)]
        assert split([(0, 30), (40, 70), (100, 130), (135, 170)], 70) == [(0, 70), (100, 170)]
        # a piece with no pause: ceil(len / max) parts at s + floor(k len / parts)
        assert split([(10, 110)], 30) == [(10, 35), (35, 60), (60, 85), (85, 110)]
        assert split([(0, 7)], 3) == [(0, 2), (2, 4), (4, 7)]
        assert split([(0, 50), (60, 400)], 200) == [(0, 50), (60, 230), (230, 400)]


# ---- tools ----

def test_cli_flags_parse_and_defaults_are_unchanged():
    import inference
    a = vars(inference.build_parser().parse_args([]))
    assert a["active_level"] is None and a["trim_silence"] is False and a["loudness"] is None and a["true_peak_db"] == -1.0
    assert a["mode"] == "roundtrip" and a["resample"] == "host" and a["flac"] == "host" and a["output_format"] == "wav" and a["in_flight"] == 2
    a = vars(inference.build_parser().parse_args(["--active_level", "-26", "--trim_silence", "--mode", "encode"]))
    assert a["active_level"] == -26.0 and a["trim_silence"] is True and a["mode"] == "encode"
    with pytest.raises(SystemExit, match="one of them"):
        inference.main(["--active_level", "-26", "--loudness", "-23", "--input_dir", "A", "--output_dir", "B"])
    with pytest.raises(SystemExit, match="CUDA"):
        inference.main(["--trim_silence", "--device", "cpu", "--input_dir", "A", "--output_dir", "B"])
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import measure_activity
    a = vars(measure_activity.build_parser().parse_args(["--input_dir", "D"]))
    assert a["sample_rate"] == 16000 and a["batch_size"] == 32 and a["input_dir"] == "D"
    assert vars(measure_activity.build_parser().parse_args(["D"]))["dir"] == "D"
    with pytest.raises(SystemExit):
        measure_activity.main([])
    st = measure_activity.pause_stats([(800, 16000), (24000, 40000)], 48000, 16000)
    assert st == {"segments": 2, "speech_s": 1.95, "leading_s": 0.05, "trailing_s": 0.5, "pauses": 1, "longest_pause_s": 0.5}
    assert measure_activity.pause_stats([], 16000, 16000)["leading_s"] == 1.0
    nan = math.nan
    rows = [dict(dict.fromkeys(measure_activity.COLUMNS, -20.0), activity=0.5, **st),
            dict(dict.fromkeys(measure_activity.COLUMNS, nan), sample_peak_db=-60.0, **measure_activity.pause_stats([], 100, 16000)),
            dict(dict.fromkeys(measure_activity.COLUMNS, -30.0), activity=0.7, **st)]
    means, out = measure_activity.summarise(["a", "b", "c"], rows)
    assert out == ["b"] and means["active_level_db"] == -25.0 and abs(means["activity"] - 0.6) < 1e-12 and means["pauses"] == 1
    assert "not measured" in measure_activity.format_line("b", rows[1]) and "-20.00 dBov" in measure_activity.format_line("a", rows[0])
    readme = open(os.path.join(ROOT, "tools", "README.md")).read()
    assert "measure_activity.py" in readme and "bench_activity.py" in readme
