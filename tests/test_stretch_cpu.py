"""include/swc_stretch.h without a GPU: the ABI (declarations == table == exports, argument counts, the #defines), every
argument check before any launch, the length and workspace formulas, three properties of the numpy restatement
(tests/stretch_ref.py), the Python refusals with the loader patched to fail, check_condition on the new keys and the CLI flags.
row() and CASES are what the GPU test runs as well."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stretch_ref as ref  # noqa: E402

NAMES = {"swc_stretch_out_len", "swc_stretch_workspace_bytes", "swc_stretch"}
KINDS = ("noise", "period", "zeros", "quiet", "square")
SPEEDS = ((1, 1), (4, 5), (5, 4), (17, 18), (1, 2), (2, 1), (1, 4), (4, 1))


def row(kind, n, seed=0):
    """the rows of the checks: white noise; two harmonics with the integer period 100; exact zeros; noise at a peak of 1e-4; a
    full-scale square wave of period 74 (q = +-16384: many d reach the same Dm, the tie rule decides)"""
    t = np.arange(n)
    rng = np.random.default_rng([seed, n, KINDS.index(kind) if kind in KINDS else 9])
    if kind == "noise":
        return rng.uniform(-1.0, 1.0, n).astype(np.float32)
    if kind == "period":
        return (0.4 * np.sin(2 * np.pi * t / 100) + 0.3 * np.sin(2 * np.pi * t / 50 + 1.0)).astype(np.float32)
    if kind == "zeros":
        return np.zeros(n, np.float32)
    if kind == "quiet":
        return (1e-4 * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
    if kind == "square":
        return np.where((t // 37) % 2 == 0, 1.0, -1.0).astype(np.float32)
    raise ValueError(kind)


def lengths(W):
    Hs = W // 2
    return (0, 1, Hs - 1, Hs, Hs + 1, W, W + 1, 3 * W + 5, 5000)


def _cycle(W, B):
    """B rows: every length of lengths(W) and every kind, with empty rows among them"""
    ns = lengths(W)
    return [(KINDS[b % len(KINDS)], ns[(4 * b + 8) % len(ns)], b) for b in range(B)]


def _cases():
    """(W, D, num, den, rows) of every call, rows = (kind, n, seed).  Every W, D, speed and batch size of the issue occurs, and
    every length with the largest W and D (the first three calls)."""
    n = lengths(2048)
    return [
        (2048, 1024, 4, 5, [("noise", n[0], 0), ("noise", n[1], 1), ("noise", n[2], 2)]),
        (2048, 1024, 5, 4, [("noise", n[3], 0), ("period", n[4], 1), ("noise", n[5], 2)]),
        (2048, 1024, 1, 2, [("noise", n[6], 0), ("period", n[7], 1), ("square", n[8], 2)]),
        (512, 128, 17, 18, _cycle(512, 33)),
        (64, 7, 1, 1, _cycle(64, 33)),
        (16, 1, 2, 1, [("noise", 5000, 0), ("period", 53, 1), ("zeros", 0, 2)]),
        (16, 0, 1, 4, [("noise", 5000, 0)]),
        (64, 128, 4, 1, [("square", 5000, 0), ("noise", 65, 1), ("quiet", 31, 2)]),
        (512, 1024, 5, 4, [("square", 5000, 0)]),
        (2048, 7, 4, 5, [("quiet", 5000, 0)]),
    ]


CASES = _cases()


def test_the_cases_cover_the_issues_values():
    assert {c[0] for c in CASES} == {16, 64, 512, 2048} and {c[1] for c in CASES} == {0, 1, 7, 128, 1024}
    assert {(c[2], c[3]) for c in CASES} == set(SPEEDS) and {len(c[4]) for c in CASES} == {1, 3, 33}
    big = [r[1] for c in CASES if c[:2] == (2048, 1024) for r in c[4]]
    assert sorted(big) == sorted(lengths(2048))
    for W in (512, 64):
        rows = next(c[4] for c in CASES if c[0] == W and len(c[4]) == 33)
        assert {r[1] for r in rows} == set(lengths(W)) and {r[0] for r in rows} == set(KINDS) and sum(r[1] == 0 for r in rows) >= 2


def _header(name="swc_stretch.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


def _lib():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    return _lib, _lib.load()


# ---- ABI ----

def test_stretch_header_declarations_are_bound():
    _l, lib = _lib()
    declared = _declared("swc_stretch.h")
    assert declared == NAMES == set(_l.STRETCH_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)                       # exported by the library
        argtypes, restype = _l.STRETCH_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    seen = {}
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        seen[m.group(1)] = len(m.group(2).split(","))
    assert seen == {n: len(_l.STRETCH_SIGNATURES[n][0]) for n in NAMES}
    assert [seen[n] for n in sorted(NAMES)] == [18, 3, 5]


def test_stretch_table_is_apart_from_the_others():
    from simwhisper_codec_amd import _lib, build
    mine = set(_lib.STRETCH_SIGNATURES)
    assert not mine & set(_lib.exported_symbols())
    others = {k: v for k, v in vars(_lib).items() if (k.endswith("SIGNATURES") or k == "PLAIN") and k != "STRETCH_SIGNATURES"}
    assert len(others) >= 20 and "DEGRADE_SIGNATURES" in others
    for other in others.values():
        assert not mine & set(other)
    text = _header()
    for name in mine:
        text = text.replace(name, " ")
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "swc_stretch.h":
            assert not mine & _declared(h)
            for name in mine:
                assert name not in _header(h), (h, name)
            for name in _declared(h):   # the new header's text names no function that another table owns
                assert name not in text, (h, name)
    assert "swc_stretch.hip" in build.SOURCES and build.EXTRA_FLAGS["swc_stretch.hip"] == ["-ffp-contract=off"]


def test_defines_agree_with_the_bindings():
    from simwhisper_codec_amd import _lib
    d = {k: eval(v, {}) for k, v in re.findall(r"#define (SWC_\w+) (\(?[-\d <]+\)?)\s", _header())}
    assert d["SWC_STRETCH_MIN_W"] == _lib.STRETCH_MIN_W == ref.MIN_W == 16
    assert d["SWC_STRETCH_MAX_W"] == _lib.STRETCH_MAX_W == ref.MAX_W == 2048
    assert d["SWC_STRETCH_MAX_D"] == _lib.STRETCH_MAX_D == ref.MAX_D == 1024
    assert d["SWC_STRETCH_MAX_TERM"] == _lib.STRETCH_MAX_TERM == ref.MAX_TERM == 65535
    assert d["SWC_STRETCH_MAX_RATIO"] == _lib.STRETCH_MAX_RATIO == ref.MAX_RATIO == 4
    assert d["SWC_STRETCH_MAX_N"] == _lib.STRETCH_MAX_N == ref.MAX_N == 1 << 22
    assert d["SWC_STRETCH_CHUNK"] == _lib.STRETCH_CHUNK == ref.CHUNK == 4096
    assert d["SWC_STRETCH_UNDEFINED"] == _lib.STRETCH_UNDEFINED == ref.UNDEFINED == 1
    assert len(d) == 8


def test_out_len_and_workspace_bytes_are_the_headers_formulas():
    _l, lib = _lib()
    for n in (0, 1, 255, 256, 257, 5000, 160000, 1 << 22):
        for num, den in SPEEDS + ((1000, 999), (65535, 65534), (65535, 16384), (16384, 65535)):
            assert lib.swc_stretch_out_len(n, num, den) == ref.out_len(n, num, den) == -(-n * den // num)
    for bad in ((-1, 1, 1), ((1 << 22) + 1, 1, 1), (10, 0, 1), (10, 1, 0), (10, 65536, 65535), (10, 5, 1), (10, 1, 5), (10, -4, -5)):
        assert lib.swc_stretch_out_len(*bad) == ref.out_len(*bad) == -1, bad
    for B, max_n, W, num, den in ((1, 0, 16, 1, 1), (3, 1, 16, 1, 4), (33, 5000, 512, 17, 18), (7, 6149, 2048, 4, 5), (65535, 100, 64, 4, 1),
                                  (0, 480000, 512, 4, 5), (32, 1 << 22, 2048, 1, 4), (32, 1 << 22, 16, 1, 4)):
        assert lib.swc_stretch_workspace_bytes(B, max_n, W, num, den) == ref.workspace_bytes(B, max_n, W, num, den) > 0
    for bad in ((-1, 10, 512, 1, 1), (65536, 10, 512, 1, 1), (1, -1, 512, 1, 1), (1, (1 << 22) + 1, 512, 1, 1), (1, 10, 8, 1, 1),
                (1, 10, 2056, 1, 1), (1, 10, 20, 1, 1), (1, 10, 512, 0, 1), (1, 10, 512, 1, 65536), (1, 10, 512, 5, 1), (1, 10, 512, 1, 5)):
        assert lib.swc_stretch_workspace_bytes(*bad) == ref.workspace_bytes(*bad) == -1, bad


def test_every_argument_check_comes_before_any_launch():
    """host memory stands in for device memory: a call that got as far as a launch would not return SWC_E_ARG"""
    _l, lib = _lib()
    buf = (C.c_char * 16384)()
    p = C.addressof(buf)
    p = p + (-p) % 256
    ws = lib.swc_stretch_workspace_bytes(2, 1000, 512, 4, 5)
    J = ref.frames(1000, 512, 4, 5)
    assert J == 5
    good = dict(x=p, n=p + 64, max_n=1000, W=512, D=128, num=4, den=5, out=p + 1024, ld=1300, cols=1250, pos=p + 128, dist=p + 256, ldm=J,
                flags=p + 512, ws=p + 4096, wsb=ws, B=2)

    def call(**kw):
        a = dict(good, **kw)
        return lib.swc_stretch(a["x"], a["n"], a["max_n"], a["W"], a["D"], a["num"], a["den"], a["out"], a["ld"], a["cols"], a["pos"],
                               a["dist"], a["ldm"], a["flags"], a["ws"], a["wsb"], a["B"], None)

    for kw in (dict(B=-1), dict(B=65536), dict(x=None), dict(n=None), dict(ws=None), dict(out=None, pos=None, dist=None, flags=None),
               dict(x=p + 4), dict(n=p + 68), dict(out=p + 1026), dict(pos=p + 130), dict(dist=p + 260), dict(flags=p + 514),
               dict(ws=p + 4096 + 128), dict(W=8), dict(W=2056), dict(W=20), dict(W=0), dict(D=1025), dict(D=-1), dict(num=0), dict(den=0),
               dict(num=65536), dict(den=65536), dict(num=5, den=1), dict(num=1, den=5), dict(num=65535, den=16383),
               dict(max_n=(1 << 22) + 1), dict(max_n=-1), dict(cols=1301), dict(cols=-1), dict(ldm=J - 1), dict(ldm=J - 1, pos=None),
               dict(ldm=0, dist=None), dict(wsb=ws - 1), dict(wsb=0)):
        assert call(**kw) == -1, kw
        assert b"swc_stretch" in lib.swc_last_error()
    # B == 0 launches nothing; ldm, cols and ld are looked at only where their outputs are given
    assert call(B=0) == 0 and call(B=0, x=None, n=None, ws=None, wsb=0) == 0
    assert call(B=0, ldm=0, pos=None, dist=None) == 0 and call(B=0, out=None, cols=5, ld=1) == 0


# ---- the reference ----

def test_speed_one_is_the_identity():
    """On white noise at W = 512, D = 128.  Every d is 0: the exact continuation has Dm = 0.  y[t] = fmaf(w1, x, w2 x) with
    w1 + w2 = 1 up to the two table roundings (at most 2^-25 + 2^-26) and a product rounded to at most half an ulp of x: less
    than 1.5 ulp of x in all, so y is x or one of its neighbours, |y - x| <= ulp(x).  Every sample but the peak lies below
    the peak's power of two, where ulp(x) <= 2^-24 max|x| for a peak of exactly 1; the peak itself sits at t = 0, where
    w1 = 0, w2 = 1 and y = x exactly.  Hence the row: uniform noise in (-1, 1) with x[0] = 1."""
    x = row("noise", 5000)
    x[0] = 1.0
    assert np.abs(x).max() == 1.0
    pos, dist, defined = ref.track(x, 512, 128, 1, 1)
    assert defined and np.array_equal(pos, 256 * np.arange(len(pos))) and not dist.any()
    y = ref.synthesise(x, pos, defined, 512, 1, 1)
    err = float(np.abs(y.astype(np.float64) - x).max())
    print(f"speed 1/1: max |y - x| = {err:.3e} = {err * 2 ** 24:.3f} x 2^-24 max|x|")
    assert y.shape == x.shape and err <= 2.0 ** -24 * np.abs(x).max()


@pytest.mark.parametrize("num,den", [(4, 5), (5, 4), (17, 18), (3, 2), (1, 2)])
def test_a_periodic_row_stays_periodic(num, den):
    """period 100 <= 2 D: some d in the range continues the row exactly, so every frame whose target and span lie wholly inside
    the row has dist 0; and the f32 output is within 3 x 2^-24 max|x| of the float64 evaluation (two table roundings, one
    product, one final rounding)"""
    W, D, n = 512, 128, 6000
    x = row("period", n)
    pos, dist, defined = ref.track(x, W, D, num, den)
    inside = [m for m in range(1, len(pos)) if pos[m - 1] + W // 2 >= 0 and pos[m - 1] + W // 2 + W <= n
              and (m * (W // 2) * num) // den - D >= 0 and (m * (W // 2) * num) // den + D + W <= n]
    assert len(inside) >= 10 and not dist[inside].any()
    y, y64 = ref.synthesise(x, pos, defined, W, num, den), ref.stretch64(x, pos, W, num, den)
    err = float(np.abs(y - y64).max() / np.abs(x).max())
    print(f"speed {num}/{den}: {len(inside)} of {len(pos)} frames inside, f32 against float64 {err * 2 ** 24:.3f} x 2^-24 max|x|")
    assert len(y) == ref.out_len(n, num, den) and err <= 3 * 2.0 ** -24
    # the stretched row is the same periodic row: over the frames inside, it repeats after 100 samples as well as f32 lets it
    # (x[t] and x[t + 100] are a rounding of the sine apart, y is 1.5 x 2^-24 from its float64 value at either end)
    assert inside == list(range(1, len(inside) + 1))
    lo, hi = W // 2, (inside[-1] + 1) * (W // 2)
    assert np.abs(y[lo:hi - 100] - y[lo + 100:hi]).max() <= 8 * 2.0 ** -24


def test_reference_float64_bound_on_noise_and_ties_on_the_square_wave():
    x = row("noise", 5000)
    for num, den in ((4, 5), (5, 4)):
        pos, dist, defined = ref.track(x, 512, 128, num, den)
        err = float(np.abs(ref.synthesise(x, pos, defined, 512, num, den) - ref.stretch64(x, pos, 512, num, den)).max() / np.abs(x).max())
        # (noise has no other continuation than the exact one: the track follows it while it is in range, then jumps)
        assert err <= 3 * 2.0 ** -24 and (dist[1:] == 0).any() and (dist[1:] > 0).any()
    assert ref.track(row("square", 5000), 64, 128, 4, 1, count_ties=True)[3] >= 1
    pos, dist, defined, ties = ref.track(row("zeros", 700), 64, 7, 4, 5, count_ties=True)
    assert ties == len(pos) - 1 and np.array_equal(pos, (np.arange(len(pos)) * 32 * 4) // 5) and not dist.any()   # every d is 0
    pos, dist, defined = ref.track(np.array([0.5, np.nan, 0.25] * 100, np.float32), 64, 7, 4, 5)
    assert not defined and not pos.any() and not dist.any() and len(pos) == ref.frames(300, 64, 4, 5)


# ---- the Python layers ----

def test_python_refusals_come_before_the_library(monkeypatch):
    import torch
    from simwhisper_codec_amd import _lib, degrade, ops
    from simwhisper_codec_amd._lib import SwcError

    def no_library():
        raise AssertionError("a refused call reached the library")
    monkeypatch.setattr(_lib, "load", no_library)
    x = [torch.zeros(1600)]
    cases = [
        (lambda: ops.stretch(x, 4, 5), "stretch: expected the input rows on one HIP device"),
        (lambda: degrade.time_stretch(x, 0.8), "time_stretch: expected the waveform rows on one HIP device"),
        (lambda: degrade.pitch_shift(x, semitones=2), "pitch_shift: expected the waveform rows on one HIP device"),
        (lambda: degrade.apply(x, [{"speed": 0.8}]), "apply: expected the waveform rows on one HIP device"),
        (lambda: ops.stretch([torch.zeros(1600, dtype=torch.float64)], 4, 5), "input row is a 1-D f32 tensor"),
        (lambda: degrade.time_stretch([torch.zeros(1600, dtype=torch.int16)], 0.8), "a waveform row is a 1-D f32 tensor"),
        (lambda: degrade.pitch_shift([torch.zeros(2, 1600)], semitones=2), "a waveform row is a 1-D f32 tensor"),
        (lambda: degrade.time_stretch([], 0.8), "0 waveform rows"),
        (lambda: degrade.time_stretch(x, 0.0), "time_stretch: speed=0.0: a finite number > 0"),
        (lambda: degrade.time_stretch(x, -1.25), "time_stretch: speed=-1.25: a finite number > 0"),
        (lambda: degrade.time_stretch(x, float("nan")), "time_stretch: speed=nan: a finite number > 0"),
        (lambda: degrade.time_stretch(x, float("inf")), "time_stretch: speed=inf: a finite number > 0"),
        (lambda: degrade.time_stretch(x, "fast"), "time_stretch: speed='fast': a finite number > 0"),
        (lambda: degrade.time_stretch(x, 4.5), "time_stretch: speed=4.5: between 1/4 and 4"),
        (lambda: degrade.time_stretch(x, 0.2), "time_stretch: speed=0.2: between 1/4 and 4"),
        (lambda: degrade.time_stretch(x, [0.8, 1.25]), "time_stretch: 2 values of speed for 1 waveforms"),
        (lambda: degrade.time_stretch(x, 0.8, window_ms=200.0), "time_stretch: window_ms=200.0, search_ms=8.0 at 16000 Hz give W=3200"),
        (lambda: degrade.time_stretch(x, 0.8, search_ms=100.0), "give W=512, D=1600"),
        (lambda: degrade.pitch_shift(x, semitones=12.5), "pitch_shift: semitones=12.5: at most 12 up or down"),
        (lambda: degrade.pitch_shift(x, semitones=-13), "pitch_shift: semitones=-13.0: at most 12 up or down"),
        (lambda: degrade.pitch_shift(x, semitones=2, ratio=1.125), "pitch_shift: give semitones= or ratio= (one of them)"),
        (lambda: degrade.pitch_shift(x), "pitch_shift: give semitones= or ratio= (one of them)"),
        (lambda: degrade.pitch_shift(x, ratio=2.5), "pitch_shift: ratio=2.5: between 0.5 and 2"),
        (lambda: degrade.pitch_shift(x, semitones=float("nan")), "pitch_shift: semitones=nan: a finite number"),
        (lambda: ops.stretch(x, 5, 1), "stretch: speed 5/1"),
        (lambda: ops.stretch(x, 1, 5), "stretch: speed 1/5"),
        (lambda: ops.stretch(x, 0, 1), "stretch: speed 0/1"),
        (lambda: ops.stretch(x, 4, 5, W=20), "stretch: W=20: a multiple of 8 in 16..2048"),
        (lambda: ops.stretch(x, 4, 5, D=1025), "stretch: D=1025 (0..1024)"),
        (lambda: ops.stretch(x, 4, 5, want=("out", "taps")), "stretch: want=('out', 'taps')"),
    ]
    for call, text in cases:
        with pytest.raises(SwcError, match=re.escape(text)):
            call()


def test_the_resamplers_table_is_checked_on_the_host(monkeypatch):
    from simwhisper_codec_amd import degrade, metrics
    from simwhisper_codec_amd._lib import SwcError
    for p, q in ((9, 8), (8, 9), (55, 49), (63, 64), (2, 1), (1, 2), (1, 1)):
        degrade._resample_table_fits("pitch_shift", p, q)
    monkeypatch.setattr(metrics, "RESAMPLE_MAX_LDS_FLOATS", 1000)
    with pytest.raises(SwcError, match="RESAMPLE_MAX_LDS_FLOATS = 1000 fit"):
        degrade._resample_table_fits("pitch_shift", 55, 49)


def test_pitch_ratio_and_its_error_in_cents():
    from fractions import Fraction
    from simwhisper_codec_amd import degrade
    r, f = degrade._pitch_ratio("t", 2, None)
    assert f == Fraction(2.0 ** (2 / 12)).limit_denominator(64) == Fraction(55, 49) and r == 2.0 ** (2 / 12)
    assert degrade._pitch_ratio("t", None, 1.125)[1] == Fraction(9, 8) and degrade._pitch_ratio("t", 12, None)[1] == 2
    assert degrade._pitch_ratio("t", -12, None)[1] == Fraction(1, 2) and degrade._pitch_ratio("t", 0, None)[1] == 1
    assert degrade._stretch_window("t", 32.0, 8.0, 16000) == (512, 128) and degrade._stretch_window("t", 32.1, 8.0, 16000) == (520, 128)
    assert degrade._speed_fraction("t", 0.8) == Fraction(4, 5) and degrade._speed_fraction("t", 1.25) == Fraction(5, 4)
    assert degrade._speed_fraction("t", 0.9) == Fraction(9, 10) and degrade._speed_fraction("t", 1) == 1


def test_check_condition_on_the_new_keys():
    from fractions import Fraction
    from simwhisper_codec_amd import degrade
    from simwhisper_codec_amd._lib import SwcError
    for key in ("speed", "semitones", "pitch_ratio", "window_ms", "search_ms"):
        assert key in degrade.CONDITION_KEYS
    for good in ({"speed": 0.8}, {"speed": 1}, {"semitones": -2, "snr_db": 10}, {"pitch_ratio": 1.125, "rt60": 0.3}, {"speed": 1.25, "window_ms": 20, "search_ms": 5},
                 {"speed": None, "semitones": None}):
        degrade.check_condition("t", good)
    for bad, text in (({"speed": 0}, "speed=0"), ({"speed": float("nan")}, "speed=nan"), ({"speed": 5}, "between 1/4 and 4"),
                      ({"semitones": 13}, "at most 12"), ({"semitones": 1, "pitch_ratio": 1.1}, "one of them"), ({"pitch_ratio": 3}, "between 0.5 and 2"),
                      ({"speed": 0.8, "window_ms": 500}, "W=8000"), ({"speed": 0.8, "search_ms": -1}, "D=-16"), ({"stretch": 0.8}, "keys out of")):
        with pytest.raises(SwcError, match=re.escape(text)):
            degrade.check_condition("t", bad)
    degrade.check_condition("t", {"speed": 0.8, "window_ms": 100}, 16000)              # W = 1600
    with pytest.raises(SwcError, match=re.escape("at 48000 Hz give W=4800")):      # the same window at another rate
        degrade.check_condition("t", {"speed": 0.8, "window_ms": 100}, 48000)
    degrade.check_condition("t", {"speed": 0.8, "window_ms": 1.0}, 48000)              # W = 48
    with pytest.raises(SwcError, match=re.escape("at 8000 Hz give W=8")):
        degrade.check_condition("t", {"speed": 0.8, "window_ms": 1.0}, 8000)
    assert degrade.condition_speed({}) is None and degrade.condition_speed({"speed": 1.0}) is None
    assert degrade.condition_speed({"speed": 0.8}) == Fraction(4, 5) and degrade.condition_speed({"semitones": 2}) is None


def test_cli_flags_parse_and_default_to_off():
    import inference
    p = inference.build_parser()
    a = p.parse_args([])
    assert a.time_stretch is None and a.pitch_shift is None
    a = p.parse_args(["--mode", "encode", "--time_stretch", "0.9", "--pitch_shift", "-2"])
    assert (a.time_stretch, a.pitch_shift) == (0.9, -2.0)
    with pytest.raises(SystemExit):
        p.parse_args(["--time_stretch", "fast"])
    with pytest.raises(SystemExit, match="--time_stretch / --pitch_shift degrade the input of --mode encode and roundtrip"):
        inference.main(["--mode", "decode", "--time_stretch", "0.9", "--device", "cpu"])
    with pytest.raises(SystemExit, match="--time_stretch / --pitch_shift degrade the input of --mode encode and roundtrip"):
        inference.main(["--mode", "decode", "--pitch_shift", "2", "--device", "cpu"])
    with pytest.raises(SystemExit, match="--add_noise_snr / --reverb_rt60 degrade the input of --mode encode and roundtrip"):
        inference.main(["--mode", "decode", "--add_noise_snr", "10", "--device", "cpu"])
