"""include/swc_degrade.h without a GPU: the ABI (declarations == table == exports, argument counts, a table apart from every
other table and header, the #defines), every argument check before any launch, the workspace formula, the numpy restatement
(tests/degrade_ref.py) on Random123's known answers, on the issue's noise values and against np.convolve, the Python refusals
with the loader patched to fail, and the CLI flags.  conv_cases() are the convolution cases the GPU test runs as well."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import degrade_ref as ref  # noqa: E402

NAMES = {"swc_noise", "swc_mix", "swc_convolve_workspace_bytes", "swc_convolve"}
FORBIDDEN = ("swc_activity", "swc_loudness", "swc_align", "swc_lag_", "swc_warp", "swc_stoi", "swc_quality", "swc_spectral", "swc_pitch",
             "swc_dtw", "swc_cepstra", "swc_segmental", "swc_subdtw", "swc_cmvn", "swc_code_usage", "swc_code_compare", "swc_entropy")

CONV_N = (0, 1, 1023, 1024, 1025, 2049, 5000)
CONV_L = (1, 2, 1024, 1025, 2048, 2049)
CONV_D = (0, 1, 1023, 1024, 1025)
# the largest error of degrade_ref.convolve_partitioned (the header's method in complex64 / float32 numpy) against the float64
# definition over (conv_cases() and impulse_cases()) x CONV_N, as a fraction of ||h||_1 max|x|: 5.37e-7, at n = 5000 with the
# unit impulse at k = d = 1023 (4.56e-7 over conv_cases() alone, at L = 1: with one tap ||h||_1 is as small as it gets against
# the transforms' own rounding); rounded up.  The device is gated at 4 x this figure
REF_ERROR = 5.4e-7


def conv_signal(kind, n, seed):
    rng = np.random.default_rng([seed, n, {"x": 0, "h": 1}[kind]])
    return rng.uniform(-1.0, 1.0, n).astype(np.float32)


def conv_cases():
    """(L, d, extra) of every call; each call takes the rows CONV_N"""
    out = []
    for L in CONV_L:
        for d in CONV_D:
            if d < L:
                for extra in sorted({0, L - 1}):
                    out.append((L, d, extra))
    return out


IMPULSE_K = (0, 1, 1023, 1024, 1025, 2047, 2048)


def impulse_cases():
    """(k, d): a unit impulse at tap k (L = k + 1) with the direct path at d, extra = 0; each call takes the rows CONV_N"""
    return [(k, d) for k in IMPULSE_K for d in sorted({0, k})]


def impulse(k):
    h = np.zeros(k + 1, dtype=np.float32)
    h[k] = 1
    return h


def shifted(x, k, d):
    """what a unit impulse at tap k gives: y[i] = x[i + d - k]"""
    want = np.zeros(len(x))
    src = np.arange(len(x)) + d - k
    ok = (src >= 0) & (src < len(x))
    want[ok] = x[src[ok]]
    return want


def _header(name="swc_degrade.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


def _lib():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    return _lib, _lib.load()


# ---- ABI ----

def test_degrade_header_declarations_are_bound():
    _l, lib = _lib()
    declared = _declared("swc_degrade.h")
    assert declared == NAMES == set(_l.DEGRADE_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)                       # exported by the library
        argtypes, restype = _l.DEGRADE_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    seen = {}
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        seen[m.group(1)] = len(m.group(2).split(","))
    assert seen == {n: len(_l.DEGRADE_SIGNATURES[n][0]) for n in NAMES}
    assert [seen[n] for n in sorted(NAMES)] == [17, 4, 17, 9]


def test_degrade_table_is_apart_from_the_others():
    from simwhisper_codec_amd import _lib, build
    mine = set(_lib.DEGRADE_SIGNATURES)
    assert not mine & set(_lib.exported_symbols())
    others = {k: v for k, v in vars(_lib).items() if (k.endswith("SIGNATURES") or k == "PLAIN") and k != "DEGRADE_SIGNATURES"}
    assert len(others) >= 19
    for other in others.values():
        assert not mine & set(other)
    text = _header()
    for word in FORBIDDEN:
        assert word not in text, word
    for name in mine:
        text = text.replace(name, " ")
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "swc_degrade.h":
            assert not mine & _declared(h)
            for name in mine:
                assert name not in _header(h), (h, name)
            for name in _declared(h):   # the new header's text names no function that another table owns
                assert name not in text, (h, name)
    for other in others.values():
        for name in other:
            assert name not in text, name
    assert "swc_degrade.hip" in build.SOURCES and "swc_degrade.hip" not in build.EXTRA_FLAGS


def test_defines_agree_with_the_bindings():
    from simwhisper_codec_amd import _lib
    d = {k: eval(v, {}) for k, v in re.findall(r"#define (SWC_\w+) (\(?[-\d <]+\)?)\s", _header())}
    assert d["SWC_CONV_MAX_TAPS"] == _lib.DEGRADE_MAX_TAPS == ref.MAX_TAPS == 131072
    assert d["SWC_CONV_BLOCK"] == _lib.DEGRADE_BLOCK == ref.N == 1024
    assert d["SWC_CONV_MAX_N"] == _lib.DEGRADE_MAX_N == 1 << 30
    assert d["SWC_CONV_MAX_IRS"] == _lib.DEGRADE_MAX_IRS == 65535
    assert d["SWC_DEGRADE_CHUNK"] == _lib.DEGRADE_CHUNK == 4096
    assert (d["SWC_MIX_UNMIXED"], d["SWC_MIX_OVER"]) == (_lib.DEGRADE_UNMIXED, _lib.DEGRADE_OVER) == (ref.UNMIXED, ref.OVER) == (1, 2)
    assert len(d) == 7


def test_workspace_bytes_is_the_headers_formula():
    _l, lib = _lib()
    for B, max_n, R, max_L in ((1, 0, 1, 1), (3, 1, 2, 1024), (33, 1024, 1, 1025), (7, 1025, 6, 2049), (65535, 5000, 65535, 131072),
                               (0, 480000, 1, 16000), (32, 1 << 30, 1, 1)):
        assert lib.swc_convolve_workspace_bytes(B, max_n, R, max_L) == ref.workspace_bytes(B, max_n, R, max_L)
    for bad in ((-1, 10, 1, 1), (65536, 10, 1, 1), (1, -1, 1, 1), (1, (1 << 30) + 1, 1, 1), (1, 10, 0, 1), (1, 10, 65536, 1), (1, 10, 1, 0),
                (1, 10, 1, 131073)):
        assert lib.swc_convolve_workspace_bytes(*bad) == -1, bad


def test_every_argument_check_comes_before_any_launch():
    """host memory stands in for device memory: a call that got as far as a launch would not return SWC_E_ARG"""
    _l, lib = _lib()
    buf = (C.c_char * 8192)()
    p = C.addressof(buf)
    p = p + (-p) % 256

    good = dict(seed=1, ids=p, n=p + 64, first=0, out=p + 1024, ld=16, cols=16, B=2)

    def noise(**kw):
        a = dict(good, **kw)
        return lib.swc_noise(a["seed"], a["ids"], a["n"], a["first"], a["out"], a["ld"], a["cols"], a["B"], None)

    for kw in (dict(B=-1), dict(B=65536), dict(ids=None), dict(n=None), dict(out=None), dict(first=-1), dict(cols=17), dict(cols=-1),
               dict(ids=p + 4), dict(n=p + 68), dict(out=p + 1026)):
        assert noise(**kw) == -1, kw
        assert b"swc_noise" in lib.swc_last_error()
    assert noise(B=0) == 0 and noise(B=0, ids=None, n=None, out=None) == 0 and noise(cols=0) == 0

    gm = dict(x=p, nx=p + 64, v=p + 128, nv=p + 192, lx=p + 256, slx=8, ln=p + 264, sln=8, snr=p + 512, ssnr=1, out=p + 1024, ld=16, cols=16,
              gains=p + 2048, flags=p + 2112, B=2)

    def mix(**kw):
        a = dict(gm, **kw)
        return lib.swc_mix(a["x"], a["nx"], a["v"], a["nv"], a["lx"], a["slx"], a["ln"], a["sln"], a["snr"], a["ssnr"], a["out"], a["ld"],
                           a["cols"], a["gains"], a["flags"], a["B"], None)

    for kw in (dict(B=-1), dict(B=65536), dict(x=None), dict(nx=None), dict(v=None), dict(nv=None), dict(lx=None), dict(ln=None),
               dict(snr=None), dict(out=None, gains=None, flags=None), dict(slx=-1), dict(sln=-8), dict(ssnr=-1), dict(cols=17), dict(cols=-1),
               dict(lx=p + 260), dict(out=p + 1025), dict(flags=p + 2113), dict(nx=p + 68)):
        assert mix(**kw) == -1, kw
        assert b"swc_mix" in lib.swc_last_error()
    assert mix(B=0) == 0 and mix(B=0, x=None, nx=None, v=None, nv=None, lx=None, ln=None, snr=None) == 0

    ws = lib.swc_convolve_workspace_bytes(2, 100, 2, 2049)
    gc = dict(x=p, n=p + 64, max_n=100, h=p + 128, hl=p + 192, R=2, L=2049, hi=p + 256, d=5, extra=7, out=p + 1024, ld=128, cols=107,
              ws=p + 4096, wsb=ws, B=2)

    def conv(**kw):
        a = dict(gc, **kw)
        return lib.swc_convolve(a["x"], a["n"], a["max_n"], a["h"], a["hl"], a["R"], a["L"], a["hi"], a["d"], a["extra"], a["out"], a["ld"],
                                a["cols"], a["ws"], a["wsb"], a["B"], None)

    for kw in (dict(B=-1), dict(B=65536), dict(x=None), dict(n=None), dict(h=None), dict(hl=None), dict(hi=None), dict(out=None), dict(ws=None),
               dict(L=0), dict(L=131073), dict(d=2049), dict(d=-1), dict(d=5000), dict(extra=2049), dict(extra=-1), dict(cols=129),
               dict(cols=-1), dict(wsb=ws - 1), dict(wsb=0), dict(R=0), dict(R=65536), dict(max_n=-1), dict(max_n=(1 << 30) + 1),
               dict(ws=p + 4096 + 128), dict(out=p + 1026), dict(n=p + 68), dict(hi=p + 260)):
        assert conv(**kw) == -1, kw
        assert b"swc_convolve" in lib.swc_last_error()
    assert conv(B=0) == 0 and conv(B=0, x=None, n=None, h=None, hl=None, out=None, ws=None, wsb=0) == 0
    assert conv(R=1, hi=None, B=0) == 0        # h_index may be null with one response


# ---- the reference ----

def test_philox_reproduces_random123():
    kat = [((0,) * 4, (0,) * 2, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{w:08x}" for w in ref.philox4x32_10(ctr, key)) == want


def test_reference_noise_values():
    assert [ref.noise_v(0x123456789, 7, i) for i in range(4)] == [168346, -50660, 75042, -73636]
    x = ref.noise(0x123456789, 7, 4)
    assert x.dtype == np.float32 and list(x * 2.0 ** 19) == [168346, -50660, 75042, -73636]
    # the vector form is the scalar form, also past 2^32 in the index and in the stream id
    for s, first in ((7, 0), (2 ** 40 + 3, 2 ** 32 - 2), (2 ** 64 - 1, 2 ** 33 + 5)):
        assert list(ref.noise(5, s, 6, first) * 2.0 ** 19) == [ref.noise_v(5, s, first + i) for i in range(6)]
    big = ref.noise(1, 2, 1 << 16).astype(np.float64)
    assert np.abs(big).max() < 1 and abs(big.mean()) < 4e-3
    assert abs(big.var() / ((8 / 3) * (2 ** 32 - 1) / 2 ** 38) - 1) < 0.02


def test_reference_fmaf_is_fused():
    a = np.array([1 + 2 ** -23, 3.0, 0.1, 2 ** -19], dtype=np.float32)
    b = np.array([1 - 2 ** -23, 1 / 3, 0.7, 2 ** -20], dtype=np.float32)
    c = np.array([-1.0, -1.0, 1e-9, 1.0], dtype=np.float32)
    import fractions
    want = [np.float32(float(fractions.Fraction(float(x)) * fractions.Fraction(float(y)) + fractions.Fraction(float(z)))) for x, y, z in zip(a, b, c)]
    assert list(ref.fmaf(a, b, c)) == want
    assert ref.fmaf(a, b, c)[0] == np.float32(-2.0 ** -46)     # what a separate multiply and add would lose


def test_partitioned_reference_matches_np_convolve():
    worst = 0.0
    for n, L, d, extra in ((5000, 1, 0, 0), (1, 1, 0, 0), (1023, 2, 1, 1), (1025, 1024, 1023, 1023), (2049, 1025, 1024, 0), (5000, 2049, 1025, 2048),
                           (1024, 2048, 0, 2047), (0, 1025, 3, 1024)):
        x, h = conv_signal("x", n, 1), conv_signal("h", L, 2)
        y64 = ref.convolve64(x, h, d, extra)
        direct = np.array([sum(float(h[k]) * float(x[i + d - k]) for k in range(L) if 0 <= i + d - k < n) for i in range(min(n + extra, 3))])
        assert np.allclose(y64[:3], direct, rtol=0, atol=1e-12)
        y = ref.convolve_partitioned(x, h, d, extra)
        assert y.dtype == np.float32 and y.shape == y64.shape == (n + extra,)
        if n:
            worst = max(worst, float(np.abs(y - y64).max() / (np.abs(h).sum() * np.abs(x).max())))
    x = conv_signal("x", 5000, 1)       # the worst of all the cases: it sets the figure
    worst = max(worst, float(np.abs(ref.convolve_partitioned(x, impulse(1023), 1023, 0) - shifted(x, 1023, 1023)).max() / np.abs(x).max()))
    assert 0.9 * REF_ERROR < worst <= REF_ERROR
    # a unit impulse at tap k shifts the row
    x = conv_signal("x", 1500, 3)
    for k, d in impulse_cases():
        want = shifted(x, k, d)
        assert np.array_equal(ref.convolve64(x, impulse(k), d, 0), want)
        assert np.abs(ref.convolve_partitioned(x, impulse(k), d, 0) - want).max() <= REF_ERROR * np.abs(x).max()


def test_gain_and_mix_reference():
    g, mixed = ref.gain(-26.0, -13.8, 10.0, 5)
    assert mixed and g == np.float32(10.0 ** ((-26.0 + 13.8 - 10.0) / 20.0))
    for bad in ((float("nan"), 0, 0, 5), (0, float("inf"), 0, 5), (0, 0, float("-inf"), 5), (0, 0, 0, 0)):
        assert ref.gain(*bad) == (np.float32(0), False)
    x = np.array([0.5, -0.25, 0.125, 0.9, 0.0], dtype=np.float32)
    v = np.array([0.5, -0.5], dtype=np.float32)
    out, flag = ref.mix(x, v, np.float32(0.5), True)
    assert list(out) == [0.75, -0.5, 0.375, 0.65, 0.25] and flag == 0
    out, flag = ref.mix(x, v, np.float32(1.0), True)
    assert flag == ref.OVER or np.abs(out).max() <= 1
    out, flag = ref.mix(x, v, np.float32(0), False)
    assert np.array_equal(out, x) and flag == ref.UNMIXED


# ---- the Python layers ----

def test_python_refusals_come_before_the_library(monkeypatch):
    import torch
    from simwhisper_codec_amd import _lib, degrade, ops
    from simwhisper_codec_amd._lib import SwcError

    def no_library():
        raise AssertionError("a refused call reached the library")
    monkeypatch.setattr(_lib, "load", no_library)
    x = [torch.zeros(160)]
    cases = [
        (lambda: degrade.add_noise(x, 10.0), "add_noise: expected the waveform rows on one HIP device"),
        (lambda: degrade.reverberate(x, rt60=0.3), "reverberate: expected the waveform rows on one HIP device"),
        (lambda: degrade.apply(x, [{"snr_db": 10}]), "apply: expected the waveform rows on one HIP device"),
        (lambda: degrade.white_noise([5], 1, device="cpu"), "white_noise: the degradations are HIP kernels"),
        (lambda: degrade.synthetic_rir(0.3, device="cpu"), "synthetic_rir: the degradations are HIP kernels"),
        (lambda: ops.noise([5], 1, device="cpu"), "noise: the generator is a HIP kernel"),
        (lambda: ops.mix(x, x, None, None, None), "mix: expected the speech rows on one HIP device"),
        (lambda: ops.convolve(x, x), "convolve: expected the input rows on one HIP device"),
        (lambda: degrade.add_noise([torch.zeros(160, dtype=torch.float64)], 10.0), "a waveform row is a 1-D f32 tensor"),
        (lambda: degrade.add_noise([torch.zeros(160, dtype=torch.int16)], 10.0), "a waveform row is a 1-D f32 tensor"),
        (lambda: degrade.add_noise([torch.zeros(2, 160)], 10.0), "a waveform row is a 1-D f32 tensor"),
        (lambda: degrade.reverberate([torch.zeros(2, 160)], rt60=0.3), "a waveform row is a 1-D f32 tensor"),
        (lambda: degrade.add_noise([], 10.0), "0 waveform rows"),
        (lambda: degrade.add_noise(x, 10.0, noise=x * 2), "add_noise: 1 waveforms and 2 noise rows"),
        (lambda: degrade.add_noise(x, [10.0, 20.0]), "add_noise: 2 values of snr_db for 1 waveforms"),
        (lambda: ops.mix(x, x * 2, None, None, None), "mix: 1 speech rows and 2 noise rows"),
        (lambda: degrade.add_noise(x, float("nan")), "add_noise: snr_db=nan: a finite number"),
        (lambda: degrade.add_noise(x, float("inf")), "add_noise: snr_db=inf: a finite number"),
        (lambda: degrade.add_noise(x, "loud"), "add_noise: snr_db='loud': a finite number"),
        (lambda: degrade.add_noise(x, 10.0, level="peak"), "add_noise: level='peak'"),
        (lambda: degrade.add_noise(x, 10.0, sample_rate=7999), "activity: sample_rate=7999"),
        (lambda: degrade.reverberate(x, rt60=0.0), "reverberate: rt60=0.0"),
        (lambda: degrade.reverberate(x, rt60=-1.0), "reverberate: rt60=-1.0"),
        (lambda: degrade.reverberate(x, rt60=float("nan")), "reverberate: rt60=nan: a finite number"),
        (lambda: degrade.synthetic_rir(0.0), "synthetic_rir: rt60=0.0"),
        (lambda: degrade.synthetic_rir(8.2), "synthetic_rir: an impulse response of 131201 taps (at most 131072"),
        (lambda: degrade.reverberate(x, rt60=8.2), "reverberate: an impulse response of 131201 taps (at most 131072"),
        (lambda: degrade.reverberate(x, rir=torch.zeros(131073)), "reverberate: an impulse response is a 1-D tensor of 1..131072 taps"),
        (lambda: degrade.reverberate(x, rir=torch.zeros(0)), "reverberate: an impulse response is a 1-D tensor of 1..131072 taps"),
        (lambda: degrade.reverberate(x), "reverberate: give rir= or rt60="),
        (lambda: degrade.reverberate(x, rir=torch.zeros(4), rt60=0.3), "reverberate: give rir= or rt60="),
        (lambda: degrade.apply(x, [{"snr": 10}]), "apply: a condition is a dict with keys out of"),
        (lambda: degrade.apply(x, [{}, {"rt60": 0}]), "apply: rt60=0: a time > 0"),
        (lambda: degrade.apply(x, [{"snr_db": float("nan")}]), "apply: snr_db=nan: a finite number"),
    ]
    for call, text in cases:
        with pytest.raises(SwcError, match=re.escape(text)):
            call()


def test_cli_flags_parse_and_default_to_off():
    import inference
    p = inference.build_parser()
    a = p.parse_args([])
    assert a.add_noise_snr is None and a.reverb_rt60 is None and a.noise_seed == 0
    a = p.parse_args(["--mode", "encode", "--add_noise_snr", "10", "--noise_seed", "7", "--reverb_rt60", "0.4"])
    assert (a.add_noise_snr, a.noise_seed, a.reverb_rt60) == (10.0, 7, 0.4)
    with pytest.raises(SystemExit):
        p.parse_args(["--add_noise_snr", "loud"])
    with pytest.raises(SystemExit, match="--add_noise_snr / --reverb_rt60 degrade the input of --mode encode and roundtrip"):
        inference.main(["--mode", "decode", "--add_noise_snr", "10", "--device", "cpu"])
    assert inference.stream_id_of("a/b/utt1.wav") == inference.stream_id_of("/c/utt1.wav") != inference.stream_id_of("utt2.wav")
    assert 0 <= inference.stream_id_of("utt1.wav") < 2 ** 64
