"""swc_align (the lag, overlap, correlation and level ratio of every pair in one call), the parts that need no GPU: the C-ABI of
include/swc_align.h (declarations == bindings == exports, a table apart from the other eight; every argument check before any
launch; the workspace arithmetic against its documented formula), properties of the numpy restatement (tests/align_ref.py):
shift equivariance, the tie rule, no positive c, a negated pair, the gain; the envelope mode on pairs that share an envelope
and nothing else; the refusals of the Python surface and the flags of the four tools."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_ref as ref  # noqa: E402


# ---- ABI and arguments ----

def _header(name="swc_align.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


def test_align_header_declarations_are_bound():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    declared = _declared("swc_align.h")
    assert declared == {"swc_align", "swc_align_workspace_bytes"} == set(_lib.ALIGN_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)                       # exported by the library
        argtypes, restype = _lib.ALIGN_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    seen = set()
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        assert len(m.group(2).split(",")) == len(_lib.ALIGN_SIGNATURES[m.group(1)][0]), m.group(1)
        seen.add(m.group(1))
    assert seen == declared
    assert len(_lib.ALIGN_SIGNATURES["swc_align"][0]) == 16 and len(_lib.ALIGN_SIGNATURES["swc_align_workspace_bytes"][0]) == 4


def test_align_table_is_apart_from_the_other_eight():
    from simwhisper_codec_amd import _lib
    mine = set(_lib.ALIGN_SIGNATURES)
    assert not mine & set(_lib.exported_symbols())
    for other in (_lib.SIGNATURES, _lib.PLAIN, _lib.AUDIO_SIGNATURES, _lib.CODES_SIGNATURES, _lib.METRICS_SIGNATURES,
                  _lib.QUALITY_SIGNATURES, _lib.FLAC_SIGNATURES, _lib.FLAC_IO_SIGNATURES, _lib.FLAC_ENC_SIGNATURES,
                  _lib.SPECTRAL_SIGNATURES, _lib.PITCH_SIGNATURES):
        assert not mine & set(other)
    for h in ("swc.h", "swc_audio.h", "swc_codes.h", "swc_metrics.h", "swc_quality.h", "swc_flac.h", "swc_flac_enc.h", "swc_spectral.h",
              "swc_pitch.h"):
        assert not mine & _declared(h)
        assert "swc_align" not in _header(h)


def test_constants_agree_with_the_header_and_the_reference():
    from simwhisper_codec_amd import _lib, ops
    hdr = _header()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert (val("SWC_ALIGN_WAVEFORM"), val("SWC_ALIGN_ENVELOPE")) == (_lib.ALIGN_WAVEFORM, _lib.ALIGN_ENVELOPE) == (ref.WAVEFORM, ref.ENVELOPE)
    assert ops.ALIGN_MODES == ref.MODES
    assert val("SWC_ALIGN_MAX_LAG") == _lib.ALIGN_MAX_LAG == ref.MAX_LAG == 32768
    assert val("SWC_ALIGN_MAX_N") == _lib.ALIGN_MAX_N == ref.MAX_N == 1 << 22
    assert (val("SWC_ALIGN_CHUNK"), val("SWC_ALIGN_LAG_BLOCK"), val("SWC_ALIGN_SPILL")) == (_lib.ALIGN_CHUNK, _lib.ALIGN_LAG_BLOCK, _lib.ALIGN_SPILL)
    assert (val("SWC_ALIGN_INFO"), val("SWC_ALIGN_VALUES")) == (_lib.ALIGN_INFO, _lib.ALIGN_VALUES) == (4, 4)
    # the bounds the header states: a digit's products between two spills fit int32, every sum converts to double exactly
    assert (_lib.ALIGN_SPILL // 2) * 2 * 128 * 32767 < 2 ** 31 and _lib.ALIGN_MAX_N * 32767 ** 2 < 2 ** 53
    assert "Bits" in hdr and "depend on its samples, L and the mode only" in hdr


def test_build_sees_a_touched_align_header(monkeypatch):
    from simwhisper_codec_amd import build
    build.build_library()
    assert not build._stale()
    assert "swc_align.hip" in build.SOURCES
    hdr = os.path.join(ROOT, "include", "swc_align.h")
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

    def call(x=p, y=p, n_x=p, n_y=p, max_nx=9000, max_ny=8000, L=800, mode=0, info=p, values=p, xc=p, ldc=None, ws=p, ws_bytes=None, B=2):
        ldc = 2 * L + 1 if ldc is None else ldc
        if ws_bytes is None:
            ws_bytes = 1 << 40
        return lib.swc_align(x, y, n_x, n_y, max_nx, max_ny, L, mode, info, values, xc, ldc, ws, ws_bytes, B, None)

    need = lib.swc_align_workspace_bytes(2, 9000, 8000, 800)
    assert need > 0
    odd = C.c_void_p(p.value + 4)
    for kw, word in [(dict(x=None), b"null"), (dict(y=None), b"null"), (dict(n_x=None), b"null"), (dict(n_y=None), b"null"),
                     (dict(ws=None), b"null"),
                     (dict(L=-1), b"search range"), (dict(L=32769), b"search range"),
                     (dict(mode=2), b"mode"), (dict(mode=-1), b"mode"),
                     (dict(ldc=1600), b"ldc"), (dict(ldc=0), b"ldc"),
                     (dict(B=65536), b"B="), (dict(B=-1), b"B="),
                     (dict(max_nx=(1 << 22) + 1), b"out of range"), (dict(max_ny=(1 << 22) + 1), b"out of range"),
                     (dict(max_nx=-1), b"out of range"), (dict(max_ny=-1), b"out of range"),
                     (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"),
                     (dict(ws=odd), b"aligned")]:
        assert call(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    # nothing to do: no launch, no device needed.  ldc does not matter without xc; every subset of outputs; both limits
    assert call(B=0) == 0 and call(B=0, ws_bytes=lib.swc_align_workspace_bytes(0, 9000, 8000, 800)) == 0
    assert call(B=0, xc=None, ldc=0) == 0
    for info in (p, None):
        for values in (p, None):
            for xc in (p, None):
                assert call(B=0, info=info, values=values, xc=xc) == 0
    assert call(B=0, L=0, ldc=1) == 0 and call(B=0, L=32768, max_nx=1 << 22, max_ny=1 << 22, mode=1) == 0
    del keep


def test_workspace_bytes_against_the_documented_formula():
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    up = lambda v: (v + 255) & ~255
    for B, nx, ny, L in [(1, 0, 0, 0), (1, 1, 1, 0), (3, 9000, 8000, 800), (32, 160000, 160000, 16000), (33, 100, 5000, 1), (0, 5000, 5000, 800),
                         (65535, 1 << 22, 1 << 22, 32768), (5, 4096, 4097, 255)]:
        want = up(2 * B * 4) + up(2 * B * 8) + up(8 * B * 8) + up(B * (2 * L + 1) * 8)
        assert lib.swc_align_workspace_bytes(B, nx, ny, L) == want, (B, nx, ny, L)
        assert ops.align_workspace_bytes(B, nx, ny, L) == want and want % 256 == 0
    for bad in [(-1, 10, 10, 1), (65536, 10, 10, 1), (1, -1, 10, 1), (1, 10, -1, 1), (1, (1 << 22) + 1, 10, 1), (1, 10, (1 << 22) + 1, 1),
                (1, 10, 10, -1), (1, 10, 10, 32769)]:
        assert lib.swc_align_workspace_bytes(*bad) == -1, bad
        with pytest.raises(_lib.SwcError):
            ops.align_workspace_bytes(*bad)


# ---- the reference on itself ----

def _speechlike(n, seed):
    """noise with a slow envelope: a sharp correlation peak and a level that moves"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * (0.2 + np.abs(np.sin(np.arange(n) / 700.0)))).astype(np.float32) * np.float32(0.3)


@pytest.mark.parametrize("mode", ["waveform", "envelope"])
def test_shift_equivariance(mode):
    """the lag of a pair cut d samples later is exactly d larger: a zero-padded shift, not a rotation"""
    x = _speechlike(3000, 1)
    y0 = (0.7 * ref.delayed(x, 4) + 0.01 * np.random.default_rng(2).standard_normal(3000)).astype(np.float32)
    base = int(ref.align(x, y0, 64, mode)["info"][0])
    assert base == 4
    for d in (-40, -7, -1, 1, 2, 33, 60):
        r = ref.align(x, ref.delayed(y0, d), 64, mode)
        lag, x0, y0_, m = (int(v) for v in r["info"])
        assert lag == base + d, (mode, d, lag)
        assert (x0, y0_) == (max(0, -lag), max(0, lag)) and m == 3000 - abs(lag)
    # a true lag beyond the range cannot be reported: the answer stays inside -L .. L
    assert abs(int(ref.align(x, ref.delayed(y0, 100), 64, mode)["info"][0])) <= 64


def test_the_tie_rule():
    """x = one pulse; y = three equal pulses at +3, -3 and +5 from it: c is equal at the three lags, and +3 wins (the smaller
    |d| beats 5, d >= 0 beats -3)"""
    x = np.zeros(32, np.float32); x[10] = 1.0
    y = np.zeros(32, np.float32); y[[13, 7, 15]] = 1.0
    r = ref.align(x, y, 8, "waveform")
    c = r["xc"]
    assert c[8 + 3] == c[8 - 3] == c[8 + 5] > 0 and (np.delete(c, [5, 11, 13]) == 0).all()
    assert r["info"].tolist() == [3, 0, 3, 29]
    y[13] = 0.0
    assert ref.align(x, y, 8, "waveform")["info"][0] == -3         # |d| = 3 beats 5 whatever the sign
    y[7] = 0.0
    assert ref.align(x, y, 8, "waveform")["info"][0] == 5
    assert ref.choose(np.array([5, 0, 5], np.int64), 1) == 1 and ref.choose(np.array([5, 5, 5], np.int64), 1) == 0
    assert ref.choose(np.array([6, 5, 5], np.int64), 1) == -1


def test_no_positive_c_gives_lag_zero_and_a_negated_pair_has_negative_corr():
    x = np.zeros(16, np.float32); x[4] = 1.0
    y = np.zeros(16, np.float32); y[5] = -1.0
    r = ref.align(x, y, 4, "waveform")
    assert (r["xc"] <= 0).all() and r["xc"].min() < 0 and r["info"].tolist() == [0, 0, 0, 16]
    assert r["values"][0] == 0.0                       # c[0] = 0 over energies that are not
    x = _speechlike(2000, 3)
    r = ref.align(x, -x, 0, "waveform")
    assert r["info"].tolist() == [0, 0, 0, 2000] and r["values"][0] == -1.0 and r["values"][1] == 1.0
    # silence on one side: nothing is positive, no correlation; a silent degraded side has no gain either
    r = ref.align(x, np.zeros(2000, np.float32), 5, "waveform")
    assert r["info"].tolist() == [0, 0, 0, 2000] and np.isnan(r["values"][:2]).all() and not r["xc"].any()
    r = ref.align(np.zeros(2000, np.float32), x, 5, "envelope")
    assert np.isnan(r["values"][0]) and r["values"][1] == 0.0


def test_gain_and_corr_of_a_scaled_copy_are_exact():
    x = _speechlike(2500, 4)
    for mode in ("waveform", "envelope"):
        r = ref.align(x, (np.float32(0.25) * x).astype(np.float32), 16, mode)
        assert r["info"].tolist() == [0, 0, 0, 2500] and r["values"].tolist() == [1.0, 4.0, 0.0, 0.0], (mode, r["values"])
    r = ref.align((x * np.float32(8.0)).astype(np.float32), x, 16, "waveform")
    assert r["values"].tolist() == [1.0, 8.0, 0.0, 0.0]
    y = ref.delayed(x, 9, n=2600)                      # separate lengths: the rows are not cut to the shorter one
    r = ref.align(x, y, 16, "waveform")
    assert r["info"].tolist() == [9, 0, 9, 2500] and r["values"][0] == 1.0


def test_empty_and_undefined_pairs():
    x = _speechlike(100, 5)
    for a, b in ((x[:0], x), (x, x[:0]), (x[:0], x[:0])):
        r = ref.align(a, b, 3, "waveform")
        assert r["info"].tolist() == [0, 0, 0, 0] and np.isnan(r["values"][:2]).all() and not r["values"][2:].any() and not r["xc"].any()
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy(); y[17] = bad
        for a, b in ((x, y), (y, x)):
            r = ref.align(a, b, 3, "envelope")
            assert r["info"].tolist() == [0, 0, 0, 0] and np.isnan(r["values"][:2]).all() and not r["xc"].any()


def test_the_int64_bounds_at_the_limits():
    """full-scale constants: every product is 32767^2; n = 2^22 of them stay below 2^52 and convert to double exactly"""
    q, e, state = ref.quantise(np.full(1000, 1.0, np.float32) * np.float32(1.9999999))
    assert state == "ok" and (q == 32767).all()
    top = ref.MAX_N * 32767 ** 2
    assert 2 ** 51 < top < 2 ** 52 and int(float(top)) == top
    c = ref.xcorr(q, q, 2)
    assert c.tolist() == [998 * 32767 ** 2, 999 * 32767 ** 2, 1000 * 32767 ** 2, 999 * 32767 ** 2, 998 * 32767 ** 2]
    # the envelope sequence stays inside 16 bits
    s = ref.sequence(np.array([32767, 0, -32767, 5], np.int64), ref.ENVELOPE)
    assert s.tolist() == [32767 - 16384, -16384, 32767 - 16384, 5 - 16384]


# ---- the envelope mode earns its place ----

def test_the_envelope_mode_finds_what_the_waveform_mode_cannot():
    """x = env noise_1, y = 0.5 env noise_2 delayed by d (ref.envelope_pair: env = the square of Hann-smoothed white noise,
    independent carriers), n = 32000, L = 800, seeds 0 - 7, d in {0, 5, -333, 700}.  The envelope lag is within 32 samples of d
    for every pair; the waveform mode, which has nothing to lock on, is off by more than 32 on at least half of them.
    Measured with this restatement: envelope worst case 17 samples, waveform off on 21 of the 32 pairs."""
    worst, missed, total = 0, 0, 0
    for seed in range(8):
        for d in (0, 5, -333, 700):
            x, y = ref.envelope_pair(seed, d)
            assert len(x) == len(y) == 32000
            env = int(ref.align(x, y, 800, "envelope")["info"][0])
            wav = int(ref.align(x, y, 800, "waveform")["info"][0])
            worst = max(worst, abs(env - d))
            missed += abs(wav - d) > 32
            total += 1
            assert abs(env - d) <= 32, (seed, d, env)
    print(f"envelope mode: worst |lag - d| = {worst}; waveform mode off by more than 32 on {missed} of {total}")
    assert total == 32 and 2 * missed >= total


# ---- the Python surface and the tools ----

def test_python_surface_refuses_what_it_cannot_do():
    from simwhisper_codec_amd import _lib, metrics
    x = torch.zeros(9000)
    calls = [metrics.stoi, metrics.quality, metrics.estoi, metrics.si_sdr, metrics.spectral, metrics.mel_distance, metrics.stft_distance,
             metrics.lsd, metrics.pitch]
    for f in calls:
        with pytest.raises(_lib.SwcError, match="CPU"):
            f([x], [x], align="waveform", device="cpu")
        with pytest.raises(_lib.SwcError, match="align="):
            f([x], [x], align="pesq")
        with pytest.raises(_lib.SwcError, match="align="):
            f([x], [x], align=True)
        for bad in (-1.0, float("nan"), float("inf"), "soon"):
            with pytest.raises(_lib.SwcError, match="max_lag_ms"):
                f([x], [x], align="envelope", max_lag_ms=bad)
    for f in (metrics.align, metrics.aligned):
        with pytest.raises(_lib.SwcError, match="CPU"):
            f([x], [x], device="cpu")
        with pytest.raises(_lib.SwcError, match="mode="):
            f([x], [x], mode="pesq")
        with pytest.raises(_lib.SwcError, match="at most 32768"):
            f([x], [x], max_lag_ms=2049.0)                       # 32784 samples at 16 kHz
        with pytest.raises(_lib.SwcError, match="max_lag_ms"):
            f([x], [x], max_lag_ms=-0.5)
        with pytest.raises(_lib.SwcError, match="1 reference and 2"):
            f([x], [x, x], device="cuda")
    assert metrics.align_range(16000, 50.0) == 800 and metrics.align_range(16000, 2048.0) == 32768 and metrics.align_range(8000, 0) == 0
    assert metrics.align_range(44100, 50.0) == 2205


def test_stage_with_and_without_the_cut():
    """metrics._stage on the host: rows of unequal lengths (an empty and a one-sample row against five samples among them), a
    float64, an int16 and a non-contiguous row -> contiguous f32 rows with the values of the inputs; cut=True is the common
    prefix of what cut=False gives."""
    from simwhisper_codec_amd import metrics
    g = torch.Generator().manual_seed(5)
    wide = torch.randn(14, generator=g)
    refs = [torch.randn(7, generator=g, dtype=torch.float64), torch.zeros(0), torch.randn(5, generator=g), wide[::2]]
    degs = [torch.randn(4, generator=g), torch.randn(5, generator=g), torch.tensor([-3], dtype=torch.int16),
            torch.tensor([5, -32768, 32767, 0, 1, 2, 3, 4, 9], dtype=torch.int16)]
    assert not refs[3].is_contiguous()
    xu, yu = metrics._stage(refs, degs, "cpu", cut=False)
    xc, yc = metrics._stage(refs, degs, "cpu", cut=True)
    assert [(x.numel(), y.numel()) for x, y in zip(xu, yu)] == [(7, 4), (0, 5), (5, 1), (7, 9)]
    assert [(x.numel(), y.numel()) for x, y in zip(xc, yc)] == [(4, 4), (0, 0), (1, 1), (7, 7)]
    for given, uncut, cut in zip(refs + degs, xu + yu, xc + yc):
        for r in (uncut, cut):
            assert r.dtype == torch.float32 and r.dim() == 1 and r.is_contiguous() and r.device.type == "cpu"
        assert torch.equal(uncut, given.to(torch.float32))
        assert torch.equal(cut, uncut[:cut.numel()])
    d = metrics._stage(refs, degs, "cpu")        # the default is the cut
    assert all(torch.equal(a, b) for a, b in zip(d[0] + d[1], xc + yc))


@pytest.mark.parametrize("tool", ["evaluate_stoi", "evaluate_quality", "evaluate_spectral", "evaluate_pitch"])
def test_tools_parse_the_alignment_flags(tool):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    mod = __import__(tool)
    base = ["--original_dir", "A", "--synthesized_dir", "B"]
    a = vars(mod.build_parser().parse_args(base))
    assert a["align"] == "none" and a["max_lag_ms"] == 50.0
    a = vars(mod.build_parser().parse_args(base + ["--align", "envelope", "--max_lag_ms", "12.5"]))
    assert a["align"] == "envelope" and a["max_lag_ms"] == 12.5
    assert vars(mod.build_parser().parse_args(base + ["--align", "waveform"]))["align"] == "waveform"
    with pytest.raises(SystemExit):
        mod.build_parser().parse_args(base + ["--align", "pesq"])


def test_tool_alignment_summary():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_stoi
    nan = float("nan")
    lines = evaluate_stoi.format_alignment(["a", "b", "c", "d"], [3, -40, 0, 7], [0.9, 0.0, nan, -0.2])
    text = "\n".join(lines)
    assert "mean |lag| 12.500 samples" in text and "largest |lag| 40" in text
    assert "not aligned (corr <= 0 or not defined) (3): b, c, d" in text
    assert "not aligned" not in "\n".join(evaluate_stoi.format_alignment(["a"], [3], [0.5]))
