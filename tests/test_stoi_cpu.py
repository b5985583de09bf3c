"""STOI, the parts that need no GPU: the C-ABI of include/swc_metrics.h (declarations == bindings == exported symbols, apart
from the other three headers; argument checks before any launch), the build wiring, the 10 kHz filter against
scipy.signal.resample_poly, the band edges, and the properties of the float64 reference (tests/stoi_ref.py) that
tests/test_stoi_gpu.py holds the kernels to."""
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

import stoi_ref  # noqa: E402

RATES = (8000, 10000, 16000, 24000, 32000, 48000)


def _declared(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


def test_metrics_header_declarations_are_bound_and_exported():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    declared = _declared("swc_metrics.h")
    assert declared == {"swc_stoi", "swc_stoi_workspace_bytes"} == set(_lib.METRICS_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)
        argtypes, restype = _lib.METRICS_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    # the number of parameters in the header equals the number of bound argument types
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "swc_metrics.h")).read(), flags=re.S)
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        assert len(m.group(2).split(",")) == len(_lib.METRICS_SIGNATURES[m.group(1)][0]), m.group(1)


def test_metrics_table_is_apart_from_the_other_three_headers():
    from simwhisper_codec_amd import _lib
    mine = set(_lib.METRICS_SIGNATURES)
    assert not mine & set(_lib.exported_symbols())
    assert not mine & set(_lib.SIGNATURES) and not mine & set(_lib.PLAIN)
    assert not mine & set(_lib.AUDIO_SIGNATURES) and not mine & set(_lib.CODES_SIGNATURES)
    for h in ("swc.h", "swc_audio.h", "swc_codes.h"):
        assert not mine & _declared(h)
        assert "swc_stoi" not in open(os.path.join(ROOT, "include", h)).read()
    assert _lib.STOI_TILE == 16 and "#define SWC_STOI_TILE 16" in open(os.path.join(ROOT, "include", "swc_metrics.h")).read()


def test_build_knows_the_source_and_the_header(monkeypatch):
    from simwhisper_codec_amd import build
    assert "swc_stoi.hip" in build.SOURCES
    build.build_library()
    assert not build._stale()
    hdr = os.path.join(ROOT, "include", "swc_metrics.h")
    real = os.path.getmtime
    newer = real(build.LIB_PATH) + 10
    monkeypatch.setattr(os.path, "getmtime", lambda p: newer if os.path.abspath(p) == hdr else real(p))   # a touched header
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
    need = lib.swc_stoi_workspace_bytes(2, 9000, 8, 5)
    assert need > 0

    def call(x=p, y=p, n_in=p, max_n=9000, orig=8, new=5, width=58, taps=p, start=p, run=117, d=p, segs=p, ws=p, ws_bytes=need, B=2):
        return lib.swc_stoi(x, y, n_in, max_n, orig, new, width, taps, start, run, d, segs, ws, ws_bytes, B, None)

    odd = C.c_void_p(p.value + 4)
    for kw, word in [(dict(x=None), b"null"), (dict(y=None), b"null"), (dict(n_in=None), b"null"), (dict(taps=None), b"null"),
                     (dict(start=None), b"null"), (dict(d=None), b"null"), (dict(segs=None), b"null"), (dict(ws=None), b"null"),
                     (dict(B=-1), b"B="), (dict(B=65536), b"B="), (dict(orig=0), b"rates"), (dict(new=0), b"rates"),
                     (dict(max_n=-1), b"max_n_in"), (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"),
                     (dict(ws=odd), b"aligned"), (dict(run=0), b"table size"),
                     (dict(orig=441, new=100, width=160, run=320,
                           ws_bytes=lib.swc_stoi_workspace_bytes(2, 9000, 441, 100)), b"does not fit")]:
        assert call(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    assert call(B=0) == 0          # nothing to do: no launch, no device needed
    del keep


def test_workspace_bytes_and_its_python_mirror():
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    for B, n, o, w in [(1, 0, 8, 5), (1, 255, 1, 1), (1, 256, 1, 1), (3, 9000, 8, 5), (32, 160000, 8, 5), (4, 48000, 24, 5), (2, 7000, 4, 5)]:
        L = ops.stoi_workspace_layout(B, n, o, w)
        assert lib.swc_stoi_workspace_bytes(B, n, o, w) == L["total"] == ops.stoi_workspace_bytes(B, n, o, w)
        assert L["n10max"] == (n if o == w else math.ceil(n * w / o))
        for k in ("x10", "y10", "e", "src", "K", "Xt", "Yt"):
            assert L[k] % 256 == 0
    for bad in [(-1, 10, 8, 5), (65536, 10, 8, 5), (1, -1, 8, 5), (1, 10, 0, 5), (1, 10, 8, 0)]:
        assert lib.swc_stoi_workspace_bytes(*bad) == -1
        with pytest.raises(_lib.SwcError):
            ops.stoi_workspace_bytes(*bad)


@pytest.mark.parametrize("fs", [r for r in RATES if r != 10000])
def test_filter_design_against_scipy(fs):
    from scipy.signal import resample_poly
    from simwhisper_codec_amd import metrics
    x = np.random.default_rng(fs).standard_normal(2 * fs // 5 + 13)
    h, p, q = stoi_ref.resample_filter(fs)
    want = resample_poly(x, p, q, window=h)
    got = stoi_ref.resample(x, fs)
    assert len(got) == math.ceil(len(x) * p / q) and np.abs(got - want[:len(got)]).max() < 1e-13
    # the product's own design is the same filter ...
    h2, p2, q2 = metrics.stoi_filter(fs)
    assert (p2, q2) == (p, q) and np.array_equal(h2, h)
    # ... and its table, applied the way swc_resample applies one, is that resampler up to the f32 rounding of the taps
    K, orig, new, width = metrics.stoi_taps(fs)
    L = (len(h) - 1) // 2
    assert (orig, new, width) == (q, p, math.ceil(L / p)) and K.shape == (new, 2 * width + orig) and K.dtype == torch.float32
    taps = K.shape[1]
    frames = math.ceil(len(got) / new)
    xpad = np.zeros(width + len(x) + frames * orig + taps)
    xpad[width:width + len(x)] = x
    win = np.lib.stride_tricks.sliding_window_view(xpad, taps)[::orig][:frames]      # xpad[f orig + t]
    y = (win @ K.double().numpy().T).reshape(-1)[:len(got)]
    mag = (np.abs(win) @ np.abs(K.double().numpy()).T).reshape(-1)[:len(got)]
    assert (np.abs(y - got) <= 2.0 ** -24 * mag + 1e-14).all()
    if fs == 16000:
        assert (L, len(h), orig, new, width, taps) == (290, 581, 8, 5, 58, 124)


def test_packed_tables_fit_and_44100_is_refused():
    from simwhisper_codec_amd import _lib, metrics
    for fs in RATES:
        t = metrics.stoi_table(fs, "cpu")
        K, orig, new, width = metrics.stoi_taps(fs)
        R = torch.zeros_like(K)
        for ph in range(new):
            s = int(t["start"][ph])
            R[ph, s:s + t["run"]] = t["taps"][ph]
        assert torch.equal(R, K) and (t["orig"], t["new"], t["width"]) == (orig, new, width)
        assert metrics.stoi_table(fs, "cpu") is t
    with pytest.raises(_lib.SwcError, match="44100"):
        metrics.stoi_table(44100, "cpu")


def test_default_resample_table_is_unchanged_without_a_table():
    """ops.resample_table gained `taps=`: without it, the table is what the packing of wavio.resample_taps always gave"""
    from simwhisper_codec_amd import ops, wavio
    for o, w in [(24000, 16000), (44100, 16000), (8000, 16000), (16000, 16000)]:
        t = ops.resample_table(o, w, "cpu")
        if o == w:
            K, orig, new, width = torch.ones(1, 1), 1, 1, 0
        else:
            K, orig, new, width = wavio.resample_taps(o, w)
        taps = K.shape[1]
        nz = K != 0
        pos = torch.arange(taps)
        first = torch.where(nz, pos, taps).amin(dim=1)
        last = torch.where(nz, pos, -1).amax(dim=1)
        run = max(int((last - first).max()) + 1, 1)
        start = first.clamp(max=taps - run).clamp(min=0)
        packed = torch.gather(K, 1, start[:, None] + torch.arange(run)[None, :])
        assert (t["orig"], t["new"], t["width"], t["run"], t["nnz"]) == (orig, new, width, run, int(nz.sum(1).max()))
        assert torch.equal(t["taps"], packed) and torch.equal(t["start"], start.to(torch.int32))
        # a caller's table goes through the same packing and is not kept
        mine = ops.resample_table(o, w, "cpu", taps=(K * 2, orig, new, width))
        assert torch.equal(mine["taps"], packed * 2) and ops.resample_table(o, w, "cpu") is t


def test_band_edges():
    assert stoi_ref.EDGES == [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219]
    src = open(os.path.join(ROOT, "simwhisper_codec_amd", "csrc", "swc_stoi.hip")).read()
    assert "{7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219}" in src


def test_test_signals_fill_every_band():
    for fs in RATES:
        assert stoi_ref.band_range_db(stoi_ref.harmonic(fs // 2, fs, seed=fs % 7), fs) <= stoi_ref.BAND_RANGE_DB


def test_reference_identity_and_monotone_in_snr():
    x = stoi_ref.harmonic(30000, 16000)
    r = stoi_ref.stoi(x, x, 16000)
    assert abs(r["d"] - 1.0) < 1e-12 and r["segs"] == stoi_ref.frames_at_10k(30000, 16000) - 29
    ds = []
    for snr in stoi_ref.SNRS:
        r = stoi_ref.stoi(x, stoi_ref.add_noise(x, snr), 16000)
        assert r["margin"] >= stoi_ref.MARGIN_DB and len(r["kept"]) == stoi_ref.frames_at_10k(30000, 16000) + 1
        ds.append(r["d"])
    assert all(a > b for a, b in zip(ds, ds[1:])), ds
    assert ds[0] < 1.0 and ds[-1] > 0.0


@pytest.mark.parametrize("fs", [8000, 10000, 16000])
def test_reference_boundary_lengths(fs):
    n29, n30 = stoi_ref.boundary_lengths(fs)
    assert n30 == n29 + 1
    x = stoi_ref.harmonic(n30, fs)
    y = stoi_ref.add_noise(x, 10)
    short, one = stoi_ref.stoi(x[:n29], y[:n29], fs), stoi_ref.stoi(x, y, fs)
    assert (short["segs"], short["d"]) == (0, 1e-5) and len(short["kept"]) == 30
    assert one["segs"] == 1 and 0.0 < one["d"] < 1.0 and len(one["kept"]) == 31
    assert stoi_ref.stoi(x[:0], y[:0], fs)["segs"] == 0 and stoi_ref.stoi(x[:100], y[:100], fs)["d"] == 1e-5


def test_reference_removes_all_zero_frames():
    fs = 10000
    x = stoi_ref.with_gaps(stoi_ref.harmonic(12000, fs), fs, [(0.0, 0.2), (0.6, 0.75)])
    y = stoi_ref.add_noise(x, 5)
    r = stoi_ref.stoi(x, y, fs)
    e = stoi_ref.frame_energies(x.astype(np.float64))
    silent = np.nonzero(e < -300)[0]                      # frames of exact zeros: 20 log10(EPS) = -313 dB
    assert len(silent) >= 10 and not set(silent) & set(r["kept"])
    assert r["kept"][0] > 0 and (np.diff(r["kept"]) > 1).any()          # a leading hole and an inner one
    assert r["margin"] >= stoi_ref.MARGIN_DB and r["segs"] == len(r["kept"]) - 1 - 29
    # the gaps change the score: the frames are taken out of both signals, not only skipped in the sum
    assert r["d"] != stoi_ref.stoi(stoi_ref.harmonic(12000, fs), y, fs)["d"]


def test_python_surface_refuses_what_it_cannot_do():
    from simwhisper_codec_amd import _lib, metrics
    x = torch.zeros(9000)
    with pytest.raises(_lib.SwcError, match="CPU"):
        metrics.stoi([x], [x], device="cpu")
    with pytest.raises(_lib.SwcError, match="1 reference and 2"):
        metrics.stoi([x], [x, x], device="cuda")
    with pytest.raises(_lib.SwcError):
        metrics.stoi_filter(0)


def test_tool_parser_and_pairing(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_stoi
    a = vars(evaluate_stoi.build_parser().parse_args(["--original_dir", "A", "--synthesized_dir", "B"]))
    assert a["sample_rate"] == 16000 and a["batch_size"] >= 1 and a["verbose"] is False
    for d in ("o", "s"):
        os.makedirs(tmp_path / d)
        for name in ("b.wav", "a.wav", "c.txt"):
            open(tmp_path / d / name, "wb").write(b"")
    pairs = evaluate_stoi.pair_files(str(tmp_path / "o"), str(tmp_path / "s"))
    assert [(os.path.basename(o), os.path.basename(s)) for o, s in pairs] == [("a.wav", "a.wav"), ("b.wav", "b.wav")]
    mean, skipped = evaluate_stoi.summarise(["a", "b", "c"], [0.5, 1e-5, 0.7006], [3, 0, 1])
    assert mean == pytest.approx(0.6003, abs=1e-12) and skipped == ["b"]
    assert evaluate_stoi.summarise(["a"], [1e-5], [0]) == (None, ["a"])
