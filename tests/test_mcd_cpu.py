"""swc_cepstra and swc_dtw (mel-cepstral distortion), the parts that need no GPU: the C-ABI of include/swc_mcd.h (declarations ==
bindings == exports, a table apart from the other nine; every argument check before any launch; the workspace arithmetic against
its documented formula), properties of the numpy restatement (tests/dtw_ref.py): the band always reaches the end, the tie
rule, repeated frames, the diagonal, scale invariance, the mean on a case worked by hand; the float64 cepstra (tests/mcd_ref.py)
on signals whose answer is known; the refusals of the Python surface and the flags of the tool."""
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

import dtw_ref as ref  # noqa: E402
import mcd_ref  # noqa: E402


# ---- ABI and arguments ----

def _header(name="swc_mcd.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


NAMES = {"swc_cepstra", "swc_cepstra_workspace_bytes", "swc_dtw", "swc_dtw_workspace_bytes"}


def test_mcd_header_declarations_are_bound():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    declared = _declared("swc_mcd.h")
    assert declared == NAMES == set(_lib.MCD_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)                       # exported by the library
        argtypes, restype = _lib.MCD_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    seen = set()
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        assert len(m.group(2).split(",")) == len(_lib.MCD_SIGNATURES[m.group(1)][0]), m.group(1)
        seen.add(m.group(1))
    assert seen == declared
    assert [len(_lib.MCD_SIGNATURES[n][0]) for n in sorted(NAMES)] == [20, 4, 19, 4]


def test_mcd_table_is_apart_from_the_other_nine():
    from simwhisper_codec_amd import _lib
    mine = set(_lib.MCD_SIGNATURES)
    assert not mine & set(_lib.exported_symbols())
    for other in (_lib.SIGNATURES, _lib.PLAIN, _lib.AUDIO_SIGNATURES, _lib.CODES_SIGNATURES, _lib.METRICS_SIGNATURES,
                  _lib.QUALITY_SIGNATURES, _lib.FLAC_SIGNATURES, _lib.FLAC_IO_SIGNATURES, _lib.FLAC_ENC_SIGNATURES,
                  _lib.SPECTRAL_SIGNATURES, _lib.PITCH_SIGNATURES, _lib.ALIGN_SIGNATURES):
        assert not mine & set(other)
    for h in ("swc.h", "swc_audio.h", "swc_codes.h", "swc_metrics.h", "swc_quality.h", "swc_flac.h", "swc_flac_enc.h", "swc_spectral.h",
              "swc_pitch.h", "swc_align.h"):
        assert not mine & _declared(h)
        assert "swc_dtw" not in _header(h) and "swc_cepstra" not in _header(h)


def test_constants_agree_with_the_header_and_the_reference():
    from simwhisper_codec_amd import _lib, metrics, ops
    hdr = _header()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert (val("SWC_DTW_WARP"), val("SWC_DTW_DIAGONAL")) == (_lib.DTW_WARP, _lib.DTW_DIAGONAL) == (ref.WARP, ref.DIAGONAL)
    assert ops.DTW_MODES == ref.MODES
    assert val("SWC_DTW_MAX_FRAMES") == _lib.DTW_MAX_FRAMES == ref.MAX_FRAMES == metrics.MAX_FRAMES == 8192
    assert val("SWC_DTW_MAX_D") == _lib.DTW_MAX_D == ref.MAX_D == 32 and val("SWC_CEPSTRA_MAX_K") == _lib.CEPSTRA_MAX_K == 32
    assert val("SWC_DTW_QBITS") == _lib.DTW_QBITS == ref.QBITS == 13 and val("SWC_DTW_INFO") == _lib.DTW_INFO == 4
    assert val("SWC_DTW_STRIP") == _lib.DTW_STRIP == 256
    assert "SWC_CEPSTRA_CLAMP 1e-5f" in hdr and mcd_ref.CLAMP == 1e-5
    # the bounds the header states
    assert 2 * ref.QMAX <= 32767 and 8 * (2 * ref.QMAX) ** 2 < 2 ** 31 and ref.MAX_D * (2 * ref.QMAX) ** 2 < 2 ** 33
    assert ref.D_MAX < 2 ** 21 and ref.D_MAX * (2 * ref.MAX_FRAMES - 1) < 2 ** 35 and 2 * ref.MAX_FRAMES - 1 < 2 ** ref.NBITS
    assert int(ref.INF) > (2 ** 35 << ref.NBITS)
    assert "Bits" in hdr and "depend on its Tx D and Ty D features, r and the mode only" in hdr
    assert metrics.MCD_DB == mcd_ref.MCD_DB == 10.0 * math.sqrt(2.0) / math.log(10.0)


def test_build_sees_the_new_object_and_a_touched_header(monkeypatch):
    from simwhisper_codec_amd import build
    build.build_library()
    assert not build._stale()
    assert "swc_mcd.hip" in build.SOURCES
    hdr = os.path.join(ROOT, "include", "swc_mcd.h")
    real = os.path.getmtime
    newer = real(build.LIB_PATH) + 10
    monkeypatch.setattr(os.path, "getmtime", lambda p: newer if os.path.abspath(p) == hdr else real(p))
    assert build._stale()


def _aligned_buffer():
    raw = (C.c_char * 1024)()
    base = C.addressof(raw)
    return raw, C.c_void_p((base + 255) & ~255)


def test_dtw_arg_checks_without_gpu():
    """every check happens before any launch: host pointers that are never dereferenced stand in for device memory"""
    from simwhisper_codec_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_buffer()

    def call(xf=p, yf=p, tx=p, ty=p, Tx=300, Ty=200, D=13, ldf=16, band=0, mode=0, total=p, info=p, mean=p, path=p, ldp=None, ws=p,
             ws_bytes=1 << 50, B=2):
        ldp = max(Tx + Ty - 1, 0) if ldp is None else ldp
        return lib.swc_dtw(xf, yf, tx, ty, Tx, Ty, D, ldf, band, mode, total, info, mean, path, ldp, ws, ws_bytes, B, None)

    need = lib.swc_dtw_workspace_bytes(2, 300, 200, 1)
    assert need > lib.swc_dtw_workspace_bytes(2, 300, 200, 0) > 0
    odd = C.c_void_p(p.value + 4)
    for kw, word in [(dict(xf=None), b"null"), (dict(yf=None), b"null"), (dict(tx=None), b"null"), (dict(ty=None), b"null"),
                     (dict(ws=None), b"null"), (dict(total=None, info=None, mean=None, path=None), b"no output"),
                     (dict(B=65536), b"B="), (dict(B=-1), b"B="),
                     (dict(Tx=8193), b"out of range"), (dict(Ty=8193), b"out of range"), (dict(Tx=-1), b"out of range"),
                     (dict(Ty=-1), b"out of range"),
                     (dict(D=0), b"features"), (dict(D=33, ldf=40), b"features"), (dict(D=13, ldf=12), b"ldf"),
                     (dict(band=-1), b"band"), (dict(mode=2), b"mode"), (dict(mode=-1), b"mode"),
                     (dict(ldp=498), b"ldp"), (dict(ldp=0), b"ldp"),
                     (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"),
                     (dict(path=None, ws_bytes=lib.swc_dtw_workspace_bytes(2, 300, 200, 0) - 1), b"workspace"),
                     (dict(ws=odd), b"aligned")]:
        assert call(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    # nothing to do: no launch, no device needed.  ldp does not matter without path; every subset of outputs but the empty one
    assert call(B=0) == 0 and call(B=0, ws_bytes=lib.swc_dtw_workspace_bytes(0, 300, 200, 1)) == 0
    assert call(B=0, path=None, ldp=0) == 0 and call(B=0, path=None, ws_bytes=lib.swc_dtw_workspace_bytes(0, 300, 200, 0)) == 0
    for total in (p, None):
        for info in (p, None):
            for mean in (p, None):
                for path in (p, None):
                    if total or info or mean or path:
                        assert call(B=0, total=total, info=info, mean=mean, path=path) == 0
    assert call(B=0, Tx=8192, Ty=8192, D=32, ldf=32, band=1 << 30, mode=1) == 0 and call(B=0, Tx=0, Ty=0, D=1, ldf=1, ldp=0) == 0
    del keep


def test_cepstra_arg_checks_without_gpu():
    from simwhisper_codec_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_buffer()

    def call(rows=p, n_in=p, max_n=16000, W=512, H=160, M=80, first=p, count=p, off=p, w=p, w_len=1000, dct=p, K=13, cep=p, ldf=16,
             frames=p, ws=None, ws_bytes=0, R=2):
        return lib.swc_cepstra(rows, n_in, max_n, W, H, M, first, count, off, w, w_len, dct, K, cep, ldf, frames, ws, ws_bytes, R, None)

    odd = C.c_void_p(p.value + 4)
    for kw, word in [(dict(rows=None), b"null"), (dict(n_in=None), b"null"), (dict(first=None), b"null"), (dict(count=None), b"null"),
                     (dict(off=None), b"null"), (dict(w=None), b"null"), (dict(dct=None), b"null"), (dict(cep=None), b"null"),
                     (dict(frames=None), b"null"),
                     (dict(R=65536), b"R="), (dict(R=-1), b"R="), (dict(max_n=-1), b"max_n_in"),
                     (dict(W=500), b"window"), (dict(W=16), b"window"), (dict(W=4096), b"window"), (dict(W=0), b"window"),
                     (dict(H=0), b"hop"), (dict(H=513), b"hop"), (dict(M=0), b"n_mels"), (dict(M=258), b"n_mels"),
                     (dict(w_len=-1), b"fb_w_len"), (dict(K=0), b"K="), (dict(K=33, ldf=40), b"K="), (dict(ldf=12), b"ldf"),
                     (dict(max_n=1 << 40, H=1), b"frames"), (dict(ws_bytes=-1), b"workspace"), (dict(ws=odd, ws_bytes=8), b"aligned")]:
        assert call(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    assert call(R=0) == 0 and call(R=0, ws=p, ws_bytes=256) == 0 and call(R=0, W=32, H=32, M=17, K=32, ldf=32) == 0
    assert call(R=0, W=2048, H=1, M=1025, K=1, ldf=1, max_n=48000) == 0
    del keep


def test_workspace_bytes_against_the_documented_formula():
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    up = lambda v: (v + 255) & ~255
    for B, Tx, Ty in [(1, 0, 0), (1, 1, 1), (3, 300, 200), (32, 1001, 1001), (33, 529, 17), (0, 500, 500), (65535, 8192, 8192), (5, 255, 257)]:
        base = up(4 * B) + up(8 * B) + up(64 * B * Tx) + up(64 * B * Ty) + up(2 * 8 * B * Ty)
        for with_path in (0, 1):
            want = base + (up(4 * B * Tx * ((Ty + 15) // 16)) if with_path else 0)
            assert lib.swc_dtw_workspace_bytes(B, Tx, Ty, with_path) == want, (B, Tx, Ty, with_path)
            assert ops.dtw_workspace_bytes(B, Tx, Ty, with_path) == want and want % 256 == 0
    for bad in [(-1, 10, 10, 0), (65536, 10, 10, 0), (1, -1, 10, 0), (1, 10, -1, 1), (1, 8193, 10, 0), (1, 10, 8193, 1)]:
        assert lib.swc_dtw_workspace_bytes(*bad) == -1, bad
        with pytest.raises(_lib.SwcError):
            ops.dtw_workspace_bytes(*bad)
    for ok in [(0, 0, 32, 1), (1, 16000, 512, 160), (65535, 1 << 30, 2048, 2048), (3, 48000, 2048, 1)]:
        assert lib.swc_cepstra_workspace_bytes(*ok) == 0 == ops.cepstra_workspace_bytes(*ok)
    for bad in [(-1, 10, 512, 160), (65536, 10, 512, 160), (1, -1, 512, 160), (1, 10, 500, 160), (1, 10, 16, 8), (1, 10, 512, 0), (1, 10, 512, 513),
                (1, 1 << 40, 512, 1)]:
        assert lib.swc_cepstra_workspace_bytes(*bad) == -1, bad
        with pytest.raises(_lib.SwcError):
            ops.cepstra_workspace_bytes(*bad)


# ---- the DTW reference on itself ----

def test_the_band_always_reaches_the_end():
    """for every Tx, Ty <= 40 and r = 1, 2, 3: both corners are allowed and the end is reachable through allowed cells"""
    for Tx in range(1, 41):
        for Ty in range(1, 41):
            d = np.zeros((Tx, Ty), np.int64)
            for r in (1, 2, 3):
                ok = ref.allowed(Tx, Ty, r)
                assert ok[0, 0] and ok[-1, -1]
                K, _ = ref.recurrence(d, ok)
                assert K[-1, -1] < ref.INF, (Tx, Ty, r)
                assert int(K[-1, -1]) == max(Tx, Ty), (Tx, Ty, r)            # all costs 0: the key is the shortest path's N
    assert ref.allowed(7, 9, 0).all()


def test_the_tie_rule_on_all_zero_features():
    """Tx = 3, Ty = 5, every cost 0: every path has C = 0, the shortest have N = 5, and among those the rule (the diagonal first,
    then (i-1, j), then (i, j-1), decided cell by cell from the start) leaves exactly one"""
    r = ref.dtw(np.zeros((3, 4), np.float32), np.zeros((5, 4), np.float32))
    assert r["total"] == 0 and r["info"].tolist() == [5, 3, 5, 0] and r["mean"] == 0.0
    assert r["path"].tolist() == [[0, 0], [0, 1], [0, 2], [1, 3], [2, 4]]
    r = ref.dtw(np.zeros((5, 4), np.float32), np.zeros((3, 4), np.float32))
    assert r["info"].tolist() == [5, 5, 3, 0] and r["path"].tolist() == [[0, 0], [1, 0], [2, 0], [3, 1], [4, 2]]
    r = ref.dtw(np.zeros((1, 1), np.float32), np.zeros((4, 1), np.float32))
    assert r["info"].tolist() == [4, 1, 4, 0] and r["path"].tolist() == [[0, 0], [0, 1], [0, 2], [0, 3]]


def test_equal_cost_with_different_step_counts_takes_the_shorter_path():
    """x = 0, 0, 1 against y = 0, 1: C = 0 is reached at the end both through (1, 0) (three steps) and along (0, 0), (1, 0),
    (2, 1) ... and through the diagonal first: the key orders by C and then by N"""
    x = np.array([[0.0], [0.0], [1.0]], np.float32)
    y = np.array([[0.0], [1.0]], np.float32)
    r = ref.dtw(x, y)
    assert r["total"] == 0 and r["info"][0] == 3 and r["path"].tolist() == [[0, 0], [1, 0], [2, 1]]
    # a detour of equal cost is longer and loses: cost matrix of zeros on two routes
    d = np.array([[0, 0, 9], [9, 0, 0], [9, 9, 0]], np.int64)
    K, choice = ref.recurrence(d, np.ones((3, 3), bool))
    assert int(K[-1, -1]) == 3 and ref.backtrack(choice, 3).tolist() == [[0, 0], [1, 1], [2, 2]]      # not the five-step staircase
    d = np.array([[0, 0, 0], [9, 9, 0], [9, 9, 0]], np.int64)
    K, choice = ref.recurrence(d, np.ones((3, 3), bool))
    assert int(K[-1, -1]) == 4 and ref.backtrack(choice, 4).tolist() == [[0, 0], [0, 1], [1, 2], [2, 2]]


def test_repeated_frames_cost_nothing():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((40, 13)).astype(np.float32)
    reps = rng.integers(1, 4, 40)
    y = np.repeat(x, reps, axis=0)
    r = ref.dtw(x, y)
    want = np.stack([np.repeat(np.arange(40), reps), np.arange(len(y))], 1)
    assert r["total"] == 0 and r["mean"] == 0.0 and r["info"].tolist()[:3] == [len(y), 40, len(y)]
    assert np.array_equal(r["path"], want)
    assert ref.dtw(x, y, mode="diagonal")["total"] > 0
    for band in (1, 2):
        assert ref.dtw(x, y, band=band)["total"] >= 0
    wide = ref.dtw(x, y, band=40)
    assert wide["total"] == 0 and np.array_equal(wide["path"], want)


def test_diagonal_equals_warp_on_identical_inputs_and_is_cut_to_the_shorter_side():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((50, 24)).astype(np.float32)
    a, b = ref.dtw(x, x), ref.dtw(x, x, mode="diagonal")
    assert a["total"] == b["total"] == 0 and a["info"].tolist() == b["info"].tolist() == [50, 50, 50, a["info"][3]]
    assert np.array_equal(a["path"], b["path"])
    y = rng.standard_normal((30, 24)).astype(np.float32)
    d = ref.dtw(x, y, mode="diagonal", band=5)
    e = int(d["info"][3])
    qx, qy = ref.quantise(x, e), ref.quantise(y, e)
    assert d["info"].tolist() == [30, 50, 30, e] and d["total"] == sum(int(ref.root256(((qx[t] - qy[t]) ** 2).sum())) for t in range(30))
    assert ref.dtw(x, y)["total"] <= ref.dtw(x, np.concatenate([y, y[-1:].repeat(20, 0)]), mode="diagonal")["total"]


def test_scale_invariance_and_one_scale_for_both_sides():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((33, 13)).astype(np.float32)
    y = (0.01 * rng.standard_normal((41, 13))).astype(np.float32)          # a far quieter side: it shares x's scale
    base = ref.dtw(x, y, band=3)
    for k in (-20, -3, 1, 9):
        r = ref.dtw(np.ldexp(x, k), np.ldexp(y, k), band=3)
        assert r["total"] == base["total"] and np.array_equal(r["path"], base["path"])
        assert r["info"].tolist() == (base["info"] + np.array([0, 0, 0, k])).tolist()
        assert r["mean"] == np.ldexp(base["mean"], k)
    e = int(base["info"][3])
    assert np.abs(ref.quantise(x, e)).max() > 4095 and np.abs(ref.quantise(y, e)).max() < 600
    # the quantised distance tracks the float64 one
    p = base["path"]
    exact = np.sqrt(((x[p[:, 0]].astype(np.float64) - y[p[:, 1]]) ** 2).sum(1)).mean()
    assert abs(float(base["mean"]) - exact) < 13 ** 0.5 * 2.0 ** (e - 13)


def test_the_mean_on_a_case_worked_by_hand():
    """x = (3, 0), (0, 0); y = (0, 4), (0, 0): peak 4 = 0.5 2^3, e = 3, q = v 2^10: 3072, 4096.  d[0][0] = 16 * 5120, d[0][1] = 16 *
    3072, d[1][0] = 16 * 4096, d[1][1] = 0.  The path is (0, 0), (1, 1): total = 81920, N = 2, mean = 81920 / 32 / 1024 = 2.5"""
    x = np.array([[3.0, 0.0], [0.0, 0.0]], np.float32)
    y = np.array([[0.0, 4.0], [0.0, 0.0]], np.float32)
    r = ref.dtw(x, y)
    assert r["total"] == 81920 and r["info"].tolist() == [2, 2, 2, 3] and r["path"].tolist() == [[0, 0], [1, 1]]
    assert r["mean"] == np.float32(2.5) and r["mean"].dtype == np.float32
    assert ref.local_cost(ref.quantise(x, 3), ref.quantise(y, 3)).tolist() == [[81920, 49152], [65536, 0]]
    # the exact root: 256 s one below and at a square
    assert ref.root256(np.array([0, 1, 2, 3, 2 ** 33 - 1], np.int64)).tolist() == [0, 16, 22, 27, math.isqrt(256 * (2 ** 33 - 1))]
    big = np.array([(1 << 20) ** 2 // 256 * 256], np.int64)
    assert int(ref.root256(big // 256)[0]) == math.isqrt(int(big[0]))


def test_empty_and_not_defined_pairs():
    z = np.zeros((0, 3), np.float32)
    x = np.ones((4, 3), np.float32)
    for a, b in ((z, x), (x, z), (z, z)):
        r = ref.dtw(a, b)
        assert r["total"] == 0 and r["info"].tolist() == [0, 0, 0, 0] and np.isnan(r["mean"]) and len(r["path"]) == 0
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy(); y[2, 1] = bad
        for a, b in ((x, y), (y, x)):
            for mode in ("warp", "diagonal"):
                r = ref.dtw(a, b, mode=mode)
                assert r["info"].tolist() == [0, 0, 0, 0] and np.isnan(r["mean"]) and r["total"] == 0
    assert ref.quantise(np.array([1.0, -1.0, 0.99999994], np.float32), 1).tolist() == [4096, -4096, 4096]
    assert ref.quantise(np.array([1.9999999, -1.9999999], np.float32), 1).tolist() == [8191, -8191]       # rint gives 8192: clamped
    assert ref.peak_exp(ref.peak_of(x, 2 * x)) == 2 and ref.peak_exp(0) == 0


# ---- the cepstral reference ----

def _tables(sr):
    from simwhisper_codec_amd import metrics
    W, H = metrics.mcd_params(sr)
    first, count, off, w = metrics.pack_filterbanks([metrics.mel_filterbank(sr, W, metrics.MCD_MELS)])
    dct = metrics.dct_matrix(metrics.MCD_COEFFS, metrics.MCD_MELS).astype(np.float32)
    return W, H, mcd_ref.dense_bank(first, count, off, w, W // 2 + 1), dct


def test_default_parameters_per_rate():
    from simwhisper_codec_amd import metrics
    want = {8000: (256, 80), 10000: (256, 100), 16000: (512, 160), 24000: (1024, 240), 32000: (1024, 320), 48000: (2048, 480)}
    assert {sr: metrics.mcd_params(sr) for sr in metrics.RATES} == want
    for sr, (W, H) in want.items():
        assert W >= 0.025 * sr > W // 2 and H == round(0.010 * sr)
    with pytest.raises(metrics.SwcError):
        metrics.mcd_params(96000)
    d = metrics.dct_matrix(80, 80, first=0)
    assert np.abs(d @ d.T - np.eye(80)).max() < 1e-13                         # orthonormal
    assert np.array_equal(metrics.dct_matrix(13, 80), d[1:14]) and np.abs(d[1:14].sum(1)).max() < 1e-13   # c0 is left out: a level shift vanishes
    assert metrics.mcd_band(16000, None) == 0 and metrics.mcd_band(16000, 100) == 10 and metrics.mcd_band(16000, 10.0) == 1
    for bad in (9.9, 0, -5, float("nan"), float("inf"), "wide"):
        with pytest.raises(metrics.SwcError, match="band_ms"):
            metrics.mcd_band(16000, bad)


def test_cepstra_reference_frames_level_and_silence():
    W, H, bank, dct = _tables(16000)
    rng = np.random.default_rng(6)
    x = (0.1 * rng.standard_normal(4000)).astype(np.float32)
    c = mcd_ref.cepstra(x, W, H, bank, dct)
    assert c.shape == (1 + 4000 // H, 13)
    for n in (0, 1, H - 1, H, H + 1, W // 2 - 1, W // 2 + 1):
        assert mcd_ref.cepstra(x[:n], W, H, bank, dct).shape == ((1 + n // H) if n else 0, 13)
    # a level change moves c0 only, which is left out: the cepstra of 2 x equal those of x where nothing sits at the clamp floor
    assert np.abs(mcd_ref.cepstra(2 * x, W, H, bank, dct) - c)[2:-2].max() < 1e-9
    # silence: every band at the floor, every coefficient ln(1e-5) times a DCT row's sum (zero up to the table's f32 rounding)
    s = mcd_ref.cepstra(np.zeros(1000, np.float32), W, H, bank, dct)
    assert np.abs(s - math.log(1e-5) * dct.astype(np.float64).sum(1)[None, :]).max() < 1e-12 and np.abs(s).max() < 1e-4
    # frame t is centred on sample t H: a click at t H peaks in frame t
    click = np.zeros(3000, np.float32); click[5 * H] = 1.0
    energy = np.abs(np.fft.rfft(mcd_ref.frames(click, W, H), axis=1)).sum(1)
    assert int(energy.argmax()) == 5
    assert np.isnan(mcd_ref.cepstra(np.array([np.nan] * 10, np.float32), W, H, bank, dct)).all()
    path = np.stack([np.arange(len(c)), np.arange(len(c))], 1)
    assert mcd_ref.mcd_float64(c, c, path) == 0.0


# ---- the Python surface and the tool ----

def test_python_surface_refuses_what_it_cannot_do():
    from simwhisper_codec_amd import _lib, metrics
    x = torch.zeros(9000)
    with pytest.raises(_lib.SwcError, match="CPU"):
        metrics.mcd([x], [x], device="cpu")
    with pytest.raises(_lib.SwcError, match="CPU"):
        metrics.mcd([x], [x], align="waveform", device="cpu")
    with pytest.raises(_lib.SwcError, match="align="):
        metrics.mcd([x], [x], align="pesq")
    with pytest.raises(_lib.SwcError, match="max_lag_ms"):
        metrics.mcd([x], [x], align="envelope", max_lag_ms=-1.0)
    for bad in (5.0, 0.0, float("nan"), "wide"):
        with pytest.raises(_lib.SwcError, match="band_ms"):
            metrics.mcd([x], [x], band_ms=bad)
    with pytest.raises(_lib.SwcError, match="sample_rate"):
        metrics.mcd([x], [x], sample_rate=96000)
    # a row of more than MAX_FRAMES frames is refused by name before anything touches a GPU (there is none here)
    long = torch.zeros(160 * 8192)
    for pair in (([long], [x]), ([x], [long])):
        with pytest.raises(_lib.SwcError, match="MAX_FRAMES"):
            metrics.mcd(*pair)
        with pytest.raises(_lib.SwcError, match="MAX_FRAMES"):
            metrics.mcd(*pair, dtw=False)
    with pytest.raises(_lib.SwcError, match="CPU"):
        metrics.dtw([torch.zeros(4, 3)], [torch.zeros(5, 3)], device="cpu")
    from simwhisper_codec_amd.codec import AudioCodec
    assert callable(AudioCodec.mcd)


def test_tool_parses_its_flags():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_mcd
    base = ["--original_dir", "A", "--synthesized_dir", "B"]
    a = vars(evaluate_mcd.build_parser().parse_args(base))
    assert a["align"] == "none" and a["max_lag_ms"] == 50.0 and a["no_dtw"] is False and a["band_ms"] is None and a["batch_size"] == 32
    a = vars(evaluate_mcd.build_parser().parse_args(base + ["--align", "envelope", "--max_lag_ms", "12.5", "--no_dtw", "--band_ms", "200"]))
    assert a["align"] == "envelope" and a["max_lag_ms"] == 12.5 and a["no_dtw"] is True and a["band_ms"] == 200.0
    with pytest.raises(SystemExit):
        evaluate_mcd.build_parser().parse_args(base + ["--align", "pesq"])
    nan = float("nan")
    assert evaluate_mcd.summarise(["a", "b", "c"], [1.0, nan, 3.0]) == (2.0, ["b"])
    assert evaluate_mcd.summarise(["a"], [nan]) == (None, ["a"])
    assert "bench_mcd.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
