"""swc_cmvn and swc_subdtw (the score after WARP-Q), the parts that need no GPU: the C-ABI of include/swc_subdtw.h (declarations
== bindings == exports, a table apart from the others; every argument check before any launch; the workspace arithmetic against
its documented formula), the numpy restatement (tests/subdtw_ref.py) against an independent enumeration of every step sequence
and on planted truths, the summation order of the normalisation, the mel bank's new upper edge (and its unchanged default), the
front end's tables, the refusals of the Python surface and the flags of the tool."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import subdtw_ref as ref  # noqa: E402

STEP_SETS = (((1, 1), (1, 0), (0, 1)), ((1, 0), (0, 3), (1, 3)), ((1, 1), (3, 2), (1, 3)), ((1, 1), (2, 1), (1, 2)), ((1, 1),))
NAMES = {"swc_cmvn", "swc_subdtw", "swc_subdtw_workspace_bytes"}


# ---- ABI and arguments ----

def _header(name="swc_subdtw.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


def test_subdtw_header_declarations_are_bound():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    declared = _declared("swc_subdtw.h")
    assert declared == NAMES == set(_lib.SUBDTW_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)                       # exported by the library
        argtypes, restype = _lib.SUBDTW_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    seen = set()
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        assert len(m.group(2).split(",")) == len(_lib.SUBDTW_SIGNATURES[m.group(1)][0]), m.group(1)
        seen.add(m.group(1))
    assert seen == declared
    assert [len(_lib.SUBDTW_SIGNATURES[n][0]) for n in sorted(NAMES)] == [9, 22, 5]


def test_subdtw_table_is_apart_from_the_others():
    from simwhisper_codec_amd import _lib
    mine = set(_lib.SUBDTW_SIGNATURES)
    assert not mine & set(_lib.exported_symbols())
    others = [v for k, v in vars(_lib).items() if (k.endswith("SIGNATURES") or k == "PLAIN") and k != "SUBDTW_SIGNATURES"]
    assert len(others) >= 16
    for other in others:
        assert not mine & set(other)
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "swc_subdtw.h":
            assert not mine & _declared(h)
            assert "swc_subdtw" not in _header(h) and "swc_cmvn" not in _header(h)


def test_constants_agree_with_the_header_and_the_reference():
    from simwhisper_codec_amd import _lib, metrics, ops
    hdr = _header()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert val("SWC_SUBDTW_MAX_PATCH") == _lib.SUBDTW_MAX_PATCH == ref.MAX_PATCH == metrics.MAX_PATCH == 256
    assert val("SWC_SUBDTW_MAX_STEPS") == _lib.SUBDTW_MAX_STEPS == ref.MAX_STEPS == 4
    assert val("SWC_SUBDTW_MAX_STRIDE") == _lib.SUBDTW_MAX_STRIDE == ref.MAX_STRIDE == 3
    assert val("SWC_SUBDTW_MAX_FRAMES") == _lib.SUBDTW_MAX_FRAMES == _lib.DTW_MAX_FRAMES == ref.MAX_FRAMES == 8192
    assert val("SWC_SUBDTW_MAX_D") == _lib.SUBDTW_MAX_D == _lib.DTW_MAX_D == ref.MAX_D == 32
    assert val("SWC_SUBDTW_INFO") == _lib.SUBDTW_INFO == 4 and val("SWC_CMVN_BLOCK") == _lib.CMVN_BLOCK == ref.CMVN_BLOCK == 256
    assert [val(f"SWC_SUBDTW_ST_{n}") for n in ("OK", "UNREACHABLE", "UNDEFINED", "QUERY")] == [0, 1, 2, 3]
    assert (_lib.SUBDTW_ST_OK, _lib.SUBDTW_ST_UNREACHABLE, _lib.SUBDTW_ST_UNDEFINED, _lib.SUBDTW_ST_QUERY) == (0, 1, 2, 3)
    assert (ref.ST_OK, ref.ST_UNREACHABLE, ref.ST_UNDEFINED, ref.ST_QUERY) == (0, 1, 2, 3)
    assert ref.QBITS == _lib.DTW_QBITS == 13
    # the bound the header shows: N < 2^14 and C < 2^35, so the key of swc_dtw is kept
    n_max = ref.MAX_PATCH + ref.MAX_FRAMES - 1
    assert n_max < 2 ** ref.NBITS and ref.D_MAX * n_max < 2 ** 35 and ref.D_MAX ** 2 >= 256 * ref.MAX_D * (2 * ref.QMAX) ** 2
    assert "91 * 16382 * 8447 < 2^35" in hdr and int(ref.INF) > (2 ** 35 << ref.NBITS)
    assert "depend on its Tq D and Ty D features, Lp, Sp and the step set only" in hdr
    assert ops.SUBDTW_SYMMETRIC == metrics.SYMMETRIC_STEPS == ref.SYMMETRIC and metrics.WARPQ_STEPS == ref.WARPQ == STEP_SETS[2] and metrics.ASYMMETRIC_STEPS == ref.ASYMMETRIC == STEP_SETS[1]
    # "after WARP-Q", never "is WARP-Q"
    for doc in (hdr, open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "DESIGN.md")).read()):
        assert "after WARP-Q" in doc and "is WARP-Q" not in doc


def test_build_sees_the_new_object_and_a_touched_header(monkeypatch):
    from simwhisper_codec_amd import build
    build.build_library()
    assert not build._stale()
    assert "swc_subdtw.hip" in build.SOURCES and build.EXTRA_FLAGS["swc_subdtw.hip"] == ["-ffp-contract=off"]
    hdr = os.path.join(ROOT, "include", "swc_subdtw.h")
    real = os.path.getmtime
    newer = real(build.LIB_PATH) + 10
    monkeypatch.setattr(os.path, "getmtime", lambda p: newer if os.path.abspath(p) == hdr else real(p))
    assert build._stale()


def _aligned_buffer():
    raw = (C.c_char * 1024)()
    base = C.addressof(raw)
    return raw, C.c_void_p((base + 255) & ~255)


def _steps(st):
    flat = [v for s in st for v in s]
    return (C.c_int32 * max(len(flat), 1))(*flat), len(st)


def test_subdtw_arg_checks_without_gpu():
    """every check happens before any launch: host pointers that are never dereferenced stand in for device memory"""
    from simwhisper_codec_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_buffer()

    def call(qf=p, yf=p, tq=p, ty=p, Tq=300, Ty=200, D=13, ldf=16, Lp=100, Sp=50, steps=ref.WARPQ, n_steps=None, cost=p, info=p,
             ldp=None, score=p, patches=p, exps=p, ws=p, ws_bytes=1 << 50, B=2):
        arr, n = _steps(steps) if steps is not None else (None, 0)
        ldp = 8 if ldp is None else ldp
        return lib.swc_subdtw(qf, yf, tq, ty, Tq, Ty, D, ldf, Lp, Sp, arr, n if n_steps is None else n_steps, cost, info, ldp, score,
                              patches, exps, ws, ws_bytes, B, None)

    need = lib.swc_subdtw_workspace_bytes(2, 300, 200, 100, 50)
    assert need > 0
    odd = C.c_void_p(p.value + 4)
    five = ((1, 1), (1, 0), (0, 1), (1, 2), (2, 1))
    for kw, word in [(dict(qf=None), b"null"), (dict(yf=None), b"null"), (dict(tq=None), b"null"), (dict(ty=None), b"null"),
                     (dict(ws=None), b"null"), (dict(steps=None, n_steps=1), b"null"),
                     (dict(cost=None, info=None, score=None, patches=None, exps=None), b"no output"),
                     (dict(B=65536), b"B="), (dict(B=-1), b"B="),
                     (dict(Tq=8193), b"out of range"), (dict(Ty=8193), b"out of range"), (dict(Tq=-1), b"out of range"),
                     (dict(D=0), b"features"), (dict(D=33, ldf=40), b"features"), (dict(D=13, ldf=12), b"ldf"),
                     (dict(Lp=257), b"patch length"), (dict(Lp=-1), b"patch length"), (dict(Sp=0), b"patch step"),
                     (dict(steps=()), b"n_steps"), (dict(steps=five), b"n_steps"), (dict(n_steps=-1), b"n_steps"),
                     (dict(steps=((1, 1), (0, 0))), b"step 1 is (0, 0)"), (dict(steps=((1, 1), (1, 0), (1, 1))), b"given twice"),
                     (dict(steps=((0, 1), (0, 2))), b"no step with di >= 1"), (dict(steps=((4, 1),)), b"step 0 is (4, 1)"),
                     (dict(steps=((1, 4),)), b"step 0 is (1, 4)"), (dict(steps=((-1, 1),)), b"step 0 is (-1, 1)"),
                     (dict(ldp=4), b"ldp"), (dict(Lp=0, ldp=0), b"ldp"),
                     (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"), (dict(ws=odd), b"aligned")]:
        assert call(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    # nothing to do: no launch, no device needed.  ldp does not matter without cost and info
    assert call(B=0) == 0 and call(B=0, ws_bytes=lib.swc_subdtw_workspace_bytes(0, 300, 200, 100, 50)) == 0
    assert call(B=0, cost=None, info=None, ldp=0) == 0
    for st in STEP_SETS:
        assert call(B=0, steps=st) == 0
    for outs in itertools.product((p, None), repeat=5):
        if any(o is not None for o in outs):
            assert call(B=0, **dict(zip(("cost", "info", "score", "patches", "exps"), outs))) == 0


def test_cmvn_arg_checks_without_gpu():
    from simwhisper_codec_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_buffer()
    other = C.c_void_p(p.value + 256)

    def call(cep=p, frames=p, Tmax=100, K=13, ldf=16, out=other, ldo=16, R=2):
        return lib.swc_cmvn(cep, frames, Tmax, K, ldf, out, ldo, R, None)

    for kw, word in [(dict(cep=None), b"null"), (dict(frames=None), b"null"), (dict(out=None), b"null"), (dict(R=-1), b"R="),
                     (dict(R=65536), b"R="), (dict(Tmax=-1), b"Tmax"), (dict(Tmax=2 ** 31 - 1), b"Tmax"), (dict(K=0), b"K="),
                     (dict(K=33, ldf=40, ldo=40), b"K="), (dict(ldf=12), b"ldf"), (dict(ldo=12), b"ldo"),
                     (dict(out=p, ldo=20), b"in place")]:
        assert call(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    assert call(R=0) == 0 and call(Tmax=0) == 0 and call(R=0, out=p) == 0


def test_workspace_arithmetic_c_against_python():
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    for B, tq, ty, Lp, Sp in [(0, 0, 0, 0, 1), (1, 1, 1, 1, 1), (1, 8192, 8192, 1, 1), (3, 300, 200, 100, 50), (33, 2501, 2501, 100, 50),
                              (65535, 8192, 8192, 256, 1), (2, 99, 7, 100, 50), (2, 100, 7, 100, 50), (2, 101, 7, 100, 3),
                              (5, 256, 100, 0, 1), (5, 8192, 100, 0, 7), (7, 0, 10, 0, 1), (7, 10, 0, 5, 2)]:
        parts, total = ops.subdtw_workspace_layout(B, tq, ty, Lp, Sp)
        assert lib.swc_subdtw_workspace_bytes(B, tq, ty, Lp, Sp) == total == ops.subdtw_workspace_bytes(B, tq, ty, Lp, Sp)
        assert all(o % 256 == 0 for o, _ in parts.values()) and list(parts) == ["peaks", "qq", "yq", "cost"]
        p_max = 1 if Lp == 0 else ref.patch_count(tq, Lp, Sp)
        assert parts["cost"][1] == 8 * B * max(p_max, 1) and ops.subdtw_patches(tq, Lp, Sp) == ref.patch_count(tq, Lp, Sp)
    for bad in [(-1, 1, 1, 1, 1), (65536, 1, 1, 1, 1), (1, 8193, 1, 1, 1), (1, 1, 8193, 1, 1), (1, -1, 1, 1, 1), (1, 1, 1, 257, 1),
                (1, 1, 1, -1, 1), (1, 1, 1, 1, 0)]:
        assert lib.swc_subdtw_workspace_bytes(*bad) == -1
        with pytest.raises(_lib.SwcError):
            ops.subdtw_workspace_bytes(*bad)
    # the first and the last frame that still give P patches
    assert [ref.patch_count(t, 100, 50) for t in (0, 99, 100, 149, 150, 2501)] == [0, 0, 1, 1, 2, 49]
    assert [ref.patch_count(t, 0, 9) for t in (0, 1, 256, 257)] == [0, 1, 1, 0]


# ---- the reference against an independent enumeration, and on planted truths ----

@pytest.mark.parametrize("steps", STEP_SETS)
def test_reference_against_the_enumeration_of_every_step_sequence(steps):
    rng = np.random.default_rng(len(steps) * 7 + sum(a + 2 * b for a, b in steps))
    for L, Ty in itertools.product((1, 2, 3, 4), (1, 2, 3, 5, 7)):
        for trial in range(6):
            # small integer costs: equal keys are common, so the tie rules are what is compared
            d = rng.integers(0, 2 if trial < 3 else 50, size=(L, Ty)).astype(np.int64)
            got = ref.patch_dp(d, list(steps))
            want = ref.brute(d, list(steps))
            if want is None:
                assert got == (0, 0, 0, 0, ref.ST_UNREACHABLE), (L, Ty, d)
            else:
                key, start, end = want
                assert got == (key >> ref.NBITS, key & (2 ** ref.NBITS - 1), start, end, ref.ST_OK), (L, Ty, d, got, want)


def _features(rng, T, D):
    return rng.standard_normal((T, D)).astype(np.float32)


@pytest.mark.parametrize("steps", STEP_SETS)
def test_a_query_cut_out_of_the_reference_is_found_with_cost_zero(steps):
    rng = np.random.default_rng(5)
    y = _features(rng, 60, 9)
    for a, L in [(0, 1), (0, 7), (17, 20), (40, 20), (59, 1)]:
        stride = [(di, dj) for di, dj in steps if di == 1]
        if not any(dj == 1 for _, dj in stride):
            continue                                   # this set has no step that walks the diagonal frame by frame
        r = ref.subdtw(y[a:a + L], y, 0, 1, steps)
        assert r["patches"] == (1, 1) and r["cost"][0] == 0 and r["score"] == 0.0
        assert r["info"][0].tolist() == [L, a, a + L - 1, ref.ST_OK]


def test_every_second_frame_repeated_costs_nothing_under_the_symmetric_set():
    rng = np.random.default_rng(6)
    y = _features(rng, 50, 13)
    q = np.repeat(y[10:30], [2 if t % 2 else 1 for t in range(20)], axis=0)
    r = ref.subdtw(q, y, 0, 1, ref.SYMMETRIC)
    assert r["cost"][0] == 0 and r["info"][0].tolist() == [len(q), 10, 29, ref.ST_OK] and r["score"] == 0.0
    # the other way round (frames dropped from the query) as well: (0, 1) skips nothing, it walks
    r = ref.subdtw(y[10:30:2], y, 0, 1, ref.SYMMETRIC)
    assert r["info"][0, 3] == ref.ST_OK and r["cost"][0] > 0


def test_reference_statuses_patches_and_median():
    rng = np.random.default_rng(7)
    q, y = _features(rng, 23, 8), _features(rng, 40, 8)
    r = ref.subdtw(q, y, 5, 3, ref.SYMMETRIC)
    assert r["patches"] == (7, 7) and (r["info"][:, 3] == 0).all()
    s = sorted(int(c) for c in r["cost"])
    assert r["score"] == np.ldexp(np.float64(s[3]), r["e"] - 17)
    r = ref.subdtw(q[:20], y, 5, 3, ref.SYMMETRIC)                      # an even count: the mean of the two middle ones
    s = sorted(int(c) for c in r["cost"])
    assert r["patches"] == (6, 6) and r["score"] == np.ldexp(np.float64(s[2] + s[3]) / 2, r["e"] - 17)
    assert ref.subdtw(q[:4], y, 5, 3, ref.SYMMETRIC)["patches"] == (0, 0) and np.isnan(ref.subdtw(q[:4], y, 5, 3, ref.SYMMETRIC)["score"])
    # Ty too short for the steps: (1, 3) alone needs 3 columns per row
    r = ref.subdtw(q[:5], y[:12], 5, 1, ((1, 3),))
    assert r["patches"] == (0, 1) and r["info"][0].tolist() == [0, 0, 0, ref.ST_UNREACHABLE] and np.isnan(r["score"])
    r = ref.subdtw(q[:5], y[:13], 5, 1, ((1, 3),))
    assert r["patches"] == (1, 1) and r["info"][0, 0] == 5 and r["info"][0, 2] - r["info"][0, 1] == 12
    bad = y.copy()
    bad[3, 2] = np.nan
    r = ref.subdtw(q, bad, 5, 3, ref.SYMMETRIC)
    assert r["patches"] == (0, 7) and (r["info"][:, 3] == ref.ST_UNDEFINED).all() and (r["cost"] == 0).all()
    r = ref.subdtw(q, y[:0], 5, 3, ref.SYMMETRIC)
    assert r["patches"] == (0, 7) and (r["info"][:, 3] == ref.ST_UNREACHABLE).all()
    for T, st in ((0, ref.ST_QUERY), (257, ref.ST_QUERY)):
        r = ref.subdtw(_features(rng, T, 8), y, 0, 1, ref.SYMMETRIC)
        assert r["patches"] == (0, 0) and r["query_status"] == st
    # all-zero features: cost 0 everywhere, every tie falls to N, then the step order, then the smallest j
    z = np.zeros((6, 4), np.float32)
    r = ref.subdtw(z[:3], z, 0, 1, ref.SYMMETRIC)
    assert r["info"][0].tolist() == [3, 0, 0, 0] and r["score"] == 0.0      # (1, 0) twice down column 0: the smallest j
    r = ref.subdtw(z[:3], z, 0, 1, ((1, 1),))
    assert r["info"][0].tolist() == [3, 0, 2, 0]
    # the step order decides between two predecessors of one key: the end (1, 1) comes from (0, 0) or from (0, 1)
    d = np.array([[0, 0, 0], [5, 0, 7]], np.int64)
    assert ref.patch_dp(d, [(1, 1), (1, 0)]) == (0, 2, 0, 1, ref.ST_OK)
    assert ref.patch_dp(d, [(1, 0), (1, 1)]) == (0, 2, 1, 1, ref.ST_OK)


# ---- swc_cmvn's reference ----

def test_cmvn_reference_order_and_properties():
    rng = np.random.default_rng(8)
    for T in (1, 2, 255, 256, 257, 1000):
        c = (rng.standard_normal((T, 5)) * [1, 10, 0.1, 3, 1] + [0, 5, -2, 100, 0]).astype(np.float32)
        c[:, 4] = 0.75                                   # a constant column
        out = ref.cmvn(c)
        assert out.dtype == np.float32 and out.shape == c.shape and (out[:, 4] == 0).all()
        if T == 1:
            assert (out == 0).all()
            continue
        assert np.abs(out[:, :4].astype(np.float64).mean(0)).max() < 1e-6 and np.abs(out[:, :4].astype(np.float64).std(0) - 1).max() < 1e-6
        # the stated order, spelled out with Python floats for one column
        col = [float(v) for v in c[:, 1].astype(np.float64)]
        parts = []
        for b0 in range(0, T, 256):
            a = 0.0
            for v in col[b0:b0 + 256]:
                a += v
            parts.append(a)
        tot = 0.0
        for a in parts:
            tot += a
        assert ref.block_sum(c.astype(np.float64))[1] == tot
    c = rng.standard_normal((300, 3)).astype(np.float32)
    c[7, 1] = np.nan
    out = ref.cmvn(c)
    assert np.isnan(out[:, 1]).all() and np.isfinite(out[:, [0, 2]]).all()
    assert ref.cmvn(np.zeros((0, 3), np.float32)).shape == (0, 3)


# ---- the front end: the mel bank and the tables ----

def test_mel_filterbank_default_is_unchanged_and_f_max_moves_the_upper_edge():
    from simwhisper_codec_amd import metrics
    from simwhisper_codec_amd._lib import SwcError

    def before(sample_rate, W, n_mels):
        """mel_filterbank as it stood before f_max"""
        sr, W, M = float(sample_rate), int(W), int(n_mels)
        edges = metrics._mel_to_hz(np.linspace(0.0, float(metrics._hz_to_mel(sr / 2.0)), M + 2))
        edges[0], edges[-1] = 0.0, sr / 2.0
        bins = np.arange(W // 2 + 1, dtype=np.float64) * (sr / W)
        rising = (bins[None, :] - edges[:M, None]) / (edges[1:M + 1] - edges[:M])[:, None]
        falling = (edges[2:, None] - bins[None, :]) / (edges[2:] - edges[1:M + 1])[:, None]
        return np.maximum(0.0, np.minimum(rising, falling)) * (2.0 / (edges[2:] - edges[:M]))[:, None]

    for sr, W, M in [(16000, 512, 80), (16000, 2048, 320), (8000, 256, 40), (22050, 1024, 80), (48000, 2048, 25), (16000, 32, 5)]:
        a, b = metrics.mel_filterbank(sr, W, M), before(sr, W, M)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        assert metrics.mel_filterbank(sr, W, M, f_max=None).tobytes() == b.tobytes()
        assert metrics.mel_filterbank(sr, W, M, f_max=sr / 2.0).tobytes() == b.tobytes()
    fb = metrics.mel_filterbank(16000, 512, 40, f_max=5000.0)
    bins = np.arange(257) * (16000 / 512)
    assert fb.shape == (40, 257) and (fb[:, bins >= 5000.0] == 0).all() and fb[-1][bins < 5000.0].max() > 0
    for f_max in (0.0, -1.0, 8000.1, float("nan")):
        with pytest.raises(SwcError):
            metrics.mel_filterbank(16000, 512, 40, f_max=f_max)


@pytest.mark.parametrize("sr,W,H,L", [(8000, 256, 32, 100), (16000, 512, 64, 100), (22050, 1024, 88, 100), (48000, 2048, 192, 100)])
def test_warpq_table_shapes(sr, W, H, L):
    from simwhisper_codec_amd import metrics
    assert metrics.warpq_params(sr) == (W, H)
    assert metrics.warpq_patch(sr, 400.0) == (L, L // 2)
    t = metrics.warpq_table(sr, "cpu")
    assert (t["W"], t["H"], t["n_mels"], t["K"]) == (W, H, 40, 13) and t["f_max"] == min(5000.0, sr / 2)
    assert t["dct"].shape == (13, 40) and t["dct"].dtype == torch.float32
    assert all(t[k].shape == (40,) and t[k].dtype == torch.int32 for k in ("first", "count", "off"))
    assert int(t["off"][-1] + t["count"][-1]) == t["w"].numel()
    assert int((t["first"] + t["count"]).max()) <= int(np.ceil(t["f_max"] * W / sr)) + 1 <= W // 2 + 1
    # row 0 of the DCT is the level (c0): a constant, and the rows are orthonormal
    d = metrics.dct_matrix(13, 40, first=0)
    assert np.allclose(d[0], 1 / np.sqrt(40)) and np.allclose(d @ d.T, np.eye(13), atol=1e-12)
    assert metrics.warpq_table(sr, "cpu") is t


def test_the_reference_alone_orders_noise_levels():
    """the whole chain on the host in float64 (tests/mcd_ref.py's cepstra with warpq_table's bank and DCT, then the reference's
    normalisation and search): white noise at 0 dB scores worse than at 30 dB, and both worse than 0"""
    import mcd_ref
    from simwhisper_codec_amd import metrics, synth
    t = metrics.warpq_table(16000, "cpu")
    bank = mcd_ref.dense_bank(t["first"].numpy(), t["count"].numpy(), t["off"].numpy(), t["w"].numpy(), t["W"] // 2 + 1)
    feats = lambda v: ref.cmvn(mcd_ref.cepstra(v, t["W"], t["H"], bank, t["dct"].numpy().astype(np.float64)).astype(np.float32))
    x = synth.synth_audio(24000, index=3, kind="speech").numpy().astype(np.float32)
    noise = np.random.default_rng(5).standard_normal(len(x))
    g = np.sqrt(np.mean(x.astype(np.float64) ** 2) / np.mean(noise ** 2))
    fx = feats(x)
    score = [ref.subdtw(feats((x + g * 10.0 ** (-snr / 20.0) * noise).astype(np.float32)), fx, 100, 50, ref.WARPQ)["score"] for snr in (0.0, 30.0)]
    print("the reference's score at 0 dB and 30 dB SNR:", score)
    assert ref.subdtw(fx, fx, 100, 50, ref.WARPQ)["score"] == 0.0
    # why the default has a (1, 1) step: without one the diagonal cannot be walked, and identity is not 0 (59.08 here)
    assert ref.subdtw(fx, fx, 100, 50, ref.ASYMMETRIC)["score"] > 0.0
    assert score[0] > score[1] > 0.0


def test_python_surface_refusals_without_gpu():
    from simwhisper_codec_amd import metrics
    from simwhisper_codec_amd._lib import SwcError
    x = [torch.zeros(1600)]
    with pytest.raises(SwcError, match="no CPU fallback"):
        metrics.warpq(x, x, device="cpu")
    with pytest.raises(SwcError, match="no CPU fallback"):
        metrics.subsequence_dtw([torch.zeros(3, 2)], [torch.zeros(5, 2)], device="cpu")
    for ms in (0.0, -1.0, 1.9, 1030.0, float("nan"), "x"):
        with pytest.raises(SwcError, match="patch_ms"):
            metrics.warpq_patch(16000, ms)
    assert metrics.warpq_patch(16000, 1024.0) == (256, 128) and metrics.warpq_patch(16000, 4.0) == (1, 1)
    for sr in (0, -5, "x", 200000):
        with pytest.raises(SwcError):
            metrics.warpq_params(sr)
    for st in ((), ((0, 0),), ((1, 1), (1, 1)), ((0, 1),), ((4, 0),), ((1, -1),), ((1, 1),) * 5, 7, ((1, 2, 3),)):
        with pytest.raises(SwcError, match="steps"):
            metrics.check_steps("warpq", st)
    for st in STEP_SETS:
        assert metrics.check_steps("warpq", [list(s) for s in st]) == st


def test_the_tool_parses_its_flags():
    import evaluate_warpq
    p = evaluate_warpq.build_parser()
    a = p.parse_args(["--original_dir", "A", "--synthesized_dir", "B"])
    assert (a.sample_rate, a.batch_size, a.no_vad, a.patch_ms, a.align, a.max_lag_ms, a.verbose) == (16000, 32, False, 400.0, "none", 50.0, False)
    a = p.parse_args(["--original_dir", "A", "--synthesized_dir", "B", "--no_vad", "--patch_ms", "200", "--align", "envelope",
                      "--max_lag_ms", "20", "--verbose", "--sample_rate", "8000"])
    assert (a.no_vad, a.patch_ms, a.align, a.max_lag_ms, a.verbose, a.sample_rate) == (True, 200.0, "envelope", 20.0, True, 8000)
    with pytest.raises(SystemExit):
        p.parse_args(["--original_dir", "A"])
    nan = float("nan")
    assert evaluate_warpq.summarise(["a", "b", "c", "d"], [1.0, nan, 3.0, 8.0]) == (4.0, 3.0, ["b"])
    assert evaluate_warpq.summarise(["a", "b"], [1.0, 2.0]) == (1.5, 1.5, [])
    assert evaluate_warpq.summarise(["a"], [nan]) == (None, None, ["a"])
