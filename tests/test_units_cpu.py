"""swc_code_usage and swc_code_compare (the token-level measures), the parts that need no GPU: the C-ABI of include/swc_units.h
(declarations == bindings == exports, a table apart from the others, the limits), every argument check before any launch, the
plain-Python restatement (tests/units_ref.py) against independent definitions, usage_from_counts on closed forms, the refusals
of the Python surface and the CLI flag."""
import ctypes as C
import functools
import itertools
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

import units_ref as ref  # noqa: E402

NAMES = {"swc_code_usage", "swc_code_compare"}


# ---- ABI and arguments ----

def _header(name="swc_units.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", " ", _header(name), flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(swc_\w+)\s*\(", hdr, flags=re.M))


def test_units_header_declarations_are_bound():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    declared = _declared("swc_units.h")
    assert declared == NAMES == set(_lib.UNITS_SIGNATURES)
    for name in declared:
        fn = getattr(lib, name)                       # exported by the library
        argtypes, restype = _lib.UNITS_SIGNATURES[name]
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    seen = set()
    for m in re.finditer(r"\b(?:int|int64_t)\s+(swc_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        assert len(m.group(2).split(",")) == len(_lib.UNITS_SIGNATURES[m.group(1)][0]), m.group(1)
        seen.add(m.group(1))
    assert seen == declared
    assert [len(_lib.UNITS_SIGNATURES[n][0]) for n in sorted(NAMES)] == [22, 12]


def test_units_table_is_apart_from_the_others():
    from simwhisper_codec_amd import _lib
    mine = set(_lib.UNITS_SIGNATURES)
    assert not mine & set(_lib.exported_symbols())
    others = [v for k, v in vars(_lib).items() if (k.endswith("SIGNATURES") or k == "PLAIN") and k != "UNITS_SIGNATURES"]
    assert len(others) >= 17
    for other in others:
        assert not mine & set(other)
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "swc_units.h":
            assert not mine & _declared(h)
            assert "swc_code_usage" not in _header(h) and "swc_code_compare" not in _header(h)


def test_constants_agree_with_the_header_and_the_reference():
    from simwhisper_codec_amd import _lib, units
    hdr = _header()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert val("SWC_UNITS_MAX_GROUPS") == _lib.UNITS_MAX_GROUPS == ref.MAX_GROUPS == 8
    assert val("SWC_UNITS_MAX_CODES") == _lib.UNITS_MAX_CODES == ref.MAX_CODES == 16384
    assert val("SWC_UNITS_MAX_FRAMES") == _lib.UNITS_MAX_FRAMES == ref.MAX_FRAMES == units.MAX_FRAMES == 8192
    assert val("SWC_UNITS_CHUNK") == _lib.UNITS_CHUNK == ref.CHUNK
    assert val("SWC_UNITS_STRIP") == _lib.UNITS_STRIP == ref.STRIP == 256
    assert re.search(r"#define SWC_UNITS_USAGE_MAX_FRAMES \(1 << 24\)", hdr) and _lib.UNITS_USAGE_MAX_FRAMES == ref.USAGE_MAX_FRAMES == 1 << 24
    # what the limits are for: one group's int32 histogram in 64 KB, a symbol in 16 bits beside the reserved one, and the LDS of
    # the edit distance (two symbol rows, one int32 boundary row) inside the 160 KB of a compute unit
    assert 4 * ref.MAX_CODES == 64 << 10 and ref.MAX_CODES < 0xffff
    assert 2 * 2 * ref.MAX_FRAMES + 4 * (ref.MAX_FRAMES + 1) + 2 * 4 * (ref.STRIP + 1) < 160 << 10


def test_build_sees_the_new_object_and_a_touched_header(monkeypatch):
    from simwhisper_codec_amd import build
    build.build_library()
    assert not build._stale()
    assert "swc_units.hip" in build.SOURCES and "swc_units.hip" not in build.EXTRA_FLAGS
    hdr = os.path.join(ROOT, "include", "swc_units.h")
    real = os.path.getmtime
    newer = real(build.LIB_PATH) + 10
    monkeypatch.setattr(os.path, "getmtime", lambda p: newer if os.path.abspath(p) == hdr else real(p))
    assert build._stale()


def _buffer():
    raw = (C.c_char * 1024)()
    return raw, C.c_void_p((C.addressof(raw) + 255) & ~255)


def _lv(*levels):
    return (C.c_int32 * 4)(*levels) if levels else None


def test_usage_arg_checks_without_gpu():
    """every check happens before any launch: host pointers that are never dereferenced stand in for device memory"""
    from simwhisper_codec_amd import _lib
    lib = _lib.load()
    keep, p = _buffer()

    def call(rows=p, ldg=p, n=p, es=4, lv=(8, 7, 6, 6), G=8, mf=100, hist=p, rep=p, tot=p, B=2):
        return lib.swc_code_usage(rows, ldg, n, es, _lv(*lv) if lv is not None else None, G, mf, hist, rep, tot, B, None)

    for kw, word in [(dict(rows=None), b"null"), (dict(ldg=None), b"null"), (dict(n=None), b"null"), (dict(lv=None), b"null"),
                     (dict(hist=None), b"null"), (dict(rep=None), b"null"), (dict(tot=None), b"null"),
                     (dict(B=65536), b"B="), (dict(B=-1), b"B="), (dict(G=0), b"G="), (dict(G=9), b"G="),
                     (dict(es=2), b"elem_size"), (dict(lv=(5, 29, 113, 1)), b"levels"), (dict(lv=(129, 127, 1, 1)), b"levels"),
                     (dict(lv=(8, 1, 6, 6)), b"levels"), (dict(lv=(16385, 1, 1, 1)), b"levels"), (dict(lv=(5, 29, 113, 1)), b"levels"),
                     (dict(lv=(2, 2, 4097, 1)), b"levels"), (dict(lv=(11, 11, 11, 13)), b"levels"),
                     (dict(mf=-1), b"max_frames"), (dict(mf=(1 << 24) + 1), b"max_frames")]:
        assert call(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    assert 11 * 11 * 11 * 13 > 16384 and 5 * 29 * 113 == 16385     # products just above the limit
    assert call(B=0) == 0 and call(mf=0) == 0                        # nothing to launch
    assert call(B=0, lv=(16, 16, 8, 8)) == 0                         # 16384 codes exactly are accepted


def test_compare_arg_checks_without_gpu():
    from simwhisper_codec_amd import _lib
    lib = _lib.load()
    keep, p = _buffer()
    ptrs = ("ra", "la", "na", "rb", "lb", "nb", "match", "both", "lm", "l1", "fm", "bad", "edit", "len_a", "len_b")

    def call(es=4, lv=(8, 7, 6, 6), G=8, mf=100, dedup=1, B=2, **kw):
        a = {k: kw.get(k, p) for k in ptrs}
        return lib.swc_code_compare(a["ra"], a["la"], a["na"], a["rb"], a["lb"], a["nb"], es, _lv(*lv) if lv is not None else None, G,
                                    mf, dedup, a["match"], a["both"], a["lm"], a["l1"], a["fm"], a["bad"], a["edit"], a["len_a"],
                                    a["len_b"], B, None)

    cases = [({k: None}, b"null") for k in ptrs] + [
        (dict(lv=None), b"null"), (dict(B=65536), b"B="), (dict(B=-1), b"B="), (dict(G=0), b"G="), (dict(G=9), b"G="),
        (dict(es=2), b"elem_size"), (dict(lv=(8, 1, 6, 6)), b"levels"), (dict(lv=(11, 11, 11, 13)), b"levels"),
        (dict(lv=(2, 2, 2, 1025)), b"levels"), (dict(mf=8193), b"max_frames"), (dict(mf=-1), b"max_frames")]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        assert word in lib.swc_last_error(), (kw, lib.swc_last_error())
    assert call(B=0) == 0 and call(B=0, mf=8192) == 0


# ---- the reference against itself ----

def _lev_recursive(a, b, n_codes):
    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(d(i - 1, j) + 1, d(i, j - 1) + 1, d(i - 1, j - 1) + (0 if ref.equal(a[i - 1], b[j - 1], n_codes) else 1))
    return d(len(a), len(b))


def test_reference_levenshtein_against_the_recursive_definition():
    strings = [s for n in range(5) for s in itertools.product((0, 1), repeat=n)]
    assert len(strings) == 31
    for a in strings:
        for b in strings:
            assert ref.levenshtein(list(a), list(b), 16) == _lev_recursive(a, b, 16), (a, b)
    assert ref.levenshtein([0, 1, 1, 0], [1, 1, 0, 0], 16) == 2 and ref.levenshtein([], [3, 4], 16) == 2
    # an invalid value matches nothing: two rows of the same invalid value are as far apart as two rows can be
    for bad in (-1, 16, 2047):
        assert ref.levenshtein([bad] * 3, [bad] * 3, 16) == 3 == _lev_recursive((bad,) * 3, (bad,) * 3, 16)
        assert not ref.equal(bad, bad, 16)
    assert ref.levenshtein([1, -1, 2], [1, -1, 2], 16) == 1


def test_reference_dedup_and_counts():
    assert ref.dedup([5] * 40, 16) == [5] and ref.dedup([], 16) == []
    assert ref.dedup([1, 1, 2, 2, 2, 1, 3, 3], 16) == [1, 2, 1, 3]
    assert ref.dedup([-1, -1, 4, 4, 99, 99, 99, 4], 16) == [-1, -1, 4, 99, 99, 99, 4]      # every invalid value is kept
    assert ref.code_levels(8 * 7 * 6 * 5 + 8 * 7 * 2 + 8 * 3 + 1, (8, 7, 6, 6)) == [1, 3, 2, 5]
    rows = np.array([[3, 3, -1, -1, 3, 16, 3, 3]])
    hist, rep, tot = ref.usage([rows], (2, 2, 2, 2), 1)
    assert hist[0].tolist() == [0, 0, 0, 5] + [0] * 12 and rep.tolist() == [2] and tot.tolist() == [8, 3]
    r = ref.compare(rows, rows, (2, 2, 2, 2), 1, do_dedup=True)
    assert r["match"].tolist() == [5] and r["both_valid"].tolist() == [5] and int(r["frame_match"]) == 5 and r["bad"].tolist() == [3, 3]
    assert r["len_a"].tolist() == [6] and r["edit"].tolist() == [3]     # 3 -1 -1 3 16 3 against itself: the three invalid ones
    r = ref.compare(np.array([[0, 15, 5]]), np.array([[15, 15]]), (2, 2, 2, 2), 1, do_dedup=False)
    assert r["match"].tolist() == [1] and r["level_match"].tolist() == [[1, 1, 1, 1]] and r["level_l1"].tolist() == [[1, 1, 1, 1]]
    assert r["edit"].tolist() == [2] and r["len_a"].tolist() == [3] and r["len_b"].tolist() == [2]


# ---- usage_from_counts ----

def test_usage_from_counts_closed_forms():
    from simwhisper_codec_amd import units
    for k in range(0, 5):
        hist = np.zeros((2, 16), dtype=np.int64)
        hist[:, :2 ** k] = 7
        r = units.usage_from_counts(hist, [0, 0], [7 * 2 ** k, 0], (2, 2, 2, 2))
        assert r["entropy_bits"].tolist() == [float(k)] * 2 and r["perplexity"].tolist() == [float(2 ** k)] * 2
        assert r["used"].tolist() == [2 ** k] * 2 and r["utilisation"].tolist() == [2 ** k / 16] * 2
        assert r["bits_per_frame"] == 2.0 * k and r["bitrate_bps"] == 2.0 * k * 12.5 and r["nominal_bps"] == 2 * 4 * 12.5
    hist = np.zeros((1, 2016), dtype=np.int64)
    hist[0, 1234] = 99
    r = units.usage_from_counts(hist, [98], [99, 1], (8, 7, 6, 6), frame_rate=12.5)
    assert r["entropy_bits"].tolist() == [0.0] and r["perplexity"].tolist() == [1.0] and r["used"].tolist() == [1]
    assert r["repeat_rate"].tolist() == [98 / 99] and r["frames"] == 99 and r["bad"] == 1
    assert abs(r["nominal_bps"] - math.log2(2016) * 12.5) < 1e-12
    assert r["level_hist"].shape == (1, 4, 8)
    lv = ref.code_levels(1234, (8, 7, 6, 6))
    for d in range(4):
        want = [0] * 8
        want[lv[d]] = 99
        assert r["level_hist"][0, d].tolist() == want
    empty = units.usage_from_counts(np.zeros((3, 16), dtype=np.int64), [0] * 3, [0, 0], (2, 2, 2, 2))
    assert np.isnan(empty["entropy_bits"]).all() and np.isnan(empty["perplexity"]).all() and np.isnan(empty["repeat_rate"]).all()
    assert math.isnan(empty["bits_per_frame"]) and math.isnan(empty["bitrate_bps"]) and empty["used"].tolist() == [0, 0, 0]
    # a hand-made histogram over levels (3, 2, 2, 2): code = l0 + 3 l1 + 6 l2 + 12 l3
    hist = np.zeros((1, 24), dtype=np.int64)
    hist[0, 2 + 3 * 1 + 6 * 0 + 12 * 1] = 5
    hist[0, 0 + 3 * 1 + 6 * 1 + 12 * 0] = 3
    hist[0, 1] = 2
    r = units.usage_from_counts(hist, [0], [10, 0], (3, 2, 2, 2))
    assert r["level_hist"][0].tolist() == [[3, 2, 5], [2, 8, 0], [7, 3, 0], [5, 5, 0]]


def test_usage_from_counts_random_histogram():
    from simwhisper_codec_amd import units
    rng = np.random.default_rng(5)
    hist = rng.integers(0, 1000, size=(8, 2016)).astype(np.int64)
    hist[rng.random(hist.shape) < 0.3] = 0
    r = units.usage_from_counts(hist, rng.integers(0, 50, 8), [int(hist[0].sum()), 0], (8, 7, 6, 6))
    for g in range(8):
        c = hist[g][hist[g] > 0].astype(np.float64)
        n = c.sum()
        want = float(np.log2(n) - (c * np.log2(c)).sum() / n)                 # the same entropy, another expression and order
        # the two sum 2016 terms in different orders: n_codes 2^-53 = 2.2e-13 relative, with four orders of margin
        assert abs(r["entropy_bits"][g] - want) <= 1e-9 * want
        assert abs(r["perplexity"][g] - 2.0 ** want) <= 1e-9 * 2.0 ** want * 11
        assert r["used"][g] == len(c)
        for d in range(4):
            want_h = [0] * 8
            for code in range(2016):
                want_h[ref.code_levels(code, (8, 7, 6, 6))[d]] += int(hist[g, code])
            assert r["level_hist"][g, d].tolist() == want_h
    assert abs(r["bits_per_frame"] - r["entropy_bits"].sum()) < 1e-12


# ---- the refusals of the Python surface, each before any CUDA call ----

@pytest.fixture
def no_cuda(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a CUDA call before the refusal")
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    monkeypatch.setattr(torch.Tensor, "cuda", boom)
    monkeypatch.setattr(torch.Tensor, "to", boom)
    from simwhisper_codec_amd import _lib
    monkeypatch.setattr(_lib, "load", boom)


def test_python_refusals(no_cuda):
    from simwhisper_codec_amd import units
    from simwhisper_codec_amd._lib import SwcError
    good = [torch.zeros(8, 5, dtype=torch.int32)]
    with pytest.raises(SwcError, match=r"Usage: the counting is a HIP kernel \(there is no CPU fallback\)"):
        units.Usage(device="cpu")
    with pytest.raises(SwcError, match=r"Usage: the counting is a HIP kernel \(there is no CPU fallback\)"):
        units.usage(good, device=torch.device("cpu"))
    with pytest.raises(SwcError, match=r"agreement: the comparison is a HIP kernel \(there is no CPU fallback\)"):
        units.agreement(good, good, device="cpu")
    for lv in ((8, 7, 6), (8, 1, 6, 6), (16, 16, 16, 16), (8, 7, 6, 6, 2), None, (2, 2, 2, 1025)):
        with pytest.raises(SwcError, match="levels"):
            units.Usage(levels=lv)
        with pytest.raises(SwcError, match="levels"):
            units.agreement(good, good, levels=lv)
        with pytest.raises(SwcError, match="levels"):
            units.usage_from_counts(np.zeros((1, 4)), [0], [0, 0], lv)
    with pytest.raises(SwcError, match="groups"):
        units.Usage(groups=9)
    with pytest.raises(SwcError, match="1 reference and 2 other"):
        units.agreement(good, good + good)
    for bad in ([torch.zeros(5, dtype=torch.int32)], [torch.zeros(8, 5)], [torch.zeros(7, 5, dtype=torch.int64)], [np.zeros((8, 5))],
                [torch.zeros(8, 2, 5, dtype=torch.int32)]):
        with pytest.raises(SwcError, match=r"expected \(8, T\) int32 or int64 code tensors"):
            units.agreement(good, bad)
    with pytest.raises(SwcError, match=r"8193 frames \(at most 8192\)"):
        units.agreement(good, [torch.zeros(8, 8193, dtype=torch.int32)])
    with pytest.raises(SwcError, match=r"8193 frames \(at most 8192\)"):
        units.agreement([torch.zeros(8, 8193, dtype=torch.int64)], good)
    with pytest.raises(SwcError, match="hist must be"):
        units.usage_from_counts(np.zeros((8, 2017)), [0] * 8, [0, 0], (8, 7, 6, 6))


def test_ops_refusals(no_cuda, monkeypatch):
    """the wrappers refuse on their own too (rows on the host, wrong counters), before the library is loaded... the levels first"""
    from simwhisper_codec_amd import _lib, ops
    monkeypatch.setattr(_lib, "load", lambda: None)
    good = [torch.zeros(8, 5, dtype=torch.int32)]
    hist, rep, tot = torch.zeros(8, 2016, dtype=torch.int64), torch.zeros(8, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(_lib.SwcError, match="levels"):
        ops.code_usage(good, hist, rep, tot, (8, 7, 6, 1))
    with pytest.raises(_lib.SwcError, match="hist must be"):
        ops.code_usage(good, hist[:, :100], rep, tot, (8, 7, 6, 6))
    with pytest.raises(_lib.SwcError, match="no CPU fallback"):
        ops.code_usage(good, hist, rep, tot, (8, 7, 6, 6))
    with pytest.raises(_lib.SwcError, match="0 utterances"):
        ops.code_usage([], hist, rep, tot, (8, 7, 6, 6))
    with pytest.raises(_lib.SwcError, match="no CPU fallback"):
        ops.code_compare(good, good, (8, 7, 6, 6))
    with pytest.raises(_lib.SwcError, match="1 reference and 0 other"):
        ops.code_compare(good, [], (8, 7, 6, 6))
    with pytest.raises(_lib.SwcError, match=r"8193 frames"):
        ops.code_compare([torch.zeros(8, 8193, dtype=torch.int32)], good, (8, 7, 6, 6))


# ---- the CLI flag ----

def test_code_stats_flag_parses_and_is_refused_outside_encode(tmp_path):
    import inference
    p = inference.build_parser()
    assert p.parse_args([]).code_stats is None
    assert p.parse_args(["--mode", "encode", "--code_stats", "x.json"]).code_stats == "x.json"
    for mode in ("roundtrip", "decode"):
        with pytest.raises(SystemExit, match="--code_stats counts the codes --mode encode writes"):
            inference.main(["--mode", mode, "--code_stats", str(tmp_path / "x.json"), "--device", "cpu"])
    assert not (tmp_path / "x.json").exists()


def test_evaluate_codes_tool_flags():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_codes
    a = evaluate_codes.build_parser().parse_args(["dir"])
    assert a.dir == "dir" and a.against is None and not a.no_dedup and a.levels == [8, 7, 6, 6]
    a = evaluate_codes.build_parser().parse_args(["dir", "--against", "d2", "--no_dedup", "--levels", "2", "2", "2", "2"])
    assert a.against == "d2" and a.no_dedup and a.levels == [2, 2, 2, 2]
    assert evaluate_codes.pair_up(["a/x.swc", "a/y.swc", "a/z.swc"], ["b/z.swc", "b/x.swc", "b/w.swc"]) == [("a/x.swc", "b/x.swc"), ("a/z.swc", "b/z.swc")]
