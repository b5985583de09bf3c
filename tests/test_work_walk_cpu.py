"""The work-walk case table (tests/work_walk.py) against the plan functions, without a GPU: every case still reports the
regime it is named for, the table covers the regimes the walks have, the regimes it leaves out cannot be reached, and the
plan functions refuse what swc_gemm / swc_dwconv7_ln refuse.  swc_gemm_plan / swc_dwconv7_ln_plan are host arithmetic."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import work_walk as ww  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    return _lib.load()


@pytest.mark.parametrize("case", ww.GEMM_CASES, ids=lambda c: c["name"])
def test_gemm_case_reports_its_regime(lib, case):
    p = ww.gemm_plan(case)
    assert (p["tile_m"], p["waves"]) == (case["tile"], case["waves"]), p
    assert p["tile_n"] == (256 if case["waves"] == 8 else 128) and p["slots"] == (256 if case["waves"] == 8 else 512)
    assert p["k_slice"] == ww.K_SLICE[case["a"]] and p["k_slices"] == -(-case["K"] // p["k_slice"])
    ntiles = p["n_tiles_m"] * p["n_tiles_n"]
    assert ntiles > p["slots"] and p["grid"] == p["slots"], p                   # a capped grid: workgroups walk
    assert ww.walk_class(p) == case["walk"], (ww.walk_class(p), p)
    lengths = ww.walk_lengths(p)
    if case["walk"] == "plus1":
        assert ntiles == p["slots"] + 1 and lengths == {1, 2}
    elif case["walk"] == "mixed":
        assert ntiles % 8 != 0 and lengths == {2, 3}
    elif case["walk"] == "deep":
        assert max(lengths) >= 4
    assert p["band"] == case["band"] and (p["band"] == 4) == (p["n_tiles_n"] >= 12)
    # ragged tails throughout
    assert case["M"] % p["tile_m"] != 0 and case["N"] % p["tile_n"] != 0
    plain = case["conv"] is None and case["K"] % p["k_slice"] == 0
    assert p["plain"] == int(plain)
    compiled = case["c"] != "f32" and plain
    assert p["act_body"] == ((1 if case["gelu"] else 0) if compiled else 2)
    # the bit-equality split of the GPU test: every launch on the same kernel, one tile per workgroup, together the whole window
    chunks = ww.gemm_chunks(case)
    if case["split"] is None:                                  # no cut exists, along M or along N
        assert chunks is None
        return
    assert chunks, "no cut into one-tile-per-workgroup launches"
    assert (case["split"] == "cols") == (p["n_tiles_m"] == 1)
    covered = 0
    for row0, rows, col0, cols in chunks:
        assert (row0, col0) == ((covered, 0) if case["split"] == "rows" else (0, covered))
        covered += rows if case["split"] == "rows" else cols
        q = ww.gemm_plan(case, rows, cols)
        assert q["grid"] == q["n_tiles_m"] * q["n_tiles_n"] <= q["slots"]
        assert all(q[k] == p[k] for k in ww.SAME_KERNEL)
    assert covered == (case["M"] if case["split"] == "rows" else case["N"])


def test_gemm_table_covers_the_walk_regimes(lib):
    cases = ww.GEMM_CASES
    plans = {c["name"]: ww.gemm_plan(c) for c in cases}
    have = lambda **kw: [c for c in cases if all((v(c) if callable(v) else c[k] == v) for k, v in kw.items())]
    # geometry x operand mode
    for tile in (256, 192, 128):
        for a in ("bf16", "fp8", "f16s"):
            assert have(tile=tile, waves=8, a=a), (tile, a)
    for a in ("f32", "bf16", "fp8", "f16s"):
        assert have(tile=128, waves=4, a=a), a
    for a in ("bf16", "f16s"):
        assert have(tile=64, waves=4, a=a), a
    # walk shape per geometry, where the chooser can reach it (work_walk.py lists what it cannot)
    for tile, waves in ((256, 8), (192, 8), (128, 8), (128, 4)):
        for walk in ("mixed", "deep"):
            assert have(tile=tile, waves=waves, walk=walk), (tile, waves, walk)
    assert have(tile=128, waves=4, walk="plus1") and have(tile=64, waves=4, walk="plus1")
    # band
    assert have(band=1)
    for mod in (1, 2, 3):
        assert [c for c in have(band=4) if plans[c["name"]]["n_tiles_m"] % 4 == mod], mod
    # staging
    assert have(conv=None)
    assert have(conv=lambda c: c["conv"] and c["conv"][:3] == (7, 3, 1))
    s2 = have(conv=lambda c: c["conv"] and c["conv"][:3] == (3, 1, 2))
    assert s2 and all(ww.conv_geometry(c["conv"])[4] != ww.conv_geometry(c["conv"])[5] for c in s2)
    # K: one, two, five or more slices; a K that is no slice multiple (the non-plain staging of a GEMM)
    slices = {plans[c["name"]]["k_slices"] for c in cases if c["conv"] is None}
    assert 1 in slices and 2 in slices and max(slices) >= 5
    assert [c for c in cases if c["conv"] is None and c["K"] % ww.K_SLICE[c["a"]] and not plans[c["name"]]["plain"]]
    # epilogue
    full = dict(c="f32", bias=True, gelu=True, gamma=True, residual=True)
    assert have(unaligned=False, **full) and have(unaligned=True, **full)       # both f32 paths, every epilogue input
    assert have(inplace=True) and have(c="bf16") and have(c="f16s") and have(ldc_pad=lambda c: c["ldc_pad"] > 0)
    assert have(c="fp8", out_scale=lambda c: c["out_scale"] != 1.0)
    # tiles == slots + 1 on every 8-wave tile that reaches it (one row panel x 257 column tiles)
    for tile, reachable in ww.PLUS1_8WAVE.items():
        assert bool(have(tile=tile, waves=8, walk="plus1")) == reachable, tile
    # every kernel geometry x operand mode has a case with the bit-equality cut; one shape has none (work_walk.py says why)
    assert [c["name"] for c in cases if c["split"] is None] == ["fp8-192-plus1-1x257"]
    for c in cases:
        assert have(tile=c["tile"], waves=c["waves"], a=c["a"], split=lambda d: d["split"] is not None), c["name"]
    assert len({c["name"] for c in cases}) == len(cases)


def test_regimes_the_chooser_cannot_reach(lib):
    """what work_walk.py leaves out, shown through the plan: a retuned chooser that opens one of these fails here"""
    # tiles == slots + 1 on an 8-wave tile: 257 is prime, so it is 257 row panels x 1 column tile (N <= 256; below 256 columns no
    # 8-wave tile is taken) or 1 row panel x 257 column tiles (M <= tile rows, 65536 < N <= 65792).  Every M of both, at the ends
    # and in the middle of the N range
    for a in ("bf16", "fp8", "f16s"):
        reached = {tile: False for tile in ww.PLUS1_8WAVE}
        probe = ww.G("probe", a, "f32", 1, 256, 128, tile=0, waves=8, walk="plus1")
        shapes = [(m, n) for n in (255, 256) for m in range(256 * 128 + 1, 257 * 256 + 1)]
        shapes += [(m, n) for n in (65537, 65664, 65792) for m in range(1, 257)]
        for m, n in shapes:
            q = ww.gemm_plan(dict(probe, M=m, N=n))
            if q["waves"] == 8 and q["n_tiles_m"] * q["n_tiles_n"] == 257:
                reached[q["tile_m"]] = True
        assert reached == ww.PLUS1_8WAVE, (a, reached)
    # the 64-row tile: never for f32 / fp8, never more than 2 * slots tiles
    for a in ("f32", "fp8", "bf16", "f16s"):
        for m in range(512, 49153, 61):
            for n in (96, 224, 352):
                q = ww.gemm_plan(ww.G("probe", a, "f32", m, n, 128, tile=64, waves=4, walk="two"))
                if q["tile_m"] == 64:
                    assert a in ("bf16", "f16s") and q["n_tiles_m"] * q["n_tiles_n"] <= 2 * q["slots"], (a, m, n, q)


@pytest.mark.parametrize("case", ww.DW_CASES, ids=lambda c: c["name"])
def test_dwconv_case_reports_its_regime(lib, case):
    p = ww.dw_plan(case)
    assert (p["S"], p["FULL"], p["slots"], p["per"]) == (case["S"], case["full"], case["slots"], case["per"]), p
    assert p["NK"] == (1 if case["C"] <= 256 else 2 if case["C"] <= 512 else 4)
    assert p["nst"] == -(-case["T"] // p["S"]) and p["nstrips"] == case["B"] * p["nst"] > p["slots"]
    assert case["T"] % p["S"] != 0 and 3 <= case["B"] <= 6
    assert p["grid"] % 8 == 0 and p["grid"] * p["per"] >= p["nstrips"] > (p["grid"] - 8) * p["per"]
    assert (p["nstrips"] % p["per"] != 0) == case["partial_last"]
    assert (ww.dw_straddles(p) > 0) == case["straddle"]
    groups = ww.dw_groups(case)
    assert groups and sum(n for _, n in groups) == case["B"]
    assert all(ww.dw_plan(case, n)["per"] == 1 for _, n in groups)


def test_dwconv_table_covers_the_walk_regimes(lib):
    for C_ in (64, 256, 260, 512, 768, 1024):
        assert {c["out"] for c in ww.DW_CASES if c["C"] == C_} == {"f32", "bf16"}, C_
    for per in (2, 3):
        assert [c for c in ww.DW_CASES if c["per"] == per and c["straddle"]]
        assert [c for c in ww.DW_CASES if c["per"] == per and c["partial_last"]]
    assert {c["slots"] for c in ww.DW_CASES} == {256, 512} and {c["full"] for c in ww.DW_CASES} == {0, 1}
    assert {c["B"] for c in ww.DW_CASES} == {3, 4, 5, 6}
    from simwhisper_codec_amd import ops
    p = ops.dwconv7_ln_plan(3, 2750, 512)                                      # the worked example of the header comment
    assert (p["nstrips"], p["slots"], p["per"]) == (516, 512, 2)


def test_plan_functions_refuse_what_the_launchers_refuse(lib):
    from simwhisper_codec_amd import _lib, ops
    good = ww.GEMM_CASES[0]
    assert lib.swc_gemm_plan(C.byref(ww.gemm_args(good)), None) == -1 and b"null plan" in lib.swc_last_error()
    out = _lib.GemmPlan()
    assert lib.swc_gemm_plan(None, C.byref(out)) == -1

    def bad(**kw):
        a = ww.gemm_args(good)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    refused = [bad(A=None), bad(C=None), bad(N=0), bad(K=0), bad(M=-1), bad(a_dtype=7), bad(c_dtype=_lib.FP8),
               bad(c_dtype=_lib.F16S), bad(a_dtype=_lib.F16S, c_dtype=_lib.BF16, K=64), bad(act=2), bad(K=68), bad(lda=60),
               bad(A=ww.FAKE + 8), bad(taps=0), bad(t_out=1000), bad(ldw=32), bad(ldc=good["N"] - 8), bad(ldr=8),
               bad(c_dtype=_lib.BF16, gamma=ww.FAKE), bad(a_dtype=_lib.F16S, c_dtype=_lib.F16S, N=344)]
    for a in refused:
        out.grid = 99
        rc_plan, msg_plan = lib.swc_gemm_plan(C.byref(a), C.byref(out)), lib.swc_last_error()
        assert rc_plan == -1 and out.grid == 0 and out.tile_m == 0
        assert lib.swc_gemm(C.byref(a), None) == -1 and lib.swc_last_error() == msg_plan   # refused before any launch
    with pytest.raises(_lib.SwcError):
        ops.gemm_plan(refused[0])
    # M == 0: swc_gemm launches nothing, the plan says so
    assert lib.swc_gemm_plan(C.byref(bad(M=0, t_in=1, t_out=1)), C.byref(out)) == 0 and out.grid == 0
    d = _lib.Dwconv7LnPlan()
    for B, T, C_, dt in ((2, 100, 0, 0), (2, 100, 258, 0), (2, 100, 1028, 1), (2, 100, 512, _lib.F16S), (2, 100, 512, _lib.FP8)):
        d.grid = 99
        assert lib.swc_dwconv7_ln_plan(B, T, C_, dt, C.byref(d)) == -1 and d.grid == 0 and d.S == 0
        msg = lib.swc_last_error()
        p1 = C.c_void_p(ww.FAKE)
        assert lib.swc_dwconv7_ln(p1, p1, p1, p1, p1, p1, B, T, C_, 1e-6, dt, None) == -1 and lib.swc_last_error() == msg
    assert lib.swc_dwconv7_ln_plan(2, 100, 512, 0, None) == -1
    assert lib.swc_dwconv7_ln_plan(0, 100, 512, 0, C.byref(d)) == 0 and (d.grid, d.per, d.S, d.slots) == (0, 0, 16, 512)
    with pytest.raises(_lib.SwcError):
        ops.dwconv7_ln_plan(2, 100, 258)
