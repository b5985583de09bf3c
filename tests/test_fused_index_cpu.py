"""The fused-kernel index tables (tests/fused_index.py) without a GPU: every branch of REQUIRED has a case and no case can be
deleted without uncovering one, the float64 references agree with independent statements, the hostile rows are as hostile as
promised, the fault model's walks pass the GPU test's criteria without a fault and fail them, in the case named for the
branch, with each fault, and profiles/fused_index_cases.txt is what the table computes."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_index as fi  # noqa: E402


# ------------------------------------------------------------------------------------------------------------ the table
def test_every_named_branch_has_a_case():
    rows = fi.all_cases()
    assert {k for k, _, _ in rows} == set(fi.REQUIRED)
    assert fi.uncovered(rows) == {}


def test_no_case_can_be_deleted():
    """without any one case of a table some branch of REQUIRED has no case left: uncovered() names it"""
    rows = fi.all_cases()
    texts = sorted({(k.split()[0], s) for k, s, _ in rows})       # an attention case is one row per form and layout
    assert len(texts) == len(fi.ATT_CASES) + len(fi.BLOCK_CASES) + len(fi.TAIL_M)
    for kind, text in texts:
        left = [r for r in rows if not (r[0].split()[0] == kind and r[1] == text)]
        assert fi.uncovered(left), f"the {kind} case `{text}` covers no branch of its own"


def test_case_list_file_matches_the_table():
    with open(os.path.join(ROOT, "profiles", "fused_index_cases.txt")) as f:
        assert f.read() == fi.cases_text()


def test_inputs_are_the_same_in_every_process():
    import zlib
    assert fi._g("attn", "T15").initial_seed() == zlib.crc32(b"('attn', 'T15')")
    assert torch.equal(fi.attn_base("T15"), torch.randn(5, 15, 384, generator=fi._g("attn", "T15")) * 0.7)


# ------------------------------------------------------------------------------------------------------------ attention
def test_attention_geometry_and_table():
    assert fi.LARGEST_T == 1500 and fi.att_case("T-largest")["lens"] == (1500,) and fi.att_case("T-largest")["H"] == 2
    d = fi.att_case("dense")
    assert d["T"] == 193 and d["lens"] == tuple(range(194)) and d["H"] == 2
    assert 194 * 193 * 3 * 2 * 64 < 15_000_000
    assert fi.eff_lens((-3, 70, 65), 65) == [0, 65, 65]
    assert fi.row_starts((64, 0, 0, 63, 17), 64) == ([0, 64, 64, 64, 127], 144)
    # 16-bit kernel: 128 queries per workgroup, 32 per wave; f32 kernel: 64 and 16
    assert "tile16-beyond-len" in fi.attn_branches("bf16", 128, (70,), 1) and "tile16-beyond-len" not in fi.attn_branches("f32", 128, (70,), 1)
    assert "wave-beyond-len" in fi.attn_branches("f32", 128, (70,), 1)                 # queries 80 .. 95: wave 1 of block 1
    assert "block-beyond-len" not in fi.attn_branches("bf16", 128, (70,), 1) and "block-beyond-len" in fi.attn_branches("f32", 128, (64,), 1)
    assert {"last-tile-full", "ntile=2", "len=128", "len=T"} <= fi.attn_branches("bf16", 128, (128,), 1)
    assert {"last-tile-one-key", "ntile=4"} <= fi.attn_branches("f16s", 193, (193,), 1)


@pytest.mark.parametrize("name", [c["name"] for c in fi.ATT_CASES if c["name"] not in ("dense", "B65535")])
def test_attention_reference_is_softmax_of_the_masked_scores(name):
    c = fi.att_case(name)
    T, H, lens = c["T"], c["H"], fi.eff_lens(c["lens"], c["T"])
    for form in ("f32", "bf16"):
        src = fi.source(fi.attn_input(name), form)
        ref = fi.attn_ref(src, c["lens"], T, H)
        q, k, v = (t.reshape(len(lens), T, H, 64).transpose(1, 2) for t in src.chunk(3, dim=-1))
        mask = torch.arange(T).view(1, 1, 1, T) >= torch.tensor(lens).view(-1, 1, 1, 1)
        p = torch.softmax((q @ k.transpose(-1, -2)).masked_fill(mask, float("-inf")), -1)
        want = (torch.nan_to_num(p) @ v).transpose(1, 2).reshape(len(lens), T, H * 64)
        ok = fi.valid_mask(c["lens"], T)
        assert float((ref - want)[ok].abs().max()) < 1e-12 and bool((ref[~ok] == 0).all())


def test_attention_reference_dense_and_single_row():
    src = fi.source(fi.attn_input("dense"), "f32")
    ref = fi.attn_ref(src, range(194), 193, 2)
    for n in (1, 64, 129, 193):
        q, k, v = (src[n, :n, i * 128:(i + 1) * 128].reshape(n, 2, 64).transpose(0, 1) for i in range(3))
        want = (torch.softmax(q @ k.transpose(1, 2), -1) @ v).transpose(0, 1).reshape(n, 128)
        assert float((ref[n, :n] - want).abs().max()) < 1e-12
    c = fi.att_case("B65535")
    src = fi.source(fi.attn_input("B65535"), "f32")
    ref = fi.attn_ref(src, c["lens"], 1, 2)
    assert torch.equal(ref[0], src[0, :, 256:]) and bool((ref[1] == 0).all()) and ref.shape == (65535, 1, 128)


@pytest.mark.parametrize("name", [c["name"] for c in fi.ATT_CASES])
def test_hostile_rows(name):
    """trap keys beat every valid score of their query by more than 40 (f32 and bf16-rounded inputs), trap values are a
    constant far from every valid one, everything is finite and below the split-f16 range"""
    c = fi.att_case(name)
    T, H, D = c["T"], c["H"], c["H"] * 64
    x = fi.attn_input(name)
    assert bool(torch.isfinite(x).all()) and float(x.abs().max()) < fi.TRAP_LIMIT
    ok = fi.valid_mask(c["lens"], T)
    assert torch.equal(x[ok], fi.attn_base(name)[ok])
    if bool((~ok).any()):
        assert bool((x[~ok][:, 2 * D:] == fi.TRAP_V).all()) and float(x[ok][:, 2 * D:].abs().max()) < fi.TRAP_V / 50
        assert float(x[~ok][:, :2 * D].abs().max()) > 2 * float(x[ok].abs().max())
    if T > 1:
        for form in ("f32", "bf16"):
            assert fi.trap_margin(fi.source(x, form), c["lens"], T, H) > fi.TRAP_MARGIN
        z = fi.with_traps(fi.attn_base(name), c["lens"], T, H, zeros=True)
        assert torch.equal(z[ok], x[ok]) and bool((z[~ok] == 0).all())
    hot, cold = fi.spike_input()
    n = fi.SPIKE["n"]
    assert torch.equal(hot[0, n, 64:128], hot[0, n - 1, 64:128]) and bool((cold[0, n] == 0).all()) and torch.equal(hot[0, :n], cold[0, :n])
    q10 = hot[0, fi.SPIKE["query"], :64].double()
    s = hot[0, :n, 64:128].double() @ q10
    assert int(s.argmax()) == n - 1 and float(s[n - 1] - s[:n - 1].max()) > fi.TRAP_MARGIN and float(hot.abs().max()) < fi.TRAP_LIMIT


def _walk(form, fault=None):
    return lambda buf, lens, T, H, rs: fi.attn_walk(buf, lens, T, H, form, fault=fault, row_start=rs)


@pytest.mark.parametrize("form", ["f32", "bf16"])      # the two geometries (64 / 128 queries per workgroup); bf16: lazy rescale, packed
def test_attention_walk_without_fault_passes_every_criterion(form):
    for c in fi.ATT_CASES:
        if c["model"]:
            assert fi.attn_criteria(_walk(form), form, c["name"]) == [], (form, c["name"])


@pytest.mark.parametrize("fault", sorted(fi.ATT_FAULTS))
def test_attention_fault_is_caught_by_the_case_named_for_its_branch(fault):
    branch = fi.ATT_FAULTS[fault][1]
    form = "bf16"                                           # (the 16-bit geometry has every branch the faults touch)
    caught = {}
    for c in fi.ATT_CASES:
        own = fi.attn_branches(form, c["T"], c["lens"], c["H"]) | fi.attn_branches(form, c["T"], c["lens"], c["H"], packed=True)
        if c["model"] and c["name"] != "dense" and branch in own:
            caught[c["name"]] = fi.attn_criteria(_walk(form, fault), form, c["name"])
    assert caught and any(caught.values()), (fault, branch, caught)
    want = {"mask<=": "values", "ntile-floor": "values", "slot-reuse": "values", "clamp-len": "traps-as-zeros",
            "packed-r0": "packed-equals-padded", "head-offset": "values"}[fault]
    assert any(want in v for v in caught.values()), (fault, caught)


def test_attention_faults_in_the_f32_geometry():
    """the faults that exist in attn_kernel too (no query clamp, no packed layout there)"""
    for fault, name in (("mask<=", "T128"), ("ntile-floor", "clamp"), ("slot-reuse", "T192"), ("head-offset", "H12")):
        assert fi.ATT_FAULTS[fault][1] in fi.attn_branches("f32", *(fi.att_case(name)[k] for k in ("T", "lens", "H")))
        assert "values" in fi.attn_criteria(_walk("f32", fault), "f32", name), (fault, name)


def test_tolerance_table_quotes_the_existing_tests():
    with open(os.path.join(ROOT, "tests", "test_kernels_gpu.py")) as f:
        text = f.read()
    for line in ("assert err < (1e-5 if dtype == torch.float32 else 1e-2), (b, L, err)", "src, tol = qd.float(), 1.5e-2",
                 "src, tol = qkv, 1e-5", "assert (a[i, :L] - bb[i, :L]).abs().max().item() < 2e-6",
                 "assert e_ref < 1.5e-2, e_ref", "assert e_pair < 2e-3, e_pair", "assert e16 < 3e-3 and eb < 2e-2, (e16, eb)",
                 "assert e_ref < 1e-2, (e_ref, e_two_ref)", "assert e_ref < 2.0 * e_two_ref + 1e-4, (e_ref, e_two_ref)",
                 "assert e_two < 5e-3, e_two"):
        assert line in text, line
    assert fi.ATT_TOL == {"f32": 1e-5, "bf16 legacy": 1e-2, "bf16": 1.5e-2, "f16s": 1e-5, "f32->f16s": 1e-5} and fi.F16S_VS_F32 == 2e-6
    assert fi.CX_TOL == {"bf16": {"e_ref": 1.5e-2, "e_pair": 2e-3}, "f16": {"e_ref": 3e-3}} and fi.TAIL_TOL == {"e_ref": 1e-2, "e_two": 5e-3}


# ------------------------------------------------------------------------------------------------------- ConvNeXt block
def test_block_table():
    for c in fi.BLOCK_CASES:
        assert c["B"] * c["T"] >= 2 * fi.CX_BM + 1 or c["T"] >= 100, c
    assert {c["B"] * c["T"] % 128 for c in fi.BLOCK_CASES} >= {1, 31, 32, 33, 127}
    assert {c["I"] for c in fi.BLOCK_CASES} == set(fi.CX_I) and len(fi.BLOCK_CASES) == 22
    assert fi.block_interior(32, 384, 128) and not fi.block_interior(0, 384, 128) and not fi.block_interior(96, 384, 128)
    assert not fi.block_interior(352, 384, 128)           # f0w + 35 >= M
    # T = 128: the border is the tile border, and all three halo rows of the neighbour tile are another utterance's
    assert {"border-at-tile-edge", "border-at-wave-edge", "border%4=0"} <= fi.block_branches(3, 128, 256, None)
    t = fi.block_tiles(2, 300, (100, 130))
    assert [need for _, need, _, _ in t] == [True, False, True, True, False] and t[2][2:] == ([0, 1], [1])
    assert fi.block_tiles(2, 128, (128, 0))[1][1] is False and fi.block_tiles(2, 128, (128, 0), "limit<=")[1][1] is True
    assert fi.block_tiles(8, 40, (0, 0, 0, 5, 0, 0, 40, 40))[0][2:] == ([0, 1, 2, 3], [3])


@pytest.mark.parametrize("case", fi.BLOCK_CASES, ids=lambda c: f"B{c['B']}-T{c['T']}")
def test_block_reference_and_walk(case):
    """block_ref is F.conv1d + F.layer_norm + F.gelu as test_convnext_block_fused writes it; the walk without a fault equals it
    on every row of a tile that computes and passes the criteria"""
    B, T, I, lim = case["B"], case["T"], case["I"], case["t_limit"]
    t = fi.block_input(B, T, I)
    for operands in fi.CX_OPERANDS:
        w1, w2 = fi.block_weights(t, operands)
        x0 = t["x"].double()
        conv = F.conv1d(x0.transpose(1, 2), t["w7"].double().T.unsqueeze(1), t["db"].double(), padding=3, groups=fi.CX_C).transpose(1, 2)
        yn = F.layer_norm(conv, (fi.CX_C,), t["lw"].double(), t["lb"].double(), 1e-6)
        want = x0 + t["gam"].double() * (F.gelu(yn @ w1.T + t["b1"].double()) @ w2.T + t["b2"].double())
        ref = fi.block_ref(B, T, I, operands)
        assert float((ref - want.reshape(-1, fi.CX_C)).abs().max()) < 1e-10
    out, done = fi.block_walk(B, T, I, lim, "bf16")
    assert done == [tile for tile, need, _, _ in fi.block_tiles(B, T, lim) if need]
    computed = ~fi.block_skipped_rows(B, T, lim)
    assert float((out - ref_bf16(B, T, I))[computed].abs().max()) < 1e-10
    assert fi.block_criteria(out, B, T, I, lim, "bf16") == []
    if lim is not None:
        rows = fi.block_check_rows(B, T, lim)
        assert bool(rows.any()) and not bool((rows & ~computed).any())


def ref_bf16(B, T, I):
    return fi.block_ref(B, T, I, "bf16")


@pytest.mark.parametrize("fault", sorted(fi.BLOCK_FAULTS))
def test_block_fault_is_caught_by_the_case_named_for_its_branch(fault):
    branch = fi.BLOCK_FAULTS[fault][1]
    caught = {}
    for c in fi.BLOCK_CASES:
        B, T, I, lim = c["B"], c["T"], c["I"], c["t_limit"]
        if branch in fi.block_branches(B, T, I, lim):
            caught[(B, T)] = fi.block_criteria(fi.block_walk(B, T, I, lim, "bf16", fault)[0], B, T, I, lim, "bf16")
    want = "skipped-tiles-left-alone" if fault == "limit<=" else "values"
    assert caught and any(want in v for v in caught.values()), (fault, branch, caught)
    if fault == "beyond-M-last-row":        # (with t_limit the last rows may lie in a skipped tile, or beyond what is checked)
        caught = {k: v for k, v in caught.items() if next(c for c in fi.BLOCK_CASES if (c["B"], c["T"]) == k)["t_limit"] is None}
    assert all(want in v for v in caught.values()), (fault, branch, caught)


# ----------------------------------------------------------------------------------------------------------- layer tail
def test_tail_table():
    assert fi.TAIL_M == (1, 63, 64, 65, 129) and fi.TAIL_F == 256
    t = fi.tail_input(65)
    assert t["x"].shape == (65, 768) and t["w1"].dtype == torch.bfloat16 and fi.tail_ref(65, True).shape == (65, 768)


# ------------------------------------------------------------------------------------------- what the launchers refuse
def test_attention_launchers_refuse_65536_utterances():
    """SWC_CHECK_ARG runs before any launch, so this needs no device: with T == 0 an accepted call returns SWC_OK without
    touching a pointer, a refused one returns -1 and leaves its message"""
    from simwhisper_codec_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    p = C.c_void_p(0x10000)
    assert lib.swc_attention(p, p, p, 65535, 0, 1, _lib.F32, None) == 0
    assert lib.swc_attention(p, p, p, 65536, 0, 1, _lib.F32, None) == -1 and b"grid" in lib.swc_last_error()
    assert lib.swc_attention(p, p, p, 65536, 0, 1, _lib.BF16, None) == -1
    assert lib.swc_attention_ex(p, p, p, 65535, 0, 1, _lib.F16S, None) == 0
    assert lib.swc_attention_ex(p, p, p, 65536, 0, 1, _lib.F16S, None) == -1
    for dt in (_lib.BF16, _lib.F16S):
        assert lib.swc_attention16(p, p, p, 65535, 0, 1, dt, None, None) == 0
        assert lib.swc_attention16(p, p, p, 65536, 0, 1, dt, None, None) == -1 and b"bad B/T/H" in lib.swc_last_error()
    with pytest.raises(_lib.SwcError):
        _lib.check(lib.swc_attention16(p, p, p, 65536, 0, 1, _lib.BF16, None, None), "swc_attention16")


def test_header_states_the_length_clamp():
    with open(os.path.join(ROOT, "include", "swc.h")) as f:
        assert "lens[b] outside [0, T] is clamped to that range" in f.read()
