"""tests/sat_sites.py against the kernel sources (no GPU): every sat_commit in simwhisper_codec_amd/csrc/ is claimed by a table
entry, every entry's site still exists, every entry has a GPU test that exists, and every function that converts to split-f16 /
fp8 either commits or is listed as bounded by construction.  A producer added later cannot go untested silently."""
import os
import re

import sat_sites
from common import ROOT

CSRC = os.path.join(ROOT, "simwhisper_codec_amd", "csrc")
_FUNC = re.compile(r"^(?!#|//|\}|typedef|using|struct|namespace|template\b).*?\b(?:void|int|float|unsigned|bool|long)\s*\*?\s+\*?(\w+)\s*\(")
_COMMIT = re.compile(r"\bsat_commit(?:_out\s*<[^>]*>)?\s*\(")
_CONVERT = re.compile(r"\b(?:f16s_store4|f16s_split2?|fp8_pack4|store_row4\s*<[^>]*>|pack2_f16)\s*\(")


def _code(line):
    return line.split("//", 1)[0]


def scan(text):
    """-> (commits, converts): lists of (enclosing function, n-th such line inside it, stripped line, line number) over the text of one file.
    The enclosing function is the last definition that started in column 0 (lambdas and nested blocks are indented)."""
    func, commits, converts, n = None, [], [], {}
    for no, raw in enumerate(text.splitlines(), 1):
        line = _code(raw)
        m = _FUNC.match(line) if line[:1] not in (" ", "\t", "") else None
        if m:
            func = m.group(1)
        if m and re.search(r"\b(?:sat_commit(?:_out)?|f16s_store4|f16s_split2?|fp8_pack4|store_row4|pack2_f16)\s*\(", line) and \
                m.group(1) in ("sat_commit", "sat_commit_out", "f16s_store4", "f16s_split", "f16s_split2", "fp8_pack4", "store_row4", "pack2_f16"):
            continue                                  # the helper's own definition line
        for rx, out, kind in ((_COMMIT, commits, "c"), (_CONVERT, converts, "v")):
            if rx.search(line):
                k = n.get((func, kind), 0)
                n[(func, kind)] = k + 1
                out.append((func, k, line.strip(), no))
    return commits, converts


def scan_tree(root=CSRC):
    res = {}
    for name in sorted(os.listdir(root)):
        if name.endswith((".hip", ".h", ".cpp", ".c")):
            res[name] = scan(open(os.path.join(root, name)).read())
    return res


def check(tree):
    """the list of disagreements between the table and the scanned sources (empty: they agree)"""
    bad = []
    claimed = {(e["file"], e["func"], e["nth"]): e for e in sat_sites.COUNTED}
    if len(claimed) != len(sat_sites.COUNTED):
        bad.append("two COUNTED entries claim one site")
    found = {}
    for file, (commits, _) in tree.items():
        for func, k, line, _ in commits:
            if (file, func) in sat_sites.HELPERS:
                continue
            found[(file, func, k)] = line
            if (file, func, k) not in claimed:
                bad.append(f"unclaimed sat_commit: {file}, {func}, commit #{k}: {line}")
    for key, e in claimed.items():
        if key not in found:
            bad.append(f"{e['id']}: no commit #{e['nth']} in {e['func']} of {e['file']} any more")
        elif e["text"] not in found[key]:
            bad.append(f"{e['id']}: the line reads `{found[key]}`, the table says `{e['text']}`")
        if e["unreachable"]:
            # a commit that is never instantiated: it names the test of THIS module that pins why, and claims no GPU case
            if e["gpu"] or not callable(globals().get(e["unreachable"])) or not e["unreachable"].startswith("test_"):
                bad.append(f"{e['id']}: unreachable entries list no GPU case and name the CPU test that pins the reason")
        elif not e["gpu"] or not e["paths"]:
            bad.append(f"{e['id']}: no GPU case attached")
    counted_funcs = {(e["file"], e["func"]) for e in sat_sites.COUNTED}
    bounded = {}
    for e in sat_sites.BOUNDED:
        bounded.setdefault((e["file"], e["func"]), []).append(e)
        lines = [l for f, _, l, _ in tree.get(e["file"], ([], []))[1] if f == e["func"]]
        if not any(e["text"] in l for l in lines):
            bad.append(f"{e['id']}: no converting line `{e['text']}` in {e['func']} of {e['file']} any more")
        if not e["reason"]:
            bad.append(f"{e['id']}: no reason")
    for file, (_, converts) in tree.items():
        for func, k, line, _ in converts:
            if (file, None) in sat_sites.CONVERTERS or (file, func) in sat_sites.CONVERTERS:
                continue
            if (file, func) in bounded:
                if (file, func) in counted_funcs or any(e["text"] in line for e in bounded[(file, func)]):
                    continue
                bad.append(f"untracked conversion that no BOUNDED entry explains: {file}, {func}: {line}")
            elif (file, func) not in counted_funcs:
                bad.append(f"converting function without a commit and without a BOUNDED entry: {file}, {func}: {line}")
    return bad


def test_table_matches_the_sources():
    tree = scan_tree()
    n = sum(len(c) for c, _ in tree.values())
    assert n >= len(sat_sites.COUNTED) + 2, n            # the scan sees the commits (sat_commit_out's two lines included)
    assert check(tree) == []


def test_tracked_conversions_feed_the_commit():
    """in a counted function every converting line passes the running maximum (`amax` / `amax8` / `am`) on, or is a listed zero
    store.  Each site is read at its own line (the statement may run over several lines)."""
    tree = scan_tree()
    counted_funcs = {(e["file"], e["func"]) for e in sat_sites.COUNTED if not e["unreachable"]}
    checked = set()
    for file, (_, converts) in tree.items():
        src = open(os.path.join(CSRC, file)).read().splitlines()
        for func, k, line, no in converts:
            if (file, func) not in counted_funcs:
                continue
            zero = any(e["file"] == file and e["func"] == func and e["text"] in line for e in sat_sites.BOUNDED)
            rest = "\n".join([_code(src[no - 1])[_code(src[no - 1]).index(_CONVERT.search(_code(src[no - 1])).group(0)):]] +
                             [_code(l) for l in src[no:no + 6]])
            stmt = rest[:rest.index(");") + 1]              # from the converting call to the end of its statement
            assert zero or re.search(r"\b(?:amax8?|am)\)$", stmt), (file, func, no, line)   # (am: folded into amax8 for live tokens)
            checked.add((file, func))
    # the snake converts inside its `emit` lambda (indented: it belongs to snake_aa_kernel here) and the direct GEMM epilogue in three bodies
    assert {("swc_pointwise.hip", "snake_aa_kernel"), ("swc_gemm.hip", "gemm_epilogue_direct"), ("swc_mlp.hip", "mlp_block_kernel")} <= checked


def test_every_gpu_case_exists():
    for ref in sat_sites.gpu_cases():
        file, name = ref.split("::")
        src = open(os.path.join(ROOT, "tests", file)).read()
        assert re.search(rf"^def {name}\(", src, flags=re.M), ref
        assert "pytest.mark.gpu" in src, ref


def test_the_slab_epilogue_admits_f32_outputs_only():
    """gemm.slab.fp8 (marked unreachable in tests/sat_sites.py) is compiled out by this gate; fp8 and split-f16 outputs take the
    direct epilogue in every geometry"""
    assert [e["unreachable"] for e in sat_sites.COUNTED if e["id"] == "gemm.slab.fp8"] == ["test_the_slab_epilogue_admits_f32_outputs_only"]
    src = open(os.path.join(CSRC, "swc_gemm.hip")).read()
    assert src.count(sat_sites.SLAB_GATE) == 1
    body = src[src.index(sat_sites.SLAB_GATE):]
    assert body.index("gemm_epilogue_slab<OutT, MT, true>") < body.index("gemm_epilogue_direct<OutT, MT, ACT>")


def test_the_check_notices_a_new_or_a_lost_site():
    """the scan itself: a commit added to a kernel, a commit removed, and a new converting kernel are each reported"""
    tree = scan_tree()
    name = "swc_pointwise.hip"
    text = open(os.path.join(CSRC, name)).read()
    # (a) one more commit in an existing kernel
    added = text.replace("    if (i < n) y[i] = f32_to_bf16(x[i]);", "    if (i < n) y[i] = f32_to_bf16(x[i]);\n    sat_commit(sat, 0, 1.f, SWC_F16S_LIMIT);", 1)
    assert added != text
    t2 = dict(tree)
    t2[name] = scan(added)
    assert any("unclaimed sat_commit" in b and "cast_bf16_kernel" in b for b in check(t2))
    # (b) a commit lost
    lost = text.replace("    sat_commit(sat, 0, amax, SWC_F16S_LIMIT);\n", "", 1)
    assert lost != text
    t3 = dict(tree)
    t3[name] = scan(lost)
    assert any(b.startswith("cast.f16s: no commit") for b in check(t3))
    # (c) a new kernel that converts without tracking
    new = text + "\n__global__ void new_producer_kernel(const float* x, unsigned short* y) {\n    f16s_store4(y, 0, x[0], x[1], x[2], x[3]);\n}\n"
    t4 = dict(tree)
    t4[name] = scan(new)
    assert any("new_producer_kernel" in b for b in check(t4))
