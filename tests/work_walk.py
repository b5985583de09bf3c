"""The work-walk case table shared by tests/test_work_walk_cpu.py and tests/test_work_walk_gpu.py.

swc_gemm and swc_dwconv7_ln keep a fixed number of workgroups resident ("slots") and let each one walk several work items
(output tiles / strips of frames) once there are more items than slots.  Every case below names the regime it is there for
as the fields swc_gemm_plan / swc_dwconv7_ln_plan must report for it; the CPU test asserts that each case still reports
them (a retuned chooser must not move the table out of its regimes unnoticed) and that the table covers every regime
(test_gemm_table_covers_the_walk_regimes, test_dwconv_table_covers_the_walk_regimes); the GPU test runs every case.
The shapes are the smallest found by a search over the plan functions that reach the regime with ragged M and N tails; K is as small as the case allows (the shapes are wide, not deep).

Nothing here needs a GPU: the plan functions are host arithmetic.
"""
import torch

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16s": torch.float16, "fp8": torch.float8_e4m3fn}
K_SLICE = {"f32": 32, "bf16": 64, "f16s": 32, "fp8": 128}   # logical elements of K per LDS slice (checked against the plan)
FAKE = 0x10000                                              # an aligned non-null pointer the plan functions never follow


def conv_geometry(conv):
    """(taps, dil, stride, pad, t_in, t_out) of a conv case: `conv` is (taps, dil, stride, B, T)"""
    taps, dil, stride, B, T = conv
    pad = dil * (taps - 1) // 2
    t_out = (T + 2 * pad - dil * (taps - 1) - 1) // stride + 1
    return taps, dil, stride, pad, T, t_out


def G(name, a, c, M, N, K, *, tile, waves, walk, band=1, conv=None, bias=True, gelu=False, gamma=False, residual=False,
      inplace=False, unaligned=False, ldc_pad=0, out_scale=1.0, split="rows"):
    """One swc_gemm case.  a / c: operand / output format.  tile: rows per tile; walk: "plus1" (tiles == slots + 1: exactly one
    workgroup walks 2), "mixed" (a tile count with ntiles % 8 != 0 between 2 and 3 times the slots: walks of 2 and 3), "deep"
    (some walk of 4 or more), "two" (slots < tiles <= 2 * slots: the most a 64-row geometry reaches).  conv: (taps, dil, stride,
    B, T) with M == B * t_out.  split: how the case is cut into one-tile-per-workgroup launches of the same kernel: "rows" (M, at
    tile-row multiples), "cols" (N, at tile-column multiples: the shapes of one row panel), or None where neither cut exists."""
    d = dict(name=name, a=a, c=c, M=M, N=N, K=K, tile=tile, waves=waves, walk=walk, band=band, conv=conv, bias=bias, gelu=gelu,
             gamma=gamma, residual=residual or inplace, inplace=inplace, unaligned=unaligned, ldc_pad=ldc_pad,
             out_scale=out_scale, split=split)
    if conv is not None:
        assert M == conv[3] * conv_geometry(conv)[5], name
    return d


def gemm_args(case, M=None, N=None):
    """the swc_gemm_args of a case (or of its first M rows / N columns) with placeholder pointers: what the plan depends on"""
    from simwhisper_codec_amd import _lib
    a = _lib.GemmArgs()
    M = case["M"] if M is None else M
    N, K = case["N"] if N is None else N, case["K"]
    a.A = a.W = a.C = FAKE
    a.bias = FAKE + (4 if case["unaligned"] else 0) if case["bias"] else None
    a.gamma = FAKE + (4 if case["unaligned"] else 0) if case["gamma"] else None
    a.residual = FAKE if case["residual"] else None
    a.M, a.N, a.K = M, N, K
    if case["conv"] is None:
        a.taps, a.dil, a.stride, a.pad, a.t_in, a.t_out = 1, 1, 1, 0, M, M
        a.lda, a.ldw = K, K
    else:
        a.taps, a.dil, a.stride, a.pad, a.t_in, a.t_out = conv_geometry(case["conv"])
        a.lda, a.ldw = K, a.taps * K
    a.ldc = case["N"] + case["ldc_pad"]
    a.ldr = a.ldc if case["residual"] else 0
    code = {"f32": _lib.F32, "bf16": _lib.BF16, "f16s": _lib.F16S, "fp8": _lib.FP8}
    a.a_dtype, a.c_dtype = code[case["a"]], code[case["c"]]
    a.act = _lib.ACT_GELU if case["gelu"] else _lib.ACT_NONE
    a.alpha, a.out_scale = 1.0, case["out_scale"]
    return a


def gemm_plan(case, M=None, N=None):
    from simwhisper_codec_amd import ops
    return ops.gemm_plan(gemm_args(case, M, N))


def max_walk(plan):
    """the longest walk of a launch: tiles are cut into 8 per-XCD chunks (the first ntiles % 8 one longer), the grid / 8
    workgroups of an XCD stride through their chunk"""
    ntiles = plan["n_tiles_m"] * plan["n_tiles_n"]
    longest = 0
    for xcd in range(8):
        gw = (plan["grid"] - xcd + 7) >> 3
        chunk = ntiles // 8 + (1 if xcd < ntiles % 8 else 0)
        if gw:
            longest = max(longest, -(-chunk // gw))
    return longest


def walk_lengths(plan):
    """the set of walk lengths over all workgroups of a launch"""
    ntiles = plan["n_tiles_m"] * plan["n_tiles_n"]
    out = set()
    for wg in range(plan["grid"]):
        xcd, tl = wg & 7, wg >> 3
        gw = (plan["grid"] - xcd + 7) >> 3
        chunk = ntiles // 8 + (1 if xcd < ntiles % 8 else 0)
        out.add(len(range(tl, chunk, gw)))
    return out


def walk_class(plan):
    ntiles, slots = plan["n_tiles_m"] * plan["n_tiles_n"], plan["slots"]
    if ntiles <= slots:
        return "none"
    if ntiles == slots + 1:
        return "plus1"
    if max_walk(plan) >= 4:
        return "deep"
    if 2 * slots < ntiles < 3 * slots and ntiles % 8 != 0:
        return "mixed"
    return "two" if ntiles <= 2 * slots else "other"


SAME_KERNEL = ("a_dtype", "tile_m", "tile_n", "waves", "plain", "act_body", "k_slice", "k_slices")


def gemm_chunks(case):
    """Cut a case into launches [(row0, rows, col0, cols), ..] that swc_gemm runs on the SAME kernel (tile, waves, staging,
    epilogue body) with one tile per workgroup (grid == tiles): the M rows at tile-row multiples (split "rows"; conv cases: at
    whole utterances), or the N columns at tile-column multiples (split "cols").  Largest chunks first, backtracking; None when
    no such cut exists."""
    if case["split"] is None:                                  # neither cut is claimed to exist: look for both
        return gemm_chunks(dict(case, split="rows")) or gemm_chunks(dict(case, split="cols"))
    full = gemm_plan(case)
    rows_cut = case["split"] == "rows"
    # conv cases are cut at whole utterances instead (a launch addresses rows as utterance * t_in + frame): an output element's
    # k-sum does not depend on where its row sits inside a tile, only on the kernel
    if rows_cut:
        unit, total = full["tile_m"] if case["conv"] is None else conv_geometry(case["conv"])[5], case["M"]
    else:
        unit, total = full["tile_n"], case["N"]

    def fits(n):
        p = gemm_plan(case, n, None) if rows_cut else gemm_plan(case, None, n)
        return all(p[k] == full[k] for k in SAME_KERNEL) and p["grid"] == p["n_tiles_m"] * p["n_tiles_n"] and \
            p["n_tiles_n" if rows_cut else "n_tiles_m"] == full["n_tiles_n" if rows_cut else "n_tiles_m"]

    dead = set()

    def cut(at):
        if at == total:
            return []
        if at in dead:
            return None
        left = total - at
        # candidates: the whole rest, then multiples of `unit`, largest first
        for n in [left] + [u * unit for u in range(min((left - 1) // unit, full["slots"]), 0, -1)]:
            if fits(n):
                rest = cut(at + n)
                if rest is not None:
                    return [(at, n)] + rest
        dead.add(at)
        return None

    parts = cut(0)
    if parts is None:
        return None
    return [(at, n, 0, case["N"]) if rows_cut else (0, case["M"], at, n) for at, n in parts]


# ------------------------------------------------------------------------------------------------------------ swc_gemm cases
# Regimes the chooser cannot reach (test_regimes_the_chooser_cannot_reach probes them through the plan, so a retuned chooser
# that opens one fails it):
#  * tiles == slots + 1 on the 256-row 8-wave tile.  257 is prime: 257 x 1 tiles have N <= 256 and 342 tiles of 192 rows are
#    cheaper; 1 x 257 tiles have M <= 256 and one row panel of 128 or 192 rows is cheaper.  The 192- and 128-row tiles reach
#    it as 1 x 257 (M <= 192 / M <= 128, N > 65536): one row panel, so those cases are cut along N;
#  * more than 2 * slots tiles on the 64-row tile (it needs fewer than 384 tiles of 128 x 128), and 64-row tiles for f32 / fp8.
_EPI = dict(gelu=True, gamma=True, residual=True)
GEMM_CASES = [
    # ---- 8-wave tiles (256 columns, 256 slots)
    G("bf16-256-mixed-epi", "bf16", "f32", 81957, 352, 64, tile=256, waves=8, walk="mixed", **_EPI),
    G("fp8-256-deep-fp8out", "fp8", "fp8", 122917, 352, 128, tile=256, waves=8, walk="deep", gelu=True, out_scale=16.0),
    G("f16s-256-band4-m1-f16sout", "f16s", "f16s", 14373, 2912, 64, tile=256, waves=8, walk="mixed", band=4, out_scale=64.0),
    G("bf16-256-band4-m3-ktail", "bf16", "f32", 7717, 3168, 72, tile=256, waves=8, walk="two", band=4, residual=True),
    G("bf16-192-mixed-k5-bf16out", "bf16", "bf16", 65701, 352, 320, tile=192, waves=8, walk="mixed", gelu=True),
    G("fp8-192-band4-m2-inplace", "fp8", "f32", 9445, 3424, 256, tile=192, waves=8, walk="mixed", band=4, inplace=True),
    G("f16s-192-deep-direct", "f16s", "f32", 98341, 352, 32, tile=192, waves=8, walk="deep", unaligned=True, **_EPI),
    G("bf16-128w8-deep-ldc", "bf16", "f32", 73765, 352, 128, tile=128, waves=8, walk="deep", ldc_pad=24, residual=True),
    G("fp8-128w8-mixed-ktail-bf16out", "fp8", "bf16", 10789, 2144, 144, tile=128, waves=8, walk="mixed"),
    G("f16s-128w8-band4-m3-deep", "f16s", "f16s", 6412, 5024, 64, tile=128, waves=8, walk="deep", band=4, gelu=True,
      out_scale=64.0),
    # one row panel x 257 column tiles: tiles == slots + 1 (band 4, one row per band), cut along N.  The 192-row one has no cut
    # (split=None): one row panel cannot be cut along M, and 129 < M <= 192 stays on 192 rows only above 128 column tiles (up
    # to 128, 128-row tiles fill the chip in one round and are cheaper), so 257 column tiles are no sum of one-round launches
    G("fp8-192-plus1-1x257", "fp8", "f32", 150, 65552, 128, tile=192, waves=8, walk="plus1", band=4, residual=True,
      split=None),
    G("f16s-128w8-plus1-1x257", "f16s", "f16s", 100, 65568, 64, tile=128, waves=8, walk="plus1", band=4, gelu=True,
      out_scale=64.0, split="cols"),
    G("bf16-128w8-plus1-1x257", "bf16", "f32", 120, 65544, 64, tile=128, waves=8, walk="plus1", band=4, unaligned=True,
      split="cols", **_EPI),
    # ---- the 4-wave 128 x 128 tile (512 slots)
    G("f32-128-plus1-conv7d3", "f32", "f32", 65600, 96, 32, tile=128, waves=4, walk="plus1", conv=(7, 3, 1, 16, 4100)),
    G("bf16-128-mixed-conv3s2", "bf16", "f32", 147528, 96, 64, tile=128, waves=4, walk="mixed", conv=(3, 1, 2, 36, 8195),
      residual=True),
    G("f32-128-band4-m1-k5-epi", "f32", "f32", 10277, 1632, 160, tile=128, waves=4, walk="mixed", band=4, **_EPI),
    G("f32-128-deep-ktail", "f32", "f32", 196645, 96, 36, tile=128, waves=4, walk="deep"),
    G("f32-128-band4-m2-direct-ldc", "f32", "f32", 4773, 1760, 32, tile=128, waves=4, walk="two", band=4, unaligned=True,
      ldc_pad=8, **_EPI),
    G("bf16-128-plus1-bf16out", "bf16", "bf16", 65573, 96, 64, tile=128, waves=4, walk="plus1"),
    G("fp8-128-plus1-fp8out", "fp8", "fp8", 65573, 96, 128, tile=128, waves=4, walk="plus1", out_scale=16.0),
    G("fp8-128-deep-k2", "fp8", "f32", 196645, 96, 256, tile=128, waves=4, walk="deep", residual=True),
    G("f16s-128-mixed-f16sout", "f16s", "f16s", 131109, 96, 64, tile=128, waves=4, walk="mixed", gelu=True, residual=True,
      out_scale=64.0),
    G("f16s-128-plus1-inplace", "f16s", "f32", 65573, 96, 32, tile=128, waves=4, walk="plus1", inplace=True),
    # ---- the 64-row tile (half_rows; at most 2 tiles per workgroup)
    G("bf16-64-plus1", "bf16", "f32", 32805, 96, 64, tile=64, waves=4, walk="plus1", **_EPI),
    G("f16s-64-two-f16sout", "f16s", "f16s", 32869, 96, 64, tile=64, waves=4, walk="two", out_scale=64.0),
]
PLUS1_8WAVE = {256: False, 192: True, 128: True}   # 8-wave tile rows: can tiles == slots + 1 be reached (any operand mode)

# ------------------------------------------------------------------------------------------------------ swc_dwconv7_ln cases
def D(name, C_, out, B, T, *, S, full, slots, per, partial_last=False, straddle=True):
    """One swc_dwconv7_ln case: the plan must report strips of S frames, FULL == full, `slots` resident workgroups and `per`
    strips per workgroup.  Every case has T % S != 0.  straddle: the strips per utterance are no multiple of `per`, so some walks
    run from the last strip of one utterance into the first of the next.  partial_last: the last walk is shorter than `per`."""
    return dict(name=name, C=C_, out=out, B=B, T=T, S=S, full=full, slots=slots, per=per, partial_last=partial_last,
                straddle=straddle)


DW_CASES = [
    D("c64-f32-per2", 64, "f32", 3, 5445, S=32, full=0, slots=512, per=2, partial_last=True),
    D("c64-bf16-per3", 64, "bf16", 5, 6533, S=32, full=0, slots=512, per=3, partial_last=True),
    D("c256-f32-per3", 256, "f32", 4, 8197, S=32, full=1, slots=512, per=3, partial_last=True),
    D("c256-bf16-per2", 256, "bf16", 6, 2757, S=32, full=1, slots=512, per=2),
    D("c260-f32-per2", 260, "f32", 5, 1637, S=16, full=0, slots=512, per=2, partial_last=True),
    D("c260-bf16-per3", 260, "bf16", 3, 5477, S=16, full=0, slots=512, per=3),
    D("c512-f32-per2", 512, "f32", 3, 2725, S=16, full=1, slots=512, per=2, partial_last=True),
    D("c512-f32-per2-even", 512, "f32", 3, 2750, S=16, full=1, slots=512, per=2, straddle=False),   # 516 strips on 512 slots, 172 per utterance
    D("c512-bf16-per3", 512, "bf16", 4, 4101, S=16, full=1, slots=512, per=3, partial_last=True),
    # C = 768: (16 + 6) rows are 66 KiB of LDS, two workgroups still fit a CU: 512 slots.  C = 1024 (88 KiB): one, 256 slots
    D("c768-f32-per3", 768, "f32", 6, 2741, S=16, full=0, slots=512, per=3),
    D("c768-bf16-per2", 768, "bf16", 5, 1637, S=16, full=0, slots=512, per=2, partial_last=True),
    D("c1024-f32-per2", 1024, "f32", 5, 837, S=16, full=1, slots=256, per=2, partial_last=True),
    D("c1024-bf16-per3", 1024, "bf16", 3, 2741, S=16, full=1, slots=256, per=3),
]


def dw_plan(case, B=None):
    from simwhisper_codec_amd import ops
    return ops.dwconv7_ln_plan(case["B"] if B is None else B, case["T"], case["C"], DT[case["out"]])


def dw_straddles(plan):
    """number of walks that run from one utterance into the next"""
    n = 0
    for first in range(0, plan["nstrips"], plan["per"]):
        last = min(first + plan["per"], plan["nstrips"]) - 1
        n += first // plan["nst"] != last // plan["nst"]
    return n


def dw_groups(case):
    """utterance groups [(b0, nb), ..] that swc_dwconv7_ln runs with one strip per workgroup (per == 1), or None"""
    groups, b0 = [], 0
    while b0 < case["B"]:
        nb = next((n for n in range(case["B"] - b0, 0, -1) if dw_plan(case, n)["per"] == 1), None)
        if nb is None:
            return None
        groups.append((b0, nb))
        b0 += nb
    return groups
