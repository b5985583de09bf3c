"""swc_subdtw and swc_cmvn on the GPU against the restatement of include/swc_subdtw.h (tests/subdtw_ref.py): cost, N, start, end,
status, patches and score bit for bit over patch lengths round the wave and strip sizes, reference lengths round the LDS ring's
refill, feature counts and five step sets; the patch geometry, the median, the whole-query form, ties, planted truths, the key
bound at the extremes; NaN / Inf and padding; bit independence of everything that is not the pair; the memory contract; the
normalisation against its float64 reference; metrics.warpq end to end and the wiring down to the tool."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import poison  # noqa: E402
import subdtw_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

OUTPUTS = ("cost", "info", "score", "patches", "exps")
DTYPES = {"cost": torch.int64, "info": torch.int32, "score": torch.float64, "patches": torch.int32, "exps": torch.int32}
STEP_SETS = (((1, 1), (1, 0), (0, 1)), ((1, 0), (0, 3), (1, 3)), ((1, 1), (3, 2), (1, 3)), ((1, 1), (2, 1), (1, 2)), ((1, 1),))
FAST = STEP_SETS[3]          # no step with di == 0: the reference is vectorised over a whole row
LENGTHS = (1, 2, 63, 64, 65, 100, 255, 256)
REF_LENGTHS = (1, 2, 3, 255, 256, 257, 511, 513)
TOP = np.float32(1.9999999)  # the largest f32 below 2: q = 8191
_CACHE = {}


def device():
    return torch.device("cuda", torch.cuda.current_device())


def make_pair(Tq, Ty, D, seed, kind=0):
    """kind 0: q = a stretch of y (where it fits) played along a wobbling time axis, plus noise; kind 1: features in {-1, 0, 1}
    (equal costs everywhere: the tie rules decide); kind 2: all zero"""
    key = ("pair", Tq, Ty, D, seed, kind)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        if kind == 2:
            q, y = np.zeros((Tq, D), np.float32), np.zeros((Ty, D), np.float32)
        elif kind == 1:
            q, y = rng.integers(-1, 2, (Tq, D)).astype(np.float32), rng.integers(-1, 2, (Ty, D)).astype(np.float32)
        else:
            y = (np.cumsum(rng.standard_normal((Ty, D)), axis=0) * 0.37).astype(np.float32)
            if Ty:
                t = np.linspace(0.0, Ty - 1, Tq) * 0.6 + 0.2 * Ty + 2.0 * np.sin(np.arange(Tq) / 7.0 + seed)
                q = (y[np.clip(np.rint(t).astype(int), 0, Ty - 1)] + 0.05 * rng.standard_normal((Tq, D))).astype(np.float32)
            else:
                q = rng.standard_normal((Tq, D)).astype(np.float32)
        _CACHE[key] = (q, y)
    return _CACHE[key]


def reference(q, y, Lp, Sp, steps):
    key = ("ref", q.tobytes(), y.tobytes(), q.shape, y.shape, Lp, Sp, tuple(steps))
    if key not in _CACHE:
        _CACHE[key] = ref.subdtw(q, y, Lp, Sp, steps)
    return _CACHE[key]


def run(pairs, Lp, Sp, steps, want=OUTPUTS, fill="nan", ldf=None, tmax_q=None, tmax_y=None, ldp=None, pad=float("nan")):
    """one swc_subdtw call on guarded, pre-filled outputs and workspace -> dict of host tensors for every output plus "before"
    (the fill of every output).  The feature matrices are [B][Tmax][ldf] with `pad` in every padding column and frame.  Outputs
    that were not asked for must keep their fill; nothing may be written outside the windows."""
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    dev = device()
    B, D = len(pairs), pairs[0][0].shape[1]
    tq, ty = [len(q) for q, _ in pairs], [len(y) for _, y in pairs]
    tmax_q = max(tq) if tmax_q is None else tmax_q
    tmax_y = max(ty) if tmax_y is None else tmax_y
    ldf = D if ldf is None else ldf
    hq, hy = np.full((B, max(tmax_q, 1), ldf), pad, np.float32), np.full((B, max(tmax_y, 1), ldf), pad, np.float32)
    for b, (q, y) in enumerate(pairs):
        hq[b, :min(len(q), tmax_q), :D], hy[b, :min(len(y), tmax_y), :D] = q[:tmax_q], y[:tmax_y]   # a count beyond the bound stays in tq / ty
    qf, yf = torch.from_numpy(hq).to(dev), torch.from_numpy(hy).to(dev)
    counts = torch.tensor(tq + ty, dtype=torch.int32).to(dev)
    p_max = 1 if Lp == 0 else ref.patch_count(tmax_q, Lp, Sp)
    ldp = max(p_max, 1) if ldp is None else ldp
    need = ops.subdtw_workspace_bytes(B, tmax_q, tmax_y, Lp, Sp)
    shapes = {"cost": (B, ldp), "info": (B, ldp * 4), "score": (B, 1), "patches": (B, 2), "exps": (B, 1)}
    outs, checks = {}, []
    for name in OUTPUTS:
        outs[name], chk = poison.guarded(shapes[name], DTYPES[name], device=dev, band_rows=16)
        outs[name].zero_() if fill == "zero" else poison.fill_(outs[name], fill)
        checks.append(chk)
    before = {k: v.cpu().clone() for k, v in outs.items()}
    ws, check_w = poison.guarded((max(need // 256, 1), 256), torch.uint8, device=dev, band_rows=16)
    assert ws.is_contiguous() and ws.data_ptr() % 256 == 0 and need % 256 == 0
    ws.zero_() if fill == "zero" else poison.fill_(ws.view(torch.float32), fill)
    P = lambda t: C.c_void_p(t.data_ptr())
    arg = lambda name: P(outs[name]) if name in want else None
    flat = [v for s in steps for v in s]
    rc = lib.swc_subdtw(P(qf), P(yf), P(counts[:B]), P(counts[B:]), tmax_q, tmax_y, D, ldf, Lp, Sp, (C.c_int32 * len(flat))(*flat),
                        len(steps), arg("cost"), arg("info"), ldp, arg("score"), arg("patches"), arg("exps"), P(ws), need, B,
                        ops._stream())
    _lib.check(rc, "swc_subdtw")
    torch.cuda.synchronize()
    for chk in checks + [check_w]:
        chk()
    res = {k: v.cpu().clone() for k, v in outs.items()}
    res["info"], before["info"] = res["info"].reshape(B, ldp, 4), before["info"].reshape(B, ldp, 4)
    for name in OUTPUTS:
        if name not in want:
            assert poison.same_bits(res[name].reshape(-1), before[name].reshape(-1)), f"{name} was not asked for and changed"
    res["before"] = before
    return res


def compare(got, pairs, Lp, Sp, steps, tmax_q=None, tmax_y=None, want=OUTPUTS):
    """every wanted output of every pair against the reference, bit for bit; entries of patches a pair does not have keep their fill"""
    for b, (q, y) in enumerate(pairs):
        q = q[:tmax_q] if tmax_q is not None else q
        y = y[:tmax_y] if tmax_y is not None else y
        w = reference(q, y, Lp, Sp, steps)
        P = w["patches"][1]
        tag = (b, len(q), len(y), Lp, Sp, steps)
        written = P
        if w["query_status"] is not None:                       # the one entry a refused whole query writes
            written = 1
            if "cost" in want:
                assert int(got["cost"][b, 0]) == 0, tag
            if "info" in want:
                assert got["info"][b, 0].tolist() == [0, 0, 0, ref.ST_QUERY], tag
        else:
            if "cost" in want:
                assert got["cost"][b, :P].tolist() == w["cost"].tolist(), tag
            if "info" in want:
                assert got["info"][b, :P].tolist() == w["info"].tolist(), tag
        if "cost" in want:
            assert poison.same_bits(got["cost"][b, written:], got["before"]["cost"][b, written:]), tag
        if "info" in want:
            assert poison.same_bits(got["info"][b, written:], got["before"]["info"][b, written:]), tag
        if "score" in want:
            assert poison.same_bits(got["score"][b].reshape(1), torch.tensor([w["score"]], dtype=torch.float64)), (tag, got["score"][b], w["score"])
        if "patches" in want:
            assert tuple(got["patches"][b].tolist()) == w["patches"], tag
        if "exps" in want:
            assert int(got["exps"][b]) == w["e"], tag


# ---- swc_subdtw: the sweeps ----

def test_every_patch_length_against_every_reference_length():
    """the whole-query form, one pair per (L, Ty): every wave count of a workgroup, and the LDS ring's refill every 256 columns"""
    pairs = [make_pair(L, Ty, 13, 100 + i) for i, (L, Ty) in enumerate(itertools.product(LENGTHS, REF_LENGTHS))]
    compare(run(pairs, 0, 1, FAST), pairs, 0, 1, FAST)


SWEEP = ((1, 3), (2, 255), (63, 513), (64, 2), (65, 257), (100, 511), (255, 256), (256, 1))


@pytest.mark.parametrize("steps", STEP_SETS)
def test_every_step_set(steps):
    pairs = [make_pair(L, Ty, 13, 200 + i) for i, (L, Ty) in enumerate(SWEEP)]
    compare(run(pairs, 0, 1, steps), pairs, 0, 1, steps)


@pytest.mark.parametrize("D,steps", [(1, STEP_SETS[2]), (8, STEP_SETS[2]), (9, STEP_SETS[2]), (13, STEP_SETS[2]), (32, STEP_SETS[2]),
                                     (1, STEP_SETS[1]), (32, STEP_SETS[0])])
def test_every_feature_count(D, steps):
    big = steps == STEP_SETS[2]
    pairs = [make_pair(L, Ty, D, 300 + i, kind=i % 2) for i, (L, Ty) in enumerate(SWEEP if big else SWEEP[:3] + SWEEP[4:6])]
    compare(run(pairs, 0, 1, steps, ldf=D + 3), pairs, 0, 1, steps)


@pytest.mark.parametrize("steps", (STEP_SETS[0], STEP_SETS[1], FAST))
def test_patch_geometry_and_the_median(steps):
    """Lp = 20 every 7: P = 0 (Tq = L - 1), P = 1, a last patch that ends on the last frame (Tq = 27, 34, 41) and one frame short
    of it (26, 33), odd and even counts of ok patches; then a batch whose bound is larger than every pair"""
    pairs = [make_pair(Tq, 90 + 3 * i, 13, 400 + i) for i, Tq in enumerate((19, 20, 26, 27, 33, 34, 41, 48, 0))]
    assert [ref.patch_count(len(q), 20, 7) for q, _ in pairs] == [0, 1, 1, 2, 2, 3, 4, 5, 0]
    compare(run(pairs, 20, 7, steps), pairs, 20, 7, steps)
    compare(run(pairs, 20, 7, steps, tmax_q=60, tmax_y=130, ldf=16, ldp=9), pairs, 20, 7, steps)
    # counts beyond the bounds are clamped on the device
    compare(run(pairs, 20, 7, steps, tmax_q=30, tmax_y=95), pairs, 20, 7, steps, tmax_q=30, tmax_y=95)


def test_a_reference_too_short_for_the_steps_disturbs_nothing_else():
    steps = ((1, 3),)
    rng = np.random.default_rng(9)
    f = lambda T: rng.standard_normal((T, 8)).astype(np.float32)
    pairs = [(f(5), f(13)), (f(5), f(12)), (f(9), f(40)), (f(5), f(0)), (f(7), f(30))]
    got = run(pairs, 5, 2, steps)
    compare(got, pairs, 5, 2, steps)
    assert got["patches"].tolist() == [[1, 1], [0, 1], [3, 3], [0, 1], [2, 2]]
    assert got["info"][1, 0].tolist() == [0, 0, 0, ref.ST_UNREACHABLE] and torch.isnan(got["score"][1]) and torch.isnan(got["score"][3])
    # some patches of a pair reachable, some not, is impossible (every patch sees the same Ty); but with the symmetric set and
    # Ty = 1 every patch is reachable along column 0
    pairs = [(f(6), f(1))]
    compare(run(pairs, 3, 1, STEP_SETS[0]), pairs, 3, 1, STEP_SETS[0])


def test_the_whole_query_form_and_its_limits():
    rng = np.random.default_rng(10)
    f = lambda T: rng.standard_normal((T, 9)).astype(np.float32)
    pairs = [(f(0), f(20)), (f(1), f(20)), (f(256), f(300)), (f(257), f(20)), (f(30), f(0))]
    got = run(pairs, 0, 1, FAST)
    compare(got, pairs, 0, 1, FAST)
    assert got["patches"].tolist() == [[0, 0], [1, 1], [1, 1], [0, 0], [0, 1]]
    assert [int(v) for v in got["info"][:, 0, 3]] == [ref.ST_QUERY, 0, 0, ref.ST_QUERY, ref.ST_UNREACHABLE]


@pytest.mark.parametrize("steps", STEP_SETS)
def test_all_zero_features_every_tie(steps):
    pairs = [make_pair(Tq, Ty, 4, 0, kind=2) for Tq, Ty in ((12, 30), (7, 7), (30, 12))] + [make_pair(14, 40, 4, 3, kind=1)]
    got = run(pairs, 6, 2, steps)
    compare(got, pairs, 6, 2, steps)
    assert got["score"][0] == 0.0 and (got["cost"][0, :4] == 0).all()


def test_planted_truths():
    rng = np.random.default_rng(11)
    y = rng.standard_normal((300, 13)).astype(np.float32)
    cut = [(y[a:a + L].copy(), y) for a, L in ((0, 1), (0, 40), (130, 100), (44, 256), (299, 1))]
    got = run(cut, 0, 1, STEP_SETS[0])
    compare(got, cut, 0, 1, STEP_SETS[0])
    assert got["info"][:, 0].tolist() == [[1, 0, 0, 0], [40, 0, 39, 0], [100, 130, 229, 0], [256, 44, 299, 0], [1, 299, 299, 0]]
    assert (got["cost"][:, 0] == 0).all() and (got["score"] == 0.0).all()
    rep = np.repeat(y[50:150], [2 if t % 2 else 1 for t in range(100)], axis=0)
    got = run([(rep, y)], 0, 1, STEP_SETS[0])
    compare(got, [(rep, y)], 0, 1, STEP_SETS[0])
    assert got["info"][0, 0].tolist() == [150, 50, 149, 0] and int(got["cost"][0, 0]) == 0


def test_the_key_bound_at_the_extremes():
    """L = 256, Ty = 8192, D = 32, every feature at +-peak: every cost is the largest one, 91 * 16382 rounded down, and every key
    ties with its neighbours'.  The cheapest way down 255 rows is 127 steps (2, 1) and one of one row: 129 cells"""
    q, y = np.full((256, 32), TOP, np.float32), np.full((8192, 32), -TOP, np.float32)
    got = run([(q, y)], 0, 1, FAST)
    compare(got, [(q, y)], 0, 1, FAST)
    d = int(ref.root256(np.int64(32 * 16382 ** 2)))
    assert int(got["cost"][0, 0]) == 129 * d and int(got["info"][0, 0, 0]) == 129 and int(got["info"][0, 0, 3]) == 0 and d <= ref.D_MAX
    # and the longest paths: the single step (1, 0) ... is not a search; (1, 1), (0, 1) along a cheap last row
    q2 = np.concatenate([np.full((255, 32), TOP, np.float32), np.zeros((1, 32), np.float32)])
    y2 = np.concatenate([np.full((1000, 32), -TOP, np.float32), np.zeros((7192, 32), np.float32)])
    got = run([(q2, y2)], 0, 1, ((1, 1), (2, 1)))
    compare(got, [(q2, y2)], 0, 1, ((1, 1), (2, 1)))


def test_nan_and_inf_pairs_stay_alone_and_padding_is_never_read():
    pairs = [make_pair(45, 70, 13, 500 + i) for i in range(5)]
    for b, (side, v) in {1: (0, np.nan), 3: (1, np.inf)}.items():
        q, y = (a.copy() for a in pairs[b])
        (q if side == 0 else y)[7, 5] = v
        pairs[b] = (q, y)
    clean = run(pairs, 20, 10, STEP_SETS[1], pad=0.0)
    compare(clean, pairs, 20, 10, STEP_SETS[1])
    assert clean["patches"].tolist() == [[3, 3], [0, 3], [3, 3], [0, 3], [3, 3]]
    assert (clean["info"][1, :3, 3] == ref.ST_UNDEFINED).all() and torch.isnan(clean["score"][3])
    for pad in poison.PATTERNS:
        v = float("nan") if pad == "nan" else poison.BIG * 1e30
        got = run(pairs, 20, 10, STEP_SETS[1], pad=v, ldf=16, tmax_q=50, tmax_y=77, fill="zero")
        for k in ("score", "patches", "exps"):
            assert poison.same_bits(got[k], clean[k]), (pad, k)
        assert torch.equal(got["cost"][:, :3], clean["cost"][:, :3]) and torch.equal(got["info"][:, :3], clean["info"][:, :3])


def test_bits_do_not_depend_on_the_batch_the_layout_or_the_outputs():
    steps = STEP_SETS[1]
    base = [make_pair(50, 80, 13, 600), make_pair(33, 120, 13, 601), make_pair(61, 47, 13, 602, kind=1)]
    one = [run([p], 15, 4, steps) for p in base]
    three = run(base, 15, 4, steps)
    others = [make_pair(20 + i, 30 + 2 * i, 13, 610 + i) for i in range(30)]
    order = list(np.random.default_rng(1).permutation(33))
    batch = (base + others)
    mixed = [batch[i] for i in order]
    many = run(mixed, 15, 4, steps, ldf=19, tmax_q=64, tmax_y=130, ldp=20, fill="big")
    for b in range(3):
        P = ref.patch_count(len(base[b][0]), 15, 4)
        at = order.index(b)
        for k in OUTPUTS:
            rows = [one[b][k][0], three[k][b], many[k][at]]
            if k in ("cost", "info"):
                rows = [r[:P] for r in rows]
            assert poison.same_bits(rows[0].contiguous(), rows[1].contiguous()) and poison.same_bits(rows[0].contiguous(), rows[2].contiguous()), (b, k)
    compare(many, mixed, 15, 4, steps)
    for want in (("score",), ("cost",), ("info", "exps"), ("patches",)):
        part = run(base, 15, 4, steps, want=want)
        compare(part, base, 15, 4, steps, want=want)


@pytest.mark.parametrize("fill", poison.PATTERNS)
def test_guarded_windows_with_two_fills(fill):
    pairs = [make_pair(40 + 9 * i, 300 - 31 * i, 13, 700 + i) for i in range(4)]
    compare(run(pairs, 16, 8, STEP_SETS[0], fill=fill, ldf=14, ldp=11), pairs, 16, 8, STEP_SETS[0])


def test_an_empty_batch_launches_nothing():
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    dev = device()
    out = torch.full((64,), 7, dtype=torch.int64, device=dev)
    ws = torch.full((4096,), 5, dtype=torch.uint8, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    flat = (C.c_int32 * 2)(1, 1)
    assert lib.swc_subdtw(P(out), P(out), P(out), P(out), 100, 100, 13, 16, 20, 10, flat, 1, P(out), P(out), 16, P(out), P(out), P(out),
                          P(ws), 4096, 0, ops._stream()) == 0
    assert lib.swc_cmvn(P(out), P(out), 100, 13, 16, P(out), 16, 0, ops._stream()) == 0
    torch.cuda.synchronize()
    assert (out == 7).all() and (ws == 5).all()
    with pytest.raises(_lib.SwcError):
        ops.subdtw(torch.zeros((0, 4, 4), device=dev), torch.zeros((0, 4, 4), device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                   torch.zeros(0, dtype=torch.int32, device=dev))


# ---- swc_cmvn ----

CMVN_T = (1, 2, 255, 256, 257, 1000, 0)


def cmvn_rows(K, seed):
    """rows of CMVN_T frames whose columns have sigma >= 1e-3 max|c| (asserted), but for one constant column"""
    rng = np.random.default_rng(seed)
    rows = []
    for T in CMVN_T:
        c = (rng.standard_normal((T, K)) * rng.uniform(0.5, 20.0, K) + rng.uniform(-30.0, 30.0, K)).astype(np.float32)
        if K > 1:
            c[:, K - 1] = np.float32(-3.25)
        if T >= 2:
            live = c[:, :max(K - 1, 1)].astype(np.float64)
            assert (live.std(0) >= 1e-3 * np.abs(live).max(0)).all()
        rows.append(c)
    return rows


def run_cmvn(rows, K, ldf, ldo=None, in_place=False, tmax=None, fill="nan"):
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    dev = device()
    R = len(rows)
    tmax = max(len(r) for r in rows) if tmax is None else tmax
    h = np.full((R, tmax, ldf), np.nan, np.float32)          # padding columns and frames are NaN: never read
    for r, c in enumerate(rows):
        h[r, :len(c), :K] = c
    frames = torch.tensor([len(c) for c in rows], dtype=torch.int32).to(dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    if in_place:
        win, chk = poison.guarded((R * tmax, ldf), torch.float32, device=dev)
        win.copy_(torch.from_numpy(h).reshape(R * tmax, ldf))
        _lib.check(lib.swc_cmvn(P(win), P(frames), tmax, K, ldf, P(win), ldf, R, ops._stream()), "swc_cmvn")
        torch.cuda.synchronize()
        chk()
        return win.cpu().contiguous().reshape(R, tmax, ldf).numpy(), h
    ldo = ldf if ldo is None else ldo
    cep = torch.from_numpy(h).to(dev)
    win, chk = poison.guarded((R * tmax, K), torch.float32, ld=ldo, device=dev)
    poison.fill_(win, fill)
    before = win.cpu().contiguous().reshape(R, tmax, K).numpy().copy()
    assert win.stride(0) == ldo
    _lib.check(lib.swc_cmvn(P(cep), P(frames), tmax, K, ldf, P(win), ldo, R, ops._stream()), "swc_cmvn")
    torch.cuda.synchronize()
    chk()
    assert poison.same_bits(cep.cpu(), torch.from_numpy(h))
    return win.cpu().contiguous().reshape(R, tmax, K).numpy(), before


@pytest.mark.parametrize("K", (1, 13, 32))
def test_cmvn_against_the_float64_reference(K):
    """outputs are O(1) by construction; the float64 error bound T 2^-52 max|c| / sigma is far below 1e-6 for inputs with
    sigma >= 1e-3 max|c| (cmvn_rows asserts it).  The device turned out bit-equal to the reference on an MI355X (the header fixes
    the order of the sums and the rounding of every operation), so the comparison is equality"""
    rows = cmvn_rows(K, 40 + K)
    for fill in poison.PATTERNS:
        got, before = run_cmvn(rows, K, ldf=K + 3, ldo=K + 1, tmax=1003, fill=fill)
        for r, c in enumerate(rows):
            want = ref.cmvn(c)
            T = len(c)
            assert np.abs(got[r, :T].astype(np.float64) - want.astype(np.float64)).max(initial=0.0) <= 1e-6, (K, T)
            assert got[r, :T].tobytes() == want.tobytes(), (K, T)
            assert got[r, T:].tobytes() == before[r, T:].tobytes(), (K, T)       # frames beyond T are not written
            if K > 1 and T:
                assert (got[r, :T, K - 1] == 0).all()                             # the constant column
            if T == 1:
                assert (got[r, 0] == 0).all()


def test_cmvn_nan_stays_in_its_column_and_in_place():
    rows = cmvn_rows(13, 77)
    bad = rows[5].copy()
    bad[600, 4] = np.nan
    bad[10, 9] = np.inf
    rows[5] = bad
    out, _ = run_cmvn(rows, 13, ldf=16)
    inp, h = run_cmvn(rows, 13, ldf=16, in_place=True)
    for r, c in enumerate(rows):
        T = len(c)
        assert out[r, :T].tobytes() == inp[r, :T, :13].tobytes(), r                 # in place gives the same bits
        assert inp[r, :T, 13:].tobytes() == h[r, :T, 13:].tobytes() and inp[r, T:].tobytes() == h[r, T:].tobytes()
    assert np.isnan(out[5, :1000, 4]).all() and np.isnan(out[5, :1000, 9]).all()
    keep = [k for k in range(13) if k not in (4, 9)]
    assert np.isfinite(out[5, :1000][:, keep]).all()
    assert out[5, :1000][:, keep].tobytes() == ref.cmvn(rows[5])[:, keep].tobytes()


# ---- metrics.warpq end to end ----

def speech(seed, n=None):
    import pitch_ref
    key = ("speech", seed)
    if key not in _CACHE:
        _CACHE[key] = (pitch_ref.test_signal(seed, noise=1e-3) * np.float32(0.8)).astype(np.float32)
    return _CACHE[key][:n]


def noisy(x, snr_db, seed):
    rng = np.random.default_rng(seed)
    n = rng.standard_normal(len(x))
    g = np.sqrt(np.mean(x.astype(np.float64) ** 2) / np.mean(n ** 2)) * 10.0 ** (-snr_db / 20.0)
    return (x + g * n).astype(np.float32)


def device_features(rows):
    """the device's own normalised cepstra of a list of host rows -> list of f32 [T][13]"""
    from simwhisper_codec_amd import metrics, ops
    dev = device()
    c = ops.cepstra([torch.from_numpy(r).to(dev) for r in rows], metrics.warpq_table(16000, dev), ldf=16)
    f = ops.cmvn(c["cep"], c["frames"], metrics.WARPQ_COEFFS).cpu().numpy()
    return [f[i, :T, :metrics.WARPQ_COEFFS] for i, T in enumerate(c["counts"])]


def test_warpq_is_the_reference_on_the_devices_own_features():
    from simwhisper_codec_amd import metrics
    dev = device()
    x, x2 = speech(1, 20000), speech(2, 17000)
    refs, degs = [x, x2, x], [noisy(x, 15.0, 1)[:18000], noisy(x2, 5.0, 2), x[:1500]]
    got = metrics.warpq([torch.from_numpy(r) for r in refs], [torch.from_numpy(d).to(dev) for d in degs], vad=False, tracks=True, device=dev)
    feats = device_features(refs + degs)
    assert set(got) == {"warpq", "patches", "frames_ref", "frames_deg", "cost", "start", "end"}
    assert got["warpq"].dtype == torch.float64 and got["warpq"].device == dev
    assert got["frames_ref"].tolist() == [len(f) for f in feats[:3]] and got["frames_deg"].tolist() == [len(f) for f in feats[3:]]
    for b in range(3):
        w = ref.subdtw(feats[3 + b], feats[b], 100, 50, ref.WARPQ)
        assert poison.same_bits(got["warpq"][b].cpu().reshape(1), torch.tensor([w["score"]], dtype=torch.float64)), (b, got["warpq"][b], w["score"])
        assert tuple(got["patches"][b].tolist()) == w["patches"]
        assert got["start"][b].tolist() == w["info"][:, 1].tolist() and got["end"][b].tolist() == w["info"][:, 2].tolist()
        assert got["cost"][b].cpu().tolist() == [float(np.ldexp(np.float64(c), w["e"] - 17)) for c in w["cost"]]
    assert got["patches"][2].tolist() == [0, 0] and torch.isnan(got["warpq"][2]) and got["warpq"][0] > 0


def test_warpq_of_a_row_with_itself_is_zero_and_noise_is_ordered():
    from simwhisper_codec_amd import metrics, synth
    dev = device()
    x = synth.synth_audio(24000, index=3, kind="speech").numpy().astype(np.float32)
    rows = [torch.from_numpy(x).to(dev), torch.from_numpy(speech(4, 24000)).to(dev)]
    for vad in (True, False):
        z = metrics.warpq(rows, [r.clone() for r in rows], vad=vad, device=dev)
        assert z["warpq"].tolist() == [0.0, 0.0] and (z["patches"][:, 0] == z["patches"][:, 1]).all() and (z["patches"][:, 0] > 0).all(), vad
    s = metrics.warpq([rows[0]] * 2, [torch.from_numpy(noisy(x, 0.0, 5)), torch.from_numpy(noisy(x, 30.0, 5))], vad=False, device=dev)["warpq"].tolist()
    print("score after WARP-Q at 0 dB and 30 dB SNR:", s)
    assert s[0] > s[1] > 0.0


def test_a_cut_in_the_middle_shows_in_the_start_track():
    """0.3 s (75 frames) cut out of the degraded row's middle: under the symmetric step set the patches after the cut are matched
    75 frames later in the reference than their own position.  The bound: a window of 512 samples is 8 hops, so the frames within
    4 hops of the cut hold samples of both sides, and a patch is trusted when it keeps 8 frames away from the cut; the median over
    such patches may be off by those 4 frames"""
    from simwhisper_codec_amd import metrics
    dev = device()
    x = speech(6, 28000)
    cut = np.concatenate([x[:12000], x[12000 + 4800:]])
    got = metrics.warpq([torch.from_numpy(x)], [torch.from_numpy(cut)], steps=metrics.SYMMETRIC_STEPS, patch_ms=200.0, vad=False,
                        tracks=True, device=dev)
    f = device_features([x, cut])
    w = ref.subdtw(f[1], f[0], 50, 25, ref.SYMMETRIC)
    assert got["start"][0].tolist() == w["info"][:, 1].tolist() and got["end"][0].tolist() == w["info"][:, 2].tolist()
    start = np.array(got["start"][0].tolist())
    own = np.arange(len(start)) * 25
    lead = start - own
    print("start - own position per patch:", lead.tolist())
    before, after = lead[own + 50 <= 12000 // 64 - 8], lead[own >= 12000 // 64 + 8]
    assert len(before) >= 3 and len(after) >= 3 and abs(np.median(before)) <= 4 and abs(np.median(after) - 75) <= 4


def test_silence_the_frame_limit_and_alignment():
    import align_ref
    from simwhisper_codec_amd import metrics
    from simwhisper_codec_amd._lib import SwcError
    dev = device()
    x = speech(7, 24000)
    got = metrics.warpq([torch.from_numpy(x), torch.from_numpy(x)], [torch.zeros(24000), torch.from_numpy(x)], device=dev)
    assert torch.isnan(got["warpq"][0]) and got["frames_deg"][0] == 0 and got["patches"][0].tolist() == [0, 0] and got["warpq"][1] == 0.0
    long = torch.zeros(8192 * 64, device=dev)
    with pytest.raises(SwcError, match="at most MAX_FRAMES = 8192"):
        metrics.warpq([long], [torch.from_numpy(x)], vad=False, device=dev)
    with pytest.raises(SwcError, match="at most MAX_FRAMES = 8192"):
        metrics.warpq([torch.from_numpy(x)], [long], vad=False, device=dev)
    ok = metrics.warpq([long[:-64]], [torch.from_numpy(x)], vad=False, device=dev)
    assert ok["frames_ref"].tolist() == [8192]
    refs = [torch.from_numpy(x), torch.from_numpy(speech(8, 20000))]
    degs = [torch.from_numpy((0.8 * align_ref.delayed(x, 37, n=len(x) + 50)).astype(np.float32)).to(dev),
            torch.from_numpy(noisy(align_ref.delayed(speech(8, 20000), -12), 30.0, 3)).to(dev)]
    a = metrics.warpq(refs, degs, align="waveform", max_lag_ms=10.0, vad=False, device=dev)
    xs, ys, al = metrics.aligned(refs, degs, max_lag_ms=10.0, device=dev)
    want = metrics.warpq(xs, ys, vad=False, device=dev)
    assert set(a) == set(want) | {"lag"} and a["lag"].tolist() == al["lag"].tolist() == [37, -12]
    for k in want:
        assert poison.same_bits(a[k].cpu().contiguous(), want[k].cpu().contiguous()), k


def test_subsequence_dtw_finds_a_snippet():
    from simwhisper_codec_amd import metrics
    dev = device()
    rng = np.random.default_rng(12)
    y = [rng.standard_normal((400, 20)).astype(np.float32), rng.standard_normal((90, 20)).astype(np.float32)]
    q = [y[0][210:290].copy(), y[1][5:25].copy()]
    r = metrics.subsequence_dtw([torch.from_numpy(v) for v in q], [torch.from_numpy(v).to(dev) for v in y], device=dev)
    assert set(r) == {"cost", "steps", "start", "end", "status", "score", "patches"}
    assert r["start"][:, 0].tolist() == [210, 5] and r["end"][:, 0].tolist() == [289, 24] and r["steps"][:, 0].tolist() == [80, 20]
    assert r["cost"][:, 0].tolist() == [0, 0] and r["score"].tolist() == [0.0, 0.0] and r["status"][:, 0].tolist() == [0, 0]
    r = metrics.subsequence_dtw([torch.from_numpy(v) for v in q], [torch.from_numpy(v) for v in y], patch=10, step=10, device=dev)
    assert r["patches"].tolist() == [[8, 8], [2, 2]] and r["start"][0].tolist() == [210 + 10 * p for p in range(8)]


def test_audiocodec_warpq_and_the_tool(tmp_path, capsys):
    import common
    from simwhisper_codec_amd import synth, wavio
    from simwhisper_codec_amd.codec import AudioCodec
    dev = device()
    model = AudioCodec(common.tiny_params(), precision="fp32")
    model.load_state_dict(common.state_dict("tiny"), strict=True)
    model = model.to(dev).eval()
    wavs = [synth.synth_audio(18000, index=0, kind="speech").to(dev), synth.synth_audio(17000, index=1, kind="speech").to(dev)]
    q = model.warpq(wavs, vad=False)
    assert set(q) == {"warpq", "patches", "frames_ref", "frames_deg"} and q["warpq"].shape == (2,) and q["warpq"].device == dev
    print("AudioCodec.warpq:", q["warpq"].cpu().tolist(), q["patches"].cpu().tolist())
    assert torch.isfinite(q["warpq"]).all() and (q["warpq"] > 0).all() and (q["patches"][:, 0] > 0).all()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_warpq
    os.makedirs(tmp_path / "orig"); os.makedirs(tmp_path / "syn")
    x = speech(1, 24000)
    for i, v in enumerate((noisy(x, 10.0, 1), x, np.zeros(24000, np.float32))):
        wavio.save_audio(str(tmp_path / "orig" / f"utt{i}.wav"), torch.from_numpy(x), 16000)
        wavio.save_audio(str(tmp_path / "syn" / f"utt{i}.wav"), torch.from_numpy(v), 16000)
    args = ["--original_dir", str(tmp_path / "orig"), "--synthesized_dir", str(tmp_path / "syn"), "--batch_size", "2", "--verbose"]
    assert evaluate_warpq.main(args) == 0
    out = capsys.readouterr().out
    assert evaluate_warpq.main(args + ["--no_vad", "--patch_ms", "200", "--align", "waveform", "--max_lag_ms", "10"]) == 0
    plain = capsys.readouterr().out
    print(out, plain)
    assert "utt1.wav: 0.0000" in out and "utt2.wav: not defined" in out and "NaN pairs: 1" in out and "over 2 pairs" in out
    assert "not defined, left out (1): utt2.wav" in out and "mean " in out and "median " in out
    assert "alignment: mean |lag|" in plain and "utt1.wav: 0.0000" in plain
