"""swc_dtw and swc_cepstra on the GPU against the restatements of include/swc_mcd.h (tests/dtw_ref.py in numpy int64,
tests/mcd_ref.py in float64): total, info and path bit for bit, mean within one f32 ulp; the sweep of frame counts round the
strip height, feature counts, bands and both modes; the accumulator bounds at 8192 x 8192; bit independence of everything that
is not the pair; the memory contract; NaN / Inf; the cepstra's frame counts and error; metrics.mcd end to end, its known
answers, and the wiring down to the tool."""
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

import dtw_ref as ref  # noqa: E402
import mcd_ref  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu

POISON_ADDRESS = 0x10       # the "address" of an empty row: never dereferenced
OUTPUTS = ("total", "info", "mean", "path")
DTYPES = {"total": torch.int64, "info": torch.int32, "mean": torch.float32, "path": torch.int32}
S = 256                      # SWC_DTW_STRIP
FRAMES = (1, 2, 3, 63, 64, 65, S - 1, S, S + 1, 2 * S + 17)
TOP = np.float32(1.9999999)  # the largest f32 below 2: q = 8191 where 1.0 gives 4096
# The largest |cep - float64 reference| relative to the row's cepstral peak, measured on an MI355X.
#   test_cepstra_shapes_and_error: 4.1e-6 at W = 32, 1.8e-4 at W = 512, 3.9e-3 at W = 2048.  The worst row is the one-sample row:
#   a click has a flat spectrum, so every mel band has the same logarithm up to the sampling of the triangles, c1 .. c13 nearly
#   cancel (the finer the bins, the more completely) and the row's cepstral peak, the yardstick, is itself a rounding-sized
#   remainder of 80-term f32 sums.  The bound over all cases is four times the largest: 1.6e-2.
#   Every row of more than one sample, in that test and in test_cepstra_rates (1 s of noise at three levels and of the
#   speech-like signal, the default parameters of every rate): 1.6e-6 .. 2.3e-5, growing with W (a longer f32 FFT; the
#   chance-small bins of a noise spectrum carry the FFT's absolute error into narrow mel bands).  Those rows get their own bound,
#   four times their largest: 9.3e-5.
CEP_BOUND = 1.6e-2
CEP_BOUND_ROWS = 9.3e-5
# |metrics.mcd - the all-float64 chain| in dB (float64 cepstra, float64 distances, float64 DTW).  Measured over the eight values
# of test_end_to_end: 3.3e-5 .. 2.0e-3 dB (the features are rounded to a step of 2^(e - 13), 2^-7 where the cepstral peak is
# between 32 and 64: an error of that size per coefficient, averaged along the path and times 6.14).  The bound is four times
# the largest.
MCD_BOUND_DB = 7.9e-3
_CACHE = {}


def device():
    return torch.device("cuda", torch.cuda.current_device())


# ---- swc_dtw: pairs, the call, the comparison ----

def make_pair(Tx, Ty, D, seed, kind):
    """kind 0: y = x resampled along a wobbling time axis, plus noise (a path that wanders); kind 1: features in {-1, 0, 1}
    (equal costs everywhere: the tie rule decides); kind 2: all zero"""
    key = ("pair", Tx, Ty, D, seed, kind)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        if kind == 2:
            x, y = np.zeros((Tx, D), np.float32), np.zeros((Ty, D), np.float32)
        elif kind == 1:
            x, y = rng.integers(-1, 2, (Tx, D)).astype(np.float32), rng.integers(-1, 2, (Ty, D)).astype(np.float32)
        else:
            base = np.cumsum(rng.standard_normal((max(Tx, 1), D)), axis=0).astype(np.float32) * np.float32(0.37)
            x = base[:Tx]
            t = np.linspace(0.0, max(Tx - 1, 0), Ty) + 3.0 * np.sin(np.arange(Ty) / 9.0 + seed)
            y = (base[np.clip(np.rint(t).astype(int), 0, max(Tx - 1, 0))] + 0.05 * rng.standard_normal((Ty, D))).astype(np.float32) if Tx else np.zeros((Ty, D), np.float32)
        _CACHE[key] = (x, y)
    return _CACHE[key]


def reference(x, y, band, mode):
    key = ("ref", x.tobytes(), y.tobytes(), x.shape, y.shape, band, mode)
    if key not in _CACHE:
        _CACHE[key] = ref.dtw(x, y, band=band, mode=mode)
    return _CACHE[key]


def run(pairs, band=0, mode="warp", want=OUTPUTS, fill="nan", ldf=None, tmax_x=None, tmax_y=None, ldp=None, pad=float("nan"), guard=True):
    """one swc_dtw call on guarded, pre-filled outputs and workspace -> dict of host tensors for the wanted outputs plus "before"
    (the fill of every output).  The feature matrices are [B][Tmax][ldf] with `pad` in every padding column and frame.  Outputs
    that were not asked for must keep their fill; nothing may be written outside the windows."""
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    dev = device()
    B, D = len(pairs), pairs[0][0].shape[1]
    tx, ty = [len(x) for x, _ in pairs], [len(y) for _, y in pairs]
    tmax_x = max(tx) if tmax_x is None else tmax_x
    tmax_y = max(ty) if tmax_y is None else tmax_y
    ldf = D if ldf is None else ldf
    hx, hy = np.full((B, tmax_x, ldf), pad, np.float32), np.full((B, tmax_y, ldf), pad, np.float32)
    for b, (x, y) in enumerate(pairs):
        hx[b, :min(len(x), tmax_x), :D], hy[b, :min(len(y), tmax_y), :D] = x[:tmax_x], y[:tmax_y]      # a count beyond the bound stays in tx / ty
    xf, yf = torch.from_numpy(hx).to(dev), torch.from_numpy(hy).to(dev)
    counts = torch.tensor(tx + ty, dtype=torch.int32).to(dev)
    steps = tmax_x + tmax_y - 1 if tmax_x and tmax_y else 0
    ldp = steps if ldp is None else ldp
    need = ops.dtw_workspace_bytes(B, tmax_x, tmax_y, "path" in want)
    shapes = {"total": (B, 1), "info": (B, 4), "mean": (B, 1), "path": (B, max(ldp, 1) * 2)}
    outs, checks = {}, []
    for name in OUTPUTS:
        outs[name], chk = poison.guarded(shapes[name], DTYPES[name], device=dev, band_rows=4 if name == "path" else 256)
        outs[name].zero_() if fill == "zero" else poison.fill_(outs[name], fill)
        checks.append(chk)
    before = {k: v.cpu().clone() for k, v in outs.items()}
    if guard:
        ws, check_w = poison.guarded((max(need // 256, 1), 256), torch.uint8, device=dev, band_rows=16)
    else:
        ws, check_w = torch.zeros(max(need, 256), dtype=torch.uint8, device=dev), lambda: None
    assert ws.is_contiguous() and ws.data_ptr() % 256 == 0 and need % 256 == 0
    ws.zero_() if fill == "zero" else poison.fill_(ws.view(torch.float32), fill)
    P = lambda t: C.c_void_p(t.data_ptr())
    arg = lambda name: P(outs[name]) if name in want else None
    rc = lib.swc_dtw(P(xf), P(yf), P(counts[:B]), P(counts[B:]), tmax_x, tmax_y, D, ldf, band, ops.DTW_MODES[mode], arg("total"), arg("info"),
                     arg("mean"), arg("path"), ldp, P(ws), need, B, ops._stream())
    _lib.check(rc, "swc_dtw")
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    check_w()
    res = {"before": before}
    for name in OUTPUTS:
        got = outs[name].cpu().clone()
        if name in want:
            res[name] = got
        else:
            assert poison.same_bits(got, before[name]), f"{name} was not asked for and was written"
    return res


def row_bits(res, b):
    """what the call says about pair b, as bytes (the path up to its N)"""
    parts = []
    n = int(res["info"][b, 0]) if "info" in res else None
    for k in OUTPUTS:
        if k in res:
            v = res[k][b, :2 * n] if k == "path" and n is not None else res[k][b]
            parts.append(v.contiguous().view(torch.uint8).numpy().tobytes())
    return b"".join(parts)


def compare(got, b, want):
    """pair b of a call against its reference dict: total, info and path equal, the path entries at and beyond N untouched, mean
    within one f32 ulp (-> the distance seen)"""
    assert int(got["total"][b, 0]) == want["total"], (b, int(got["total"][b, 0]), want["total"])
    assert got["info"][b].tolist() == want["info"].tolist(), (b, got["info"][b].tolist(), want["info"].tolist())
    n = int(want["info"][0])
    path = got["path"][b].numpy()
    assert np.array_equal(path[:2 * n].reshape(n, 2), want["path"]), (b, n)
    assert poison.same_bits(got["path"][b, 2 * n:].contiguous(), got["before"]["path"][b, 2 * n:].contiguous()), (b, "path beyond N")
    v, w = got["mean"][b].numpy()[0], want["mean"]
    if np.isnan(w):
        assert np.isnan(v), (b, v)
        return 0
    u = abs(int(np.float32(v).view(np.int32)) - int(np.float32(w).view(np.int32)))
    assert u <= 1, (b, v, w)
    return u


def batch_of(B, D, seed=0):
    """B pairs: frame counts walking FRAMES at two strides (Tx != Ty in most), the three kinds in turn, two empty pairs from
    B = 12 on"""
    out = []
    for k in range(B):
        Tx, Ty = FRAMES[(3 * k + 9) % 10], FRAMES[(7 * k + 4) % 10]
        if k in (11, 23):
            Tx, Ty = (0, 65) if k == 11 else (3, 0)
        out.append(make_pair(Tx, Ty, D, seed + k, kind=(k % 5 == 3) + 2 * (k % 11 == 7)))
    return out


def check_batch(pairs, band, mode):
    got = run(pairs, band, mode)
    worst = max(compare(got, b, reference(x, y, band, mode)) for b, (x, y) in enumerate(pairs))
    return got, worst


# ---- against the reference ----

@pytest.mark.parametrize("B", [1, 3, 33])
def test_total_info_path_and_mean(B):
    pairs = batch_of(B, 13)
    for band, mode in ((0, "warp"), (2, "warp"), (0, "diagonal")):
        got, worst = check_batch(pairs, band, mode)
        print(f"B={B} r={band} {mode}: largest distance of a mean {worst} ulp; steps {got['info'][:, 0].tolist()}")
    if B == 33:
        shapes = {(len(x), len(y)) for x, y in pairs}
        assert {t for s in shapes for t in s} >= set(FRAMES) and sum(1 for a, b in shapes if a != b) > len(shapes) // 2
        assert sum(1 for x, y in pairs if len(x) == 0 or len(y) == 0) == 2


@pytest.mark.parametrize("D,bands", [(1, (0, 1)), (2, (2, 7)), (13, (1, 7)), (24, (0, 7)), (31, (1, 2)), (32, (0, 2))])
def test_frame_count_feature_and_band_sweep(D, bands):
    """every frame count round the strip height on both sides, every feature count round the groups of eight, bands 0, 1, 2, 7,
    both modes"""
    pairs = []
    for k in range(12):
        Tx, Ty = FRAMES[(k + 6) % 10], FRAMES[(3 * k + 7) % 10]
        pairs.append(make_pair(Tx, Ty, D, 100 + k, kind=int(k % 4 == 2)))
    pairs.append(make_pair(2 * S + 17, 2 * S + 17, D, 113, 0))
    pairs.append(make_pair(S + 1, 2 * S + 17, D, 114, 1))
    assert {len(x) for x, _ in pairs} >= set(FRAMES) and {len(y) for _, y in pairs} >= set(FRAMES)
    assert sum(1 for x, y in pairs if len(x) != len(y)) > len(pairs) // 2
    for band in bands:
        got, worst = check_batch(pairs, band, "warp")
        print(f"D={D} r={band}: largest distance of a mean {worst} ulp; steps {got['info'][:, 0].tolist()}")
    check_batch(pairs, bands[0], "diagonal")


def test_the_accumulator_bounds():
    """features alternating +-peak over D = 32 against their negation: every difference is +-16382, every s is 32 16382^2, every
    d the largest there is.  A small pair against the reference, then 8192 x 8192 frames against the closed form: the diagonal,
    N = 8192, total = 8192 d_max (C beyond 2^33, the last strip, the direction matrix at its largest)"""
    sign = np.where(np.arange(32) % 2 == 0, 1.0, -1.0).astype(np.float32)
    frame = TOP * sign
    assert (np.abs(ref.quantise(frame, 1)) == ref.QMAX).all()
    small = (np.tile(frame, (S + 3, 1)), np.tile(-frame, (S - 2, 1)))
    for band, mode in ((0, "warp"), (3, "warp"), (0, "diagonal")):
        got, _ = check_batch([small], band, mode)
        n = int(got["info"][0, 0])
        assert int(got["total"][0, 0]) == n * ref.D_MAX and n == (S + 3 if mode == "warp" else S - 2)
    T = ref.MAX_FRAMES
    big = (np.tile(frame, (T, 1)), np.tile(-frame, (T, 1)))
    for mode in ("warp", "diagonal"):
        got = run([big], 0, mode, guard=False)
        assert int(got["total"][0, 0]) == T * ref.D_MAX > 2 ** 33 and got["info"][0].tolist() == [T, T, T, 1]
        assert np.array_equal(got["path"][0].numpy()[:2 * T].reshape(T, 2), np.repeat(np.arange(T, dtype=np.int32)[:, None], 2, 1))
        assert poison.same_bits(got["path"][0, 2 * T:].contiguous(), got["before"]["path"][0, 2 * T:].contiguous())
        want = np.float32(np.ldexp(np.float64(T * ref.D_MAX) / np.float64(16 * T), 1 - 13))
        assert got["mean"][0, 0].numpy() == want and abs(float(want) - 2.0 * 2.0 * 32 ** 0.5) < 1e-2


# ---- independence ----

def test_bits_do_not_depend_on_anything_but_the_pair():
    pairs = batch_of(33, 13)
    for band, mode in ((0, "warp"), (2, "warp"), (0, "diagonal")):
        base = run(pairs, band, mode)
        bits = [row_bits(base, b) for b in range(33)]
        empty = [b for b, (x, y) in enumerate(pairs) if len(x) == 0 or len(y) == 0]
        assert empty and all(base["info"][b].tolist() == [0, 0, 0, 0] and int(base["total"][b, 0]) == 0 for b in empty)
        for b in (0, 6, 20):                                                   # B and the pair's index
            assert row_bits(run(pairs[b:b + 1], band, mode), 0) == bits[b], (mode, b)
        three = run(pairs[4:7], band, mode)
        assert [row_bits(three, k) for k in range(3)] == bits[4:7]
        rev = run(pairs[::-1], band, mode)
        assert [row_bits(rev, 32 - b) for b in range(33)] == bits
        wide = run(pairs, band, mode, ldf=19, tmax_x=2 * S + 40, tmax_y=3 * S + 1, ldp=5 * S + 90)     # strides, bounds: other grids
        assert [row_bits(wide, b) for b in range(33)] == bits
        x, y = pairs[6]                                                        # a count beyond the bound is cut there
        cut = run([(np.concatenate([x, x[:5]]), np.concatenate([y, y[:7]]))], band, mode, tmax_x=len(x), tmax_y=len(y))
        assert len(x) > 5 and len(y) > 7 and row_bits(cut, 0) == bits[6]
        for k in range(1, len(OUTPUTS) + 1):                                   # which outputs are asked for: every subset
            for want in itertools.combinations(OUTPUTS, k):
                part = run(pairs[:7], band, mode, want=want)
                for name in want:
                    if name == "path":
                        for b in range(7):
                            n = int(base["info"][b, 0])
                            assert poison.same_bits(part[name][b, :2 * n].contiguous(), base[name][b, :2 * n].contiguous()), (mode, want, b)
                    else:
                        assert poison.same_bits(part[name], base[name][:7].contiguous()), (mode, want, name)


def test_memory_contract_and_fill_independence():
    """outputs and workspace are pre-filled two ways (and with zeros) and guarded: run() checks the bands, compare() the path
    entries at and beyond N; the results must not depend on what the workspace or the outputs held"""
    pairs = batch_of(7, 13)
    for band, mode in ((0, "warp"), (1, "warp"), (0, "diagonal")):
        res = [run(pairs, band, mode, fill=f, ldp=4 * S + 40) for f in ("nan", "big", "zero")]
        for b, (x, y) in enumerate(pairs):
            for r in res:
                compare(r, b, reference(x, y, band, mode))
            assert row_bits(res[0], b) == row_bits(res[1], b) == row_bits(res[2], b), (mode, b)


def test_nan_and_inf_stay_alone_and_padding_is_never_read():
    pairs = batch_of(33, 13)
    bad = [b for b, (x, y) in enumerate(pairs) if len(x) > 60 and len(y) > 60][:3]
    assert len(bad) == 3
    for band, mode in ((0, "warp"), (0, "diagonal")):
        base = run(pairs, band, mode)                                # NaN in every padding column and frame
        for pad in (0.0, float("inf")):
            other = run(pairs, band, mode, pad=pad, ldf=16, tmax_x=2 * S + 20)
            assert [row_bits(other, b) for b in range(33)] == [row_bits(base, b) for b in range(33)], (mode, pad)
        hit_pairs = [(x.copy(), y.copy()) for x, y in pairs]
        hit_pairs[bad[0]][1][50, 3] = np.nan          # a degraded side
        hit_pairs[bad[1]][0][3, 0] = np.inf           # a clean side
        hit_pairs[bad[2]][1][-1, -1] = -np.inf
        hit = run(hit_pairs, band, mode)
        for b in range(33):
            if b in bad:
                assert base["info"][b, 0] > 0
                assert hit["info"][b].tolist() == [0, 0, 0, 0] and int(hit["total"][b, 0]) == 0 and torch.isnan(hit["mean"][b, 0])
                compare(hit, b, ref.dtw(*hit_pairs[b], band=band, mode=mode))
            else:
                assert row_bits(hit, b) == row_bits(base, b), (mode, b)


# ---- swc_cepstra ----

def make_table(sr, W, H, M, K=13):
    """the parameters and tables of a swc_cepstra call as host arrays: `M` Slaney filters at rate sr, the DCT rows 1 .. K"""
    from simwhisper_codec_amd import metrics
    first, count, off, w = metrics.pack_filterbanks([metrics.mel_filterbank(sr, W, M)])
    return {"W": W, "H": H, "n_mels": M, "K": K, "first": first, "count": count, "off": off, "w": w,
            "dct": metrics.dct_matrix(K, M).astype(np.float32)}


def run_cepstra(rows, t, fill="nan", ldf=None, max_n=None):
    """one swc_cepstra call on guarded, pre-filled outputs -> (cep [R][T_max][K] host tensor, frames list, before); empty rows
    sit behind the poison address; the entries with t >= T of a row must keep their fill"""
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    dev = device()
    R, K, H = len(rows), t["K"], t["H"]
    keep, ptrs = [], []
    for v in rows:
        if len(v) == 0:
            ptrs.append(POISON_ADDRESS)
            continue
        buf = torch.full((len(v) + 1,), float("nan"), device=dev)
        buf[1:] = torch.from_numpy(v)                     # 4-byte alignment only
        keep.append(buf)
        ptrs.append(buf.data_ptr() + 4)
    n_in = [len(v) for v in rows]
    max_n = max(n_in) if max_n is None else max_n
    t_max = 1 + max_n // H
    ldf = K if ldf is None else ldf
    cep, chk_c = poison.guarded((R * t_max, K), torch.float32, ld=ldf, device=dev, band_rows=64)
    frames, chk_f = poison.guarded((R, 1), torch.int32, device=dev)
    poison.fill_(cep, fill), poison.fill_(frames, fill)
    before = cep.cpu().clone().reshape(R, t_max, K)
    dt = {k: torch.from_numpy(np.ascontiguousarray(t[k])).to(dev) for k in ("first", "count", "off", "w", "dct")}
    meta = torch.tensor(ptrs + n_in, dtype=torch.int64).to(dev)
    P = lambda x: C.c_void_p(x.data_ptr())
    rc = lib.swc_cepstra(P(meta[:R]), P(meta[R:]), max_n, t["W"], H, t["n_mels"], P(dt["first"]), P(dt["count"]), P(dt["off"]), P(dt["w"]),
                         dt["w"].numel(), P(dt["dct"]), K, P(cep), ldf, P(frames), None, 0, R, ops._stream())
    _lib.check(rc, "swc_cepstra")
    torch.cuda.synchronize()
    chk_c(), chk_f()
    return cep.cpu().clone().reshape(R, t_max, K), frames.cpu().reshape(-1).tolist(), before


def noise(n, seed, level=0.1):
    rng = np.random.default_rng(seed)
    return (level * rng.standard_normal(n) * (0.3 + np.abs(np.sin(np.arange(n) / 500.0 + seed)))).astype(np.float32)


def cepstra_error(rows, t, **kw):
    """run, check frame counts and untouched entries -> the largest |cep - reference| relative to the row's cepstral peak, over
    all rows and over the rows of more than one sample"""
    got, frames, before = run_cepstra(rows, t, **kw)
    bank = mcd_ref.dense_bank(t["first"], t["count"], t["off"], t["w"], t["W"] // 2 + 1)
    max_n = kw.get("max_n")
    worst, worst_rows = 0.0, 0.0
    for r, v in enumerate(rows):
        v = v if max_n is None else v[:max_n]
        T = 1 + len(v) // t["H"] if len(v) else 0
        assert frames[r] == T, (r, len(v), frames[r], T)
        assert poison.same_bits(got[r, T:].contiguous(), before[r, T:].contiguous()), (r, "frames beyond T were written")
        if T:
            want = mcd_ref.cepstra(v, t["W"], t["H"], bank, t["dct"])
            e = float(np.abs(got[r, :T].numpy().astype(np.float64) - want).max() / np.abs(want).max())
            print(f"  row of {len(v)} samples: error {e:.3e} of its cepstral peak {np.abs(want).max():.3e}")
            worst, worst_rows = max(worst, e), max(worst_rows, e if len(v) > 1 else 0.0)
    return worst, worst_rows


@pytest.mark.parametrize("W", [32, 512, 2048])
def test_cepstra_shapes_and_error(W):
    """lengths 0, 1, H - 1, H, H + 1, W / 2 - 1, W / 2 + 1 and 3 s at hops 1, W / 4 and W.  (At H = 1 the 3 s row is kept for
    W = 32 only: the float64 reference of 48001 frames of 2048 samples is a gigabyte; the long row there is 4 W + 3 samples.)"""
    sr = 16000
    worst, worst_rows = 0.0, 0.0
    for H in (1, W // 4, W):
        t = make_table(sr, W, H, min(80, W // 2 - 2))
        long = 3 * sr if (H > 1 or W == 32) else 4 * W + 3
        lengths = sorted({0, 1, max(H - 1, 0), H, H + 1, W // 2 - 1, W // 2 + 1, long})
        rows = [noise(n, 7 * k + W) for k, n in enumerate(lengths)]
        e, e_rows = cepstra_error(rows, t, ldf=16 if H > 1 else None)
        print(f"W={W} H={H}: lengths {lengths}: largest error relative to the row's cepstral peak {e:.3e}, {e_rows:.3e} without the one-sample row")
        worst, worst_rows = max(worst, e), max(worst_rows, e_rows)
    assert worst <= CEP_BOUND and worst_rows <= CEP_BOUND_ROWS, (worst, worst_rows)


def test_cepstra_rates():
    """the default parameters of every rate of metrics.RATES, 1 s of noise at three levels and of the pitch tests' signal (a
    stretch of exact zeros and a stretch at 1e-4: bands at the clamp floor); a row longer than max_n_in is cut"""
    import pitch_ref
    from simwhisper_codec_amd import metrics
    worst = 0.0
    for sr in metrics.RATES:
        W, H = metrics.mcd_params(sr)
        t = make_table(sr, W, H, metrics.MCD_MELS)
        rows = [noise(sr, 1, 0.1), noise(sr + 17, 2, 1e-3), noise(sr - 5, 3, 0.9), pitch_ref.test_signal(3, sr=sr)[:sr + H]]
        e, _ = cepstra_error(rows, t, ldf=16, max_n=sr + 3)
        print(f"{sr} Hz (W={W}, H={H}): largest error relative to the row's cepstral peak {e:.3e}")
        worst = max(worst, e)
    assert worst <= CEP_BOUND_ROWS, worst


def test_identical_rows_give_identical_cepstra_and_nan_stays_in_its_frames():
    t = make_table(16000, 512, 160, 80)
    x = noise(16000, 11)
    bad = x.copy(); bad[8000] = np.nan
    rows = [x, noise(5000, 12), x.copy(), np.zeros(0, np.float32), bad, x[:9000].copy()]
    got, frames, _ = run_cepstra(rows, t, ldf=16)
    assert frames == [101, 32, 101, 0, 101, 57]
    assert poison.same_bits(got[0], got[2]) and not np.isnan(got[0].numpy()).any()
    alone, _, _ = run_cepstra([x], t, fill="big")
    assert poison.same_bits(alone[0], got[0])                        # the batch, the row's index, the stride and the fill do not matter
    assert poison.same_bits(got[5, :54].contiguous(), got[0, :54].contiguous())         # frames that see the same samples
    nan_frames = np.isnan(got[4].numpy()).any(axis=1)
    assert nan_frames[49:52].all() and nan_frames.sum() <= 4 and poison.same_bits(got[4, :48].contiguous(), got[0, :48].contiguous())


# ---- metrics.mcd ----

def speech(seed, sr=16000):
    import pitch_ref
    key = ("speech", seed, sr)
    if key not in _CACHE:
        _CACHE[key] = (pitch_ref.test_signal(seed, sr=sr, noise=1e-3) * np.float32(0.8)).astype(np.float32)
    return _CACHE[key]


def duplicated(x, H, share=0.05, seed=0):
    """x with that share of its hops (blocks of H samples) played twice"""
    blocks = [x[i:i + H] for i in range(0, len(x), H)]
    twice = set(np.random.default_rng(seed).choice(len(blocks), int(round(share * len(blocks))), replace=False).tolist())
    return np.concatenate([np.concatenate([b, b]) if k in twice else b for k, b in enumerate(blocks)]).astype(np.float32)


def test_end_to_end():
    """metrics.mcd is bit-equal to dtw_ref on the kernel's own cepstra read back (times 10 sqrt 2 / ln 10 in f32), and agrees with
    the all-float64 chain (float64 cepstra, float64 DTW) within MCD_BOUND_DB"""
    from simwhisper_codec_amd import metrics, ops
    dev = device()
    sr = 16000
    x0, x1, x2 = speech(1), speech(2), speech(3)[:20000]
    refs = [x0, x1, x2, x0[:7000]]
    degs = [(x0 + noise(len(x0), 5, 0.01)).astype(np.float32), duplicated(x1, 160)[:30000], (0.5 * x2[400:]).astype(np.float32), speech(4)[:9000]]
    R, Dg = [torch.from_numpy(v) for v in refs], [torch.from_numpy(v).to(dev) for v in degs]     # host and device rows mixed
    table = metrics.mcd_table(sr, dev)
    with torch.cuda.device(dev):
        xr, yr = metrics._stage(R, Dg, dev, cut=False)
        c = ops.cepstra(xr + yr, table, ldf=16)
    cep, frames = c["cep"].cpu().numpy(), c["frames"].cpu().tolist()
    assert frames == c["counts"] == [1 + len(v) // 160 for v in refs + degs]
    t = make_table(sr, 512, 160, 80)
    bank = mcd_ref.dense_bank(t["first"], t["count"], t["off"], t["w"], 257)
    worst = 0.0
    for dtw, band_ms, band in ((True, None, 0), (True, 300.0, 30), (False, None, 0)):
        got = metrics.mcd(R, Dg, sample_rate=sr, dtw=dtw, band_ms=band_ms, path=True, device=dev)
        assert set(got) == {"mcd", "frames_ref", "frames_deg", "steps", "path"} and all(v.device == dev for v in got.values())
        for b in range(4):
            cx, cy = cep[b, :frames[b], :13], cep[4 + b, :frames[4 + b], :13]
            want = ref.dtw(cx, cy, band=band, mode="warp" if dtw else "diagonal")
            n = int(want["info"][0])
            assert [int(got[k][b]) for k in ("steps", "frames_ref", "frames_deg")] == want["info"].tolist()[:3]
            assert np.array_equal(got["path"][b, :n].cpu().numpy(), want["path"]) and not got["path"][b, n:].any()
            db = np.float32(want["mean"]) * np.float32(metrics.MCD_DB)
            assert got["mcd"][b].cpu().numpy().tobytes() == db.tobytes(), (dtw, b, float(got["mcd"][b]), db)
            if band == 0:
                fx, fy = mcd_ref.cepstra(refs[b], 512, 160, bank, t["dct"]), mcd_ref.cepstra(degs[b], 512, 160, bank, t["dct"])
                if dtw:
                    total, steps = mcd_ref.dtw_float64(fx, fy)
                    exact = mcd_ref.MCD_DB * total / steps
                else:
                    m = min(len(fx), len(fy))
                    exact = mcd_ref.mcd_float64(fx, fy, np.repeat(np.arange(m)[:, None], 2, 1))
                err = abs(float(got["mcd"][b]) - exact)
                print(f"dtw={dtw} pair {b}: {float(got['mcd'][b]):.5f} dB, all-float64 {exact:.5f} dB, |difference| {err:.2e}")
                worst = max(worst, err)
    assert worst <= MCD_BOUND_DB, worst
    empty = metrics.mcd([], [], device=dev)
    assert all(empty[k].numel() == 0 for k in ("mcd", "frames_ref", "frames_deg", "steps"))


def test_known_answers():
    """x against x is exactly 0.0 dB either way.  A speech-like signal against itself with 5 % of its hops played twice: without
    DTW frame t of one faces frame t of the other up to ten hops (100 ms) apart, so plain MCD is that of two different stretches
    of speech, several dB; DTW pays only at the frames whose window straddles a repeated hop (two or three of every twenty), and
    there a part of the distance: a small fraction of the plain value.  Asserted: plain > 2 dB, DTW < plain / 4."""
    from simwhisper_codec_amd import metrics
    dev = device()
    xs = [torch.from_numpy(speech(k)) for k in (1, 2)]
    for dtw in (True, False):
        same = metrics.mcd(xs, xs, dtw=dtw, device=dev)
        assert same["mcd"].tolist() == [0.0, 0.0] and same["steps"].tolist() == same["frames_ref"].tolist() == [1 + len(x) // 160 for x in xs]
    ys = [torch.from_numpy(duplicated(x.numpy(), 160, seed=k)) for k, x in enumerate(xs)]
    warped, plain = metrics.mcd(xs, ys, device=dev), metrics.mcd(xs, ys, dtw=False, device=dev)
    print("5 % of the hops played twice: MCD-DTW", warped["mcd"].tolist(), "dB, plain MCD", plain["mcd"].tolist(), "dB; steps",
          warped["steps"].tolist(), "frames", warped["frames_ref"].tolist(), warped["frames_deg"].tolist())
    assert (plain["mcd"] > 2.0).all() and (warped["mcd"] < plain["mcd"] / 4).all()
    assert (warped["frames_deg"] > warped["frames_ref"]).all() and (warped["steps"] >= warped["frames_deg"]).all()
    assert plain["steps"].tolist() == plain["frames_ref"].tolist()
    f = metrics.dtw([torch.from_numpy(make_pair(65, 255, 13, 3, 0)[0])], [torch.from_numpy(make_pair(65, 255, 13, 3, 0)[1]).to(dev)], band=2)
    want = reference(*make_pair(65, 255, 13, 3, 0), 2, "warp")
    assert int(f["total"][0]) == want["total"] and int(f["steps"][0]) == want["info"][0]
    assert np.array_equal(f["path"][0, :want["info"][0]].cpu().numpy(), want["path"])


def test_alignment_composes_and_the_tool_runs(tmp_path, capsys):
    import align_ref
    from simwhisper_codec_amd import metrics, wavio
    dev = device()
    x = speech(1)
    x2 = speech(2)
    pairs = [(x, (0.8 * align_ref.delayed(x, 37, n=len(x) + 50)).astype(np.float32)),
             (x2, (align_ref.delayed(x2, -12) + noise(len(x2), 9, 0.003)).astype(np.float32))]
    refs, degs = [torch.from_numpy(a) for a, _ in pairs], [torch.from_numpy(b).to(dev) for _, b in pairs]
    got = metrics.mcd(refs, degs, align="waveform", max_lag_ms=10.0, device=dev)
    xs, ys, a = metrics.aligned(refs, degs, max_lag_ms=10.0, device=dev)
    want = metrics.mcd(xs, ys, device=dev)
    assert set(got) == set(want) | {"lag"} and got["lag"].tolist() == a["lag"].tolist() == [37, -12]
    for k in want:
        assert poison.same_bits(got[k].cpu().contiguous(), want[k].cpu().contiguous()), k
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_mcd
    os.makedirs(tmp_path / "orig"); os.makedirs(tmp_path / "syn")
    for i, (u, v) in enumerate(pairs):
        wavio.save_audio(str(tmp_path / "orig" / f"utt{i}.wav"), torch.from_numpy(u), 16000)
        wavio.save_audio(str(tmp_path / "syn" / f"utt{i}.wav"), torch.from_numpy(v), 16000)
    args = ["--original_dir", str(tmp_path / "orig"), "--synthesized_dir", str(tmp_path / "syn"), "--batch_size", "2", "--verbose"]
    assert evaluate_mcd.main(args + ["--align", "waveform", "--max_lag_ms", "10", "--band_ms", "500"]) == 0
    out = capsys.readouterr().out
    assert evaluate_mcd.main(args + ["--no_dtw"]) == 0
    plain = capsys.readouterr().out
    print(out, plain)
    assert "alignment: mean |lag| 24.500 samples, largest |lag| 37" in out and "not aligned" not in out
    assert "mean MCD-DTW:" in out and "utt1.wav: MCD-DTW" in out and "over 2 pairs" in out
    assert "alignment" not in plain and "mean MCD:" in plain and "over 2 pairs" in plain


def test_audiocodec_mcd_on_the_synthetic_checkpoint():
    """model.mcd(wavs) is metrics.mcd of the model's own reconstruction against the input, bit for bit, and dtw=, band_ms= and
    path= reach it"""
    import common
    from simwhisper_codec_amd import metrics, synth
    from simwhisper_codec_amd.codec import AudioCodec
    dev = device()
    model = AudioCodec(common.tiny_params(), precision="fp32")
    model.load_state_dict(common.state_dict("tiny"), strict=True)
    wavs = [synth.synth_audio(18000, index=0, kind="speech"), synth.synth_audio(17000, index=1, kind="speech")]
    with pytest.raises(metrics.SwcError, match=r"^mcd: the metrics are HIP kernels \(there is no CPU fallback\)$"):
        model.mcd(wavs, device="cpu")                                 # the model is still on the host
    model = model.to(dev).eval()
    wavs = [w.to(dev) for w in wavs]
    syn = model.decode(model.encode(wavs)["codes_list"])["syn_wav_list"]
    got = {}
    for name, kw in (("warped", {}), ("plain", {"dtw": False}), ("path", {"path": True}), ("band", {"band_ms": 200.0, "path": True})):
        got[name] = model.mcd(wavs, **kw)
        want = metrics.mcd(wavs, syn, sample_rate=model.input_sample_rate, device=dev, **kw)
        assert set(got[name]) == set(want) == {"mcd", "frames_ref", "frames_deg", "steps"} | ({"path"} if kw.get("path") else set()), name
        for k in want:
            assert got[name][k].device == dev and poison.same_bits(got[name][k].cpu().contiguous(), want[k].cpu().contiguous()), (name, k)
    warped, plain = got["warped"], got["plain"]
    H = metrics.mcd_params(model.input_sample_rate)[1]
    assert warped["mcd"].shape == (2,) and warped["mcd"].dtype == torch.float32 and not torch.isnan(warped["mcd"]).any()
    assert warped["frames_ref"].tolist() == [1 + 18000 // H, 1 + 17000 // H]
    assert plain["steps"].tolist() == torch.minimum(plain["frames_ref"], plain["frames_deg"]).tolist()      # dtw=False: the diagonal
    assert (warped["steps"] >= torch.maximum(warped["frames_ref"], warped["frames_deg"])).all()            # dtw=True: a path
    assert poison.same_bits(got["path"]["mcd"].cpu(), warped["mcd"].cpu()) and got["path"]["path"].shape[0] == 2
