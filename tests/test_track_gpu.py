"""swc_lag_track, swc_lag_fit and swc_warp on the GPU against the numpy restatement of include/swc_track.h (tests/track_ref.py).
swc_lag_track: every c_k[d], the status and the segment count equal; lag, rho, weight and centre within 1e-12 relative (both sides
run the same individually rounded float64 chain over the same table; a wrong d* moves lag, rho and the centre, so d* is
checked through them and through the status).  swc_lag_fit: a, b, rms within 1e-12 relative, counts and flags equal.  swc_warp:
within the bound of its f32 chain of the float64 evaluation of the same table, x0 and m equal.  Then bit independence of
everything that is not the pair, the memory contract under three fills, not-defined pairs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_ref  # noqa: E402
import poison  # noqa: E402
import track_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

POISON_ADDRESS = 0x10       # the "address" of the rows of an empty pair: never dereferenced
OUTPUTS = ("vals", "status", "nseg", "xc")
DTYPES = {"vals": torch.float64, "status": torch.int32, "nseg": torch.int32, "xc": torch.int64}
TOP = np.float32(1.9999999)  # the largest f32 below 2: q = 32767
REL = 1e-12
_CACHE = {}
P = lambda t: C.c_void_p(t.data_ptr())


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def signal(n, seed):
    rng = np.random.default_rng(seed)
    return (0.3 * rng.standard_normal(n) * (0.2 + np.abs(np.sin(np.arange(n) / 300.0 + seed)))).astype(np.float32)


def make_pair(nx, ny, d, seed, gain=0.6, noise=0.003):
    """x of nx samples and y of ny samples = gain x delayed by d, smoothed a little so that the peak has a shape, plus noise"""
    x = signal(nx + 2, seed)
    x = (0.25 * x[:-2] + 0.5 * x[1:-1] + 0.25 * x[2:]).astype(np.float32)
    y = (gain * align_ref.delayed(x, d, n=ny) + noise * np.random.default_rng(1000 + seed).standard_normal(ny)).astype(np.float32)
    return x, y


def reference(key, x, y, d0, S, H, Rs, mode):
    k = (key, d0, S, H, Rs, mode)
    if k not in _CACHE:
        _CACHE[k] = ref.lag_track(x, y, d0, S, H, Rs, mode)
    return _CACHE[k]


def upload_rows(pairs, offsets=None):
    """-> (keep, ptrs_x, ptrs_y, n_x, n_y): rows offsets[b] elements behind a 16-byte boundary, empty pairs behind a poison address"""
    offsets = offsets or [(0, 0)] * len(pairs)
    keep, ptrs_x, ptrs_y, n_x, n_y = [], [], [], [], []
    for (x, y), offs in zip(pairs, offsets):
        n_x.append(len(x))
        n_y.append(len(y))
        for v, ptrs, off in ((x, ptrs_x, offs[0]), (y, ptrs_y, offs[1])):
            if len(x) == 0 or len(y) == 0:
                ptrs.append(POISON_ADDRESS)
                continue
            buf = torch.full((len(v) + off,), float("nan"), device=dev())
            assert buf.data_ptr() % 16 == 0
            buf[off:] = torch.from_numpy(np.ascontiguousarray(v))
            keep.append(buf)
            ptrs.append(buf.data_ptr() + 4 * off)
    return keep, ptrs_x, ptrs_y, n_x, n_y


def run_track(pairs, d0s, S, H, Rs, mode, want=OUTPUTS, fill="nan", offsets=None, max_nx=None, max_ny=None, ldk=None, ldc=None, ld_d0=1):
    """one swc_lag_track call on guarded, pre-filled outputs and workspace -> dict of host tensors for the wanted outputs, "K"
    and "before".  Outputs that were not asked for must keep their fill; nothing may be written outside the windows."""
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    B = len(pairs)
    keep, ptrs_x, ptrs_y, n_x, n_y = upload_rows(pairs, offsets)
    max_nx = max(n_x) if max_nx is None else max_nx
    max_ny = max(n_y) if max_ny is None else max_ny
    K = ops.track_segments(max_nx, S, H)
    nl = 2 * (Rs + 17) + 1
    ldk = max(K, 1) if ldk is None else ldk
    ldc = nl if ldc is None else ldc
    need = ops.lag_track_workspace_bytes(B, max_nx, max_ny, S, H, Rs)
    shapes = {"vals": (B, ldk * 4), "status": (B, ldk), "nseg": (B, 1), "xc": (B * ldk, ldc)}
    outs, checks = {}, []
    for name in OUTPUTS:
        outs[name], chk = poison.guarded(shapes[name], DTYPES[name], device=dev(), band_rows=4)
        outs[name].zero_() if fill == "zero" else poison.fill_(outs[name], fill)
        checks.append(chk)
    before = {k: v.cpu().clone() for k, v in outs.items()}
    ws, check_w = poison.guarded((max(need // 256, 1), 256), torch.uint8, device=dev(), band_rows=16)
    assert ws.is_contiguous() and ws.data_ptr() % 256 == 0 and need % 256 == 0
    ws.zero_() if fill == "zero" else poison.fill_(ws.view(torch.float32), fill)
    meta = torch.tensor(ptrs_x + ptrs_y + n_x + n_y, dtype=torch.int64).to(dev())
    d0 = torch.full((B, ld_d0), 12345, dtype=torch.int32)
    d0[:, 0] = torch.tensor(d0s, dtype=torch.int32)
    d0 = d0.to(dev())
    table = ops._track_tables(dev())[0]
    arg = lambda name: P(outs[name]) if name in want else None
    rc = lib.swc_lag_track(P(meta[:B]), P(meta[B:2 * B]), P(meta[2 * B:3 * B]), P(meta[3 * B:]), max_nx, max_ny, P(d0), ld_d0, S, H, Rs,
                           ops.ALIGN_MODES[mode], P(table), arg("vals"), arg("status"), ldk, arg("nseg"), arg("xc"), ldc, P(ws), need,
                           B, ops._stream())
    _lib.check(rc, "swc_lag_track")
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    check_w()
    res = {"before": before, "K": K, "ldk": ldk, "nl": nl}
    for name in OUTPUTS:
        got = outs[name].cpu().clone()
        if name in want:
            res[name] = got
        else:
            assert poison.same_bits(got, before[name]), f"{name} was not asked for and was written"
    del keep
    return res


def close(got, want):
    """within 1e-12 relative; NaN matches NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - want) <= REL * np.abs(want)
    return bool((ok | both_nan).all())


def compare_track(res, b, want, what):
    """pair b of a call against its reference dict; slots at and beyond the pair's K hold "none" up to the call's K and keep
    the fill beyond; columns of xc at and beyond 2 R + 1 keep the fill"""
    K, ldk, nl = res["K"], res["ldk"], res["nl"]
    kb = len(want["status"])
    if "nseg" in res:
        assert int(res["nseg"][b, 0]) == kb, what
    if "xc" in res:
        xc = res["xc"].view(-1, ldk, res["xc"].shape[1])[b]
        assert np.array_equal(xc[:kb, :nl].numpy(), want["xc"]), what
        assert not xc[kb:K, :nl].any(), what
        fill = res["before"]["xc"].view(-1, ldk, xc.shape[1])[b]
        assert poison.same_bits(xc[K:].contiguous(), fill[K:].contiguous()) and poison.same_bits(xc[:, nl:].contiguous(), fill[:, nl:].contiguous()), what
    if "status" in res:
        st = res["status"][b]
        assert np.array_equal(st[:kb].numpy(), want["status"]), (what, st[:kb], want["status"])
        assert not st[kb:K].any() and poison.same_bits(st[K:].contiguous(), res["before"]["status"][b, K:].contiguous()), what
    if "vals" in res:
        v = res["vals"][b].view(ldk, 4)
        assert close(v[:kb].numpy(), want["vals"]), (what, v[:kb].numpy() - want["vals"])
        none = v[kb:K].numpy()
        assert np.isnan(none[:, [0, 1, 3]]).all() and not none[:, 2].any(), what
        assert poison.same_bits(v[K:].contiguous(), res["before"]["vals"][b].view(ldk, 4)[K:].contiguous()), what


# (S, H, Rs, mode, [(nx, ny, true delay, d0)]): the smallest shapes that reach each branch.  S round the chunk (4096, 4097: a
# segment of two chunks); H = S, S / 2, 3; Rs = 0, 1, 8, 128, 1024 (1, 2 and 9 lag blocks); rows of 1, 2, W, 2 W + 3, S - 1, S,
# S + 1, 2 S + 17 samples with nx != ny; d0 that puts a segment's y span partly and wholly outside the row; d0 = +-L = +-32768
def track_cases():
    W = ref.W
    S = 256
    lengths = [1, 2, W, 2 * W + 3, S - 1, S, S + 1, 2 * S + 17]
    many = []
    for i in range(33):                                # B = 33
        nx = lengths[i % 8]
        ny = max(1, nx + (5, -3, 9, -1)[i % 4])
        d = (0, 3, -2, 5, -6)[i % 5]
        d0 = d + (0, 1, -1, 2, -3, 0, 7)[i % 7]       # within and at the edge of Rs = 8
        many.append((nx, ny, d, d0))
    many[8] = (2 * S + 17, 300, 0, 200)                # the later segments' y span partly outside the row
    many[9] = (2 * S + 17, 100, 0, -400)               # wholly outside for the first segment
    many[10] = (2 * S + 17, 500, 0, 32768)             # d0 = +L
    many[11] = (2 * S + 17, 500, 0, -32768)            # d0 = -L
    yield (S, S, 8, "waveform", many)
    yield (S, S // 2, 1, "envelope", [(S + 1, S + 9, 1, 1), (2 * S + 17, 2 * S, -1, 0), (S - 1, S + 2, 0, 0)])   # B = 3
    yield (S, 3, 0, "waveform", [(2 * S + 17, 2 * S + 11, 2, 2)])                                            # B = 1, 92 segments
    yield (4096, 2048, 128, "waveform", [(4095, 4099, 40, 30), (4097, 4090, -100, -60), (2 * 4096 + 17, 8300, 7, 0)])
    yield (4097, 4097, 1024, "envelope", [(2 * 4097 + 17, 8100, -700, 100)])
    yield (0, 0, 8, "waveform", [(1, 4, 0, 0), (2 * W + 3, 30, 3, 2), (9000, 9100, 33, 30)])                 # three chunks


@pytest.mark.parametrize("case", list(track_cases()), ids=lambda c: f"S{c[0]}-H{c[1]}-Rs{c[2]}-{c[3]}-B{len(c[4])}")
def test_lag_track_against_the_reference(case):
    S, H, Rs, mode, specs = case
    pairs = [make_pair(nx, ny, d, 7 * i + nx) for i, (nx, ny, d, _) in enumerate(specs)]
    d0s = [s[3] for s in specs]
    res = run_track(pairs, d0s, S, H, Rs, mode, ldc=2 * (Rs + 17) + 4)
    defined = 0
    for b, ((x, y), d0) in enumerate(zip(pairs, d0s)):
        want = reference(("case", S, H, b, len(x), len(y)), x, y, d0, S, H, Rs, mode)
        compare_track(res, b, want, (case[:4], b, specs[b]))
        defined += int((want["status"] & 1).sum())
    assert defined > 0


def test_full_scale_square_waves_longer_than_the_spill_interval():
    """every product is +-32767^2 over 5000 samples: an int32 accumulator that was not spilled would wrap after 2 samples"""
    n = 5000
    sq = np.where((np.arange(n) // 37) % 2 == 0, TOP, -TOP).astype(np.float32)
    pairs = [(sq, sq.copy()), (sq, -sq)]
    res = run_track(pairs, [0, 0], 0, 0, 8, "waveform")
    for b, (x, y) in enumerate(pairs):
        want = ref.lag_track(x, y, 0, 0, 0, 8, "waveform")
        compare_track(res, b, want, b)
    assert int(res["xc"][0, 25]) == n * 32767 ** 2 and int(res["xc"][1, 25]) == -n * 32767 ** 2
    assert int(res["status"][0, 0]) & 1


def test_shift_equivariance_and_the_edge_bit():
    """the same pair cut d samples later: lag_k moves by exactly d while d0 follows; with d0 left behind the peak reaches the
    edge of +-Rs and the status says so"""
    x, y = make_pair(1500, 1500, 4, 3)
    base = run_track([(x, y)], [4], 512, 256, 8, "waveform")
    k = int(base["nseg"][0, 0])
    assert k == 5 and (base["status"][0, :k] == 1).all()
    for d in (-7, 1, 20):
        yd = align_ref.delayed(y, d)
        r = run_track([(x, yd)], [4 + d], 512, 256, 8, "waveform")
        lag0, lag1 = base["vals"][0].view(-1, 4)[1:k - 1, 0], r["vals"][0].view(-1, 4)[1:k - 1, 0]   # segments that lose no sample
        assert close((lag1 - d).numpy(), lag0.numpy()), d
    r = run_track([(x, align_ref.delayed(y, 8))], [4], 512, 256, 8, "waveform")
    assert (r["status"][0, :k] == 3).all()


def batch_for_bits():
    specs = [(700, 690, 3, 2), (0, 50, 0, 0), (300, 310, -2, 0), (50, 0, 0, 0), (257, 255, 0, 1), (1, 1, 0, 0), (600, 640, 5, 5)]
    return [make_pair(nx, ny, d, 11 + i) if nx and ny else (signal(nx, i), signal(ny, i)) for i, (nx, ny, d, _) in enumerate(specs)], [s[3] for s in specs]


def pair_bits(res, b):
    K, ldk, nl = res["K"], res["ldk"], res["nl"]
    parts = []
    if "vals" in res:
        parts.append(res["vals"][b].view(ldk, 4)[:K])     # slots at and beyond K keep the fill
    if "status" in res:
        parts.append(res["status"][b, :K])
    out = [p.contiguous().view(torch.uint8).numpy().tobytes() for p in parts]
    if "nseg" in res:
        out.append(res["nseg"][b].numpy().tobytes())
    if "xc" in res:
        out.append(res["xc"].view(-1, ldk, res["xc"].shape[1])[b, :K, :nl].contiguous().numpy().tobytes())
    return out


def test_bit_independence_of_everything_that_is_not_the_pair():
    """B, the order, addresses 0 - 7 elements behind a 16-byte boundary, the bounds, the strides and the subset of outputs;
    empty pairs sit behind a poison address"""
    pairs, d0s = batch_for_bits()
    S, H, Rs = 256, 128, 8
    for mode in ("waveform", "envelope"):
        base = run_track(pairs, d0s, S, H, Rs, mode, max_nx=700, max_ny=690)
        K = base["K"]
        assert base["nseg"][:, 0].tolist() == [5, 0, 2, 0, 2, 1, 4]
        want = [pair_bits(base, b) for b in range(len(pairs))]
        # one pair alone, at every offset
        for off in range(8):
            r = run_track([pairs[0]], [d0s[0]], S, H, Rs, mode, offsets=[(off, 7 - off)])
            assert pair_bits(r, 0) == want[0], (mode, off)
        # reversed order, other bounds and strides, a wider d0
        order = list(range(len(pairs)))[::-1]
        r = run_track([pairs[i] for i in order], [d0s[i] for i in order], S, H, Rs, mode, max_nx=900, max_ny=4000, ldk=K + 3, ldc=2 * (Rs + 17) + 6,
                      ld_d0=4, fill="big")
        assert r["K"] >= K
        for pos, i in enumerate(order):
            got = pair_bits(dict(r, K=K, vals=r["vals"].view(len(pairs), -1, 4)[:, :K].reshape(len(pairs), -1), status=r["status"][:, :K],
                                 xc=r["xc"].view(len(pairs), K + 3, -1)[:, :K].reshape(len(pairs) * K, -1), ldk=K), pos)
            assert got == want[i], (mode, i)
        # every subset of outputs
        for want_set in (("vals",), ("status",), ("nseg",), ("xc",), ("vals", "xc"), ()):
            r = run_track(pairs, d0s, S, H, Rs, mode, want=want_set, max_nx=700, max_ny=690)
            for b in range(len(pairs)):
                sub = pair_bits({k: v for k, v in base.items() if k in want_set or k in ("K", "ldk", "nl")}, b)
                assert pair_bits(r, b) == sub, (mode, want_set, b)


def test_memory_contract_and_fill_independence():
    pairs, d0s = batch_for_bits()
    res = [run_track(pairs, d0s, 256, 128, 8, "envelope", fill=f, ldc=60, ldk=8) for f in ("nan", "big", "zero")]
    for b in range(len(pairs)):
        assert pair_bits(res[0], b) == pair_bits(res[1], b) == pair_bits(res[2], b)
        x, y = pairs[b]
        compare_track(res[0], b, reference(("bits", b), x, y, d0s[b], 256, 128, 8, "envelope"), b)


def test_nan_and_inf_pairs_are_not_defined_and_touch_no_other_pair():
    pairs, d0s = batch_for_bits()
    base = run_track(pairs, d0s, 256, 128, 8, "waveform")
    for bad in (np.nan, np.inf, -np.inf):
        for side in (0, 1):
            broken = [list(p) for p in pairs]
            v = broken[2][side].copy()
            v[17] = bad
            broken[2][side] = v
            r = run_track([tuple(p) for p in broken], d0s, 256, 128, 8, "waveform")
            assert int(r["nseg"][2, 0]) == 0 and not r["status"][2, :r["K"]].any()
            assert not r["xc"].view(len(pairs), r["ldk"], -1)[2, :r["K"]].any()
            assert np.isnan(r["vals"][2].view(-1, 4)[:r["K"], 0].numpy()).all()
            for b in (0, 1, 3, 4, 5, 6):
                assert pair_bits(r, b) == pair_bits(base, b), (bad, side, b)


# ---- swc_lag_fit ----

def fit_tracks():
    """[(vals [K][4], status [K], d0)]: 0, 1, 2 and many usable segments; outliers beyond one sample; low and NaN rho; edge bits;
    undefined slots; two usable segments at one centre"""
    rng = np.random.default_rng(5)
    nan = np.nan

    def track(K, a, b, jitter=0.01, rho=0.9):
        t = 8000.0 * np.arange(K) + 7999.5
        lag = a + b * t + jitter * rng.standard_normal(K)
        w = rng.integers(1 << 30, 1 << 44, K).astype(np.float64)
        return np.stack([lag, np.full(K, rho), w, t], axis=1), np.ones(K, np.int32)

    out = []
    v, s = track(19, 12.3, 50e-6)
    out.append((v, s, 12))
    v, s = track(19, -5.6, -200e-6)
    v[[3, 11], 0] += (2.5, -1.7)                       # outliers: out in the second pass
    s[5] = 3                                           # an edge peak among the used
    v[7, 1] = 0.1                                      # below rho_min
    v[9] = (nan, nan, 0.0, nan)
    s[9] = 0                                           # not defined
    out.append((v, s, -6))
    v, s = track(2, 3.25, 1e-5)
    out.append((v, s, 3))                              # two usable
    v, s = track(1, 3.25, 0.0)
    out.append((v, s, 3))                              # one: a lag, no drift
    v, s = track(4, 1.0, 0.0)
    s[:] = 0
    out.append((v, s, 9))                              # none
    v, s = track(3, 1.0, 0.0)
    v[:, 3] = 500.0
    out.append((v, s, -4))                             # three at one centre: stt == 0
    v, s = track(6, 0.0, 0.0, rho=0.2)
    out.append((v, s, 1))                              # all below rho_min
    v, s = track(5, 2.0, 0.0)
    v[1:, 0] += 40.0
    v[0, 2] = 2.0 ** 50                                # a heavy first segment far from the rest: the second pass keeps it alone
    out.append((v, s, 2))
    out.append((np.zeros((0, 4)), np.zeros(0, np.int32), 5))   # no segment at all
    v, s = track(6, 1.5, 0.0)
    s[2] = 3
    out.append((v, s, 1))                              # a constant lag with an edge peak among the used: flag 4 with and without drift
    return out


@pytest.mark.parametrize("drift", [True, False])
def test_lag_fit_against_the_reference(drift):
    from simwhisper_codec_amd import _lib
    lib = _lib.load()
    tracks = fit_tracks()
    B, ldk = len(tracks), 24
    vals = torch.full((B, ldk, 4), float("nan"), dtype=torch.float64)
    status = torch.full((B, ldk), 1, dtype=torch.int32)     # slots beyond nseg look usable: they must not be read
    nseg = torch.zeros(B, dtype=torch.int32)
    d0 = torch.zeros((B, 4), dtype=torch.int32)
    for b, (v, s, d) in enumerate(tracks):
        vals[b, :len(v)] = torch.from_numpy(v)
        vals[b, len(v):] = torch.tensor([1.0, 1.0, 1.0, 1.0], dtype=torch.float64)
        status[b, :len(s)] = torch.from_numpy(s)
        nseg[b], d0[b, 0] = len(s), d
    vals, status, nseg, d0 = (t.to(dev()) for t in (vals, status, nseg, d0))
    for fill in ("nan", "big"):
        fit, chk_f = poison.guarded((B, 4), torch.float64, device=dev(), band_rows=8)
        cnt, chk_c = poison.guarded((B, 4), torch.int32, device=dev(), band_rows=8)
        poison.fill_(fit, fill)
        poison.fill_(cnt, fill)
        from simwhisper_codec_amd import ops
        _lib.check(lib.swc_lag_fit(P(vals), P(status), ldk, P(nseg), ldk, P(d0), 4, 0.3, int(drift), P(fit), P(cnt), B, ops._stream()), "swc_lag_fit")
        torch.cuda.synchronize()
        chk_f()
        chk_c()
        fit, cnt = fit.cpu(), cnt.cpu()
        seen = set()
        for b, (v, s, d) in enumerate(tracks):
            want = ref.lag_fit(v, s, d, 0.3, drift)
            assert cnt[b].tolist() == [want["used"], want["offered"], want["flags"], 0], (b, cnt[b], want)
            assert close(fit[b, :3].numpy(), [want["a"], want["b"], want["rms"]]), (b, fit[b], want)
            assert float(fit[b, 3]) == 0.0
            seen.add(want["flags"])
        assert {0, 4}.issubset(seen) and ({1, 3}.issubset(seen) if drift else 2 in seen)


# ---- swc_warp ----

def run_warp(ys, n_x, ab, cols, fill="nan", ld_out=None, ld_fit=2, offsets=None, max_nx=None, max_ny=None):
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    B = len(ys)
    keep, _, ptrs_y, _, n_y = upload_rows([(y, y) for y in ys], [(o, o) for o in (offsets or [0] * B)])   # an empty row: a poison address
    ld_out = max(cols, 1) if ld_out is None else ld_out
    out, chk_o = poison.guarded((B, cols), torch.float32, ld=ld_out, device=dev(), band_rows=4)
    info, chk_i = poison.guarded((B, 4), torch.int32, device=dev(), band_rows=8)
    poison.fill_(info, "nan")
    if cols:
        out.zero_() if fill == "zero" else out.fill_(float("nan") if fill == "nan" else poison.BIG)
    fit = torch.full((B, ld_fit), 7.0, dtype=torch.float64)
    fit[:, :2] = torch.tensor(ab, dtype=torch.float64)
    fit = fit.to(dev())
    meta = torch.tensor(ptrs_y + list(n_x) + n_y, dtype=torch.int64).to(dev())
    table = ops._track_tables(dev())[1]
    first = out.data_ptr() if cols else info.data_ptr()
    rc = lib.swc_warp(P(meta[:B]), P(meta[B:2 * B]), P(meta[2 * B:]), max(n_x) if max_nx is None else max_nx,
                      max(n_y) if max_ny is None else max_ny, P(fit), ld_fit, P(table), C.c_void_p(first), ld_out, cols, P(info), B, ops._stream())
    _lib.check(rc, "swc_warp")
    torch.cuda.synchronize()
    chk_o()
    chk_i()
    del keep
    return out.cpu().clone(), info.cpu().clone()


# Why 34 * 2^-24 * sum_t |h_t y_t|.  With u = 2^-24, the kernel's out is a chain of 32 fmaf: each adds h_t y_t exactly and
# rounds once, so the computed sum is sum_t h_t y_t (1 + e_t) with |e_t| <= (1 + u)^32 - 1 (the first term passes 32 roundings):
# at most 32 u (1 + 16 u) sum |h_t y_t|.  The reference forms h_t from the same f32 table entries through the same two f32
# roundings (the difference of the two rows, then the fused multiply-add), emulated in float64 where the second can round
# twice: one more u on a term.  32 u + u + the float64 dot product's own 2^-48 stay below 34 u.
WARP_BOUND = 34.0 * 2.0 ** -24


@pytest.mark.parametrize("cols", [0, 1, 255, 256, 257, 700])
def test_warp_against_the_float64_evaluation(cols):
    rng = np.random.default_rng(cols)
    ab = [(0.0, 0.0), (3.25, 0.0), (-7.5, 1e-4), (12.3, -1e-4), (-5.6, 1e-2), (40.25, -1e-2), (-900.0, 0.0), (900.0, 1e-4), (0.5, 0.02),
          (float("nan"), 0.0), (1e9, 0.0), (-300.0, 1e-2)]
    n_x = [700, 300, 650, 257, 700, 400, 700, 700, 300, 300, 300, 1]
    ys = [(0.5 * rng.standard_normal(n)).astype(np.float32) for n in (700, 280, 700, 300, 512, 450, 600, 650, 300, 300, 300, 320)]
    out, info = run_warp(ys, n_x, ab, cols, ld_out=cols + 5, ld_fit=4, offsets=[i % 8 for i in range(len(ys))])
    nonempty = 0
    for b, (y, nx, (a, bb)) in enumerate(zip(ys, n_x, ab)):
        want = ref.warp(y, a, bb, nx, cols)
        assert info[b].tolist() == [want["x0"], want["m"], want["flag"], 0], (b, info[b], want["x0"], want["m"])
        if cols == 0:
            continue
        got = out[b].numpy().astype(np.float64)
        assert np.isfinite(got).all()
        assert (np.abs(got - want["out"]) <= WARP_BOUND * want["bound"]).all(), (b, np.abs(got - want["out"]).max())
        assert not got[want["m"]:].any()
        nonempty += want["m"] > 0
    if cols:
        assert nonempty >= 6
        assert info[6].tolist()[:2] == [0, 0] and info[8, 2] == 1 and info[9, 2] == 1 and info[10, 2] == 1   # beyond the row; refused


def test_warp_bits_do_not_depend_on_the_batch_or_the_fill():
    rng = np.random.default_rng(3)
    ys = [(0.5 * rng.standard_normal(n)).astype(np.float32) for n in (600, 0, 300)]
    n_x, ab = [600, 50, 310], [(12.3, 50e-6), (0.0, 0.0), (-5.6, -200e-6)]
    base, info = run_warp(ys, n_x, ab, 600)
    assert info[1].tolist() == [0, 0, 0, 0] and not base[1].any()
    for fill, off in (("big", 3), ("zero", 7)):
        for b in (0, 2):
            o, i = run_warp([ys[b]], [n_x[b]], [ab[b]], 600, fill=fill, ld_out=777, offsets=[off], max_nx=4000, max_ny=9000)
            assert poison.same_bits(o[0], base[b]) and torch.equal(i[0], info[b]), (fill, b)


# ---- the three calls chained through ops, on an analytic pair ----

def test_ops_chain_on_an_analytic_pair():
    """align -> lag_track -> lag_fit -> warp through the ops wrappers, nothing read back in between: the same numbers as the
    reference chain (tests/track_ref.py pipeline) on 20000 samples with a = 12.3, 50 ppm"""
    from simwhisper_codec_amd import ops
    x, y = ref.analytic_pair(0, 20000, 12.3, 50e-6)
    want = ref.pipeline(x, y, 100, 4000, 2000, 32)
    xs, ys = [torch.from_numpy(x).to(dev())], [torch.from_numpy(y).to(dev())]
    al = ops.align(xs, ys, 100, "waveform", want=("info",))
    tr = ops.lag_track(xs, ys, al["info"], 4000, 2000, 32, "waveform")
    ft = ops.lag_fit(tr["vals"], tr["status"], tr["nseg"], al["info"])
    wp = ops.warp(ys, [len(x)], ft["fit"])
    torch.cuda.synchronize()
    assert int(al["info"][0, 0]) == want["d0"] and tr["K"] == 9
    f = want["fit"]
    assert close(ft["fit"][0, :3].cpu().numpy(), [f["a"], f["b"], f["rms"]])
    assert ft["counts"][0].tolist() == [f["used"], f["offered"], f["flags"], 0] == [9, 9, 0, 0]
    w = want["warp"]
    assert wp["info"][0].tolist() == [w["x0"], w["m"], 0, 0]
    got = wp["out"][0].cpu().numpy().astype(np.float64)
    assert (np.abs(got - w["out"]) <= WARP_BOUND * w["bound"]).all()


# ---- end to end: metrics and a tool ----

def test_quality_with_fine_drift_on_an_analytic_pair(capsys):
    """a = 12.3 samples, 50 ppm over 10 s: SI-SDR after the integer alignment alone is near 0 dB; with fine="drift" it is above
    the gate the CPU reference sets for this case (tests/test_track_cpu.py E2E_GATE_DB), and the fit is inside the group's gates"""
    import test_track_cpu as cpu
    from simwhisper_codec_amd import metrics
    x, y = cpu.analytic("a12.3+50ppm")
    xs, ys = [torch.from_numpy(x)], [torch.from_numpy(y)]
    q = metrics.quality(xs, ys, align="waveform", fine="drift", device=dev())
    coarse = metrics.quality(xs, ys, align="waveform", device=dev())
    sdr, before = float(q["si_sdr"][0]), float(coarse["si_sdr"][0])
    gate_a, gate_b, _ = cpu.GATES["clean", True]
    print(f"SI-SDR {before:.2f} dB at the integer lag, {sdr:.2f} dB after the warp; lag_fine {float(q['lag_fine'][0]):.6f}, drift {float(q['drift_ppm'][0]):.5f} ppm")
    assert sdr >= cpu.E2E_GATE_DB > before
    assert abs(float(q["lag_fine"][0]) - 12.3) <= gate_a and abs(float(q["drift_ppm"][0]) - 50.0) <= gate_b * 1e6
    assert set(q) == set(coarse) | {"lag_fine", "drift_ppm"} and int(q["lag"][0]) == int(coarse["lag"][0])
    # the same numbers as the reference chain
    want = cpu.run_case("a12.3+50ppm", "drift")
    a = metrics.align(xs, ys, fine="drift", device=dev())
    assert close([float(a["lag_fine"][0]), float(a["drift_ppm"][0]) / 1e6, float(a["residual"][0])], [want["fit"][k] for k in ("a", "b", "rms")])
    assert a["segments"][0].tolist() == [19, 19] and int(a["flags"][0]) == 0
    tr = metrics.lag_track(xs, ys, device=dev())[0]
    assert set(tr) == {"t", "lag", "corr", "status"} and tr["lag"].numel() == 19
    assert close(tr["lag"].cpu().numpy(), want["track"]["vals"][:, 0]) and close(tr["t"].cpu().numpy(), want["track"]["vals"][:, 3])


def test_fine_none_is_what_it_was():
    """without fine= the dicts, the views and the scores are those of the alignment alone, bit for bit"""
    from simwhisper_codec_amd import metrics
    pairs = [make_pair(20000, 20100, 37, 1), make_pair(18000, 17000, -12, 2)]
    xs, ys = [torch.from_numpy(p[0]) for p in pairs], [torch.from_numpy(p[1]) for p in pairs]
    a = metrics.align(xs, ys, device=dev())
    assert set(a) == set(metrics.ALIGN_KEYS) and a["lag"].tolist() == [37, -12]
    vx, vy, info = metrics.aligned(xs, ys, device=dev())
    assert set(info) == set(metrics.ALIGN_KEYS)
    for b, (x, y) in enumerate(pairs):
        x0, y0, m = (int(info[k][b]) for k in ("start_ref", "start_deg", "length"))
        assert torch.equal(vx[b].cpu(), torch.from_numpy(x[x0:x0 + m])) and torch.equal(vy[b].cpu(), torch.from_numpy(y[y0:y0 + m]))
    q = metrics.quality(xs, ys, align="waveform", device=dev())
    direct = metrics.quality(vx, vy, device=dev())
    assert set(q) == set(direct) | {"lag"}
    for k in direct:
        assert poison.same_bits(q[k].cpu(), direct[k].cpu()), k
    q2 = metrics.quality(xs, ys, align="waveform", fine=None, device=dev())
    assert all(poison.same_bits(q[k].cpu(), q2[k].cpu()) for k in q)
    # fine="lag" on the same pairs (integer delays): new tensors, the same lags
    wx, wy, fine = metrics.aligned(xs, ys, fine="lag", device=dev())
    assert [round(float(v)) for v in fine["lag_fine"]] == [37, -12] and not fine["drift_ppm"].any() and not fine["flags"].any()
    assert all(a_.numel() == b_.numel() for a_, b_ in zip(wx, wy)) and wy[0].data_ptr() != vy[0].data_ptr()


def test_evaluate_tool_prints_the_drift(tmp_path, capsys):
    import test_track_cpu as cpu
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_quality
    import re
    from simwhisper_codec_amd import wavio
    x, y = cpu.analytic("a12.3+50ppm")
    x, y = x * np.float32(0.5), y * np.float32(0.5)          # below full scale: the files are 16-bit PCM
    os.makedirs(tmp_path / "orig"); os.makedirs(tmp_path / "syn")
    wavio.save_audio(str(tmp_path / "orig" / "utt0.wav"), torch.from_numpy(x), 16000)
    wavio.save_audio(str(tmp_path / "syn" / "utt0.wav"), torch.from_numpy(y), 16000)
    args = ["--original_dir", str(tmp_path / "orig"), "--synthesized_dir", str(tmp_path / "syn")]
    assert evaluate_quality.main(args + ["--align", "waveform", "--align_fine", "drift"]) == 0
    out = capsys.readouterr().out
    m = re.search(r"fine alignment: mean \|drift\| ([0-9.]+) ppm", out)
    # the files are 16-bit: their rounding is far below the noise of the noisy group, whose drift gate is asked here
    assert m and abs(float(m.group(1)) - 50.0) <= cpu.GATES["noisy", True][1] * 1e6
    assert "no fine fit" not in out and "edge of the track" not in out
    assert evaluate_quality.main(args + ["--align", "waveform"]) == 0
    assert "fine alignment" not in capsys.readouterr().out
    print(out)
