"""swc_align on the GPU against the numpy restatement of include/swc_align.h (tests/align_ref.py): xc equal at every lag in
int64, info equal, values within one f32 ulp, in both modes; the sweep of lengths and ranges round the kernel's chunk and lag
block, the accumulator bounds, the int64 range, bit independence of everything that is not the pair, the memory contract,
not-defined pairs, and the Python surface down to a tool."""
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

import align_ref as ref  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu

POISON_ADDRESS = 0x10       # the "address" of the rows of an empty pair: never dereferenced
OUTPUTS = ("info", "values", "xc")
DTYPES = {"info": torch.int32, "values": torch.float32, "xc": torch.int64}
MODES = ("waveform", "envelope")
TOP = np.float32(1.9999999)  # the largest f32 below 2: q = 32767 where 1.0 gives 16384
_CACHE = {}


def consts():
    from simwhisper_codec_amd import _lib
    return _lib.ALIGN_CHUNK, _lib.ALIGN_LAG_BLOCK, _lib.ALIGN_SPILL


def signal(n, seed):
    """noise under a slow envelope at a moderate level: a sharp correlation peak in either mode"""
    rng = np.random.default_rng(seed)
    return (0.3 * rng.standard_normal(n) * (0.2 + np.abs(np.sin(np.arange(n) / 300.0 + seed)))).astype(np.float32)


def make_pair(nx, ny, d, seed, gain=0.6, noise=0.003):
    """x of nx samples and y of ny samples = gain x delayed by d, plus a little noise"""
    x = signal(nx, seed)
    y = (gain * ref.delayed(x, d, n=ny) + noise * np.random.default_rng(1000 + seed).standard_normal(ny)).astype(np.float32)
    return x, y


def reference(key, x, y, L, mode):
    """the reference of one pair, computed once per key"""
    k = (key, L, mode)
    if k not in _CACHE:
        _CACHE[k] = ref.align(x, y, L, mode)
    return _CACHE[k]


def run(pairs, L, mode, want=OUTPUTS, fill="nan", offsets=None, max_nx=None, max_ny=None, ldc=None):
    """one swc_align call on guarded, pre-filled outputs and workspace -> dict of host tensors for the wanted outputs plus
    "before" (the fill of every output).  offsets[b] = (ox, oy): the rows of pair b start that many elements into their
    (16-byte aligned) allocations.  Outputs that were not asked for must keep their fill; nothing may be written outside the
    windows."""
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    B = len(pairs)
    offsets = offsets or [(0, 0)] * B
    keep, ptrs_x, ptrs_y, n_x, n_y = [], [], [], [], []
    for (x, y), offs in zip(pairs, offsets):
        n_x.append(len(x))
        n_y.append(len(y))
        for v, ptrs, off in ((x, ptrs_x, offs[0]), (y, ptrs_y, offs[1])):
            if len(x) == 0 or len(y) == 0:
                ptrs.append(POISON_ADDRESS)
                continue
            buf = torch.full((len(v) + off,), float("nan"), device=dev)
            assert buf.data_ptr() % 16 == 0
            buf[off:] = torch.from_numpy(v)
            keep.append(buf)
            ptrs.append(buf.data_ptr() + 4 * off)
    max_nx = max(n_x) if max_nx is None else max_nx
    max_ny = max(n_y) if max_ny is None else max_ny
    ldc = 2 * L + 1 if ldc is None else ldc
    need = ops.align_workspace_bytes(B, max_nx, max_ny, L)
    shapes = {"info": (B, 4), "values": (B, 4), "xc": (B, ldc)}
    outs, checks = {}, []
    for name in OUTPUTS:
        outs[name], chk = poison.guarded(shapes[name], DTYPES[name], device=dev, band_rows=4 if name == "xc" else 256)
        outs[name].zero_() if fill == "zero" else poison.fill_(outs[name], fill)
        checks.append(chk)
    before = {k: v.cpu().clone() for k, v in outs.items()}
    ws, check_w = poison.guarded((max(need // 256, 1), 256), torch.uint8, device=dev, band_rows=16)
    assert ws.is_contiguous() and ws.data_ptr() % 256 == 0 and need % 256 == 0
    ws.zero_() if fill == "zero" else poison.fill_(ws.view(torch.float32), fill)
    meta = torch.tensor(ptrs_x + ptrs_y + n_x + n_y, dtype=torch.int64).to(dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    arg = lambda name: P(outs[name]) if name in want else None
    rc = lib.swc_align(P(meta[:B]), P(meta[B:2 * B]), P(meta[2 * B:3 * B]), P(meta[3 * B:]), max_nx, max_ny, L, ops.ALIGN_MODES[mode],
                       arg("info"), arg("values"), arg("xc"), ldc, P(ws), need, B, ops._stream())
    _lib.check(rc, "swc_align")
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


def row_bits(res, b, L):
    """what the call says about pair b, as bytes"""
    parts = []
    for k in OUTPUTS:
        if k in res:
            v = res[k][b, :2 * L + 1] if k == "xc" else res[k][b]
            parts.append(v.contiguous().view(torch.uint8).numpy().tobytes())
    return b"".join(parts)


def compare(got, b, want, L):
    """pair b of a call against its reference dict: xc and info equal, values within one f32 ulp (-> the largest distance seen),
    the columns of xc at and beyond 2 L + 1 untouched"""
    xc = got["xc"][b].numpy()
    assert np.array_equal(xc[:2 * L + 1], want["xc"]), (b, np.nonzero(xc[:2 * L + 1] != want["xc"])[0][:8])
    assert poison.same_bits(got["xc"][b, 2 * L + 1:].contiguous(), got["before"]["xc"][b, 2 * L + 1:].contiguous()), (b, "xc beyond 2 L + 1")
    assert got["info"][b].tolist() == want["info"].tolist(), (b, got["info"][b].tolist(), want["info"].tolist())
    v, w = got["values"][b].numpy(), want["values"]
    assert np.array_equal(np.isnan(v), np.isnan(w)), (b, v, w)
    ok = ~np.isnan(w)
    u = np.abs(v[ok].view(np.int32).astype(np.int64) - w[ok].view(np.int32).astype(np.int64))
    assert (u <= 1).all(), (b, v, w)
    return int(u.max()) if ok.any() else 0


# ---- against the reference ----

LENGTHS = (0, 1, 2, 3, 63, 777, 4096, 4099, 2500, 5001, 1531)
LAGS = (0, 1, -1, 5, -12, 40, -40, 44, -300, 17, -2)


def batch_of(B):
    """B pairs: lengths walking LENGTHS at two strides (nx != ny in most), true lags walking LAGS"""
    out = []
    for k in range(B):
        nx, ny = LENGTHS[(3 * k + 5) % len(LENGTHS)], LENGTHS[(7 * k + 8) % len(LENGTHS)]
        out.append(("batch", k, nx, ny, LAGS[k % len(LAGS)]))
    return out


def pair_of(spec):
    if spec not in _CACHE:
        _, k, nx, ny, d = spec
        _CACHE[spec] = make_pair(nx, ny, d, seed=k)
    return _CACHE[spec]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [1, 3, 33])
def test_xc_info_and_values(B, mode):
    L = 40
    specs = batch_of(B)
    got = run([pair_of(s) for s in specs], L, mode)
    worst = max(compare(got, b, reference(s, *pair_of(s), L, mode), L) for b, s in enumerate(specs))
    print(f"B={B} {mode}: largest distance of a value {worst} ulp; lags {got['info'][:, 0].tolist()}")
    if B == 33:
        lags = got["info"][:, 0].tolist()
        assert {0, 1, 5, 17, 40} <= set(lags) and min(lags) < 0
        assert sum(1 for s in specs if s[2] == 0 or s[3] == 0) >= 2       # empty pairs among them


@pytest.mark.parametrize("L_name", ["0", "1", "2", "G-1", "G", "G+1", "800"])
def test_length_and_lag_sweep(L_name):
    """lengths round the chunk C (and tiny ones), ranges round the lag block G, true lags at 0, +-1 (both pair alignments),
    +-L and one beyond +-L, in both modes"""
    Cn, G, _ = consts()
    L = {"0": 0, "1": 1, "2": 2, "G-1": G - 1, "G": G, "G+1": G + 1, "800": 800}[L_name]
    lengths = (1, 2, 3, 63, 64, 65, Cn - 1, Cn, Cn + 1, 2 * Cn + 17)
    lags = (0, 1, -1, L, -L, L + 1, -(L + 1))
    specs = []
    for k in range(14):
        nx, ny = lengths[(k + 6) % 10], lengths[(3 * k + 7) % 10]
        specs.append(("sweep", L_name, k, nx, ny, lags[k % 7]))
    specs.append(("sweep", L_name, 14, 2 * Cn + 17, 2 * Cn + 17, lags[5]))
    specs.append(("sweep", L_name, 15, Cn + 1, 2 * Cn + 17, lags[4]))
    assert sum(1 for s in specs if s[3] != s[4]) > len(specs) // 2
    pairs = {}
    for s in specs:
        pairs[s] = make_pair(s[3], s[4], s[5], seed=s[2])
    for mode in MODES:
        got = run([pairs[s] for s in specs], L, mode)
        for b, s in enumerate(specs):
            want = reference(s, *pairs[s], L, mode)
            compare(got, b, want, L)
            nx, ny, d = s[3], s[4], s[5]
            if mode == "waveform" and min(nx, ny) >= Cn - 1 and abs(d) <= L:
                assert int(got["info"][b, 0]) == d, (s, got["info"][b].tolist())     # the true lag, where it can be found
        print(f"L={L} {mode}: lags {got['info'][:, 0].tolist()}")


def test_the_accumulator_bounds():
    """full-scale square waves, longer than the int32 spill interval, on both sides: every product is +-32767^2, every digit
    product the largest there is; and the same under the envelope (constant |q|: s = 0) """
    Cn, G, spill = consts()
    n = 2 * Cn + 17
    assert n > 8 * spill
    sq = lambda period, n: (TOP * np.where((np.arange(n) // period) % 2 == 0, 1.0, -1.0)).astype(np.float32)
    pairs = [(sq(n + 1, n), sq(n + 1, n)),                   # constant +full scale: c[0] = n 32767^2
             (sq(n + 1, n), -sq(n + 1, n)),                  # every product -32767^2
             (sq(1024, n), sq(1024, n - 5)), (sq(2, n), sq(2, n)), (sq(700, n), -sq(64, n))]
    q = ref.quantise(pairs[0][0])[0]
    assert (np.abs(q) == 32767).all()
    L = G + 1
    for mode in MODES:
        got = run(pairs, L, mode)
        for b, (x, y) in enumerate(pairs):
            compare(got, b, reference(("square", b), x, y, L, mode), L)
        if mode == "waveform":
            assert int(got["xc"][0, L]) == n * 32767 ** 2 and int(got["xc"][1, L]) == -n * 32767 ** 2
            assert got["info"][0].tolist() == [0, 0, 0, n] and got["info"][1].tolist() == [0, 0, 0, n]
            assert got["values"][0].tolist()[:2] == [1.0, 1.0] and got["values"][1].tolist()[:2] == [-1.0, 1.0]
        else:
            assert not got["xc"][0].any() and torch.isnan(got["values"][0, 0]) and float(got["values"][0, 1]) == 1.0


def test_the_int64_range():
    """one pair of 2^22 constant full-scale samples, L = 1: c[0] = 2^22 32767^2 = 4.5e15, beyond 2^52 / 2 and still exact"""
    n = ref.MAX_N
    x = np.full(n, TOP, np.float32)
    want = ref.align(x, x, 1, "waveform")
    assert int(want["xc"][1]) == n * 32767 ** 2 > 2 ** 51
    got = run([(x, x)], 1, "waveform")
    compare(got, 0, want, 1)
    assert got["xc"][0].tolist() == [(n - 1) * 32767 ** 2, n * 32767 ** 2, (n - 1) * 32767 ** 2]
    assert got["info"][0].tolist() == [0, 0, 0, n] and got["values"][0].tolist() == [1.0, 1.0, 0.0, 0.0]


# ---- independence ----

def test_bits_do_not_depend_on_anything_but_the_pair():
    L = 40
    for mode in MODES:
        specs = batch_of(33)
        pairs = [pair_of(s) for s in specs]
        base = run(pairs, L, mode)
        bits = [row_bits(base, b, L) for b in range(33)]
        empty = [b for b, (x, y) in enumerate(pairs) if len(x) == 0 or len(y) == 0]
        assert empty and all(base["info"][b].tolist() == [0, 0, 0, 0] for b in empty)
        # B and the pair's index: alone, three of them, the batch reversed
        for b in (0, 6, 20):
            assert row_bits(run(pairs[b:b + 1], L, mode), 0, L) == bits[b], (mode, b)
        three = run(pairs[4:7], L, mode)
        assert [row_bits(three, k, L) for k in range(3)] == bits[4:7]
        rev = run(pairs[::-1], L, mode)
        assert [row_bits(rev, 32 - b, L) for b in range(33)] == bits
        # rows 0 .. 7 elements behind a 16-byte boundary
        off = run(pairs, L, mode, offsets=[(b % 8, (3 * b + 1) % 8) for b in range(33)])
        assert [row_bits(off, b, L) for b in range(33)] == bits
        # wider length bounds and a wider stride of xc: other grids
        wide = run(pairs, L, mode, max_nx=9000, max_ny=20000, ldc=2 * L + 9)
        assert [row_bits(wide, b, L) for b in range(33)] == bits
        # a longer row is cut at the bounds
        x, y = pairs[6]
        cut = run([(np.concatenate([x, x[:50]]), np.concatenate([y, y[:70]]))], L, mode, max_nx=len(x), max_ny=len(y))
        assert len(x) > 0 and len(y) > 0 and row_bits(cut, 0, L) == bits[6]
        # which outputs are asked for: every subset
        for k in range(len(OUTPUTS) + 1):
            for want in itertools.combinations(OUTPUTS, k):
                part = run(pairs[:7], L, mode, want=want)
                for name in want:
                    assert poison.same_bits(part[name], base[name][:7].contiguous()), (mode, want, name)


def test_memory_contract_and_fill_independence():
    """outputs and workspace are pre-filled two ways (and with zeros) and guarded: run() checks the bands, compare() the columns
    of xc at and beyond 2 L + 1; the results must not depend on what the workspace or the outputs held"""
    L = 40
    specs = batch_of(7)
    pairs = [pair_of(s) for s in specs]
    for mode in MODES:
        res = [run(pairs, L, mode, fill=f, ldc=2 * L + 6) for f in ("nan", "big", "zero")]
        for b, s in enumerate(specs):
            for r in res:
                compare(r, b, reference(s, *pairs[b], L, mode), L)
            assert row_bits(res[0], b, L) == row_bits(res[1], b, L) == row_bits(res[2], b, L), (mode, b)


def test_not_defined_pairs_stay_alone():
    L = 40
    specs = batch_of(33)
    pairs = [pair_of(s) for s in specs]
    bad = [b for b, (x, y) in enumerate(pairs) if len(x) > 100 and len(y) > 100][:3]
    assert len(bad) == 3
    for mode in MODES:
        base = run(pairs, L, mode)
        hit_pairs = [(x.copy(), y.copy()) for x, y in pairs]
        hit_pairs[bad[0]][1][100] = np.nan          # a degraded side
        hit_pairs[bad[1]][0][3] = np.inf            # a clean side
        hit_pairs[bad[2]][1][-1] = -np.inf
        hit = run(hit_pairs, L, mode)
        for b in range(33):
            if b in bad:
                assert base["info"][b, 3] > 0
                assert hit["info"][b].tolist() == [0, 0, 0, 0] and torch.isnan(hit["values"][b, :2]).all()
                assert hit["values"][b, 2:].tolist() == [0.0, 0.0] and not hit["xc"][b, :2 * L + 1].any()
                compare(hit, b, ref.align(*hit_pairs[b], L, mode), L)
            else:
                assert row_bits(hit, b, L) == row_bits(base, b, L), (mode, b)


# ---- the Python surface ----

def _speech_pair(d=37, extra=0):
    """about 2 s of the pitch tests' signal and a copy 0.8 as loud, d samples late, with a little noise"""
    import pitch_ref
    key = ("speech", d, extra)
    if key not in _CACHE:
        x = pitch_ref.test_signal(7)
        y = (0.8 * ref.delayed(x, d, n=len(x) + extra) + 0.001 * np.random.default_rng(5).standard_normal(len(x) + extra)).astype(np.float32)
        _CACHE[key] = (x, y)
    return _CACHE[key]


def test_ops_and_metrics_align_match_the_c_call():
    from simwhisper_codec_amd import metrics, ops
    dev = torch.device("cuda", torch.cuda.current_device())
    L = 40
    specs = batch_of(7)
    pairs = [pair_of(s) for s in specs]
    for mode in MODES:
        base = run(pairs, L, mode)
        xs = [torch.from_numpy(x).to(dev) for x, _ in pairs]
        ys = [torch.from_numpy(y).to(dev) for _, y in pairs]
        r = ops.align(xs, ys, L, mode, want=OUTPUTS)
        for k in OUTPUTS:
            assert poison.same_bits(r[k].cpu(), base[k]), (mode, k)
        a = metrics.align([torch.from_numpy(x) for x, _ in pairs], ys, sample_rate=16000, max_lag_ms=2.5, mode=mode, device=dev)   # host and device rows mixed
        assert set(a) == set(metrics.ALIGN_KEYS) and all(a[k].device == dev and a[k].shape == (7,) for k in a)
        for k, (src, col) in {"lag": ("info", 0), "start_ref": ("info", 1), "start_deg": ("info", 2), "length": ("info", 3),
                              "corr": ("values", 0), "gain": ("values", 1)}.items():
            assert poison.same_bits(a[k].cpu().contiguous(), base[src][:, col].contiguous()), (mode, k)
        vx, vy, info = metrics.aligned(xs, ys, sample_rate=16000, max_lag_ms=2.5, mode=mode, device=dev)
        for b in range(7):
            d, x0, y0, m = base["info"][b].tolist()
            assert vx[b].shape == vy[b].shape == (m,)
            assert vx[b].data_ptr() == xs[b].data_ptr() + 4 * x0 or m == 0          # views: nothing is copied
            assert vy[b].data_ptr() == ys[b].data_ptr() + 4 * y0 or m == 0
    empty = metrics.align([], [], device=dev)
    assert all(empty[k].numel() == 0 for k in metrics.ALIGN_KEYS) and metrics.aligned([], [], device=dev)[:2] == ([], [])


def test_metrics_on_aligned_pairs_equal_the_hand_cut_pairs():
    """align="waveform" scores the views of the aligned pair: bit for bit what the same call gives on copies cut by hand; align=None
    is the call as it was"""
    from simwhisper_codec_amd import metrics, ops
    dev = torch.device("cuda", torch.cuda.current_device())
    d = 37
    x, y = _speech_pair(d)
    n = len(x)
    x2, y2 = _speech_pair(-12, extra=100)
    refs, degs = [torch.from_numpy(x), torch.from_numpy(x2).to(dev)], [torch.from_numpy(y).to(dev), torch.from_numpy(y2)]
    cut_r = [torch.from_numpy(x[:n - d].copy()).to(dev), torch.from_numpy(x2[12:].copy()).to(dev)]
    cut_d = [torch.from_numpy(y[d:].copy()).to(dev), torch.from_numpy(y2[:n - 12].copy()).to(dev)]
    a = metrics.align(refs, degs, device=dev)
    assert a["lag"].tolist() == [d, -12] and a["length"].tolist() == [n - d, n - 12]
    assert (a["corr"] > 0.99).all() and torch.allclose(a["gain"].cpu(), torch.tensor([1.25, 1.25]), rtol=1e-2)
    same = lambda u, v: poison.same_bits(u.cpu().contiguous(), v.cpu().contiguous())
    for call, keys in ((metrics.quality, ("stoi", "estoi", "si_sdr", "segs")), (metrics.spectral, ("mel", "stft", "lsd", "parts")),
                       (metrics.pitch, metrics.PITCH_KEYS + ("frames",))):
        got, want = call(refs, degs, device=dev, align="waveform"), call(cut_r, cut_d, device=dev)
        assert set(got) == set(want) | {"lag"} and got["lag"].tolist() == [d, -12]
        for k in keys:
            assert same(got[k], want[k]), (call.__name__, k)
        plain, none = call(refs, degs, device=dev), call(refs, degs, device=dev, align=None, max_lag_ms=3.0)
        assert set(plain) == set(none) and "lag" not in none
        for k in keys:
            assert same(plain[k], none[k]), (call.__name__, k)
    raw, fixed = metrics.si_sdr(refs, degs, device=dev), metrics.si_sdr(refs, degs, device=dev, align="waveform")
    print("SI-SDR as given", raw.tolist(), "aligned", fixed.tolist())
    assert (fixed > raw + 10.0).all()                               # what the alignment is for
    got, want = metrics.stoi(refs, degs, device=dev, align="waveform"), metrics.stoi(cut_r, cut_d, device=dev)
    assert isinstance(got, tuple) and len(got) == 2 and same(got[0], want[0]) and same(got[1], want[1]) and int(got[1][0]) > 0
    plain, none = metrics.stoi(refs, degs, device=dev), metrics.stoi(refs, degs, device=dev, align=None)
    assert same(plain[0], none[0]) and same(plain[1], none[1])
    # the parent's path itself: the rows cut to the shorter length, one ops call
    with torch.cuda.device(dev):
        xr, yr = metrics._stage(refs, degs, dev)
        direct = ops.quality(xr, yr, metrics.stoi_table(16000, dev), want=ops.QUALITY_METRICS)
    plain = metrics.quality(refs, degs, device=dev)
    assert all(same(plain[k], direct[k]) for k in direct)
    for one, key, src in ((metrics.si_sdr, "si_sdr", metrics.quality), (metrics.lsd, "lsd", metrics.spectral)):
        assert same(one(refs, degs, device=dev, align="waveform"), src(cut_r, cut_d, device=dev)[key])
    # the envelope mode finds the same delay on this pair
    assert metrics.align(refs, degs, device=dev, mode="envelope")["lag"].tolist() == [d, -12]


def test_evaluate_tool_with_alignment(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_quality
    from simwhisper_codec_amd import wavio
    fs = 16000
    os.makedirs(tmp_path / "orig"); os.makedirs(tmp_path / "syn")
    for i, d in enumerate((37, -12)):
        x, y = _speech_pair(d, extra=100 * i)
        wavio.save_audio(str(tmp_path / "orig" / f"utt{i}.wav"), torch.from_numpy(x), fs)
        wavio.save_audio(str(tmp_path / "syn" / f"utt{i}.wav"), torch.from_numpy(y), fs)
    args = ["--original_dir", str(tmp_path / "orig"), "--synthesized_dir", str(tmp_path / "syn"), "--batch_size", "2"]
    assert evaluate_quality.main(args + ["--align", "waveform", "--max_lag_ms", "10"]) == 0
    out = capsys.readouterr().out
    assert "alignment: mean |lag| 24.500 samples, largest |lag| 37" in out and "not aligned" not in out
    assert evaluate_quality.main(args) == 0
    plain = capsys.readouterr().out
    print(out, plain)
    assert "alignment" not in plain and "mean SI-SDR" in plain
