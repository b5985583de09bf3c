"""swc_segmental on the GPU (include/swc_segmental.h) and the layers above it: the eight row values and the per-frame track
against the float64 restatement (tests/segmental_ref.py) at two rates and at the smallest and the largest window, at every edge
of the frame count and of the run length, batches of 1, 3, 12 and 33 with empty rows; frames left out by digital silence on
either side; identical rows and the two power-of-two scaling properties, bit for bit; the bits contract (batch, place,
alignment, length bound, outputs asked for, K = 0); NaN and Inf kept to their row; the ends of P and K and two bad band tables;
the memory contract in the manner of tests/test_activity_gpu.py; metrics.segmental, AudioCodec.segmental and
tools/evaluate_segmental.py.  All pointers and lengths handed to the kernels are valid: nothing here provokes a fault.

Signals are seeded AR-filtered noise plus three harmonics over a noise floor; degradations are additive noise at 5 .. 30 dB SNR
and one low-passed row.  Counts, exclusions (the NaNs of the track), identical rows, the scaling properties and the bits
contract are compared exactly.

Measured on the MI355X over value_cases() below (tools/bench_segmental.py, profiles/segmental_bench.txt),
the largest deviation of a row value or a track entry from the reference: llr 1.110e-16, is 4.441e-16, cd 0 dB, segsnr
7.105e-15 dB (both sides are float64 in one order of operations and differ in the library's log and log10 alone; cd has
neither), fwsegsnr 1.595e-4 dB (the device's f32 FFT of both sides against a float64 one; the largest with K = 1, where the one
band's Ex - Ey is a small difference of two sums over the whole spectrum; 3.3e-5 dB over the cases with 8 bands or more).  Each
TOL is ten times its number, rounded up to two digits."""
import math
import os
import struct
import sys

import numpy as np
import pytest
import torch

import poison
import segmental_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {"llr": 1.2e-15, "is": 4.5e-15, "cd": 0.0, "segsnr": 7.2e-14, "fwsegsnr": 1.6e-3}   # see the docstring: 10 x the measured deviations
MEASURES = ("llr", "is", "cd", "segsnr", "fwsegsnr")
BANDS = 25


def signal(n, fs, seed):
    """n samples: AR(2)-filtered seeded noise, three harmonics of a seeded pitch and a noise floor, peak about 0.4"""
    from scipy.signal import lfilter
    rng = np.random.default_rng(seed)
    if n == 0:
        return np.zeros(0, np.float32)
    x = lfilter([1.0], [1.0, -1.3, 0.6], rng.standard_normal(n + 200))[200:]
    x = 0.3 * x / np.abs(x).max()
    t = np.arange(n, dtype=np.float64) / fs
    f0 = 110.0 + 90.0 * rng.random()
    for k in range(3):
        x = x + (0.06 / (k + 1)) * np.sin(2.0 * math.pi * (k + 1) * f0 * t + rng.random())
    return (x + 1e-3 * rng.standard_normal(n)).astype(np.float32)


def noisy(x, snr_db, seed):
    rng = np.random.default_rng(1000 + seed)
    if len(x) == 0:
        return x.copy()
    rms = math.sqrt(float(np.mean(x.astype(np.float64) ** 2)))
    return (x + rms * 10.0 ** (-snr_db / 20.0) * rng.standard_normal(len(x))).astype(np.float32)


def lowpassed(x):
    from scipy.signal import lfilter
    return lfilter([0.25, 0.5, 0.25], [1.0], lfilter([0.25, 0.5, 0.25], [1.0], x.astype(np.float64))).astype(np.float32)


def degraded(xs, first=0):
    """additive noise at 5, 10, .. 30 dB SNR in turn; every seventh row low-passed instead"""
    return [lowpassed(x) if (first + i) % 7 == 6 and len(x) else noisy(x, 5.0 + 5.0 * ((first + i) % 6), first + i) for i, x in enumerate(xs)]


_TABLES = {}


def bands(fs, W, K=BANDS):
    """(first, count, off, w): K Slaney mel triangles on the bins of W at fs, as metrics.segmental_table packs them"""
    from simwhisper_codec_amd import metrics
    if (fs, W, K) not in _TABLES:
        _TABLES[(fs, W, K)] = metrics.pack_filterbanks([metrics.mel_filterbank(fs, W, K)])
    return _TABLES[(fs, W, K)]


def on_device(rows):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in rows]


def device_table(table):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in zip(("first", "count", "off", "w"), table)}


def unaligned(rows):
    """the rows as views one element off a 16-byte boundary"""
    out = []
    for x in rows:
        buf = torch.zeros(len(x) + 5, dtype=torch.float32, device=DEV)
        v = buf[1:1 + len(x)]
        v.copy_(torch.from_numpy(np.ascontiguousarray(x)))
        assert len(x) == 0 or v.data_ptr() % 16 == 4
        out.append(v)
    return out


def same(a, b):
    """bit equality of two tensors whatever their strides (a one-element column of a [1][8] result is not a byte view)"""
    return a.shape == b.shape and a.dtype == b.dtype and a.detach().cpu().numpy().tobytes() == b.detach().cpu().numpy().tobytes()


_REF = {}


def reference(key, x, y, W, P, table):
    """the reference of one pair, computed once per key and left alone"""
    if key not in _REF:
        _REF[key] = ref.measure(x, y, W, P, table)
    return _REF[key]


def run(xs, ys, W, P, table, **kw):
    from simwhisper_codec_amd import ops
    kw.setdefault("track", True)
    r = ops.segmental(xs, ys, W, P, table=device_table(table) if table is not None else None, **kw)
    return {k: v.cpu() for k, v in r.items()}


def deviations(got, b, want):
    """row b of ops.segmental's result (on the host) against the reference: counts and exclusions exactly -> the largest
    deviation of a row value or a track entry, per measure"""
    vals = got["vals"][b].numpy()
    assert vals[5:].tolist() == want["vals"][5:].tolist(), ("counts", vals[5:], want["vals"][5:])
    T = int(want["frames"])
    track = got["track"][b, :T].numpy()
    assert np.array_equal(np.isnan(track), np.isnan(want["track"])), "exclusions"
    assert np.array_equal(np.isnan(vals[:5]), np.isnan(want["vals"][:5])), ("NaN values", vals, want["vals"])
    dev = {}
    for k, name in enumerate(MEASURES):
        d = 0.0 if math.isnan(want["vals"][k]) else abs(float(vals[k]) - float(want["vals"][k]))
        if T and not np.isnan(want["track"][:, k]).all():
            d = max(d, float(np.nanmax(np.abs(track[:, k] - want["track"][:, k]))))
        dev[name] = d
    return dev


def edge_lengths(W):
    H, R = W // 4, 32768 // W
    of = lambda T: W + (T - 1) * H
    return [0, W - 1, W, W + 1, W + H - 1, W + H, of(R - 1) + 3, of(R), of(R + 1) + H - 1, of(19), of(20), of(21)]


CONFIGS = [(8000, 256, 10), (16000, 512, 16), (16000, 64, 16), (16000, 2048, 16)]


def lengths_33(fs, W):
    return [2 * fs + 7, 0, W] + [W + 37 * i + (W // 4) * (3 + 5 * i) for i in range(27)] + [0, fs + 1, W - 1]


def value_cases():
    """every batch that is compared with the reference -> [(name, fs, W, P, table, xs, ys)]: what the TOLs are measured over"""
    cases = []
    for fs, W, P in CONFIGS:
        lens = edge_lengths(W) + ([2 * fs + 13] if W in (256, 512) else [])
        xs = [signal(n, fs, 10 + i) for i, n in enumerate(lens)]
        cases.append((f"edges-{fs}-{W}", fs, W, P, bands(fs, W), xs, degraded(xs)))
    for fs, W, P in CONFIGS[:2]:
        xs = [signal(n, fs, 40 + i) for i, n in enumerate([int(1.1 * fs) + 5])]
        cases.append((f"alone-{fs}", fs, W, P, bands(fs, W), xs, degraded(xs, 2)))
        xs = [signal(n, fs, 50 + i) for i, n in enumerate([fs + 3, 0, 3 * W + 1])]
        cases.append((f"three-{fs}", fs, W, P, bands(fs, W), xs, degraded(xs, 3)))
    fs, W, P = CONFIGS[0]
    xs = [signal(n, fs, 60 + i) for i, n in enumerate(lengths_33(fs, W))]
    cases.append((f"batch33-{fs}", fs, W, P, bands(fs, W), xs, degraded(xs)))
    xs, ys = silence_rows()
    cases.append(("silence", 16000, 512, 16, bands(16000, 512), xs, ys))
    xs, ys = ends_rows()
    cases += [(f"ends-{name}", 16000, 512, P, table, xs, ys) for name, P, table in ends_tables()]
    return cases


def case(name):
    if not _CASES:
        _CASES.update({c[0]: c for c in value_cases()})
    return _CASES[name]


def check_case(case):
    name, fs, W, P, table, xs, ys = case
    got = run(on_device(xs), on_device(ys), W, P, table)
    worst = dict.fromkeys(MEASURES, 0.0)
    for b, (x, y) in enumerate(zip(xs, ys)):
        dev = deviations(got, b, reference((name, b), x, y, W, P, table))
        for k in MEASURES:
            worst[k] = max(worst[k], dev[k])
    print(f"{name}: B={len(xs)} largest deviations " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k in MEASURES:
        assert worst[k] <= TOL[k], (name, k, worst[k], TOL[k])
    return got


CASE_NAMES = [f"edges-{fs}-{W}" for fs, W, _ in CONFIGS] + ["alone-8000", "three-8000", "alone-16000", "three-16000", "batch33-8000"]
_CASES = {}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_values_and_track_against_the_reference(name):
    got = check_case(case(name))
    frames = got["vals"][:, 5].tolist()
    if name.startswith("edges"):
        W = case(name)[2]
        R = 32768 // W
        assert frames[:12] == [0, 0, 1, 1, 1, 2, R - 1, R, R + 1, 19, 20, 21]
        assert torch.isnan(got["vals"][0, :5]).all() and not torch.isnan(got["vals"][2, :5]).any()
    if name.startswith("batch33"):
        assert frames.count(0.0) == 3 and len(frames) == 33


def silence_rows(fs=16000, W=512):
    """three pairs of 1.2 s with a stretch of exact zeros (W + H samples and more) on the clean side, the degraded side, both"""
    H, n = W // 4, int(1.2 * fs)
    xs = [signal(n, fs, 70 + i) for i in range(3)]
    ys = degraded(xs, 1)
    xs[0][3000:3000 + W + H] = 0.0
    ys[1][5000:5000 + 2 * W] = 0.0
    xs[2][2000:2000 + W + H + 7] = 0.0
    ys[2][2000 + H:2000 + 2 * W + H] = 0.0
    ys[2][9000:9000 + W + H] = 0.0
    return xs, ys


def test_frames_with_digital_silence_are_counted_out_exactly():
    _, fs, W, P, table, xs, ys = case("silence")
    got = check_case(case("silence"))                                  # counts and NaNs exactly
    for b in range(3):
        want = reference(("silence", b), xs[b], ys[b], W, P, table)
        T, T_lpc, T_fw = (int(want[k]) for k in ("frames", "frames_lpc", "frames_fw"))
        assert T_lpc < T and (T_fw < T) == (b != 1)                    # silence on the clean side alone empties the bands
        silent_clean = np.isnan(want["track"][:, 4])                   # a silent clean frame scores -10 in segsnr
        assert (got["track"][b, :T, 3].numpy()[silent_clean] == -10.0).all() and silent_clean.sum() == T - T_fw


def test_identical_rows_give_exactly_0_0_0_35_35():
    for fs, W, P in CONFIGS:
        xs = [signal(n, fs, 80 + i) for i, n in enumerate([fs + 11, W, 0, 3 * W + 5])]
        got = run(on_device(xs), on_device([x.copy() for x in xs]), W, P, bands(fs, W))
        for b, x in enumerate(xs):
            T = float(ref.frames(len(x), W))
            if T:
                assert got["vals"][b].tolist() == [0.0, 0.0, 0.0, 35.0, 35.0, T, T, T], (W, b, got["vals"][b])
                assert torch.equal(got["track"][b, :int(T)], torch.tensor([0.0, 0.0, 0.0, 35.0, 35.0], dtype=torch.float64).expand(int(T), 5))
            else:
                assert torch.isnan(got["vals"][b, :5]).all() and got["vals"][b, 5:].tolist() == [0.0, 0.0, 0.0]


def test_power_of_two_scalings_bit_for_bit():
    fs, W, P = 16000, 512, 16
    xs = [signal(n, fs, 90 + i) for i, n in enumerate([fs + 301, 5 * W + 3])]
    ys = degraded(xs, 2)
    table = bands(fs, W)
    base = run(on_device(xs), on_device(ys), W, P, table)
    assert not torch.isnan(base["vals"]).any() and (base["vals"][:, 0] > 0).all()
    for s in (0.125, 4.0):                                              # y alone: llr and cd
        r = run(on_device(xs), on_device([y * np.float32(s) for y in ys]), W, P, table)
        for col in (0, 2):
            assert poison.same_bits(base["vals"][:, col], r["vals"][:, col]) and poison.same_bits(base["track"][:, :, col], r["track"][:, :, col]), (s, col)
        assert not poison.same_bits(base["vals"][:, 3], r["vals"][:, 3])
    for s in (0.0625, 0.5, 8.0):                                        # both rows: all five
        r = run(on_device([x * np.float32(s) for x in xs]), on_device([y * np.float32(s) for y in ys]), W, P, table)
        assert poison.same_bits(base["vals"], r["vals"]) and poison.same_bits(base["track"], r["track"]), s


def test_a_rows_results_do_not_depend_on_batch_place_alignment_bound_or_outputs():
    from simwhisper_codec_amd import ops
    fs, W, P = CONFIGS[0]
    table = bands(fs, W)
    xs = [signal(n, fs, 60 + i) for i, n in enumerate(lengths_33(fs, W))]
    ys = degraded(xs)
    k = 0                                                               # 2 s: two runs
    T = ref.frames(len(xs[k]), W)
    alone = run(on_device([xs[k]]), on_device([ys[k]]), W, P, table)
    assert T > 32768 // W and not torch.isnan(alone["vals"]).any()
    for place in (0, 16, 32):
        order = list(range(1, 33))
        order.insert(place, k)
        batch = run(on_device([xs[i] for i in order]), on_device([ys[i] for i in order]), W, P, table)
        assert poison.same_bits(alone["vals"][0], batch["vals"][place]), place
        assert poison.same_bits(alone["track"][0, :T].contiguous(), batch["track"][place, :T].contiguous()), place
    odd = run(unaligned([xs[k]]), unaligned([ys[k]]), W, P, table)
    longer = run(on_device([xs[k]]), on_device([ys[k]]), W, P, table, max_n_in=len(xs[k]) + 12345, ld_t=T + 5)
    for other in (odd, longer):
        assert poison.same_bits(alone["vals"], other["vals"]) and poison.same_bits(alone["track"][0, :T].contiguous(), other["track"][0, :T].contiguous())
    assert longer["track"].shape[1] == T + 5 and not longer["track"][0, T:].any()  # rows behind a pair's frames are not written
    plain = run(on_device([xs[k]]), on_device([ys[k]]), W, P, table, track=False)
    assert "track" not in plain and poison.same_bits(alone["vals"], plain["vals"])
    short = run(on_device([xs[k]]), on_device([ys[k]]), W, P, table, ld_t=7)      # a track shorter than the row
    assert poison.same_bits(short["track"][0], alone["track"][0, :7].contiguous()) and poison.same_bits(alone["vals"], short["vals"])
    nobands = run(on_device([xs[k]]), on_device([ys[k]]), W, P, None)              # K = 0: the other four values
    assert poison.same_bits(alone["vals"][:, :4].contiguous(), nobands["vals"][:, :4].contiguous())
    assert poison.same_bits(alone["track"][0, :T, :4].contiguous(), nobands["track"][0, :T, :4].contiguous())
    assert math.isnan(float(nobands["vals"][0, 4])) and nobands["vals"][0, 5:].tolist() == [float(T), float(T), 0.0]
    assert torch.isnan(nobands["track"][0, :T, 4]).all()
    assert ops.segmental_workspace_bytes(1, len(xs[k]), W, P, BANDS) == ref.workspace_bytes(1, len(xs[k]), W, P)


def test_nan_and_inf_stay_in_their_row():
    fs, W, P = 16000, 512, 16
    table = bands(fs, W)
    xs = [signal(n, fs, 100 + i) for i, n in enumerate([fs, fs + 40, 4 * W, fs - 9, 3 * W])]
    ys = degraded(xs, 4)
    clean = run(on_device(xs), on_device(ys), W, P, table)
    bx, by = [x.copy() for x in xs], [y.copy() for y in ys]
    bx[1][5000] = np.nan
    by[3][300] = np.inf
    bad = run(on_device(bx), on_device(by), W, P, table)
    for b in (0, 2, 4):
        assert poison.same_bits(clean["vals"][b], bad["vals"][b]) and poison.same_bits(clean["track"][b], bad["track"][b]), b
    for b in (1, 3):
        assert torch.isnan(bad["vals"][b, :5]).any() and bad["vals"][b, 5] == clean["vals"][b, 5], (b, bad["vals"][b])
        want = ref.measure(bx[b], by[b], W, P, table)
        assert np.array_equal(np.isnan(bad["vals"][b].numpy()), np.isnan(want["vals"])) and bad["vals"][b, 5:].tolist() == want["vals"][5:].tolist()
        cols = 5 if b == 1 else 4                                      # (an Inf goes through the f32 FFT as Inf or NaN, bin by bin)
        assert np.array_equal(np.isnan(bad["track"][b, :int(want["frames"]), :cols].numpy()), np.isnan(want["track"][:, :cols]))
    assert math.isnan(float(bad["vals"][1, 3])) and math.isnan(float(bad["vals"][1, 4]))      # every frame counts there


def ends_rows(fs=16000, W=512):
    xs = [signal(n, fs, 110 + i) for i, n in enumerate([fs // 2 + 3, 0, 2 * W])]
    return xs, degraded(xs, 1)


def ends_tables(fs=16000, W=512):
    """[(name, P, table)]: P = 1 and 32; K = 0, 1 and 64; a table with an empty filter; one whose ranges leave [0, F) and the
    weights (cut by the kernel and by the reference alike: wrong numbers, the same ones)"""
    F = W // 2 + 1
    first, count, off, w = (v.copy() for v in bands(fs, W, 8))
    count[3] = 0
    empty = (first, count, off, w)
    first, count, off, w = (v.copy() for v in bands(fs, W, 8))
    first[0], count[7], off[5] = -3, 400, len(w) - 2
    assert first[7] + count[7] > F
    return [("P1", 1, bands(fs, W)), ("P32", 32, bands(fs, W)), ("K0", 16, None), ("K1", 16, bands(fs, W, 1)), ("K64", 16, bands(fs, W, 64)),
            ("empty", 16, empty), ("cut", 16, (first, count, off, w))]


def test_the_ends_of_P_and_K_and_two_bad_band_tables():
    for name, P, table in ends_tables():
        got = check_case(case(f"ends-{name}"))
        assert (got["vals"][0, 7] > 0) == (table is not None), name


FILLS = {"zero": (0.0, 0x00), "poison": (math.nan, poison.U8_POISON), "ones": (poison.BIG, 0xFF)}


def test_memory_contract():
    """vals, track and the workspace are poison.guarded windows with slack behind them; whatever they held before, the results
    are the same bits, the slack and the bands keep what they held, and the rows (views with other samples around them) are
    unchanged"""
    from simwhisper_codec_amd import ops
    fs, W, P = 8000, 256, 10
    table = device_table(bands(fs, W))
    lens = [fs + 5, 0, W - 1, 32768 + 3 * (W // 4), 2701]
    xs = [signal(n, fs, 120 + i) for i, n in enumerate(lens)]
    ys = degraded(xs)
    B, max_n = len(xs), max(lens)
    flat = torch.full((2 * sum(n + 3 for n in lens) + 1,), 0.25, dtype=torch.float32, device=DEV)
    rows, at = [], 1
    for v in xs + ys:
        flat[at:at + len(v)] = torch.from_numpy(v).to(DEV)
        rows.append(flat[at:at + len(v)])
        at += len(v) + 3
    xr, yr = rows[:B], rows[B:]
    snap = flat.clone()
    need = ops.segmental_workspace_bytes(B, max_n, W, P, BANDS)
    cap = ref.frames(max_n, W) + 3
    frames = [ref.frames(n, W) for n in lens]
    res = []
    for fill, (number, byte) in FILLS.items():
        vview, vcheck = poison.guarded((1, B * 8), torch.float64, ld=B * 8 + 5, band_rows=8, device=DEV)
        tview, tcheck = poison.guarded((1, B * cap * 5), torch.float64, ld=B * cap * 5 + 6, band_rows=8, device=DEV)
        wview, wcheck = poison.guarded((1, need), torch.uint8, ld=(need + 255) // 256 * 256 + 256, band_rows=2, device=DEV)
        vview.fill_(number), tview.fill_(number), wview.fill_(byte)
        assert wview[0].data_ptr() % 256 == 0
        r = ops.segmental(xr, yr, W, P, table=table, track=True, ld_t=cap,
                          out={"vals": vview[0].view(B, 8), "track": tview[0].view(B, cap, 5)}, workspace=wview[0])
        torch.cuda.synchronize()
        for check in (vcheck, tcheck, wcheck):
            check()
        assert poison.same_bits(flat, snap), "a read-only input changed"
        held = torch.full((1,), number, dtype=torch.float64, device=DEV)
        for b in range(B):
            behind = r["track"][b, frames[b]:].reshape(-1)
            assert poison.same_bits(behind, held.expand(behind.numel()).contiguous()), "an entry behind a row's frames was written"
        res.append((r["vals"].clone(), torch.cat([r["track"][b, :frames[b]].reshape(-1) for b in range(B)])))
    for r in res[1:]:
        assert all(poison.same_bits(a, b) for a, b in zip(res[0], r))
    plain = ops.segmental(on_device(xs), on_device(ys), W, P, table=table, track=True)
    assert poison.same_bits(plain["vals"], res[0][0])
    assert res[0][0][:, 5].tolist() == [float(t) for t in frames]
    for pattern in poison.PATTERNS:                                        # no result depends on uninitialised memory
        with poison.poisoned_empty(pattern) as spy:
            r = ops.segmental(xr, yr, W, P, table=table, track=True)
        assert spy.device_calls > 0, pattern
        got = (r["vals"], torch.cat([r["track"][b, :frames[b]].reshape(-1) for b in range(B)]))
        assert all(poison.same_bits(a, b) for a, b in zip(res[0], got)), pattern


def test_metrics_segmental_matches_ops_and_want_and_align():
    from simwhisper_codec_amd import _lib, metrics, ops
    fs = 16000
    dev = torch.device("cuda", torch.cuda.current_device())
    W, P = metrics.segmental_params(fs)
    assert (W, P) == (512, 16) and metrics.segmental_params(8000) == (256, 10) and metrics.segmental_params(48000) == (2048, 16)
    xs = [signal(n, fs, 130 + i) for i, n in enumerate([fs + 9, 0, 2 * fs])]
    ys = degraded(xs, 2)
    dx, dy = on_device(xs), on_device(ys)
    base = ops.segmental(dx, dy, W, P, table=metrics.segmental_table(fs, dev), track=True)
    q = metrics.segmental([torch.from_numpy(xs[0])] + dx[1:], dy, sample_rate=fs, tracks=True, device=dev)          # host and device rows
    assert set(q) == set(metrics.SEGMENTAL_KEYS) | {"frames", "frames_lpc", "frames_fw", "track"}
    for i, k in enumerate(metrics.SEGMENTAL_KEYS):
        assert q[k].dtype == torch.float64 and q[k].device == dev and same(q[k], base["vals"][:, i]), k
    T = q["frames"].cpu().tolist()
    assert T == [ref.frames(len(x), W) for x in xs] and q["frames"].dtype == torch.int32 and T[1] == 0
    assert all(same(t, base["track"][b, :T[b]]) for b, t in enumerate(q["track"]))
    few = metrics.segmental(dx, dy, sample_rate=fs, want=("llr", "segsnr"), device=dev)
    assert set(few) == {"llr", "segsnr", "frames", "frames_lpc", "frames_fw"} and few["frames_fw"].tolist() == [0, 0, 0]
    assert same(few["llr"], q["llr"]) and same(few["segsnr"], q["segsnr"])
    for name, key in (("llr", "llr"), ("itakura_saito", "is"), ("lpc_cd", "cd"), ("seg_snr", "segsnr"), ("fw_seg_snr", "fwsegsnr")):
        assert same(getattr(metrics, name)(dx, dy, sample_rate=fs, device=dev), q[key]), name
    with pytest.raises(_lib.SwcError):
        metrics.segmental(dx, dy, sample_rate=fs, want=("pesq",), device=dev)
    empty = metrics.segmental([], [], sample_rate=fs, tracks=True, device=dev)
    assert all(empty[k].numel() == 0 for k in metrics.SEGMENTAL_KEYS) and empty["track"] == []
    lag, n = 37, len(xs[2])
    late = np.concatenate([np.zeros(lag, np.float32), ys[2]])[:n]
    a = metrics.segmental([dx[2]], on_device([late]), sample_rate=fs, align="waveform", device=dev)
    want = metrics.segmental(on_device([xs[2][:n - lag]]), on_device([ys[2][:n - lag]]), sample_rate=fs, device=dev)
    assert a["lag"].tolist() == [lag] and all(same(a[k], want[k]) for k in want)
    shifted = metrics.segmental([dx[2]], on_device([late]), sample_rate=fs, device=dev)
    assert float(shifted["segsnr"][0]) < float(want["segsnr"][0]) - 5.0          # the shift is what the alignment removed


def _tiny_model(dev):
    import common
    from simwhisper_codec_amd.codec import AudioCodec
    model = AudioCodec(common.tiny_params(), precision="fp32")
    model.load_state_dict(common.state_dict("tiny"), strict=True)
    return model.to(dev).eval()


def test_audiocodec_segmental_on_the_synthetic_checkpoint():
    from simwhisper_codec_amd import metrics, synth
    dev = torch.device("cuda", torch.cuda.current_device())
    model = _tiny_model(dev)
    wavs = [synth.synth_audio(18000, index=0, kind="speech").to(dev), synth.synth_audio(17000, index=1, kind="speech").to(dev)]
    q = model.segmental(wavs, tracks=True)
    assert set(q) == set(metrics.SEGMENTAL_KEYS) | {"frames", "frames_lpc", "frames_fw", "track"}
    syn = model.decode(model.encode(wavs)["codes_list"])["syn_wav_list"]
    want = metrics.segmental(wavs, syn, sample_rate=model.input_sample_rate, device=dev)
    for k in metrics.SEGMENTAL_KEYS:
        assert q[k].shape == (2,) and q[k].dtype == torch.float64 and same(q[k], want[k]), k
    assert (q["frames"] > 100).all() and not torch.isnan(q["segsnr"]).any() and len(q["track"]) == 2
    assert set(model.segmental(wavs, want=("cd",))) == {"cd", "frames", "frames_lpc", "frames_fw"}


def _write_wav(path, pcm, sr=16000):
    raw = pcm.numpy().astype("<i2").tobytes()
    open(path, "wb").write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
                           struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16) + b"data" + struct.pack("<I", len(raw)) + raw)


def test_the_directory_tool_prints_the_means_and_names_an_empty_pair(tmp_path, capsys):
    import common
    from simwhisper_codec_amd import metrics
    sys.path.insert(0, os.path.join(common.ROOT, "tools"))
    import evaluate_segmental
    fs = 16000
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    pairs = []
    for i, n in enumerate([fs + 100, 300, fs // 2]):                      # the second pair is shorter than one window
        x = signal(n, fs, 140 + i)
        px, py = (torch.from_numpy(v * 32767.0).round().clamp(-32768, 32767).to(torch.int16) for v in (x, noisy(x, 15.0, i)))
        _write_wav(str(a / f"f{i}.wav"), px)
        _write_wav(str(b / f"f{i}.wav"), py)
        pairs.append((px.float() / 32768.0, py.float() / 32768.0))
    assert evaluate_segmental.main(["--original_dir", str(a), "--synthesized_dir", str(b), "--batch_size", "2", "--verbose"]) == 0
    out = capsys.readouterr().out
    dev = torch.device("cuda", torch.cuda.current_device())
    q = metrics.segmental([p[0] for p in pairs], [p[1] for p in pairs], sample_rate=fs, device=dev)
    keep = [0, 2]
    for k, label in (("llr", "LLR"), ("is", "IS"), ("cd", "CD"), ("segsnr", "SegSNR"), ("fwsegsnr", "fwSegSNR")):
        mean = sum(float(q[k][i]) for i in keep) / 2
        assert f"mean {label}: {mean:.3f}" in out, (label, mean, out)
    assert "no frame, left out of the means (1): f1.wav" in out and "over 2 pairs" in out and "f0.wav:" in out
