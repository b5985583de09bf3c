"""swc_activity and swc_activity_normalise on the GPU (include/swc_activity.h) and the layers above them: the values, the
fifteen counts and the runs against the float64 restatement (tests/activity_ref.py) at every edge of the sub-block, carry-group
and hangover lengths, four rates and three batch sizes; two bursts whose exceedance gap is exactly the hangover and one sample
more; crossings at different thresholds; independence of the batch around a row and of its alignment; the gain, the scaled rows
and the two flags; the memory contract in the manner of tests/test_loudness_gpu.py; AudioCodec.encode(active_level=),
metrics.trimmed / split_at_pauses, the CLI flags and tools/measure_activity.py.  All pointers and lengths handed to the kernels
are valid: nothing here provokes a fault.

Every case first asserts on the CPU that no sample's envelope is within 1e-9 (relative) of any of the fifteen thresholds or of
c*: under that condition counts and run boundaries are compared exactly.

Measured on the MI355X (profiles/activity_bench.txt): the largest deviation of a dB output from the
reference over the cases below is 2.842e-14 dB (both sides are float64 and differ in the order of the sum of squares and in the
library's log10 and pow); TOL is ten times that, rounded up to two digits."""
import math

import numpy as np
import pytest
import torch

import activity_ref as ref
import poison

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2.9e-13                                # dB; see the docstring: 10 x the measured deviation
MARGIN = 1e-9                                # relative distance of every envelope sample from every threshold (asserted on the CPU)
GAIN_MARGIN = 2.0 * TOL * math.log(10.0) / 20.0   # a dB deviation of TOL moves a gain by TOL ln(10) / 20 of itself
SUB, GROUP = 256, 64                         # SWC_ACTIVITY_SUBBLOCK, SWC_ACTIVITY_GROUP


def signal(n, fs, seed, level_db=-20.0):
    """n samples of speech-like bursts: seeded noise and sines of 0.25 .. 0.6 s at levels within 12 dB of level_db, between
    pauses of 0.05 .. 0.5 s (some shorter than the hangover, some longer), behind a short leading silence"""
    rng = np.random.default_rng(seed)
    x = np.zeros(n)
    t = np.arange(n, dtype=np.float64) / fs
    at, k = int(0.03 * fs) + seed % 7, 0
    while at < n:
        dur = int((0.25 + 0.35 * rng.random()) * fs)
        a, b = at, min(at + dur, n)
        amp = 10.0 ** ((level_db - 12.0 * rng.random()) / 20.0)
        if (k + seed) % 2:
            x[a:b] = amp * np.sin(2.0 * math.pi * (180.0 + 70.0 * ((k + seed) % 5)) * t[a:b])
        else:
            x[a:b] = amp * rng.standard_normal(b - a) * 0.5
        at = b + int((0.05 + 0.45 * rng.random()) * fs)
        k += 1
    return x.astype(np.float32)


_REF = {}


def reference(key, x, fs):
    """the reference of one row, computed once per key and left alone"""
    if key not in _REF:
        m = ref.margin(x, fs, every_threshold=True)
        assert m >= MARGIN, (key, m)          # a flipped sample cannot hide: every case keeps its distance
        _REF[key] = ref.measure(x, fs)
    return _REF[key]


def on_device(rows):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in rows]


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


def db_outputs(v):
    """the four dB outputs of a row of values: A, L, the factor and c* in dB"""
    f = lambda t, k: k * math.log10(t) if t > 0.0 else (math.nan if math.isnan(t) else -math.inf)
    return [float(v[0]), float(v[1]), f(float(v[2]), 10.0), f(float(v[3]), 20.0)]


def compare(res, i, want, what):
    """row i of ops.activity's result (on the host) against the reference dict -> the largest deviation of its dB outputs"""
    v = res["values"][i]
    worst = 0.0
    w4 = db_outputs([want["active_level"], want["long_term"], want["activity"], want["threshold"]])
    for name, g, w in zip(("active_level", "long_term", "activity", "threshold"), db_outputs(v), w4):
        if math.isnan(w):
            assert math.isnan(g), (what, name, g)
        else:
            assert abs(g - w) <= TOL, (what, name, g, w, abs(g - w))
            worst = max(worst, abs(g - w))
    assert float(v[4]) == want["sample_peak"], (what, "sample_peak")
    assert res["counts"][i].tolist() == want["counts"], (what, "counts", res["counts"][i].tolist(), want["counts"])      # exact
    assert float(v[5]) == want["active_samples"] and float(v[6]) == want["runs"], (what, "active samples, runs", v[5:7], want["runs"])
    assert (math.isnan(float(v[7])) and math.isnan(want["crossing"])) or float(v[7]) == want["crossing"], (what, "crossing")
    k = len(want["run_list"])
    assert [tuple(r) for r in res["runs"][i, :k].tolist()] == want["run_list"], (what, "runs")                             # exact
    return worst


def measure(rows, fs, **kw):
    from simwhisper_codec_amd import ops
    return {k: v.cpu() for k, v in ops.activity(rows, fs, **kw).items()}


def edge_lengths(fs=8000):
    I = ref.hangover(fs)
    return [0, 1, SUB - 1, SUB, SUB + 1, I, I + 1, I + 2, GROUP * SUB - 1, GROUP * SUB, GROUP * SUB + 1, 12 * fs]


def test_values_counts_and_runs_at_every_edge_length():
    fs = 8000
    rows = [signal(n, fs, seed=2 + i) for i, n in enumerate(edge_lengths(fs))]
    want = [reference(("edge", fs, i), x, fs) for i, x in enumerate(rows)]
    assert want[-1]["runs"] >= 4 and 0.3 < want[-1]["activity"] < 0.98 and sum(not math.isnan(w["active_level"]) for w in want) >= 7
    got = measure(on_device(rows), fs)
    worst = max(compare(got, i, want[i], ("edge", i)) for i in range(len(rows)))
    print(f"fs={fs} B={len(rows)}: largest deviation of a dB output {worst:.3e} dB")


@pytest.mark.parametrize("fs", [8000, 16000, 44100, 48000])
def test_batch_of_5_with_an_empty_row_at_four_rates(fs):
    I = ref.hangover(fs)
    lens = [int(2.3 * fs) + 11, 0, SUB + 1, I + 2, 4096 + I + 3]
    rows = [signal(n, fs, seed=20 + i) for i, n in enumerate(lens)]
    want = [reference(("b5", fs, i), x, fs) for i, x in enumerate(rows)]
    assert want[0]["runs"] >= 2 and math.isnan(want[1]["active_level"]) and want[1]["run_list"] == []
    got = measure(on_device(rows), fs)
    worst = max(compare(got, i, want[i], (fs, i)) for i in range(5))
    print(f"fs={fs} B=5: largest deviation of a dB output {worst:.3e} dB")


def test_one_row_alone():
    fs = 16000
    x = signal(3 * fs + 5, fs, seed=31)
    want = reference(("alone", fs), x, fs)
    assert want["runs"] >= 2
    print(f"fs={fs} B=1: largest deviation of a dB output {compare(measure(on_device([x]), fs), 0, want, 'alone'):.3e} dB")


def batch_of_33(fs=8000):
    """33 rows at fs: many lengths, an all-zero row, an empty row, a click in silence"""
    lens = [3 * fs + 7, 2 * fs] + [SUB * (3 + 5 * i) + 37 * i for i in range(28)] + [0, fs, 4 * fs + 1]
    rows = [signal(n, fs, seed=40 + i) for i, n in enumerate(lens)]
    rows[1] = np.zeros(2 * fs, np.float32)
    rows[31] = np.zeros(fs, np.float32)
    rows[31][fs // 3] = 1.0                            # a full-scale click: the envelope never comes near it
    return rows


def test_batch_of_33_with_a_silent_row_a_click_and_unaligned_views():
    fs = 8000
    rows = batch_of_33(fs)
    want = [reference(("b33", fs, i), x, fs) for i, x in enumerate(rows)]
    for i in (1, 30, 31):                               # all zero, empty, the click: NaN values and no runs
        assert math.isnan(want[i]["active_level"]) and math.isnan(want[i]["activity"]) and want[i]["run_list"] == []
    assert math.isnan(want[1]["long_term"]) and want[31]["sample_peak"] == 1.0 and not math.isnan(want[31]["long_term"])
    got = measure(on_device(rows), fs)
    worst = max(compare(got, i, want[i], ("b33", i)) for i in range(33))
    print(f"fs={fs} B=33: largest deviation of a dB output {worst:.3e} dB")
    assert float(got["values"][31][5]) == 0.0 and float(got["values"][31][6]) == 0.0
    again = measure(unaligned(rows), fs)
    assert all(poison.same_bits(got[k], again[k]) for k in got)


def two_bursts(fs, gap):
    """two 0.4 s tone bursts with `gap` silent samples between them and 0.5 s of silence behind"""
    t = np.arange(int(0.4 * fs), dtype=np.float64) / fs
    b = 0.3 * np.sin(2.0 * math.pi * 310.0 * t)
    return np.concatenate([b, np.zeros(gap), b, np.zeros(fs // 2)]).astype(np.float32)


def exceedance_gap(r):
    """the longest stretch of samples under c* between two samples at or above it"""
    at = np.flatnonzero(r["q"] >= r["threshold"])
    return int(np.max(np.diff(at))) - 1


def gap_rows(fs=8000):
    """the two-burst row with the largest signal gap that is still one run, and the one with one silent sample more: the signal
    gap is stepped in the reference (bisection on its run count)"""
    lo, hi = 0, 2 * ref.hangover(fs)
    assert ref.measure(two_bursts(fs, lo), fs)["runs"] == 1 and ref.measure(two_bursts(fs, hi), fs)["runs"] == 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ref.measure(two_bursts(fs, mid), fs)["runs"] == 1:
            lo = mid
        else:
            hi = mid
    return [two_bursts(fs, lo), two_bursts(fs, hi)]


def test_an_exceedance_gap_of_exactly_the_hangover_is_one_run_and_one_sample_more_is_two():
    fs = 8000
    I = ref.hangover(fs)
    rows = gap_rows(fs)
    want = [reference(("gap", fs, i), x, fs) for i, x in enumerate(rows)]
    assert [exceedance_gap(w) for w in want] == [I, I + 1] and [w["runs"] for w in want] == [1, 2]
    got = measure(on_device(rows), fs)
    for i in range(2):
        compare(got, i, want[i], ("gap", i))
    assert got["values"][:, 6].tolist() == [1.0, 2.0]


LEVELS = (-10.0, -20.0, -30.0, -40.0, -50.0, -60.0, -70.0, -80.0)


def test_the_crossing_falls_at_different_thresholds_the_first_one_included():
    fs = 8000
    rows = [signal(2 * fs + 100 * i, fs, seed=60 + i, level_db=lv) for i, lv in enumerate(LEVELS)]
    want = [reference(("levels", fs, i), x, fs) for i, x in enumerate(rows)]
    crossings = [w["crossing"] for w in want]
    assert 0.0 in crossings and len(set(crossings)) >= 5 and not any(math.isnan(c) for c in crossings)
    got = measure(on_device(rows), fs)
    worst = max(compare(got, i, want[i], ("levels", i)) for i in range(len(rows)))
    print(f"fs={fs} levels {LEVELS}: crossings {crossings}, largest deviation of a dB output {worst:.3e} dB")


def test_a_rows_results_do_not_depend_on_the_batch_its_place_its_alignment_or_the_length_bound():
    fs = 8000
    rows = batch_of_33(fs)
    k = 32                                                      # 4 fs + 1 samples: two carry groups, eight tiles
    alone = measure(on_device([rows[k]]), fs)
    batch = measure(on_device(rows), fs)
    back = measure(on_device(rows[::-1]), fs)
    odd = measure(unaligned([rows[k]]), fs)
    longer = measure(on_device([rows[k]]), fs, max_n_in=len(rows[k]) + 12345)
    nr = int(alone["values"][0, 6])
    assert nr >= 2 and not torch.isnan(alone["values"][0, :4]).any()
    for other, i in ((batch, k), (back, 32 - k), (odd, 0), (longer, 0)):
        assert poison.same_bits(alone["values"][0], other["values"][i]) and poison.same_bits(alone["counts"][0], other["counts"][i])
        assert poison.same_bits(alone["runs"][0, :nr].contiguous(), other["runs"][i, :nr].contiguous())
    assert poison.same_bits(batch["values"], back["values"].flip(0)) and poison.same_bits(batch["counts"], back["counts"].flip(0))


def normalise_rows(fs=8000):
    """-> rows: ordinary ones, one whose click makes 1 / peak bind, one silent, one empty"""
    rows = [signal(int(2.37 * fs), fs, seed=71, level_db=-35.0), signal(2 * fs + 13, fs, seed=72, level_db=-14.0)]
    peaky = signal(2 * fs, fs, seed=73, level_db=-26.0)               # some 8 dB under the target, and 1 / 0.9 is 0.9 dB
    peaky[fs] = 0.9
    return rows + [peaky, np.zeros(fs, np.float32), np.zeros(0, np.float32)]


def test_normalise_gains_rows_and_flags():
    from simwhisper_codec_amd import ops
    fs = 8000
    rows = normalise_rows(fs)
    dev = on_device(rows)
    values = ops.activity(dev, fs)["values"]
    cols = max(len(x) for x in rows) + 9
    out, gains, flags = ops.activity_normalise(dev, values, -26.0, cols=cols)
    gains, flags, out = gains.cpu(), flags.cpu().tolist(), out.cpu()
    want_flags = []
    for i, x in enumerate(rows):
        w = reference(("norm", fs, i), x, fs)
        g, f = ref.gain(w["active_level"], w["sample_peak"], -26.0)
        if f == 0:
            assert ref.f32_margin(g) >= GAIN_MARGIN, (i, g)      # the rounding to f32 cannot hinge on the last bits of A
        assert float(gains[i]) == float(np.float32(g)), (i, float(gains[i]), g)
        want_flags.append(f)
        n = len(x)
        assert poison.same_bits(out[i, :n], torch.from_numpy(x) * gains[i])       # one f32 multiply
        assert not out[i, n:].any()
    assert flags == want_flags == [0, 0, ref.PEAK_LIMITED, ref.UNMEASURED, ref.UNMEASURED]
    assert float(gains[2]) == float(np.float32(1.0 / np.float64(np.float32(0.9)))) and float(gains[0]) > 1.0 > float(gains[1])
    after = measure([out[i, :len(rows[i])].contiguous().to(DEV) for i in range(2)], fs)   # the scaled rows sit at the target, up to
    assert (after["values"][:, 0] + 26.0).abs().max() < 0.5                        # what the fixed thresholds make of a scaled row
    cut, _, _ = ops.activity_normalise(dev, values, -26.0, cols=1000)              # a longer row is cut at cols
    assert poison.same_bits(cut.cpu(), out[:, :1000].contiguous())


FILLS = {"zero": (0.0, 0, 0x00), "poison": (math.nan, poison.INT_POISON, poison.U8_POISON), "ones": (poison.BIG, -1, 0xFF)}


def memory_rows(fs=8000):
    return [signal(n, fs, seed=80 + i) for i, n in enumerate([3 * fs + 5, 0, SUB - 1, GROUP * SUB + 1, 2701])]


def test_memory_contract():
    """values, counts, runs, the workspace and the normalised batch are poison.guarded windows with slack behind them; whatever
    they held before, the results are the same bits, the slack and the bands keep what they held, and the rows (views with
    other samples around them) are unchanged"""
    from simwhisper_codec_amd import ops
    fs = 8000
    I = ref.hangover(fs)
    xs = memory_rows(fs)
    B, max_n = len(xs), max(len(x) for x in xs)
    flat = torch.full((sum(len(x) + 3 for x in xs) + 1,), 0.25, dtype=torch.float32, device=DEV)   # (what surrounds a row is audible)
    rows, at = [], 1
    for x in xs:
        flat[at:at + len(x)] = torch.from_numpy(x).to(DEV)
        rows.append(flat[at:at + len(x)])
        at += len(x) + 3
    snap = flat.clone()
    need = ops.activity_workspace_bytes(B, max_n, fs)
    cap = ops.activity_run_capacity(max_n, I)
    ld_ws = (need + 255) // 256 * 256 + 256
    cols, ld = max_n + 7, max_n + 7 + 13
    res = []
    for fill, (number, whole, byte) in FILLS.items():
        vview, vcheck = poison.guarded((1, B * 8), torch.float64, ld=B * 8 + 5, band_rows=8, device=DEV)
        cview, ccheck = poison.guarded((1, B * 15), torch.int64, ld=B * 15 + 3, band_rows=8, device=DEV)
        rview, rcheck = poison.guarded((1, B * cap * 2), torch.int64, ld=B * cap * 2 + 6, band_rows=8, device=DEV)
        wview, wcheck = poison.guarded((1, need), torch.uint8, ld=ld_ws, band_rows=2, device=DEV)
        oview, ocheck = poison.guarded((B, cols), torch.float32, ld=ld, band_rows=4, device=DEV)
        vview.fill_(number), oview.fill_(number), cview.fill_(whole), rview.fill_(whole), wview.fill_(byte)
        assert wview[0].data_ptr() % 256 == 0
        r = ops.activity(rows, fs, out={"values": vview[0].view(B, 8), "counts": cview[0].view(B, 15), "runs": rview[0].view(B, cap, 2)},
                         workspace=wview[0])
        out, gains, flags = ops.activity_normalise(rows, r["values"], -26.0, out=oview)
        torch.cuda.synchronize()
        for check in (vcheck, ccheck, rcheck, wcheck, ocheck):
            check()
        assert out is oview and poison.same_bits(flat, snap), "a read-only input changed"
        nr = r["values"][:, 6].to(torch.int64).tolist()
        assert all((r["runs"][b, nr[b]:] == whole).all() for b in range(B)), "an entry behind a row's runs was written"
        res.append((r["values"].clone(), r["counts"].clone(), torch.cat([r["runs"][b, :nr[b]].reshape(-1) for b in range(B)]),
                    oview.contiguous().clone(), gains.clone(), flags.clone()))
    for r in res[1:]:
        assert all(poison.same_bits(a, b) for a, b in zip(res[0], r))
    plain = ops.activity(on_device(xs), fs)
    assert poison.same_bits(plain["values"], res[0][0]) and poison.same_bits(plain["counts"], res[0][1])
    for i, x in enumerate(xs):
        want = reference(("mem", fs, i), x, fs)
        assert float(res[0][0][i, 6]) == want["runs"] and res[0][1][i].tolist() == want["counts"]
        assert not res[0][3][i, len(x):].any()
    for pattern in poison.PATTERNS:                                        # no result depends on uninitialised memory
        with poison.poisoned_empty(pattern) as spy:
            r = ops.activity(rows, fs)
            out, gains, flags = ops.activity_normalise(rows, r["values"], -26.0, cols=cols)
        assert spy.device_calls > 0, pattern
        nr = r["values"][:, 6].to(torch.int64).tolist()
        got = (r["values"], r["counts"], torch.cat([r["runs"][b, :nr[b]].reshape(-1) for b in range(B)]), out, gains, flags)
        assert all(poison.same_bits(a, b) for a, b in zip(res[0], got)), pattern


def test_metrics_surface_segments_trim_and_split():
    from simwhisper_codec_amd import metrics, ops
    fs = 8000
    dev = torch.device("cuda", torch.cuda.current_device())
    pad = lambda x: np.concatenate([np.zeros(int(0.3 * fs), np.float32), x, np.zeros(fs // 2, np.float32)])   # silence to trim
    xs = [pad(signal(11 * fs, fs, seed=3)), pad(signal(2 * fs + 7, fs, seed=91)), np.zeros(fs, np.float32)]
    rows = on_device(xs)
    base = ops.activity(rows, fs)["values"]
    q = metrics.active_level([torch.from_numpy(xs[0])] + rows[1:], sample_rate=fs, device=dev)             # host and device rows
    assert tuple(q) == metrics.ACTIVE_LEVEL_KEYS
    for k, want in zip(metrics.ACTIVE_LEVEL_KEYS, (base[:, 0], base[:, 1], base[:, 2], 20.0 * torch.log10(base[:, 3]), 20.0 * torch.log10(base[:, 4]))):
        assert q[k].shape == (3,) and q[k].dtype == torch.float64 and q[k].device == dev and poison.same_bits(q[k].contiguous(), want.contiguous()), k
    assert all(v.numel() == 0 for v in metrics.active_level([], fs, device=dev).values())
    want = [reference(("seg", fs, i), x, fs) for i, x in enumerate(xs)]
    segs = metrics.speech_segments(rows, fs, device=dev)
    assert segs == [ref.segments(w["run_list"], fs) for w in want] and segs[2] == [] and len(segs[0]) >= 4
    cut, bounds = metrics.trimmed(rows, fs, device=dev)
    assert bounds == [ref.trim(s) for s in segs] and bounds[2] == (0, 0) and cut[2].numel() == 0
    for r, c, (a, b) in zip(rows[:2], cut[:2], bounds[:2]):
        assert c.data_ptr() == r.data_ptr() + 4 * a and c.numel() == b - a and 0 < b - a < r.numel()     # a view of the input
    pieces, index = metrics.split_at_pauses(rows, fs, max_seconds=2.5, device=dev)
    assert index == [(i, a, b) for i, s in enumerate(segs) for a, b in ref.split(s, int(2.5 * fs))]
    assert len([i for i in index if i[0] == 0]) >= 4 and not any(i[0] == 2 for i in index)
    for p, (i, a, b) in zip(pieces, index):
        assert p.data_ptr() == rows[i].data_ptr() + 4 * a and p.numel() == b - a
    out, gains, flags = metrics.level_normalised(rows, fs, device=dev)
    o2, g2, f2 = ops.activity_normalise(rows, base, -26.0)
    assert poison.same_bits(gains, g2) and poison.same_bits(flags, f2) and flags.cpu().tolist() == [0, 0, ref.UNMEASURED]
    assert all(poison.same_bits(r.contiguous(), o2[i, :len(xs[i])].contiguous()) for i, r in enumerate(out))
    assert metrics.level_normalised([], fs, device=dev)[0] == [] and metrics.speech_segments([], fs, device=dev) == []


def _tiny_model(dev):
    import common
    from simwhisper_codec_amd.codec import AudioCodec
    model = AudioCodec(common.tiny_params(), precision="fp32")
    model.load_state_dict(common.state_dict("tiny"), strict=True)
    return model.to(dev).eval()


def test_audiocodec_encode_with_and_without_active_level():
    from simwhisper_codec_amd import _lib, metrics, synth
    dev = torch.device("cuda", torch.cuda.current_device())
    model = _tiny_model(dev)
    wavs = [synth.synth_audio(18000, index=0, kind="speech").to(dev), synth.synth_audio(17000, index=1, kind="speech").to(dev)]
    n = [18000, 17000]
    plain = model.encode(wavs)["codes_list"]
    explicit = model.encode(wavs, active_level=None)["codes_list"]
    batch = torch.zeros(2, 18000, device=dev)
    for i, w in enumerate(wavs):
        batch[i, :n[i]] = w
    padded = model.encode_padded(batch, n)                                   # the parent's codes of the same rows
    for i in range(2):
        T = n[i] // model.encoder_downsample_rate
        assert torch.equal(plain[i], explicit[i]) and torch.equal(plain[i].to(torch.int32), padded[:, i, :T])
    rows, gains, flags = metrics.level_normalised(wavs, 16000, device=dev)
    assert model.input_sample_rate == 16000 and set(flags.cpu().tolist()) <= {0, ref.PEAK_LIMITED}   # both rows are measured
    assert (gains - 1.0).abs().min() > 1e-3                                   # the normalisation does something here
    want = model.encode(rows)["codes_list"]
    got = model.encode(wavs, active_level=-26)["codes_list"]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with model.deferred_range_check() as chk:                                # no read-back: composes with the deferred check
        deferred = model.encode(wavs, active_level=-26.0)["codes_list"]
    assert not chk.clipped and all(torch.equal(a, b) for a, b in zip(deferred, want))
    with pytest.raises(_lib.SwcError, match="one of them"):
        model.encode(wavs, loudness=-23.0, active_level=-26.0)
    q = model.active_level(wavs)
    assert set(q) == {"ref", "deg", "active_level_db_diff", "long_term_db_diff", "activity_diff"} and tuple(q["ref"]) == metrics.ACTIVE_LEVEL_KEYS
    assert q["active_level_db_diff"].shape == (2,) and q["active_level_db_diff"].dtype == torch.float64
    assert poison.same_bits(q["ref"]["active_level_db"], metrics.active_level(wavs, 16000, device=dev)["active_level_db"])


def _write_wav(path, pcm, sr=16000):
    import struct
    raw = pcm.numpy().astype("<i2").tobytes()
    open(path, "wb").write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
                           struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16) + b"data" + struct.pack("<I", len(raw)) + raw)


def _wav_samples(path):
    raw = open(path, "rb").read()
    return (len(raw) - 44) // 2


def test_cli_trim_silence_active_level_and_the_tool(tmp_path, capsys):
    import os
    import sys
    import yaml
    import common
    import inference
    from simwhisper_codec_amd import bitstream, metrics, synth
    sys.path.insert(0, os.path.join(common.ROOT, "tools"))
    import measure_activity
    cfg = tmp_path / "tiny.yaml"
    cfg.write_text(yaml.safe_dump({"generator_params": common.tiny_params()}))
    ind = tmp_path / "in"
    ind.mkdir()
    fs = 16000
    names, pcms = ["a", "b", "c"], []
    for i, (name, n) in enumerate(zip(names, [fs * 2 + 123, 14000, fs])):
        speech = synth.synth_audio(n, index=60 + i, kind="speech").clamp(-1, 1) * 0.25
        lead, tail = (4000, 6000) if name != "c" else (0, 0)
        wav = torch.cat([torch.zeros(lead), speech if name != "c" else torch.zeros(n), torch.zeros(tail)])   # "c": silence, nothing to find
        pcm = (wav * 32767).round().to(torch.int16)
        _write_wav(str(ind / f"{name}.wav"), pcm)
        pcms.append(pcm)
    base = ["--config_path", str(cfg), "--synthetic_checkpoint", "--device", "cuda", "--batch_size", "3", "--precision", "mixed"]
    plain, trim, swc = (tmp_path / d for d in ("plain", "trim", "swc"))
    inference.main(base + ["--input_dir", str(ind), "--output_dir", str(plain)])
    inference.main(base + ["--trim_silence", "--input_dir", str(ind), "--output_dir", str(trim)])
    inference.main(base + ["--active_level", "-26", "--mode", "encode", "--input_dir", str(ind), "--output_dir", str(swc)])
    assert sorted(os.listdir(plain)) == sorted(os.listdir(trim)) == [f"{n}.wav" for n in names]
    dev = torch.device("cuda", torch.cuda.current_device())
    model = _tiny_model(dev)
    model.precision = "mixed"
    wavs = [p.to(dev).float() * (1.0 / 32768.0) for p in pcms]
    cut, bounds = metrics.trimmed(wavs, fs, device=dev)
    for name, w, c, (a, b) in zip(names, wavs, cut, bounds):
        kept = c if b > a else w                                               # no speech found: untrimmed
        for d, row in ((trim, kept), (plain, w)):                              # a trimmed round trip writes the trimmed length
            syn = model.decode(model.encode([row])["codes_list"])["syn_wav_list"][0]
            assert _wav_samples(str(d / f"{name}.wav")) == syn.numel(), (name, d)
    assert bounds[2] == (0, 0) and all(0 < b - a < w.numel() - 4000 for w, (a, b) in zip(wavs[:2], bounds[:2]))
    assert all(_wav_samples(str(trim / f"{n}.wav")) < _wav_samples(str(plain / f"{n}.wav")) for n in names[:2])
    assert _wav_samples(str(trim / "c.wav")) == _wav_samples(str(plain / "c.wav"))   # (its samples depend on the batch around it)
    codes = model.encode(wavs, active_level=-26.0)["codes_list"]
    for name, c in zip(names, codes):
        bitstream.write_codes(str(tmp_path / "want.swc"), c)
        assert (swc / f"{name}.swc").read_bytes() == (tmp_path / "want.swc").read_bytes(), name
    with pytest.raises(SystemExit, match="one of them"):
        inference.main(base + ["--active_level", "-26", "--loudness", "-23", "--input_dir", str(ind), "--output_dir", str(swc)])
    capsys.readouterr()
    assert measure_activity.main(["--input_dir", str(ind), "--batch_size", "2"]) == 0
    out = capsys.readouterr().out
    assert out.count("dBov") == 2 and "c.wav: not measured" in out and "left out of the means (1): c.wav" in out and "means over 2 files" in out
