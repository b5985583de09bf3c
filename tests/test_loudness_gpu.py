"""swc_loudness and swc_loudness_normalise on the GPU (include/swc_loudness.h) and the layers above them: the eight values
against the float64 restatement (tests/loudness_ref.py) at every edge of the block counts, four rates and three batch sizes; the
true peak against ops.resample bit for bit; independence of the batch around a row and of its alignment; the gain, the scaled
rows and the two flags; the memory contract in the manner of tests/test_codefile_gpu.py; AudioCodec.encode(loudness=) and
metrics.spectral(level=).  All pointers and lengths handed to the kernels are valid: nothing here provokes a fault.

Measured on the MI355X (profiles/loudness_bench.txt): the largest deviation of a dB output from the
reference over the cases below is 2.842e-14 LU (a few units in the last place of a double near 30: the K-weighting recursion
and the sums are float64 on both sides, in different orders); TOL is ten times that, rounded up to two digits."""
import math

import numpy as np
import pytest
import torch

import loudness_ref as ref
import poison

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2.9e-13                                # LU; see the docstring: 10 x the measured deviation, never above 1e-6
MARGIN = 1e-6                                # LU: no block of any case is closer to a gate than this (asserted on the CPU)
GAIN_MARGIN = 2.0 * TOL * math.log(10.0) / 20.0   # a dB deviation of TOL moves a gain by TOL ln(10) / 20 of itself
DB = (0, 1, 2, 3)


def signal(n, fs, seed):
    """n samples of seeded noise bursts and sines at stepped levels: steps of 0.7 s, levels between -20 and -75 dBFS (the last
    one under the absolute gate), so that both gates of I and of LRA have blocks on either side"""
    rng = np.random.default_rng(seed)
    levels = (-20.0, -35.0, -50.0, -26.0, -75.0, -30.0, -41.0)
    step = int(0.7 * fs)
    t = np.arange(n, dtype=np.float64) / fs
    x = np.zeros(n)
    for k in range(-(-n // step)):
        a, b = k * step, min((k + 1) * step, n)
        amp = 10.0 ** (levels[(k + seed) % len(levels)] / 20.0)
        if (k + seed) % 2:
            x[a:b] = amp * np.sin(2.0 * math.pi * (220.0 + 110.0 * ((k + seed) % 5)) * t[a:b])
        else:
            x[a:b] = amp * rng.standard_normal(b - a) * 0.5
    return x.astype(np.float32)


_REF = {}


def reference(key, x, fs):
    """the reference of one row, computed once per key and left alone"""
    if key not in _REF:
        m = ref.gate_margin(x, fs)
        assert m >= MARGIN, (key, m)          # a flipped block cannot hide in a tolerance: every case keeps its distance
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


def device_true_peak(x, fs):
    """the header's definition, on the device: the largest magnitude of what swc_resample returns from fs to 4 fs"""
    from simwhisper_codec_amd import ops
    if len(x) == 0:
        return 0.0
    y, n_out = ops.resample(on_device([x]), fs, 4 * fs)
    assert n_out == [4 * len(x)]
    return float(y[0, :n_out[0]].abs().max())


def compare(got, want, x, fs, what):
    """one row of values against the reference dict -> the largest deviation of its dB outputs"""
    worst = 0.0
    for i in DB:
        g, w = float(got[i]), want[ref.KEYS[i]]
        if math.isnan(w) or math.isinf(w):
            assert (math.isnan(g) and math.isnan(w)) or g == w, (what, ref.KEYS[i], g, w)
        else:
            assert abs(g - w) <= TOL, (what, ref.KEYS[i], g, w, abs(g - w))
            worst = max(worst, abs(g - w))
    assert float(got[4]) == want["sample_peak"], (what, "sample_peak")
    assert float(got[5]) == device_true_peak(x, fs), (what, "true_peak")               # bit for bit
    assert abs(float(got[5]) - want["true_peak"]) <= 1e-5 * max(want["true_peak"], 1e-30), (what, "true_peak against the host resampler")
    assert float(got[6]) == want["blocks"] and float(got[7]) == want["blocks_kept"], (what, "counts", got[6:], want)   # exact
    return worst


def edge_lengths(fs):
    L = fs // 10
    return [0, L - 1, 4 * L - 1, 4 * L, int(3.37 * fs)]


@pytest.mark.parametrize("fs", [8000, 16000, 44100, 48000])
def test_values_at_the_block_edges_batch_of_5(fs):
    from simwhisper_codec_amd import ops
    rows = [signal(n, fs, seed=2 + i) for i, n in enumerate(edge_lengths(fs))]
    want = [reference(("edge", fs, i), x, fs) for i, x in enumerate(rows)]
    assert [w["blocks"] for w in want] == [0, 0, 0, 1, 30] and math.isnan(want[2]["integrated"]) and math.isnan(want[3]["range"])
    assert want[3]["blocks_kept"] == 1 and not math.isnan(want[3]["integrated"]) and not math.isnan(want[3]["momentary_max"]) and math.isnan(want[3]["short_term_max"]) and not math.isnan(want[4]["short_term_max"])
    got = ops.loudness(on_device(rows), fs).cpu()
    worst = max(compare(got[i], want[i], rows[i], fs, (fs, i)) for i in range(5))
    print(f"fs={fs} B=5: largest deviation of a dB output {worst:.3e} LU")


def test_one_row_of_12_seconds():
    from simwhisper_codec_amd import ops
    fs = 48000
    x = signal(12 * fs, fs, seed=3)
    want = reference(("long", fs), x, fs)
    assert want["blocks"] == 117 and 0 < want["blocks_kept"] < 117 and want["range"] > 1.0
    got = ops.loudness(on_device([x]), fs).cpu()
    print(f"fs={fs} B=1, 12 s: largest deviation of a dB output {compare(got[0], want, x, fs, 'long'):.3e} LU")


def batch_of_33(fs=16000):
    """33 rows at fs: the short-term edge (30 L - 1, 30 L), an all-zero row, rows of many lengths; -> rows"""
    L = fs // 10
    lens = [30 * L - 1, 30 * L, 4 * fs] + [L * (3 + i) + 37 * i for i in range(28)] + [0, 31 * L + 1]
    rows = [signal(n, fs, seed=10 + i) for i, n in enumerate(lens)]
    rows[2] = np.zeros(4 * fs, np.float32)            # every block fails the absolute gate
    return rows


def test_batch_of_33_with_the_short_term_edge_a_silent_row_and_unaligned_views():
    from simwhisper_codec_amd import ops
    fs = 16000
    rows = batch_of_33(fs)
    want = [reference(("b33", fs, i), x, fs) for i, x in enumerate(rows)]
    assert math.isnan(want[0]["range"]) and want[0]["blocks"] == 26 and not math.isnan(want[1]["range"]) and want[1]["blocks"] == 27
    assert want[2]["blocks"] == 37 and want[2]["blocks_kept"] == 0 and math.isnan(want[2]["integrated"]) and want[2]["momentary_max"] == -math.inf
    got = ops.loudness(on_device(rows), fs).cpu()
    worst = max(compare(got[i], want[i], rows[i], fs, ("b33", i)) for i in range(33))
    print(f"fs={fs} B=33: largest deviation of a dB output {worst:.3e} LU")
    again = ops.loudness(unaligned(rows), fs).cpu()
    assert poison.same_bits(got, again)


def test_true_peak_between_the_samples():
    """a sine at fs / 4 sampled at 45 degrees: every sample is +-0.7071, the wave between them reaches 1.  The row fades in
    and out over 10 ms: a row that starts at full level is a step, whose own overshoot (1.2 %) is not what is looked at here"""
    from simwhisper_codec_amd import ops
    fs = 48000
    fade = 0.5 - 0.5 * np.cos(math.pi * np.minimum(np.arange(fs), np.arange(fs)[::-1]).clip(max=480) / 480.0)
    x = (fade * np.sin(0.5 * math.pi * np.arange(fs) + 0.25 * math.pi)).astype(np.float32)
    v = ops.loudness(on_device([x]), fs).cpu()[0]
    assert abs(float(v[4]) - math.sqrt(0.5)) < 1e-4 and abs(float(v[5]) - 1.0) <= 0.01
    assert float(v[5]) == device_true_peak(x, fs)


def test_a_rows_values_do_not_depend_on_the_batch_its_place_or_its_alignment():
    from simwhisper_codec_amd import ops
    fs = 16000
    rows = batch_of_33(fs)
    k = 32                                                      # 31 L + 1 samples: both filters, both gates, the selection
    alone = ops.loudness(on_device([rows[k]]), fs).cpu()[0]
    batch = ops.loudness(on_device(rows), fs).cpu()
    back = ops.loudness(on_device(rows[::-1]), fs).cpu()
    odd = ops.loudness(unaligned([rows[k]]), fs).cpu()[0]
    longer = ops.loudness(on_device([rows[k]]), fs, max_n_in=len(rows[k]) + 12345).cpu()[0]
    assert not torch.isnan(alone[:4]).any()
    for other in (batch[k], back[32 - k], odd, longer):
        assert poison.same_bits(alone, other)
    assert poison.same_bits(batch, back.flip(0))


def normalise_rows(fs=16000):
    """-> rows: ordinary ones, one whose click makes the ceiling bind, one too short to measure, one silent, one empty"""
    rows = [signal(int(3.37 * fs), fs, seed=21), signal(2 * fs + 13, fs, seed=22)]
    peaky = (10 ** (-40 / 20) * np.sin(2.0 * math.pi * 300.0 * np.arange(2 * fs) / fs)).astype(np.float32)
    peaky[fs] = 0.9
    return rows + [peaky, signal(fs // 10 * 4 - 1, fs, seed=23), np.zeros(fs, np.float32), np.zeros(0, np.float32)]


def test_normalise_gains_rows_and_flags():
    from simwhisper_codec_amd import ops
    fs = 16000
    rows = normalise_rows(fs)
    dev = on_device(rows)
    values = ops.loudness(dev, fs)
    cols = max(len(x) for x in rows) + 9
    out, gains, flags = ops.loudness_normalise(dev, values, -23.0, -1.0, cols=cols)
    gains, flags, out = gains.cpu(), flags.cpu().tolist(), out.cpu()
    want_flags = []
    for i, x in enumerate(rows):
        w = reference(("norm", fs, i), x, fs)
        g, f = ref.gain(w["integrated"], device_true_peak(x, fs), -23.0, -1.0)
        if f != ref.UNMEASURED:
            assert ref.f32_margin(g) >= GAIN_MARGIN, (i, g)      # the rounding to f32 cannot hinge on the last bits of I
        assert float(gains[i]) == float(np.float32(g)), (i, float(gains[i]), g)
        want_flags.append(f)
        n = len(x)
        assert poison.same_bits(out[i, :n], torch.from_numpy(x) * gains[i])       # one f32 multiply
        assert not out[i, n:].any()
    assert flags == want_flags == [0, 0, ref.PEAK_LIMITED, ref.UNMEASURED, ref.UNMEASURED, ref.UNMEASURED]
    assert float(gains[2]) * 0.9 < 10 ** (-1 / 20) * 1.02 and float(gains[0]) > 1.0
    # the normalised rows measure what the reference says of them: the target, up to the blocks the gain moves across a gate
    scaled = [out[i, :len(rows[i])].contiguous() for i in range(2)]
    after = ops.loudness([r.to(DEV) for r in scaled], fs).cpu()
    for i, r in enumerate(scaled):
        compare(after[i], reference(("scaled", fs, i), r.numpy(), fs), r.numpy(), fs, ("scaled", i))
    assert (after[:, 0] + 23.0).abs().max() < 0.5
    cut, _, _ = ops.loudness_normalise(dev, values, -23.0, -1.0, cols=1000)           # a longer row is cut at cols
    assert poison.same_bits(cut.cpu(), out[:, :1000].contiguous())


FILLS = {"zero": (0.0, 0x00), "poison": (math.nan, poison.U8_POISON), "ones": (poison.BIG, 0xFF)}   # (float windows, byte window)


def test_memory_contract():
    """values, the workspace and the normalised batch are poison.guarded windows with slack behind them (the batch with slack
    behind every row); whatever they held before, the results are the same bits, the slack and the bands keep what they held,
    and the rows (views with other samples around them) are unchanged"""
    from simwhisper_codec_amd import ops
    fs = 8000
    xs = [signal(n, fs, seed=40 + i) for i, n in enumerate([31 * 800 + 5, 0, 799, 4 * 800, 2701])]
    B, max_n = len(xs), max(len(x) for x in xs)
    flat = torch.full((sum(len(x) + 3 for x in xs) + 1,), 0.25, dtype=torch.float32, device=DEV)   # (what surrounds a row is audible)
    rows, at = [], 1
    for x in xs:
        flat[at:at + len(x)] = torch.from_numpy(x).to(DEV)
        rows.append(flat[at:at + len(x)])
        at += len(x) + 3
    snap = flat.clone()
    need = ops.loudness_workspace_bytes(B, max_n, fs)
    ld_ws = (need + 255) // 256 * 256 + 256
    cols, ld = max_n + 7, max_n + 7 + 13
    res = []
    for fill, (number, byte) in FILLS.items():
        vview, vcheck = poison.guarded((1, B * 8), torch.float64, ld=B * 8 + 5, band_rows=8, device=DEV)
        wview, wcheck = poison.guarded((1, need), torch.uint8, ld=ld_ws, band_rows=2, device=DEV)
        oview, ocheck = poison.guarded((B, cols), torch.float32, ld=ld, band_rows=4, device=DEV)
        vview.fill_(number), oview.fill_(number), wview.fill_(byte)
        assert wview[0].data_ptr() % 256 == 0
        values = ops.loudness(rows, fs, out={"values": vview[0].view(B, 8)}, workspace=wview[0])
        out, gains, flags = ops.loudness_normalise(rows, values, -23.0, -1.0, out=oview)
        torch.cuda.synchronize()
        for check in (vcheck, wcheck, ocheck):
            check()
        assert out is oview and poison.same_bits(flat, snap), "a read-only input changed"
        res.append((values.clone(), oview.contiguous().clone(), gains.clone(), flags.clone()))
    for r in res[1:]:
        assert all(poison.same_bits(a, b) for a, b in zip(res[0], r))
    plain = ops.loudness(on_device(xs), fs)
    assert poison.same_bits(plain, res[0][0])
    for i, x in enumerate(xs):
        assert not res[0][1][i, len(x):].any()
    for pattern in poison.PATTERNS:                                        # no result depends on uninitialised memory
        with poison.poisoned_empty(pattern) as spy:
            values = ops.loudness(rows, fs)
            out, gains, flags = ops.loudness_normalise(rows, values, -23.0, -1.0, cols=cols)
        assert spy.device_calls > 0, pattern
        assert all(poison.same_bits(a, b) for a, b in zip(res[0], (values, out, gains, flags))), pattern


def test_metrics_surface():
    from simwhisper_codec_amd import metrics, ops
    fs = 16000
    dev = torch.device("cuda", torch.cuda.current_device())
    xs = normalise_rows(fs)[:4]
    base = ops.loudness(on_device(xs), fs)
    q = metrics.loudness([torch.from_numpy(x) for x in xs[:2]] + on_device(xs[2:]), sample_rate=fs, device=dev)   # host and device rows
    assert tuple(q) == metrics.LOUDNESS_KEYS
    for i, k in enumerate(metrics.LOUDNESS_KEYS):
        assert q[k].shape == (4,) and q[k].dtype == torch.float64 and q[k].device == dev
        want = 20.0 * torch.log10(base[:, i]) if k.endswith("_db") else base[:, i]
        assert poison.same_bits(q[k].contiguous(), want.contiguous()), k
    assert set(metrics.loudness(on_device(xs), fs, device=dev, want=("integrated", "blocks"))) == {"integrated", "blocks"}
    assert all(v.numel() == 0 for v in metrics.loudness([], fs, device=dev).values())
    rows, gains, flags = metrics.normalised(on_device(xs), fs, device=dev)
    out, g2, f2 = ops.loudness_normalise(on_device(xs), base)
    assert [r.numel() for r in rows] == [len(x) for x in xs] and poison.same_bits(gains, g2) and poison.same_bits(flags, f2)
    assert all(poison.same_bits(r.contiguous(), out[i, :len(xs[i])].contiguous()) for i, r in enumerate(rows))
    assert rows[0]._base is rows[1]._base                                   # views of one batch
    assert metrics.normalised([], fs, device=dev)[0] == []
    # level_matched: the quieter copy comes back at the clean row's loudness; an unmeasured pair is left alone
    ref_rows = on_device(xs)
    deg_rows = [0.5 * r for r in ref_rows]
    matched, gm = metrics.level_matched(ref_rows, deg_rows, fs, device=dev)
    assert abs(float(gm[0]) - 2.0) < 1e-6 and abs(float(gm[1]) - 2.0) < 1e-6 and float(gm[3]) == 1.0
    assert poison.same_bits(matched[3].contiguous(), deg_rows[3].contiguous())
    assert torch.allclose(matched[0], ref_rows[0], rtol=1e-6, atol=0)


def _tiny_model(dev):
    import common
    from simwhisper_codec_amd.codec import AudioCodec
    model = AudioCodec(common.tiny_params(), precision="fp32")
    model.load_state_dict(common.state_dict("tiny"), strict=True)
    return model.to(dev).eval()


def test_audiocodec_encode_with_and_without_loudness():
    from simwhisper_codec_amd import metrics, synth
    dev = torch.device("cuda", torch.cuda.current_device())
    model = _tiny_model(dev)
    wavs = [synth.synth_audio(18000, index=0, kind="speech").to(dev), synth.synth_audio(17000, index=1, kind="speech").to(dev)]
    n = [18000, 17000]
    plain = model.encode(wavs)["codes_list"]
    explicit = model.encode(wavs, loudness=None)["codes_list"]
    batch = torch.zeros(2, 18000, device=dev)
    for i, w in enumerate(wavs):
        batch[i, :n[i]] = w
    padded = model.encode_padded(batch, n)                                   # the parent's codes of the same rows
    for i in range(2):
        T = n[i] // model.encoder_downsample_rate
        assert torch.equal(plain[i], explicit[i]) and torch.equal(plain[i].to(torch.int32), padded[:, i, :T])
    rows, gains, flags = metrics.normalised(wavs, model.input_sample_rate, device=dev)
    assert set(flags.cpu().tolist()) <= {0, ref.PEAK_LIMITED}                  # both rows are measured
    assert (gains - 1.0).abs().min() > 1e-3                                   # the normalisation does something here
    want = model.encode(rows)["codes_list"]
    got = model.encode(wavs, loudness=-23)["codes_list"]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with model.deferred_range_check() as chk:                                # no read-back: composes with the deferred check
        deferred = model.encode(wavs, loudness=-23.0, true_peak_db=-1.0)["codes_list"]
    assert not chk.clipped and all(torch.equal(a, b) for a, b in zip(deferred, want))
    q = model.loudness(wavs)
    assert set(q) == {"ref", "deg", "integrated_diff", "range_diff", "true_peak_db_diff"} and tuple(q["ref"]) == metrics.LOUDNESS_KEYS
    assert q["integrated_diff"].shape == (2,) and q["integrated_diff"].dtype == torch.float64 and q["integrated_diff"].device == dev
    assert poison.same_bits(q["ref"]["integrated"], metrics.loudness(wavs, model.input_sample_rate, device=dev)["integrated"])


def test_spectral_level_matching():
    from simwhisper_codec_amd import metrics, synth
    dev = torch.device("cuda", torch.cuda.current_device())
    refs = [synth.synth_audio(18000, index=0, kind="speech").to(dev), synth.synth_audio(17000, index=1, kind="speech").to(dev)]
    degs = [0.5 * r for r in refs]
    a = metrics.spectral(refs, degs, device=dev)
    b = metrics.spectral(refs, degs, device=dev, level=None)
    assert set(a) == set(b) and "gain_db" not in a
    for k in ("mel", "stft", "lsd", "parts"):
        assert poison.same_bits(a[k], b[k]), k
    same = metrics.spectral(refs, refs, device=dev)
    m = metrics.spectral(refs, degs, device=dev, level="loudness")
    assert m["gain_db"].shape == (2,) and (m["gain_db"] - 6.02).abs().max() <= 0.01
    for k in ("mel", "stft", "lsd"):
        # the matched rows are the clean rows to an f32 rounding of every sample: distances at the level of spectral(ref, ref),
        # far under what the 6 dB offset costs
        assert (m[k] - same[k]).abs().max() <= 1e-3 and float(a[k].min()) > 10.0 * max(float(m[k].max()), 1e-4), k


def _write_wav(path, pcm, sr=16000):
    import struct
    raw = pcm.numpy().astype("<i2").tobytes()
    open(path, "wb").write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
                           struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16) + b"data" + struct.pack("<I", len(raw)) + raw)


def test_cli_loudness_in_the_three_modes_and_the_tools(tmp_path, capsys):
    import os
    import sys
    import yaml
    import common
    import inference
    from simwhisper_codec_amd import bitstream, synth
    sys.path.insert(0, os.path.join(common.ROOT, "tools"))
    import evaluate_spectral
    import measure_loudness
    cfg = tmp_path / "tiny.yaml"
    cfg.write_text(yaml.safe_dump({"generator_params": common.tiny_params()}))
    ind = tmp_path / "in"
    ind.mkdir()
    names, pcms = ["a", "b", "c"], []
    for i, (name, n) in enumerate(zip(names, [16000 * 2 + 123, 14000, 500])):          # "c": too short to measure or to encode
        pcm = (synth.synth_audio(n, index=60 + i, kind="speech").clamp(-1, 1) * 0.25 * 32767).round().to(torch.int16)
        _write_wav(str(ind / f"{name}.wav"), pcm)
        pcms.append(pcm)
    base = ["--config_path", str(cfg), "--synthetic_checkpoint", "--device", "cuda", "--batch_size", "2", "--precision", "mixed"]
    plain, loud, swc, dec = (tmp_path / d for d in ("plain", "loud", "swc", "dec"))
    inference.main(base + ["--input_dir", str(ind), "--output_dir", str(plain)])
    inference.main(base + ["--loudness", "-23", "--input_dir", str(ind), "--output_dir", str(loud)])
    inference.main(base + ["--loudness", "-23", "--true_peak_db", "-2", "--mode", "encode", "--input_dir", str(ind), "--output_dir", str(swc)])
    inference.main(base + ["--loudness", "-20", "--mode", "decode", "--input_dir", str(swc), "--output_dir", str(dec)])
    assert sorted(os.listdir(plain)) == sorted(os.listdir(loud)) == sorted(os.listdir(dec)) == [f"{n}.wav" for n in names]
    assert (plain / "a.wav").read_bytes() != (loud / "a.wav").read_bytes()              # the input level moved, and so did the codes
    dev = torch.device("cuda", torch.cuda.current_device())
    model = _tiny_model(dev)
    model.precision = "mixed"
    for k in range(0, 3, 2):                                                             # the CLI's batches
        wavs = [p.to(dev).float() * (1.0 / 32768.0) for p in pcms[k:k + 2]]
        codes = model.encode(wavs, loudness=-23.0, true_peak_db=-2.0)["codes_list"]
        for name, c in zip(names[k:k + 2], codes):
            bitstream.write_codes(str(tmp_path / "want.swc"), c)
            assert (swc / f"{name}.swc").read_bytes() == (tmp_path / "want.swc").read_bytes(), name
    capsys.readouterr()
    assert measure_loudness.main(["--input_dir", str(ind), "--batch_size", "2"]) == 0
    out = capsys.readouterr().out
    assert out.count("LUFS") == 2 and "c.wav: not measured" in out and "left out of the means (1): c.wav" in out and "means over 2 files" in out
    assert evaluate_spectral.main(["--original_dir", str(plain), "--synthesized_dir", str(loud), "--level_match"]) == 0
    assert "mean level-match gain" in capsys.readouterr().out
