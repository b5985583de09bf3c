"""swc_pitch on the GPU against the numpy restatement of include/swc_pitch.h (tests/pitch_ref.py): tau and counts equal, f0
within one f32 ulp, the pair values against the header's formulas applied to the GPU's own stored tracks; the second rates,
the limit configuration, bit independence of everything that is not the row, the memory contract, NaN rows, and the Python
surface down to the tool."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pitch_ref as ref  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu

P16 = ref.params(16000)
SPAN, HOP = P16["W"] + P16["tau_max"], P16["H"]
POISON_ADDRESS = 0x10       # the "address" of a row with n_in = 0: never dereferenced
OUTPUTS = ("tau_x", "f0_x", "tau_y", "f0_y", "values", "counts")
FILLS = ("nan", "big", "zero")
# values against the formulas on the GPU's own tracks: the float64 sums of at most 200 terms err below 1e-12 relative, log2 is
# the only libm call (a few ulp of float64), then one f32 rounding (6e-8): 1e-6 leaves a factor ten
RTOL = 1e-6
SEED = 7
_CACHE = {}


def signals():
    """(clean, degraded): about 2 s at 16 kHz; the degraded side is the same signal plus noise with its second glide shifted
    in pitch by 30 %"""
    if "sig" not in _CACHE:
        _CACHE["sig"] = (ref.test_signal(SEED), ref.test_signal(SEED, shift=1.3, noise=0.002))
    return _CACHE["sig"]


def pair(start, n):
    x, y = signals()
    assert start + n <= len(x)
    return x[start:start + n].copy(), y[start:start + n].copy()


# lengths 0, 1, the four frame-count edges, and others that are multiples of nothing; starts that put every kind of stretch
# (glide, noise, zeros, square wave, quiet) first in some row
LENGTHS = (0, 1, SPAN - 1, SPAN, SPAN + HOP - 1, SPAN + HOP, 1531, 2777, 4099, 3001)
STARTS = (0, 6000, 11000, 17000, 20500, 25000, 9000)


def rows_of(B):
    """B rows: the whole signal first, then (start, length) pairs walking both tables"""
    n_all = len(signals()[0])
    specs = [(0, n_all)] + [(STARTS[k % len(STARTS)], LENGTHS[k % len(LENGTHS)]) for k in range(B - 1)]
    return specs[:B]


def reference(spec, p=None, key="16k"):
    """the reference of one (start, n) row pair, computed once"""
    p = p or P16
    k = (key, spec)
    if k not in _CACHE:
        _CACHE[k] = ref.pitch(*pair(*spec), **p)
    return _CACHE[k]


def run(pairs, p=None, want=OUTPUTS, fill="nan", offsets=None, max_n=None, ldt=None, with_y=True):
    """one swc_pitch call on guarded, pre-filled outputs and workspace -> dict of host tensors for the wanted outputs (tracks
    [B][ldt]: entries t >= T keep the fill) plus "before" (the fill of every output).  offsets[b] = (ox, oy): row b's samples
    start that many elements into their (16-byte aligned) allocations.  Outputs that were not asked for must keep their fill;
    nothing may be written outside the windows."""
    from simwhisper_codec_amd import _lib, ops
    lib = _lib.load()
    p = p or P16
    dev = torch.device("cuda", torch.cuda.current_device())
    B = len(pairs)
    offsets = offsets or [(0, 0)] * B
    keep, ptrs_x, ptrs_y, n_in = [], [], [], []
    for (x, y), offs in zip(pairs, offsets):
        n = len(x)
        n_in.append(n)
        for v, ptrs, off in ((x, ptrs_x, offs[0]), (y, ptrs_y, offs[1])):
            if n == 0:
                ptrs.append(POISON_ADDRESS)
                continue
            buf = torch.full((n + off,), float("nan"), device=dev)
            assert buf.data_ptr() % 16 == 0
            buf[off:] = torch.from_numpy(v)
            keep.append(buf)
            ptrs.append(buf.data_ptr() + 4 * off)
    max_n = max(n_in) if max_n is None else max_n
    T = ref.n_frames(max_n, p["W"], p["tau_max"], p["H"])
    ldt = max(T, 1) if ldt is None else ldt
    need = ops.pitch_workspace_bytes(B, max_n, p)
    shapes = {"values": (B, 8), "counts": (B, 4)}
    outs, checks = {}, []
    for name in OUTPUTS:
        dtype = torch.float32 if name in ("f0_x", "f0_y", "values") else torch.int32
        outs[name], chk = poison.guarded(shapes.get(name, (B, ldt)), dtype, device=dev)
        outs[name].zero_() if fill == "zero" else poison.fill_(outs[name], fill)
        checks.append(chk)
    before = {k: v.cpu().clone() for k, v in outs.items()}
    ws, check_w = poison.guarded((max(need // 256, 1), 256), torch.uint8, device=dev)
    assert ws.is_contiguous() and ws.data_ptr() % 256 == 0 and need % 256 == 0
    ws.zero_() if fill == "zero" else poison.fill_(ws.view(torch.float32), fill)
    meta = torch.tensor(ptrs_x + ptrs_y + n_in, dtype=torch.int64).to(dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    arg = lambda name: P(outs[name]) if name in want else None
    rc = lib.swc_pitch(P(meta[:B]), P(meta[B:2 * B]) if with_y else None, P(meta[2 * B:]), max_n, p["sr"], p["W"], p["tau_min"],
                       p["tau_max"], p["H"], arg("tau_x"), arg("f0_x"), arg("tau_y"), arg("f0_y"), ldt, arg("values"), arg("counts"),
                       P(ws), need, B, ops._stream())
    _lib.check(rc, "swc_pitch")
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


def row_bits(res, b, T):
    """what the call says about row b, as bytes: its T track entries and its values and counts"""
    parts = []
    for k in OUTPUTS:
        if k in res:
            v = res[k][b, :T] if k in ("tau_x", "f0_x", "tau_y", "f0_y") else res[k][b]
            parts.append(v.contiguous().view(torch.uint8).numpy().tobytes())
    return b"".join(parts)


def ulps(a, b):
    """the distance of two f32 arrays in units in the last place (both finite, same sign or zero)"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def compare(got, b, want):
    """row b of a call against its reference dict: tau and counts equal, f0 within 1 ulp (-> the largest seen), values against
    the formulas on the GPU's own tracks, entries t >= T untouched"""
    T = int(want["counts"][0])
    worst = 0
    for side in ("x", "y"):
        tau, f0 = got["tau_" + side][b].numpy(), got["f0_" + side][b].numpy()
        assert np.array_equal(tau[:T], want["tau_" + side]), (b, side)
        u = ulps(f0[:T], want["f0_" + side])
        worst = max(worst, int(u.max()) if T else 0)
        assert (u <= 1).all(), (b, side, int(u.max()))
        for k in ("tau_" + side, "f0_" + side):
            assert poison.same_bits(got[k][b, T:].contiguous(), got["before"][k][b, T:].contiguous()), (b, k, "t >= T was written")
    assert np.array_equal(got["counts"][b].numpy(), want["counts"]), (b, got["counts"][b], want["counts"])
    v_want, c_want = ref.pair_values(got["f0_x"][b, :T].numpy(), got["f0_y"][b, :T].numpy())
    assert np.array_equal(c_want, want["counts"])
    v = got["values"][b].numpy().astype(np.float64)
    assert np.array_equal(np.isnan(v), np.isnan(v_want)), (b, v, v_want)
    ok = ~np.isnan(v)
    assert (np.abs(v[ok] - v_want[ok]) <= RTOL * np.abs(v_want[ok])).all(), (b, v, v_want)
    return worst


def test_the_signal_reaches_every_measure():
    """on the CPU reference: no metric is tested on an empty set"""
    r = reference(rows_of(1)[0])
    T, n_vx, n_vy, n_vv = (int(v) for v in r["counts"])
    print("counts", r["counts"], "values", r["values"])
    assert 0 < n_vv < n_vx < T and 0 < n_vy < T
    v = r["values"]
    assert 0 < v[2] < 1 and 0 < v[3] < 1 and 0 < v[4] < 1 and v[0] > 100 and -1 < v[1] < 1
    quiet = ref.track(pair(26000, 4000)[0], **P16)[0]        # the quiet stretch alone is rescaled and voiced
    assert (quiet > 0).all()


@pytest.mark.parametrize("B", [1, 5, 33])
def test_tracks_counts_and_values(B):
    specs = rows_of(B)
    got = run([pair(*s) for s in specs])
    worst = max(compare(got, b, reference(s)) for b, s in enumerate(specs))
    print(f"B={B}: largest f0 distance {worst} ulp")
    if B == 33:
        assert {int(got["counts"][b, 0]) for b in range(B)} >= {0, 1, 2, 197}


def test_identical_rows_are_exact():
    specs = rows_of(5)
    rows = [(pair(*s)[0],) * 2 for s in specs]
    got = run(rows)
    for b in range(5):
        T, n_vx, n_vy, n_vv = (int(v) for v in got["counts"][b])
        assert poison.same_bits(got["f0_x"][b, :T].contiguous(), got["f0_y"][b, :T].contiguous()) and n_vx == n_vy == n_vv
        v = got["values"][b]
        if n_vv > 0:
            assert float(v[0]) == 0.0 and float(v[2]) == 0.0 and float(v[3]) == 0.0 and float(v[4]) == 1.0, (b, v)
        elif T > 0:
            assert float(v[3]) == 0.0 and math.isnan(float(v[0])) and math.isnan(float(v[4])), (b, v)
        else:
            assert torch.isnan(v[:7]).all(), (b, v)
    assert int(got["counts"][0, 3]) > 100


@pytest.mark.parametrize("sr", [8000, 48000])
def test_a_second_rate(sr):
    p = ref.params(sr)
    span = p["W"] + p["tau_max"]
    n = span + 7 * p["H"] + 3
    x = np.concatenate([ref.harmonic_complex(np.linspace(110.0, 170.0, n - 2 * p["H"]), n - 2 * p["H"], sr), np.zeros(2 * p["H"], np.float32)])
    y = (ref.harmonic_complex(np.linspace(113.0, 160.0, n), n, sr) + 0.002 * np.random.default_rng(1).standard_normal(n)).astype(np.float32)
    want = ref.pitch(x, y, **p)
    assert int(want["counts"][0]) == 8 and int(want["counts"][3]) > 0
    got = run([(x, y), (x[:span - 1], y[:span - 1])], p=p)
    print(f"{sr} Hz: {p}, largest f0 distance {compare(got, 0, want)} ulp")
    compare(got, 1, ref.pitch(x[:span - 1], y[:span - 1], **p))


def test_the_limit_configuration():
    """W = 2048, tau_max = 1024 on the full-scale alternating row (every product the largest there is: 64-bit accumulation, d tau
    near 2^53, the packed products) and on a glide"""
    p = dict(sr=48000, W=2048, tau_min=2, tau_max=1024, H=331)
    n = 3072 + 2 * 331 + 5
    alt = ref.alternating(n)
    glide = ref.harmonic_complex(np.linspace(74.0, 76.0, n), n, 48000)
    full = np.sign(glide).astype(np.float32)          # +-1: every |q| is 32767
    top = ref.alternating(n, ref.TOP)                 # +-32767 where the +-1 row is +-16384
    want = [ref.pitch(alt, glide, **p), ref.pitch(full, alt, **p), ref.pitch(top, full * ref.TOP, **p)]
    assert list(want[0]["tau_x"]) == [2, 2, 2] and (want[0]["tau_y"] > 600).all() and (want[1]["tau_x"] > 600).all()
    assert list(want[2]["tau_x"]) == [2, 2, 2] and (want[2]["tau_y"] > 600).all()
    got = run([(alt, glide), (full, alt), (top, full * ref.TOP)], p=p)
    print("limit configuration: largest f0 distance", max(compare(got, b, w) for b, w in enumerate(want)), "ulp")


def test_bits_do_not_depend_on_anything_but_the_row():
    specs = rows_of(5)
    pairs = [pair(*s) for s in specs]
    base = run(pairs)
    T = [int(v) for v in base["counts"][:, 0]]
    bits = [row_bits(base, b, T[b]) for b in range(5)]
    # B and the row's index: each row alone, and the batch reversed
    for b in (0, 3, 4):
        alone = run(pairs[b:b + 1])
        assert row_bits(alone, 0, T[b]) == bits[b], b
    rev = run(pairs[::-1])
    assert [row_bits(rev, 4 - b, T[b]) for b in range(5)] == bits
    # rows 4, 8 and 12 bytes off a 16-byte boundary
    off = run(pairs, offsets=[(1, 3), (0, 0), (2, 1), (3, 2), (1, 1)])
    assert [row_bits(off, b, T[b]) for b in range(5)] == bits
    # a wider length bound and a wider track stride: other grids, another workspace layout
    wide = run(pairs, max_n=40000, ldt=300)
    assert [row_bits(wide, b, T[b]) for b in range(5)] == bits
    # a longer row is cut at max_n_in
    n1 = len(pairs[1][0])
    longer = run([(np.concatenate([x, x[:50]]), np.concatenate([y, y[:50]])) for x, y in pairs[1:2]], max_n=n1)
    assert row_bits(longer, 0, T[1]) == bits[1]
    # which outputs are asked for
    for want in (("values",), ("counts",), ("f0_y",), ("tau_x", "counts"), ("f0_x", "tau_y", "values")):
        part = run(pairs, want=want)
        for k in want:
            assert poison.same_bits(part[k], base[k]), (want, k)


def test_without_degraded_rows_the_call_is_the_clean_half():
    specs = rows_of(5)
    pairs = [pair(*s) for s in specs]
    base = run(pairs)
    only = run(pairs, want=("tau_x", "f0_x", "counts"), with_y=False)
    assert poison.same_bits(only["tau_x"], base["tau_x"]) and poison.same_bits(only["f0_x"], base["f0_x"])
    assert torch.equal(only["counts"][:, :2], base["counts"][:, :2]) and not only["counts"][:, 2:].any()
    assert poison.same_bits(run(pairs, want=("f0_x",), with_y=False)["f0_x"], base["f0_x"])


def test_memory_contract_and_fill_independence():
    """outputs and workspace are pre-filled three ways and guarded (run() checks the bands and compare() the entries t >= T);
    the results must not depend on what the workspace or the outputs held"""
    specs = rows_of(5)
    pairs = [pair(*s) for s in specs]
    res = [run(pairs, fill=f, ldt=250) for f in FILLS]
    T = [int(v) for v in res[0]["counts"][:, 0]]
    assert max(T) < 250
    for b, s in enumerate(specs):
        for r in res:
            compare(r, b, reference(s))
        assert row_bits(res[0], b, T[b]) == row_bits(res[1], b, T[b]) == row_bits(res[2], b, T[b]), b


def test_nan_in_one_row_stays_in_that_row():
    specs = rows_of(5)
    pairs = [pair(*s) for s in specs]
    base = run(pairs)
    T = [int(v) for v in base["counts"][:, 0]]
    hit_pairs = [(x.copy(), y.copy()) for x, y in pairs]
    hit_pairs[0][1][20000] = np.nan          # the degraded side of row 0
    hit_pairs[4][0][17] = np.inf             # the clean side of row 4
    hit = run(hit_pairs)
    for b in (1, 2, 3):
        assert row_bits(hit, b, T[b]) == row_bits(base, b, T[b]), b
    for b, bad, good in ((0, "y", "x"), (4, "x", "y")):
        assert T[b] > 0
        assert torch.isnan(hit["values"][b, :7]).all() and float(hit["values"][b, 7]) == 0.0
        assert hit["counts"][b].tolist() == [T[b], 0, 0, 0]
        assert torch.isnan(hit["f0_" + bad][b, :T[b]]).all() and (hit["tau_" + bad][b, :T[b]] == -1).all()
        assert poison.same_bits(hit["f0_" + good][b, :T[b]].contiguous(), base["f0_" + good][b, :T[b]].contiguous())
        assert poison.same_bits(hit["tau_" + good][b, :T[b]].contiguous(), base["tau_" + good][b, :T[b]].contiguous())


def test_python_surface_matches_the_c_call():
    from simwhisper_codec_amd import metrics
    dev = torch.device("cuda", torch.cuda.current_device())
    specs = rows_of(5)
    pairs = [pair(*s) for s in specs]
    base = run(pairs)
    T = [int(v) for v in base["counts"][:, 0]]
    xs = [torch.from_numpy(x) for x, _ in pairs]
    ys = [torch.from_numpy(y).to(dev) for _, y in pairs]          # host rows and device rows mixed
    q = metrics.pitch(xs, ys, sample_rate=16000, device=dev, tracks=True)
    assert set(q) == set(metrics.PITCH_KEYS) | {"frames", "tracks_ref", "tracks_deg"}
    for i, k in enumerate(metrics.PITCH_KEYS):
        assert q[k].shape == (5,) and q[k].dtype == torch.float32 and q[k].device == dev
        assert poison.same_bits(q[k].cpu().contiguous(), base["values"][:, i].contiguous()), k
    assert q["frames"].cpu().tolist() == T
    for b in range(5):
        for tr, side in ((q["tracks_ref"], "x"), (q["tracks_deg"], "y")):
            f0, voiced = tr[b]
            assert f0.shape == voiced.shape == (T[b],) and voiced.dtype == torch.bool
            assert poison.same_bits(f0.cpu().contiguous(), base["f0_" + side][b, :T[b]].contiguous())
            assert torch.equal(voiced.cpu(), base["tau_" + side][b, :T[b]] > 0)
    one = metrics.pitch(xs, ys, sample_rate=16000, device=dev, want=("gpe",))
    assert set(one) == {"gpe", "frames"} and poison.same_bits(one["gpe"].cpu().contiguous(), base["values"][:, 2].contiguous())
    tracks = metrics.f0(xs, sample_rate=16000, device=dev)
    assert len(tracks) == 5
    for b, (f0, voiced) in enumerate(tracks):
        assert poison.same_bits(f0.cpu().contiguous(), base["f0_x"][b, :T[b]].contiguous()) and int(voiced.sum()) == int(base["counts"][b, 1])
    empty = metrics.pitch([], [], device=dev)
    assert all(empty[k].numel() == 0 for k in metrics.PITCH_KEYS) and metrics.f0([], device=dev) == []


def test_audiocodec_pitch_on_the_synthetic_checkpoint():
    import common
    from simwhisper_codec_amd import metrics, synth
    from simwhisper_codec_amd.codec import AudioCodec
    dev = torch.device("cuda", torch.cuda.current_device())
    model = AudioCodec(common.tiny_params(), precision="fp32")
    model.load_state_dict(common.state_dict("tiny"), strict=True)
    model = model.to(dev).eval()
    wavs = [synth.synth_audio(18000, index=0, kind="speech").to(dev), synth.synth_audio(17000, index=1, kind="speech").to(dev)]
    q = model.pitch(wavs, tracks=True)
    assert set(q) == set(metrics.PITCH_KEYS) | {"frames", "tracks_ref", "tracks_deg"}
    for k in metrics.PITCH_KEYS:
        assert q[k].shape == (2,) and q[k].device == dev and q[k].dtype == torch.float32, k
    print("AudioCodec.pitch:", {k: q[k].cpu().tolist() for k in metrics.PITCH_KEYS}, q["frames"].cpu().tolist())
    frames = q["frames"].cpu().tolist()
    # a pair is cut to the shorter of the input and its reconstruction (whole code frames): at most the input's frame count
    full = [ref.n_frames(18000, 512, 256, 160), ref.n_frames(17000, 512, 256, 160)]
    assert all(f - 3 <= g <= f for g, f in zip(frames, full)), (frames, full)
    assert torch.isfinite(q["vde"]).all() and ((q["vde"] >= 0) & (q["vde"] <= 1)).all()
    # equal to the C call on what the codec gave back: the clean track is that of the input, cut as the pair was
    syn = model.decode(model.encode(wavs)["codes_list"])["syn_wav_list"]
    cut = [w[:min(w.numel(), s.numel())] for w, s in zip(wavs, syn)]
    assert [ref.n_frames(c.numel(), 512, 256, 160) for c in cut] == frames
    mine = metrics.f0(cut, sample_rate=16000, device=dev)
    for b in range(2):
        assert poison.same_bits(mine[b][0].cpu().contiguous(), q["tracks_ref"][b][0].cpu().contiguous())
        assert q["tracks_deg"][b][0].shape == (frames[b],)
        want, _ = ref.pair_values(q["tracks_ref"][b][0].cpu().numpy(), q["tracks_deg"][b][0].cpu().numpy())
        got = np.array([float(q[k][b]) for k in metrics.PITCH_KEYS])
        assert np.array_equal(np.isnan(got), np.isnan(want[:7]))
        ok = ~np.isnan(got)
        assert (np.abs(got[ok] - want[:7][ok]) <= RTOL * np.abs(want[:7][ok])).all()


def test_evaluate_tool_on_a_two_file_directory_pair(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_pitch
    from evaluate_stoi import load_first_channel
    from simwhisper_codec_amd import metrics, wavio
    fs = 16000
    dev = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(tmp_path / "orig"); os.makedirs(tmp_path / "syn")
    for i, spec in enumerate(((0, 12000), (9000, 9000))):
        x, y = pair(*spec)
        wavio.save_audio(str(tmp_path / "orig" / f"utt{i}.wav"), torch.from_numpy(x), fs)
        wavio.save_audio(str(tmp_path / "syn" / f"utt{i}.wav"), torch.from_numpy(y[: len(y) - 5 * i]), fs)   # cut to the shorter
    xs = [load_first_channel(str(tmp_path / "orig" / f"utt{i}.wav"), fs) for i in range(2)]
    ys = [load_first_channel(str(tmp_path / "syn" / f"utt{i}.wav"), fs) for i in range(2)]
    q = metrics.pitch(xs, ys, sample_rate=fs, device=dev)
    assert evaluate_pitch.main(["--original_dir", str(tmp_path / "orig"), "--synthesized_dir", str(tmp_path / "syn"),
                                "--batch_size", "1", "--verbose"]) == 0
    out = capsys.readouterr().out
    print(out)
    cols = {k: [float(v) for v in q[k].cpu()] for k in evaluate_pitch.KEYS}
    for line in evaluate_pitch.format_summary(evaluate_pitch.summarise(["utt0.wav", "utt1.wav"], cols), 2):
        assert line in out, line
    assert "mean F0 RMSE (cents):" in out and "of 2 files" in out
    assert all(not math.isnan(v) for v in cols["vde"])
