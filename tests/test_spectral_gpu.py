"""swc_spectral (include/swc_spectral.h) on the GPU against the float64 restatement of the contract (tests/spectral_ref.py).

Values: |gpu - f64| <= 1e-4 |f64| + 1e-6 for mel, stft, lsd and every entry of parts: ten times the condition the inputs
meet in a float32 numpy run of the same steps (tests/test_spectral_cpu.py, asserted again here about every row used), which
leaves room for another summation order, the device's log10f and sqrtf and the f32 table.  Identical rows: exactly 0.0.

Shapes: at most 3 pairs x 18000 samples.  Lengths 1 .. 2049 are the frame-count steps of H = 8 and H = 512 and the edge frames
that read zeros on both sides; 8191, 8192, 8193 are the run boundary R_W H of every window; one case of 18000 samples per
rate.  The float64 results are computed once per case, shared, and never written to.  Each case prints the deviation it saw
(pytest -s)."""
import ctypes as C
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import poison  # noqa: E402
import spectral_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-6
CONDITION = 1e-5
POISON_ADDRESS = 0x10       # the "address" of a row with n_in = 0: never dereferenced
OUTPUTS = ("mel", "stft", "lsd", "parts")
EMPTY = (np.zeros(0, np.float32),) * 2
ALL = ref.MEL | ref.STFT | ref.LSD
SNRS = (20, 0, 10)


def _rows(lengths, fs, seed0=0):
    return [ref.pair(n, fs, SNRS[k % 3], seed=(seed0 + k) % 4) for k, n in enumerate(lengths)]


GROUPS = [ref.VALUE_LENGTHS[i:i + 3] for i in range(0, len(ref.VALUE_LENGTHS), 3)]
CASES = [f"lengths_{g[0]}_16000" for g in GROUPS] + [f"{kind}_{fs}" for fs in ref.RATES for kind in ("run_edges", "18000")]
_CACHE = {}


def _pairs(name):
    """name -> (sample_rate, [(x, y), ...]), built on first use"""
    kind, fs = name.rsplit("_", 1)
    fs = int(fs)
    if kind == "run_edges":
        return fs, _rows((8191, 8192, 8193), fs, 1)
    if kind == "18000":
        return fs, [ref.pair(18000, fs, snr, seed=k) for k, snr in enumerate((40, 20, 0))]
    i = [g[0] for g in GROUPS].index(int(kind.split("_")[1]))
    return fs, _rows(GROUPS[i], fs, 3 * i)


def reference(key, fs, pairs, scales=None):
    """float64 results of the rows, built once; the float32 condition on the inputs is asserted here, before the GPU is touched"""
    if key not in _CACHE:
        refs = []
        for b, (x, y) in enumerate(pairs):
            a = ref.spectral(x, y, fs, scales)
            if len(x):
                c = ref.spectral(x, y, fs, scales, dtype=np.float32)
                nz = (a["parts"] != 0)
                cond = float((np.abs(c["parts"] - a["parts"])[nz] / np.abs(a["parts"][nz])).max()) if nz.any() else 0.0
                assert cond <= CONDITION, (key, b, cond)
                assert np.isfinite(x).all() and np.isfinite(y).all()
            refs.append(a)
        _CACHE[key] = refs
    return _CACHE[key]


def case(name):
    """(sample_rate, pairs, float64 results): built once, shared, never written to"""
    if ("pairs", name) not in _CACHE:
        _CACHE[("pairs", name)] = _pairs(name)
    fs, pairs = _CACHE[("pairs", name)]
    return fs, pairs, reference(("ref", name), fs, pairs)


def make_table(fs, scales, dev, banks=None):
    """the `table` of ops.spectral for any scale list"""
    from simwhisper_codec_amd import metrics
    dense = [metrics.mel_filterbank(fs, W, M) if M > 0 else np.zeros((0, W // 2 + 1)) for W, M, _ in scales] if banks is None else banks
    first, count, off, w = metrics.pack_filterbanks(dense)
    t = {"win": [s[0] for s in scales], "n_mels": [s[1] for s in scales], "flags": [s[2] for s in scales]}
    for k, v in (("first", first), ("count", count), ("off", off), ("w", w)):
        t[k] = torch.from_numpy(v).to(dev)
    return t


def run(pairs, fs, want=OUTPUTS, pattern="nan", offsets=None, max_n=None, table=None):
    """one swc_spectral call on guarded, poisoned outputs and workspace -> dict of host tensors for the wanted outputs.
    offsets[b] = (ox, oy): row b's samples start that many elements into their (16-byte aligned) allocations.  Outputs that
    were not asked for must keep their poison; nothing may be written outside the windows."""
    from simwhisper_codec_amd import _lib, metrics, ops
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    table = metrics.spectral_table(fs, dev) if table is None else table
    B, S = len(pairs), len(table["win"])
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
    L = ops.spectral_workspace_layout(B, max_n, table["win"])
    assert L["total"] == ops.spectral_workspace_bytes(B, max_n, table["win"]) and L["total"] % 256 == 0
    outs, checks = {}, []
    for name in OUTPUTS:
        outs[name], chk = poison.guarded((B, S * 4) if name == "parts" else (B,), torch.float32, device=dev)
        poison.fill_(outs[name], pattern)
        checks.append(chk)
    before = {k: v.cpu().clone() for k, v in outs.items()}
    ws, check_w = poison.guarded((max(L["total"] // 256, 1), 256), torch.uint8, device=dev)
    assert ws.is_contiguous() and ws.data_ptr() % 256 == 0 and outs["parts"].is_contiguous()
    poison.fill_(ws.view(torch.float64), pattern)
    meta = torch.tensor(ptrs_x + ptrs_y + n_in, dtype=torch.int64).to(dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    arg = lambda name: P(outs[name]) if name in want else None
    i32 = lambda v: (C.c_int32 * len(v))(*v)
    rc = lib.swc_spectral(P(meta[:B]), P(meta[B:2 * B]), P(meta[2 * B:]), max_n, i32(table["win"]), i32(table["n_mels"]),
                          i32(table["flags"]), S, P(table["first"]), P(table["count"]), P(table["off"]), P(table["w"]),
                          table["w"].numel(), arg("mel"), arg("stft"), arg("lsd"), arg("parts"), P(ws), L["total"], B, ops._stream())
    _lib.check(rc, "swc_spectral")
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    check_w()
    res = {}
    for name in OUTPUTS:
        got = outs[name].cpu().clone()
        if name in want:
            res[name] = got.reshape(B, S, 4) if name == "parts" else got
        else:
            assert poison.same_bits(got, before[name]), f"{name} was not asked for and was written"
    return res


def _same(a, b):
    return set(a) == set(b) and all(poison.same_bits(a[k], b[k]) for k in a)


def compare(name, got, refs):
    """every value of every row against float64; -> the worst deviation in units of the bound"""
    worst, worst_rel = 0.0, 0.0
    for b, r in enumerate(refs):
        pairs = [(k, float(got[k][b]), float(r[k])) for k in ("mel", "stft", "lsd") if k in got]
        if "parts" in got:
            pairs += [(f"parts[{s}][{j}]", float(got["parts"][b, s, j]), float(r["parts"][s, j]))
                      for s in range(r["parts"].shape[0]) for j in range(4)]
        row = 0.0
        for k, v, want in pairs:
            if math.isnan(want):
                assert math.isnan(v), (name, b, k, v)
                continue
            assert math.isfinite(v), (name, b, k, v)
            if want == 0.0:
                assert v == 0.0, (name, b, k, v)
                continue
            err = abs(v - want)
            row = max(row, err / (RTOL * abs(want) + ATOL))
            worst_rel = max(worst_rel, err / abs(want))
            assert err <= RTOL * abs(want) + ATOL, (name, b, k, v, want, err)
        print(f"{name} row {b}: " + " ".join(f"{k} {v:.6f}/{w:.6f}" for k, v, w in pairs[:3]) + f" worst |diff| / bound {row:.3f}")
        worst = max(worst, row)
    print(f"{name}: worst |gpu - f64| / (1e-4 |f64| + 1e-6) = {worst:.3f}, worst relative {worst_rel:.2e}")
    return worst


@pytest.mark.parametrize("name", CASES)
def test_values_against_float64(name):
    fs, pairs, refs = case(name)
    compare(name, run(pairs, fs), refs)


def test_the_cases_reach_the_branches_they_are_named_for():
    from simwhisper_codec_amd import _lib
    lengths = sorted(len(x) for n in CASES if n.startswith("lengths_") for x, _ in case(n)[1])
    assert lengths == sorted(ref.VALUE_LENGTHS) and {1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049} <= set(lengths)
    for W in ref.WINDOWS:
        edge = _lib.SPECTRAL_RUN[W] * (W // 4)
        assert {edge - 1, edge, edge + 1} <= set(lengths)
        T = lambda n: 1 + n // (W // 4)
        assert math.ceil(T(edge - 1) / _lib.SPECTRAL_RUN[W]) == 1 and math.ceil(T(edge) / _lib.SPECTRAL_RUN[W]) == 2
    assert {int(n.rsplit("_", 1)[1]) for n in CASES} == set(ref.RATES)
    assert [len(x) for x, _ in case("run_edges_48000")[1]] == [8191, 8192, 8193]
    assert max(len(GROUPS[k]) for k in range(len(GROUPS))) == 3 and max(ref.VALUE_LENGTHS) < 18000


@pytest.mark.parametrize("W", ref.WINDOWS)
def test_every_window_as_a_single_scale_call(W):
    """one scale with all three flags: STFT and LSD run at every window, not only at 512 and 2048"""
    dev = torch.device("cuda", torch.cuda.current_device())
    M = ref.MELS[ref.WINDOWS.index(W)]
    scales = [(W, M, ALL)]
    pairs = _rows((8193, 2049, 513), 16000, 2)
    refs = reference(("single", W), 16000, pairs, scales)
    got = run(pairs, 16000, table=make_table(16000, scales, dev))
    compare(f"single_{W}", got, refs)
    # the scale's numbers are those it has inside the full list (mel_s always; logmag_s, mag_s, lsd_s where the list flags them)
    if ("full", "single") not in _CACHE:
        _CACHE[("full", "single")] = run(pairs, 16000)
    full = _CACHE[("full", "single")]
    s = ref.WINDOWS.index(W)
    fl = ref.default_scales()[s][2]
    cols = [0] + ([1, 2] if fl & ref.STFT else []) + ([3] if fl & ref.LSD else [])
    assert poison.same_bits(full["parts"][:, s, cols].contiguous(), got["parts"][:, 0, cols].contiguous())


def test_identical_rows_give_exactly_zero_and_ten_times_gives_seven_and_two():
    xs = [ref.pair(n, 16000, 20, seed=k)[0] for k, n in enumerate((1, 513, 8193))]
    got = run([(x, x.copy()) for x in xs], 16000)
    for k in OUTPUTS:
        assert not got[k].any() and not torch.signbit(got[k]).any(), k           # +0.0, every bit
    fs, x, y = ref.case_table()["white_x10_16000"]
    r = reference(("x10", fs), fs, [(x, y)])
    assert r[0]["clamped"] == 0
    got = run([(x, y)], fs)
    compare("ten_times", got, r)
    assert abs(float(got["mel"][0]) - 7.0) <= RTOL * 7.0 + ATOL and abs(float(got["lsd"][0]) - 2.0) <= RTOL * 2.0 + ATOL
    for s, (_, _, fl) in enumerate(ref.default_scales()):
        assert abs(float(got["parts"][0, s, 0]) - 1.0) <= RTOL + ATOL
        if fl & ref.STFT:
            assert abs(float(got["parts"][0, s, 1]) - 2.0) <= RTOL * 2.0 + ATOL


def _full(name="run_edges_16000"):
    key = ("full", name)
    if key not in _CACHE:
        fs, pairs, _ = case(name)
        _CACHE[key] = run(pairs, fs)
    return _CACHE[key]


SUBSETS = [c for k in (1, 2, 3) for c in itertools.combinations(OUTPUTS, k)]


@pytest.mark.parametrize("want", SUBSETS, ids=["+".join(c) for c in SUBSETS])
def test_a_subset_of_the_outputs_has_the_bits_of_the_full_call(want):
    """run() asserts that an output that was not asked for keeps its poison"""
    fs, pairs, _ = case("run_edges_16000")
    part = run(pairs, fs, want=want)
    assert set(part) == set(want)
    for k in part:
        assert poison.same_bits(part[k], _full()[k]), k


def test_bits_do_not_depend_on_batch_position_alignment_or_the_length_bound():
    fs, pairs, _ = case("run_edges_16000")
    alone = run(pairs[2:3], fs)
    other = case("lengths_2049_16000")[1]
    three = run([other[0], other[1], pairs[2]], fs, offsets=[(0, 0), (0, 0), (1, 1)])     # row 2, 4 bytes off a 16-byte boundary
    for k in OUTPUTS:
        assert poison.same_bits(alone[k][0:1], three[k][2:3]), k
        assert poison.same_bits(_full()[k][2:3], alone[k][0:1]), k
    wide = run(pairs[2:3], fs, max_n=18000)                                               # another layout, other grids
    assert _same(alone, wide)
    cut = run([(np.concatenate([x, x[:100]]), np.concatenate([y, y[:100]])) for x, y in pairs[2:3]], fs, max_n=8193)
    assert _same(alone, cut)                                                              # a longer row is cut at max_n_in


@pytest.mark.parametrize("B", [1, 3, 33])
def test_an_empty_row_gives_nan_and_leaves_the_others_alone(B):
    fs, pairs, _ = case("lengths_513_16000")
    rows = [pairs[k % 3] for k in range(B)]
    base = run(rows, fs)
    at = B // 2
    rows[at] = EMPTY
    hit = run(rows, fs)
    flags = [s[2] for s in ref.default_scales()]
    for b in range(B):
        for k in OUTPUTS:
            if b != at:
                assert poison.same_bits(base[k][b:b + 1], hit[k][b:b + 1]), (b, k)
                assert poison.same_bits(base[k][b:b + 1], base[k][b % 3:b % 3 + 1]), (b, k)
    assert all(math.isnan(float(hit[k][at])) for k in ("mel", "stft", "lsd"))
    for s, fl in enumerate(flags):
        want = [True, bool(fl & ref.STFT), bool(fl & ref.STFT), bool(fl & ref.LSD)]
        got = hit["parts"][at, s]
        assert [math.isnan(float(v)) for v in got] == want and all(float(v) == 0.0 for v, w in zip(got, want) if not w)


def test_memory_contract_and_poison_independence():
    """outputs and workspace are poisoned before the call and guarded (run() checks the bands); the results must not depend on
    what the workspace or the outputs held"""
    for name in ("run_edges_16000", "lengths_1_16000"):
        fs, pairs, _ = case(name)
        a = run(pairs, fs, pattern="nan")
        b = run(pairs, fs, pattern="big")
        assert _same(a, b)
        assert all(torch.isfinite(a[k]).all() for k in OUTPUTS)
    fs, pairs, _ = case("lengths_513_16000")
    rows = [pairs[0], EMPTY, pairs[1]]
    assert _same(run(rows, fs, pattern="nan"), run(rows, fs, pattern="big"))


def test_nan_in_one_row_stays_in_that_row():
    fs, pairs, _ = case("run_edges_16000")
    clean = _full()
    y = pairs[1][1].copy()
    y[5000] = np.nan
    x = pairs[2][0].copy()
    x[17] = np.inf
    hit = run([pairs[0], (pairs[1][0], y), (x, pairs[2][1])], fs)
    for k in OUTPUTS:
        assert poison.same_bits(clean[k][0:1], hit[k][0:1]), k
    for b in (1, 2):
        assert all(math.isnan(float(hit[k][b])) for k in ("mel", "stft", "lsd")), b
        assert torch.isnan(hit["parts"][b, :, 0]).all()


def test_a_bad_mel_table_cannot_reach_outside_the_spectrum_or_the_weights():
    """filter ranges past F, before bin 0, negative counts and offsets outside the weights: the kernel cuts every filter's range
    into [0, F) and into [0, fb_w_len) (csrc/swc_spectral.hip, the MEL loop), so the call runs, the values that do not read the
    table keep their bits, and nothing is written outside the windows"""
    dev = torch.device("cuda", torch.cuda.current_device())
    fs, pairs, _ = case("lengths_513_16000")
    good = run(pairs, fs)
    from simwhisper_codec_amd import metrics
    t = dict(metrics.spectral_table(fs, dev))
    first, count, off = (t[k].cpu().clone() for k in ("first", "count", "off"))
    K, nw = first.numel(), t["w"].numel()
    first[0::4] += 5                               # the top filters of every scale now run past F
    count[1::4] = 100000
    first[2::4] = -7
    off[3::4] = nw - 1
    off[4::8] = -3
    count[5::8] = -2
    off[6::16] = 2 ** 31 - 1
    first[7::16] = 2 ** 31 - 1
    for k, v in (("first", first), ("count", count), ("off", off)):
        t[k] = v.to(dev)
    assert t["first"].numel() == K
    bad = run(pairs, fs, table=t)
    assert poison.same_bits(bad["stft"], good["stft"]) and poison.same_bits(bad["lsd"], good["lsd"])
    assert poison.same_bits(bad["parts"][:, :, 1:].contiguous(), good["parts"][:, :, 1:].contiguous())
    assert not poison.same_bits(bad["mel"], good["mel"])
    # weights that are all zero, offsets still wild: Mx = My = 0, the clamp on both sides
    t2 = dict(t, w=torch.zeros(4, device=dev))
    none = run(pairs, fs, table=t2, want=("mel", "parts"))
    assert torch.isfinite(none["mel"]).all()


def test_python_surface_matches_the_ops_level_call():
    from simwhisper_codec_amd import _lib, metrics, ops
    dev = torch.device("cuda", torch.cuda.current_device())
    fs, pairs, refs = case("lengths_513_16000")
    pairs = list(pairs) + [EMPTY]
    rows_x = [torch.from_numpy(x).to(dev) for x, _ in pairs]
    rows_y = [torch.from_numpy(y).to(dev) for _, y in pairs]
    raw = run(pairs, fs)
    q0 = {k: v.cpu() for k, v in ops.spectral(rows_x, rows_y, metrics.spectral_table(fs, dev)).items()}
    assert _same(q0, raw)
    # host tensors, the degraded side longer than the clean one: cut to the shorter length
    longer = [torch.cat([torch.from_numpy(y), torch.ones(17)]) for _, y in pairs[:3]] + [torch.zeros(0)]
    q1 = metrics.spectral([torch.from_numpy(x) for x, _ in pairs], longer, sample_rate=fs, device=dev)
    q2 = metrics.spectral(rows_x, rows_y, sample_rate=fs, device="cuda")
    for q in (q1, q2):
        assert q["scales"] == ref.default_scales() and set(q) == set(OUTPUTS) | {"scales"}
        for k in OUTPUTS:
            assert q[k].shape == ((4, 7, 4) if k == "parts" else (4,)) and q[k].device == dev and q[k].dtype == torch.float32
        assert _same({k: q[k].cpu() for k in OUTPUTS}, q0)
    compare("metrics.spectral", {k: q1[k].cpu() for k in OUTPUTS}, refs + [ref.spectral(*EMPTY, fs)])
    for fn, k in ((metrics.mel_distance, "mel"), (metrics.stft_distance, "stft"), (metrics.lsd, "lsd")):
        assert poison.same_bits(fn(rows_x, rows_y, sample_rate=fs, device=dev).cpu(), q0[k]), k
    only = metrics.spectral(rows_x, rows_y, sample_rate=fs, device=dev, want=("mel",))
    assert set(only) == {"mel", "parts", "scales"} and [s[2] for s in only["scales"]] == [ref.MEL] * 7
    assert poison.same_bits(only["parts"][:, :, 0].cpu().contiguous(), q0["parts"][:, :, 0].contiguous())
    assert not only["parts"][:3, :, 1:].any()
    # any rate works: it enters through the mel banks only
    q44 = metrics.spectral(rows_x, rows_y, sample_rate=44100, device=dev)
    assert poison.same_bits(q44["stft"].cpu(), q0["stft"]) and poison.same_bits(q44["lsd"].cpu(), q0["lsd"])
    assert not poison.same_bits(q44["mel"].cpu(), q0["mel"])
    with pytest.raises(_lib.SwcError, match="want"):
        metrics.spectral(rows_x, rows_y, sample_rate=fs, device=dev, want=("pesq",))
    empty = metrics.spectral([], [], sample_rate=fs, device=dev)
    assert all(empty[k].numel() == 0 for k in OUTPUTS) and empty["parts"].shape == (0, 7, 4)


def test_audiocodec_spectral_on_the_synthetic_checkpoint():
    import common
    from simwhisper_codec_amd import synth
    from simwhisper_codec_amd.codec import AudioCodec
    dev = torch.device("cuda", torch.cuda.current_device())
    model = AudioCodec(common.tiny_params(), precision="fp32")
    model.load_state_dict(common.state_dict("tiny"), strict=True)
    model = model.to(dev).eval()
    wavs = [synth.synth_audio(18000, index=0, kind="speech").to(dev), synth.synth_audio(17000, index=1, kind="speech").to(dev)]
    q = model.spectral(wavs)
    assert set(q) == set(OUTPUTS) | {"scales"}
    for k in OUTPUTS:
        assert q[k].shape == ((2, 7, 4) if k == "parts" else (2,)) and q[k].device == dev and q[k].dtype == torch.float32, k
        assert torch.isfinite(q[k]).all(), k
    print("AudioCodec.spectral:", {k: q[k].cpu().tolist() for k in ("mel", "stft", "lsd")})
    assert (q["mel"] > 0).all() and (q["stft"] > 0).all() and (q["lsd"] > 0).all()
    assert torch.allclose(q["parts"][:, :, 0].sum(dim=1), q["mel"], rtol=1e-6)


def test_evaluate_tool_on_four_small_wavs(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_spectral
    from evaluate_stoi import load_first_channel
    from simwhisper_codec_amd import wavio
    fs = 16000
    specs = [(9000, 10, 0), (11000, 0, 1), (8000, 20, 2), (8193, 5, 3)]
    os.makedirs(tmp_path / "orig"); os.makedirs(tmp_path / "syn")
    for i, (n, snr, seed) in enumerate(specs):
        x, y = ref.pair(n, fs, snr, seed)
        wavio.save_audio(str(tmp_path / "orig" / f"utt{i}.wav"), torch.from_numpy(x), fs)
        wavio.save_audio(str(tmp_path / "syn" / f"utt{i}.wav"), torch.from_numpy(y[: n - 3 * i]), fs)   # cut to the shorter
    rs = []
    for i in range(4):
        x = load_first_channel(str(tmp_path / "orig" / f"utt{i}.wav"), fs).numpy()
        y = load_first_channel(str(tmp_path / "syn" / f"utt{i}.wav"), fs).numpy()
        rs.append(ref.spectral(x[:len(y)], y, fs))
    assert evaluate_spectral.main(["--original_dir", str(tmp_path / "orig"), "--synthesized_dir", str(tmp_path / "syn"),
                                   "--batch_size", "3", "--verbose"]) == 0
    out = capsys.readouterr().out
    print(out)
    # four decimals are printed: a value within the bound of a rounding boundary may print either neighbour
    def shown(label, want, text):
        tol = RTOL * abs(want) + ATOL
        return any(f"{label} {v:.4f}" in text for v in (want - tol, want, want + tol))
    lines = out.splitlines()
    for i in range(4):
        line = next(ln for ln in lines if ln.startswith(f"utt{i}.wav:"))
        assert shown("mel", rs[i]["mel"], line) and shown("STFT", rs[i]["stft"], line) and shown("LSD", rs[i]["lsd"], line), line
    assert shown("mean mel distance:", float(np.mean([r["mel"] for r in rs])), out) and "over 4 pairs" in out
    assert shown("mean STFT distance:", float(np.mean([r["stft"] for r in rs])), out)
    assert shown("mean LSD:", float(np.mean([r["lsd"] for r in rs])), out)
