"""swc_stoi (include/swc_metrics.h) on the GPU against the float64 restatement of the contract (tests/stoi_ref.py).

Every value check: |d_gpu - d_f64| <= 1e-5, segs equal, and the kept-frame list the kernel left in its workspace equal to the
reference's, for inputs whose frame energies stay MARGIN_DB away from the removal threshold (asserted about each input: an
f32 energy may legitimately fall on the other side of a threshold it sits on).  The bound: the reference's tool reports three
decimals; a numpy float32 run of the restatement deviates from float64 by at most 2.4e-7 over 9 000 .. 48 000 samples and
30 / 5 / -5 dB SNR; 1e-5 leaves forty times that for another summation order and the MFMA's accumulation, and fails any path
whose operands slipped to 16 bits.  Each case prints the deviation it saw (pytest -s).

Shapes: the smallest that reach each branch.  SWC_STOI_TILE (16 STFT frames per workgroup of the spectrum kernel) and
SELECT_CHUNK (256 frames per round of the selection kernel's scan) are the two tile sizes; the cases cross both.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import poison  # noqa: E402
import stoi_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-5
SELECT_CHUNK = 256          # frames per scan round of stoi_select_kernel (csrc/swc_stoi.hip)
POISON_ADDRESS = 0x10       # the "address" of a row with n_in = 0: never dereferenced


def _length_for_frames(M, fs):
    n = 1
    while stoi_ref.frames_at_10k(n, fs) < M:
        n += 1
    return n


def _pair(n, fs, snr, seed=0, gaps=()):
    x = stoi_ref.harmonic(n, fs, seed)
    if gaps:
        x = stoi_ref.with_gaps(x, fs, gaps)
    return x, stoi_ref.add_noise(x, snr, seed)


def _cases():
    from simwhisper_codec_amd import _lib
    n29, n30 = stoi_ref.boundary_lengths(16000)
    tile = _lib.STOI_TILE
    return {
        # name: (fs, [(x, y), ...])
        "9000_at_16k": (16000, [_pair(9000, 16000, 10), _pair(9000, 16000, 0, seed=1)]),     # M = 41: 12 segments
        "two_segments": (16000, [_pair(_length_for_frames(31, 16000), 16000, 5)]),           # M = 31
        "boundary": (16000, [_pair(n30, 16000, 10), _pair(n29, 16000, 10)]),                 # segs 1 and 0
        "gaps": (16000, [_pair(16000, 16000, 5, seed=2, gaps=[(0.0, 0.15), (0.5, 0.62)])]),
        "48000_at_16k": (16000, [_pair(48000, 16000, 0, seed=3)]),                           # M = 232
        "tile_edges": (10000, [_pair(_length_for_frames(2 * tile, 10000), 10000, 10),        # exactly two tiles
                               _pair(_length_for_frames(2 * tile + 1, 10000), 10000, 10)]),  # ... and one frame past them
        "select_chunk": (10000, [_pair(_length_for_frames(SELECT_CHUNK + 1, 10000), 10000, 20, seed=4,
                                       gaps=[(1.0, 1.1)])]),                                 # F = 258: a second scan round
        "10k": (10000, [_pair(6000, 10000, 10, seed=5)]),
        "8k_upsampled": (8000, [_pair(5000, 8000, 10, seed=6)]),
        "ragged": (16000, [_pair(9000, 16000, 20), _pair(12345, 16000, 5, seed=1), (np.zeros(0, np.float32),) * 2,
                           _pair(7001, 16000, -5, seed=2)]),
    }


_CACHE = {}


def case(name):
    """(fs, pairs, float64 results): built once, shared, never written to"""
    if name not in _CACHE:
        fs, pairs = _cases()[name]
        refs = [stoi_ref.stoi(x, y, fs) for x, y in pairs]
        for r in refs:
            assert r["margin"] >= stoi_ref.MARGIN_DB, (name, r["margin"])       # condition 1 on the inputs
        for x, _ in pairs:
            assert stoi_ref.band_range_db(x, fs) <= stoi_ref.BAND_RANGE_DB      # no empty band (stoi_ref.harmonic)
        for x, y in pairs:
            assert np.isfinite(x).all() and np.isfinite(y).all()                # condition 2
        _CACHE[name] = (fs, pairs, refs)
    return _CACHE[name]


def run(pairs, fs, pattern="nan", offsets=None, max_n=None):
    """one swc_stoi call on guarded, poisoned outputs and workspace -> (d, segs, kept lists) on the host.  offsets[b]: row b's
    samples start that many elements into their allocation (its address alignment)."""
    from simwhisper_codec_amd import _lib, metrics, ops
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    B = len(pairs)
    offsets = offsets or [0] * B
    table = metrics.stoi_table(fs, dev)
    keep, ptrs_x, ptrs_y, n_in = [], [], [], []
    for (x, y), off in zip(pairs, offsets):
        n = len(x)
        n_in.append(n)
        for v, ptrs in ((x, ptrs_x), (y, ptrs_y)):
            if n == 0:
                ptrs.append(POISON_ADDRESS)
                continue
            buf = torch.full((n + off,), float("nan"), device=dev)
            buf[off:] = torch.from_numpy(v)
            keep.append(buf)
            ptrs.append(buf.data_ptr() + 4 * off)
    max_n = max(n_in) if max_n is None else max_n
    L = ops.stoi_workspace_layout(B, max_n, table["orig"], table["new"])
    assert L["total"] == ops.stoi_workspace_bytes(B, max_n, table["orig"], table["new"]) and L["total"] % 256 == 0
    d, check_d = poison.guarded((B,), torch.float32, device=dev)
    segs, check_s = poison.guarded((B,), torch.int32, device=dev)
    ws, check_w = poison.guarded((L["total"] // 256, 256), torch.uint8, device=dev)
    assert ws.is_contiguous() and ws.data_ptr() % 256 == 0
    poison.fill_(d, pattern)
    poison.fill_(segs, pattern)
    poison.fill_(ws.view(torch.float32), pattern)
    meta = torch.tensor(ptrs_x + ptrs_y + n_in, dtype=torch.int64).to(dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.swc_stoi(P(meta[:B]), P(meta[B:2 * B]), P(meta[2 * B:]), max_n, table["orig"], table["new"], table["width"],
                      P(table["taps"]), P(table["start"]), table["run"], P(d), P(segs), P(ws), L["total"], B, ops._stream())
    _lib.check(rc, "swc_stoi")
    torch.cuda.synchronize()
    check_d(); check_s(); check_w()
    flat = ws.reshape(-1)
    K = flat[L["K"]:L["K"] + 4 * B].view(torch.int32).cpu()
    src = flat[L["src"]:L["src"] + 4 * B * L["Fmax"]].view(torch.int32).reshape(B, L["Fmax"]).cpu() if L["Fmax"] else None
    kept = [src[b, :int(K[b])].tolist() if src is not None else [] for b in range(B)]
    return d.cpu().clone(), segs.cpu().clone(), kept


def compare(name, d, segs, kept, refs):
    worst = 0.0
    for b, r in enumerate(refs):
        assert kept[b] == [int(v) for v in r["kept"]], f"{name} row {b}: kept frames differ"
        assert int(segs[b]) == r["segs"], (name, b, int(segs[b]), r["segs"])
        err = abs(float(d[b]) - r["d"])
        worst = max(worst, err)
        print(f"{name} row {b}: d_gpu {float(d[b]):.8f} d_f64 {r['d']:.8f} |diff| {err:.2e} segs {r['segs']} kept {len(kept[b])}")
        assert err <= TOL, (name, b, float(d[b]), r["d"])
        if r["segs"] == 0:
            assert float(d[b]) == float(np.float32(1e-5))
    print(f"{name}: worst |d_gpu - d_f64| = {worst:.2e}")


@pytest.mark.parametrize("name", ["9000_at_16k", "two_segments", "boundary", "gaps", "48000_at_16k", "tile_edges",
                                  "select_chunk", "10k", "8k_upsampled", "ragged"])
def test_values_against_float64(name):
    fs, pairs, refs = case(name)
    d, segs, kept = run(pairs, fs)
    compare(name, d, segs, kept, refs)


def test_the_cases_reach_the_branches_they_are_named_for():
    from simwhisper_codec_amd import _lib
    seg = lambda name: [r["segs"] for r in case(name)[2]]
    assert seg("boundary") == [1, 0] and seg("two_segments") == [2] and seg("9000_at_16k") == [12, 12]
    g = case("gaps")[2][0]["kept"]
    assert g[0] > 0 and (np.diff(g) > 1).any()                          # a kept frame follows removed ones, twice
    M = [len(r["kept"]) - 1 for r in case("tile_edges")[2]]
    assert M == [2 * _lib.STOI_TILE, 2 * _lib.STOI_TILE + 1]
    c = case("select_chunk")[2][0]
    assert stoi_ref.frames_at_10k(len(case("select_chunk")[1][0][0]), 10000) + 1 == SELECT_CHUNK + 2 and c["kept"][-1] > SELECT_CHUNK
    assert len(c["kept"]) < SELECT_CHUNK + 2                            # frames were removed in front of the second round
    assert len(case("48000_at_16k")[2][0]["kept"]) - 1 == 232
    assert [len(x) for x, _ in case("ragged")[1]] == [9000, 12345, 0, 7001] and seg("ragged")[2] == 0


def test_bits_do_not_depend_on_batch_position_or_alignment():
    fs, pairs, refs = case("9000_at_16k")
    alone, segs1, _ = run(pairs[:1], fs)
    other = case("ragged")[1]
    d3, segs3, _ = run([other[1], other[3], pairs[0]], fs, offsets=[0, 0, 1])        # row 2, 4 bytes off a 16-byte boundary
    assert poison.same_bits(alone[0:1], d3[2:3]) and int(segs1[0]) == int(segs3[2])
    # ... nor on the host's length bound (another workspace layout, other grids)
    wide, _, _ = run(pairs[:1], fs, max_n=20000)
    assert poison.same_bits(alone, wide)


def test_memory_contract_and_poison_independence():
    """d, segs and the workspace are poisoned before the call and guarded (run() checks the bands); the results must not
    depend on what the workspace held"""
    for name in ("ragged", "gaps", "10k"):
        fs, pairs, refs = case(name)
        a = run(pairs, fs, pattern="nan")
        b = run(pairs, fs, pattern="big")
        assert poison.same_bits(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
        assert torch.isfinite(a[0]).all()


def test_python_surface_matches_the_ops_level_call():
    from simwhisper_codec_amd import metrics, ops
    dev = torch.device("cuda", torch.cuda.current_device())
    fs, pairs, refs = case("ragged")
    rows_x = [torch.from_numpy(x).to(dev) for x, _ in pairs]
    rows_y = [torch.from_numpy(y).to(dev) for _, y in pairs]
    d0, s0 = ops.stoi(rows_x, rows_y, metrics.stoi_table(fs, dev))
    # host tensors, the degraded side longer than the clean one: cut to the shorter length
    longer = [torch.cat([torch.from_numpy(y), torch.ones(17)]) for _, y in pairs]
    d1, s1 = metrics.stoi([torch.from_numpy(x) for x, _ in pairs], longer, sample_rate=fs, device=dev)
    d2, s2 = metrics.stoi(rows_x, rows_y, sample_rate=fs, device="cuda")
    for d, s in ((d1, s1), (d2, s2)):
        assert d.shape == (4,) and d.dtype == torch.float32 and d.device == dev
        assert s.shape == (4,) and s.dtype == torch.int32 and s.device == dev
        assert poison.same_bits(d.cpu(), d0.cpu()) and torch.equal(s.cpu(), s0.cpu())
    compare("metrics.stoi", d1.cpu(), s1.cpu(), [[int(v) for v in r["kept"]] for r in refs], refs)


def test_every_supported_rate_runs():
    from simwhisper_codec_amd import metrics
    dev = torch.device("cuda", torch.cuda.current_device())
    for fs in (24000, 32000, 48000):
        n = _length_for_frames(31, fs)
        x, y = _pair(n, fs, 10, seed=7)
        r = stoi_ref.stoi(x, y, fs)
        assert r["margin"] >= stoi_ref.MARGIN_DB
        d, segs = metrics.stoi([torch.from_numpy(x)], [torch.from_numpy(y)], sample_rate=fs, device=dev)
        print(f"{fs} Hz: d_gpu {float(d[0]):.8f} d_f64 {r['d']:.8f} |diff| {abs(float(d[0]) - r['d']):.2e}")
        assert int(segs[0]) == r["segs"] == 2 and abs(float(d[0]) - r["d"]) <= TOL


def test_audiocodec_stoi_on_the_synthetic_checkpoint():
    import common
    from simwhisper_codec_amd import metrics, synth
    from simwhisper_codec_amd.codec import AudioCodec
    dev = torch.device("cuda", torch.cuda.current_device())
    model = AudioCodec(common.tiny_params(), precision="fp32")
    model.load_state_dict(common.state_dict("tiny"), strict=True)
    model = model.to(dev).eval()
    wavs = [synth.synth_audio(24000, index=0, kind="speech"), synth.synth_audio(17000, index=1, kind="speech")]
    d, segs = model.stoi([w.to(dev) for w in wavs])
    assert d.shape == (2,) and d.device == dev and d.dtype == torch.float32 and segs.dtype == torch.int32 and segs.device == dev
    assert ((d > 0) & (d <= 1)).all() and (segs >= 0).all()
    # the same as the three steps by hand
    codes = model.encode([w.to(dev) for w in wavs], device=dev)["codes_list"]
    syn = model.decode(codes, device=dev)["syn_wav_list"]
    d2, segs2 = metrics.stoi(wavs, syn, sample_rate=16000, device=dev)
    assert poison.same_bits(d.cpu(), d2.cpu()) and torch.equal(segs.cpu(), segs2.cpu())
    same, n_same = metrics.stoi(wavs[:1], wavs[:1], sample_rate=16000, device=dev)
    assert int(n_same[0]) > 0 and abs(float(same[0]) - 1.0) <= TOL          # a signal against itself


def test_evaluate_tool_on_four_small_wavs(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_stoi
    from simwhisper_codec_amd import wavio
    fs = 16000
    n29, _ = stoi_ref.boundary_lengths(fs)
    specs = [(9000, 10, 0), (11000, 0, 1), (n29, 10, 2), (8000, 5, 3)]            # the third is too short to score
    os.makedirs(tmp_path / "orig"); os.makedirs(tmp_path / "syn")
    for i, (n, snr, seed) in enumerate(specs):
        x, y = _pair(n, fs, snr, seed)
        wavio.save_audio(str(tmp_path / "orig" / f"utt{i}.wav"), torch.from_numpy(x), fs)
        wavio.save_audio(str(tmp_path / "syn" / f"utt{i}.wav"), torch.from_numpy(y[: n - 3 * i]), fs)   # cut to the shorter
    want = []
    for i in range(4):
        x = evaluate_stoi.load_first_channel(str(tmp_path / "orig" / f"utt{i}.wav"), fs).numpy()
        y = evaluate_stoi.load_first_channel(str(tmp_path / "syn" / f"utt{i}.wav"), fs).numpy()
        r = stoi_ref.stoi(x[:len(y)], y, fs)
        assert r["margin"] >= stoi_ref.MARGIN_DB
        want.append(r)
    assert [r["segs"] > 0 for r in want] == [True, True, False, True]
    mean = np.mean([r["d"] for r in want if r["segs"]])
    assert evaluate_stoi.main(["--original_dir", str(tmp_path / "orig"), "--synthesized_dir", str(tmp_path / "syn"),
                               "--batch_size", "3", "--verbose"]) == 0
    out = capsys.readouterr().out
    print(out)
    assert f"mean STOI: {mean:.3f} over 3 pairs" in out
    assert "left out of the mean (1): utt2.wav" in out and "utt2.wav: too short to score" in out
    for i in (0, 1, 3):
        assert f"utt{i}.wav: STOI {want[i]['d']:.3f} ({want[i]['segs']} segments)" in out
