"""swc_stretch on the GPU (include/swc_stretch.h) and the layers above it, every call through the C-ABI (ops.stretch).
Positions, distances and samples are compared bit for bit with tests/stretch_ref.py over the cases of test_stretch_cpu.py.

The end-to-end check goes through the existing metrics.f0: a harmonic complex at 125 Hz keeps its F0 under a stretch and moves
it by p / q under a shift.  Its gate is twice the error of the same chain on the CPU (stretch_ref, wavio.resample, pitch_ref),
or 0.5 %, whichever is larger.

All pointers, strides and lengths handed to the kernels are valid: nothing here provokes a fault.
On the commit before this one every test of this file fails: the header, the symbols and the functions do not exist there."""
import functools

import numpy as np
import pytest
import torch

import pitch_ref
import poison
import stretch_ref as ref
from common import PARAMS, state_dict
from test_stretch_cpu import CASES, row

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a, offset=0):
    """offset = 1: the row starts one element into its allocation (4-byte alignment only)"""
    t = torch.from_numpy(np.array(a))      # a copy: the shared references stay read-only
    if not offset:
        return t.to(DEV)
    raw = torch.full((len(a) + offset,), 3.0e4, dtype=torch.float32, device=DEV)
    raw[offset:] = t.to(DEV)
    return raw[offset:]


def ops():
    from simwhisper_codec_amd import ops
    return ops


def same(got, want):
    """bit equality of a device tensor and a numpy array of the same kind"""
    got = got.detach().cpu().contiguous().numpy()
    want = np.ascontiguousarray(want, dtype=got.dtype)
    return got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


@functools.lru_cache(maxsize=None)
def reference(kind, n, seed, W, D, num, den):
    """computed once, shared and left unchanged -> (x, pos, dist, out, flag, ties)"""
    x = row(kind, n, seed)
    pos, dist, defined, ties = ref.track(x, W, D, num, den, count_ties=True)
    out = ref.synthesise(x, pos, defined, W, num, den)
    for a in (x, pos, dist, out):
        a.setflags(write=False)
    return x, pos, dist, out, 0 if defined else ref.UNDEFINED, ties


def check_call(res, refs, W, num, den, max_n, cols=None):
    """every output of a call against the references of its rows"""
    Jmax = ref.frames(max_n, W, num, den)
    for b, (x, pos, dist, out, flag, _) in enumerate(refs):
        J = len(pos)
        if "pos" in res:
            assert res["pos"].shape[1] >= Jmax and same(res["pos"][b, :J], pos), (b, len(x))
            assert not res["pos"][b, J:Jmax].any()
        if "dist" in res:
            assert same(res["dist"][b, :J], dist) and not res["dist"][b, J:Jmax].any(), (b, len(x))
        if "flags" in res:
            assert int(res["flags"][b]) == flag
        if "out" in res:
            c = res["out"].shape[1] if cols is None else cols
            k = min(len(out), c)
            assert same(res["out"][b, :k], out[:k]), (b, len(x))
            assert not res["out"][b, k:c].any()


@pytest.mark.parametrize("case", range(len(CASES)))
def test_positions_distances_and_samples_bit_for_bit(case):
    W, D, num, den, rows = CASES[case]
    refs = [reference(kind, n, seed, W, D, num, den) for kind, n, seed in rows]
    res = ops().stretch([dev(r[0]) for r in refs], num, den, W=W, D=D, want=("out", "pos", "dist", "flags"))
    max_n = max(len(r[0]) for r in refs)
    assert res["out"].shape == (len(rows), ref.out_len(max_n, num, den)) and res["pos"].shape == (len(rows), ref.frames(max_n, W, num, den))
    check_call(res, refs, W, num, den, max_n)
    frames = sum(len(r[1]) for r in refs)
    ties = sum(r[5] for r in refs)
    print(f"W={W} D={D} {num}/{den} B={len(rows)}: {frames} frames, {ties} with a tie")
    squares = [r for (kind, n, _), r in zip(rows, refs) if kind == "square" and n == 5000 and 2 * D >= 74]
    for r in squares:             # its period of 74 lies inside the search range: d and d + 74 reach the same Dm
        assert r[5] >= 1          # the reference sees ties there: the tie rule decided, and the device agrees bit for bit
    zeros = [r for (kind, n, _), r in zip(rows, refs) if kind == "zeros" and n > W]
    for r in zeros:
        assert np.array_equal(r[1], (np.arange(len(r[1])) * (W // 2) * num) // den)     # every d is 0


def test_the_square_wave_case_has_ties():
    hit = [c for c in CASES if 2 * c[1] >= 74 and any(kind == "square" and n == 5000 for kind, n, _ in c[4])]
    assert len(hit) >= 2 and all(reference("square", 5000, seed, *c[:4])[5] >= 1 for c in hit for kind, n, seed in c[4] if kind == "square")


def _batch33():
    W, D, num, den, rows = CASES[3]
    assert (W, D, len(rows)) == (512, 128, 33)
    return W, D, num, den, rows, [reference(kind, n, seed, W, D, num, den) for kind, n, seed in rows]


def test_a_row_alone_is_the_row_in_a_batch_of_33():
    W, D, num, den, rows, refs = _batch33()
    xs = [dev(r[0]) for r in refs]
    want = ("out", "pos", "dist", "flags")
    batch = ops().stretch(xs, num, den, W=W, D=D, want=want)
    picked = [b for b, (kind, n, _) in enumerate(rows) if n in (5000, 3 * W + 5, W + 1)][:5]
    assert len(picked) == 5
    for b in picked:
        alone = ops().stretch([xs[b]], num, den, W=W, D=D, want=want)
        n_out, J = len(refs[b][3]), len(refs[b][1])
        assert torch.equal(alone["out"][0], batch["out"][b, :n_out]) and torch.equal(alone["pos"][0], batch["pos"][b, :J])
        assert torch.equal(alone["dist"][0], batch["dist"][b, :J]) and int(alone["flags"][0]) == int(batch["flags"][b])
    # another max_n, another ld and cols, rows at 4-byte alignment only, and only some of the outputs: the same bits
    sub = [0, 1, 2, 3, 4, 5, 6]
    cols = 7000
    view, check = poison.guarded((len(sub), cols), torch.float32, ld=cols + 13, device=DEV)
    again = ops().stretch([dev(refs[b][0], offset=1) for b in sub], num, den, W=W, D=D, want=("out", "pos"), max_n=20000, out={"out": view})
    check()
    check_call(again, [refs[b] for b in sub], W, num, den, 20000)
    assert again["out"] is view and again["pos"].shape[1] == ref.frames(20000, W, num, den)
    # a cols that cuts the longest rows, and the track alone
    cut = ops().stretch([xs[b] for b in sub], num, den, W=W, D=D, want=("out",), cols=1000)
    check_call(cut, [refs[b] for b in sub], W, num, den, 5000, cols=1000)
    assert cut["out"].shape == (len(sub), 1000)
    track = ops().stretch([xs[b] for b in sub], num, den, W=W, D=D, want=("pos", "dist"))
    check_call(track, [refs[b] for b in sub], W, num, den, max(len(refs[b][0]) for b in sub))


def test_a_row_with_a_nan_is_flagged_and_leaves_its_neighbours_alone():
    W, D, num, den = 64, 7, 4, 5
    good = [reference("noise", 700, 3, W, D, num, den), reference("period", 900, 4, W, D, num, den)]
    for bad_value in (float("nan"), float("inf")):
        bad = row("noise", 800, 5)
        bad[123] = bad_value
        res = ops().stretch([dev(good[0][0]), dev(bad), dev(good[1][0])], num, den, W=W, D=D, want=("out", "pos", "dist", "flags"))
        assert res["flags"].tolist() == [0, ref.UNDEFINED, 0]
        assert not res["out"][1].any() and not res["pos"][1].any() and not res["dist"][1].any()
        check_call({k: v[[0, 2]] for k, v in res.items()}, good, W, num, den, 900)


def test_memory_contract_and_workspace():
    o = ops()
    W, D, num, den = 64, 128, 4, 5
    rows = [("noise", 0, 0), ("noise", 1500, 1), ("square", 5000, 2), ("quiet", 33, 3), ("noise", 4097, 4)]
    refs = [reference(kind, n, seed, W, D, num, den) for kind, n, seed in rows]
    bad = row("noise", 300, 9)
    bad[7] = np.nan
    xs = [dev(r[0]) for r in refs] + [dev(bad)]
    B, max_n = len(xs), 5000
    cols, Jmax = ref.out_len(max_n, num, den) + 5, ref.frames(max_n, W, num, den)
    want = o.stretch(xs, num, den, W=W, D=D, want=("out", "pos", "dist", "flags"), cols=cols)
    check_call({k: v[:5] for k, v in want.items()}, refs, W, num, den, max_n)
    need = o.stretch_workspace_bytes(B, max_n, W, num, den)
    assert need == ref.workspace_bytes(B, max_n, W, num, den)
    for fill, ws_fill in (("big", 0x00), ("nan", 0xFF)):
        out, c_out = poison.guarded((B, cols), torch.float32, ld=cols + 9, device=DEV)
        pos, c_pos = poison.guarded((B, Jmax), torch.int32, ld=Jmax + 5, device=DEV)
        dist, c_dist = poison.guarded((B, Jmax), torch.int64, ld=Jmax + 5, device=DEV)
        flags, c_flags = poison.guarded((B,), torch.int32, device=DEV)
        ws, c_ws = poison.guarded((need,), torch.uint8, device=DEV)
        for t in (out, pos, dist, flags):
            poison.fill_(t, fill)
        ws.fill_(ws_fill)                                    # what the workspace held before changes nothing
        with poison.poisoned_empty(fill):
            got = o.stretch(xs, num, den, W=W, D=D, want=("out", "pos", "dist", "flags"), out={"out": out, "pos": pos, "dist": dist, "flags": flags},
                            workspace=ws)
        for c in (c_out, c_pos, c_dist, c_flags, c_ws):
            c()
        for k in ("out", "pos", "dist", "flags"):
            assert torch.equal(got[k], want[k]), k          # every promised entry was written, nothing else
        # out may be absent: the track alone writes the same positions
        pos2, c_pos2 = poison.guarded((B, Jmax), torch.int32, ld=Jmax + 5, device=DEV)
        poison.fill_(pos2, fill)
        ws.fill_(ws_fill)
        got = o.stretch(xs, num, den, W=W, D=D, want=("pos",), out={"pos": pos2}, workspace=ws)
        c_pos2()
        c_ws()
        assert torch.equal(got["pos"], want["pos"])


# ---- the Python layer ----

def _speech(n, index):
    from simwhisper_codec_amd import synth
    return synth.synth_audio(n, index=index, kind="speech")


def test_time_stretch_is_ops_stretch():
    from simwhisper_codec_amd import degrade
    o = ops()
    wavs = [(0.1 * _speech(8000 + 91 * i, 90 + i)).to(DEV) for i in range(4)]
    n = [w.numel() for w in wavs]
    rows, pos = degrade.time_stretch(wavs, 0.8, tracks=True)
    hand = o.stretch(wavs, 4, 5, W=512, D=128, want=("out", "pos"))
    for b in range(4):
        n_out = o.stretch_out_len(n[b], 4, 5)
        assert rows[b].numel() == n_out == -(-n[b] * 5 // 4) and torch.equal(rows[b], hand["out"][b, :n_out])
        assert torch.equal(pos[b], hand["pos"][b, :-(-n_out // 256)])
    # a window of 20 ms and a search of 5 ms: W = 320, D = 80
    rows = degrade.time_stretch(wavs[:2], 1.25, window_ms=20.0, search_ms=5.0)
    hand = o.stretch(wavs[:2], 5, 4, W=320, D=80, want=("out",))
    assert all(torch.equal(rows[b], hand["out"][b, :-(-n[b] * 4 // 5)]) for b in range(2))
    # one speed per row: the grouped calls
    speeds = [0.8, 1.25, 0.8, 1.0]
    rows = degrade.time_stretch(wavs, speeds)
    slow = degrade.time_stretch([wavs[0], wavs[2]], 0.8)
    fast = degrade.time_stretch([wavs[1]], 1.25)
    same_speed = degrade.time_stretch([wavs[3]], 1.0)
    assert torch.equal(rows[0], slow[0]) and torch.equal(rows[2], slow[1]) and torch.equal(rows[1], fast[0]) and torch.equal(rows[3], same_speed[0])
    assert rows[3].numel() == n[3] and float((rows[3] - wavs[3]).abs().max()) <= 2.0 ** -23 * float(wavs[3].abs().max())
    # apply(): a speed of 1 runs nothing, the new keys come first
    a, b = degrade.apply(wavs[:2], [{"speed": 1.0}, {"speed": 0.8, "snr_db": 20.0, "seed": 3}])
    assert all(x is y or torch.equal(x, y) for x, y in zip(a, wavs)) and [r.numel() for r in b] == [-(-k * 5 // 4) for k in n[:2]]
    noisy = degrade.add_noise(degrade.time_stretch(wavs[:2], 0.8), 20.0, seed=3)[0]
    assert all(torch.equal(x, y) for x, y in zip(b, noisy))


def test_pitch_shift_is_stretch_then_resample_then_cut():
    from simwhisper_codec_amd import degrade
    o = ops()
    wavs = [(0.1 * _speech(8000 + 91 * i, 94 + i)).to(DEV) for i in range(3)]
    n = [w.numel() for w in wavs]
    for kw, (p, q) in (({"semitones": 2}, (55, 49)), ({"ratio": 1.125}, (9, 8)), ({"semitones": -2}, (49, 55)), ({"ratio": 8 / 9}, (8, 9))):
        rows, info = degrade.pitch_shift(wavs, **kw)
        assert (info["p"], info["q"]) == (p, q) and info["ratio"] == p / q and abs(info["cents_error"]) < 4.0
        st = o.stretch(wavs, q, p, W=512, D=128, want=("out",))["out"]
        slow = [st[b, :-(-n[b] * p // q)] for b in range(3)]
        rs, n_rs = o.resample(slow, p, q, cols=max(n))
        for b in range(3):
            assert rows[b].numel() == n[b] and torch.equal(rows[b], rs[b, :n[b]])
            assert n_rs[b] >= n[b] or not rows[b][n_rs[b]:].any()
    rows, info = degrade.pitch_shift(wavs, semitones=0)
    assert info["ratio"] == 1 and info["cents_error"] == 0 and [r.numel() for r in rows] == n
    assert abs(degrade.pitch_shift(wavs, semitones=2)[1]["cents_error"] - 1200 * np.log2((55 / 49) / 2 ** (2 / 12))) < 1e-9


# ---- end to end, through metrics.f0 ----

F0, FS = 125.0, 16000


def _median_f0_ref(x):
    _, f0 = pitch_ref.track(x, **pitch_ref.params(FS))
    f0 = f0[f0 > 0]
    return float(np.median(f0))


@functools.lru_cache(maxsize=None)
def _chain_on_the_cpu(kind, a, b):
    """the same chain on the CPU -> (relative F0 error against the expected value, length)"""
    from simwhisper_codec_amd import wavio
    x = pitch_ref.harmonic_complex(F0, 2 * FS, FS)
    if kind == "stretch":      # speed a / b
        y = ref.stretch(x, 512, 128, a, b)["out"]
        want = F0
    else:                      # ratio p / q = a / b
        slow = ref.stretch(x, 512, 128, b, a)["out"]
        y = wavio.resample(torch.from_numpy(slow), a, b).numpy()[:len(x)]
        y = np.concatenate([y, np.zeros(len(x) - len(y), np.float32)])
        want = F0 * a / b
    return abs(_median_f0_ref(y) / want - 1.0), len(y)


@pytest.mark.parametrize("kind,value,frac", [("stretch", 0.8, (4, 5)), ("stretch", 1.25, (5, 4)), ("shift", 2, (55, 49)), ("shift", -2, (49, 55))])
def test_f0_of_a_harmonic_complex_end_to_end(kind, value, frac):
    from simwhisper_codec_amd import degrade, metrics
    x = pitch_ref.harmonic_complex(F0, 2 * FS, FS)       # 125 Hz at 16 kHz: an integer period of 128 samples
    cpu_err, cpu_len = _chain_on_the_cpu(kind, *frac)
    gate = max(2 * cpu_err, 0.005)
    wav = [torch.from_numpy(x).to(DEV)]
    if kind == "stretch":
        y = degrade.time_stretch(wav, value)[0]
        assert y.numel() == ops().stretch_out_len(len(x), *frac) == cpu_len
        want = F0
    else:
        rows, info = degrade.pitch_shift(wav, semitones=value)
        y = rows[0]
        assert y.numel() == len(x) == cpu_len and (info["p"], info["q"]) == frac
        want = F0 * frac[0] / frac[1]
    f0, voiced = metrics.f0([y], sample_rate=FS)[0]
    med = float(f0[voiced].median())
    err = abs(med / want - 1.0)
    print(f"{kind} {value}: median F0 {med:.3f} Hz, expected {want:.3f} Hz: error {err:.2e} (CPU chain {cpu_err:.2e}, gate {gate:.2e})")
    assert int(voiced.sum()) > 100 and err <= gate


# ---- AudioCodec.robustness and the CLI ----

_MODELS = {}


def model():
    from simwhisper_codec_amd.codec import AudioCodec
    if "m" not in _MODELS:
        m = AudioCodec(PARAMS["tiny"](), precision="mixed")
        m.load_state_dict(state_dict("tiny"), strict=True)
        _MODELS["m"] = m.to(DEV).eval()
    return _MODELS["m"]


def test_robustness_under_speed_and_pitch():
    m = model()
    wavs = [(0.1 * _speech(16000 * 2 + 211, 70)).to(DEV), (0.1 * _speech(16000 + 9000, 71)).to(DEV)]
    conds = [{"speed": 1.0}, {"speed": 0.8}, {"semitones": 2}, {"speed": 0.8}]
    res = m.robustness(wavs, conds)
    G = m.num_groups
    assert res["ued"].shape == res["code_match"].shape == (4, G) and res["frame_match"].shape == (4,)
    assert (res["ued"][0] == 0).all() and (res["code_match"][0] == 1).all() and res["frame_match"][0] == 1
    assert np.isfinite(res["ued"][1]).all() and np.isnan(res["code_match"][1]).all() and np.isnan(res["frame_match"][1])
    assert np.isfinite(res["ued"][2]).all() and np.isfinite(res["code_match"][2]).all() and np.isfinite(res["frame_match"][2])
    assert np.array_equal(res["ued"][1], res["ued"][3])            # the same call twice: equal bits
    for k, v in res["counts"][1].items():
        assert np.array_equal(res["counts"][3][k], v), k
    again = m.robustness(wavs, conds[1:3])
    assert np.array_equal(again["ued"], res["ued"][1:3]) and np.array_equal(again["code_match"][1], res["code_match"][2])


def _write_wav(path, pcm, sr=16000):
    import struct
    raw = pcm.numpy().astype("<i2").tobytes()
    open(path, "wb").write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
                           struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16) + b"data" + struct.pack("<I", len(raw)) + raw)


def test_cli_stretch_does_not_depend_on_the_batch(tmp_path, monkeypatch):
    import yaml
    import inference
    cfg = tmp_path / "tiny.yaml"
    cfg.write_text(yaml.safe_dump({"generator_params": PARAMS["tiny"]()}))
    ind = tmp_path / "in"
    ind.mkdir()
    names = ["a", "b"]
    for i, (name, n) in enumerate(zip(names, [16000 * 2 + 123, 16000 + 4567])):
        _write_wav(str(ind / f"{name}.wav"), (0.2 * _speech(n, 60 + i).clamp(-1, 1) * 32767).round().to(torch.int16))
    common = ["--config_path", str(cfg), "--synthetic_checkpoint", "--device", "cuda", "--precision", "mixed", "--mode", "encode",
              "--input_dir", str(ind)]
    runs = {"plain": ["--batch_size", "2"], "together": ["--batch_size", "2", "--time_stretch", "0.9"],
            "apart": ["--batch_size", "1", "--time_stretch", "0.9"], "shift": ["--batch_size", "2", "--pitch_shift", "2"]}
    data = {}
    for tag, extra in runs.items():
        inference.main(common + extra + ["--output_dir", str(tmp_path / tag)])
        data[tag] = [(tmp_path / tag / f"{n}.swc").read_bytes() for n in names]
    assert data["together"] == data["apart"]
    assert data["together"] != data["plain"] and data["shift"] != data["plain"]
    assert all(len(s) > len(p) for s, p in zip(data["together"], data["plain"]))      # slower: more frames
    assert [len(s) for s in data["shift"]] == [len(p) for p in data["plain"]]            # a shift keeps the length
    # without the new flags ops.stretch is never reached, and the files are those of the run above
    from simwhisper_codec_amd import ops as o

    def never(*a, **k):
        raise AssertionError("ops.stretch was called without a flag")
    monkeypatch.setattr(o, "stretch", never)
    inference.main(common + ["--batch_size", "1", "--output_dir", str(tmp_path / "plain1")])
    assert [(tmp_path / "plain1" / f"{n}.swc").read_bytes() for n in names] == data["plain"]
