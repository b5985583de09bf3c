"""swc_noise, swc_mix and swc_convolve on the GPU (include/swc_degrade.h) and the layers above them, every call through the
C-ABI (ops.noise / ops.mix / ops.convolve).  Noise and the mixture are compared bit for bit with tests/degrade_ref.py.

The convolution is compared with the float64 definition.  Its tolerance is 4 x REF_ERROR x ||h||_1 x max|x| with REF_ERROR =
5.4e-7 (test_degrade_cpu.py): the largest error of the header's method restated in complex64 / float32 numpy against float64
over these same cases is 5.37e-7 of ||h||_1 max|x| (at n = 5000, a unit impulse at k = d = 1023), so the device is gated at
2.16e-6; its butterflies are fused multiply-adds in another order than numpy's.

All pointers, strides and lengths handed to the kernels are valid: nothing here provokes a fault."""
import functools

import numpy as np
import pytest
import torch

import degrade_ref as ref
import poison
from common import PARAMS, state_dict
from test_degrade_cpu import CONV_L, CONV_N, REF_ERROR, conv_cases, conv_signal, impulse, impulse_cases, shifted

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 4 * REF_ERROR
NOISE_N = (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025)
SEED = 0x123456789


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def same(got, want):
    """bit equality of an f32 device tensor and an f32 numpy array"""
    want = np.ascontiguousarray(want, dtype=np.float32)
    return tuple(got.shape) == want.shape and np.array_equal(bits(got), want.view(np.uint32))


def ops():
    from simwhisper_codec_amd import ops
    return ops


# ---- noise ----

def noise_batch(B):
    n = [NOISE_N[(3 * b + 1) % len(NOISE_N)] for b in range(B)]
    if B > 1:
        n[1] = 0
    ids = [7, 2 ** 32 + 5, 2 ** 63 + 11, 2 ** 64 - 1][:B] + list(range(100, 100 + max(0, B - 4)))
    return n, ids


@pytest.mark.parametrize("B", [1, 3, 33])
def test_noise_is_the_reference_bit_for_bit(B):
    n, ids = noise_batch(B)
    cols = max(n) + 3
    got = ops().noise(n, SEED, stream_ids=ids, cols=cols, device=DEV)
    assert same(got, ref.noise_batch(SEED, ids, n, cols))


def test_noise_every_length_and_the_issues_values():
    got = ops().noise(list(NOISE_N), SEED, stream_ids=[7] * len(NOISE_N), device=DEV)
    assert same(got, ref.noise_batch(SEED, [7] * len(NOISE_N), NOISE_N, max(NOISE_N)))
    assert (got[5, :4].cpu().numpy() * 2.0 ** 19).tolist() == [168346, -50660, 75042, -73636]


def test_noise_index_beyond_32_bits():
    for first in (2 ** 32 - 3, 2 ** 32 + 5, 2 ** 40 + 1):     # across the carry into the counter's second word, and beyond it
        got = ops().noise([9, 0, 300], 5, stream_ids=[1, 2, 2 ** 33], first=first, device=DEV)
        assert same(got, ref.noise_batch(5, [1, 2, 2 ** 33], [9, 0, 300], 300, first=first))
    whole = ops().noise([4096 + 600], 5, stream_ids=[3], device=DEV)
    piece = ops().noise([600], 5, stream_ids=[3], first=4096, device=DEV)
    assert torch.equal(whole[0, 4096:], piece[0])


def test_noise_row_alone_and_strided_views():
    n, ids = noise_batch(33)
    batch = ops().noise(n, SEED, stream_ids=ids, device=DEV)
    for b in (0, 2, 17, 32):
        alone = ops().noise([n[b]], SEED, stream_ids=[ids[b]], device=DEV)
        assert torch.equal(alone[0], batch[b, :n[b]])
    for fill in (7.0, float("nan")):
        view, check = poison.guarded((33, max(n)), torch.float32, ld=max(n) + 13, device=DEV)
        view.fill_(fill)
        out = ops().noise(n, SEED, stream_ids=ids, out=view)
        check()
        assert out is view and torch.equal(view, batch)      # every column was written, zeros behind a row


# ---- mix ----

def mix_rows(rng, n_list, m_list):
    x = [rng.uniform(-0.5, 0.5, n).astype(np.float32) for n in n_list]
    v = [ref.noise(3, 50 + i, m) for i, m in enumerate(m_list)]
    return x, v


def run_mix(x, v, lx, ln, snr, **kw):
    B = len(x)
    vals = torch.full((B, 8), float("nan"), dtype=torch.float64)
    vals[:, 0], vals[:, 1] = torch.tensor(lx, dtype=torch.float64), torch.tensor(ln, dtype=torch.float64)
    vals = vals.to(DEV)
    target = torch.tensor(snr if isinstance(snr, list) else [snr], dtype=torch.float64, device=DEV)
    return ops().mix([dev(r) for r in x], [dev(r) for r in v], vals[:, 0], vals[:, 1], target, **kw)    # strided columns


def check_mix(x, v, lx, ln, snr, out, gains, flags):
    g_dev, f_dev = gains.cpu().numpy(), flags.cpu().numpy()
    snr = snr if isinstance(snr, list) else [snr] * len(x)
    for b in range(len(x)):
        g_ref, mixed = ref.gain(lx[b], ln[b], snr[b], len(v[b]))
        if mixed:
            assert abs(int(g_dev[b:b + 1].view(np.int32)[0]) - int(np.array([g_ref]).view(np.int32)[0])) <= 1, (b, g_dev[b], g_ref)
        else:
            assert g_dev[b] == 0
        want, flag = ref.mix(x[b], v[b], g_dev[b], mixed)          # the device's own gain
        assert same(out[b, :len(x[b])], want), b
        assert not out[b, len(x[b]):].any()
        assert f_dev[b] == flag, (b, f_dev[b], flag)


def test_mix_is_one_fma_with_the_devices_gain():
    rng = np.random.default_rng(11)
    n_list, m_list = [], []
    for n in (2, 5, 257, 4097, 9001):
        for m in (1, n - 1, n, n + 1):
            n_list.append(n)
            m_list.append(m)
    n_list += [0, 1, 4096]
    m_list += [5, 1, 3]
    x, v = mix_rows(rng, n_list, m_list)
    B = len(x)
    lx = list(rng.uniform(-40, -10, B))
    ln = list(rng.uniform(-30, -5, B))
    snr = list(rng.uniform(-5, 40, B))
    out, gains, flags = run_mix(x, v, lx, ln, snr, cols=max(n_list) + 2)
    check_mix(x, v, lx, ln, snr, out, gains, flags)
    # a row alone is the row in the batch; one target serves every row
    alone = run_mix(x[6:7], v[6:7], lx[6:7], ln[6:7], snr[6:7])
    assert torch.equal(alone[0][0], out[6, :n_list[6]]) and torch.equal(alone[1], gains[6:7])
    out1, gains1, flags1 = run_mix(x[:4], v[:4], lx[:4], ln[:4], 12.5)
    check_mix(x[:4], v[:4], lx[:4], ln[:4], 12.5, out1, gains1, flags1)


def test_mix_unmixed_rows_and_full_scale():
    rng = np.random.default_rng(12)
    x, v = mix_rows(rng, [300, 300, 300, 300, 300, 5000], [300, 300, 300, 0, 300, 7])
    lx = [float("nan"), -20.0, -20.0, -20.0, -20.0, -20.0]
    ln = [-13.8, float("inf"), -13.8, -13.8, -13.8, -13.8]
    snr = [10.0, 10.0, float("-inf"), 10.0, -40.0, -40.0]
    out, gains, flags = run_mix(x, v, lx, ln, snr)
    check_mix(x, v, lx, ln, snr, out, gains, flags)
    assert flags.tolist()[:4] == [1, 1, 1, 1] and gains.tolist()[:4] == [0, 0, 0, 0]
    assert flags.tolist()[4:] == [2, 2]                       # driven past full scale: bit 1 (checked against the reference above)
    loud = [np.full(10, 1.5, dtype=np.float32)]
    _, _, f = run_mix(loud, [np.zeros(0, dtype=np.float32)], [-20.0], [-20.0], [10.0])
    assert f.tolist() == [3]                                  # an unmixed copy that is itself beyond full scale


@pytest.mark.parametrize("snr_db", [40.0, 20.0, 0.0, -5.0])
def test_mix_reaches_the_target_snr(snr_db):
    from simwhisper_codec_amd import synth
    x = [(0.05 * synth.synth_audio(16000 + 37 * i, index=80 + i, kind="speech")).numpy().astype(np.float32) for i in range(3)]
    v = [ref.noise(9, i, len(r)) for i, r in enumerate(x)]
    level = lambda r: 10.0 * np.log10(np.mean(r.astype(np.float64) ** 2))   # noqa: E731
    lx, ln = [level(r) for r in x], [level(r) for r in v]
    out, gains, flags = run_mix(x, v, lx, ln, snr_db)
    for b, r in enumerate(x):
        y = out[b, :len(r)].cpu().numpy().astype(np.float64)
        got = 10.0 * np.log10(np.sum(r.astype(np.float64) ** 2) / np.sum((y - r.astype(np.float64)) ** 2))
        print(f"snr target {snr_db} dB, row {b}: {got:.7f} dB")
        assert abs(got - snr_db) <= 1e-3


def test_mix_memory_contract():
    rng = np.random.default_rng(13)
    x, v = mix_rows(rng, [0, 5, 4097, 300], [3, 2, 4096, 301])
    lx, ln, snr = [-20.0] * 4, [-13.8] * 4, [5.0, 10.0, 15.0, 20.0]
    want = run_mix(x, v, lx, ln, snr, cols=4100)
    for fill in (7.0, float("nan")):
        view, check = poison.guarded((4, 4100), torch.float32, ld=4111, device=DEV)
        view.fill_(fill)
        with poison.poisoned_empty("nan" if fill != fill else "big"):
            got = run_mix(x, v, lx, ln, snr, out=view)
        check()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


# ---- convolve ----

@functools.lru_cache(maxsize=None)
def conv_x(n):
    return conv_signal("x", n, 1)


@functools.lru_cache(maxsize=None)
def conv_h(L):
    return conv_signal("h", L, 2)


def run_conv(xs, hs, h_index=None, d=0, extra=0, offset=0, **kw):
    """offset = 1: every row starts one element into its allocation (4-byte alignment only)"""
    def place(a):
        if not offset:
            return dev(a)
        raw = torch.full((len(a) + offset,), 3.0e4, dtype=torch.float32, device=DEV)
        raw[offset:] = dev(a)
        return raw[offset:]
    return ops().convolve([place(a) for a in xs], [place(a) for a in hs], h_index=h_index, d=d, extra=extra, **kw)


def check_conv(out, xs, hs, h_index, d, extra, tol=TOL):
    worst = 0.0
    for b, x in enumerate(xs):
        h = hs[h_index[b] if h_index is not None else 0]
        want = ref.convolve64(x, h, d, extra)
        got = out[b].cpu().numpy()
        assert not got[len(want):].any(), b                      # zeros behind a row's output
        if len(x):
            err = float(np.abs(got[:len(want)] - want).max() / (np.abs(h).sum() * np.abs(x).max()))
            worst = max(worst, err)
            assert err <= tol, (b, len(x), len(h), d, extra, err)
        else:
            assert not got.any()
    return worst


@pytest.mark.parametrize("L,d,extra", conv_cases())
def test_convolve_against_float64(L, d, extra):
    xs = [conv_x(n) for n in CONV_N]
    out = run_conv(xs, [conv_h(L)], d=d, extra=extra)
    assert out.shape == (len(CONV_N), max(CONV_N) + extra)
    print(f"L={L} d={d} extra={extra}: error {check_conv(out, xs, [conv_h(L)], None, d, extra):.3e} of ||h||_1 max|x| (gate {TOL:.3e})")


def test_convolve_rows_with_responses_of_different_partition_counts():
    xs = [conv_x(n) for n in CONV_N for _ in CONV_L]
    hs = [conv_h(L) for L in CONV_L]
    idx = [k for _ in CONV_N for k in range(len(CONV_L))]
    out = run_conv(xs, hs, h_index=idx, d=0, extra=0, offset=1)     # rows and responses at 4-byte alignment only
    print(f"mixed responses: error {check_conv(out, xs, hs, idx, 0, 0):.3e}")
    out_t = run_conv(xs, hs, h_index=idx, d=0, extra=2048)
    check_conv(out_t, xs, hs, idx, 0, 2048)
    # a row's output depends on its own response only: alone with that response it is the same bits
    for b in (len(CONV_L) * 6 + 1, len(CONV_L) * 4 + 5):
        alone = run_conv([xs[b]], [hs[idx[b]]])
        assert torch.equal(alone[0], out[b, :len(xs[b])])


@pytest.mark.parametrize("k,d", impulse_cases())
def test_convolve_unit_impulse_shifts_the_row(k, d):
    xs = [conv_x(n) for n in CONV_N]
    out = run_conv(xs, [impulse(k)], d=d)
    for b, x in enumerate(xs):
        if len(x):
            err = np.abs(out[b, :len(x)].cpu().numpy() - shifted(x, k, d)).max() / np.abs(x).max()
            assert err <= TOL, (len(x), k, d, err)
        assert not out[b, len(x):].any()


def test_convolve_row_alone_is_the_row_in_a_batch_of_33():
    rng = np.random.default_rng(21)
    lens = [int(v) for v in rng.integers(0, 6000, 33)]
    lens[5], lens[20] = 5000, 2049
    xs = [conv_signal("x", n, 40 + i) for i, n in enumerate(lens)]
    hs = [conv_h(2049), conv_h(1024)]
    idx = [b % 2 for b in range(33)]
    batch = run_conv(xs, hs, h_index=idx, d=1000, extra=1000)
    check_conv(batch, xs, hs, idx, 1000, 1000)
    for b in (5, 20, 32):
        alone = run_conv([xs[b]], [hs[idx[b]]], d=1000, extra=1000)
        assert torch.equal(alone[0], batch[b, :lens[b] + 1000]), b
    # another max_n and other neighbours change no bit either
    again = run_conv(xs[:7], hs, h_index=idx[:7], d=1000, extra=1000, max_n=20000)
    assert torch.equal(again, batch[:7, :again.shape[1]]) and not batch[:7, again.shape[1]:].any()


def test_convolve_memory_contract_and_workspace():
    o = ops()
    xs = [conv_x(n) for n in (0, 1025, 5000, 1)]
    hs = [conv_h(2049), conv_h(2)]
    idx = [0, 1, 0, 1]
    cols = 5000 + 700
    want = run_conv(xs, hs, h_index=idx, d=1, extra=700, cols=cols)
    need = o.convolve_workspace_bytes(4, 5000, 2, 2049)
    for fill, ws_fill in ((7.0, 0x00), (float("nan"), 0xFF)):
        view, check = poison.guarded((4, cols), torch.float32, ld=cols + 9, device=DEV)
        view.fill_(fill)
        ws, ws_check = poison.guarded((need,), torch.uint8, device=DEV)
        ws.fill_(ws_fill)                                    # 0xFF: every float of it a NaN
        got = run_conv(xs, hs, h_index=idx, d=1, extra=700, out=view, workspace=ws)
        check()
        ws_check()
        assert torch.equal(got, want)                        # nothing the workspace held before is read


# ---- the layers above ----

_MODELS = {}


def model():
    from simwhisper_codec_amd.codec import AudioCodec
    if "m" not in _MODELS:
        m = AudioCodec(PARAMS["tiny"](), precision="mixed")
        m.load_state_dict(state_dict("tiny"), strict=True)
        _MODELS["m"] = m.to(DEV).eval()
    return _MODELS["m"]


def _speech(n, index):
    from simwhisper_codec_amd import synth
    return synth.synth_audio(n, index=index, kind="speech")


def test_add_noise_is_activity_then_mix():
    from simwhisper_codec_amd import degrade
    o = ops()
    wavs = [(0.1 * _speech(16000 + 91 * i, 90 + i)).to(DEV) for i in range(3)]
    n = [w.numel() for w in wavs]
    for level, col in (("active", 0), ("long_term", 1)):
        rows, gains, flags = degrade.add_noise(wavs, 10.0, seed=77, level=level)
        noise = o.noise(n, 77, device=DEV)
        nrows = [noise[b, :k] for b, k in enumerate(n)]
        vals = o.activity(wavs + nrows, 16000)["values"]
        out, g, f = o.mix(wavs, nrows, vals[:3, col], vals[3:, 1], torch.tensor([10.0], dtype=torch.float64, device=DEV))
        assert torch.equal(gains, g) and torch.equal(flags, f) and not flags.any()
        for b in range(3):
            assert torch.equal(rows[b], out[b, :n[b]])
    # caller rows (shorter: they wrap) and one target per row
    babble = [(0.3 * _speech(5000, 95 + i)).to(DEV) for i in range(3)]
    rows, gains, flags = degrade.add_noise(wavs, [20.0, 10.0, 0.0], noise=babble)
    assert [r.numel() for r in rows] == n and (gains[1:] > gains[:-1]).all()
    same_seed = degrade.add_noise(wavs, 10.0, seed=77)[0]
    other_seed = degrade.add_noise(wavs, 10.0, seed=78)[0]
    again = degrade.add_noise(wavs, 10.0, seed=77)[0]
    assert all(torch.equal(a, b) for a, b in zip(same_seed, again)) and not torch.equal(same_seed[0], other_seed[0])


def test_reverberate_and_synthetic_rir():
    from simwhisper_codec_amd import degrade
    wavs = [(0.1 * _speech(8000 + 50 * i, 97 + i)).to(DEV) for i in range(2)]
    h, d = degrade.synthetic_rir(0.2, 16000, seed=3, predelay_ms=2.0)
    assert d == 32 and h.numel() == 32 + degrade.rir_length(0.2, 16000) and h[d] == 1 and not h[:d].any()
    h2, _ = degrade.synthetic_rir(0.2, 16000, seed=3, drr_db=6.0, predelay_ms=2.0)
    tail = h2.cpu().numpy().astype(np.float64)
    tail[d] = 0
    assert abs(10 * np.log10(1.0 / np.sum(tail ** 2)) - 6.0) < 1e-3
    rows = degrade.reverberate(wavs, rir=h2, d=d)
    assert [r.numel() for r in rows] == [w.numel() for w in wavs]
    for r, w in zip(rows, wavs):
        want = ref.convolve64(w.cpu().numpy(), h2.cpu().numpy(), d, 0)
        assert np.abs(r.cpu().numpy() - want).max() <= TOL * float(h2.abs().sum()) * float(w.abs().max())
    long = degrade.reverberate(wavs, rir=h2, d=d, tail=True)
    assert [r.numel() for r in long] == [w.numel() + h2.numel() - 1 - d for w in wavs]
    a, b = degrade.apply(wavs, [{}, {"rt60": 0.2, "snr_db": 15.0, "seed": 3}])
    assert all(x is y or torch.equal(x, y) for x, y in zip(a, wavs)) and [r.numel() for r in b] == [w.numel() for w in wavs]


def test_robustness():
    from simwhisper_codec_amd import degrade, units
    m = model()
    wavs = [(0.1 * _speech(16000 * 2 + 211, 70)).to(DEV), (0.1 * _speech(16000 + 9000, 71)).to(DEV)]
    conds = [{}, {"snr_db": 10.0, "seed": 5}, {"snr_db": 10.0, "seed": 5}]
    res = m.robustness(wavs, conds)
    G = m.num_groups
    assert res["ued"].shape == res["code_match"].shape == (3, G) and res["frame_match"].shape == (3,)
    assert (res["ued"][0] == 0).all() and (res["code_match"][0] == 1).all() and res["frame_match"][0] == 1
    clean = m.encode(wavs)["codes_list"]
    noisy = m.encode(degrade.add_noise(wavs, 10.0, seed=5)[0])["codes_list"]
    hand = units.agreement(clean, noisy, levels=m.fsq_levels, dedup=True, device=torch.device(DEV))
    assert np.array_equal(res["ued"][1], np.nanmean(hand["ued"], axis=0))
    assert np.array_equal(res["code_match"][1], np.nanmean(hand["code_match"], axis=0))
    assert res["frame_match"][1] == float(np.nanmean(hand["frame_match"]))
    for k, v in hand["counts"].items():
        assert np.array_equal(res["counts"][1][k], v), k
        assert np.array_equal(res["counts"][2][k], v), k         # the same seed: the same codes twice
    assert (res["ued"][1] > 0).any()                             # 10 dB of noise moves the synthetic model's tokens


def _write_wav(path, pcm, sr=16000):
    import struct
    raw = pcm.numpy().astype("<i2").tobytes()
    open(path, "wb").write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
                           struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16) + b"data" + struct.pack("<I", len(raw)) + raw)


def test_cli_noise_does_not_depend_on_the_batch(tmp_path, monkeypatch):
    import yaml
    import inference
    cfg = tmp_path / "tiny.yaml"
    cfg.write_text(yaml.safe_dump({"generator_params": PARAMS["tiny"]()}))
    ind = tmp_path / "in"
    ind.mkdir()
    names = ["a", "b"]
    for i, (name, n) in enumerate(zip(names, [16000 * 2 + 123, 16000 * 2 + 123])):
        _write_wav(str(ind / f"{name}.wav"), (0.2 * _speech(n, 60 + i).clamp(-1, 1) * 32767).round().to(torch.int16))
    common = ["--config_path", str(cfg), "--synthetic_checkpoint", "--device", "cuda", "--precision", "mixed", "--mode", "encode",
              "--input_dir", str(ind)]
    runs = {"plain": ["--batch_size", "2"], "together": ["--batch_size", "2", "--add_noise_snr", "10"],
            "apart": ["--batch_size", "1", "--add_noise_snr", "10"], "seed": ["--batch_size", "2", "--add_noise_snr", "10", "--noise_seed", "1"]}
    data = {}
    for tag, extra in runs.items():
        inference.main(common + extra + ["--output_dir", str(tmp_path / tag)])
        data[tag] = [(tmp_path / tag / f"{n}.swc").read_bytes() for n in names]
    assert data["together"] == data["apart"]
    assert data["together"] != data["plain"] and data["seed"] != data["together"]
    # without the flags the degradations are not reached at all, and the files are those of the run above
    from simwhisper_codec_amd import degrade

    def never(*a, **k):
        raise AssertionError("degrade.apply was called without a flag")
    monkeypatch.setattr(degrade, "apply", never)
    inference.main(common + ["--batch_size", "1", "--output_dir", str(tmp_path / "plain1")])
    assert [(tmp_path / "plain1" / f"{n}.swc").read_bytes() for n in names] == data["plain"]
