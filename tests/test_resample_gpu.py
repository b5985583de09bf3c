"""swc_resample on the GPU (include/swc_audio.h) and the layers above it: values against the float64 reference of
tests/test_resample_cpu.py inside the DERIVED rounding bound (no measured tolerance), determinism, the memory contract in
the manner of tests/test_memory_contract_gpu.py, encode(sample_rate=), HostStager.to_device_pcm and the CLI flag.
All pointers and lengths handed to the kernel are valid: nothing here provokes a fault."""
import math

import pytest
import torch

import poison
from common import PARAMS, state_dict
from test_resample_cpu import PAIRS, _wav_bytes, bound, resample_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"

_MODELS = {}


def model(tag, precision):
    from simwhisper_codec_amd.codec import AudioCodec
    key = (tag, precision)
    if key not in _MODELS:
        m = AudioCodec(PARAMS[tag](), precision=precision)
        m.load_state_dict(state_dict(tag), strict=True)
        _MODELS[key] = m.to(DEV).eval()
    return _MODELS[key]


def _noise(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * 0.3).clamp(-1, 1)


def _pcm(n, ch, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32768, 32768, (n, ch), generator=g, dtype=torch.int32).to(torch.int16)


def _mono_of(pcm):
    """the header's definition in torch f32: the int32 sum is exact in f32, so this is one rounding"""
    ch = pcm.shape[1]
    return pcm.to(torch.int32).sum(dim=1).float() * torch.tensor(2.0 ** -15 / ch, dtype=torch.float32)


def _at_offset(t, off, fill=0):
    """a device copy of the contiguous CPU tensor t that starts `off` elements into a (16-byte aligned) allocation"""
    flat = t.reshape(-1)
    buf = torch.full((flat.numel() + off + 16,), fill, dtype=t.dtype, device=DEV)
    buf[off:off + flat.numel()] = flat.to(DEV)
    v = buf[off:off + flat.numel()]
    assert buf.data_ptr() % 16 == 0 and (not flat.numel() or v.data_ptr() == buf.data_ptr() + off * t.element_size())
    return v.view(t.shape) if t.dim() > 1 else v


def _lengths(orig_freq, new_freq):
    from simwhisper_codec_amd import wavio
    _, orig, _, width = wavio.resample_taps(orig_freq, new_freq)
    return [0, 1, width - 1, orig, int(1.3 * orig_freq) + 37, int(0.7 * orig_freq) - 11, 2 * orig + 3]


def _check_rows(out, n_out, monos, orig_freq, new_freq, what):
    out = out.cpu()
    worst = 0.0
    for b, x in enumerate(monos):
        y64, mag, nnz = resample_reference(x, orig_freq, new_freq)
        assert n_out[b] == math.ceil(new_freq * x.numel() / orig_freq) == y64.numel(), (what, b)
        y = out[b, : n_out[b]].double()
        err, lim = (y - y64).abs(), bound(mag, nnz)
        if err.numel():
            worst = max(worst, float((err / lim.clamp(min=1e-300)).max()) if (lim > 0).any() else 0.0)
        print(f"{what} row {b} n_in={x.numel()} n_out={n_out[b]} max err / bound = "
              f"{float((err / lim.clamp(min=1e-300)).max()) if err.numel() else 0.0:.3f}")
        assert (err <= lim).all(), (what, b, float(err.max()), int((err > lim).sum()))
        assert (out[b, n_out[b]:] == 0).all(), (what, b, "tail not zero")
    return worst


@pytest.mark.parametrize("orig_freq,new_freq", PAIRS)
def test_values_f32(orig_freq, new_freq):
    from simwhisper_codec_amd import ops
    lens = _lengths(orig_freq, new_freq)
    monos = [_noise(n, 100 + i) for i, n in enumerate(lens)]
    for odd in (False, True):
        rows = [_at_offset(x, (1 + i % 3) if odd else 0) for i, x in enumerate(monos)]
        out, n_out = ops.resample(rows, orig_freq, new_freq)
        assert out.shape == (len(rows), max(n_out)) and out.dtype == torch.float32
        _check_rows(out, n_out, monos, orig_freq, new_freq, f"f32 {orig_freq}->{new_freq} odd={odd}")


@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("orig_freq,new_freq", PAIRS)
def test_values_int16(orig_freq, new_freq, ch, tmp_path):
    from simwhisper_codec_amd import ops, wavio
    lens = _lengths(orig_freq, new_freq)
    pcms = [_pcm(n, ch, 200 + 7 * i + ch) for i, n in enumerate(lens)]
    monos = [_mono_of(p) for p in pcms]
    if ch <= 2:   # ... which is load_audio's arithmetic for the same file, exactly
        path = str(tmp_path / "x.wav")
        open(path, "wb").write(_wav_bytes(1, ch, orig_freq, 16, pcms[4].numpy().astype("<i2").tobytes()))
        assert torch.equal(wavio.load_audio(path, orig_freq).reshape(-1), monos[4])
    # offsets in int16 elements: 16-byte aligned; whole frames but not 16 bytes; one sample (frames straddle the vectors)
    for name, offs in (("aligned", [0] * len(pcms)), ("frame", [ch * (1 + i % 3) for i in range(len(pcms))]),
                       ("odd", [1 + 2 * (i % 3) for i in range(len(pcms))])):
        rows = [_at_offset(p, o) for p, o in zip(pcms, offs)]
        # the kernel's mono signal, bit for bit: the 1-tap identity filter hands it out unchanged
        ident, n_id = ops.resample(rows, orig_freq, orig_freq, channels=ch)
        for b, x in enumerate(monos):
            assert n_id[b] == x.numel() and torch.equal(ident[b, : n_id[b]].cpu(), x), (name, b)
        out, n_out = ops.resample(rows, orig_freq, new_freq, channels=ch)
        _check_rows(out, n_out, monos, orig_freq, new_freq, f"int16 ch={ch} {orig_freq}->{new_freq} {name}")
    flat, n_flat = ops.resample([r.reshape(-1) for r in rows], orig_freq, new_freq, channels=ch)   # flat interleaved rows
    assert n_flat == n_out and torch.equal(flat, out)


@pytest.mark.parametrize("orig_freq,new_freq", [(24000, 16000), (44100, 16000), (11025, 16000), (16000, 48000)])
def test_determinism(orig_freq, new_freq):
    """an output sample's bits depend on its row and the table only: not on B, the row's index, its address, cols or the run"""
    from simwhisper_codec_amd import ops
    n = int(1.1 * orig_freq) + 5
    x = _noise(n, 7)
    p = _pcm(n, 2, 8)
    others = [_noise(k, 9 + k) for k in (3000, 17, 0, 2 * orig_freq)]
    alone, (n_out,) = ops.resample([x.to(DEV)], orig_freq, new_freq)
    again, _ = ops.resample([x.to(DEV)], orig_freq, new_freq)
    assert torch.equal(alone, again)
    rows = [o.to(DEV) for o in others[:3]] + [_at_offset(x, 3)] + [others[3].to(DEV)]
    batch, n_b = ops.resample(rows, orig_freq, new_freq)
    assert n_b[3] == n_out and torch.equal(batch[3, :n_out], alone[0])
    wide, _ = ops.resample([_at_offset(x, 1)], orig_freq, new_freq, cols=n_out + 1029)
    assert torch.equal(wide[0, :n_out], alone[0]) and (wide[0, n_out:] == 0).all()
    cut, n_c = ops.resample([x.to(DEV)], orig_freq, new_freq, cols=n_out - 777)
    assert n_c == [n_out] and torch.equal(cut[0], alone[0, : n_out - 777])
    s_alone, (m_out,) = ops.resample([p.to(DEV)], orig_freq, new_freq, channels=2)
    s_batch, _ = ops.resample([_pcm(555, 2, 1).to(DEV), _at_offset(p, 1), _at_offset(p, 2)], orig_freq, new_freq, channels=2, cols=m_out + 3)
    assert torch.equal(s_batch[1, :m_out], s_alone[0]) and torch.equal(s_batch[2, :m_out], s_alone[0])


FILLS = ("zero", "nan", "big")


def _fill_f32(t, fill):
    return t.zero_() if fill == "zero" else poison.fill_(t, fill)


def _fill_i16(t, fill):
    return t.fill_({"zero": 0, "nan": poison.I16_POISON, "big": -32768}[fill])


@pytest.mark.parametrize("fmt", ["f32", "int16x2"])
@pytest.mark.parametrize("orig_freq,new_freq", [(24000, 16000), (44100, 16000), (16000, 24000)])
def test_memory_contract(orig_freq, new_freq, fmt):
    """output in a poison.guarded window with ld_out > cols; the three fills of the output's previous content, of what
    surrounds the input rows and (second variant, unguarded buffer) of the ld padding give bit-identical rows; [n_out, cols)
    is zero, [cols, ld_out) and the bands keep what they held; the inputs are bit-unchanged."""
    from simwhisper_codec_amd import ops
    ch = 1 if fmt == "f32" else 2
    lens = [int(0.4 * orig_freq) + 3, 0, 2500, 1]
    data = [_noise(n, 40 + i) if fmt == "f32" else _pcm(n, 2, 40 + i) for i, n in enumerate(lens)]
    n_want = [math.ceil(new_freq * n / orig_freq) for n in lens]
    cols = max(n_want) + 21
    ld = cols + 13
    res = []
    for fill in FILLS:
        # the rows live inside one buffer whose every other element is the fill: a read beyond a row's ends would change a result
        gap = 64
        total = sum(t.numel() for t in data) + gap * (len(data) + 1)
        back = torch.empty(total, dtype=data[0].dtype, device=DEV)
        (_fill_f32 if fmt == "f32" else _fill_i16)(back, fill)
        rows, pos = [], gap + 1                                   # (+ 1: the rows start at odd addresses)
        for t in data:
            k = t.numel()
            back[pos:pos + k] = t.reshape(-1).to(DEV)
            rows.append(back[pos:pos + k])
            pos += k + gap
        snap = back.clone()
        view, check = poison.guarded((len(data), cols), torch.float32, ld=ld, device=DEV)
        _fill_f32(view, fill)
        out, n_out = ops.resample(rows, orig_freq, new_freq, channels=ch, out=view)
        torch.cuda.synchronize()
        assert out is view and n_out == n_want
        check()                                                   # bands and [cols, ld_out) keep the sentinel
        assert poison.same_bits(back, snap), "a read-only input changed"
        for b in range(len(data)):
            assert (view[b, n_out[b]:] == 0).all() and torch.isfinite(view[b]).all()
        # second variant: one plain buffer, the ld padding and everything around the window hold the fill
        plain = torch.empty((len(data) + 2) * ld, dtype=torch.float32, device=DEV)
        _fill_f32(plain, fill)
        before = plain.clone()
        win = plain.as_strided((len(data), cols), (ld, 1), ld)
        ops.resample(rows, orig_freq, new_freq, channels=ch, out=win)
        torch.cuda.synchronize()
        assert poison.same_bits(win.contiguous(), view.contiguous())
        mask = torch.ones_like(plain, dtype=torch.bool)
        mask.as_strided((len(data), cols), (ld, 1), ld).fill_(False)
        assert poison.same_bits(plain[mask], before[mask]), "a store outside the window"
        res.append(view.contiguous().clone())
    for fill, r in zip(FILLS[1:], res[1:]):
        assert poison.same_bits(res[0], r), f"rows differ between the zero fill and the {fill} fill"


def _speech(n, index):
    from simwhisper_codec_amd import synth
    return synth.synth_audio(n, index=index, kind="speech")


@pytest.mark.parametrize("precision", ["fp32", "mixed"])
def test_encode_with_a_sample_rate(precision):
    from simwhisper_codec_amd import ops
    m = model("tiny", precision)
    sr = 24000
    lens = [int(1.5 * sr) + 7, 9000, 3 * sr, 100]
    wavs = [_speech(n, 30 + i).to(DEV) for i, n in enumerate(lens)]
    y, n_out = ops.resample(wavs, sr, 16000)
    want = m.encode([y[b, : n_out[b]] for b in range(len(wavs))])["codes_list"]
    got = m.encode(wavs, sample_rate=sr)["codes_list"]
    for n, a, b in zip(lens, got, want):
        assert a.shape[-1] == math.ceil(16000 * n / sr) // 1280 and torch.equal(a, b)
    # host tensors are moved and converted on the device: the same codes
    host = m.encode([w.cpu() for w in wavs], sample_rate=sr)["codes_list"]
    assert all(torch.equal(a, b) for a, b in zip(host, got))
    # the model's own rate, named or not, is today's path
    at16 = [_speech(n, 50 + i).to(DEV) for i, n in enumerate([16000, 7000])]
    for a, b in zip(m.encode(at16, sample_rate=16000)["codes_list"], m.encode(at16, sample_rate=None)["codes_list"]):
        assert torch.equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(m.encode(at16)["codes_list"], m.encode(at16, sample_rate=[16000, 16000])["codes_list"]))
    # no result depends on uninitialised memory
    for pattern in poison.PATTERNS:
        with poison.poisoned_empty(pattern) as spy:
            again = m.encode(wavs, sample_rate=sr)["codes_list"]
        assert spy.device_calls > 0 and all(torch.equal(a, b) for a, b in zip(again, got)), pattern


@pytest.mark.parametrize("precision", ["fp32", "mixed"])
def test_encode_mixed_rates_equal_the_single_calls(precision):
    m = model("tiny", precision)
    rates = [16000, 24000, 44100]
    wavs = [_speech(int(1.2 * sr) + 11 * i, 60 + i).to(DEV) for i, sr in enumerate(rates)]
    got = m.encode(wavs, sample_rate=rates)["codes_list"]
    for w, sr, a in zip(wavs, rates, got):
        one = m.encode([w], sample_rate=sr)["codes_list"][0]
        assert a.shape[-1] == math.ceil(16000 * w.numel() / sr) // 1280 and torch.equal(a, one), sr
    with pytest.raises(Exception):
        m.encode(wavs, sample_rate=[16000, 24000])


def test_encode_long_recording_at_another_rate():
    """70 s at 24 kHz: several 30 s windows; the whole row is resampled first, then windowed as usual"""
    from simwhisper_codec_amd import ops
    m = model("tiny", "mixed")
    sr = 24000
    w = _speech(70 * sr + 123, 77).to(DEV)
    y, (n_out,) = ops.resample([w], sr, 16000)
    want = m.encode([y[0, :n_out]])["codes_list"][0]
    got = m.encode([w], sample_rate=sr)["codes_list"][0]
    assert got.shape[-1] == math.ceil(16000 * w.numel() / sr) // 1280 > 2 * 250 and torch.equal(got, want)


def _items():
    return [(_pcm(16000 + 333, 1, 1), 16000), (_pcm(int(1.4 * 24000) + 5, 1, 2), 24000), (_pcm(int(1.1 * 44100) + 2, 2, 3), 44100)]


def test_stager_to_device_pcm():
    from simwhisper_codec_amd import ops
    from simwhisper_codec_amd.pipeline import HostStager
    st = HostStager()
    items = _items()
    got = st.to_device_pcm(items, torch.device(DEV), 16000)
    torch.cuda.synchronize()
    assert [g.dtype for g in got] == [torch.float32] * 3 and all(g.is_cuda and g.dim() == 1 for g in got)
    for g, (pcm, sr) in zip(got, items):
        y, (n_out,) = ops.resample([pcm.to(DEV)], sr, 16000, channels=pcm.shape[1])
        assert g.numel() == n_out == math.ceil(16000 * pcm.shape[0] / sr) and torch.equal(g, y[0, :n_out])
    as16 = st.to_device_pcm16([items[0][0][:, 0].contiguous()], torch.device(DEV))[0]
    assert torch.equal(got[0], as16) and torch.equal(got[0].cpu(), items[0][0][:, 0].float() * 2.0 ** -15)
    # flat mono tensors (wavio.read_pcm16's form) are accepted too
    flat = st.to_device_pcm([(items[1][0][:, 0].contiguous(), 24000)], torch.device(DEV), 16000)[0]
    assert torch.equal(flat, got[1])


def test_cli_resample_gpu(tmp_path):
    import yaml
    import inference
    from simwhisper_codec_amd import ops, wavio
    from simwhisper_codec_amd.pipeline import HostStager
    cfg = tmp_path / "tiny.yaml"
    cfg.write_text(yaml.safe_dump({"generator_params": PARAMS["tiny"]()}))
    ind, outd = tmp_path / "in", tmp_path / "out"
    ind.mkdir()
    # audible content (the round trip of full-scale noise would clip): speech-like synthetic audio quantised to 16 bits
    items = []
    for i, ((pcm, sr), name) in enumerate(zip(_items(), ("a16.wav", "b24.wav", "c44.wav"))):
        n, ch = pcm.shape
        x = torch.stack([_speech(n, 90 + i + c) for c in range(ch)], dim=1)
        pcm = (x.clamp(-1, 1) * 32767).round().to(torch.int16)
        (ind / name).write_bytes(_wav_bytes(1, ch, sr, 16, pcm.numpy().astype("<i2").tobytes()))
        got = wavio.read_pcm(str(ind / name))
        assert got is not None and got[1] == sr and torch.equal(got[0], pcm)
        items.append((pcm, sr))
    inference.main(["--config_path", str(cfg), "--synthetic_checkpoint", "--device", "cuda", "--batch_size", "3",
                    "--input_dir", str(ind), "--output_dir", str(outd), "--precision", "mixed", "--resample", "gpu"])
    m = model("tiny", "mixed")
    wavs = HostStager().to_device_pcm(items, torch.device(DEV), 16000)
    syn = m.decode(m.encode(wavs)["codes_list"])["syn_wav_list"]
    for (pcm, sr), name, w in zip(items, ("a16.wav", "b24.wav", "c44.wav"), syn):
        want_len = (math.ceil(16000 * pcm.shape[0] / sr) // 1280) * 1280
        out = wavio.read_pcm(str(outd / name))
        assert out is not None and out[1] == 16000 and tuple(out[0].shape) == (want_len, 1), name
        assert torch.equal(out[0][:, 0], ops.f32_to_pcm16(w.contiguous()).cpu()), name
