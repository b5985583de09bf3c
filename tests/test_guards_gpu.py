"""Guards around the hot path: range guard of the split-f16 / fp8 operands, device guard, default-device fast path,
out-of-range inputs that the reference tolerates."""
import logging

import numpy as np
import pytest
import torch

from common import PARAMS, oracle, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
NO_CLIPS = {"f16s": 0, "fp8": 0, "decode_f16s": 0, "decode_fp8": 0}       # saturation_count("all")


def _model(tag, precision, sd=None):
    from simwhisper_codec_amd.codec import AudioCodec
    m = AudioCodec(PARAMS[tag](), precision=precision)
    m.load_state_dict(sd if sd is not None else state_dict(tag), strict=True)
    return m.to(DEV).eval()


def test_saturation_counter_unit():
    """|x * 64| > 65504 in a split-f16 producer and |x * 16| > 448 in an fp8 producer set their counters; in-range
    data leaves them at zero."""
    from simwhisper_codec_amd import ops
    cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
    ops.set_saturation_counter(cnt)
    try:
        x = torch.full((4, 64), 3.0, device=DEV)
        ops.cast_f16s(x, 64)
        ops.cast_fp8(x)
        assert cnt.tolist() == [0, 0]
        x[1, 5] = 1023.4  # 1023.4 * 64 = 65497.6 < 65504: still representable
        ops.cast_f16s(x, 64)
        assert cnt.tolist() == [0, 0]
        x[1, 5] = -1024.0
        y = ops.cast_f16s(x, 64)
        assert cnt.tolist()[0] == 1
        v = y.view(4, 2, 2, 32).float()
        assert float((v[1, 0, 0, 5] + v[1, 0, 1, 5]) / 64) == -65504.0 / 64  # clipped, not inf
        x[1, 5] = 30.0  # 30 * 16 = 480 > 448
        ops.cast_fp8(x)
        assert cnt.tolist() == [1, 1]
        # LayerNorm with a large gain: output 50 * ~N(0,1) * 64 stays in range; gain 2000 does not
        h = torch.randn(8, 128, device=DEV)
        w, b = torch.full((128,), 50.0, device=DEV), torch.zeros(128, device=DEV)
        ops.layernorm(h, w, b, 1e-5, B=1, t_in=8, C_=128, out_dtype=torch.float16)
        assert cnt.tolist() == [1, 1]
        ops.layernorm(h, w * 40, b, 1e-5, B=1, t_in=8, C_=128, out_dtype=torch.float16)
        assert cnt.tolist()[0] > 1
    finally:
        ops.set_saturation_counter(None)
    n0 = cnt.tolist()
    ops.cast_f16s(torch.full((4, 64), 5000.0, device=DEV), 64)  # accounting off: nothing is counted
    assert cnt.tolist() == n0


def _outlier_state_dict(tag):
    """Whisper-style outlier channels on top of the synthetic checkpoint, as a function-preserving re-scaling: the
    LayerNorm gain / bias of a few channels x1024 and the consuming linears' columns / 1024 (powers of two: exact in
    fp32, so the reference's codes do not move), which pushes those LayerNorm outputs beyond the split-f16 range
    |x| < 1023."""
    sd = {k: v.clone() for k, v in state_dict(tag).items()}
    ch = [3, 4, 77]
    p = "acoustic_encoder.layers.0."
    sd[p + "final_layer_norm.weight"][ch] *= 1024.0
    sd[p + "final_layer_norm.bias"][ch] *= 1024.0
    sd[p + "fc1.weight"][:, ch] /= 1024.0
    p = "acoustic_encoder.layers.1."
    sd[p + "self_attn_layer_norm.weight"][ch] *= 1024.0
    sd[p + "self_attn_layer_norm.bias"][ch] *= 1024.0
    for w in ("q_proj", "k_proj", "v_proj"):
        sd[p + f"self_attn.{w}.weight"][:, ch] /= 1024.0
    return sd


def test_outlier_checkpoint_falls_back_and_stays_bit_exact(caplog):
    """A checkpoint whose activations leave the split-f16 range must still give the reference's codes: the encode is
    re-run on exact-f32 operands (policy "fallback"), and "raise" reports it instead."""
    from oracle.ref_cpu import Oracle
    from simwhisper_codec_amd import synth
    from simwhisper_codec_amd._lib import SwcError
    tag = "tiny"
    sd = _outlier_state_dict(tag)
    wavs = [synth.synth_audio(30000, index=300, kind="speech"), synth.synth_audio(21111, index=301, kind="noise")]
    want = Oracle(PARAMS[tag](), sd).encode(wavs, trim=True)["codes_list"]
    m = _model(tag, "mixed", sd)
    m.saturation_policy = "raise"
    with pytest.raises(SwcError, match="clipped"):
        m.encode([w.to(DEV) for w in wavs])
    m.saturation_policy = "ignore"
    bad = m.encode([w.to(DEV) for w in wavs])["codes_list"]
    assert m.precision == "mixed" and m.saturation_count()["f16s"] > 0
    m.saturation_policy = "fallback"
    with caplog.at_level(logging.WARNING):
        got = m.encode([w.to(DEV) for w in wavs])["codes_list"]
    assert m.precision == "mixed_f32" and "clipped" in caplog.text
    for a, b in zip(got, want):
        assert torch.equal(a.cpu().long(), b.long())
    # the clipped run really was different (otherwise this test exercises nothing)
    assert any(not torch.equal(a.cpu().long(), b.long()) for a, b in zip(bad, want))
    # the synthetic checkpoint itself never clips
    m2 = _model(tag, "mixed")
    m2.encode([w.to(DEV) for w in wavs])
    assert m2.saturation_count() == {"f16s": 0, "fp8": 0} and m2.precision == "mixed"


def test_replica_follows_the_range_fallback():
    """Batches in flight (pipeline.InFlight): a replica has no weights to pack from.  When ITS batch clips, the origin packs
    the exact-f32 preset once and the replica adopts it; the other replica follows at its next call.  Codes = the oracle's."""
    from oracle.ref_cpu import Oracle
    from simwhisper_codec_amd import synth
    from simwhisper_codec_amd.pipeline import InFlight
    tag = "tiny"
    sd = _outlier_state_dict(tag)
    wavs = [synth.synth_audio(30000, index=300, kind="speech"), synth.synth_audio(21111, index=301, kind="noise")]
    want = Oracle(PARAMS[tag](), sd).encode(wavs, trim=True)["codes_list"]
    m = _model(tag, "mixed", sd)
    assert m.precision == "mixed"
    dw = [w.to(DEV) for w in wavs]
    with InFlight(m, 2) as pipe:
        outs = pipe.map(lambda mdl, w: mdl.encode(w)["codes_list"], [dw] * 6)
        outs += [mm.encode(dw)["codes_list"] for mm in pipe.models]   # a model that sat idle follows at its next call
        assert all(mm.precision == "mixed_f32" for mm in pipe.models)
        assert pipe.models[1]._packed() is m._packed()
    for got in outs:
        for a, b in zip(got, want):
            assert torch.equal(a.cpu().long(), b.long())


def test_device_guard(monkeypatch):
    """Kernels run on the CURRENT device's stream: a tensor of another GPU is refused, and the public entry points make
    the model's GPU current (no second GPU needed: the current-device query is patched)."""
    from simwhisper_codec_amd import ops
    from simwhisper_codec_amd._lib import SwcError
    x = torch.zeros(4, 64, device=DEV)
    real = torch._C._cuda_getDevice
    monkeypatch.setattr(torch._C, "_cuda_getDevice", lambda: 1)
    with pytest.raises(SwcError, match="is current"):
        ops.cast_f16s(x, 64)
    monkeypatch.setattr(torch._C, "_cuda_getDevice", real)
    ops.cast_f16s(x, 64)
    m = _model("tiny", "mixed")
    with pytest.raises(SwcError, match="move the model"):
        m.encode([torch.zeros(4000, device=DEV)], device=torch.device("cuda", 1))


def test_default_device_takes_the_gather_path(monkeypatch):
    """encode()/decode() with the reference's default device=torch.device("cuda") (no index) must reach the one-kernel
    batch assembly and give the same bits as the indexed-device call."""
    from simwhisper_codec_amd import ops, synth
    m = _model("tiny", "mixed")
    wavs = [synth.synth_audio(20000 + 999 * i, index=500 + i).to(DEV) for i in range(3)]
    calls = []
    real = ops.gather_rows
    monkeypatch.setattr(ops, "gather_rows", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    c_def = m.encode(wavs)["codes_list"]
    assert len(calls) == 1
    w_def = m.decode(c_def)["syn_wav_list"]
    assert len(calls) == 2
    c_idx = m.encode(wavs, device=torch.device("cuda", 0))["codes_list"]
    w_idx = m.decode(c_idx, device=torch.device("cuda", 0))["syn_wav_list"]
    assert len(calls) == 4
    for a, b in zip(c_def + w_def, c_idx + w_idx):
        assert torch.equal(a, b)


def test_fsq_decode_out_of_range_codes():
    """quantizer.py:214-216 uses torch's floor `//` and `%`: negative and >= 2016 codes wrap the same way."""
    from simwhisper_codec_amd import ops
    codes = torch.tensor([-1, -7, -2016, -2017, 2016, 2017, 5000, 0, 2015, 336 * 6 + 5], dtype=torch.int64)
    G, B, T = 8, 1, codes.numel()
    c = codes.view(1, 1, T).expand(G, B, T).contiguous().to(DEV)
    lens = torch.tensor([T], dtype=torch.int32, device=DEV)
    zq = ops.fsq_decode(c, lens, B=B, T=T, G=G).cpu()
    base = torch.tensor([1, 8, 56, 336])
    lev = torch.tensor([8, 7, 6, 6])
    nn = (codes[:, None] // base) % lev
    want = (nn - lev // 2).float() / (lev // 2).float()
    for g in range(G):
        assert torch.equal(zq[0, :, 4 * g:4 * g + 4], want)


def test_tokenize_length_beyond_the_row():
    """model.py:180 slices xi[:, :x_len]: a length larger than the tensor is the tensor (no read past the row)."""
    from simwhisper_codec_amd import synth
    m = _model("tiny", "mixed")
    w = synth.synth_audio(16000, index=600).to(DEV)
    a = m.inference_tokenize(w.view(1, 1, -1), torch.tensor([16000]))
    b = m.inference_tokenize(w.view(1, 1, -1), torch.tensor([999999]))
    assert torch.equal(a["codes"], b["codes"]) and torch.equal(a["codes_lengths"], b["codes_lengths"])


@pytest.mark.parametrize("precision", ["mixed", "fp8"])
def test_packed_operand_checkpoint_is_identical(tmp_path, precision):
    """tools/pack_checkpoint.py --fold: a model loaded from the packed-operand file never runs the fold /
    scale / cast pass and must give bit-identical codes and waveforms to the model loaded from the reference layout."""
    import subprocess, sys, yaml
    from audiocodec.model import AudioCodec
    from simwhisper_codec_amd import synth
    from simwhisper_codec_amd._lib import SwcError
    from common import ROOT
    import os
    gp = PARAMS["tiny"]()
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump({"generator_params": gp}))
    torch.save(state_dict("tiny"), tmp_path / "ref.pt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pack_checkpoint.py"), "--config", str(cfg), "--in",
                        str(tmp_path / "ref.pt"), "--fold", "--precision", precision, "--out", str(tmp_path / "pk.safetensors")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-1500:]
    a = AudioCodec.load_from_checkpoint(str(cfg), str(tmp_path / "ref.pt"))
    a.precision = precision
    a = a.to(DEV).eval()
    b = AudioCodec.load_from_checkpoint(str(cfg), str(tmp_path / "pk.safetensors")).to(DEV).eval()
    assert b.precision == precision and len(list(b.buffers())) == 1  # no state_dict tensors were built or moved
    called = []
    b._pack = lambda dev: called.append(1)
    wavs = [synth.synth_audio(30000 + 777 * i, index=900 + i, kind="speech" if i % 2 else "noise").to(DEV) for i in range(3)]
    ca, cb = a.encode(wavs)["codes_list"], b.encode(wavs)["codes_list"]
    wa, wb = a.decode(ca)["syn_wav_list"], b.decode(cb)["syn_wav_list"]
    assert not called
    for x, y in zip(ca + wa, cb + wb):
        assert torch.equal(x, y)
    with pytest.raises(SwcError, match="packed for precision"):
        b.precision = "fp32"
    # a packed file is bound to its configuration
    gp2 = PARAMS["tiny"]()
    gp2["vocos"]["num_layers"] = 2
    cfg2 = tmp_path / "cfg2.yaml"
    cfg2.write_text(yaml.safe_dump({"generator_params": gp2}))
    with pytest.raises(SwcError, match="another configuration"):
        AudioCodec.load_from_checkpoint(str(cfg2), str(tmp_path / "pk.safetensors"))


def test_deferred_range_check_redo():
    """deferred_range_check(): no read-back (no stream sync) between encode and decode; one read-back when the block ends;
    on clipping the model has switched to exact-f32 operands and the redone block gives the reference's codes."""
    from oracle.ref_cpu import Oracle
    from simwhisper_codec_amd import synth
    tag = "tiny"
    sd = _outlier_state_dict(tag)
    wavs = [synth.synth_audio(30000, index=300, kind="speech"), synth.synth_audio(21111, index=301, kind="noise")]
    want = Oracle(PARAMS[tag](), sd).encode(wavs, trim=True)["codes_list"]
    m = _model(tag, "mixed", sd)
    dw = [w.to(DEV) for w in wavs]
    with m.deferred_range_check() as chk:
        c = m.encode(dw)["codes_list"]
        assert m.precision == "mixed"          # nothing was read back yet
        m.decode(c)
    assert chk.clipped and m.precision == "mixed_f32"
    with m.deferred_range_check() as chk2:
        c = m.encode(dw)["codes_list"]
        m.decode(c)
    assert not chk2.clipped
    for a, b in zip(c, want):
        assert torch.equal(a.cpu().long(), b.long())
    m2 = _model(tag, "mixed")               # the plain checkpoint: nothing clips, nothing changes
    with m2.deferred_range_check() as chk3:
        m2.decode(m2.encode(dw)["codes_list"])
    assert not chk3.clipped and m2.precision == "mixed"


def test_packed_outlier_checkpoint_falls_back(tmp_path, caplog):
    """The deployment case of the range guard: an outlier checkpoint shipped as a packed-operand file (`export_packed` /
    tools/pack_checkpoint.py --fold, preset `mixed`).  The file carries the exact-f32 encoder operands of the fallback
    preset beside the split-f16 ones; when the encode clips, the model adopts them (no f32 weights exist to pack from)
    and returns the reference's codes — also from a replica running beside its origin (pipeline.InFlight)."""
    import yaml
    from audiocodec.model import AudioCodec
    from oracle.ref_cpu import Oracle
    from simwhisper_codec_amd import packed, synth
    from simwhisper_codec_amd.pipeline import InFlight
    tag = "tiny"
    sd = _outlier_state_dict(tag)
    wavs = [synth.synth_audio(30000, index=300, kind="speech"), synth.synth_audio(21111, index=301, kind="noise")]
    want = Oracle(PARAMS[tag](), sd).encode(wavs, trim=True)["codes_list"]
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump({"generator_params": PARAMS[tag]()}))
    path = str(tmp_path / "outlier.mixed.safetensors")
    src = _model(tag, "mixed", sd)
    src.export_packed(path)
    assert src.precision == "mixed"                       # exporting the fallback operands did not switch the source
    assert packed.peek(path)["fallback"] == "mixed_f32"
    dw = [w.to(DEV) for w in wavs]
    m = AudioCodec.load_from_checkpoint(str(cfg), path).to(DEV).eval()
    assert m.precision == "mixed" and len(list(m.buffers())) == 1
    with caplog.at_level(logging.WARNING):
        got = m.encode(dw)["codes_list"]
    assert m.precision == "mixed_f32" and "clipped" in caplog.text
    for a, b in zip(got, want):
        assert torch.equal(a.cpu().long(), b.long())
    wav = m.decode(got)["syn_wav_list"]                    # the decode side of the file is untouched by the switch
    ref = src.decode([c.to(DEV) for c in want])["syn_wav_list"]
    for a, b in zip(wav, ref):
        assert torch.equal(a, b)
    # replicas of a packed-file model follow the same way
    m2 = AudioCodec.load_from_checkpoint(str(cfg), path).to(DEV).eval()
    with InFlight(m2, 2) as pipe:
        outs = pipe.map(lambda mdl, w: mdl.encode(w)["codes_list"], [dw] * 4)
        outs += [mm.encode(dw)["codes_list"] for mm in pipe.models]
        assert all(mm.precision == "mixed_f32" for mm in pipe.models)
    for got in outs:
        for a, b in zip(got, want):
            assert torch.equal(a.cpu().long(), b.long())
    # a file without the fallback part (older writer): the clip is reported as such, not as a packing mismatch
    P = src._packed()
    old = str(tmp_path / "old.safetensors")
    from simwhisper_codec_amd.codec import _PACK_CLASSES, _config_digest
    from simwhisper_codec_amd import ops
    from simwhisper_codec_amd._lib import SwcError
    packed.save(old, P, _PACK_CLASSES, {"precision": "mixed", "config": _config_digest(PARAMS[tag]()), "abi": ops.abi_version()})
    m3 = AudioCodec.load_from_checkpoint(str(cfg), old).to(DEV).eval()
    with pytest.raises(SwcError, match="clipped"):
        m3.encode(dw)


def test_nested_models_keep_their_range_counters():
    """_on_model_device restores the calling thread's counter pointer: a call into a second model from inside (or between)
    calls of a first one must not leave the first one's later kernels uncounted."""
    from simwhisper_codec_amd import synth
    tag = "tiny"
    sd = _outlier_state_dict(tag)
    a = _model(tag, "mixed", sd)
    a.saturation_policy = "ignore"
    b = _model(tag, "mixed")
    w = [synth.synth_audio(30000, index=300, kind="speech").to(DEV)]
    real = a._encode_padded

    def nested(*args, **kw):      # model b runs to completion in the middle of a's encode
        b.encode(w)
        return real(*args, **kw)
    a._encode_padded = nested
    try:
        a.encode(w)
    finally:
        del a._encode_padded
    assert a.saturation_count()["f16s"] > 0 and b.saturation_count() == {"f16s": 0, "fp8": 0}


def _vocos_outlier_state_dict(tag):
    """The decode side's outlier checkpoint, function-preserving like _outlier_state_dict: gain and bias of Vocos' final
    LayerNorm x1024 on a few channels, the head's columns / 1024.  That LayerNorm writes split-f16 in every 16-bit preset
    (vocos_head_split_f16), so its output leaves |x| < 1023 on the DECODE side; no encode-side tensor changes."""
    sd = {k: v.clone() for k, v in state_dict(tag).items()}
    ch = [3, 4, 37]
    sd["vocos.backbone.final_layer_norm.weight"][ch] *= 1024.0
    sd["vocos.backbone.final_layer_norm.bias"][ch] *= 1024.0
    sd["vocos.head.out.weight"][:, ch] /= 1024.0
    return sd


def _guard_records(caplog):
    return [r.getMessage() for r in caplog.records if "clipped" in r.getMessage()]


def test_decode_clips_are_not_charged_to_the_encoder(caplog):
    """decode() clips (Vocos' final LayerNorm, split-f16 in `mixed`) count into the decode side's own pair and are reported
    on their own, once; the encode() after it neither warns of clipped encoder operands, nor raises, nor re-runs, nor leaves
    `mixed`, and gives the codes of a model that never decoded.  The same inside forward() (encode + decode in one entry
    point) and inside deferred_range_check().
    On the parent commit: the encode after the decode re-ran and left the model on mixed_f32 ("fallback"), raised ("raise")."""
    from simwhisper_codec_amd import synth
    from simwhisper_codec_amd._lib import SwcError
    tag = "tiny"
    sd = _vocos_outlier_state_dict(tag)
    dw = [synth.synth_audio(30000, index=300, kind="speech").to(DEV), synth.synth_audio(21111, index=301, kind="noise").to(DEV)]
    fresh = _model(tag, "mixed", sd)
    want = fresh.encode(dw)["codes_list"]
    assert fresh.saturation_count("all") == NO_CLIPS and fresh.precision == "mixed"     # the encode side of this checkpoint is clean
    m = _model(tag, "mixed", sd)
    runs = []
    real = m._encode_mel
    m._encode_mel = lambda *a, **k: (runs.append(1), real(*a, **k))[1]
    with caplog.at_level(logging.WARNING):
        m.decode(want)
        got = m.encode(dw)["codes_list"]
        n = m.saturation_count("all")
    assert m.precision == "mixed" and len(runs) == 1
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert n["decode_f16s"] > 0 and n["f16s"] == 0 and n["fp8"] == 0 and n["decode_fp8"] == 0, n
    rec = _guard_records(caplog)
    assert len(rec) == 1 and rec[0].startswith("decode-side"), rec
    with caplog.at_level(logging.WARNING):                                         # ... once: later decodes count on silently
        m.decode(want)
        m.encode(dw)
        n2 = m.saturation_count("all")
    assert n2["decode_f16s"] > n["decode_f16s"] and n2["f16s"] == 0 and len(_guard_records(caplog)) == 1 and m.precision == "mixed"
    # "raise": the decode call itself reports; the encode after it is untouched
    m.saturation_policy = "raise"
    with pytest.raises(SwcError, match="decode-side"):
        m.decode(want)
    got = m.encode(dw)["codes_list"]
    assert m.precision == "mixed" and all(torch.equal(a, b) for a, b in zip(got, want))
    # "ignore" counts only
    caplog.clear()
    m3 = _model(tag, "mixed", sd)
    m3.saturation_policy = "ignore"
    with caplog.at_level(logging.WARNING):
        m3.decode(want)
        assert m3.saturation_count("all")["decode_f16s"] > 0 and not _guard_records(caplog)
    # decode-only use: no encode-side read-back ever comes; the third decode looks at the snapshot the second left behind
    caplog.clear()
    m6 = _model(tag, "mixed", sd)
    with caplog.at_level(logging.WARNING):
        for _ in range(4):
            m6.decode(want)
            torch.cuda.synchronize()
    rec = _guard_records(caplog)
    assert len(rec) == 1 and rec[0].startswith("decode-side") and m6.precision == "mixed", rec
    # encode and decode inside one entry point
    caplog.clear()
    g = torch.Generator().manual_seed(3)
    batch = {"mel_features": (torch.rand(2, 80, 200, generator=g) * 0.8 + 0.2).to(DEV), "mel_lens": torch.tensor([200, 121], device=DEV)}
    m4 = _model(tag, "mixed", sd)
    with caplog.at_level(logging.WARNING):
        m4.forward(batch)
        m4.forward(batch)
        n4 = m4.saturation_count("all")
    assert m4.precision == "mixed" and n4["decode_f16s"] > 0 and n4["f16s"] == 0
    rec = _guard_records(caplog)
    assert len(rec) == 1 and rec[0].startswith("decode-side"), rec
    # deferred_range_check(): the decode inside the block is not read as a clip of the block's encode
    m5 = _model(tag, "mixed", sd)
    for _ in range(2):
        with m5.deferred_range_check() as chk:
            c = m5.encode(dw)["codes_list"]
            m5.decode(c)
        assert not chk.clipped and m5.precision == "mixed"
        assert all(torch.equal(a, b) for a, b in zip(c, want))
    assert m5.saturation_count("all")["decode_f16s"] > 0 and m5.saturation_count("all")["f16s"] == 0


def test_stale_snapshot_reports_nothing(caplog):
    """_check_clipping(snapshot=True) on a snapshot that is older than `seen` (a full read-back was checked after the snapshot
    was taken): no warning, no fallback, no raise, `seen` does not move back; and a full read-back retires a pending snapshot.
    On the parent commit: new16 = 0 - seen < 0 is truthy: SwcError under "raise", a switch to mixed_f32 under "fallback"."""
    from simwhisper_codec_amd import synth
    tag = "tiny"
    m = _model(tag, "mixed", _outlier_state_dict(tag))
    dw = [synth.synth_audio(30000, index=300, kind="speech").to(DEV)]
    m.saturation_policy = "ignore"
    m.encode(dw)                                         # creates the counters; full read-back: seen = c1 > 0
    st = m._sat
    c1 = list(st["seen"])
    assert c1[0] > 0 and st["snap_ev"] is None
    torch.cuda.synchronize()
    st["buf"].zero_()                                    # a snapshot of "before those clips": what an older snapshot holds
    m._snapshot_counters()
    torch.cuda.synchronize()
    st["buf"].copy_(torch.tensor(c1, dtype=torch.int32))
    assert st["snap"].tolist()[:2] == [0, 0] and st["snap_ev"] is not None
    for policy in ("raise", "fallback"):
        m.saturation_policy = policy
        ev = st["snap_ev"]
        with caplog.at_level(logging.WARNING):
            assert m._check_clipping("mixed", snapshot=True) is False
        assert m.precision == "mixed" and st["seen"] == c1 and st["snap_ev"] is None and not _guard_records(caplog)
        st["snap_ev"] = ev                               # the same stale snapshot again for the next policy
    with caplog.at_level(logging.WARNING):               # the fp8 side of the same arithmetic: slot 1 behind `seen`
        st["seen"] = [c1[0], 5]
        assert m._check_clipping("fp8", snapshot=True) is False
    assert st["seen"] == [c1[0], 5] and not st["warned"] and not [r for r in caplog.records if "fp8 preset" in r.getMessage()]
    # a full read-back supersedes a pending snapshot
    m.saturation_policy = "ignore"
    st["seen"] = list(c1)
    m._snapshot_counters()
    m._check_clipping("mixed")
    assert st["snap_ev"] is None and st["seen"] == c1


# ------------------------------------------------------------------------------------------- encode-side site sweep
# One checkpoint per producer of a split-f16 activation on the encode path of `mixed`, each pushing that site's output (and
# no other reduced-range tensor) beyond |x| = 1023 on a few channels, by powers of two.  Linear sites are re-scaled
# function-preservingly as in _outlier_state_dict (producer rows x 2^k, consumer columns / 2^k); behind a GELU or a snake the
# function changes, and through a weight-normed conv the column re-scaling is exact only up to the re-normalisation — so the
# oracle is computed afresh for every checkpoint.
def _rows(sd, p, rows, s):
    """output channels `rows` of the linear / conv at `p` times s, its bias too (a weight-normed conv: through weight_g)"""
    key = p + ".weight_g" if p + ".weight_g" in sd else p + ".weight"
    sd[key] = sd[key].clone()
    sd[key][rows] *= s
    if p + ".bias" in sd:
        sd[p + ".bias"] = sd[p + ".bias"].clone()
        sd[p + ".bias"][rows] *= s


def _cols(sd, p, cols, s):
    """input channels `cols` of the linear / conv at `p` times s (a weight-normed conv: weight_v columns, weight_g re-normalised)"""
    if p + ".weight_v" in sd:
        v = sd[p + ".weight_v"].clone()
        old = v.reshape(v.shape[0], -1).norm(dim=1)
        v[:, cols] *= s
        sd[p + ".weight_v"] = v
        sd[p + ".weight_g"] = sd[p + ".weight_g"] * (v.reshape(v.shape[0], -1).norm(dim=1) / old).view(-1, 1, 1)
    else:
        w = sd[p + ".weight"].clone()
        w[:, cols] *= s
        sd[p + ".weight"] = w


def _site_state_dict(tag, site):
    sd = dict(state_dict(tag))
    gp = PARAMS[tag]()
    L0 = "acoustic_encoder.layers.0."
    ch, hc = [3, 4, 77], [3, 4, 37]                       # channels of d_model / of the down-sampler's hidden_dim
    big, inv = 2.0 ** 14, 2.0 ** -14
    if site == "conv1_gelu":
        _rows(sd, "acoustic_encoder.conv1", ch, big)
        _cols(sd, "acoustic_encoder.conv2", ch, inv)
    elif site in ("q", "k"):
        a, b = ("q_proj", "k_proj") if site == "q" else ("k_proj", "q_proj")
        head0 = list(range(64))                           # every channel of head 0: a few clipped channels do not move a code
        _rows(sd, L0 + "self_attn." + a, head0, big)      # q . k is unchanged
        _rows(sd, L0 + "self_attn." + b, head0, inv)
    elif site == "v":
        _rows(sd, L0 + "self_attn.v_proj", ch, big)
        _cols(sd, L0 + "self_attn.out_proj", ch, inv)
    elif site == "fc1_gelu":
        wide = list(range(64))                            # GELU zeroes the negative half: enough channels for any 2 s input
        _rows(sd, L0 + "fc1", wide, 2.0 ** 16)
        _cols(sd, L0 + "fc2", wide, 2.0 ** -16)
    elif site == "encoder_ln":
        for k in ("weight", "bias"):
            sd["acoustic_encoder.layer_norm." + k] = sd["acoustic_encoder.layer_norm." + k].clone()
            sd["acoustic_encoder.layer_norm." + k][ch] *= 1024.0
        s = gp["downsample"]["stack_factor"]
        _cols(sd, "downsample.in_proj", [c * s + i for c in ch for i in range(s)], 1.0 / 1024.0)
    elif site in ("snake1", "snake2"):
        # snake(x) = x + sin^2(alpha x) / beta with beta = exp(parameter): 1 / beta = e^10 = 22026 on a few channels
        blk, nxt = ("0", "1") if site == "snake1" else ("2", "3")
        key = f"downsample.res_blocks.0.block.{blk}.act.beta"
        sd[key] = sd[key].clone()
        sd[key][hc] = -10.0
        _cols(sd, f"downsample.res_blocks.0.block.{nxt}", hc, inv)
    elif site == "to_latent_cast":
        _rows(sd, "downsample.res_blocks.2.block.3", hc, big)     # the last residual unit's output: only the cast reads it
        _cols(sd, "downsample.to_latent", hc, inv)
    else:
        raise ValueError(site)
    return sd


ENCODE_SITES = ["conv1_gelu", "q", "k", "v", "fc1_gelu", "encoder_ln", "snake1", "snake2", "to_latent_cast"]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x.cpu().long(), y.cpu().long()) for x, y in zip(a, b))


def _policies(m, dw, want, caplog):
    """the assertions of test_outlier_checkpoint_falls_back_and_stays_bit_exact on model m (`mixed`) against the codes `want`"""
    from simwhisper_codec_amd._lib import SwcError
    m.saturation_policy = "raise"
    with pytest.raises(SwcError, match="clipped"):
        m.encode(dw)
    m.saturation_policy = "ignore"
    bad = m.encode(dw)["codes_list"]
    n = m.saturation_count()
    assert m.precision == "mixed" and n["f16s"] > 0 and n["fp8"] == 0, n
    assert not _same(bad, want), "the clipped run gave the reference's codes: the checkpoint exercises nothing"
    m.saturation_policy = "fallback"
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        got = m.encode(dw)["codes_list"]
    assert m.precision == "mixed_f32" and "clipped" in caplog.text
    assert _same(got, want)


@pytest.mark.parametrize("site", ENCODE_SITES)
def test_encode_site_sweep_tiny(site, caplog):
    """every encode-side producer site, `tiny` configuration: "raise" raises; "ignore" counts and its codes really differ;
    "fallback" ends on mixed_f32 with the codes of a fresh mixed_f32 model on the same checkpoint, which are the oracle's."""
    from oracle.ref_cpu import Oracle
    from simwhisper_codec_amd import synth
    tag = "tiny"
    sd = _site_state_dict(tag, site)
    wavs = [synth.synth_audio(30000, index=300, kind="speech"), synth.synth_audio(21111, index=301, kind="noise")]
    dw = [w.to(DEV) for w in wavs]
    want = Oracle(PARAMS[tag](), sd).encode(wavs, trim=True)["codes_list"]
    fresh = _model(tag, "mixed_f32", sd)
    ref = fresh.encode(dw)["codes_list"]
    assert fresh.saturation_count("all") == NO_CLIPS and fresh.precision == "mixed_f32"
    assert _same(ref, want), "a fresh mixed_f32 model disagrees with the oracle on this checkpoint"
    _policies(_model(tag, "mixed", sd), dw, want, caplog)


_REAL_REF = {}


def _real_inputs(form):
    from simwhisper_codec_amd import synth
    if form == "padded":
        return [synth.synth_audio(32000, index=310, kind="speech").to(DEV)]
    return [synth.synth_audio(32000, index=310, kind="speech").to(DEV), synth.synth_audio(14000, index=311, kind="noise").to(DEV)]


@pytest.mark.parametrize("form", ["padded", "ragged"])
@pytest.mark.parametrize("site", ENCODE_SITES)
def test_encode_site_sweep_real(site, form, caplog):
    """the same on the real configuration (d_model 768, hidden 512: the real GEMM geometries and layernorm2_kernel) with one 2 s
    utterance, and with a ragged pair whose transformer runs on valid-token packing; against a fresh mixed_f32 model, built
    once per site (its codes for both forms are kept in _REAL_REF).  Measured on an MI355X: 1.3 s for the first case (it builds the
    real configuration's synthetic checkpoint), 0.12 - 0.25 s for each of the other 17."""
    tag = "real"
    sd = _site_state_dict(tag, site)
    if site not in _REAL_REF:
        fresh = _model(tag, "mixed_f32", sd)
        _REAL_REF[site] = {f: fresh.encode(_real_inputs(f))["codes_list"] for f in ("padded", "ragged")}
        assert fresh.saturation_count("all") == NO_CLIPS and fresh.precision == "mixed_f32"
        del fresh
    dw = _real_inputs(form)
    m = _model(tag, "mixed", sd)
    if form == "ragged":
        packed = []
        real = m._pack_plan
        m._pack_plan = lambda *a, **k: (packed.append(real(*a, **k)), packed[-1])[1]
    _policies(m, dw, _REAL_REF[site][form], caplog)
    if form == "ragged":
        # (every `mixed` run of it; the re-run on exact-f32 operands has no packed attention kernel)
        assert len([p for p in packed if p[0] is not None]) >= 3, "the ragged pair did not take valid-token packing"


@pytest.mark.parametrize("precision", ["fp8", "fp8_fc1"])
def test_fp8_presets_warn_once_and_never_rerun(precision, caplog):
    """fp8 presets: a clip moves slot 1 only, warns once (looked at when the next call comes in), never re-runs the encode and
    leaves the preset unchanged."""
    from simwhisper_codec_amd import synth
    tag = "tiny"
    m = _model(tag, precision, _outlier_state_dict(tag))
    dw = [synth.synth_audio(30000, index=300, kind="speech").to(DEV)]
    runs = []
    real = m._encode_mel
    m._encode_mel = lambda *a, **k: (runs.append(1), real(*a, **k))[1]
    with caplog.at_level(logging.WARNING):
        for _ in range(4):
            m.encode(dw)
            torch.cuda.synchronize()
    n = m.saturation_count()
    assert len(runs) == 4 and m.precision == precision
    assert n["fp8"] > 0 and n["f16s"] == 0, n
    assert len([r for r in caplog.records if "fp8 preset" in r.getMessage()]) == 1
    assert not [r for r in caplog.records if "re-running" in r.getMessage()]
