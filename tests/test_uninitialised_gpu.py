"""The product path must not depend on uninitialised memory (DESIGN.md "Memory contract").

Every scratch buffer and output of the path is torch.empty: a fresh test process mostly gets zero pages, a serving process
gets recycled blocks holding the previous batch.  Each case here runs the same call three times — clean, under
poison.poisoned_empty("nan") and under poisoned_empty("big") — and requires every returned tensor (bit for bit), every
shape, the range-guard counters and the preset the model ended in to be equal.  The poisoned runs use a model that was
BUILT under the poison (packed operands, streams) and whose cached scratch (pinned staging rows, uploaded length lists,
counters) is born under the poison of that run.  A spy on the wrappers proves the poisoned runs really allocated.
Each preset, batch, knob and surface appears at least once; this is not a cross product.
"""
import contextlib

import pytest
import torch

import poison
from common import PARAMS, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"

_CLEAN, _POISONED = {}, {}


def _build(tag, precision):
    from simwhisper_codec_amd.codec import AudioCodec
    m = AudioCodec(PARAMS[tag](), precision=precision)
    m.load_state_dict(state_dict(tag), strict=True)
    m = m.to(DEV).eval()
    m._packed()
    return m


def _reset_scratch(m):
    """scratch a model keeps across calls: the pinned staging ring and the uploaded length lists of _dev_ints, the counters"""
    for k in ("_ints_cache", "_pin", "_sat"):
        m.__dict__.pop(k, None)


def _model(tag, precision, pattern):
    """clean: built and run outside any poison.  Poisoned: built under "nan" (call this inside the poisoned block); its cached
    scratch is dropped so that it is born again under the pattern of the current run."""
    key = (tag, precision)
    if pattern is None:
        if key not in _CLEAN:
            _CLEAN[key] = _build(tag, precision)
        return _CLEAN[key]
    if key not in _POISONED:
        with poison.poisoned_empty("nan"):
            _POISONED[key] = _build(tag, precision)
    _reset_scratch(_POISONED[key])
    return _POISONED[key]


@contextlib.contextmanager
def _knobs(m, knobs):
    try:
        for k, v in knobs.items():
            setattr(m, k, v)
        yield
    finally:
        for k in knobs:
            m.__dict__.pop(k, None)


def _flat(o, path="out"):
    if torch.is_tensor(o):
        return [(path, o)]
    if isinstance(o, dict):
        return [x for k in sorted(o) for x in _flat(o[k], f"{path}[{k!r}]")]
    if isinstance(o, (list, tuple)):
        return [x for i, v in enumerate(o) for x in _flat(v, f"{path}[{i}]")]
    return [(path, torch.tensor(o))] if isinstance(o, (int, float, bool)) else []


def run3(tag, precision, call, knobs=None):
    """call(model) -> tensors (any nesting) under the three conditions; everything equal.  Returns the clean result."""
    results = []
    for pattern in (None, "nan", "big"):
        with (poison.poisoned_empty(pattern) if pattern else contextlib.nullcontext()) as spy:
            m = _model(tag, precision, pattern)
            before = m.saturation_count()
            with _knobs(m, knobs or {}):
                out = call(m)
            torch.cuda.synchronize()
            after = m.saturation_count()
            flat = [(p, t.detach().clone()) for p, t in _flat(out)]
        if pattern:
            assert spy.device_calls > 0, "the poisoned run allocated nothing through torch.empty: the wrapper is not in the path"
        results.append((out, flat, {k: after[k] - before[k] for k in after}, m.precision))
    _, f0, c0, p0 = results[0]
    assert p0 == precision, f"the clean run left the model on {p0}"
    for pattern, (_, f, c, p) in zip(("nan", "big"), results[1:]):
        assert p == p0, f"{pattern}: the model ended in preset {p}, the clean run in {p0} (a fallback that depends on scratch memory)"
        assert c == c0, f"{pattern}: range-guard counters {c}, clean run {c0}"
        assert [a for a, _ in f] == [a for a, _ in f0]
        for (path, a), (_, b) in zip(f0, f):
            assert a.shape == b.shape, f"{pattern}: {path} has shape {tuple(b.shape)}, clean run {tuple(a.shape)}"
            assert poison.same_bits(a, b), f"{pattern}: {path} differs from the clean run"
    return results[0][0]


def _wavs(secs, base, stride):
    from simwhisper_codec_amd import synth
    return [synth.synth_audio(int(16000 * t) + stride * i, index=base + i, kind="speech" if i % 2 else "noise").to(DEV)
            for i, t in enumerate(secs)]


def _batch8():     # the batch of test_valid_token_packing_is_exact
    return _wavs([9.0, 1.1, 4.3, 0.3, 7.7, 2.0, 0.05, 5.5], 970, 29)


def _batch10():    # the batch of test_ragged_vocos_tile_skipping_is_exact: the fused block kernel runs with t_limit
    return _wavs([27.0, 2.2, 11.3, 0.7, 19.9, 6.1, 24.5, 3.3, 14.0, 1.0], 1200, 31)


def _encode_decode(wavs):
    def call(m):
        codes = m.encode(wavs)["codes_list"]
        return {"codes_list": codes, "syn_wav_list": m.decode(codes)["syn_wav_list"]}
    return call


# ------------------------------------------------------------------------------------------------------------- presets
@pytest.mark.parametrize("tag,precision", [("real", "fp32"), ("real", "mixed"), ("real", "bf16"), ("real", "f16s"), ("real", "fp8"),
                                           ("real", "fp8_fc1"), ("tiny", "fp32"), ("tiny", "mixed")])
def test_presets_encode_decode(tag, precision):
    out = run3(tag, precision, _encode_decode(_batch8()))
    assert all(torch.isfinite(w).all() for w in out["syn_wav_list"])


@pytest.mark.parametrize("tag,precision", [("real", "fp32"), ("real", "mixed"), ("real", "bf16"), ("real", "f16s"), ("real", "fp8"),
                                           ("real", "fp8_fc1"), ("tiny", "fp32"), ("tiny", "mixed")])
def test_packed_operands_built_under_poison_equal_the_clean_ones(tag, precision):
    """_packed() tensor by tensor: every operand, scale and operand stream (prefetch tails included)"""
    from simwhisper_codec_amd import packed
    from simwhisper_codec_amd.codec import _PACK_CLASSES
    sk0, t0 = packed.flatten(_model(tag, precision, None)._packed(), _PACK_CLASSES)
    built = [_model(tag, precision, "nan")]
    if tag == "tiny" or precision == "mixed":        # a second build under the finite pattern where it is cheap / on the metric preset
        with poison.poisoned_empty("big"):
            built.append(_build(tag, precision))
    for m in built:
        sk, t = packed.flatten(m._packed(), _PACK_CLASSES)
        assert sk == sk0 and sorted(t) == sorted(t0)
        for name in t0:
            assert poison.same_bits(t0[name], t[name]), f"packed operand {name} depends on uninitialised memory"


@pytest.mark.parametrize("precision", ["fp32", "mixed"])
def test_packed_checkpoint_file_is_byte_identical(precision, tmp_path):
    """A packed-operand file (AudioCodec.export_packed, tools/pack_checkpoint.py --fold) written under poison against one written
    clean: the payload (every tensor byte, in file order) byte for byte, and every header entry.  The container's header is
    one JSON object whose key order the safetensors writer does not fix between two saves (its metadata is an unordered map),
    so the header is compared as parsed JSON and the 8-byte length + payload as bytes."""
    import json
    import struct
    files = []
    for pattern in (None, "nan", "big"):
        path = str(tmp_path / f"{pattern}.safetensors")
        with (poison.poisoned_empty(pattern) if pattern else contextlib.nullcontext()):
            m = _build("tiny", precision) if pattern else _model("tiny", precision, None)
            m.export_packed(path)
        raw = open(path, "rb").read()
        n = struct.unpack("<Q", raw[:8])[0]
        files.append((n, json.loads(raw[8:8 + n]), raw[8 + n:]))
    assert len(files[0][2]) > 1 << 16
    for pattern, f in zip(("nan", "big"), files[1:]):
        assert f[0] == files[0][0], f"{pattern}: header length differs"
        assert f[1] == files[0][1], f"{pattern}: header entries differ"
        assert f[2] == files[0][2], f"{pattern}: the payload of the packed-operand file depends on uninitialised memory"


# ------------------------------------------------------------------------------------------------------ batches and knobs
def test_ragged_batch_with_tile_skipping():
    """10 rows x up to 2700 frames: the fused ConvNeXt block runs with t_limit (skipped tiles are never written)"""
    from simwhisper_codec_amd import ops
    codes = _model("real", "mixed", None).encode(_batch10())["codes_list"]
    seen = []
    real = ops.convnext_block
    ops.convnext_block = lambda *a, **k: (seen.append(k.get("t_limit") is not None), real(*a, **k))[1]
    try:
        run3("real", "mixed", lambda m: m.decode(codes)["syn_wav_list"])
        assert seen and all(seen)
        del seen[:]
        run3("real", "mixed", lambda m: m.decode(codes)["syn_wav_list"], knobs={"ragged_vocos": False})
        assert seen and not any(seen)
    finally:
        ops.convnext_block = real


def test_ragged_detokenize_is_deterministic_beyond_the_lengths():
    """inference_detokenize(_ragged=True) returns whole padded rows: the fused ConvNeXt block skips the tiles beyond a row's
    limit (t_limit) and never writes them, so the samples beyond codes_lengths[i] * 1280 are don't-care — but they must be
    the same don't-care in every process: codec.py zero-fills the ping-pong buffer once for exactly that (the reference
    zero-fills beyond the valid length).  With torch.empty_like there, this test fails; the kept samples never do."""
    g = torch.Generator().manual_seed(8)
    m0 = _model("real", "mixed", None)
    codes = torch.randint(0, 2016, (m0.num_groups, 4, 100), generator=g).to(DEV)
    lens = torch.tensor([100, 30, 10, 60])
    seen = []
    from simwhisper_codec_amd import ops
    real = ops.convnext_block
    ops.convnext_block = lambda *a, **k: (seen.append(k.get("t_limit") is not None), real(*a, **k))[1]
    try:
        run3("real", "mixed", lambda m: m.inference_detokenize(codes, lens, _ragged=True), knobs={"fused_mlp_min_rows": 0})
    finally:
        ops.convnext_block = real
    assert seen and all(seen)


@pytest.mark.parametrize("knobs", [{"varlen_packing": False}, {"length_bucketing": False},
                                   {"fused_mlp_min_rows": 0, "fused_layer_mlp_min_rows": 0},
                                   {"fused_mlp_min_rows": 1 << 40, "fused_layer_mlp_min_rows": 1 << 40}],
                         ids=["no_varlen_packing", "no_length_bucketing", "fused_forced", "fused_excluded"])
def test_knobs(knobs):
    run3("real", "mixed", _encode_decode(_batch8()), knobs=knobs)


def test_uniform_batch_and_two_vocos_streams():
    run3("real", "mixed", _encode_decode(_wavs([3.0, 3.0], 40, 0)))
    g = torch.Generator().manual_seed(5)
    m0 = _model("real", "mixed", None)
    codes = [torch.randint(0, 2016, (m0.num_groups, 120 - (i % 3)), generator=g).to(DEV) for i in range(24)]
    run3("real", "mixed", lambda m: m.decode(codes)["syn_wav_list"], knobs={"vocos_streams": 2})


@pytest.mark.parametrize("tag,precision", [("tiny", "fp32"), ("tiny", "mixed")])
def test_empty_and_one_sample_utterances(tag, precision):
    wavs = _wavs([1.3, 0.0, 2.1], 60, 7)
    wavs[1] = wavs[1][:0]
    wavs.insert(2, _wavs([0.5], 70, 0)[0][:1])
    out = run3(tag, precision, _encode_decode(wavs))
    assert out["codes_list"][1].shape[1] == 0 and out["syn_wav_list"][1].numel() == 0


# -------------------------------------------------------------------------------------------------------------- surfaces
@pytest.mark.parametrize("tag,precision", [("tiny", "fp32"), ("tiny", "mixed")])
def test_tokenize_detokenize(tag, precision):
    wavs = _wavs([3.0, 1.2, 0.4], 80, 11)
    n = [int(w.numel()) for w in wavs]
    x = torch.zeros(3, 1, max(n), device=DEV)
    for i, w in enumerate(wavs):
        x[i, 0, :n[i]] = w

    def call(m):
        t = m.inference_tokenize(x, torch.tensor(n))
        d = m.inference_detokenize(t["codes"], t["codes_lengths"])
        return {"zq": t["zq"], "codes": t["codes"], "codes_lengths": t["codes_lengths"], "y": d["y"], "output_length": d["output_length"]}
    run3(tag, precision, call)


@pytest.mark.parametrize("tag,precision", [("tiny", "fp32"), ("tiny", "mixed")])
def test_forward(tag, precision):
    g = torch.Generator().manual_seed(3)
    mel = (torch.rand(3, 80, 200, generator=g) * 0.8 + 0.2).to(DEV)
    lens = torch.tensor([200, 121, 40], device=DEV)
    run3(tag, precision, lambda m: m.forward({"mel_features": mel, "mel_lens": lens}))


def test_bitstream_pack_unpack():
    from simwhisper_codec_amd import bitstream
    g = torch.Generator().manual_seed(4)
    for T in (1, 7, 1000):
        codes = torch.randint(0, 2016, (8, T), generator=g, dtype=torch.int32).to(DEV)

        def call(m):
            payload = bitstream.pack_codes(codes)
            return {"payload": payload, "codes": bitstream.unpack_codes(payload, T)}
        out = run3("tiny", "fp32", call)
        assert torch.equal(out["codes"], codes)


# ------------------------------------------------------------------------------------------------------ the serving loop
def test_two_batches_in_flight_and_host_staging():
    """pipeline.InFlight (two batches on two streams, replicas with their own scratch) and pipeline.HostStager (pinned
    staging buffers, one copy per batch): README's "bit-identical output" under recycled-memory conditions"""
    from simwhisper_codec_amd import pipeline
    batches = [[w.cpu() for w in _wavs([3.0, 3.0], 100 + 10 * k, 0)] for k in range(4)]

    def call(m):
        stager = pipeline.HostStager()

        def one(model, cpu_wavs):
            dev = stager.to_device(cpu_wavs, torch.device(DEV))
            codes = model.encode(dev)["codes_list"]
            wav = model.decode(codes)["syn_wav_list"]
            return codes, pipeline.HostStager.to_host(pipeline.HostStager.pcm16_on_device(wav))
        with pipeline.InFlight(m, depth=2) as fl:
            return fl.map(one, batches)
    out = run3("tiny", "mixed", call)
    serial = _model("tiny", "mixed", None)
    for (codes, _), b in zip(out, batches):
        want = serial.encode([w.to(DEV) for w in b])["codes_list"]
        assert all(torch.equal(a, c) for a, c in zip(codes, want))
