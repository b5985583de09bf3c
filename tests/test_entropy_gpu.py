"""SWC2 on the device (include/swc_entropy.h, csrc/swc_entropy.hip) against the plain-Python restatement tests/entropy_ref.py,
bit for bit: the images of ragged batches in every layout, the three modes, invalid values, independence of the batch, decode of
the reference's images and of corrupt streams, the memory both calls may touch, and the layers above (AudioCodec, the CLI)."""
import functools
import os
import struct

import numpy as np
import pytest
import torch

import entropy_ref as ref
import poison
from common import PARAMS, state_dict
from test_entropy_cpu import SHIPPED, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("uniform", "geometric", "sticky", "constant")
LENGTHS = (0, 1, 2, 63, 64, 65, 129, 400, 1500)     # around the 64-frame chunk; 400 / 1500: both halving branches


def rows_of(kind, T, levels, G, seed):
    return np.array([stream(kind, T, levels, 100 * seed + g) for g in range(G)], dtype=np.int64).reshape(G, T)


@functools.lru_cache(maxsize=None)
def image_of(kind, T, levels, G, seed):
    """(codes [G, T], the reference's image, its modes): computed once, shared, never written"""
    c = rows_of(kind, T, levels, G, seed)
    c.setflags(write=False)
    image, modes, bad = ref.encode_image([list(map(int, r)) for r in c], levels)
    assert bad == 0
    return c, image, tuple(modes)


def on_device(codes_np, layout):
    """"i32" / "i64": contiguous tensors of their own; "i32s" / "i64s": strided views (G, T) of ONE padded (G, B, L) buffer that
    starts one element into its allocation (int32 rows are then 4-byte aligned only), the padding poisoned"""
    dt = torch.int32 if layout.startswith("i32") else torch.int64
    if not layout.endswith("s"):
        return [torch.from_numpy(np.array(c)).to(dt).to(DEV) for c in codes_np]
    G, B, L = codes_np[0].shape[0], len(codes_np), max(max(c.shape[1] for c in codes_np), 1) + 5
    raw = torch.full((G * B * L + 1,), poison.INT_POISON, dtype=dt, device=DEV)
    buf = raw[1:].view(G, B, L)
    for b, c in enumerate(codes_np):
        buf[:, b, :c.shape[1]] = torch.from_numpy(np.array(c)).to(dt).to(DEV)
    return [buf[:, b, :c.shape[1]] for b, c in enumerate(codes_np)]


def gpu_images(rows, levels, **kw):
    from simwhisper_codec_amd import bitstream
    buf, off, sizes, bad = bitstream.compress_batch(rows, levels, **kw)
    host, off, sizes = bytes(buf.cpu().numpy()), off.cpu().tolist(), sizes.cpu().tolist()
    pos = 0
    for o, s in zip(off, sizes):            # row order, no gaps
        assert o == pos
        pos += s
    return [host[o:o + s] for o, s in zip(off, sizes)], int(bad.item())


def same_images(got, want):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g == w, (b, len(g), len(w), next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), None))


# ---- encode ----

@pytest.mark.parametrize("layout", ["i32", "i64", "i32s", "i64s"])
@pytest.mark.parametrize("levels,G", [(SHIPPED, 8), ((2, 2, 2, 2), 3), ((16, 16, 8, 8), 1), ((16, 16, 16, 4), 3)])
def test_images_of_every_length_bit_for_bit(levels, G, layout):
    cases = [image_of(KINDS[(i + k) % 3], T, levels, G, k) for i, T in enumerate(LENGTHS) for k in range(2 if T in (129, 400) else 1)]
    got, bad = gpu_images(on_device([c for c, _, _ in cases], layout), levels)
    same_images(got, [im for _, im, _ in cases])
    assert bad == 0
    modes = {m for _, _, ms in cases for m in ms}
    assert modes == {0, 1, 2}, modes                       # (the reference's modes: the batch reaches all three)
    for (c, im, ms), g in zip(cases, got):                   # and the table of the device's image says the same
        assert tuple(struct.unpack_from("<I", g, 24 + 4 * k)[0] >> 24 for k in range(G)) == ms


@pytest.mark.parametrize("B", [1, 3, 33])
def test_batches_with_empty_rows(B):
    lengths = [(0, 37, 5, 64, 0, 125, 1, 66)[b % 8] for b in range(B)] if B > 1 else [37]
    cases = [image_of(KINDS[b % 4], T, SHIPPED, 8, b % 5) for b, T in enumerate(lengths)]
    for layout in ("i32", "i64s"):
        got, bad = gpu_images(on_device([c for c, _, _ in cases], layout), SHIPPED)
        same_images(got, [im for _, im, _ in cases])
        assert bad == 0
    if B == 3:      # nothing but empty rows: headers and tables alone
        got, bad = gpu_images([torch.zeros(8, 0, dtype=torch.int32, device=DEV)] * 2, SHIPPED)
        same_images(got, [ref.encode_image([[]] * 8, SHIPPED)[0]] * 2)


def _golden_codes():
    out = []
    for name in ("chunked", "ragged", "short", "single", "zeros"):
        z = np.load(os.path.join(ROOT, "tests", "golden", f"real_{name}.npz"))
        out += [z[k].astype(np.int64) for k in sorted(z.files) if k.startswith("codes_")]
    return out


def test_golden_codes():
    codes = _golden_codes()
    assert len(codes) == 10 and codes[0].shape == (8, 275)
    want = [ref.encode_image([list(map(int, r)) for r in c], SHIPPED)[0] for c in codes]
    got, bad = gpu_images(on_device(codes, "i32"), SHIPPED)
    same_images(got, want)
    assert bad == 0 and len(got[0]) < 12 + 11 * 275        # (smaller than its SWC1 file; synthetic weights, not speech)
    back = _decode(want, SHIPPED)
    for c, b in zip(codes, back):
        assert np.array_equal(c, b)


@pytest.mark.parametrize("layout", ["i32", "i64"])
def test_invalid_values_are_written_raw_and_counted(layout):
    c0 = rows_of("sticky", 70, SHIPPED, 8, 1)
    c1 = rows_of("sticky", 70, SHIPPED, 8, 2)
    c0[2, 0], c0[2, 69], c0[5, 64] = -1, 2016, 2047
    c1[7, 33] = -5
    if layout == "i64":
        c1[0, 3] = (1 << 32) + 17           # a set high word over a valid low word
        c1[0, 4] = -(1 << 40)
    else:
        c1[0, 3] = 1 << 30
    n_bad = 6 if layout == "i64" else 5
    want = [ref.encode_image([list(map(int, r)) for r in c], SHIPPED) for c in (c0, c1)]
    assert sum(w[2] for w in want) == n_bad
    assert want[0][1][2] == want[0][1][5] == want[1][1][7] == want[1][1][0] == 0 and 2 in want[0][1]
    got, bad = gpu_images(on_device([c0, c1], layout), SHIPPED)
    same_images(got, [w[0] for w in want])
    assert bad == sum(w[2] for w in want)


def test_an_image_depends_on_its_own_row_only():
    cases = [image_of("sticky", 129, SHIPPED, 8, 0), image_of("geometric", 400, SHIPPED, 8, 1), image_of("uniform", 65, SHIPPED, 8, 0)]
    rows = on_device([c for c, _, _ in cases], "i32")
    batch, _ = gpu_images(rows, SHIPPED)
    for k in range(3):
        alone, _ = gpu_images([rows[k]], SHIPPED)                       # B and max_frames differ
        assert alone[0] == batch[k] == cases[k][1]
    swapped, _ = gpu_images(rows[::-1], SHIPPED)                        # the order in the batch
    assert swapped == batch[::-1]


# ---- decode ----

def _decode(images, levels, L=None, out=None, n_codes=None):
    """images (host bytes) -> numpy codes per image through decompress_batch: the tables come from the REFERENCE's parser without
    its CRC check, so corrupt streams reach the kernel"""
    from simwhisper_codec_amd import bitstream
    blob, tables, n, pos = b"", [], [], 0
    for im in images:
        T, G, lv, table = ref.parse_image(im, check_crc=False)
        tables.append([(m, pos + o, k) for m, o, k in table])
        n.append(T)
        blob += bytes(im)
        pos += len(im)
    buf = torch.frombuffer(bytearray(blob + b"\0"), dtype=torch.uint8).to(DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV) if n_codes is not None else None
    codes, views = bitstream.decompress_batch(buf, tables, n, levels, n_codes=n_codes, bad=bad, L=L, out=out)
    res = [v.cpu().numpy().astype(np.int64) for v in views]
    return (res, codes, int(bad.item())) if n_codes is not None else res


@pytest.mark.parametrize("levels,G", [(SHIPPED, 8), ((2, 2, 2, 2), 3), ((16, 16, 8, 8), 1), ((16, 16, 16, 4), 3)])
def test_decode_of_the_reference_images(levels, G):
    cases = [image_of(KINDS[(i + 1) % 3], T, levels, G, 0) for i, T in enumerate(LENGTHS)]
    L = 1505
    got, codes, bad = _decode([im for _, im, _ in cases], levels, L=L, n_codes=ref.n_codes(levels))
    assert bad == 0 and tuple(codes.shape) == (G, len(cases), L)
    full = codes.cpu().numpy()
    for b, ((c, _, _), g) in enumerate(zip(cases, got)):
        assert np.array_equal(g, c), b
        assert not full[:, b, c.shape[1]:].any()                        # zero fill up to L


def test_decode_of_corrupt_streams_matches_the_reference_and_stays_valid():
    rng = np.random.default_rng(5)
    images = []
    for T, kind in ((129, "sticky"), (400, "geometric"), (65, "sticky"), (64, "uniform")):
        c, im, modes = image_of(kind, T, SHIPPED, 8, 3)
        b = bytearray(im)
        for _ in range(40):
            b[int(rng.integers(24 + 32, len(b)))] ^= int(rng.integers(1, 256))
        images.append(bytes(b))
    got, codes, bad = _decode(images, SHIPPED, n_codes=2016)
    want = [np.array(ref.decode_image(im, check_crc=False), dtype=np.int64) for im in images]
    n_raw_bad = 0
    for im, g, w in zip(images, got, want):
        assert np.array_equal(g, w)
        modes = [m for m, _, _ in ref.parse_image(im, check_crc=False)[3]]
        for k, m in enumerate(modes):
            if m:
                assert g[k].min() >= 0 and g[k].max() < 2016               # any bytes decode to valid codes
            else:
                n_raw_bad += int((g[k] >= 2016).sum())
    assert bad == n_raw_bad
    # a stream cut short: the missing bytes read as 0
    c, im, modes = image_of("sticky", 129, SHIPPED, 8, 3)
    from simwhisper_codec_amd import bitstream
    T, G, lv, table = ref.parse_image(im)
    cut = [(m, o, k // 2) for m, o, k in table]
    buf = torch.frombuffer(bytearray(im), dtype=torch.uint8).to(DEV)
    _, views = bitstream.decompress_batch(buf, [cut], [T], SHIPPED)
    for g, (m, o, k) in enumerate(cut):
        data = im[o:o + k]
        w = ref.decode_raw(data, T, SHIPPED) if m == 0 else ref.decode_adaptive(data, T, SHIPPED, m - 1)
        assert views[0][g].cpu().tolist() == w


# ---- memory ----

@pytest.mark.parametrize("fill", [0x00, 0xA5])
def test_encode_writes_the_images_and_nothing_else(fill):
    from simwhisper_codec_amd import bitstream
    cases = [image_of("sticky", 129, SHIPPED, 8, 0), image_of("uniform", 0, SHIPPED, 8, 0), image_of("geometric", 65, SHIPPED, 8, 1)]
    rows = on_device([c for c, _, _ in cases], "i32s")
    cap = 3 * bitstream.worst_bytes2(129, SHIPPED)
    (out, c0), (lay, c1) = poison.guarded((cap,), torch.uint8, device=DEV), poison.guarded((2, 3), torch.int64, device=DEV)
    out.fill_(fill)
    lay.fill_(fill)
    got, bad = gpu_images(rows, SHIPPED, out=out, layout=lay)
    c0()
    c1()
    same_images(got, [im for _, im, _ in cases])
    total = sum(len(g) for g in got)
    assert bool((out[total:] == fill).all())                             # nothing behind the last image


@pytest.mark.parametrize("fill", [0, poison.INT_POISON])
def test_decode_writes_every_row_up_to_L_and_nothing_else(fill):
    cases = [image_of("sticky", 129, SHIPPED, 8, 0), image_of("uniform", 0, SHIPPED, 8, 0), image_of("geometric", 65, SHIPPED, 8, 1)]
    L = 140
    out, check = poison.guarded((8, 3, L), torch.int32, ld=L + 7, device=DEV)
    out.fill_(fill)
    got = _decode([im for _, im, _ in cases], SHIPPED, out=out)
    check()
    full = out.cpu().numpy()
    for b, (c, _, _) in enumerate(cases):
        assert np.array_equal(got[b], c) and np.array_equal(full[:, b, :c.shape[1]], c) and not full[:, b, c.shape[1]:].any()


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


def test_audiocodec_bytes_round_trip_in_both_formats():
    from simwhisper_codec_amd._lib import SwcError
    m = model()
    wavs = [_speech(16000 * 3 + 211, 70).to(DEV), _speech(16000 * 2 - 77, 71).to(DEV), _speech(700, 72).to(DEV)]   # the last: no frame
    codes = m.encode(wavs)["codes_list"]
    want = m.decode(codes)["syn_wav_list"]
    two = m.encode_bytes(wavs, format="swc2")
    one = m.encode_bytes(wavs)
    assert one == m.encode_bytes(wavs, format="swc1") and all(b[:4] == b"SWC1" for b in one)
    for b, c in zip(two, codes):
        assert b == ref.encode_image([list(map(int, r)) for r in c.cpu().tolist()], SHIPPED)[0]
    for blobs in (two, [two[0], one[1], two[2]], [one[0], two[1], one[2]]):      # either kind, and a mix in one call
        got = m.decode_bytes(blobs)["syn_wav_list"]
        assert len(got) == 3
        for g, w in zip(got, want):
            assert poison.same_bits(g, w)
    flipped = bytearray(two[1])
    flipped[len(flipped) - 2] ^= 0x40
    with pytest.raises(ValueError, match=r"^blob 1: not a sound SWC2 code file \(CRC mismatch\)"):
        m.decode_bytes([two[0], bytes(flipped), one[2]])
    other = ref.encode_image([[1, 2, 3]] * 8, (8, 7, 6, 5))[0]
    with pytest.raises(ValueError, match=r"^blob 0: SWC2 codes of 8 groups with levels \[8, 7, 6, 5\]"):
        m.decode_bytes([other])
    with pytest.raises(SwcError, match="format 'zip'"):
        m.encode_bytes(wavs, format="zip")


def _write_wav(path, pcm, sr=16000):
    raw = pcm.numpy().astype("<i2").tobytes()
    open(path, "wb").write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
                           struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16) + b"data" + struct.pack("<I", len(raw)) + raw)


def test_cli_code_format_round_trip_and_mixed_directory(tmp_path):
    import yaml
    import inference
    from simwhisper_codec_amd import bitstream
    cfg = tmp_path / "tiny.yaml"
    cfg.write_text(yaml.safe_dump({"generator_params": PARAMS["tiny"]()}))
    ind = tmp_path / "in"
    ind.mkdir()
    names = ["a", "b", "c", "d", "e"]
    for i, (name, n) in enumerate(zip(names, [16000 * 2 + 123, 14000, 16000 * 3 - 7, 900, 16000 + 5])):   # "d": no code frame
        _write_wav(str(ind / f"{name}.wav"), (_speech(n, 60 + i).clamp(-1, 1) * 32767).round().to(torch.int16))
    common = ["--config_path", str(cfg), "--synthetic_checkpoint", "--device", "cuda", "--batch_size", "2", "--precision", "mixed"]
    rt, one, two, mixed = (tmp_path / d for d in ("rt", "one", "two", "mixed"))
    inference.main(common + ["--input_dir", str(ind), "--output_dir", str(rt)])
    inference.main(common + ["--mode", "encode", "--input_dir", str(ind), "--output_dir", str(one)])
    inference.main(common + ["--mode", "encode", "--code_format", "swc2", "--input_dir", str(ind), "--output_dir", str(two)])
    assert sorted(os.listdir(two)) == [f"{n}.swc" for n in names]
    codes = bitstream.read_codes_batch([str(one / f"{n}.swc") for n in names], device=DEV, n_codes=2016)
    for n, c in zip(names, codes):
        image = (two / f"{n}.swc").read_bytes()
        assert image == ref.encode_image([list(map(int, r)) for r in c.cpu().tolist()], SHIPPED)[0], n
    mixed.mkdir()
    for k, n in enumerate(names):
        (mixed / f"{n}.swc").write_bytes(((two if k % 2 else one) / f"{n}.swc").read_bytes())
    for src, dst in ((two, tmp_path / "wav2"), (mixed, tmp_path / "wavm")):
        inference.main(common + ["--mode", "decode", "--input_dir", str(src), "--output_dir", str(dst)])
        for n in names:
            assert (dst / f"{n}.wav").read_bytes() == (rt / f"{n}.wav").read_bytes(), (src, n)
    got = bitstream.read_codes_batch([str(mixed / f"{n}.swc") for n in names], device=DEV, n_codes=2016, levels=SHIPPED)
    for g, c in zip(got, codes):
        assert torch.equal(g, c)
    bitstream.write_codes_batch([str(tmp_path / "w1.swc"), str(tmp_path / "w2.swc")], codes[:2])
    bitstream.write_codes_batch([str(tmp_path / "x1.swc"), str(tmp_path / "x2.swc")], codes[:2], format="swc2", levels=SHIPPED)
    assert (tmp_path / "w1.swc").read_bytes() == (one / "a.swc").read_bytes() and (tmp_path / "x2.swc").read_bytes() == (two / "b.swc").read_bytes()
    # the tool reads both kinds: the same usage, and what each directory takes on disk beside the bits its codes carry
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_codes
    res = {}
    for tag, d in (("one", one), ("two", two), ("mixed", mixed)):
        evaluate_codes.main([str(d), "--json", str(tmp_path / f"{tag}.json")])
        res[tag] = json.loads((tmp_path / f"{tag}.json").read_text())
        assert res[tag]["bytes_on_disk"] == sum(os.path.getsize(d / f"{n}.swc") for n in names)
    for k in ("used", "frames", "entropy_bits", "bits_per_frame", "bad"):
        assert res["one"][k] == res["two"][k] == res["mixed"][k], k
    frames = res["one"]["frames"]
    assert res["one"]["bytes_on_disk"] == 12 * 5 + 11 * frames and res["one"]["containers"] == {"SWC1": 5}
    assert res["two"]["containers"] == {"SWC2": 5} and res["mixed"]["containers"] == {"SWC1": 3, "SWC2": 2}
    assert res["two"]["disk_bits_per_frame"] == 8.0 * res["two"]["bytes_on_disk"] / frames
    assert res["two"]["disk_bps"] == pytest.approx(res["two"]["disk_bits_per_frame"] * 12.5, rel=1e-12)   # (the rate: a quotient)
    bad = bytearray((two / "c.swc").read_bytes())
    bad[-1] ^= 1
    (mixed / "c.swc").write_bytes(bytes(bad))
    with pytest.raises(ValueError, match=r"c\.swc: not a sound SWC2 code file \(CRC mismatch\)"):
        inference.main(common + ["--mode", "decode", "--input_dir", str(mixed), "--output_dir", str(tmp_path / "never")])
    assert not (tmp_path / "never" / "c.wav").exists()
