"""swc_codes_pack_batch / swc_codes_unpack_batch on the GPU (include/swc_codes.h) and the layers above them: file images
against bitstream.write_codes' files AND the numpy oracle (oracle/bitstream_np.py) byte for byte, independence of the batch
around an utterance, the memory contract in the manner of tests/test_resample_gpu.py, the validation counter,
AudioCodec.encode_bytes / decode_bytes, HostStager's code staging and the CLI's encode / decode modes.
All pointers, offsets and lengths handed to the kernels are valid: nothing here provokes a fault."""
import os
import shutil
import struct

import numpy as np
import pytest
import torch

import poison
from common import PARAMS, state_dict
from test_codefile_cpu import oracle_image, random_codes

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


def _speech(n, index):
    from simwhisper_codec_amd import synth
    return synth.synth_audio(n, index=index, kind="speech")


# ragged on purpose: 0 and 1 are there, nothing is a multiple of the 256-frame tile, of 4 or of 11
LENS = {1: [[0], [1], [613]], 5: [[257, 0, 1, 127, 302]], 33: [[(37 * i * i + 101 * i + 3) % 611 for i in range(31)] + [0, 1]]}
CASES = [(B, lens) for B, group in LENS.items() for lens in group]


def _rows(codes_np, layout):
    """the utterances on the device: "i32" / "i64" contiguous tensors of their own; "i32s" / "i64s" strided views (8, T) of ONE
    padded (8, B, L) buffer that starts one element into its allocation (int32 rows are then 4-byte aligned ONLY)"""
    dt = torch.int32 if layout.startswith("i32") else torch.int64
    if not layout.endswith("s"):
        return [torch.from_numpy(c).to(dt).to(DEV) for c in codes_np]
    B, L = len(codes_np), max(max(c.shape[1] for c in codes_np), 1) + 5
    flat = torch.full((8 * B * L + 1,), 2047, dtype=dt, device=DEV)      # (what surrounds the rows is a valid, wrong code)
    buf = flat[1:].view(8, B, L)
    rows = []
    for b, c in enumerate(codes_np):
        buf[:, b, :c.shape[1]] = torch.from_numpy(c).to(dt).to(DEV)
        rows.append(buf[:, b, :c.shape[1]])
    if dt == torch.int32 and rows[0].numel():
        assert rows[0].data_ptr() % 16 == 4
    return rows


def _images(packed):
    buf, offsets, sizes = packed
    host = buf.cpu().numpy().tobytes()
    return [host[o:o + s] for o, s in zip(offsets, sizes)]


@pytest.mark.parametrize("layout", ["i32", "i64", "i32s", "i64s"])
@pytest.mark.parametrize("B,lens", CASES)
def test_pack_and_unpack_ragged_batches(B, lens, layout, tmp_path):
    from oracle import bitstream_np
    from simwhisper_codec_amd import bitstream
    codes_np = [random_codes(T, 1000 * B + i) for i, T in enumerate(lens)]
    rows = _rows(codes_np, layout)
    buf, offsets, sizes = bitstream.pack_batch(rows)
    assert buf.dtype == torch.uint8 and buf.is_cuda and sizes == [12 + 11 * T for T in lens]
    assert offsets == [sum(sizes[:b]) for b in range(B)] and buf.numel() == sum(sizes)      # back to back: a concatenation
    images = _images((buf, offsets, sizes))
    for b, (img, c) in enumerate(zip(images, codes_np)):
        assert img == oracle_image(c), (b, lens[b])                      # the header + the oracle's payload
        path = str(tmp_path / f"{b}.swc")
        bitstream.write_codes(path, rows[b])
        assert img == open(path, "rb").read(), (b, lens[b])              # the file of the per-utterance path
    # ... and back: one launch over the payloads inside that very buffer
    codes, views = bitstream.unpack_batch(buf, [o + 12 for o in offsets], lens)
    L = max(max(lens), 1)
    assert codes.shape == (8, B, L) and codes.dtype == torch.int32
    got = codes.cpu().numpy()
    for b, (T, img) in enumerate(zip(lens, images)):
        want = bitstream_np.unpack(np.frombuffer(img[12:], dtype=np.uint8), T)
        assert np.array_equal(want, codes_np[b])
        assert np.array_equal(got[:, b, :T], want) and not got[:, b, T:].any(), (b, T)
        assert views[b].shape == (8, T) and torch.equal(views[b], codes[:, b, :T])
    wide, _ = bitstream.unpack_batch(buf, [o + 12 for o in offsets], lens, L=L + 300)
    assert torch.equal(wide[:, :, :L], codes) and not wide[:, :, L:].any()


def test_strided_views_of_a_real_encode_call(tmp_path):
    """encode() hands out int32 views of one padded buffer: they are packed as they are"""
    from simwhisper_codec_amd import bitstream
    m = model("tiny", "mixed")
    wavs = [_speech(n, 10 + i).to(DEV) for i, n in enumerate([16000 * 3 + 77, 1500, 16000 * 2 - 5, 1280, 41000])]
    codes = m.encode(wavs)["codes_list"]
    assert [c.shape[-1] for c in codes] == [w.numel() // 1280 for w in wavs]
    assert any(c.numel() and not c.is_contiguous() for c in codes) and all(c.dtype == torch.int32 for c in codes if c.numel())
    images = _images(bitstream.pack_batch(codes))
    for b, (img, c) in enumerate(zip(images, codes)):
        assert img == oracle_image(c.cpu().numpy()), b
        bitstream.write_codes(str(tmp_path / "one.swc"), c)
        assert img == open(str(tmp_path / "one.swc"), "rb").read(), b
    assert images == _images(bitstream.pack_batch([c.long() for c in codes]))               # what decode() also accepts


def test_bits_do_not_depend_on_the_batch_around_an_utterance():
    """B, the row order and the offsets change nothing of an image; B, the order, the payload offsets and L nothing of a row"""
    from simwhisper_codec_amd import bitstream
    x = random_codes(389, 5)
    others = [random_codes(T, 50 + T) for T in (17, 0, 600, 1)]
    alone = _images(bitstream.pack_batch(_rows([x], "i32")))[0]
    assert alone == oracle_image(x)
    for pos in range(5):
        batch = others[:pos] + [x] + others[pos:]
        rows = _rows(batch, "i32s" if pos % 2 else "i64")
        assert _images(bitstream.pack_batch(rows))[pos] == alone, pos
        # images at odd places with holes between them, in another order than the rows
        sizes = [12 + 11 * c.shape[1] for c in batch]
        offsets, at = [0] * len(batch), 3 + pos
        for b in reversed(range(len(batch))):
            offsets[b] = at
            at += sizes[b] + 1 + (b + pos) % 7
        out = torch.zeros(at + 9, dtype=torch.uint8, device=DEV)
        packed = bitstream.pack_batch(rows, offsets=offsets, out=out)
        assert packed[0] is out and packed[1] == offsets and _images(packed)[pos] == alone, pos
        # unpack from that scattered buffer
        codes, views = bitstream.unpack_batch(out, [o + 12 for o in offsets], [c.shape[1] for c in batch], L=700 + pos)
        assert np.array_equal(views[pos].cpu().numpy(), x) and not codes[:, pos, 389:].any(), pos
    with pytest.raises(Exception, match="overlap"):
        bitstream.pack_batch(_rows([x, x], "i32"), offsets=[0, 100])
    with pytest.raises(Exception, match="overlap or leave"):
        bitstream.pack_batch(_rows([x], "i32"), offsets=[8], out=torch.zeros(12 + 11 * 389 + 7, dtype=torch.uint8, device=DEV))


FILLS = {"zero": 0x00, "poison": poison.U8_POISON, "ones": 0xFF}


def test_memory_contract_pack():
    """the output is a poison.guarded window whose images sit at odd offsets with holes between them, a hole in front of the
    first and slack behind the last; whatever the window held before, the images are the same bytes, the holes keep what they
    held and the bands keep the sentinel; the code rows are strided views whose surroundings hold other codes, and are unchanged"""
    from simwhisper_codec_amd import bitstream
    lens = [300, 0, 1, 257, 64]
    codes_np = [random_codes(T, 70 + i) for i, T in enumerate(lens)]
    sizes = [12 + 11 * T for T in lens]
    offsets, at = [], 5
    for b, s in enumerate(sizes):
        offsets.append(at)
        at += s + (0 if b == 2 else 1 + 2 * b)          # (images 2 and 3 touch: they share a dword)
    width = at + 37
    want = [oracle_image(c) for c in codes_np]
    for layout in ("i32s", "i64s"):
        rows = _rows(codes_np, layout)
        base = rows[0]._base
        snap = base.clone()
        for fill, byte in FILLS.items():
            view, check = poison.guarded((1, width), torch.uint8, ld=width + 19, device=DEV)
            view.fill_(byte)
            out = view[0]
            packed = bitstream.pack_batch(rows, offsets=offsets, out=out)
            torch.cuda.synchronize()
            check()                                                        # the bands and the ld padding keep the sentinel
            assert _images(packed) == want, (layout, fill)
            mask = torch.ones(width, dtype=torch.bool)
            for o, s in zip(offsets, sizes):
                mask[o:o + s] = False
            assert mask.sum() > 37 and (out.cpu()[mask] == byte).all(), (layout, fill, "a store outside the images")
            assert poison.same_bits(base, snap), "a read-only input changed"
    for pattern in poison.PATTERNS:                                        # no result depends on uninitialised memory
        with poison.poisoned_empty(pattern) as spy:
            again = _images(bitstream.pack_batch(_rows(codes_np, "i32")))
        assert spy.device_calls > 0 and again == want, pattern


def test_memory_contract_unpack():
    """the output is a poison.guarded (8, B, L) window with slack behind every row (ldb > L); a second variant adds slack between
    the groups (ldg > B ldb) inside a plain buffer.  Whatever the window held and whatever surrounds the payloads in the byte
    buffer, the rows are the same bits: codes, then zeros up to L; slack and bands keep what they held; the bytes are unchanged"""
    from simwhisper_codec_amd import bitstream
    lens = [300, 0, 1, 257, 64]
    B, L, ld = len(lens), 300 + 21, 300 + 21 + 13
    codes_np = [random_codes(T, 90 + i) for i, T in enumerate(lens)]
    res = []
    for fill, byte in FILLS.items():
        offs, at = [], 7
        for b, c in enumerate(codes_np):
            offs.append(at)
            at += 11 * lens[b] + 1 + b
        src = torch.full((at + 11,), byte, dtype=torch.uint8, device=DEV)   # what is not a payload is the fill
        for o, c in zip(offs, codes_np):
            src[o:o + 11 * c.shape[1]] = torch.from_numpy(np.frombuffer(oracle_image(c)[12:], dtype=np.uint8).copy()).to(DEV)
        snap = src.clone()
        view, check = poison.guarded((8, B, L), torch.int32, ld=ld, device=DEV)
        view.fill_({"zero": 0, "poison": poison.INT_POISON, "ones": -1}[fill])
        codes, views = bitstream.unpack_batch(src, offs, lens, out=view)
        torch.cuda.synchronize()
        assert codes is view
        check()
        assert poison.same_bits(src, snap), "a read-only input changed"
        got = view.cpu().numpy()
        for b, (T, c) in enumerate(zip(lens, codes_np)):
            assert np.array_equal(got[:, b, :T], c) and not got[:, b, T:].any(), (fill, b)
        # second variant: a plain buffer, group stride with slack; everything around the window holds the fill
        plain = torch.full((8 * (B + 2) * ld + ld,), -7 if fill == "ones" else byte, dtype=torch.int32, device=DEV)
        before = plain.clone()
        win = plain.as_strided((8, B, L), ((B + 2) * ld, ld, 1), ld)
        bitstream.unpack_batch(src, offs, lens, out=win)
        torch.cuda.synchronize()
        assert poison.same_bits(win.contiguous(), view.contiguous())
        mask = torch.ones_like(plain, dtype=torch.bool)
        mask.as_strided((8, B, L), ((B + 2) * ld, ld, 1), ld).fill_(False)
        assert poison.same_bits(plain[mask], before[mask]), "a store outside the window"
        res.append(view.contiguous().clone())
    assert all(poison.same_bits(res[0], r) for r in res[1:])
    for pattern in poison.PATTERNS:
        with poison.poisoned_empty(pattern) as spy:
            again, _ = bitstream.unpack_batch(src, offs, lens, L=L)
        assert spy.device_calls > 0 and poison.same_bits(again, res[0]), pattern


def _planted(T, seed, where):
    """codes of T frames with the values 2016 .. 2047 (11 bits, no entry of the shipped codebook) at the cells `where`"""
    c = random_codes(T, seed)
    for k, (g, t) in enumerate(where):
        c[g, t] = 2016 + (k * 5) % 32
    return c


def test_the_counter_counts_exactly_the_values_outside_the_codebook():
    from simwhisper_codec_amd import bitstream
    where = [(0, 0), (7, 0), (3, 299), (7, 299), (5, 255), (5, 256), (2, 17), (2, 18), (2, 19), (6, 100), (0, 101)]
    clean = [random_codes(T, 200 + T) for T in (300, 0, 77)]
    dirty = clean[:1] + [_planted(300, 9, where)] + clean[1:] + [_planted(5, 10, [(1, 4)])]
    for batch, want in ((clean, 0), (dirty, len(where) + 1)):
        buf, offsets, _ = bitstream.pack_batch(_rows(batch, "i32"))
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        codes, views = bitstream.unpack_batch(buf, [o + 12 for o in offsets], [c.shape[1] for c in batch], n_codes=2016, bad=bad)
        assert int(bad.item()) == want
        for v, c in zip(views, batch):
            assert np.array_equal(v.cpu().numpy(), c)                      # values pass through unchanged
        # the full 11-bit range counts nothing; a smaller codebook counts more
        bad.zero_()
        bitstream.unpack_batch(buf, [o + 12 for o in offsets], [c.shape[1] for c in batch], n_codes=2048, bad=bad)
        assert int(bad.item()) == 0
        bad.zero_()
        bitstream.unpack_batch(buf, [o + 12 for o in offsets], [c.shape[1] for c in batch], n_codes=1000, bad=bad)
        assert int(bad.item()) == sum(int((c >= 1000).sum()) for c in batch)
    # every value 2016 .. 2047 once
    allbad = random_codes(40, 3)
    allbad[np.arange(32) % 8, np.arange(32)] = np.arange(2016, 2048)
    buf, offsets, _ = bitstream.pack_batch(_rows([allbad], "i64"))
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    bitstream.unpack_batch(buf, [12], [40], n_codes=2016, bad=bad)
    assert int(bad.item()) == 32


def test_decode_bytes_refuses_codes_outside_the_codebook(monkeypatch):
    m = model("tiny", "mixed")
    blobs = [oracle_image(random_codes(30, 1)), oracle_image(_planted(30, 2, [(4, 7)])), oracle_image(random_codes(0, 3)),
             oracle_image(_planted(9, 4, [(0, 0), (7, 8)]))]
    monkeypatch.setattr(m, "decode", lambda *a, **k: pytest.fail("the decoder ran"))
    from simwhisper_codec_amd._lib import SwcError
    with pytest.raises(SwcError, match=r"utterances \[1, 3\]"):
        m.decode_bytes(blobs)
    with pytest.raises(ValueError, match="blob 2"):                        # a header the host rejects names the blob
        m.decode_bytes([blobs[0], blobs[0], blobs[0][:-1]])
    monkeypatch.undo()
    out = m.decode_bytes([blobs[0], blobs[2]])["syn_wav_list"]
    assert [w.numel() for w in out] == [30 * 1280, 0]
    assert m.decode_bytes([])["syn_wav_list"] == [] and m.encode_bytes([]) == []


@pytest.mark.parametrize("precision", ["mixed", "fp32"])
def test_bytes_round_trip_equals_the_in_memory_round_trip(precision, tmp_path):
    """a ragged batch with a recording longer than 30 s (several windows) and one too short for a single code frame"""
    from simwhisper_codec_amd import bitstream
    m = model("tiny", precision)
    lens = [16000 * 33 + 501, 16000 * 2 + 9, 700, 16000 * 5 - 3, 1280]
    wavs = [_speech(n, 20 + i).to(DEV) for i, n in enumerate(lens)]
    codes = m.encode(wavs)["codes_list"]
    want = m.decode(codes)["syn_wav_list"]
    blobs = m.encode_bytes(wavs)
    assert all(isinstance(b, bytes) for b in blobs) and [len(b) for b in blobs] == [12 + 11 * (n // 1280) for n in lens]
    for b, (blob, c) in enumerate(zip(blobs, codes)):
        assert blob == oracle_image(c.cpu().numpy()), b
        bitstream.write_codes(str(tmp_path / "x.swc"), c)
        assert blob == open(str(tmp_path / "x.swc"), "rb").read(), b
    got = m.decode_bytes(blobs)["syn_wav_list"]
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert poison.same_bits(g, w), b
    for pattern in poison.PATTERNS:
        with poison.poisoned_empty(pattern) as spy:
            again = m.decode_bytes(m.encode_bytes(wavs[1:]))["syn_wav_list"]
        ref = m.decode(m.encode(wavs[1:])["codes_list"])["syn_wav_list"]
        assert spy.device_calls > 0 and all(poison.same_bits(a, r) for a, r in zip(again, ref)), pattern
    # encode_bytes hands sample_rate on to encode()
    at24 = [_speech(24000 * 2 + 11, 41).to(DEV), _speech(30011, 42).to(DEV)]
    c24 = m.encode(at24, sample_rate=24000)["codes_list"]
    assert m.encode_bytes(at24, sample_rate=24000) == [oracle_image(c.cpu().numpy()) for c in c24]


def test_batched_file_io_equals_the_per_utterance_functions(tmp_path):
    from simwhisper_codec_amd import bitstream
    from simwhisper_codec_amd.pipeline import HostStager
    lens = [125, 0, 1, 333, 250, 77]
    codes_np = [random_codes(T, 300 + i) for i, T in enumerate(lens)]
    rows = _rows(codes_np, "i32s")
    one, many = tmp_path / "one", tmp_path / "many"
    one.mkdir(), many.mkdir()
    for b, r in enumerate(rows):
        bitstream.write_codes(str(one / f"{b}.swc"), r)
    paths = [str(many / f"{b}.swc") for b in range(len(rows))]
    bitstream.write_codes_batch(paths, rows)
    for b in range(len(rows)):
        assert open(paths[b], "rb").read() == open(str(one / f"{b}.swc"), "rb").read() == oracle_image(codes_np[b]), b
    back = bitstream.read_codes_batch(paths, DEV)
    for b, v in enumerate(back):
        assert v.dtype == torch.int32 and np.array_equal(v.cpu().numpy(), codes_np[b]), b
        assert not lens[b] or torch.equal(v, bitstream.read_codes(paths[b], DEV)), b
    assert [v.shape[1] for v in bitstream.read_codes_batch(paths, DEV, n_codes=2016)] == lens
    # a shard: the concatenation of the files is what pack_batch's buffer holds
    assert b"".join(open(p, "rb").read() for p in paths) == bitstream.pack_batch(rows)[0].cpu().numpy().tobytes()
    # a file of another model, and a file cut short, are named
    open(paths[3], "wb").write(oracle_image(_planted(333, 5, [(2, 200)])))
    with pytest.raises(ValueError, match="3.swc"):
        bitstream.read_codes_batch(paths, DEV, n_codes=2016)
    open(paths[4], "wb").write(oracle_image(codes_np[4])[:-1])
    with pytest.raises(ValueError, match="4.swc.*truncated"):
        bitstream.read_codes_batch(paths, DEV)
    # HostStager: the same images and codes, through its per-thread pinned buffer (re-used by the second call)
    st = HostStager()
    for _ in range(2):
        images = st.codes_to_host(rows)
        assert [bytes(i.numpy()) for i in images] == [oracle_image(c) for c in codes_np]
        assert all(i.dtype == torch.uint8 and not i.is_cuda for i in images)
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        codes, views = st.codes_to_device([bytes(i.numpy())[12:] for i in images], lens, torch.device(DEV), n_codes=2016, bad=bad)
        assert codes.shape == (8, len(lens), max(lens)) and int(bad.item()) == 0
        assert all(np.array_equal(v.cpu().numpy(), c) for v, c in zip(views, codes_np))


def _write_wav(path, pcm, sr=16000):
    raw = pcm.numpy().astype("<i2").tobytes()
    open(path, "wb").write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
                           struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16) + b"data" + struct.pack("<I", len(raw)) + raw)


def test_cli_encode_then_decode_writes_the_round_trip_files(tmp_path):
    import yaml
    import inference
    from simwhisper_codec_amd import bitstream
    cfg = tmp_path / "tiny.yaml"
    cfg.write_text(yaml.safe_dump({"generator_params": PARAMS["tiny"]()}))
    ind = tmp_path / "in"
    ind.mkdir()
    names = ["a", "b", "c", "d", "e"]
    pcms = []
    for i, (name, n) in enumerate(zip(names, [16000 * 2 + 123, 14000, 16000 * 3 - 7, 900, 16000 + 5])):   # "d": no code frame
        pcm = (_speech(n, 60 + i).clamp(-1, 1) * 32767).round().to(torch.int16)
        _write_wav(str(ind / f"{name}.wav"), pcm)
        pcms.append(pcm)
    common = ["--config_path", str(cfg), "--synthetic_checkpoint", "--device", "cuda", "--batch_size", "2", "--precision", "mixed"]
    rt, swc, swc1, dec = (tmp_path / d for d in ("rt", "swc", "swc1", "dec"))
    inference.main(common + ["--input_dir", str(ind), "--output_dir", str(rt)])                          # --mode roundtrip
    inference.main(common + ["--mode", "encode", "--input_dir", str(ind), "--output_dir", str(swc)])
    inference.main(common + ["--mode", "encode", "--in_flight", "1", "--input_dir", str(ind), "--output_dir", str(swc1)])
    inference.main(common + ["--mode", "decode", "--input_dir", str(swc), "--output_dir", str(dec)])
    assert sorted(os.listdir(swc)) == sorted(os.listdir(swc1)) == [f"{n}.swc" for n in names]
    assert sorted(os.listdir(dec)) == sorted(os.listdir(rt)) == [f"{n}.wav" for n in names]
    m = model("tiny", "mixed")
    for k in range(0, len(names), 2):                                      # the CLI's batches
        codes = m.encode([p.to(DEV).float() * (1.0 / 32768.0) for p in pcms[k:k + 2]])["codes_list"]
        for name, c, p in zip(names[k:k + 2], codes, pcms[k:k + 2]):
            bitstream.write_codes(str(tmp_path / "want.swc"), c)
            got = (swc / f"{name}.swc").read_bytes()
            assert got == (tmp_path / "want.swc").read_bytes() and len(got) == 12 + 11 * (p.numel() // 1280), name
            assert got == (swc1 / f"{name}.swc").read_bytes(), name       # --in_flight 1 and 2: identical files
    for name in names:
        assert (dec / f"{name}.wav").read_bytes() == (rt / f"{name}.wav").read_bytes(), name
    # a truncated file stops the run with its name; nothing is written for its batch
    cut, out2 = tmp_path / "cut", tmp_path / "out2"
    shutil.copytree(swc, cut)
    (cut / "c.swc").write_bytes((swc / "c.swc").read_bytes()[:-1])
    with pytest.raises(ValueError, match=r"c\.swc.*truncated"):
        inference.main(common + ["--mode", "decode", "--input_dir", str(cut), "--output_dir", str(out2)])
    assert not (out2 / "c.wav").exists() and not (out2 / "d.wav").exists()
    (cut / "c.swc").write_bytes(oracle_image(_planted(20, 6, [(3, 3)])))   # codes no model of this config produced
    with pytest.raises(ValueError, match=r"c\.swc.*codebook"):
        inference.main(common + ["--mode", "decode", "--input_dir", str(cut), "--output_dir", str(tmp_path / "out3")])
    assert not (tmp_path / "out3" / "c.wav").exists()
