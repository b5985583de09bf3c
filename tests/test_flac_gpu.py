"""swc_flac_decode_batch on the GPU (include/swc_flac.h, csrc/swc_flac_gpu.hip) and the layers above it: int16 output against the
host decoder (csrc/swc_flac.c) bit for bit over batches of 1 / 5 / 33 files, independence of the batch around a file and of
the alignment of its bytes, the memory contract in the manner of tests/test_codefile_gpu.py, the status words against the host
build of the same frame decoder, HostStager.to_device_flac against the host staging paths and `inference.py --flac gpu`
against `--flac host`.
Every offset, length and table entry handed to the kernels is valid, and the damaged streams are a fixed dozen that the
sanitizer program (tests/test_flac_frame_cpu.py) decodes without a report: nothing here provokes a fault."""
import ctypes as C
import functools
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_encode as fe  # noqa: E402
import flac_streams as fs  # noqa: E402
import poison  # noqa: E402
from common import PARAMS  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def host_decode(raw):
    """csrc/swc_flac.c on the bytes -> (int32 [n, ch], channels, bits)"""
    from simwhisper_codec_amd import wavio
    lib = wavio._io()
    sr, ch, bits, total = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    assert lib.swc_flac_info(raw, len(raw), C.byref(sr), C.byref(ch), C.byref(bits), C.byref(total)) == 0
    out = np.empty((max(int(total.value), 1), ch.value), dtype=np.int32)
    md5 = C.c_int32()
    n = lib.swc_flac_decode(raw, len(raw), out.ctypes.data_as(C.c_void_p), int(total.value), C.byref(md5))
    assert n == total.value, n
    return out[:n], ch.value, bits.value


@functools.lru_cache(maxsize=None)
def pool():
    """the streams of every test here, encoded once: -> {name: (stream bytes, expected int16 [n * ch] = the host decoder's samples
    shifted up to 16 bits)}.  Frames per file 0, 1, 2, 65 (block size 16: more frames than one wave has lanes), 37 and 13;
    block sizes 16 .. 4096; 1 and 2 channels; 8, 12 and 16 bits; every stereo mode; every subframe kind (the matrix)."""
    streams = {name: raw for name, x, sr, bps, raw, tab in fs.matrix()}
    modes = fs.MODES
    streams["empty"] = fe.encode(np.zeros((0, 1), dtype=np.int64), 16000, 16, blocksize=1024)
    streams["one"] = fe.encode(fs.signal(100, 1, 16, 40), 16000, 16, blocksize=1024)
    streams["two4096"] = fe.encode(fs.signal(4096 + 904, 1, 16, 41), 16000, 16, blocksize=4096,
                                   plan=lambda fi, c: 0 if c is None else dict(kind=("lpc", 8), porder=3))
    streams["w65"] = fe.encode(fs.signal(65 * 16, 2, 8, 42), 48000, 8, blocksize=16,
                               plan=lambda fi, c: modes[fi % 4] if c is None else dict(kind=[("fixed", 1), ("lpc", 2), "verbatim"][fi % 3], porder=fi % 2))
    streams["odd37"] = fe.encode(fs.signal(37 * 192 - 5, 2, 12, 43), 44100, 12, blocksize=192,
                                 plan=lambda fi, c: modes[(fi + 1) % 4] if c is None else dict(kind=[("lpc", 12), ("fixed", 3)][fi % 2], porder=fi % 4, rice2=fi % 3 == 0))
    streams["two1024s"] = fe.encode(fs.signal(1024 + 1, 2, 16, 44), 16000, 16, blocksize=1024,
                                    plan=lambda fi, c: 10 if c is None else dict(kind=("lpc", 32), porder=2))
    out = {}
    for name, raw in streams.items():
        pcm, ch, bits = host_decode(raw)
        out[name] = (raw, (pcm.astype(np.int64) << (16 - bits)).astype(np.int16).reshape(-1))
    return out


def tables(raws, out_gap=0, byte_gap=0, byte_lead=0, out_lead=0):
    """the batch as swc_flac_decode_batch takes it -> dict(data uint8 array, frames, files (structured), spans [(out offset,
    elements)], out_elems, ws_bytes, frame ranges).  Gaps and leads (elements / bytes) put holes between and in front of the
    files' spans and bytes."""
    from simwhisper_codec_amd import _lib, ops, wavio
    fdt, idt = np.dtype(_lib.FlacFrame), np.dtype(_lib.FlacFile)
    idx = [wavio.flac_index(r) for r in raws]
    assert not any(isinstance(g, int) for g in idx), idx
    plane_off, ws_bytes = ops.flac_workspace_bytes([g[0].total for g in idx], [g[0].channels for g in idx])
    frames = np.zeros(sum(len(g[1]) for g in idx), dtype=fdt)
    files = np.zeros(len(raws), dtype=idt)
    data = bytearray(byte_lead)
    spans, ranges, at, f0 = [], [], out_lead, 0
    for i, (raw, (info, fr)) in enumerate(zip(raws, idx)):
        base = len(data)
        data += raw + bytes(byte_gap)
        frames[f0:f0 + len(fr)] = fr
        frames["byte_off"][f0:f0 + len(fr)] += base
        frames["file"][f0:f0 + len(fr)] = i
        files[i] = (at, info.total, plane_off[i], f0, len(fr), info.channels, info.bps, info.blocksize, 0)
        spans.append((at, info.total * info.channels))
        ranges.append((f0, f0 + len(fr)))
        at += info.total * info.channels + out_gap
        f0 += len(fr)
    return dict(data=np.frombuffer(bytes(data), dtype=np.uint8), frames=frames, files=files, spans=spans, out_elems=at,
                ws_bytes=ws_bytes, ranges=ranges)


def run(t, out=None, status=None, workspace=None, data=None, fpw=0):
    from simwhisper_codec_amd import ops
    n_frames = len(t["frames"])
    data = torch.from_numpy(t["data"].copy()).to(DEV) if data is None else data
    frames = torch.from_numpy(t["frames"].view(np.uint8).copy()).to(DEV) if n_frames else torch.zeros(8, dtype=torch.uint8, device=DEV)[:0]
    files = torch.from_numpy(t["files"].view(np.uint8).copy()).to(DEV)
    out = torch.full((max(t["out_elems"], 1),), 0x5A5A, dtype=torch.int16, device=DEV) if out is None else out
    status = torch.full((max(n_frames, 1),), 77, dtype=torch.int32, device=DEV) if status is None else status
    workspace = torch.empty(max(t["ws_bytes"], 16), dtype=torch.uint8, device=DEV) if workspace is None else workspace
    ops.flac_decode(data, frames, files, out, status, workspace, n_frames=n_frames, B=len(t["files"]), frames_per_wave=fpw)
    torch.cuda.synchronize()
    return out, status


def check_batch(names, **kw):
    p = pool()
    t = tables([p[n][0] for n in names], **{k: v for k, v in kw.items() if k != "fpw"})
    out, status = run(t, fpw=kw.get("fpw", 0))
    got, st = out.cpu().numpy(), status.cpu().numpy()
    assert not st[: len(t["frames"])].any(), st
    mask = np.ones(len(got), dtype=bool)
    for n, (o, e) in zip(names, t["spans"]):
        assert np.array_equal(got[o:o + e], p[n][1]), n
        mask[o:o + e] = False
    assert (got[mask] == 0x5A5A).all(), "a store outside the files' spans"
    return t


ORDER = ["kinds_c1_b16", "w65", "empty", "odd37", "one", "kinds_c2_b8", "two4096", "kinds_c2_b12", "porders", "kinds_c1_b8",
         "two1024s", "stereo_modes", "kinds_c1_b12", "kinds_c2_b16"]


@pytest.mark.parametrize("B", [1, 5, 33])
def test_batches_equal_the_host_decoder(B):
    """B = 1: every stream of the pool alone (0, 1, 2, 13, 17, 19, 37 and 65 frames; block sizes 16, 192, 256, 1024, 4096; 1 / 2
    channels; 8 / 12 / 16 bits; every subframe kind and stereo mode).  B = 5 and 33: mixed batches with gaps between the
    files' output spans and their bytes, the empty file among them.  int16 output == the host decoder's samples << (16 - bits)."""
    assert set(ORDER) == set(pool())
    if B == 1:
        for n in ORDER:
            check_batch([n])
        return
    names = ["w65", "empty", "odd37", "two4096", "kinds_c2_b12"] if B == 5 else [ORDER[i % len(ORDER)] for i in range(B)]
    assert len(names) == B and "empty" in names and "w65" in names
    t = check_batch(names, out_gap=3, byte_gap=1, byte_lead=1, out_lead=5)
    assert len(t["frames"]) > 64
    for fpw in (1, 8, 64):           # the frame kernel's mapping changes nothing
        check_batch(names, out_gap=3, byte_gap=1, byte_lead=1, out_lead=5, fpw=fpw)


def test_a_file_gives_the_same_bits_alone_in_a_batch_and_at_any_byte_offset():
    p = pool()
    for name in ("kinds_c2_b12", "w65"):
        raw, want = p[name]
        t = tables([raw])
        alone = run(t)[0].cpu().numpy()[: len(want)]
        assert np.array_equal(alone, want)
        t3 = check_batch(["odd37", name, "two4096"], out_gap=1)     # row 2 of 3
        o, e = t3["spans"][1]
        assert e == len(want)
        for shift in range(4):                                      # the file's bytes 0 .. 3 bytes behind a 16-byte boundary
            ts = tables([raw], byte_lead=16 + shift)
            buf = torch.zeros(len(ts["data"]) + 64, dtype=torch.uint8, device=DEV)
            assert buf.data_ptr() % 16 == 0
            buf[: len(ts["data"])] = torch.from_numpy(ts["data"].copy()).to(DEV)
            got = run(ts, data=buf[: len(ts["data"])])[0].cpu().numpy()[: len(want)]
            assert np.array_equal(got, want), (name, shift)


FILLS = {"zero": (0, 0x00), "poison": (poison.I16_POISON, poison.U8_POISON), "ones": (-1, 0xFF)}


def test_memory_contract():
    """output, status and workspace are poison.guarded windows: the files' spans sit at odd element offsets with holes between
    them, a hole in front and slack behind; whatever the windows held before, the spans get the same samples, the holes keep
    what they held, the status window gets one word per frame and nothing behind them, the workspace is written inside the
    files' planes only and the bands keep the sentinel.  The inputs are unchanged."""
    from simwhisper_codec_amd import ops
    p = pool()
    names = ["w65", "empty", "kinds_c1_b12", "two1024s", "one"]
    t = tables([p[n][0] for n in names], out_gap=3, out_lead=7, byte_gap=2, byte_lead=3)
    n_frames, width = len(t["frames"]), t["out_elems"] + 41
    plane_off, ws_bytes = ops.flac_workspace_layout([int(f["n_samples"]) for f in t["files"]], [int(f["channels"]) for f in t["files"]])
    assert ws_bytes == t["ws_bytes"]
    data = torch.from_numpy(t["data"].copy()).to(DEV)
    snap = data.clone()
    for fill, (word, byte) in FILLS.items():
        out_v, out_check = poison.guarded((1, width), torch.int16, ld=width + 19, device=DEV)
        st_v, st_check = poison.guarded((1, n_frames + 9), torch.int32, ld=n_frames + 12, device=DEV)
        ws_v, ws_check = poison.guarded((1, ws_bytes + 64), torch.uint8, ld=ws_bytes + 128, band_rows=4, device=DEV)
        out_v.fill_(word); st_v.fill_(word); ws_v.fill_(byte)
        assert ws_v.data_ptr() % 16 == 0
        out, status = run(t, out=out_v[0], status=st_v[0], workspace=ws_v[0], data=data)
        out_check(); st_check(); ws_check()
        got, st = out.cpu().numpy(), status.cpu().numpy()
        assert not st[:n_frames].any() and (st[n_frames:] == word).all(), fill
        mask = np.ones(width, dtype=bool)
        for n, (o, e) in zip(names, t["spans"]):
            assert np.array_equal(got[o:o + e], p[n][1]), (fill, n)
            mask[o:o + e] = False
        assert mask.sum() > 41 and (got[mask] == np.int16(word)).all(), (fill, "a store outside the files' spans")
        ws = ws_v[0].cpu().numpy()
        wmask = np.ones(len(ws), dtype=bool)
        for f, po in zip(t["files"], plane_off):
            wmask[4 * po: 4 * (po + int(f["n_samples"]) * int(f["channels"]))] = False
        assert wmask.sum() >= 64 and (ws[wmask] == byte).all(), (fill, "a store outside the planes")
        assert poison.same_bits(data, snap)
    for pattern in poison.PATTERNS:                                   # no result depends on uninitialised memory
        with poison.poisoned_empty(pattern) as spy:
            out, status = run(t)
        assert spy.device_calls > 0
        got = out.cpu().numpy()
        for n, (o, e) in zip(names, t["spans"]):
            assert np.array_equal(got[o:o + e], p[n][1]), (pattern, n)


def test_table_entries_outside_a_buffer_are_dropped_with_a_status():
    """entries that point outside `bytes`, the output, the workspace or their file are never read through: their frames get
    SWC_FLAC_ST_ENTRY, their file writes nothing, the other files of the batch decode as ever.  (Every such entry is refused
    by the kernels' own checks: no access is made with it.)"""
    p = pool()
    names = ["kinds_c1_b16", "one", "w65", "two1024s"]
    base = tables([p[n][0] for n in names], out_gap=2)
    cases = []
    for what in ("byte_off", "n_bytes", "file", "first_sample", "out_off", "plane_off", "neg"):
        t = dict(base, frames=base["frames"].copy(), files=base["files"].copy())
        f1 = t["ranges"][1][0]                                        # the one frame of file 1
        if what == "byte_off":
            t["frames"]["byte_off"][f1] = len(t["data"]) - 3
        elif what == "n_bytes":
            t["frames"]["n_bytes"][f1] = 1 << 30
        elif what == "file":
            t["frames"]["file"][f1] = 7
        elif what == "first_sample":
            t["frames"]["first_sample"][f1] = 1 << 40
        elif what == "out_off":
            t["files"]["out_off"][1] = t["out_elems"] - 5
        elif what == "plane_off":
            t["files"]["plane_off"][1] = t["ws_bytes"] // 4 - 5
        else:
            t["frames"]["byte_off"][f1] = -1
        cases.append((what, t, f1))
    for what, t, f1 in cases:
        out, status = run(t)
        got, st = out.cpu().numpy(), status.cpu().numpy()
        assert st[f1] == 1 and not np.delete(st[: len(t["frames"])], f1).any(), (what, st)
        mask = np.ones(len(got), dtype=bool)
        for k, (n, (o, e)) in enumerate(zip(names, base["spans"])):
            if k != 1:
                assert np.array_equal(got[o:o + e], p[n][1]), (what, n)
                mask[o:o + e] = False
        assert (got[mask] == 0x5A5A).all(), what


def test_status_words_equal_the_host_build(tmp_path):
    """a fixed dozen of the damaged set (all run under the sanitizers by tests/test_flac_frame_cpu.py), in one batch with two
    sound files: each frame's status equals what the host build of csrc/swc_flac_frame.h says; a file with a failed frame
    writes nothing, a damaged file whose frames all decode gives the host decoder's samples, the sound files are unaffected."""
    damaged = dict(fs.damaged_set())
    paths = []
    for name in fs.GPU_DAMAGED:
        q = tmp_path / f"{name}.flac"
        q.write_bytes(damaged[name])
        paths.append(str(q))
    rc, res, err = fs.run_check(paths, sanitize=False)
    assert rc == 0 and len(res) == 12, err
    p = pool()
    raws = [p["kinds_c2_b16"][0]] + [damaged[n] for n in fs.GPU_DAMAGED] + [p["one"][0]]
    t = tables(raws, out_gap=1)
    out, status = run(t)
    got, st = out.cpu().numpy(), status.cpu().numpy()
    mask = np.ones(len(got), dtype=bool)
    n_bad = 0
    for k, raw in enumerate(raws):
        a, b = t["ranges"][k]
        o, e = t["spans"][k]
        if k in (0, len(raws) - 1):
            want = p["kinds_c2_b16" if k == 0 else "one"][1]
            assert not st[a:b].any() and np.array_equal(got[o:o + e], want)
            mask[o:o + e] = False
            continue
        r = res[paths[k - 1]]
        assert list(st[a:b]) == r["status"], (fs.GPU_DAMAGED[k - 1], list(st[a:b]), r)
        if r["verdict"] == "equal":
            pcm, ch, bits = host_decode(raw)
            assert np.array_equal(got[o:o + e], (pcm.astype(np.int64) << (16 - bits)).astype(np.int16).reshape(-1))
            mask[o:o + e] = False
        else:
            n_bad += 1
    assert n_bad >= 8 and (got[mask] == 0x5A5A).all(), "a file with a failed frame must write nothing"


# ------------------------------------------------------------------------------------------------ the layers above
def _write_wav(path, pcm, sr, ch):
    raw = np.asarray(pcm, dtype="<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, ch, sr, sr * 2 * ch, 2 * ch, 16)
                + b"data" + struct.pack("<I", len(raw)) + raw)


def test_staging_equals_the_host_paths(tmp_path):
    import inference
    from simwhisper_codec_amd import wavio
    from simwhisper_codec_amd.pipeline import HostStager
    stager, dev = HostStager(), torch.device("cuda", torch.cuda.current_device())
    # mono, 16 kHz, 16 bit: load_audio + to_device, bit for bit (through load_file / stage_files, as the CLI goes)
    x = fs.signal(9000, 1, 16, 50)
    a = tmp_path / "a.flac"
    a.write_bytes(fe.encode(x, 16000, 16, blocksize=1152, plan=lambda fi, c: 0 if c is None else dict(kind=("lpc", 8), porder=2)))
    loaded = inference.load_file(str(a), 16000, True, "host", "gpu")
    assert isinstance(loaded, wavio.FlacRaw)
    got = inference.stage_files(stager, [loaded], dev, 16000)
    want = stager.to_device([wavio.load_audio(str(a), 16000).reshape(-1)], dev)
    torch.cuda.synchronize()
    assert poison.same_bits(got[0].cpu(), want[0].cpu()) and got[0].numel() == 9000
    assert not isinstance(inference.load_file(str(a), 16000, True, "host", "host"), wavio.FlacRaw)      # the default stays the host decoder
    assert not isinstance(inference.load_file(str(a), 16000, False, "host", "gpu"), wavio.FlacRaw)      # no device, no raw bytes
    # stereo, 48 kHz: to_device_pcm on the same samples written as a WAV, bit for bit; an 8-bit mono file rides along
    y = fs.signal(12000, 2, 16, 51)
    b = tmp_path / "b.flac"
    b.write_bytes(fe.encode(y, 48000, 16, blocksize=4096, plan=lambda fi, c: [10, 8, 9][fi % 3] if c is None else dict(kind=("fixed", 2), porder=1)))
    _write_wav(str(tmp_path / "b.wav"), y, 48000, 2)
    z = fs.signal(5000, 1, 8, 52)
    c8 = tmp_path / "c.flac"
    c8.write_bytes(fe.encode(z, 16000, 8, blocksize=576))
    raws = [wavio.read_flac_raw(str(q)) for q in (b, a, c8)]
    views, failed = stager.to_device_flac(raws, dev, 16000)
    torch.cuda.synchronize()
    assert failed() == []
    want_b = stager.to_device_pcm([wavio.read_pcm(str(tmp_path / "b.wav"))], dev, 16000)
    torch.cuda.synchronize()
    assert poison.same_bits(views[0].cpu(), want_b[0].cpu()) and views[0].numel() == 4000
    assert poison.same_bits(views[1].cpu(), want[0].cpu())
    assert poison.same_bits(views[2].cpu(), wavio.load_audio(str(c8), 16000).reshape(-1))               # 8 bits: sample * 2^-7
    for pattern in poison.PATTERNS:
        with poison.poisoned_empty(pattern):
            again, failed = stager.to_device_flac(raws, dev, 16000)
            torch.cuda.synchronize()
        assert failed() == [] and all(poison.same_bits(u.cpu(), v.cpu()) for u, v in zip(again, views)), pattern
    # a file whose frames pass the index but not the decoder: reported by failed(), its neighbours are sound
    bad = tmp_path / "bad.flac"
    bad.write_bytes(dict(fs.damaged_set())["m16_porder15"])
    views2, failed2 = stager.to_device_flac([raws[1], wavio.read_flac_raw(str(bad)), raws[2]], dev, 16000)
    torch.cuda.synchronize()
    assert failed2() == [1] and poison.same_bits(views2[0].cpu(), views[1].cpu()) and poison.same_bits(views2[2].cpu(), views[2].cpu())
    assert stager.to_device_flac([], dev, 16000)[0] == []


def test_cli_flac_gpu_writes_the_files_of_flac_host(tmp_path):
    import yaml
    import inference
    cfg = tmp_path / "tiny.yaml"
    cfg.write_text(yaml.safe_dump({"generator_params": PARAMS["tiny"]()}))
    ind = tmp_path / "in"
    ind.mkdir()
    names = ["a", "b", "c", "d", "e"]
    for i, (name, n) in enumerate(zip(names, [20000, 14000, 16000 + 5, 900, 7777])):
        x = fs.signal(n, 1, 16, 60 + i)
        (ind / f"{name}.flac").write_bytes(fe.encode(x, 16000, 16, blocksize=[4096, 1152, 4608, 256, 1024][i],
                                                     plan=lambda fi, c: 0 if c is None else dict(kind=("lpc", 8), porder=2)))
    common = ["--config_path", str(cfg), "--synthetic_checkpoint", "--device", "cuda", "--batch_size", "2", "--precision", "mixed"]
    out = {k: tmp_path / k for k in ("rt_host", "rt_gpu", "swc_host", "swc_gpu", "mixed", "bad", "bad2")}
    inference.main(common + ["--input_dir", str(ind), "--output_dir", str(out["rt_host"])])
    inference.main(common + ["--flac", "gpu", "--input_dir", str(ind), "--output_dir", str(out["rt_gpu"])])
    inference.main(common + ["--mode", "encode", "--input_dir", str(ind), "--output_dir", str(out["swc_host"])])
    inference.main(common + ["--mode", "encode", "--flac", "gpu", "--input_dir", str(ind), "--output_dir", str(out["swc_gpu"])])
    assert sorted(os.listdir(out["rt_gpu"])) == sorted(os.listdir(out["rt_host"])) == [f"{n}.wav" for n in names]
    assert sorted(os.listdir(out["swc_gpu"])) == sorted(os.listdir(out["swc_host"])) == [f"{n}.swc" for n in names]
    for n in names:
        assert (out["rt_gpu"] / f"{n}.wav").read_bytes() == (out["rt_host"] / f"{n}.wav").read_bytes(), n
        assert (out["swc_gpu"] / f"{n}.swc").read_bytes() == (out["swc_host"] / f"{n}.swc").read_bytes(), n
    # a batch that mixes a WAV, FLAC files, a 24-bit FLAC (host decoder) and a 48 kHz stereo FLAC runs
    mix = tmp_path / "mix"
    mix.mkdir()
    (mix / "a.flac").write_bytes((ind / "a.flac").read_bytes())
    _write_wav(str(mix / "b.wav"), fs.signal(15000, 1, 16, 70), 16000, 1)
    (mix / "c.flac").write_bytes(fe.encode(fs.signal(12000, 1, 24, 71), 16000, 24, blocksize=4096))
    (mix / "d.flac").write_bytes(fe.encode(fs.signal(18000, 2, 16, 72), 48000, 16, blocksize=4096))
    inference.main(common + ["--batch_size", "4", "--flac", "gpu", "--input_dir", str(mix), "--output_dir", str(out["mixed"])])
    assert sorted(os.listdir(out["mixed"])) == ["a.wav", "b.wav", "c.wav", "d.wav"]
    assert (out["mixed"] / "a.wav").stat().st_size > 44 and (out["mixed"] / "d.wav").stat().st_size > 44
    # a corrupt file is named in the error: one that fails the index (a CRC), one that passes it and fails on the device
    raw = bytearray((ind / "b.flac").read_bytes())
    raw[len(raw) // 2] ^= 0x10
    (mix / "c.flac").write_bytes(bytes(raw))
    with pytest.raises(ValueError, match=r"c\.flac.*CRC"):
        inference.main(common + ["--batch_size", "4", "--flac", "gpu", "--input_dir", str(mix), "--output_dir", str(out["bad"])])
    (mix / "c.flac").write_bytes(dict(fs.damaged_set())["m16_type_reserved"])
    with pytest.raises(ValueError, match=r"c\.flac"):
        inference.main(common + ["--batch_size", "4", "--flac", "gpu", "--input_dir", str(mix), "--output_dir", str(out["bad2"])])
