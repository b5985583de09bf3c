#!/usr/bin/env python3
"""FLAC input, measured: what a batch of 32 x 10 s FLAC files costs on its way to f32 audio on the device, by the host path
(`--flac host`, the behaviour of every earlier version: 8 loader threads run the C decoder, MD5, int -> f32, channel mean and
host resampling, then one f32 copy) and by the device path (`--flac gpu`: the loader threads only index the frames, the
compressed bytes cross PCIe, swc_flac_decode_batch decodes one frame per work item), one box, one run:

  (a) staging      load_file(flac="host") x 8 threads + stage_files     against     read_flac_raw x 8 threads + to_device_flac,
                   alternating in one loop, at 16 kHz mono and at 48 kHz stereo (both 16 bit)
  (b) the kernels  swc_flac_decode_batch alone on staged buffers (device events), for every mapping of the frame kernel
  (c) the loaders  seconds per file on one thread: swc_flac_index against the full host decode
  (d) files to files: inference.py --mode encode / roundtrip with --flac host and --flac gpu, alternating

The files are written once into a temporary directory (SWC_CLI_TMP or /tmp) by the numpy encoder below — no FLAC tool exists
offline: block size 4096, LPC order 8 with 12-bit coefficients (least squares per block), Rice partition order 3, left/side for
stereo, MD5 signature — the shape of libFLAC's default output; 8 distinct synthetic utterances, used cyclically.  The host
decoder verifies every file (CRCs, MD5) before anything is timed.  Reported: median (min - p90).  Needs the GPU.

usage: python tools/bench_flac.py [--repeats 20] [--warmup 3] [--files N | --window 1.0] [--passes 4] [--out profiles/flac_bench.txt]
"""
import argparse
import hashlib
import logging
import os
import re
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

B, SECONDS, THREADS = 32, 10, 8
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


# ------------------------------------------------------------------------------------------------ a numpy FLAC writer
def _crc_table(poly, bits):
    top, mask = 1 << (bits - 1), (1 << bits) - 1
    t = []
    for i in range(256):
        c = i << (bits - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        t.append(c)
    return t


CRC8, CRC16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def _crc8(data):
    c = 0
    for b in data:
        c = CRC8[c ^ b]
    return c


def _crc16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ CRC16[(c >> 8) ^ b]
    return c


def _bits_of(values, widths):
    """MSB-first bits of `values` (non-negative int64), widths[i] bits each -> uint8 array of 0 / 1"""
    total = int(widths.sum())
    out = np.zeros(total, dtype=np.uint8)
    start = np.cumsum(widths) - widths
    for j in range(int(widths.max()) if len(widths) else 0):
        m = widths > j
        out[start[m] + (widths[m] - 1 - j)] = (values[m] >> j) & 1
    return out


def _subframe_lpc(s, bps, order=8, prec=12, porder=3):
    """one LPC subframe of the int64 block s -> bit array"""
    bs = len(s)
    x = s.astype(np.float64)
    rows = np.stack([x[order - 1 - j:bs - 1 - j] for j in range(order)], axis=1)
    c, *_ = np.linalg.lstsq(rows, x[order:], rcond=None)
    m = max(float(np.abs(c).max()), 1e-9)
    shift = max(0, min(15, prec - 2 - int(np.ceil(np.log2(m + 1e-12)))))
    q = np.clip(np.round(c * (1 << shift)), -(1 << (prec - 1)), (1 << (prec - 1)) - 1).astype(np.int64)
    pred = np.zeros(bs - order, dtype=np.int64)
    for j in range(order):
        pred += q[j] * s[order - 1 - j:bs - 1 - j]
    res = s[order:] - (pred >> shift)
    head = _bits_of(np.array([0, 32 + order - 1, 0] + [int(v) & ((1 << bps) - 1) for v in s[:order]] + [prec - 1, shift]
                             + [int(v) & ((1 << prec) - 1) for v in q] + [0, porder], dtype=np.int64),
                    np.array([1, 6, 1] + [bps] * order + [4, 5] + [prec] * order + [2, 4], dtype=np.int64))
    parts, psize, pieces, idx = 1 << porder, bs >> porder, [head], 0
    u = np.where(res >= 0, res << 1, ((-res) << 1) - 1)
    for p in range(parts):
        cnt = psize - (order if p == 0 else 0)
        seg = u[idx:idx + cnt]
        idx += cnt
        k = max(0, min(14, int(np.log2(seg.mean() + 1)))) if cnt else 0
        quo = seg >> k
        widths = quo + 1 + k                                   # quo zeros, a one, k low bits: the value (1 << k) | low in quo + 1 + k bits
        pieces.append(_bits_of(np.array([k], dtype=np.int64), np.array([4], dtype=np.int64)))
        pieces.append(_bits_of((1 << k) | (seg & ((1 << k) - 1)), widths))
    return np.concatenate(pieces)


def write_flac(path, x, sr, bps=16, blocksize=4096):
    """x int64 [n, ch] (1 or 2 channels) -> a FLAC file: fixed block size, LPC order 8, left/side for stereo, MD5 signature"""
    n, ch = x.shape
    sig = hashlib.md5(x.astype("<i2").tobytes()).digest()
    si = (blocksize << 128) | (blocksize << 112) | (sr << 44) | ((ch - 1) << 41) | ((bps - 1) << 36) | n
    out = bytearray(b"fLaC" + bytes([0x80]) + (34).to_bytes(3, "big") + si.to_bytes(18, "big") + sig)
    codes = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
    sr_code = {8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10}[sr]
    for fi, start in enumerate(range(0, n, blocksize)):
        blk = x[start:start + blocksize]
        bs = len(blk)
        bcode = codes.get(bs, 7)
        hdr = bytes([0xFF, 0xF8, (bcode << 4) | sr_code, ((8 if ch == 2 else 0) << 4) | (4 << 1)])
        assert fi < (1 << 11)
        hdr += bytes([fi]) if fi < 0x80 else bytes([0xC0 | (fi >> 6), 0x80 | (fi & 0x3F)])
        if bcode == 7:
            hdr += (bs - 1).to_bytes(2, "big")
        hdr += bytes([_crc8(hdr)])
        po = 3 if bs % 8 == 0 and (bs >> 3) >= 8 else 0
        if ch == 1:
            bits = _subframe_lpc(blk[:, 0], bps, porder=po)
        else:
            bits = np.concatenate([_subframe_lpc(blk[:, 0], bps, porder=po), _subframe_lpc(blk[:, 0] - blk[:, 1], bps + 1, porder=po)])
        frame = hdr + np.packbits(bits).tobytes()
        out += frame + _crc16(frame).to_bytes(2, "big")
    with open(path, "wb") as f:
        f.write(bytes(out))


def make_files(tmp, sr, ch, distinct=8):
    """B files of SECONDS seconds at (sr, ch) -> their paths; `distinct` synthetic utterances, used cyclically"""
    from simwhisper_codec_amd import synth, wavio
    d = os.path.join(tmp, f"flac_{sr}_{ch}")
    os.makedirs(d)
    n = SECONDS * sr
    firsts = []
    for i in range(distinct):
        a = synth.synth_audio(n, index=i, kind="speech").numpy().astype(np.float64)
        cols = [a] if ch == 1 else [a, 0.7 * a + 0.3 * synth.synth_audio(n, index=100 + i, kind="speech").numpy().astype(np.float64)]
        x = np.clip(np.round(np.stack(cols, axis=1) * 20000.0), -32768, 32767).astype(np.int64)
        p = os.path.join(d, f"utt_{i:03d}.flac")
        write_flac(p, x, sr)
        pcm, got_sr, bits = wavio._decode_flac(p)           # the host decoder checks CRC-8, CRC-16 and MD5 of what was written
        assert got_sr == sr and bits == 16 and np.array_equal(pcm.astype(np.int64), x)
        firsts.append(p)
    paths = list(firsts)
    for i in range(distinct, B):
        p = os.path.join(d, f"utt_{i:03d}.flac")
        shutil.copyfile(firsts[i % distinct], p)
        paths.append(p)
    return paths


# ------------------------------------------------------------------------------------------------ measurements
def spread(v, unit="ms"):
    s = sorted(v)
    p90 = s[min(len(s) - 1, int(0.9 * len(s)))]
    return f"{statistics.median(s):9.3f} ({s[0]:.3f} - {p90:.3f}) {unit}"


def ordered(a, b):
    """are two samples ordered with spreads (min - p90) that do not touch?"""
    sa, sb = sorted(a), sorted(b)
    pa, pb = sa[min(len(sa) - 1, int(0.9 * len(sa)))], sb[min(len(sb) - 1, int(0.9 * len(sb)))]
    if statistics.median(sa) < statistics.median(sb) and pa < sb[0]:
        return "first"
    if statistics.median(sb) < statistics.median(sa) and pb < sa[0]:
        return "second"
    return None


def staging(paths, sr, ch, dev, args):
    import inference
    from simwhisper_codec_amd import wavio
    from simwhisper_codec_amd.pipeline import HostStager
    stager, io = HostStager(), ThreadPoolExecutor(max_workers=THREADS)
    audio = B * SECONDS

    def host():
        loaded = list(io.map(lambda p: inference.load_file(p, 16000, True, "host", "host"), paths))
        out = inference.stage_files(stager, loaded, dev, 16000)
        torch.cuda.synchronize()
        return out

    def device():
        raws = list(io.map(wavio.read_flac_raw, paths))
        out, failed = stager.to_device_flac(raws, dev, 16000)
        torch.cuda.synchronize()
        assert failed() == []
        return out

    a, b = host(), device()
    if sr == 16000 and ch == 1:
        assert all(torch.equal(u, v) for u, v in zip(a, b)), "the two paths staged different audio"
        same = "bit-identical"
    else:   # the host path resamples in f32 on the CPU, the device path in swc_resample: the sums run in different orders
        err = max(float((u - v).abs().max()) for u, v in zip(a, b))
        assert err < 1e-4, err
        same = f"equal within {err:.1e} (two resamplers, --resample host / gpu)"
    for _ in range(args.warmup):
        host(), device()
    th, td = [], []
    for _ in range(args.repeats):
        t = time.perf_counter(); host(); th.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter(); device(); td.append((time.perf_counter() - t) * 1e3)
    size = sum(os.path.getsize(p) for p in paths)
    say(f"(a) staging {B} x {SECONDS} s, {sr} Hz, {ch} ch, 16 bit ({size / 1e6:.2f} MB of FLAC, {B * SECONDS * sr * ch * 2 / 1e6:.2f} MB of PCM16); "
        f"results {same}; {args.repeats} alternating rounds after {args.warmup} warm-up rounds, files in the page cache")
    mh, md = statistics.median(th), statistics.median(td)
    say(f"  --flac host  {THREADS} threads load_file + stage_files     {spread(th)}   {audio / mh * 1e3:9.0f} audio-s/s")
    say(f"  --flac gpu   {THREADS} threads read_flac_raw + to_device_flac {spread(td)}   {audio / md * 1e3:9.0f} audio-s/s")
    o = ordered(td, th)
    say("  " + (f"the device path is {mh / md:.2f} x faster (medians ordered, spreads do not touch)" if o == "first" else
                f"THE DEVICE PATH IS {md / mh:.2f} x SLOWER (medians ordered, spreads do not touch)" if o == "second" else
                "no difference claimed: the spreads touch"))
    # (b) the kernels alone, per mapping of the frame kernel
    raws = [wavio.read_flac_raw(p) for p in paths]
    n_frames = sum(len(r.frames) for r in raws)
    say(f"(b) swc_flac_decode_batch alone, {n_frames} frames (a pair of device events around the call's two kernels, inside to_device_flac)")
    for fpw in (0, 1, 2, 4, 8, 16, 32, 64):
        ev = []
        for k in range(args.warmup + args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stager.to_device_flac(raws, dev, 16000, frames_per_wave=fpw, events=(e0, e1))
            torch.cuda.synchronize()
            if k >= args.warmup:
                ev.append(e0.elapsed_time(e1))
        say(f"  frames per wave {'auto' if fpw == 0 else fpw:>4}   {spread(ev)}   {audio / statistics.median(ev) * 1e3:10.0f} audio-s/s")
    # (c) one loader thread, per file
    ti, tf = [], []
    for p in paths:
        t = time.perf_counter(); wavio.read_flac_raw(p); ti.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter(); wavio.load_audio(p, 16000); tf.append((time.perf_counter() - t) * 1e3)
    say(f"(c) one loader thread, per file: read + index {spread(ti)}    read + full host decode to f32 at 16 kHz {spread(tf)}")
    say()
    io.shutdown()


def cli(tmp, paths, n_files, args):
    import inference

    def fill(d, n):
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
        for i in range(n):
            shutil.copyfile(paths[i % len(paths)], os.path.join(d, f"utt_{i:05d}.flac"))
    src = os.path.join(tmp, "cli_in")

    class Grab(logging.Handler):
        last, stages = None, None

        def emit(self, rec):
            m = re.search(r"([0-9.]+) s of audio in ([0-9.]+) s", rec.getMessage())
            if m:
                Grab.last = (float(m.group(1)), float(m.group(2)))
            m = re.search(r"load\+h2d ([0-9.]+)", rec.getMessage())
            if m:
                Grab.stages = float(m.group(1))
    inference.set_logging = lambda *a, **k: None
    logging.getLogger().handlers = [Grab()]
    logging.getLogger().setLevel(logging.INFO)
    common = ["--config_path", os.path.join(ROOT, "config", "SimWhisperCodec.yaml"), "--synthetic_checkpoint", "--device", "cuda",
              "--batch_size", str(B)]
    if n_files < 0:   # size the window from a first pass: the slower mode's loop should last about args.window seconds
        fill(src, 8 * B)
        outd = os.path.join(tmp, "out_probe")
        for _ in range(2):   # (the first call loads the library's code objects)
            shutil.rmtree(outd, ignore_errors=True)
            inference.main(common + ["--mode", "encode", "--flac", "host", "--input_dir", src, "--output_dir", outd])
        audio, loop = Grab.last
        n_files = min(4096, max(8 * B, int(args.window * audio / max(loop, 1e-3) / SECONDS / B + 1) * B))
        say(f"(d) window: a probe of {8 * B} files ran --mode encode at {audio / max(loop, 1e-3):.0f} audio-s/s -> {n_files} files for a loop of "
            f"about {args.window:g} s")
        shutil.rmtree(outd, ignore_errors=True)
    fill(src, n_files)
    say(f"(d) inference.py, files to files: {n_files} x {SECONDS} s FLAC files (16 kHz mono 16 bit), --batch_size {B}, defaults otherwise; "
        "host and gpu alternate, pass 0 warms up")
    for mode in ("encode", "roundtrip"):
        rates = {"host": [], "gpu": []}
        for rep in range(args.passes + 1):
            for flac in ("host", "gpu"):
                outd = os.path.join(tmp, f"out_{mode}_{flac}")
                shutil.rmtree(outd, ignore_errors=True)
                inference.main(common + ["--mode", mode, "--flac", flac, "--input_dir", src, "--output_dir", outd])
                audio, loop = Grab.last
                say(f"  --mode {mode:9s} --flac {flac:4s} pass {rep}: {audio:7.0f} s of audio, file loop {loop:6.2f} s = {audio / loop:8.1f} audio-s/s, "
                    f"load+h2d {Grab.stages:.2f} s ({100 * Grab.stages / loop:.0f} % of the loop)")
                if rep:
                    rates[flac].append(audio / loop)
        ext = ".swc" if mode == "encode" else ".wav"
        a, b = (os.path.join(tmp, f"out_{mode}_{f}") for f in ("host", "gpu"))
        same = all(open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read() for f in os.listdir(a))
        say(f"  --mode {mode}: {len(os.listdir(a))} {ext} files, byte-identical between the two paths: {same}")
        say(f"  --mode {mode}: audio-s/s  host {spread(rates['host'], '')}   gpu {spread(rates['gpu'], '')}")
        o = ordered([-r for r in rates["gpu"]], [-r for r in rates["host"]])
        say("  " + ("--flac gpu is faster (medians ordered, spreads do not touch)" if o == "first" else
                    "--flac gpu IS SLOWER (medians ordered, spreads do not touch)" if o == "second" else "no difference claimed: the spreads touch"))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--files", type=int, default=-1, help="files of the CLI runs of (d); 0 skips (d); default: sized by a first pass "
                    "so that a loop lasts about --window seconds (at most 4096)")
    ap.add_argument("--window", type=float, default=1.0, help="seconds a file loop of (d) should last when --files is not given")
    ap.add_argument("--passes", type=int, default=4, help="timed passes per mode and path in (d)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "flac_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flac: needs the GPU (nothing here can be measured without one)")
    dev = torch.device("cuda", torch.cuda.current_device())
    say(f"FLAC input of {B} x {SECONDS} s, {torch.cuda.get_device_name(0)}; reported: median (min - p90)")
    say()
    tmp = tempfile.mkdtemp(prefix="swc_flac_", dir=os.environ.get("SWC_CLI_TMP", "/tmp"))
    try:
        t = time.perf_counter()
        mono = make_files(tmp, 16000, 1)
        stereo = make_files(tmp, 48000, 2)
        say(f"files written and verified by the host decoder in {time.perf_counter() - t:.1f} s (numpy encoder: block size 4096, LPC order 8, "
            "Rice partition order 3, left/side for stereo)")
        say()
        staging(mono, 16000, 1, dev, args)
        staging(stereo, 48000, 2, dev, args)
        if args.files:
            cli(tmp, mono, args.files, args)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
