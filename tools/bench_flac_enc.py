#!/usr/bin/env python3
"""FLAC output, measured: what a batch of 32 x 10 s of 16 kHz mono costs on its way from int16 samples on the device to files, as
PCM16 WAV (the only output of every earlier version) and as FLAC compressed on the GPU (`--output_format flac`:
swc_flac_encode_batch, include/swc_flac_enc.h), one box, one run.  Two signals: (a) what the model with the synthetic
checkpoint decodes, (b) the speech-like synth_audio signal at amplitude 20000.

  (1) bytes        the .flac images against PCM16; for information, the same samples through the LPC-8 numpy writer of
                   tools/bench_flac.py (the shape of libFLAC's default output)
  (2) the kernels  swc_flac_encode_batch alone between device events, with and without the MD5 kernel, alternating
  (3) to files     pcm16_on_device -> to_host -> save_pcm16     against     pcm16_on_device -> flac_to_host -> write, 8 writer
                   threads as in inference.py, alternating, into a temporary directory
  (4) files to files: inference.py --mode decode with --output_format wav / flac (and flac --flac_md5 none), alternating

Every .flac written in (3) is decoded by the host decoder (CRC-8, CRC-16, MD5) and compared with the samples before anything
is timed.  Reported: median (min - p90).  Needs the GPU.

usage: python tools/bench_flac_enc.py [--repeats 20] [--warmup 3] [--files N | --window 1.0] [--passes 4] [--out profiles/flac_enc_bench.txt]
"""
import argparse
import logging
import os
import re
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import bench_flac as bf  # noqa: E402  (spread, ordered, the LPC-8 numpy writer)

B, SECONDS, RATE, THREADS = 32, 10, 16000, 8
say = bf.say


def model_output(dev):
    """(generator, its decoded waveforms of B synthetic utterances): f32 device rows of one padded buffer"""
    import inference
    from simwhisper_codec_amd import synth
    args = inference.build_parser().parse_args(["--config_path", os.path.join(ROOT, "config", "SimWhisperCodec.yaml"),
                                                "--synthetic_checkpoint", "--device", "cuda"])
    gen = inference.load_model(args, dev)
    wavs = [synth.synth_audio(SECONDS * gen.input_sample_rate, index=i % 8, kind="speech").to(dev) for i in range(B)]
    with torch.no_grad():
        codes = gen.encode(wavs, overlap_seconds=10, device=dev)["codes_list"]
        syn = gen.decode(codes, overlap_seconds=10, device=dev)["syn_wav_list"]
    torch.cuda.synchronize()
    return gen, syn


def speech_rows(dev):
    from simwhisper_codec_amd import synth
    buf = torch.zeros(B, SECONDS * RATE, dtype=torch.float32, device=dev)
    for i in range(B):
        buf[i].copy_(synth.synth_audio(SECONDS * RATE, index=i % 8, kind="speech") * (20000.0 / 32767.0))
    return [buf[i] for i in range(B)]


def sizes(name, rows16, tmp):
    from simwhisper_codec_amd import ops
    out = {}
    for md5 in (True, False):
        _, _, sz = ops.flac_encode(rows16, RATE, md5=md5)
        out[md5] = int(sz.sum())
    pcm = sum(2 * r.numel() + 44 for r in rows16)
    assert out[True] == out[False]
    say(f"(1) {name}: {B} files, PCM16 WAV {pcm / 1e6:.2f} MB, FLAC (fixed predictors, block size 4096) {out[True] / 1e6:.2f} MB = "
        f"{out[True] / pcm:.3f} of PCM16")
    lpc = 0
    for i in range(4):   # for information: 4 of the utterances through the LPC-8 writer
        p = os.path.join(tmp, "lpc.flac")
        bf.write_flac(p, rows16[i].cpu().numpy().astype(np.int64).reshape(-1, 1), RATE)
        lpc += os.path.getsize(p)
    _, _, sz = ops.flac_encode(rows16[:4], RATE)
    say(f"    for information, 4 of them: LPC-8 numpy writer {lpc / 1e6:.2f} MB, this encoder {int(sz.sum()) / 1e6:.2f} MB "
        f"({int(sz.sum()) / lpc:.3f} of LPC-8)")


def kernels(name, rows16, args):
    from simwhisper_codec_amd import ops
    n = max(r.numel() for r in rows16)
    ws, cap = ops.flac_encode_workspace_layout([n] * B, 4096)
    out = torch.empty(cap, dtype=torch.uint8, device=rows16[0].device)
    work = torch.empty(ws, dtype=torch.uint8, device=rows16[0].device)
    times = {True: [], False: []}
    for rep in range(args.warmup + args.repeats):
        for md5 in (True, False):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            ops.flac_encode(rows16, RATE, md5=md5, out=out, workspace=work)   # (the row table's small copy is inside)
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                times[md5].append(e0.elapsed_time(e1))
    say(f"(2) {name}: swc_flac_encode_batch, {B} x {n} samples, device events:  with MD5 {bf.spread(times[True])}   without "
        f"{bf.spread(times[False])}")


def to_files(name, syn, tmp, args):
    from simwhisper_codec_amd import wavio
    from simwhisper_codec_amd.pipeline import HostStager
    stager = HostStager()
    io = ThreadPoolExecutor(max_workers=THREADS)
    d = os.path.join(tmp, "to_files")
    os.makedirs(d, exist_ok=True)

    def wav():
        host = stager.to_host(stager.pcm16_on_device(syn))
        list(io.map(lambda it: wavio.save_pcm16(os.path.join(d, f"{it[0]}.wav"), it[1], sample_rate=RATE), enumerate(host)))

    def write(it):
        with open(os.path.join(d, f"{it[0]}.flac"), "wb") as f:
            f.write(it[1].numpy())

    def flac(md5=True):
        images = stager.flac_to_host(stager.pcm16_on_device(syn), RATE, md5=md5)
        list(io.map(write, enumerate(images)))

    wav()
    flac()
    for i in range(len(syn)):   # what was written decodes to what the WAV holds (both CRCs and the MD5 checked)
        got, sr, bits = wavio._decode_flac(os.path.join(d, f"{i}.flac"))
        assert sr == RATE and bits == 16 and np.array_equal(got.reshape(-1), wavio.read_pcm(os.path.join(d, f"{i}.wav"))[0].numpy().reshape(-1))
    paths = {"wav": wav, "flac": flac, "flac, no MD5": lambda: flac(False)}
    times = {k: [] for k in paths}
    for rep in range(args.warmup + args.repeats):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            if rep >= args.warmup:
                times[k].append((time.perf_counter() - t) * 1e3)
    say(f"(3) {name}: f32 rows on the device -> {B} files written ({THREADS} writer threads), host clock:")
    for k in paths:
        say(f"    {k:13s} {bf.spread(times[k])}")
    for k in ("flac", "flac, no MD5"):
        o = bf.ordered(times[k], times["wav"])
        say(f"    {k} against wav: " + ("faster (medians ordered, spreads do not touch)" if o == "first" else
                                        "SLOWER (medians ordered, spreads do not touch)" if o == "second" else
                                        "no difference claimed: the spreads touch"))
    io.shutdown()


def cli(tmp, n_files, args):
    import inference
    from simwhisper_codec_amd import synth, wavio

    class Grab(logging.Handler):
        last = None

        def emit(self, rec):
            m = re.search(r"([0-9.]+) s of audio in ([0-9.]+) s", rec.getMessage())
            if m:
                Grab.last = (float(m.group(1)), float(m.group(2)))
    inference.set_logging = lambda *a, **k: None
    logging.getLogger().handlers = [Grab()]
    logging.getLogger().setLevel(logging.INFO)
    common = ["--config_path", os.path.join(ROOT, "config", "SimWhisperCodec.yaml"), "--synthetic_checkpoint", "--device", "cuda",
              "--batch_size", str(B)]
    wavs, codes, src = os.path.join(tmp, "cli_wav"), os.path.join(tmp, "cli_swc"), os.path.join(tmp, "cli_in")
    os.makedirs(wavs)
    for i in range(8):
        x = synth.synth_audio(SECONDS * RATE, index=i, kind="speech")
        wavio.save_pcm16(os.path.join(wavs, f"utt_{i}.wav"), torch.round(torch.clamp(x, -1, 1) * 20000).to(torch.int16), sample_rate=RATE)
    inference.main(common + ["--mode", "encode", "--input_dir", wavs, "--output_dir", codes])
    firsts = sorted(os.listdir(codes))

    def fill(n):
        shutil.rmtree(src, ignore_errors=True)
        os.makedirs(src)
        for i in range(n):
            shutil.copyfile(os.path.join(codes, firsts[i % len(firsts)]), os.path.join(src, f"utt_{i:05d}.swc"))
    outd = os.path.join(tmp, "cli_out")
    if n_files < 0:   # size the window from a first pass: the loop should last about args.window seconds
        fill(8 * B)
        for _ in range(2):
            shutil.rmtree(outd, ignore_errors=True)
            inference.main(common + ["--mode", "decode", "--input_dir", src, "--output_dir", outd])
        audio, loop = Grab.last
        n_files = min(4096, max(8 * B, int(args.window * audio / max(loop, 1e-3) / SECONDS / B + 1) * B))
        say(f"(4) window: a probe of {8 * B} files ran --mode decode at {audio / max(loop, 1e-3):.0f} audio-s/s -> {n_files} files for a "
            f"loop of about {args.window:g} s")
    fill(n_files)
    say(f"(4) inference.py --mode decode, files to files: {n_files} x {SECONDS} s code files, --batch_size {B}, defaults otherwise; the "
        "three outputs alternate, pass 0 warms up")
    variants = {"wav": ["--output_format", "wav"], "flac": ["--output_format", "flac"],
                "flac, no MD5": ["--output_format", "flac", "--flac_md5", "none"]}
    rates, nbytes = {k: [] for k in variants}, {}
    for rep in range(args.passes + 1):
        for k, flags in variants.items():
            shutil.rmtree(outd, ignore_errors=True)
            inference.main(common + ["--mode", "decode", "--input_dir", src, "--output_dir", outd] + flags)
            audio, loop = Grab.last
            nbytes[k] = sum(os.path.getsize(os.path.join(outd, f)) for f in os.listdir(outd))
            say(f"  --output_format {k:13s} pass {rep}: {audio:7.0f} s of audio, file loop {loop:6.2f} s = {audio / loop:8.1f} audio-s/s")
            if rep:
                rates[k].append(audio / loop)
    for k in variants:
        say(f"  {k:13s} audio-s/s {bf.spread(rates[k], '')}   {nbytes[k] / 1e6:8.2f} MB written")
    for k in ("flac", "flac, no MD5"):
        o = bf.ordered([-r for r in rates[k]], [-r for r in rates["wav"]])
        say(f"  {k} against wav: " + ("faster (medians ordered, spreads do not touch)" if o == "first" else
                                      "SLOWER (medians ordered, spreads do not touch)" if o == "second" else
                                      "no difference claimed: the spreads touch"))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--files", type=int, default=-1, help="code files of the CLI runs of (4); 0 skips (4); default: sized by a first "
                    "pass so that a loop lasts about --window seconds (at most 4096)")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--passes", type=int, default=4, help="timed passes per output format in (4)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "flac_enc_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flac_enc: needs the GPU (nothing here can be measured without one)")
    from simwhisper_codec_amd.pipeline import HostStager
    dev = torch.device("cuda", torch.cuda.current_device())
    say(f"FLAC output of {B} x {SECONDS} s at {RATE} Hz mono, {torch.cuda.get_device_name(0)}; reported: median (min - p90)")
    say()
    tmp = tempfile.mkdtemp(prefix="swc_flac_enc_", dir=os.environ.get("SWC_CLI_TMP", "/tmp"))
    try:
        with torch.cuda.device(dev):
            gen, syn = model_output(dev)
            assert gen.output_sample_rate == RATE
            for name, rows in (("(a) synthetic checkpoint's output", syn), ("(b) synth_audio speech", speech_rows(dev))):
                rows16 = [r.reshape(-1) for r in HostStager.pcm16_on_device(rows)]
                torch.cuda.synchronize()
                sizes(name, rows16, tmp)
                kernels(name, rows16, args)
                to_files(name, rows, tmp, args)
                say()
            del gen, syn
            if args.files:
                cli(tmp, args.files, args)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(bf.LINES) + "\n")


if __name__ == "__main__":
    main()
