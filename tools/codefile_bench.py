#!/usr/bin/env python3
"""Code files, measured: what a batch of 32 x 10 s utterances costs on its way to and from SWC1 files (simwhisper_codec_amd/bitstream.py),
real config, synthetic weights, one box, one run:

  (a) the per-utterance loops   for c in codes: write_codes(path, c)      /  [read_codes(path) for path in paths]
      (one launch, one synchronising copy and one allocation per utterance: the baseline, unchanged by the batched path)
  (b) the batched calls         write_codes_batch(paths, codes)           /  read_codes_batch(paths)
      (one launch and one copy through pinned memory per batch)
  (c) inference.py files to files: --mode encode and --mode decode beside --mode roundtrip, in audio-seconds per second

(a) and (b) alternate inside one loop (same box, same minute, same page cache); every call is timed twice over the same span,
by the host clock between two device synchronisations and by a pair of device events, after `--warmup` untimed rounds; medians
and the spread (min, 10th / 90th percentile, max) of `--repeats` rounds are printed.  The files live in a temporary directory
(SWC_CLI_TMP or /tmp).  Needs the GPU: there is no CPU fallback and no number without one.

usage: python tools/codefile_bench.py [--repeats 40] [--warmup 5] [--files 1024] [--out profiles/codefile_bench.txt]
"""
import argparse
import logging
import os
import re
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import yaml  # noqa: E402

import inference  # noqa: E402
from bench import bench_inputs  # noqa: E402
from simwhisper_codec_amd import bitstream, synth  # noqa: E402
from simwhisper_codec_amd.codec import AudioCodec  # noqa: E402
from simwhisper_codec_amd.wavio import save_audio  # noqa: E402

B, SECONDS = 32, 10
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def timed(fn):
    """-> (host ms between two synchronisations, ms between two device events) around fn()"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def spread(v):
    s = sorted(v)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return f"median {statistics.median(s):8.3f}  min {s[0]:8.3f}  p10 {q(0.1):8.3f}  p90 {q(0.9):8.3f}  max {s[-1]:8.3f}"


def compare(title, fa, fb, repeats, warmup):
    """fa (per utterance) and fb (batched) alternate; -> medians (host clock)"""
    for _ in range(warmup):
        fa(), fb()
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(timed(fa))
        tb.append(timed(fb))
    say(f"{title}   [ms per batch of {B} x {SECONDS} s, {repeats} alternating rounds after {warmup} warm-up rounds]")
    for name, t in (("(a) per utterance", ta), ("(b) batched      ", tb)):
        say(f"  {name}  host clock    {spread([x[0] for x in t])}")
        say(f"  {name}  device events {spread([x[1] for x in t])}")
    ma, mb = statistics.median(x[0] for x in ta), statistics.median(x[0] for x in tb)
    say(f"  median (b) {mb:.3f} ms {'<' if mb < ma else '>='} median (a) {ma:.3f} ms: "
        f"{'the batched path is ' + format(ma / mb, '.1f') + ' x faster' if mb < ma else 'THE BATCHED PATH IS NOT FASTER'}")
    say()
    return ma, mb


def cli_rates(tmp, n_files, wavs):
    src, codes_dir = os.path.join(tmp, "in"), os.path.join(tmp, "codes")
    os.makedirs(src)
    for i in range(n_files):
        save_audio(os.path.join(src, f"utt_{i:05d}.wav"), wavs[i % B].reshape(1, -1), sample_rate=16000)

    class Grab(logging.Handler):
        last = None

        def emit(self, rec):
            m = re.search(r"([0-9.]+) s of audio in ([0-9.]+) s", rec.getMessage())
            if m:
                Grab.last = (float(m.group(1)), float(m.group(2)))
    inference.set_logging = lambda *a, **k: None   # keep the per-batch INFO lines out of the report
    logging.getLogger().handlers = [Grab()]
    logging.getLogger().setLevel(logging.INFO)
    common = ["--config_path", os.path.join(ROOT, "config", "SimWhisperCodec.yaml"), "--synthetic_checkpoint", "--device", "cuda",
              "--batch_size", str(B)]
    say(f"(c) inference.py, files to files: {n_files} x {SECONDS} s PCM16 files, --batch_size {B}, defaults otherwise; "
        "pass 0 warms up (library load, code objects, page cache)")
    for mode, ind, outd in (("roundtrip", src, os.path.join(tmp, "out_rt")), ("encode", src, codes_dir),
                            ("decode", codes_dir, os.path.join(tmp, "out_dec"))):
        for rep in range(3):
            shutil.rmtree(outd, ignore_errors=True)
            inference.main(common + ["--mode", mode, "--input_dir", ind, "--output_dir", outd])
            audio, loop = Grab.last
            say(f"  --mode {mode:9s} pass {rep}: {audio:7.0f} s of audio, file loop {loop:6.2f} s = {audio / loop:8.1f} audio-s/s incl. file IO")
        assert len(os.listdir(outd)) == n_files
    size = sum(os.path.getsize(os.path.join(codes_dir, f)) for f in os.listdir(codes_dir))
    say(f"  the {n_files} code files hold {size} bytes ({size // n_files} per {SECONDS} s utterance, "
        f"{8 * size / (n_files * SECONDS):.0f} bit/s incl. headers)")
    same = all(open(os.path.join(tmp, "out_rt", f), "rb").read() == open(os.path.join(tmp, "out_dec", f), "rb").read()
               for f in os.listdir(os.path.join(tmp, "out_rt")))
    say(f"  WAV files of encode + decode byte-identical to the round trip's: {same}")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--files", type=int, default=1024, help="files of the CLI runs of (c); 0 skips (c)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "codefile_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("codefile_bench: needs the GPU (nothing here can be measured without one)")
    dev = torch.device("cuda")
    gp = yaml.safe_load(open(os.path.join(ROOT, "config", "SimWhisperCodec.yaml")))["generator_params"]
    m = AudioCodec(gp, precision="mixed")
    m.load_state_dict(synth.synth_state_dict(gp), strict=True)
    m = m.to(dev).eval()
    wavs = bench_inputs(B, SECONDS * 16000)
    codes = m.encode([w.to(dev) for w in wavs])["codes_list"]
    torch.cuda.synchronize()
    say(f"code files of {B} x {SECONDS} s ({[c.shape[-1] for c in codes][0]} frames = {bitstream.image_bytes(codes[0].shape[-1])} bytes each), "
        f"{torch.cuda.get_device_name(0)}, real config, synthetic weights")
    say()
    tmp = tempfile.mkdtemp(prefix="swc_codes_", dir=os.environ.get("SWC_CLI_TMP", "/tmp"))
    try:
        pa = [os.path.join(tmp, f"a_{i:02d}.swc") for i in range(B)]
        pb = [os.path.join(tmp, f"b_{i:02d}.swc") for i in range(B)]

        def write_a():
            for p, c in zip(pa, codes):
                bitstream.write_codes(p, c)

        def write_b():
            bitstream.write_codes_batch(pb, codes)

        compare("codes on the device -> files", write_a, write_b, args.repeats, args.warmup)
        assert all(open(a, "rb").read() == open(b, "rb").read() for a, b in zip(pa, pb)), "the two paths wrote different files"

        def read_a():
            return [bitstream.read_codes(p, dev) for p in pa]

        def read_b():
            return bitstream.read_codes_batch(pb, dev)

        compare("files -> codes on the device", read_a, read_b, args.repeats, args.warmup)
        assert all(torch.equal(a, b) and torch.equal(a, c.to(torch.int32)) for a, b, c in zip(read_a(), read_b(), codes))
        say("both paths wrote the same files and read the same codes back")
        say()
        del m
        if args.files:
            cli_rates(tmp, args.files, wavs)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
