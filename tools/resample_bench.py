#!/usr/bin/env python3
"""Sample-rate conversion on the GPU against what it replaces (DESIGN.md "Sample-rate conversion").

usage: python tools/resample_bench.py [kernel] [cli [n_files=128] [seconds=10]]
kernel: 32 x 10 s at 24 / 44.1 / 48 kHz, int16 mono and stereo -> 16 kHz.
    (a) ops.resample on the device: event-timed, 5 warm-up + 30 timed launches, median / min / max, and the fraction of
        HBM's 8 TB/s the launch's bytes (int16 in + f32 out) reach;
    (b) the host path: wavio.resample over the same 32 rows (channel mean first) on 16 threads + the upload of the f32
        result, wall clock, median of 3.
cli: inference.py file to file on 24 kHz mono PCM16 files, --resample host against --resample gpu, interleaved
    (host, gpu, host, gpu), after one warm-up pass each.
"""
import logging
import os
import re
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from simwhisper_codec_amd import ops, wavio  # noqa: E402

DEV = torch.device("cuda", 0)
HBM = 8.0e12


def kernel_bench(B=32, seconds=10.0):
    g = torch.Generator().manual_seed(1234)
    for sr in (24000, 44100, 48000):
        for ch in (1, 2):
            n = int(seconds * sr)
            pcm = [torch.randint(-20000, 20000, (n, ch), generator=g, dtype=torch.int32).to(torch.int16) for _ in range(B)]
            rows = [p.to(DEV) for p in pcm]
            with torch.cuda.device(DEV):
                for _ in range(5):
                    out, n_out = ops.resample(rows, sr, 16000, channels=ch)
                torch.cuda.synchronize()
                ts = []
                for _ in range(30):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out, n_out = ops.resample(rows, sr, 16000, channels=ch)
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e3)
            nbytes = B * n * ch * 2 + out.numel() * 4
            med = statistics.median(ts)
            print(f"gpu   sr={sr} ch={ch} B={B} x {seconds:g} s: ops.resample median {med:8.1f} us (min {min(ts):.1f}, max {max(ts):.1f}, "
                  f"30 launches, events around the front end: table lookup + address upload + kernel), {nbytes / 1e6:.1f} MB -> "
                  f"{nbytes / med / 1e6:.3f} TB/s = {100 * nbytes / (med * 1e-6) / HBM:.1f} % of 8 TB/s", flush=True)
            # the kernel alone: the same launch through the C-ABI with the address list already on the device
            from simwhisper_codec_amd import _lib
            lib, t = _lib.load(), ops.resample_table(sr, 16000, DEV)
            meta = torch.tensor([r.data_ptr() for r in rows] + [n] * B, dtype=torch.int64).to(DEV)
            with torch.cuda.device(DEV):
                def launch():
                    _lib.check(lib.swc_resample(ops._ptr(meta[:B]), ops._ptr(meta[B:]), _lib.PCM_I16, ch, t["orig"], t["new"], t["width"],
                                                ops._ptr(t["taps"]), ops._ptr(t["start"]), t["run"], ops._ptr(out), out.stride(0),
                                                out.shape[1], B, ops._stream()), "swc_resample")
                for _ in range(5):
                    launch()
                torch.cuda.synchronize()
                ks = []
                for _ in range(30):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    launch()
                    e1.record()
                    e1.synchronize()
                    ks.append(e0.elapsed_time(e1) * 1e3)
            kmed = statistics.median(ks)
            print(f"gpu   sr={sr} ch={ch} B={B} x {seconds:g} s: swc_resample alone median {kmed:8.1f} us (min {min(ks):.1f}, max {max(ks):.1f}, "
                  f"30 launches) -> {nbytes / kmed / 1e6:.3f} TB/s = {100 * nbytes / (kmed * 1e-6) / HBM:.1f} % of 8 TB/s", flush=True)
            # (b) what it replaces
            torch.set_num_threads(1)
            pool = ThreadPoolExecutor(16)

            def host_one(p):
                x = p.to(torch.float32) / 32768.0
                x = x.mean(dim=1) if x.shape[1] > 1 else x[:, 0]
                return wavio.resample(x.contiguous(), sr, 16000)
            hs = []
            for _ in range(3):
                t0 = time.perf_counter()
                ys = list(pool.map(host_one, pcm))
                t1 = time.perf_counter()
                up = [y.to(DEV) for y in ys]
                torch.cuda.synchronize()
                hs.append((time.perf_counter() - t0, t1 - t0))
            pool.shutdown()
            hs.sort()
            print(f"host  sr={sr} ch={ch} B={B} x {seconds:g} s: wavio.resample on 16 threads + f32 upload median {hs[1][0] * 1e3:8.1f} ms "
                  f"(of which conversion {hs[1][1] * 1e3:.1f} ms; min {hs[0][0] * 1e3:.1f}, max {hs[2][0] * 1e3:.1f}, 3 runs)", flush=True)
            del up, ys


def cli_bench(n_files=128, seconds=10.0, sr=24000, bs=32):
    import inference
    from simwhisper_codec_amd import synth
    tmp = tempfile.mkdtemp(prefix="swc_rs_", dir=os.environ.get("SWC_CLI_TMP", "/tmp"))
    try:
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        base = [synth.synth_audio(int(seconds * sr), index=i, kind="speech") for i in range(8)]
        for i in range(n_files):
            wavio.save_audio(os.path.join(src, f"utt_{i:05d}.wav"), base[i % 8].reshape(1, -1), sample_rate=sr)

        class Grab(logging.Handler):
            last, stages = None, None

            def emit(self, rec):
                m = re.search(r"([0-9.]+) s of audio in ([0-9.]+) s", rec.getMessage())
                if m:
                    Grab.last = (float(m.group(1)), float(m.group(2)))
                if "stage wall seconds" in rec.getMessage():
                    Grab.stages = rec.getMessage()
        inference.set_logging = lambda *a, **k: None
        logging.getLogger().handlers = [Grab()]
        logging.getLogger().setLevel(logging.INFO)
        for rep, mode in enumerate(["host", "gpu", "host", "gpu", "host", "gpu"]):
            dst = os.path.join(tmp, f"out_{mode}")
            shutil.rmtree(dst, ignore_errors=True)
            inference.main(["--config_path", os.path.join(ROOT, "config", "SimWhisperCodec.yaml"), "--synthetic_checkpoint",
                            "--device", "cuda", "--batch_size", str(bs), "--input_dir", src, "--output_dir", dst, "--resample", mode])
            audio, loop = Grab.last
            print(f"cli   --resample {mode:4s} {'warm-up' if rep < 2 else 'timed  '}: {n_files} x {seconds:g} s files at {sr} Hz, file loop "
                  f"{loop:.2f} s = {audio / loop:8.1f} audio-s/s incl. file IO; {Grab.stages}", flush=True)
        a, b = os.path.join(tmp, "out_host"), os.path.join(tmp, "out_gpu")
        diff = [f for f in sorted(os.listdir(a)) if open(os.path.join(a, f), "rb").read() != open(os.path.join(b, f), "rb").read()]
        worst = 0
        for f in diff[:16]:
            x, y = wavio.read_pcm(os.path.join(a, f))[0], wavio.read_pcm(os.path.join(b, f))[0]
            worst = max(worst, int((x.int() - y.int()).abs().max()))
        print(f"cli   outputs: {len(diff)} of {n_files} files differ between the two paths (largest PCM16 difference in the first "
              f"16 of them: {worst})", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    args = sys.argv[1:] or ["kernel"]
    if "kernel" in args:
        kernel_bench()
    if "cli" in args:
        rest = args[args.index("cli") + 1:]
        cli_bench(int(rest[0]) if rest else 128, float(rest[1]) if len(rest) > 1 else 10.0)
