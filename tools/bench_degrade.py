"""ops.convolve and degrade.add_noise (include/swc_degrade.h) at the codec's shapes, 32 rows x 10 s and 32 x 30 s at 16 kHz
resident on the device, beside the obvious other path for the same result:

  reverb    ops.convolve (three launches)        against  torch.fft overlap-add on the device: one rfft of the response, then
                                                          per row rfft -> product -> irfft over blocks of 2^16 points
  noise     degrade.add_noise (long-term level)  against  the host path: tests/stoi_ref.add_noise per row in numpy, then the
                                                          upload of the batch

    python tools/bench_degrade.py [--rows 32] [--seconds 10 30] [--rir 0.3 1.0] [--repeats 10] [--warmup 2] [--out FILE]

One process, warm.  Every path ends with its result on the device, is timed with a wall clock around a synchronised region,
and the two paths of a measure alternate round by round so that they see the same clocks: median (min - p90) over --repeats
rounds after --warmup rounds.  The results of the two paths are compared before anything is timed: the two convolutions against
each other (both are f32 FFT methods), the two noisy batches by the signal-to-noise ratio they reach (their noise differs: the
host path draws Gaussian samples from numpy, the device path is the Irwin-Hall stream of the header).  The raw lines go to
--out (default profiles/degrade_bench.txt)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seconds", type=float, nargs="+", default=[10.0, 30.0])
    ap.add_argument("--rir", type=float, nargs="+", default=[0.3, 1.0])
    ap.add_argument("--snr", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "degrade_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import stoi_ref
    from simwhisper_codec_amd import degrade, ops, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_degrade: no GPU (the calls are HIP kernels; there is nothing to time without one)")
    dev = torch.device("cuda", torch.cuda.current_device())
    B = a.rows
    lines = [f"device {torch.cuda.get_device_name(dev)}; {a.repeats} alternating rounds after {a.warmup}; wall clock, results on the device"]

    def timed(calls, title):
        for _ in range(a.warmup):
            for f in calls.values():
                f()
        ms = {k: [] for k in calls}
        for _ in range(a.repeats):
            for k, f in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ms[k].append(1e3 * (time.perf_counter() - t0))
        lines.append(title)
        for k, v in ms.items():
            lines.append(f"{k} raw ms: " + " ".join(f"{t:.3f}" for t in v))
            s = sorted(v)
            lines.append(f"{k}: median {statistics.median(s):.3f} ms (min {s[0]:.3f} - p90 {s[int(0.9 * len(s))]:.3f})")

    for seconds in a.seconds:
        n = int(seconds * FS)
        host = [(0.1 * synth.synth_audio(n - 17 * i, index=200 + i, kind="speech")).numpy().astype(np.float32) for i in range(B)]
        rows = [torch.from_numpy(x).to(dev) for x in host]
        lens = [len(x) for x in host]
        for rt60 in a.rir:
            h, d = degrade.synthetic_rir(rt60, FS, seed=1, device=dev)
            L = h.numel()
            block = 1 << 16
            step = block - (L - 1)
            Hf = torch.fft.rfft(h, block)

            def conv_gpu():
                return ops.convolve(rows, [h], d=d, extra=0)

            def conv_torch():
                out = torch.zeros(B, max(lens) + L - 1, device=dev)
                for b, x in enumerate(rows):
                    for s in range(0, lens[b], step):
                        seg = x[s:s + step]
                        y = torch.fft.irfft(torch.fft.rfft(seg, block) * Hf, block)[:seg.numel() + L - 1]
                        out[b, s:s + y.numel()] += y
                return out[:, d:d + max(lens)]

            got, want = conv_gpu(), conv_torch()
            for b in range(B):
                want[b, lens[b]:] = 0
            scale = float(h.abs().sum()) * max(float(x.abs().max()) for x in rows)
            err = float((got - want).abs().max()) / scale
            assert err < 1e-5, err
            timed({"reverb: ops.convolve": conv_gpu, "reverb: torch.fft overlap-add": conv_torch},
                  f"--- {B} rows x {seconds:g} s, response of {rt60:g} s = {L} taps; the two differ by {err:.2e} of ||h||_1 max|x|")

        def noise_gpu():
            return degrade.add_noise(rows, a.snr, seed=3, level="long_term", sample_rate=FS)[0]

        def noise_host():
            out = np.zeros((B, max(lens)), dtype=np.float32)
            for b, x in enumerate(host):
                out[b, :len(x)] = stoi_ref.add_noise(x, a.snr, seed=b)
            return torch.from_numpy(out).to(dev)

        def snr_of(noisy, b):
            y = noisy[b][:lens[b]].double().cpu().numpy() if torch.is_tensor(noisy[b]) else noisy[b]
            x = host[b].astype(np.float64)
            return 10 * np.log10(np.sum(x ** 2) / np.sum((y - x) ** 2))

        g, hh = noise_gpu(), noise_host()
        worst = max(max(abs(snr_of(g, b) - a.snr), abs(snr_of(hh, b) - a.snr)) for b in range(B))
        assert worst < 1e-2, worst
        timed({"noise: degrade.add_noise": noise_gpu, "noise: numpy per row + upload": noise_host},
              f"--- {B} rows x {seconds:g} s, noise at {a.snr:g} dB against the long-term level; both within {worst:.1e} dB of the target")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
