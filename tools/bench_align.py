"""swc_align (the lag, overlap, correlation and level ratio of every pair in one call) at the codec's metric shape, 32 pairs x
10 s at 16 kHz with the audio resident on the device, at L = 800 (+-50 ms) and L = 16000 (+-1 s), in both modes, beside a
yardstick taken in the same run on the same GPU: the same lags through torch.fft (rfft of both rows zero-padded to a power of
two, the product with the conjugate, irfft, the 2 L + 1 lags cut out, argmax), in float32 and therefore NOT exact.

    python tools/bench_align.py [--pairs 32] [--seconds 10] [--sample_rate 16000] [--repeats 20] [--warmup 3] [--out FILE]

One process, warm; all calls are interleaved round by round so that they see the same clocks, each timed by events on the
stream: median (min - p90) over --repeats rounds after --warmup rounds.  The raw lines go to --out (default
profiles/align_bench.txt).  The multiply-add count printed is arithmetic (the products inside both rows, summed over the lags),
not a counter; the rate divides it by the time of the WHOLE call (peaks, staging, choice and energies included).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RANGES = (800, 16000)
MODES = ("waveform", "envelope")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sample_rate", type=int, default=16000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import align_ref
    import pitch_ref
    from simwhisper_codec_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_align: no GPU (the call is a HIP kernel; there is nothing to time without one)")
    dev = torch.device("cuda", torch.cuda.current_device())
    n = int(a.seconds * a.sample_rate)
    delays = [((37 * i) % 601) - 300 for i in range(a.pairs)]
    pairs = []
    for i in range(a.pairs):
        x = pitch_ref.test_signal(i % 8, sr=a.sample_rate)
        x = np.tile(x, -(-n // len(x)))[:n] * (0.2 + np.abs(np.sin(np.arange(n) / 9000.0 + i))).astype(np.float32)   # no two periods alike
        y = (0.5 * align_ref.delayed(x, delays[i]) + 0.002 * np.random.default_rng(i).standard_normal(n)).astype(np.float32)
        pairs.append((x.astype(np.float32), y))
    ref = [torch.from_numpy(x).to(dev) for x, _ in pairs]
    deg = [torch.from_numpy(y).to(dev) for _, y in pairs]
    X, Y = torch.stack(ref), torch.stack(deg)

    def fft_lags(L):
        N = 1 << (n + L - 1).bit_length()
        c = torch.fft.irfft(torch.fft.rfft(Y, N) * torch.fft.rfft(X, N).conj(), N)       # c[d] = sum x[i] y[i + d], d mod N
        c = torch.cat([c[:, N - L:], c[:, :L + 1]], dim=1)
        return c.argmax(dim=1) - L

    calls = {}
    for L in RANGES:
        for mode in MODES:
            calls[f"swc_align L={L} {mode}"] = (lambda L=L, mode=mode: ops.align(ref, deg, L, mode, want=("info", "values")))
        calls[f"torch.fft L={L}"] = (lambda L=L: fft_lags(L))
    for _ in range(a.warmup):
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(a.repeats):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    lines = [f"{a.pairs} pairs x {a.seconds:g} s at {a.sample_rate} Hz, true delays {min(delays)} .. {max(delays)} samples, {a.repeats} interleaved "
             f"rounds after {a.warmup}; device {torch.cuda.get_device_name(dev)}"]
    med = {}
    for k, v in ms.items():
        lines.append(f"{k} raw ms: " + " ".join(f"{t:.3f}" for t in v))
        s = sorted(v)
        med[k] = statistics.median(s)
        lines.append(f"{k}: median {med[k]:.3f} ms (min {s[0]:.3f} - p90 {s[int(0.9 * len(s))]:.3f})")
    for L in RANGES:
        macs = a.pairs * sum(max(0, n - abs(d)) for d in range(-L, L + 1))
        lines.append(f"L={L}: {macs:.3e} multiply-adds per call (arithmetic)")
        for mode in MODES:
            k = f"swc_align L={L} {mode}"
            r = calls[k]()
            found = r["info"][:, 0].cpu().tolist()
            right = sum(int(f == d) for f, d in zip(found, delays) if abs(d) <= L)
            lines.append(f"{k}: {macs / (med[k] * 1e-3) / 1e12:.2f} T multiply-adds/s over the whole call; "
                         f"{med[k] / med[f'torch.fft L={L}']:.2f} x the torch.fft yardstick's time; "
                         f"{right} of {a.pairs} true delays found, mean corr {float(r['values'][:, 0].nanmean()):.4f}")
        fl = calls[f"torch.fft L={L}"]().cpu().tolist()
        lines.append(f"torch.fft L={L}: {sum(int(f == d) for f, d in zip(fl, delays))} of {a.pairs} true delays found (float32, not exact)")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
