"""metrics.segmental (swc_segmental: LLR, Itakura-Saito, LPC cepstral distance, segmental and frequency-weighted segmental SNR)
at the codec's metric shape, 32 pairs x 10 s at 16 kHz with the audio resident on the device, beside two yardsticks:
metrics.spectral (swc_spectral, the same framed-FFT shape over seven windows) on the same batch, and the float64 host reference
(tests/segmental_ref.py) for one pair on one thread; and the largest deviation of each of the five measures from that reference
over the cases of tests/test_segmental_gpu.py (value_cases(): row values and track entries), the numbers its TOLs are ten times:

    python tools/bench_segmental.py [--rows 32] [--seconds 10] [--repeats 40] [--warmup 5] [--out FILE]

One process, warm; the two device calls are interleaved (segmental, spectral, segmental, ...) so that they see the same clocks.
Every round is timed twice: by the host clock around call + synchronize, and by events on the stream; median (min - p90) over
--repeats rounds after --warmup rounds.  The raw lines go to --out (default profiles/segmental_bench.txt).
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS = 16000


def commit():
    try:
        with open(os.path.join(ROOT, "simwhisper_codec_amd", "_build_commit.txt")) as f:
            return f.read().strip()
    except OSError:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        return r.stdout.strip() or "unknown"


def deviations():
    """the largest |device - reference| of each measure over the value cases of tests/test_segmental_gpu.py -> (dict, pairs)"""
    import test_segmental_gpu as cases
    worst, count = dict.fromkeys(cases.MEASURES, 0.0), 0
    for name, fs, W, P, table, xs, ys in cases.value_cases():
        got = cases.run(cases.on_device(xs), cases.on_device(ys), W, P, table)
        for b, (x, y) in enumerate(zip(xs, ys)):
            dev = cases.deviations(got, b, cases.reference((name, b), x, y, W, P, table))
            for k in cases.MEASURES:
                worst[k] = max(worst[k], dev[k])
            count += 1
    return worst, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segmental_bench.txt"))
    a = ap.parse_args()
    import torch
    import segmental_ref
    import test_segmental_gpu as cases
    from simwhisper_codec_amd import metrics
    if not torch.cuda.is_available():
        raise SystemExit("bench_segmental: no GPU (the calls are HIP kernels; there is nothing to time without one)")
    dev = torch.device("cuda", torch.cuda.current_device())
    n = int(a.seconds * FS)
    xs = [cases.signal(n, FS, 200 + i) for i in range(a.rows)]
    ys = cases.degraded(xs)
    W, P = metrics.segmental_params(FS)
    t0 = time.perf_counter()
    want = segmental_ref.measure(xs[0], ys[0], W, P, cases.bands(FS, W))
    host = time.perf_counter() - t0
    lines = [f"commit {commit()}; {a.rows} pairs x {a.seconds:g} s at {FS} Hz (W {W}, P {P}, {metrics.SEGMENTAL_BANDS} bands), {a.repeats} "
             f"interleaved rounds after {a.warmup}; device {torch.cuda.get_device_name(dev)}"]
    dx, dy = cases.on_device(xs), cases.on_device(ys)
    calls = {"metrics.segmental": lambda: metrics.segmental(dx, dy, sample_rate=FS, device=dev),
             "metrics.segmental without fwsegsnr": lambda: metrics.segmental(dx, dy, sample_rate=FS, device=dev, want=("llr", "is", "cd", "segsnr")),
             "metrics.spectral": lambda: metrics.spectral(dx, dy, sample_rate=FS, device=dev)}
    for _ in range(a.warmup):
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    ev, wall = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(a.repeats):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            ev[k].append(e0.elapsed_time(e1))
    audio = a.rows * a.seconds
    for k in calls:
        for name, v in (("device events", ev[k]), ("host clock", wall[k])):
            s = sorted(v)
            med = statistics.median(s)
            lines.append(f"{k}, {name}, raw ms: " + " ".join(f"{t:.3f}" for t in v))
            lines.append(f"{k}, {name}: median {med:.3f} ms (min {s[0]:.3f} - p90 {s[int(0.9 * len(s))]:.3f}), "
                         f"{audio / (med * 1e-3):,.0f} audio-s/s")
    q = metrics.segmental(dx, dy, sample_rate=FS, device=dev)
    lines.append("mean over the pairs: " + " ".join(f"{k} {float(q[k].nanmean()):.4f}" for k in metrics.SEGMENTAL_KEYS))
    lines.append("pair 0, device - reference: " + " ".join(f"{k} {float(q[k][0]) - want[k]:+.3e}" for k in metrics.SEGMENTAL_KEYS))
    lines.append(f"host float64 reference (tests/segmental_ref.py), one pair of {a.seconds:g} s on one thread: {host * 1e3:.0f} ms")
    worst, count = deviations()
    lines.append(f"largest deviation from the float64 reference over the {count} pairs of tests/test_segmental_gpu.py value_cases() "
                 "(row values and track entries): " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()) + " (llr, is: absolute; cd, segsnr, fwsegsnr: dB)")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
