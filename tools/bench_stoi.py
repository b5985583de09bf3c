"""metrics.stoi at the codec's metric shape: 32 pairs x 10 s at 16 kHz, audio resident on the device.

    python tools/bench_stoi.py [--pairs 32] [--seconds 10] [--sample_rate 16000] [--repeats 200] [--warmup 20] [--host]

Device time per call from events on the stream (warm, median and spread over --repeats), audio-seconds per second, and with
--host the float64 restatement of tests/stoi_ref.py on 16 host processes for scale (OUR restatement, not pystoi).
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _host_one(args):
    import stoi_ref
    x, y, fs = args
    return stoi_ref.stoi(x, y, fs)["d"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sample_rate", type=int, default=16000)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    import torch
    import stoi_ref
    from simwhisper_codec_amd import metrics
    dev = torch.device("cuda", torch.cuda.current_device())
    n = int(a.seconds * a.sample_rate)
    pairs = []
    for i in range(a.pairs):
        x = stoi_ref.harmonic(n, a.sample_rate, seed=i % 8)
        pairs.append((x, stoi_ref.add_noise(x, 5, seed=i)))
    ref = [torch.from_numpy(x).to(dev) for x, _ in pairs]
    deg = [torch.from_numpy(y).to(dev) for _, y in pairs]
    for _ in range(a.warmup):
        d, segs = metrics.stoi(ref, deg, sample_rate=a.sample_rate, device=dev)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d, segs = metrics.stoi(ref, deg, sample_rate=a.sample_rate, device=dev)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    med = statistics.median(ms)
    audio = a.pairs * a.seconds
    print(f"metrics.stoi {a.pairs} x {a.seconds:g} s at {a.sample_rate} Hz: median {med:.3f} ms (min {ms[0]:.3f}, p90 {ms[int(0.9 * len(ms))]:.3f}, "
          f"{a.repeats} calls after {a.warmup}), {audio / (med * 1e-3):,.0f} audio-s/s; mean d {float(d.mean()):.4f}, segs {int(segs[0])}")
    if a.host:
        from multiprocessing import Pool
        t = time.perf_counter()
        with Pool(16) as pool:
            dh = pool.map(_host_one, [(x, y, a.sample_rate) for x, y in pairs])
        dt = time.perf_counter() - t
        worst = max(abs(float(v) - w) for v, w in zip(d.cpu(), dh))
        print(f"float64 restatement (tests/stoi_ref.py, not pystoi) on 16 host processes: {dt * 1e3:.0f} ms, {audio / dt:,.0f} audio-s/s; "
              f"worst |d_gpu - d_f64| over the batch {worst:.2e}")


if __name__ == "__main__":
    main()
