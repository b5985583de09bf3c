"""metrics.stoi, metrics.quality (STOI + ESTOI + SI-SDR) and metrics.si_sdr alone at the codec's metric shape: 32 pairs x 10 s
at 16 kHz, audio resident on the device.

    python tools/bench_quality.py [--pairs 32] [--seconds 10] [--sample_rate 16000] [--repeats 200] [--warmup 20]

One process, warm; the three calls are interleaved (stoi, quality, si_sdr, stoi, ...) so that they see the same clocks, each
timed by events on the stream.  Median, min and p90 over --repeats per call, and quality's median over stoi's: the fused call
shares the front end, so it has to cost less than two separate calls (ratio below 2).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sample_rate", type=int, default=16000)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
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
    calls = {
        "metrics.stoi": lambda: metrics.stoi(ref, deg, sample_rate=a.sample_rate, device=dev),
        "metrics.quality": lambda: metrics.quality(ref, deg, sample_rate=a.sample_rate, device=dev),
        "metrics.si_sdr": lambda: metrics.si_sdr(ref, deg, sample_rate=a.sample_rate, device=dev),
    }
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
    audio = a.pairs * a.seconds
    print(f"{a.pairs} x {a.seconds:g} s at {a.sample_rate} Hz, {a.repeats} interleaved calls each after {a.warmup}")
    med = {}
    for k, v in ms.items():
        v.sort()
        med[k] = statistics.median(v)
        print(f"{k}: median {med[k]:.3f} ms (min {v[0]:.3f}, p90 {v[int(0.9 * len(v))]:.3f}), {audio / (med[k] * 1e-3):,.0f} audio-s/s")
    q = calls["metrics.quality"]()
    print(f"metrics.quality / metrics.stoi = {med['metrics.quality'] / med['metrics.stoi']:.3f} (bar: below 2); mean stoi "
          f"{float(q['stoi'].mean()):.4f}, estoi {float(q['estoi'].mean()):.4f}, si_sdr {float(q['si_sdr'].mean()):.2f} dB, "
          f"segs {int(q['segs'][0])}")


if __name__ == "__main__":
    main()
