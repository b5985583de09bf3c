"""swc_pitch (F0 tracks of both sides and the five pair measures in one call) at the codec's metric shape, 32 pairs x 10 s at
16 kHz with the audio resident on the device, beside two yardsticks taken in the same run:

  (a) the numpy restatement of the header (tests/pitch_ref.py) on the host for ONE pair, scaled by the number of pairs;
  (b) swc_spectral's default call (metrics.spectral) on the same batch: "one more metric pass".

    python tools/bench_pitch.py [--pairs 32] [--seconds 10] [--sample_rate 16000] [--repeats 40] [--warmup 5] [--out FILE]

One process, warm; the two GPU calls are interleaved (pitch, spectral, pitch, ...) so that they see the same clocks, each
timed by events on the stream: median (min - p90) over --repeats rounds after --warmup rounds.  The raw lines go to --out
(default profiles/pitch_bench.txt).  The multiply-add count printed is arithmetic (frames x W x (tau_max + 1)), not a counter.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sample_rate", type=int, default=16000)
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import pitch_ref
    from simwhisper_codec_amd import metrics, ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_pitch: no GPU (the call is a HIP kernel; there is nothing to time without one)")
    dev = torch.device("cuda", torch.cuda.current_device())
    p = ops.pitch_params(a.sample_rate)
    n = int(a.seconds * a.sample_rate)
    pairs = []
    for i in range(a.pairs):
        x = pitch_ref.test_signal(i % 8, sr=a.sample_rate)
        y = pitch_ref.test_signal(i % 8, sr=a.sample_rate, shift=1.3, noise=0.002)
        reps = -(-n // len(x))
        pairs.append((np.tile(x, reps)[:n], np.tile(y, reps)[:n]))
    ref = [torch.from_numpy(x).to(dev) for x, _ in pairs]
    deg = [torch.from_numpy(y).to(dev) for _, y in pairs]
    calls = {
        "swc_pitch": lambda: ops.pitch(ref, deg, p, want=("f0_x", "f0_y", "values", "counts")),
        "metrics.spectral": lambda: metrics.spectral(ref, deg, sample_rate=a.sample_rate, device=dev),
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
    r = calls["swc_pitch"]()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = pitch_ref.pitch(*pairs[0], **p)
    host_s = time.perf_counter() - t0
    same = bool(np.array_equal(host["f0_x"].view(np.uint32), r["f0_x"][0].cpu().numpy().view(np.uint32)) and
                np.array_equal(host["f0_y"].view(np.uint32), r["f0_y"][0].cpu().numpy().view(np.uint32)))
    frames = 2 * sum(r["frames"])
    macs = frames * p["W"] * (p["tau_max"] + 1)
    audio = a.pairs * a.seconds
    lines = [f"{a.pairs} pairs x {a.seconds:g} s at {a.sample_rate} Hz ({p}), {a.repeats} interleaved rounds after {a.warmup}; "
             f"device {torch.cuda.get_device_name(dev)}",
             f"arithmetic: {frames} frames x W x (tau_max + 1) = {macs:.3e} multiply-adds per call"]
    med = {}
    for k, v in ms.items():
        lines.append(f"{k} raw ms: " + " ".join(f"{t:.3f}" for t in v))
        s = sorted(v)
        med[k] = statistics.median(s)
        lines.append(f"{k}: median {med[k]:.3f} ms (min {s[0]:.3f} - p90 {s[int(0.9 * len(s))]:.3f}), {audio / (med[k] * 1e-3):,.0f} audio-s/s")
    lines.append(f"swc_pitch: {macs / (med['swc_pitch'] * 1e-3) / 1e12:.2f} T multiply-adds/s over the whole call (arithmetic count over measured time)")
    lines.append(f"swc_pitch / metrics.spectral = {med['swc_pitch'] / med['metrics.spectral']:.2f}")
    lines.append(f"host numpy (tests/pitch_ref.py), one pair: {host_s:.2f} s; x {a.pairs} pairs = {host_s * a.pairs:.1f} s "
                 f"= {host_s * a.pairs * 1e3 / med['swc_pitch']:,.0f} x the call; its f0 tracks {'equal' if same else 'DIFFER FROM'} the call's bit for bit")
    v = r["values"].cpu()
    lines.append("mean over the pairs: " + " ".join(f"{k} {float(v[:, i].nanmean()):.4f}" for i, k in enumerate(metrics.PITCH_KEYS)))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
